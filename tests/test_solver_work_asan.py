"""The work buffer of the device-resident solvers (solver_work.h: one
description behind every *_work_bytes and every pointer a solve takes) as a
stand-alone host program under AddressSanitizer + UBSan: the six buffers at
k = 1..8 and sizes around the tile, their regions aligned, in order, disjoint
and inside a heap block of exactly the stated size; the closed formulas; the
totals at 2^31 - 1 rows; the refusals."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_solver_work_layout_under_asan(tmp_path):
    exe = str(tmp_path / "solver_work_asan")
    subprocess.run(
        ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined",
         "-fno-omit-frame-pointer", "-fno-sanitize-recover=all",
         "-I", os.path.join(ROOT, "spmv_scpa_amd", "csrc"),
         os.path.join(ROOT, "tests", "asan", "solver_work_asan.cc"),
         "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    # 8 values of k x 36 (M, N) pairs of cgls + 8 x 6 sizes x 5 square solvers
    assert "528 layouts hold" in r.stdout
    assert "FAILED" not in r.stdout and "ERROR" not in r.stderr
