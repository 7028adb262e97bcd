"""The work buffer of spmv_*_bicgstab_trsv (solver_work.h, bicgstab_trsv_work)
as a stand-alone host program under AddressSanitizer + UBSan: the state block,
two sets of partial sums and seven vectors at k = 1..8 and sizes around the
tile, aligned, in order, disjoint and inside a heap block of exactly
solver_work_bytes; bicgstab_work beside it unchanged; the total at 2^31 - 1
rows; the refusals."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_bicgstab_trsv_work_layout_under_asan(tmp_path):
    exe = str(tmp_path / "bicgstab_trsv_work_asan")
    subprocess.run(
        ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined",
         "-fno-omit-frame-pointer", "-fno-sanitize-recover=all",
         "-I", os.path.join(ROOT, "spmv_scpa_amd", "csrc"),
         os.path.join(ROOT, "tests", "asan", "bicgstab_trsv_work_asan.cc"),
         "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "48 layouts hold" in r.stdout   # 8 values of k x 6 sizes
    assert "FAILED" not in r.stdout and "ERROR" not in r.stderr
