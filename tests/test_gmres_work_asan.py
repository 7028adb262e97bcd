"""The work buffer of spmv_*_gmres (solver_work.h, gmres_work) and the
per-column dense arithmetic (gmres_small.h) as a stand-alone host program under
AddressSanitizer + UBSan: the state with its column blocks, restart + 1 sets of
partial sums, the basis as one vector, W and Z at k = 1..8, restart 1 / 30 / 64
and sizes around the tile, aligned, in order, disjoint and inside a heap block
of exactly solver_work_bytes; the total at 2^31 - 1 rows; the refusals;
gm_step / gm_back on Hessenberg columns against rotations written out in the
program in long double."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_gmres_work_layout_and_small_arithmetic_under_asan(tmp_path):
    exe = str(tmp_path / "gmres_work_asan")
    subprocess.run(
        ["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off",
         "-fsanitize=address,undefined",
         "-fno-omit-frame-pointer", "-fno-sanitize-recover=all",
         "-I", os.path.join(ROOT, "spmv_scpa_amd", "csrc"),
         os.path.join(ROOT, "tests", "asan", "gmres_work_asan.cc"),
         "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "144 layouts hold" in r.stdout   # 8 values of k x 3 restarts x 6 sizes
    assert "70 Hessenberg columns match" in r.stdout   # m = 1, 5, 64
    assert "FAILED" not in r.stdout and "ERROR" not in r.stderr
