"""The route of a sweep plan (trsv_plan.h: trsv_sweep_route,
trsv_sweep_scratch; spmv_csr_trsv_analyse_sweeps) as a stand-alone host
program under AddressSanitizer + UBSan: for sweeps 1..6 and 4096 no sweep reads
the buffer it writes, every sweep reads what the one before it wrote, X (which
may be B) is written by the last sweep alone, and the scratch count is
min(sweeps - 1, 2); the sweeps restated over heap blocks of exactly the scratch
sizes, in place and not, against forward substitution."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_sweep_route_and_its_scratch_under_asan(tmp_path):
    exe = str(tmp_path / "trsv_sweep_asan")
    subprocess.run(
        ["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off",
         "-fsanitize=address,undefined",
         "-fno-omit-frame-pointer", "-fno-sanitize-recover=all",
         "-I", os.path.join(ROOT, "spmv_scpa_amd", "csrc"),
         os.path.join(ROOT, "tests", "asan", "trsv_sweep_asan.cc"),
         "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "4117 routed sweeps hold" in r.stdout   # 1 + .. + 6 + 4096
    assert "48 restated solves hold" in r.stdout   # k = 1..3, 8 counts, twice
    assert "FAILED" not in r.stdout and "ERROR" not in r.stderr
