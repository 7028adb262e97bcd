"""The host arithmetic of smoothed-aggregation AMG (the key of a row in the
rounds, the scratch layout of a hierarchy, the grids, the launch count of an
apply and the refusals: spmv_scpa_amd/csrc/amg_plan.h, which the launcher and
the kernels both read) compiled for the CPU as a stand-alone program and run
under AddressSanitizer + UBSan over 4000 seeded inputs.  No Python code runs
under a sanitizer."""
import os
import subprocess
import sys

import numpy as np

import _colour as CO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_amg_plan_under_asan(tmp_path):
    exe = str(tmp_path / "amg_plan_asan")
    subprocess.run(
        ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined",
         "-fno-omit-frame-pointer", "-fno-sanitize-recover=all",
         "-I", os.path.join(ROOT, "spmv_scpa_amd", "csrc"),
         os.path.join(ROOT, "tests", "asan", "amg_plan_asan.cc"),
         "-o", exe], check=True)
    r = subprocess.run([exe, "4000"], capture_output=True, text=True)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "every vector in its own part" in r.stdout
    assert "FAILED" not in r.stdout + r.stderr and "ERROR" not in r.stderr


def test_the_keys_of_the_header_order_the_rows_as_the_restatement_does():
    """hash << 31 | row orders the rows as (fmix32(row ^ seed), row), the
    order tests/_amg.py ranks them by"""
    for seed in (0, 1, 0xdeadbeef):
        M = 3000
        h = CO.priority(M, seed).astype(np.uint64)
        key = (h << np.uint64(31)) | np.arange(M, dtype=np.uint64)
        assert np.array_equal(np.argsort(key, kind="stable"),
                              np.lexsort((np.arange(M), h)))
        assert len(set(key.tolist())) == M
