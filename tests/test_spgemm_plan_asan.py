"""The host arithmetic of the sparse product (size classes, tables and LDS, the
scratch layout, the fallback's batches and the overflow guards:
spmv_scpa_amd/csrc/spgemm_plan.h, which the launcher, spmv_spgemm_shape and
the tests all read) compiled for the CPU as a stand-alone program and run
under AddressSanitizer + UBSan over 4000 seeded inputs.  No Python code runs
under a sanitizer."""
import os
import subprocess
import sys

import spmv_scpa_amd as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_spgemm_plan_under_asan(tmp_path):
    exe = str(tmp_path / "spgemm_plan_asan")
    subprocess.run(
        ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined",
         "-fno-omit-frame-pointer", "-fno-sanitize-recover=all",
         "-I", os.path.join(ROOT, "spmv_scpa_amd", "csrc"),
         os.path.join(ROOT, "tests", "asan", "spgemm_plan_asan.cc"),
         "-o", exe], check=True)
    r = subprocess.run([exe, "4000"], capture_output=True, text=True)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "every row in one class" in r.stdout
    assert "FAILED" not in r.stdout + r.stderr and "ERROR" not in r.stderr


def test_the_library_reports_the_numbers_of_the_header():
    """spmv_spgemm_shape against the header's text"""
    import re
    hdr = open(os.path.join(ROOT, "spmv_scpa_amd", "csrc",
                            "spgemm_plan.h")).read()

    def macro(name):
        m = re.search(r"#define\s+%s\s+(\w+)" % name, hdr)
        assert m, name
        return macro(m.group(1)) if not m.group(1).isdigit() \
            else int(m.group(1))

    shape = S.spgemm_shape()
    assert shape["tables"] == [macro("SPGEMM_TABLE%d" % c) for c in range(3)]
    assert shape["teams"] == [macro("SPGEMM_TEAM%d" % c) for c in range(3)]
    assert shape["edges"] == [t // 2 for t in shape["tables"]]
    assert shape["fallback_batch"] == macro("SPGEMM_FALLBACK_MAX_BATCH")
