"""The host arithmetic of the sparse sum (size classes and group widths, grids,
the scratch layout and the overflow guards: spmv_scpa_amd/csrc/add_plan.h,
which the launcher, spmv_add_shape and the tests all read) compiled for the
CPU as a stand-alone program and run under AddressSanitizer + UBSan over 4000
seeded inputs.  No Python code runs under a sanitizer."""
import os
import re
import subprocess
import sys

import spmv_scpa_amd as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_add_plan_under_asan(tmp_path):
    exe = str(tmp_path / "add_plan_asan")
    subprocess.run(
        ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined",
         "-fno-omit-frame-pointer", "-fno-sanitize-recover=all",
         "-I", os.path.join(ROOT, "spmv_scpa_amd", "csrc"),
         os.path.join(ROOT, "tests", "asan", "add_plan_asan.cc"),
         "-o", exe], check=True)
    r = subprocess.run([exe, "4000"], capture_output=True, text=True)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "every row in one class" in r.stdout
    assert "FAILED" not in r.stdout + r.stderr and "ERROR" not in r.stderr


def test_the_library_reports_the_numbers_of_the_header():
    """spmv_add_shape against the header's text"""
    hdr = open(os.path.join(ROOT, "spmv_scpa_amd", "csrc",
                            "add_plan.h")).read()

    def macro(name):
        m = re.search(r"#define\s+%s\s+(\w+)" % name, hdr)
        assert m, name
        return int(m.group(1))

    shape = S.add_shape()
    assert shape["edge"] == macro("ADD_EDGE")
    assert shape["threads"] == macro("ADD_THREADS")
    assert len(shape["widths"]) == macro("ADD_WIDTHS")
    assert shape["widths"][0] == macro("ADD_WIDTH_MIN")
    assert shape["widths"][-1] == macro("ADD_WIDTH_MAX")
    m = re.search(r"add_width_\[ADD_WIDTHS\]\s*=\s*\{([^}]*)\}", hdr)
    assert shape["widths"] == [int(x) for x in m.group(1).split(",")]
