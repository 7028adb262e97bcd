"""The sweep's chunk-fit rule (panel_launch.h "Chunk fit": a copy whose
counted steps fall by 10 % with 4608-slot chunks launches that shape) as a
stand-alone host program under AddressSanitizer + UBSan: both sides of the
threshold, the counted steps zeroed, every explicit request beside it, and
4000 seeded random shapes that must always name an instantiated kernel."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_panel_chunk_fit_rule_under_asan(tmp_path):
    exe = str(tmp_path / "panel_chunk_fit_asan")
    # the constants the library is compiled with (hip_common.h)
    hdr = open(os.path.join(ROOT, "spmv_scpa_amd", "csrc", "hip_common.h")).read()
    defs = []
    for name in ("NUM_XCD", "SPMV_VARIANT_TIMING_BITS"):
        m = re.search(r"#define\s+%s\s+(\d+|\([^)]*\))" % name, hdr)
        assert m, name
        defs.append("-D%s=%s" % (name, m.group(1)))
    subprocess.run(
        ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined",
         "-fno-omit-frame-pointer", "-fno-sanitize-recover=all"] + defs +
        ["-I", os.path.join(ROOT, "spmv_scpa_amd", "csrc"),
         os.path.join(ROOT, "tests", "asan", "panel_chunk_fit_asan.cc"),
         "-o", exe], check=True)
    r = subprocess.run([exe, "4000"], capture_output=True, text=True)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "every plan names an instantiated kernel" in r.stdout
    assert "FAILED" not in r.stdout and "ERROR" not in r.stderr
