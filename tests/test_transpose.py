"""Transposition of CSR handles on the device (spmv_csr_transpose,
spmv_transpose_plan, spmv_csr_symmetry; spmv_engine.h): what can be checked
without a GPU -- the declared surface, the ctypes signatures, the dead-handle
answers, the plan's arithmetic (also under AddressSanitizer + UBSan, as a
stand-alone program over transpose_plan.h), and the numpy restatement of the
device algorithm (tests/_transpose.py) against the four-line reference on
every shape the GPU tests run.  The kernels themselves:
tests/test_gpu_transpose.py."""
import ctypes as C
import errno
import os
import subprocess
import sys

import numpy as np
import pytest

import _transpose as TR
import spmv_scpa_amd as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["spmv_csr_transpose", "spmv_transpose_plan", "spmv_csr_symmetry"]


def test_the_headers_declare_the_transpose_entry_points():
    declared = S.declared_symbols()
    for name in NEW:
        assert name in declared, name
        assert hasattr(S._lib, name), name
    assert S.check_symbols()
    # the feature is detected by the symbol, not by the version string
    assert S.version() == "spmv_scpa_amd 0.7 gfx950"


def test_the_ctypes_signatures():
    fn = S._lib.spmv_csr_transpose
    assert fn.restype is C.c_int
    assert fn.argtypes == [C.c_void_p, C.POINTER(C.c_void_p)]
    fn = S._lib.spmv_csr_symmetry
    assert fn.restype is C.c_int
    assert fn.argtypes == [C.c_void_p, C.POINTER(C.c_int)]
    fn = S._lib.spmv_transpose_plan
    assert fn.restype is C.c_int
    assert fn.argtypes == [C.c_int, C.c_int64, C.POINTER(C.c_int),
                           C.POINTER(C.c_int), C.POINTER(C.c_int),
                           C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    assert (S.SYM_NONE, S.SYM_PATTERN, S.SYM_VALUES) == (0, 1, 2)
    assert callable(S.CsrDevice.transpose) and callable(S.CsrDevice.symmetry)


def test_dead_handles_are_refused():
    junk = C.create_string_buffer(512)  # never a handle of the library
    pj = C.cast(junk, C.c_void_p)
    dead = -errno.EBADF if S.device_count() > 0 else -errno.ENODEV
    before = S._lib.spmv_live_handles()
    out = C.c_void_p(1234)
    assert S._lib.spmv_csr_transpose(None, C.byref(out)) == -errno.EINVAL
    assert S._lib.spmv_csr_transpose(pj, None) == -errno.EINVAL
    assert S._lib.spmv_csr_transpose(pj, C.byref(out)) == dead
    assert out.value is None  # *out is NULL after an error
    sym = C.c_int(77)
    assert S._lib.spmv_csr_symmetry(None, C.byref(sym)) == -errno.EINVAL
    assert S._lib.spmv_csr_symmetry(pj, None) == -errno.EINVAL
    assert S._lib.spmv_csr_symmetry(pj, C.byref(sym)) == dead
    assert sym.value == 0
    assert S._lib.spmv_live_handles() == before
    fake = object.__new__(S.CsrDevice)  # a wrapper around no handle
    fake.h = None
    for call in (fake.transpose, fake.symmetry):
        with pytest.raises(OSError) as ei:
            call()
        assert ei.value.errno == errno.EINVAL


# ------------------------------------------------------------------ the plan
def test_the_pass_count_follows_the_digits_of_the_last_column():
    d = S.transpose_plan(1, 1)["digit_bits"]
    assert d == 8
    want = {0: 1, 1: 1, 2: 1, 2**d: 1, 2**d + 1: 2, 2**(2 * d): 2,
            2**(2 * d) + 1: 3, 2**(3 * d): 3, 2**(3 * d) + 1: 4,
            2**31 - 1: 4}
    for N, passes in want.items():
        p = S.transpose_plan(N, 1000)
        assert p["passes"] == passes, (N, p)
        assert p["passes"] == max(1, -(-max(N - 1, 0).bit_length() // d))
        assert p["digit_bits"] == d


def test_the_workgroups_cover_the_entries_and_the_scratch_does_not_wrap():
    p0 = S.transpose_plan(300, 0)
    tile = p0["tile"]
    assert tile > 0 and tile % 64 == 0
    assert p0["workgroups"] == 0
    last = p0["scratch_bytes"]
    assert last >= 0
    for NZ in (1, 63, 64, 65, tile - 1, tile, tile + 1, 3 * tile + 17,
               10**6, 320 * 10**6, 2**31 - 2, 2**31 - 1):
        p = S.transpose_plan(300, NZ)
        assert p["tile"] == tile
        assert p["workgroups"] * tile >= NZ > (p["workgroups"] - 1) * tile
        assert p["scratch_bytes"] >= last, NZ  # monotone in NZ
        last = p["scratch_bytes"]
    # exact at the largest handle (N = 2^31 - 1: four passes, two buffers):
    # the pair buffers, 2^digit_bits counters per workgroup, one tile sum per
    # 2048 scanned ints (the N + 1 column counts are the longer scan), a flag;
    # every part rounded up to 256 bytes
    NZ = N = 2**31 - 1
    p = S.transpose_plan(N, NZ)
    up = lambda b: -(-b // 256) * 256  # noqa: E731
    wgs = -(-NZ // tile)
    assert p["workgroups"] == wgs and p["passes"] == 4
    sums = max(-(-(wgs * 256) // 2048), -(-(N + 1) // 2048))
    assert p["scratch_bytes"] == (2 * up(8 * NZ) + up(4 * 256 * wgs) +
                                  up(4 * sums) + 256)
    assert p["scratch_bytes"] > 2**35
    # one pass has two buffers as well: the second holds the gather's row index
    one, two = S.transpose_plan(256, 10**6), S.transpose_plan(257, 10**6)
    assert (one["passes"], two["passes"]) == (1, 2)
    assert two["scratch_bytes"] == one["scratch_bytes"] > 2 * 8 * 10**6


def test_the_plan_refuses_negative_sizes():
    for N, NZ in ((-1, 0), (0, -1), (-5, -5), (3, 2**31)):
        assert S._lib.spmv_transpose_plan(N, NZ, None, None, None, None,
                                          None) == -errno.EINVAL
        with pytest.raises(OSError) as ei:
            S.transpose_plan(N, NZ)
        assert ei.value.errno == errno.EINVAL
    # any out-pointer may be NULL
    assert S._lib.spmv_transpose_plan(5, 5, None, None, None, None, None) == 0


def test_the_plan_arithmetic_under_asan(tmp_path):
    """transpose_plan.h as a stand-alone program under ASan + UBSan: the edges,
    2000 seeded random plans, and the sort restated with the kernels' index
    arithmetic over heap blocks of exactly the planned sizes"""
    exe = str(tmp_path / "transpose_plan_asan")
    subprocess.run(
        ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined",
         "-fno-omit-frame-pointer", "-fno-sanitize-recover=all",
         "-I", os.path.join(ROOT, "spmv_scpa_amd", "csrc"),
         os.path.join(ROOT, "tests", "asan", "transpose_plan_asan.cc"),
         "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    r = subprocess.run([exe, "2000"], capture_output=True, text=True, env=env)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "plans hold, sorts are stable" in r.stdout
    assert "FAILED" not in r.stdout and "ERROR" not in r.stderr


# ------------------------------------------------- reference and restatement
def same(got, want):
    """three arrays each, compared as integers and as the bits of the values"""
    for g, w in zip(got[:2], want[:2]):
        if g.dtype != np.int32 or not np.array_equal(g, w):
            return False
    v = np.uint64 if got[2].dtype == np.float64 else np.uint32
    return np.array_equal(np.ascontiguousarray(got[2]).view(v),
                          np.ascontiguousarray(want[2]).view(v))


def test_the_reference_on_a_matrix_written_out():
    M, N, IRP, JA, AS = TR.duplicates()
    IRP_T, JA_T, AS_T = TR.reference(IRP, JA, AS, N)
    assert IRP_T.tolist() == [0, 4, 5, 7, 8, 11, 13]
    assert JA_T.tolist() == [0, 1, 3, 3, 1, 0, 2, 2, 1, 1, 1, 0, 3]
    # (1, 4) three times and (3, 0) twice, in their stored order; the zero
    assert AS_T.tolist() == [2.0, 5.0, 7.0, 9.0, 4.0, 3.0, 0.0, 6.0, 10.0,
                             20.0, 30.0, 1.0, 8.0]
    # (A^T)^T: every row stably ordered by column
    back = TR.reference(IRP_T, JA_T, AS_T, M)
    assert same(back, TR.row_sorted(IRP, JA, AS))
    assert back[1].tolist() == [0, 2, 5, 0, 1, 4, 4, 4, 2, 3, 0, 0, 5]
    assert back[2][5:8].tolist() == [10.0, 20.0, 30.0]


def test_the_restatement_equals_the_reference_on_every_gpu_shape():
    tile = S.transpose_plan(1, 1)["tile"]
    shapes = TR.gpu_shapes(tile)
    seen_passes, most_tiles, ragged, hub_tiles = set(), 0, False, 0
    for name, (M, N, IRP, JA, AS) in shapes.items():
        assert len(IRP) == M + 1 and IRP[-1] == len(JA) == len(AS), name
        assert len(JA) == 0 or (JA.min() >= 0 and JA.max() < N), name
        plan = S.transpose_plan(N, len(JA))
        stats = {}
        got = TR.model(IRP, JA, AS, N, plan, stats)
        assert same(got, TR.reference(IRP, JA, AS, N)), name
        if len(JA):
            seen_passes.add(stats["passes"])
            most_tiles = max(most_tiles, stats["tiles"])
            ragged |= stats["tiles"] > 1 and 0 < stats["last_tile"] < tile
        if name == "hub":
            hub_tiles = stats["bucket_tiles"]
            assert stats["tiles"] == -(-3 * 70000 // tile)
    # the shapes do what they are for
    assert most_tiles > 1                      # more than one tile
    assert ragged                              # a last tile that is not full
    assert seen_passes == {1, 2, 3, 4}         # every pass count (N < 2^31)
    assert hub_tiles > 8                       # one bucket across many tiles
    M, N, IRP, JA, AS = shapes["hub"]
    assert np.count_nonzero(JA == 7) >= M > 8192  # a long row of T
    M, N, IRP, JA, AS = shapes["n=%d" % (2**24 + 1)]
    assert JA.max() == 2**24 and JA.min() == 0  # the top digit, both ends
    assert S.transpose_plan(N, len(JA))["passes"] == 4
