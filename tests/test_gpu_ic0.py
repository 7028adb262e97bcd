"""Zero-fill incomplete Cholesky on the device (spmv_csr_ic0; spmv_engine.h).

L is compared with the numpy restatement (tests/_ic0.py reference_ic0) through
download(): the index arrays as integers, the values as uint64.  The shapes are
the smallest on which each kernel can go wrong: the natural stencil (65 thin
levels: the chain kernel alone), its red-black permutation (2 wide levels: the
wide kernel alone), an arrow (a thin and a wide level), a layered matrix whose
rows share columns (both kernels, and sums with terms), M = 0 and M = 1.

Every test runs under a time limit of its own (LIMIT_S): a test that exceeds
it ends the whole process, so nothing else is started on the device.
"""
import ctypes as C
import errno
import faulthandler

import numpy as np
import pytest

import _cg as G
import _ic0 as IC
import _trsv as TV
import spmv_scpa_amd as S

pytestmark = pytest.mark.gpu

LIMIT_S = 120
SHAPE = S.trsv_shape()


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()
    S._lib.set_csr_waves_per_block(0)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def upload(mat, values="f64"):
    M, IRP, JA, AS = mat
    A = S.csr_from_arrays("ic0", M, M, IRP, JA, AS)
    d = S.CsrDevice.upload(A, values=values)
    S.csr_free(A)
    return d


def arrays(d):
    """(IRP, JA, AS) of a handle, copied out of its download"""
    p = d.download()
    assert (p.contents.M, p.contents.N, p.contents.NZ) == (d.M, d.N, d.NZ)
    out = tuple(a.copy() for a in S.csr_arrays(p))
    S.csr_free(p)
    return out


def same_factor(Ld, info, F, tag):
    """a device factor against the restatement: the pattern, then the bits
    (a NaN is a NaN: its sign and payload are not part of the contract)"""
    IRP, JA, AS = arrays(Ld)
    assert IRP.dtype == JA.dtype == np.int32, tag
    assert np.array_equal(IRP, F.IRP) and np.array_equal(JA, F.JA), tag
    nan = np.isnan(F.AS)
    assert np.array_equal(np.isnan(AS), nan), (tag, "NaNs elsewhere")
    differ = np.flatnonzero((bits(AS) != bits(F.AS)) & ~nan)
    assert len(differ) == 0, (tag, "entries that differ", len(differ),
                              differ[:4].tolist(), AS[differ[:4]],
                              F.AS[differ[:4]])
    assert info.entries == len(F.JA) == Ld.NZ, tag
    assert info.bad_pivots == F.bad_pivots, (tag, info.bad_pivots)
    return AS


@pytest.mark.parametrize("name", list(IC.MATRICES))
def test_the_factor_has_the_bits_of_the_restatement(name):
    mat = IC.MATRICES[name]()
    M = mat[0]
    F = IC.reference_ic0(*mat)
    plan = TV.reference_plan(mat[1].astype(np.int32), mat[2].astype(np.int32),
                             mat[3], "lower")
    segs = TV.segments(plan["level_ptr"], SHAPE["small_rows"])
    d = upload(mat)
    low = upload(IC.lower_of(*mat))
    live = S._lib.spmv_live_handles()
    first = None
    for waves in (0, 1, 16):
        S._lib.set_csr_waves_per_block(waves)
        for src in (d, low):  # the full matrix, its stored-lower-only copy
            tag = (name, waves, "lower only" if src is low else "full")
            Ld, info = src.ic0()
            assert S._lib.spmv_live_handles() == live + 1
            assert (Ld.M, Ld.N, Ld.value_bytes) == (M, M, 8), tag
            AS = same_factor(Ld, info, F, tag)
            assert info.levels == len(plan["level_ptr"]) - 1, tag
            assert info.launches == len(segs), tag
            first = AS if first is None else first
            assert np.array_equal(bits(AS), bits(first)), tag
            Ld.release()
            assert S._lib.spmv_live_handles() == live
    S._lib.set_csr_waves_per_block(0)
    # a shift: the same check (the diagonal grows before the subtraction)
    Ld, info = d.ic0(shift=0.25)
    same_factor(Ld, info, IC.reference_ic0(*mat, shift=0.25), (name, "shift"))
    # L is an ordinary handle: y = L x, its transpose, a plan made from it
    x = np.random.default_rng(2).uniform(-1.0, 1.0, M)
    d_x, d_y = S.DevBuffer.from_numpy(x), S.DevBuffer(M * 8)
    Ld.launch(2, d_x.ptr, d_y.ptr)
    S.stream_sync()
    F25 = IC.reference_ic0(*mat, shift=0.25)
    rows = np.repeat(np.arange(M), np.diff(F25.IRP))
    want = np.bincount(rows, F25.AS * x[F25.JA], minlength=M)
    assert np.allclose(d_y.to_numpy(np.float64, M), want, rtol=1e-12,
                       atol=1e-12)
    LT = Ld.transpose()
    lo, up = Ld.trsv_analyse("lower"), LT.trsv_analyse("upper")
    assert lo.info["levels"] == up.info["levels"] == info.levels
    assert lo.info["zero_diag"] == 0 and lo.info["entries"] == Ld.NZ - M
    for h in (lo, up, LT, Ld, low, d):
        h.release()
    d_x.free()
    d_y.free()


def test_no_rows_and_one_row():
    live = S._lib.spmv_live_handles()
    d = upload(TV.empty())
    Ld, info = d.ic0()
    assert (Ld.M, Ld.N, Ld.NZ) == (0, 0, 0)
    assert (info.levels, info.launches, info.entries, info.bad_pivots) == \
        (0, 0, 0, 0)
    assert arrays(Ld)[0].tolist() == [0]
    Ld.release()
    d.release()
    for a, shift, want, bad in ((6.25, 0.0, 2.5, 0), (4.0, 0.5625, 2.5, 0),
                                (0.0, 0.0, 0.0, 1), (-4.0, 0.0, np.nan, 1)):
        d = upload(TV.from_rows([[(0, a)]]))
        Ld, info = d.ic0(shift=shift)
        got = arrays(Ld)[2]
        assert (Ld.M, Ld.NZ, info.levels, info.launches) == (1, 1, 1, 1)
        assert info.bad_pivots == bad, (a, info.bad_pivots)
        assert (np.isnan(got[0]) if np.isnan(want) else got[0] == want), a
        Ld.release()
        d.release()
    assert S._lib.spmv_live_handles() == live


def test_an_indefinite_stencil_is_arithmetic_and_not_an_error():
    mat = G.lap2d(37, 29, -1.3)
    F = IC.reference_ic0(*mat)
    assert F.bad_pivots > 0 and F.bad_rows[0] == 128
    d = upload(mat)
    Ld, info = d.ic0()
    same_factor(Ld, info, F, "indefinite")  # NaNs in exactly its entries
    Ld.release()
    Ld, info = d.ic0(shift=0.25)
    assert info.bad_pivots == 0
    same_factor(Ld, info, IC.reference_ic0(*mat, shift=0.25), "shifted")
    Ld.release()
    d.release()


def test_every_refusal_in_the_stated_order():
    ic0 = S._lib.spmv_csr_ic0
    mat = G.lap2d(9, 7, 0.5)
    M = mat[0]
    d = upload(mat)
    live = S._lib.spmv_live_handles()
    out, info = C.c_void_p(77), S.Ic0Info()

    def refused(h, shift=0.0, cap=0):
        out.value = 77
        rc = ic0(h, shift, cap, C.byref(out), C.byref(info))
        assert out.value is None and S._lib.spmv_live_handles() == live, rc
        return -rc

    junk = C.cast(C.create_string_buffer(512), C.c_void_p)
    rect = S.CsrDevice.upload(S.csr_from_arrays(
        "r", 2, 3, np.array([0, 1, 2]), np.array([0, 1]), np.ones(2)))
    f32 = d.to_f32()
    gone = upload(mat)
    try:
        S.set_panel_schedule("chain")
        gone.build_panels(0)
        gone.release_source()
    finally:
        S.set_panel_schedule("sweep")
    far = upload((3, np.array([0, 1, 3, 4]), np.array([0, 1, 5, 2]),
                  np.ones(4)))       # a column outside [0, N), unsorted too
    live = S._lib.spmv_live_handles()
    # the arguments come before everything, a dead handle before its shape
    assert ic0(None, 0.0, 0, C.byref(out), None) == -errno.EINVAL
    assert ic0(d.h, 0.0, 0, None, None) == -errno.EINVAL
    assert refused(junk, shift=-1.0) == errno.EINVAL
    assert refused(junk, cap=-1) == errno.EINVAL
    assert refused(junk) == errno.EBADF
    assert refused(rect.h) == errno.EINVAL
    assert refused(f32.h) == errno.ENOTSUP
    assert refused(gone.h) == errno.ENODATA
    assert refused(far.h) == errno.EDOM
    assert refused(d.h, cap=14) == errno.E2BIG   # 9 + 7 - 1 = 15 levels
    out.value = 77
    assert ic0(d.h, 0.0, 15, C.byref(out), None) == 0   # info may be NULL
    assert S._lib.spmv_live_handles() == live + 1
    S._lib.spmv_csr_release(out)
    assert S._lib.spmv_live_handles() == live
    for h in (rect, f32, gone, far, d):
        h.release()
    with pytest.raises(OSError) as ei:
        d.ic0()  # released: the binding passes NULL
    assert ei.value.errno == errno.EINVAL


def without_last_entry(mat):
    M, IRP, JA, AS = mat
    IRP = IRP.copy()
    IRP[-1] -= 1
    return M, IRP, JA[:-1].copy(), AS[:-1].copy()


def test_rows_the_pattern_check_refuses():
    """unsorted, duplicate and missing-diagonal rows: -EINVAL, nothing leaks;
    disorder in the UPPER triangle is not looked at"""
    base = [[(0, 4.0), (2, -1.0)],
            [(0, -1.0), (1, 4.0)],
            [(0, -1.0), (1, -1.0), (2, 4.0), (3, 7.0)],
            [(1, -1.0), (3, 4.0)]]

    def with_row(i, row):
        rows = [list(r) for r in base]
        rows[i] = row
        return TV.from_rows(rows)

    bad = {
        "unsorted": with_row(2, [(1, -1.0), (0, -1.0), (2, 4.0)]),
        "diagonal first": with_row(2, [(2, 4.0), (0, -1.0), (1, -1.0)]),
        "duplicate": with_row(2, [(0, -1.0), (0, -1.0), (1, -1.0), (2, 4.0)]),
        "twice the diagonal": with_row(3, [(1, -1.0), (3, 2.0), (3, 2.0)]),
        "no diagonal": with_row(3, [(1, -1.0), (2, -1.0)]),
        "empty row": with_row(1, []),
        # more rows than a workgroup of the check, the fault in the last one
        "no diagonal in the last of 1073 rows": without_last_entry(
            IC.lower_of(*IC.red_black(37, 29, 0.01))),
    }
    fine = {
        "as it is": TV.from_rows(base),
        "upper unsorted, twice, between the lower": with_row(
            0, [(3, 1.0), (0, 4.0), (2, -1.0), (2, 5.0), (1, 9.0)]),
    }
    live = S._lib.spmv_live_handles()
    for name, mat in bad.items():
        d = upload(mat)
        with pytest.raises(OSError) as ei:
            d.ic0()
        assert ei.value.errno == errno.EINVAL, name
        d.release()
        assert S._lib.spmv_live_handles() == live, name
    want = IC.reference_ic0(*fine["as it is"])
    for name, mat in fine.items():
        d = upload(mat)
        Ld, info = d.ic0()
        same_factor(Ld, info, want, name)
        Ld.release()
        d.release()
    # transpose().transpose() sorts the rows of a handle
    d = upload(bad["unsorted"])
    T = d.transpose()
    TT = T.transpose()
    Ld, info = TT.ic0()
    same_factor(Ld, info, want, "sorted by two transpositions")
    for h in (Ld, TT, T, d):
        h.release()
    assert S._lib.spmv_live_handles() == live
