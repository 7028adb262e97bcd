"""Zero-fill incomplete LU on the device (spmv_csr_ilu0; spmv_engine.h).

The factor is compared with the numpy restatement (tests/_ilu0.py
reference_ilu0) through download(): the index arrays as integers, the values as
uint64.  The shapes are the smallest on which each kernel can go wrong: the
natural stencil (65 thin levels: the chain kernel alone), its red-black
permutation (2 wide levels: the wide kernel alone), an arrow (a thin and a wide
level; every row searches the tail of the dense row), its reversal (a row far
longer than a group of lanes), a layered nonsymmetric matrix whose rows share
columns (both kernels, updates in both triangles), M = 0 and M = 1.

Every test runs under a time limit of its own (LIMIT_S): a test that exceeds
it ends the whole process, so nothing else is started on the device.
"""
import ctypes as C
import errno
import faulthandler

import numpy as np
import pytest

import _bicgstab as BI
import _ilu0 as IL
import _pcg_trsv as PT
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
    A = S.csr_from_arrays("ilu0", M, M, IRP, JA, AS)
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


def same_factor(LU, info, F, mat, tag):
    """a device factor against the restatement: A's pattern, then the bits (a
    NaN is a NaN: its sign and payload are not part of the contract)"""
    IRP, JA, AS = arrays(LU)
    assert IRP.dtype == JA.dtype == np.int32, tag
    assert np.array_equal(IRP, mat[1]) and np.array_equal(JA, mat[2]), tag
    nan = np.isnan(F.AS)
    assert np.array_equal(np.isnan(AS), nan), (tag, "NaNs elsewhere")
    differ = np.flatnonzero((bits(AS) != bits(F.AS)) & ~nan)
    assert len(differ) == 0, (tag, "entries that differ", len(differ),
                              differ[:4].tolist(), AS[differ[:4]],
                              F.AS[differ[:4]])
    assert info.entries == len(mat[2]) == LU.NZ, tag
    assert info.bad_pivots == F.bad_pivots, (tag, info.bad_pivots)
    return AS


@pytest.mark.parametrize("name", list(IL.MATRICES))
def test_the_factor_has_the_bits_of_the_restatement(name):
    mat = IL.MATRICES[name]()
    M = mat[0]
    F = IL.reference_ilu0(*mat)
    plan = TV.reference_plan(*PT.int32(mat)[1:], "lower")
    segs = TV.segments(plan["level_ptr"], SHAPE["small_rows"])
    d = upload(mat)
    live = S._lib.spmv_live_handles()
    for waves in (0, 1, 16):
        S._lib.set_csr_waves_per_block(waves)
        tag = (name, waves)
        LU, info = d.ilu0()
        assert S._lib.spmv_live_handles() == live + 1
        assert (LU.M, LU.N, LU.value_bytes) == (M, M, 8), tag
        same_factor(LU, info, F, mat, tag)
        assert info.levels == len(plan["level_ptr"]) - 1, tag
        assert info.launches == len(segs), tag
        LU.release()
        assert S._lib.spmv_live_handles() == live
    S._lib.set_csr_waves_per_block(0)
    # A is unchanged
    assert np.array_equal(bits(arrays(d)[2]), bits(mat[3])), name
    # a shift: the same check (the diagonal grows before the updates)
    F25 = IL.reference_ilu0(*mat, shift=0.25)
    LU, info = d.ilu0(shift=0.25)
    same_factor(LU, info, F25, mat, (name, "shift"))
    # the factor is an ordinary handle: y = LU x, its transpose, both plans
    x = np.random.default_rng(2).uniform(-1.0, 1.0, M)
    d_x, d_y = S.DevBuffer.from_numpy(x), S.DevBuffer(M * 8)
    LU.launch(2, d_x.ptr, d_y.ptr)
    S.stream_sync()
    rows = np.repeat(np.arange(M), np.diff(F25.IRP))
    want = np.bincount(rows, F25.AS * x[F25.JA], minlength=M)
    scale = np.bincount(rows, np.abs(F25.AS * x[F25.JA]), minlength=M)
    assert np.all(np.abs(d_y.to_numpy(np.float64, M) - want)
                  <= 1e-12 * scale + 1e-300)
    T = LU.transpose()
    assert (T.M, T.N, T.NZ) == (M, M, LU.NZ)
    lo, up = LU.trsv_analyse("lower", unit=True), LU.trsv_analyse("upper")
    assert lo.info["levels"] == info.levels
    assert up.info["zero_diag"] == 0
    assert lo.info["entries"] + up.info["entries"] + M == LU.NZ
    # ... and the plans solve with the factor's bits: z = U^-1 L^-1 r
    first, second, _ = IL.ilu0(mat, shift=0.25)
    r = np.random.default_rng(3).uniform(-1.0, 1.0, (M, 2))
    d_r, d_z = S.DevBuffer.from_numpy(r), S.DevBuffer(M * 2 * 8)
    lo.solve(d_r.ptr, d_z.ptr, 2)
    up.solve(d_z.ptr, d_z.ptr, 2)
    S.stream_sync()
    z = PT.plans_apply(first, second, None, SHAPE["group"])(r)
    assert np.array_equal(bits(d_z.to_numpy(np.float64, M * 2)),
                          bits(z.ravel())), name
    for h in (lo, up, T, LU, d):
        h.release()
    for b in (d_x, d_y, d_r, d_z):
        b.free()
    assert S._lib.spmv_live_handles() == live - 1


def test_no_rows_and_one_row():
    live = S._lib.spmv_live_handles()
    d = upload(TV.empty())
    LU, info = d.ilu0()
    assert (LU.M, LU.N, LU.NZ) == (0, 0, 0)
    assert (info.levels, info.launches, info.entries, info.bad_pivots) == \
        (0, 0, 0, 0)
    assert arrays(LU)[0].tolist() == [0]
    LU.release()
    d.release()
    inf = float("inf")
    # plain arithmetic: rn(a + rn(shift * a)); 0 * inf is NaN
    for a, shift, want, bad in ((6.25, 0.0, 6.25, 0), (4.0, 0.5625, 6.25, 0),
                                (0.0, 0.0, 0.0, 1), (-4.0, 0.0, -4.0, 0),
                                (inf, 0.0, np.nan, 1), (inf, 0.5, inf, 1)):
        d = upload(TV.from_rows([[(0, a)]]))
        LU, info = d.ilu0(shift=shift)
        got = arrays(LU)[2]
        assert (LU.M, LU.NZ, info.levels, info.launches) == (1, 1, 1, 1)
        assert info.bad_pivots == bad, (a, info.bad_pivots)
        assert (np.isnan(got[0]) if np.isnan(want) else got[0] == want), a
        F = IL.reference_ilu0(*TV.from_rows([[(0, a)]]), shift=shift)
        assert F.bad_pivots == bad
        assert np.isnan(F.AS[0]) if np.isnan(want) else F.AS[0] == want
        LU.release()
        d.release()
    assert S._lib.spmv_live_handles() == live


def test_a_zero_pivot_is_arithmetic_and_not_an_error():
    mat = IL.with_zero_pivot(IL.MATRICES["layered"](), 1)
    F = IL.reference_ilu0(*mat)
    plan = TV.reference_plan(*PT.int32(mat)[1:], "lower")
    hit = TV.reachable(plan, 1)
    d = upload(mat)
    LU, info = d.ilu0()     # no OSError: the return code is 0
    AS = same_factor(LU, info, F, mat, "zero pivot")
    rows = np.repeat(np.arange(mat[0]), np.diff(mat[1]))
    got = np.bincount(rows[~np.isfinite(AS)], minlength=mat[0]) > 0
    # inf / NaN in exactly the rows that depend on row 1; row 1 itself is a
    # finite row whose pivot is the zero
    hit[1] = False
    assert np.array_equal(got, hit) and hit.sum() == mat[0] - 3
    assert info.bad_pivots == 1 + hit.sum()
    LU.release()
    d.release()


def test_every_refusal_in_the_stated_order():
    ilu0 = S._lib.spmv_csr_ilu0
    mat = BI.convdiff(9, 7, 0.5, 0.5)
    d = upload(mat)
    out, info = C.c_void_p(77), S.Ilu0Info()
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

    def refused(h, shift=0.0, cap=0):
        out.value = 77
        rc = ilu0(h, shift, cap, C.byref(out), C.byref(info))
        assert out.value is None and S._lib.spmv_live_handles() == live, rc
        return -rc

    # the arguments come before everything, a dead handle before its shape
    assert ilu0(None, 0.0, 0, C.byref(out), None) == -errno.EINVAL
    assert ilu0(d.h, 0.0, 0, None, None) == -errno.EINVAL
    assert refused(junk, shift=-1.0) == errno.EINVAL
    assert refused(d.h, shift=-1.0) == errno.EINVAL
    assert refused(d.h, shift=float("nan")) == errno.EINVAL
    assert refused(junk, cap=-1) == errno.EINVAL
    assert refused(junk) == errno.EBADF
    assert refused(rect.h) == errno.EINVAL
    assert refused(f32.h) == errno.ENOTSUP
    assert refused(gone.h) == errno.ENODATA
    assert refused(far.h) == errno.EDOM
    assert refused(d.h, cap=14) == errno.E2BIG   # 9 + 7 - 1 = 15 levels
    out.value = 77
    assert ilu0(d.h, 0.0, 15, C.byref(out), None) == 0   # info may be NULL
    assert S._lib.spmv_live_handles() == live + 1
    S._lib.spmv_csr_release(out)
    assert S._lib.spmv_live_handles() == live
    # max_levels = 3 on the natural stencil of the bit tests
    big = upload(IL.MATRICES["convdiff(37,29)"]())
    with pytest.raises(OSError) as ei:
        big.ilu0(max_levels=3)
    assert ei.value.errno == errno.E2BIG
    big.release()
    assert S._lib.spmv_live_handles() == live
    for h in (rect, f32, gone, far, d):
        h.release()
    with pytest.raises(OSError) as ei:
        d.ilu0()  # released: the binding passes NULL
    assert ei.value.errno == errno.EINVAL


def without_last_entry(mat):
    M, IRP, JA, AS = mat
    IRP = IRP.copy()
    IRP[-1] -= 1
    return M, IRP, JA[:-1].copy(), AS[:-1].copy()


def test_rows_the_pattern_check_refuses():
    """unsorted, duplicate and missing-diagonal rows: -EINVAL, nothing leaks;
    the WHOLE row is looked at, its upper part too"""
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
        "upper unsorted": with_row(0, [(0, 4.0), (3, 1.0), (2, -1.0)]),
        "upper twice": with_row(0, [(0, 4.0), (2, -1.0), (2, 5.0)]),
        # more rows than a workgroup of the check, the fault in the last one
        "no diagonal in the last of 1073 rows": without_last_entry(
            IL.MATRICES["red-black convdiff(37,29)"]()),
    }
    live = S._lib.spmv_live_handles()
    out, info = C.c_void_p(77), S.Ilu0Info()
    for name, mat in bad.items():
        d = upload(mat)
        with pytest.raises(OSError) as ei:
            d.ilu0()
        assert ei.value.errno == errno.EINVAL, name
        out.value = 77
        assert S._lib.spmv_csr_ilu0(d.h, 0.0, 0, C.byref(out),
                                    C.byref(info)) == -errno.EINVAL, name
        assert out.value is None, name   # *out is NULL, nothing was created
        assert S._lib.spmv_live_handles() == live + 1, name
        d.release()
        assert S._lib.spmv_live_handles() == live, name
    fine = TV.from_rows(base)
    want = IL.reference_ilu0(*fine)
    d = upload(fine)
    LU, info = d.ilu0()
    same_factor(LU, info, want, fine, "as it is")
    LU.release()
    d.release()
    # transpose().transpose() sorts the rows of a handle
    d = upload(bad["unsorted"])
    T = d.transpose()
    TT = T.transpose()
    sorted_ = TV.from_rows([base[0], base[1], base[2][:3], base[3]])
    LU, info = TT.ilu0()
    same_factor(LU, info, IL.reference_ilu0(*sorted_), sorted_,
                "sorted by two transpositions")
    for h in (LU, TT, T, d):
        h.release()
    assert S._lib.spmv_live_handles() == live
