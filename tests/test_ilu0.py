"""Zero-fill incomplete LU and BiCGStab preconditioned by triangular plans
(spmv_csr_ilu0, spmv_*_bicgstab_trsv; spmv_engine.h): what can be checked
without a GPU -- the declared surface, the size of the work buffer, the
binding's argument checks, and the numpy restatements of tests/_ilu0.py against
the definitions: a dense LU where the pattern has no fill, L U = A on the
pattern, and fewer iterations than Jacobi.  The kernels themselves:
tests/test_gpu_ilu0.py and tests/test_gpu_bicgstab_trsv.py."""
import ctypes as C
import errno

import numpy as np
import pytest

import _bicgstab as BI
import _cg as G
import _ic0 as IC
import _ilu0 as IL
import _pcg_trsv as PT
import _trsv as TV
import spmv_scpa_amd as S

SHAPE = S.trsv_shape()
L = SHAPE["small_rows"]
TOL = 1e-8


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ------------------------------------------------------------- the surface
def test_the_headers_declare_the_entry_points():
    declared = S.declared_symbols()
    for name in ("spmv_csr_ilu0", "spmv_bicgstab_trsv_work_bytes",
                 "spmv_csr_bicgstab_trsv", "spmv_hll_bicgstab_trsv"):
        assert name in declared and hasattr(S._lib, name), name
    assert S.check_symbols()
    assert S.version() == "spmv_scpa_amd 0.7 gfx950"
    vp, ip, i64 = C.c_void_p, C.c_int, C.c_int64
    fn = S._lib.spmv_csr_ilu0
    assert fn.restype is C.c_int
    assert fn.argtypes == [vp, C.c_double, ip, C.POINTER(vp),
                           C.POINTER(S.Ilu0Info)]
    fn = S._lib.spmv_bicgstab_trsv_work_bytes
    assert fn.restype is i64 and fn.argtypes == [ip, ip]
    for fmt in ("csr", "hll"):
        fn = getattr(S._lib, "spmv_%s_bicgstab_trsv" % fmt)
        twin = getattr(S._lib, "spmv_%s_pcg_trsv" % fmt)
        assert fn.restype is C.c_int
        assert fn.argtypes == twin.argtypes == [
            vp, C.POINTER(S.LaunchOpts), ip, vp, i64, vp, i64, vp, vp, vp,
            C.c_double, ip, ip, vp, C.c_size_t, C.POINTER(S.CgInfo), vp]
    assert [f for f, _ in S.Ilu0Info._fields_] == \
        ["levels", "launches", "entries", "bad_pivots"]
    assert C.sizeof(S.Ilu0Info) == 24
    assert callable(S.CsrDevice.ilu0)
    assert callable(S.CsrDevice.bicgstab_trsv)
    assert callable(S.HllDevice.bicgstab_trsv)


def test_the_work_buffer_has_seven_vectors():
    base = S.bicgstab_trsv_work_bytes(0, 1)
    assert base == S.bicgstab_work_bytes(0, 1) > 0
    for M in (0, 1, 1073, 10_000_000):
        for k in range(1, 9):
            assert S.bicgstab_trsv_work_bytes(M, k) == base + 7 * 8 * M * k
            # bicgstab's own buffer: unchanged, six vectors
            assert S.bicgstab_work_bytes(M, k) == base + 6 * 8 * M * k
    fn = S._lib.spmv_bicgstab_trsv_work_bytes
    for M, k in ((-1, 1), (10, 0), (10, 9), (10, -3)):
        assert fn(M, k) == -errno.EINVAL, (M, k)
        with pytest.raises(OSError):
            S.bicgstab_trsv_work_bytes(M, k)


def test_the_binding_checks_its_arguments():
    fake = object.__new__(S.CsrDevice)  # a wrapper around no handle
    fake.h = None
    for kw in (dict(shift=-0.5), dict(shift=float("nan")),
               dict(shift=float("inf")), dict(max_levels=-1)):
        with pytest.raises(ValueError):
            fake.ilu0(**kw)
    with pytest.raises(OSError) as ei:
        fake.ilu0()
    assert ei.value.errno == errno.EINVAL  # the library's answer to NULL
    for args in ((None,), (object(),)):
        with pytest.raises(ValueError):
            fake.bicgstab_trsv(0, 0, *args)


def test_dead_handles_and_argument_errors_of_the_library():
    junk = C.create_string_buffer(512)  # never a handle of the library
    pj = C.cast(junk, C.c_void_p)
    dead = -errno.EBADF if S.device_count() > 0 else -errno.ENODEV
    before = S._lib.spmv_live_handles()
    out, info = C.c_void_p(1234), S.Ilu0Info()
    ilu0 = S._lib.spmv_csr_ilu0
    assert ilu0(None, 0.0, 0, C.byref(out), None) == -errno.EINVAL
    assert ilu0(pj, 0.0, 0, None, None) == -errno.EINVAL
    for shift, cap in ((-1.0, 0), (float("nan"), 0), (float("inf"), 0),
                       (0.0, -1)):
        assert ilu0(pj, shift, cap, C.byref(out), C.byref(info)) == \
            -errno.EINVAL
    assert ilu0(pj, 0.25, 7, C.byref(out), C.byref(info)) == dead
    assert out.value is None  # *out is NULL after an error
    assert S._lib.spmv_live_handles() == before


# ------------------------------------------------------------ the reference
def test_the_reference_on_a_matrix_written_out():
    # A = L U with L = [[1], [0.5, 1], [-2, 3, 1]], U = [[2, 4, -2], [0, 1, 3],
    # [0, 0, 4]]: a full pattern has no fill to drop
    rows = [[(0, 2.0), (1, 4.0), (2, -2.0)],
            [(0, 1.0), (1, 3.0), (2, 2.0)],
            [(0, -4.0), (1, -5.0), (2, 17.0)]]
    M, IRP, JA, AS = TV.from_rows(rows)
    F = IL.reference_ilu0(M, IRP, JA, AS)
    assert F.AS.tolist() == [2.0, 4.0, -2.0, 0.5, 1.0, 3.0, -2.0, 3.0, 4.0]
    assert F.bad_pivots == 0
    # shift: the diagonal becomes a_ii + shift * a_ii before the updates
    F = IL.reference_ilu0(M, IRP, JA, AS, shift=0.5)
    assert F.AS[:4].tolist() == [3.0, 4.0, -2.0, 1.0 / 3.0]
    # dropping (1, 2) and (2, 1) from the pattern drops their updates
    rows = [[(0, 2.0), (1, 4.0), (2, -2.0)],
            [(0, 1.0), (1, 3.0)],
            [(0, -4.0), (2, 17.0)]]
    F = IL.reference_ilu0(*TV.from_rows(rows))
    assert F.AS.tolist() == [2.0, 4.0, -2.0, 0.5, 1.0, -2.0, 13.0]


@pytest.mark.parametrize("name", ["tridiagonal", "arrow2 reversed"])
def test_without_fill_the_reference_is_the_dense_lu(name):
    """the derived bound is ZERO: the dense loop does the operations of the
    contract in the contract's order, and every operation it adds has an exact
    zero for an operand (l = 0 / u, w - l * 0), so it changes no bit.

    arrow2 is compared in reversed order.  As _bicgstab.arrow2 numbers it, the
    dense row and column come FIRST and the exact LU fills the whole matrix
    (ILU(0) drops all of that: checked below); with them last there is no
    fill."""
    mat = (IL.tridiagonal(40) if name == "tridiagonal"
           else IL.MATRICES["arrow2(600,3) reversed"]())
    M, IRP, JA, AS = mat
    F = IL.reference_ilu0(*mat)
    D = IL.dense_lu(IL.dense_of(*mat))
    rows = np.repeat(np.arange(M), np.diff(IRP))
    assert np.array_equal(bits(D[rows, JA]), bits(F.AS)), name
    D[rows, JA] = 0.0
    assert not D.any(), "the exact LU has fill"
    assert F.bad_pivots == 0 and IL.pattern_ratio(mat, F) <= 1.0
    if name != "tridiagonal":
        nat = IL.MATRICES["arrow2(600,3)"]()
        full = IL.dense_lu(IL.dense_of(*nat))
        assert np.count_nonzero(full) == 600 * 600   # fill everywhere


@pytest.mark.parametrize("shift", [0.0, 0.25])
@pytest.mark.parametrize("name", list(IL.MATRICES))
def test_on_the_pattern_the_factors_reproduce_the_matrix(name, shift):
    """|sum_m l_im u_mj - a_ij| <= (n + 3) u sum_m |l_im u_mj| for every stored
    (i, j): n products and subtractions, a division, the shift's two"""
    mat = IL.MATRICES[name]()
    F = IL.reference_ilu0(*mat, shift=shift)
    assert F.bad_pivots == 0 and np.all(np.isfinite(F.AS))
    ratio = IL.pattern_ratio(mat, F, shift)
    print(name, shift, "largest ratio", ratio)
    assert ratio <= 1.0, (name, ratio)


def test_the_shapes_take_the_kernels_they_are_for():
    def segs(mat):
        plan = TV.reference_plan(*PT.int32(mat)[1:], "lower")
        return TV.segments(plan["level_ptr"], L), np.diff(plan["level_ptr"])
    s, rows = segs(IL.MATRICES["convdiff(37,29)"]())
    assert s == [(TV.CHAIN, 0, 64)] and rows.max() <= L   # the chain alone
    s, rows = segs(IL.MATRICES["red-black convdiff(37,29)"]())
    assert s == [(TV.WIDE, 0, 0), (TV.WIDE, 1, 1)]        # the wide alone
    assert rows.tolist() == [537, 536]
    s, rows = segs(IL.MATRICES["arrow2(600,3)"]())
    assert s == [(TV.CHAIN, 0, 0), (TV.WIDE, 1, 1)] and rows.tolist() == [1, 599]
    s, rows = segs(IL.MATRICES["arrow2(600,3) reversed"]())
    assert s == [(TV.WIDE, 0, 0), (TV.CHAIN, 1, 1)] and rows.tolist() == [599, 1]
    mat = IL.MATRICES["layered"]()
    s, rows = segs(mat)
    assert rows.tolist() == [3, 140, 5, 131]
    assert s == [(TV.CHAIN, 0, 0), (TV.WIDE, 1, 1), (TV.CHAIN, 2, 2),
                 (TV.WIDE, 3, 3)]
    # ... nonsymmetric, strictly dominant, and the update loop has work
    M, IRP, JA, AS = mat
    D = IL.dense_of(*mat)
    assert np.array_equal(D != 0, (D != 0).T) and not np.allclose(D, D.T)
    assert np.all(2 * np.abs(np.diag(D)) > np.abs(D).sum(axis=1))
    dpos = IL.diag_positions(M, IRP, JA)
    updates = 0
    for i in range(M):
        for t in range(IRP[i], dpos[i]):
            j = JA[t]
            updates += len(np.intersect1d(JA[t + 1:IRP[i + 1]],
                                          JA[dpos[j] + 1:IRP[j + 1]]))
    assert updates > 1000, updates


def test_a_zero_pivot_reaches_exactly_the_dependent_rows():
    mat = IL.with_zero_pivot(IL.MATRICES["layered"](), 1)
    F = IL.reference_ilu0(*mat)
    plan = TV.reference_plan(*PT.int32(mat)[1:], "lower")
    hit = TV.reachable(plan, 1)
    hit[1] = False   # row 1 itself: a finite row with a zero pivot
    assert np.array_equal(IL.nonfinite_rows(F), hit)
    assert hit.sum() == mat[0] - 3 and F.bad_rows[0] == 1
    assert F.bad_pivots == 1 + hit.sum()


# ------------------------------------------------------------- the solver
def cpu_callables(mat, B, X0):
    M, IRP, JA, AS = mat
    rows = np.repeat(np.arange(M), np.diff(IRP))

    def product(Z):
        return np.stack([np.bincount(rows, AS * Z[JA, j], minlength=M)
                         for j in range(Z.shape[1])], axis=1)
    return product, lambda: B - product(X0)


def test_with_a_diagonal_the_restatement_is_that_of_bicgstab():
    mat = BI.rowscale(BI.convdiff(15, 17, 0.5, 0.5), 5)
    M = mat[0]
    B, X0 = G.common_inputs(M)
    product, residual0 = cpu_callables(mat, B, X0)
    minv = 1.0 / IL.dense_of(*mat).diagonal()
    for d in (None, minv):
        want = BI.restate(product, residual0, B, X0, d, TOL, 200)
        got = IL.restate(product, residual0, B, X0,
                         (lambda U: U.copy()) if d is None
                         else (lambda U: d[:, None] * U), TOL, 200)
        assert np.array_equal(bits(got.X), bits(want.X))
        assert got.iterations.tolist() == want.iterations.tolist()
        assert got.status.tolist() == want.status.tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("name", ["convdiff(37,29)",
                                  "red-black convdiff(37,29)"])
def test_ilu0_takes_fewer_iterations_than_jacobi(name):
    mat = IL.MATRICES[name]()
    M = mat[0]
    B, X0 = G.common_inputs(M, 1)
    product, residual0 = cpu_callables(mat, B, X0)
    minv = 1.0 / IL.dense_of(*mat).diagonal()
    jacobi = BI.restate(product, residual0, B, X0, minv, TOL, 1000)
    ilu = IL.restate(product, residual0, B, X0,
                     PT.plans_apply(*IL.ilu0(mat), SHAPE["group"]), TOL, 1000)
    print(name, "ilu0", ilu.iterations, "jacobi", jacobi.iterations)
    assert jacobi.status.tolist() == [0] and ilu.status.tolist() == [0]
    assert ilu.iterations[0] < jacobi.iterations[0]
    M_, IRP, JA, AS = mat
    rows = np.repeat(np.arange(M), np.diff(IRP))
    res = np.linalg.norm(B[:, 0] - np.bincount(rows, AS * ilu.X[JA, 0],
                                               minlength=M))
    assert res <= 2 * TOL * np.linalg.norm(B[:, 0])
