"""Restarted GMRES on the device (spmv_*_gmres, spmv_*_gmres_trsv,
spmv_gmres_work_bytes; spmv_engine.h): what can be checked without a GPU -- the
declared surface, the ctypes signatures, the dead-handle answers, the argument
checks of the Python wrapper, the size of the work buffer, and the numpy
restatement of the solver (tests/_gmres.py) run with the CPU oracle's product
and checked against things that are not itself: finite termination, the
optimum over the Krylov space from numpy.linalg.lstsq, and BiCGStab's
restatement.  The kernels themselves: tests/test_gpu_gmres.py."""
import ctypes as C
import errno

import numpy as np
import pytest

import _bicgstab as BI
import _cg as G
import _gmres as GM
import _ilu0 as IL
import _oracle as O
import spmv_scpa_amd as S

NEW = ["spmv_csr_gmres", "spmv_hll_gmres", "spmv_csr_gmres_trsv",
       "spmv_hll_gmres_trsv", "spmv_gmres_work_bytes"]
TOL = 1e-8
SMALL = {"convdiff(5,4)": lambda: BI.convdiff(5, 4, 0.5, 0.5),
         "arrow2(17,3)": lambda: BI.arrow2(17, 3)}


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ------------------------------------------------------------ the surface
def test_the_headers_declare_the_gmres_entry_points():
    declared = S.declared_symbols()
    for name in NEW:
        assert name in declared, name
        assert hasattr(S._lib, name), name
    assert S.check_symbols()
    assert S.version() == "spmv_scpa_amd 0.7 gfx950"
    assert S.GMRES_MAX_RESTART == 64
    assert [f for f, _ in S.GmresInfo._fields_] == \
        ["status", "iterations", "restarts", "reserved", "rr", "est", "bb"]
    assert C.sizeof(S.GmresInfo) == 40


def test_the_twin_signatures_come_from_the_shared_list():
    names = [t[0] for t in S._TWINS]
    assert names.count("gmres") == 1 and names.count("gmres_trsv") == 1
    head = [C.c_void_p, C.POINTER(S.LaunchOpts), C.c_int, C.c_void_p,
            C.c_int64, C.c_void_p, C.c_int64]
    tail = [C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
            C.POINTER(S.GmresInfo), C.c_void_p]
    for fmt in ("csr", "hll"):
        fn = getattr(S._lib, "spmv_%s_gmres" % fmt)
        assert fn.restype is C.c_int
        assert fn.argtypes == head + [C.c_void_p] + tail
        fn = getattr(S._lib, "spmv_%s_gmres_trsv" % fmt)
        assert fn.restype is C.c_int
        assert fn.argtypes == head + [C.c_void_p] * 3 + tail
    assert S._lib.spmv_gmres_work_bytes.restype is C.c_int64
    assert S._lib.spmv_gmres_work_bytes.argtypes == [C.c_int] * 3


def test_work_bytes_answers_its_errors_and_grows_with_the_basis():
    einval = -errno.EINVAL
    assert S._lib.spmv_gmres_work_bytes(-1, 1, 30) == einval
    for k in (0, 9, -1):
        assert S._lib.spmv_gmres_work_bytes(10, k, 30) == einval
    for m in (0, -1, 65):
        assert S._lib.spmv_gmres_work_bytes(10, 1, m) == einval
        with pytest.raises(OSError) as ei:
            S.gmres_work_bytes(10, 1, m)
        assert ei.value.errno == errno.EINVAL
    bases = []
    for m in (1, 2, 30, 64):
        base = S.gmres_work_bytes(0, 1, m)
        assert base > 0 and base % 8 == 0
        bases.append(base)
        for k in range(1, 9):
            # the same base for every k: the state is sized for 8 columns
            assert S.gmres_work_bytes(0, k, m) == base
            # the basis of m + 1 vectors, W and Z
            assert S.gmres_work_bytes(1000, k, m) == \
                base + (m + 3) * 8 * k * 1000
    assert bases == sorted(set(bases))     # it grows with restart alone
    # no 32-bit overflow
    assert S.gmres_work_bytes(2**31 - 1, 8, 64) == \
        bases[-1] + 67 * 8 * 8 * (2**31 - 1)


def test_dead_handles_are_refused():
    x = C.create_string_buffer(64)
    px = C.cast(x, C.c_void_p)
    junk = C.create_string_buffer(512)  # never a handle of the library
    pj = C.cast(junk, C.c_void_p)
    info = (S.GmresInfo * 8)()
    dead = -errno.EBADF if S.device_count() > 0 else -errno.ENODEV
    for fmt in ("csr", "hll"):
        solve = getattr(S._lib, "spmv_%s_gmres" % fmt)
        trsv = getattr(S._lib, "spmv_%s_gmres_trsv" % fmt)
        multi = getattr(S._lib, "spmv_%s_launch_multi" % fmt)
        for minv in (None, px):
            args = (None, 1, px, 1, px, 1, minv, 30, 1e-8, 10, 0, None, 0,
                    info, None)
            assert solve(None, *args) == -errno.EINVAL
            assert solve(pj, *args) == dead
        args = (None, 1, px, 1, px, 1, pj, None, None, 30, 1e-8, 10, 0, None,
                0, info, None)
        assert trsv(None, *args) == -errno.EINVAL
        assert trsv(pj, *args) == dead     # the handle before the plans
        assert multi(None, None, 1, px, 1, px, 1, None) == -errno.EINVAL
        assert multi(pj, None, 1, px, 1, px, 1, None) == dead


@pytest.mark.parametrize("cls", [S.CsrDevice, S.HllDevice])
def test_the_wrapper_checks_its_arguments_before_anything_is_called(cls):
    fake = object.__new__(cls)  # a wrapper around no handle
    fake.h = None
    calls = []
    fake._call = lambda *a: calls.append(a)
    for kw in (dict(k=0), dict(k=9), dict(k=4, ldb=3), dict(k=4, ldx=2),
               dict(restart=0), dict(restart=65), dict(restart=-3)):
        with pytest.raises(ValueError):
            fake.gmres(1, 2, **kw)
    with pytest.raises(ValueError):
        fake.gmres_trsv(1, 2, object())        # not a TrsvPlan
    assert not calls
    # a good call reaches the library: k, B, ldb, X, ldx, minv, restart, tol,
    # maxit, check_every, work, work_bytes
    got = fake.gmres(1, 2, 4, restart=12, d_minv=3, tol=1e-6, maxit=17,
                     check_every=3, ldb=6)
    assert len(calls) == 1 and calls[0][0] == "gmres"
    assert calls[0][2:14] == (4, 1, 6, 2, 0, 3, 12, 1e-6, 17, 3, None, 0)
    assert type(calls[0][8]) is int and type(calls[0][9]) is float
    assert len(calls[0][14]) == 4  # k records for the library to fill
    assert got == [S.GmresResult(0, 0, 0, 0.0, 0.0, 0.0)] * 4
    fake.gmres(1, 2)  # one system, restart 30, no preconditioner
    assert calls[1][2] == 1 and calls[1][7:12] == (None, 30, 1e-8, 1000, 0)

    class Work:
        ptr, nbytes = 4096, 777
    fake.gmres(1, 2, 2, work=Work)
    assert calls[2][12:14] == (4096, 777)
    # the plans: first, second, d_scale, then restart
    plan = object.__new__(S.TrsvPlan)
    plan.h = 99
    fake.gmres_trsv(1, 2, plan, k=2, restart=9)
    assert calls[3][0] == "gmres_trsv"
    assert calls[3][7:11] == (99, None, None, 9)
    with pytest.raises(ValueError):
        fake.gmres_trsv(1, 2, plan, d_scale=5)  # a scale without a second
    with pytest.raises(ValueError):
        fake.gmres_trsv(1, 2, plan, restart=65)
    plan.h = None   # nothing for its finaliser to release


# ------------------------------------------------------ the restatement
def _solve(mat, restart, z=None, tol=TOL, maxit=200, B=None, X0=None, k=4,
           trace=None):
    M, IRP, JA, AS = mat
    if B is None:
        B, X0 = G.common_inputs(M, k)
    product, residual = GM.oracle_callables(mat, O.csr_spmv, B)
    s = GM.restate(product, residual, B, X0, restart, tol, maxit, z=z,
                   trace=trace)
    return s, G.true_residual(IRP, JA, AS, O.csr_spmv, B, s.X), B, X0


@pytest.mark.parametrize("name", list(SMALL))
def test_full_gmres_ends_within_M_steps(name):
    """restart = M never restarts: every column converges in at most M steps
    with a true residual of at most 2 tol ||b|| (the sanity line of
    test_gpu_cg)"""
    mat = SMALL[name]()
    M = mat[0]
    s, res, B, X0 = _solve(mat, M, maxit=M)
    print(name, s.iterations, res)
    assert s.status.tolist() == [0, 0, 0, 0]
    assert np.all(s.iterations <= M) and s.restarts.tolist() == [0] * 4
    assert np.all(res <= 2 * TOL), res
    # the zero column: converged at the start, X untouched
    assert s.iterations[1] == 0 and s.bb[1] == 0.0 and s.rr[1] == 0.0
    assert np.array_equal(bits(s.X[:, 1]), bits(X0[:, 1]))
    # est follows the true residual
    assert np.allclose(np.sqrt(s.est), np.sqrt(s.rr), rtol=0, atol=1e-12)


def _krylov_optimum(A, b, x0, j):
    """min ||b - A x|| over x in x0 + K_j(A, r0), by lstsq over an
    orthonormalised basis"""
    r0 = b - A @ x0
    K = np.empty((len(b), j))
    v = r0.copy()
    for i in range(j):
        K[:, i] = v / np.linalg.norm(v)
        v = A @ K[:, i]
    Q, _ = np.linalg.qr(K)
    y, *_ = np.linalg.lstsq(A @ Q, r0, rcond=None)
    return np.linalg.norm(r0 - A @ (Q @ y))


@pytest.mark.parametrize("name", list(SMALL))
def test_the_residual_is_the_optimum_over_the_krylov_space(name):
    """after j = 1..6 steps (no restart) the true residual norm is the lstsq
    optimum over an orthonormalised Krylov basis within 1e-6 ||b||, compared
    while both exceed 1e-4 ||b||.  On these matrices (condition below 1e2)
    rounding moves either side by orders of magnitude less: the restatement
    stays inside 2e-13 ||b|| here, printed below"""
    mat = SMALL[name]()
    M = mat[0]
    A = IL.dense_of(*mat)
    assert np.linalg.cond(A) < 1e2
    B, X0 = G.common_inputs(M, 4)
    worst, compared = 0.0, 0
    for j in range(1, 7):
        s, _, _, _ = _solve(mat, M, maxit=j, B=B, X0=X0)
        for col in (0, 2, 3):
            nb = np.linalg.norm(B[:, col])
            got = np.linalg.norm(B[:, col] - A @ s.X[:, col])
            want = _krylov_optimum(A, B[:, col], X0[:, col], j)
            if min(got, want) <= 1e-4 * nb:
                continue
            compared += 1
            worst = max(worst, abs(got - want) / nb)
            assert abs(got - want) <= 1e-6 * nb, (name, j, col, got, want)
    print(name, "compared", compared, "worst", worst)
    assert compared >= 12


@pytest.mark.parametrize("name", list(SMALL))
def test_two_steps_are_at_least_an_iteration_of_bicgstab(name):
    """x_j of BiCGStab lies in x0 + K_2j: GMRES after 2 j steps is no worse,
    with the slack of the test above"""
    mat = SMALL[name]()
    M, IRP, JA, AS = mat
    A = IL.dense_of(*mat)
    B, X0 = G.common_inputs(M, 4)
    product, residual0 = G.dense_product(IRP, JA, AS, O.csr_spmv)
    for j in range(1, 7):
        s, _, _, _ = _solve(mat, M, maxit=2 * j, B=B, X0=X0)
        b = BI.restate(product, residual0(B, X0), B, X0, None, TOL, j)
        for col in (0, 2, 3):
            nb = np.linalg.norm(B[:, col])
            gm = np.linalg.norm(B[:, col] - A @ s.X[:, col])
            bi = np.linalg.norm(B[:, col] - A @ b.X[:, col])
            assert gm <= bi + 1e-6 * nb, (name, j, col, gm, bi)


@pytest.mark.parametrize("restart", [1, 3, 30])
def test_est_never_grows_within_a_cycle(restart):
    mat = BI.convdiff(15, 17, 0.5, 0.5)
    trace = []
    s, res, _, _ = _solve(mat, restart, maxit=60, trace=trace)
    assert len(trace) >= 30
    seen = 0
    for (_, p, e0), (_, p1, e1) in zip(trace, trace[1:]):
        if p1 == p + 1:
            seen += 1
            assert np.all(e1 <= e0), (p, e0, e1)
    assert seen > 0 or restart == 1


# ------------------------------------------------------------ its own rules
def test_restart_one_restarts_after_every_step():
    mat = BI.convdiff(15, 17, 0.5, 0.5)
    s, _, _, X0 = _solve(mat, 1, maxit=5)
    assert s.status.tolist() == [1, 0, 1, 1]
    assert s.iterations.tolist() == [5, 0, 5, 5]
    assert s.restarts.tolist() == [5, 0, 5, 5]
    # to the end: the step that converges starts no new cycle
    s, res, _, _ = _solve(mat, 1, maxit=400)
    assert s.status.tolist() == [0, 0, 0, 0] and np.all(res <= 2 * TOL)
    for j in (0, 2, 3):
        assert s.restarts[j] in (s.iterations[j] - 1, s.iterations[j])


def test_maxit_in_mid_cycle_still_applies_its_steps():
    mat = BI.convdiff(15, 17, 0.5, 0.5)
    restart = 6
    at, res_at, B, X0 = _solve(mat, restart, maxit=restart)
    cut, res_cut, _, _ = _solve(mat, restart, maxit=restart + 2)
    assert cut.status.tolist() == [1, 0, 1, 1]
    assert cut.iterations.tolist() == [8, 0, 8, 8]
    assert cut.restarts.tolist() == [1, 0, 1, 1]
    for j in (0, 2, 3):
        assert not np.array_equal(bits(cut.X[:, j]), bits(at.X[:, j]))
        assert res_cut[j] < res_at[j]
    # the estimate of the two steps is the residual they reached
    assert np.allclose(np.sqrt(cut.est), np.sqrt(cut.rr), rtol=1e-9, atol=0)
    assert np.array_equal(bits(cut.X[:, 1]), bits(X0[:, 1]))


def test_a_nan_in_minv_is_a_breakdown():
    mat = BI.convdiff(15, 17, 0.5, 0.5)
    M = mat[0]
    d = np.ones(M)
    d[9] = np.nan
    s, _, _, X0 = _solve(mat, 5, z=lambda U: d[:, None] * U)
    assert s.status.tolist() == [2, 0, 2, 2]
    assert s.iterations.tolist() == [0, 0, 0, 0]
    assert np.array_equal(bits(s.X), bits(X0))
    # ones: the bits of none
    none, _, _, _ = _solve(mat, 5)
    ones, _, _, _ = _solve(mat, 5, z=lambda U: np.ones((M, 1)) * U)
    for f in GM.Solve._fields:
        assert np.array_equal(getattr(ones, f), getattr(none, f)), f


def test_a_matrix_of_stored_zeros_is_a_breakdown_with_x_untouched():
    M, IRP, JA, AS = BI.convdiff(15, 17, 0.5, 0.5)
    s, _, _, X0 = _solve((M, IRP, JA, np.zeros_like(AS)), 5)
    assert s.status.tolist() == [2, 0, 2, 2]
    assert s.iterations.tolist() == [0, 0, 0, 0]
    assert s.restarts.tolist() == [0, 0, 0, 0]
    assert np.array_equal(bits(s.X), bits(X0))


def test_a_nonfinite_right_hand_side_stops_its_own_column_only():
    mat = BI.convdiff(15, 17, 0.5, 0.5)
    B, X0 = G.common_inputs(mat[0])
    clean, _, _, _ = _solve(mat, 5, B=B, X0=X0)
    Bi = B.copy()
    Bi[7, 0] = np.inf
    s, _, _, _ = _solve(mat, 5, B=Bi, X0=X0)
    assert s.status.tolist() == [2, 0, 0, 0] and s.iterations[0] == 0
    assert np.array_equal(bits(s.X[:, 0]), bits(X0[:, 0]))
    assert np.array_equal(bits(s.X[:, 1:]), bits(clean.X[:, 1:]))
    assert s.iterations[1:].tolist() == clean.iterations[1:].tolist()
    assert np.array_equal(bits(s.est[1:]), bits(clean.est[1:]))
