"""MINRES on the device (spmv_*_minres, spmv_minres_work_bytes,
spmv_debug_sqrt; spmv_engine.h): what can be checked without a GPU -- the
declared surface, the ctypes signatures, the dead-handle answers, the argument
checks of the Python wrapper, and the numpy restatement of the solver
(tests/_minres.py) run with a dense numpy product: that the loop of the
contract solves symmetric indefinite systems on which CG breaks down, and the
edge rules.  The kernels themselves: tests/test_gpu_minres.py."""
import ctypes as C
import errno

import numpy as np
import pytest

import _cg as G
import _minres as MR
import spmv_scpa_amd as S

NEW = ["spmv_csr_minres", "spmv_hll_minres", "spmv_minres_work_bytes",
       "spmv_debug_sqrt"]
TOL = 1e-8


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_the_headers_declare_the_minres_entry_points():
    declared = S.declared_symbols()
    for name in NEW:
        assert name in declared, name
        assert hasattr(S._lib, name), name
    assert S.check_symbols()
    # the feature is detected by the symbol, not by the version string
    assert S.version() == "spmv_scpa_amd 0.7 gfx950"


def test_the_twin_signature_comes_from_the_shared_list():
    names = [t[0] for t in S._TWINS]
    assert names.count("minres") == 1
    for fmt in ("csr", "hll"):
        fn = getattr(S._lib, "spmv_%s_minres" % fmt)
        assert fn.restype is C.c_int
        assert fn.argtypes == [C.c_void_p, C.POINTER(S.LaunchOpts), C.c_int,
                               C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                               C.c_void_p, C.c_double, C.c_int, C.c_int,
                               C.c_void_p, C.c_size_t,
                               C.POINTER(S.MinresInfo), C.c_void_p]
    assert S._lib.spmv_minres_work_bytes.restype is C.c_int64
    assert S._lib.spmv_minres_work_bytes.argtypes == [C.c_int, C.c_int]
    assert S._lib.spmv_debug_sqrt.restype is C.c_int
    assert S._lib.spmv_debug_sqrt.argtypes == [C.c_void_p, C.c_void_p,
                                               C.c_int64, C.c_void_p]
    # the record: two ints and four doubles, as the header lays them out
    assert [f[0] for f in S.MinresInfo._fields_] == \
        ["status", "iterations", "pp", "bn2", "rr", "bb"]
    assert C.sizeof(S.MinresInfo) == 40
    assert S.MinresResult._fields == ("status", "iterations", "pp", "bn2",
                                      "rr", "bb")


def test_work_bytes_answers_its_errors_and_grows_with_the_vectors():
    einval = -errno.EINVAL
    assert S._lib.spmv_minres_work_bytes(-1, 1) == einval
    for k in (0, 9, -1):
        assert S._lib.spmv_minres_work_bytes(10, k) == einval
        with pytest.raises(OSError) as ei:
            S.minres_work_bytes(10, k)
        assert ei.value.errno == errno.EINVAL
    base = S.minres_work_bytes(0, 1)
    assert base > 0 and base % 8 == 0
    for k in range(1, 9):
        assert S.minres_work_bytes(0, k) == base
        # six vectors of M x k doubles: two residuals, V, Q, two directions
        assert S.minres_work_bytes(1000, k) == base + 6 * 8 * 1000 * k
        assert S.minres_work_bytes(1, k) == base + 6 * 8 * k
    # no 32-bit overflow
    assert S.minres_work_bytes(2**31 - 1, 8) == base + 6 * 8 * (2**31 - 1) * 8


def test_the_sqrt_hook_checks_its_arguments_before_the_device():
    x = C.create_string_buffer(64)
    px = C.cast(x, C.c_void_p)
    assert S._lib.spmv_debug_sqrt(px, px, -1, None) == -errno.EINVAL
    assert S._lib.spmv_debug_sqrt(None, px, 1, None) == -errno.EINVAL
    assert S._lib.spmv_debug_sqrt(px, None, 1, None) == -errno.EINVAL
    assert S._lib.spmv_debug_sqrt(None, None, 0, None) == 0


def test_dead_handles_are_refused():
    x = C.create_string_buffer(64)
    px = C.cast(x, C.c_void_p)
    junk = C.create_string_buffer(512)  # never a handle of the library
    pj = C.cast(junk, C.c_void_p)
    info = (S.MinresInfo * 8)()
    dead = -errno.EBADF if S.device_count() > 0 else -errno.ENODEV
    for fmt in ("csr", "hll"):
        solve = getattr(S._lib, "spmv_%s_minres" % fmt)
        multi = getattr(S._lib, "spmv_%s_launch_multi" % fmt)
        for minv in (None, px):
            args = (None, 1, px, 1, px, 1, minv, 1e-8, 10, 0, None, 0, info,
                    None)
            assert solve(None, *args) == -errno.EINVAL
            assert solve(pj, *args) == dead
        # one function checks the handle for both: the same answers
        assert multi(None, None, 1, px, 1, px, 1, None) == -errno.EINVAL
        assert multi(pj, None, 1, px, 1, px, 1, None) == dead


@pytest.mark.parametrize("cls", [S.CsrDevice, S.HllDevice])
def test_the_wrapper_checks_k_and_the_strides_before_anything_is_called(cls):
    fake = object.__new__(cls)  # a wrapper around no handle
    fake.h = None
    calls = []
    fake._call = lambda *a: calls.append(a)
    for kw in (dict(k=0), dict(k=9), dict(k=-1), dict(k=4, ldb=3),
               dict(k=4, ldx=2), dict(k=8, ldb=7, ldx=8)):
        with pytest.raises(ValueError):
            fake.minres(1, 2, **kw)
    assert not calls
    # a good call does reach the library: k, B, ldb, X, ldx, minv, tol, maxit,
    # check_every, work, work_bytes
    got = fake.minres(1, 2, 4, d_minv=3, tol=1e-6, maxit=17, check_every=3,
                      ldb=6)
    assert len(calls) == 1 and calls[0][0] == "minres"
    assert calls[0][2:13] == (4, 1, 6, 2, 0, 3, 1e-6, 17, 3, None, 0)
    assert type(calls[0][8]) is float
    assert len(calls[0][13]) == 4  # k records for the library to fill
    assert isinstance(calls[0][13][0], S.MinresInfo)
    assert got == [S.MinresResult(0, 0, 0.0, 0.0, 0.0, 0.0)] * 4
    fake.minres(1, 2)  # one system, no preconditioner, the defaults
    assert calls[1][2] == 1 and calls[1][7:11] == (None, 1e-8, 1000, 0)

    class Work:
        ptr, nbytes = 4096, 777
    fake.minres(1, 2, 2, work=Work)
    assert calls[2][11:13] == (4096, 777)
    # the helper still serves the other solvers with their record
    fake.bicgstab(1, 2, 2)
    assert isinstance(calls[3][13][0], S.CgInfo)


# ------------------------------------------------------ the restatement
def _solve(mat, minv=None, tol=TOL, maxit=2000, B=None, X0=None, k=4):
    """restate() with the dense numpy product -> (Solve, true relative
    residual in the 2-norm, B, X0, the dense matrix)"""
    M = mat[0]
    A = MR.dense(mat)
    if B is None:
        B, X0 = G.common_inputs(M, k)
    def product(V):   # column by column: a column's product is its own
        return np.stack([A @ V[:, j] for j in range(V.shape[1])], axis=1)
    s = MR.restate(product, lambda: -1.0 * product(X0) + 1.0 * B, B, X0,
                   minv, tol, maxit)
    with np.errstate(all="ignore"):
        r = np.linalg.norm(B - A @ s.X, axis=0)
        b = np.linalg.norm(B, axis=0)
        res = np.where(b > 0, r / np.where(b > 0, b, 1.0), r)
    return s, res, B, X0, A


def _cg_status(A, B, X0, maxit=2000):
    return G.restate(lambda P: A @ P, lambda: -1.0 * (A @ X0) + 1.0 * B, B,
                     X0, TOL, maxit).status.tolist()


def _jacobi(mat):
    return 1.0 / MR.dense(mat).diagonal()


#: name -> (matrix, minv or None, negative eigenvalues at least): the
#: convergence inputs
INPUTS = {
    "shifted_lap1d(1000,1.0)": lambda: (MR.shifted_lap1d(1000, 1.0), None),
    "shifted_lap2d(37,29,1.3)": lambda: (MR.shifted_lap2d(37, 29, 1.3), None),
    "saddle(200,60,7)": lambda: (MR.saddle(200, 60, 7), None),
    "saddle(200,60,7) 1/|d|": lambda: (
        MR.saddle(200, 60, 7), MR.abs_inverse_diag(MR.saddle(200, 60, 7))),
    "sym_arrow(300,3)": lambda: (MR.sym_arrow(300, 3), None),
    "symscale lap2d(11,13,1.3) jacobi": lambda: (
        MR.symscale(MR.shifted_lap2d(11, 13, 1.3), 5),
        _jacobi(MR.symscale(MR.shifted_lap2d(11, 13, 1.3), 5))),
}


@pytest.mark.parametrize("name", list(INPUTS))
def test_the_restatement_solves_the_indefinite_inputs_and_cg_does_not(name):
    mat, minv = INPUTS[name]()
    s, res, B, X0, A = _solve(mat, minv)
    # a condition on the inputs: symmetric, indefinite, no eigenvalue near 0
    # (of the matrix Jacobi sees, where there is one)
    assert np.array_equal(A, A.T)
    if minv is None:
        ev = np.linalg.eigvalsh(A)
    else:
        assert np.all(minv > 0)
        h = np.sqrt(minv)
        ev = np.linalg.eigvalsh(h[:, None] * A * h[None, :])
    print(name, "eigenvalues < 0:", int((ev < 0).sum()), "smallest |ev|",
          np.abs(ev).min(), "of", np.abs(ev).max())
    assert (ev < 0).any() and (ev > 0).any()
    # condition number at most 1e4: what rounding can cost the residual,
    # about cond * 2**-53 = 1e-12, stays four digits below tol
    assert np.abs(ev).min() > 1e-4 * np.abs(ev).max()
    print(name, "iterations", s.iterations, "true residual", res, "estimate",
          np.sqrt(s.pp / np.where(s.bn2 > 0, s.bn2, 1.0)))
    assert s.status.tolist() == [0, 0, 0, 0], name
    assert np.all(res <= 10 * TOL), (name, res)
    # the closing rr / bb are the true figure
    with np.errstate(invalid="ignore"):
        true = np.sqrt(s.rr / np.where(s.bb > 0, s.bb, 1.0))
    # (two roundings of b - A x differ by about cond * 2**-53 <= 1e-12)
    assert np.allclose(true, res, rtol=1e-6, atol=1e-12), (true, res)
    if minv is None:   # estimate and true residual agree (2-norm: same norm)
        est = np.sqrt(s.pp / np.where(s.bn2 > 0, s.bn2, 1.0))
        assert np.allclose(est, res, rtol=1e-2, atol=0), (est, res)
        assert np.array_equal(bits(s.bn2), bits(s.bb))
    # the zero column: converged before the first iteration, X untouched
    assert s.iterations[1] == 0 and s.bb[1] == 0.0 and s.rr[1] == 0.0
    assert s.pp[1] == 0.0
    assert np.array_equal(bits(s.X[:, 1]), bits(X0[:, 1]))
    assert np.all(s.iterations[[0, 2, 3]] > 0)
    # CG on the same inputs: p.Ap <= 0 sooner or later
    assert _cg_status(A, B, X0) == [2, 0, 2, 2], name
    # stopped early, a column keeps what it had: maxit = 3
    s3 = _solve(mat, minv, maxit=3)[0]
    assert s3.status.tolist() == [1, 0, 1, 1], name
    assert s3.iterations.tolist() == [3, 0, 3, 3], name
    # ... and the estimate never grows
    pps = [_solve(mat, minv, maxit=n)[0].pp for n in range(6)]
    assert all(np.all(b <= a) for a, b in zip(pps, pps[1:])), pps


def test_shifted_lap1d_257_is_singular_and_is_not_an_input():
    ev = np.linalg.eigvalsh(MR.dense(MR.shifted_lap1d(257, 1.0)))
    assert np.abs(ev).min() < 1e-12
    assert not any("257" in n for n in INPUTS)


def test_the_generators_give_the_stated_symmetric_matrices():
    D = MR.dense(MR.shifted_lap1d(6, 0.75))
    assert np.array_equal(D, D.T) and np.all(np.diag(D) == 1.25)
    assert np.all(np.diag(D, 1) == -1.0) and np.count_nonzero(D) == 16
    D = MR.dense(MR.shifted_lap2d(5, 4, 1.5))
    assert np.array_equal(D, D.T) and np.all(np.diag(D) == 2.5)
    assert D[6, 7] == -1.0 and D[6, 1] == -1.0 and D[4, 5] == 0.0
    n, m = 30, 9
    mat = MR.saddle(n, m, 7)
    M, IRP, JA, AS = mat
    D = MR.dense(mat)
    assert M == n + m and np.array_equal(D, D.T)
    assert np.all(D[n:, n:] == 0.0)
    rows = np.repeat(np.arange(M), np.diff(IRP))
    assert not np.any((rows == JA) & (rows >= n))      # no stored diagonal
    assert np.all(np.linalg.eigvalsh(D[:n, :n]) > 0)   # K is SPD
    assert np.linalg.matrix_rank(D[n:, :n]) == m       # C: full row rank
    ev = np.linalg.eigvalsh(D)
    assert (ev < 0).sum() == m and (ev > 0).sum() == n
    minv = MR.abs_inverse_diag(mat)
    assert np.all(minv[:n] == 1.0 / 2.5) and np.all(minv[n:] == 1.0)
    D = MR.dense(MR.sym_arrow(40, 3))
    assert np.array_equal(D, D.T) and D[0, 0] < 0 and np.all(np.diag(D)[1:] > 0)
    assert np.all(D[0, 1:] != 0) and np.count_nonzero(D) == 3 * 40 - 2
    ev = np.linalg.eigvalsh(D)
    assert (ev < 0).sum() == 1
    M, IRP, JA, AS = MR.sym_arrow(2051, 3)
    assert IRP[1] == 2051 > 2048      # the CSR long-row kernel, a wide block
    base = MR.shifted_lap2d(5, 4, 1.5)
    f = 2.0 ** np.random.default_rng(5).uniform(0, 6, 20)
    assert np.all((1.0 <= f) & (f <= 64.0)) and f.max() > 4 * f.min()
    D = MR.dense(MR.symscale(base, 5))
    assert np.array_equal(D, MR.dense(base) * f[:, None] * f[None, :])
    assert np.array_equal(D, D.T)
    assert np.array_equal(MR.dense(MR.diagm([1.0, -2.0, 3.0])),
                          np.diag([1.0, -2.0, 3.0]))


def test_jacobi_undoes_a_symmetric_scaling():
    mat = MR.symscale(MR.shifted_lap2d(11, 13, 1.3), 5)
    plain = _solve(mat, maxit=4000)[0]
    pre = _solve(mat, _jacobi(mat), maxit=4000)[0]
    print("iterations: jacobi", pre.iterations, "none", plain.iterations)
    assert plain.status.tolist() == [0, 0, 0, 0]
    assert pre.status.tolist() == [0, 0, 0, 0]
    for j in (0, 2, 3):
        assert 0 < pre.iterations[j] < plain.iterations[j], j


# ------------------------------------------------------------ the edge rules
def same(a, b):
    assert np.array_equal(bits(a.X), bits(b.X))
    assert a.status.tolist() == b.status.tolist()
    assert a.iterations.tolist() == b.iterations.tolist()
    for f in ("pp", "bn2", "rr", "bb"):
        assert np.array_equal(bits(getattr(a, f)), bits(getattr(b, f))), f


@pytest.mark.parametrize("name", ["shifted_lap2d(37,29,1.3)",
                                  "sym_arrow(300,3)"])
def test_a_preconditioner_of_ones_has_the_bits_of_none(name):
    mat = INPUTS[name]()[0]
    for maxit in (2000, 3):
        none = _solve(mat, maxit=maxit)[0]
        ones = _solve(mat, np.ones(mat[0]), maxit=maxit)[0]
        same(ones, none)


def test_a_column_is_its_own_solve_whatever_the_others_do():
    mat = MR.saddle(200, 60, 7)
    M = mat[0]
    B, X0 = G.common_inputs(M)
    B[:, 2] = np.nan                      # a NaN column: status 2 at once
    s = _solve(mat, B=B, X0=X0)[0]
    assert s.status.tolist() == [0, 0, 2, 0]
    assert s.iterations[2] == 0
    assert np.array_equal(bits(s.X[:, 2]), bits(X0[:, 2]))
    # the two that run stop at different steps
    assert 0 < s.iterations[0] != s.iterations[3] > 0
    for j in range(4):
        one = _solve(mat, B=B[:, j:j + 1], X0=X0[:, j:j + 1])[0]
        col = MR.Solve(s.X[:, j:j + 1], s.status[j:j + 1],
                       s.iterations[j:j + 1], s.pp[j:j + 1], s.bn2[j:j + 1],
                       s.rr[j:j + 1], s.bb[j:j + 1])
        same(one, col)


def test_a_frozen_column_keeps_what_it_had():
    mat = MR.shifted_lap2d(15, 17, 1.3)
    M = mat[0]
    B, X0 = G.common_inputs(M)
    loose = _solve(mat, tol=1e-2, maxit=400)[0]
    assert loose.status.tolist() == [0, 0, 0, 0]
    n = loose.iterations
    assert 0 < n[[0, 2, 3]].min() < n.max()
    # the same columns cut off by maxit at their own count: the same X
    for j in (0, 2, 3):
        cut = _solve(mat, tol=0.0, maxit=int(n[j]), B=B[:, j:j + 1],
                     X0=X0[:, j:j + 1])[0]
        assert cut.status.tolist() == [1] and cut.iterations.tolist() == [n[j]]
        assert np.array_equal(bits(cut.X[:, 0]), bits(loose.X[:, j]))
        assert np.array_equal(bits(cut.pp), bits(loose.pp[j:j + 1]))


@pytest.mark.parametrize("p", [1, 2, 3, 5])
def test_p_distinct_eigenvalues_of_mixed_sign_take_at_most_p_iterations(p):
    ev = np.array([3.0, -2.0, 0.5, -7.0, 11.0])[:p]
    M = 60
    d = np.resize(ev, M)
    B = np.random.default_rng(4).uniform(-1, 1, (M, 2))
    s, res, _, _, _ = _solve(MR.diagm(d), B=B, X0=np.zeros((M, 2)), maxit=50)
    print(p, s.iterations, res)
    assert s.status.tolist() == [0, 0]
    assert np.all(s.iterations <= p) and np.all(s.iterations >= 1)
    assert np.all(res <= 10 * TOL)
    if p >= 2:   # indefinite: CG breaks down, or its residual goes up first
        assert (d < 0).any()


def test_breakdowns_are_statuses():
    M = 70
    X0 = np.zeros((M, 2))
    B = np.random.default_rng(2).uniform(-1, 1, (M, 2))
    lap = MR.shifted_lap1d(M, 0.9)
    for tag, mat, Bt, minv in (
            ("negative minv", lap, B, np.full(M, -1.0)),
            ("inf in minv", lap, B, np.where(np.arange(M) == 9, np.inf, 1.0)),
            ("stored zeros", MR.diagm(np.zeros(M)), B, None),
            ("inf column", lap, np.where(np.arange(M)[:, None] == 7, np.inf, B),
             None)):
        s = _solve(mat, minv, B=Bt, X0=X0, maxit=50)[0]
        assert s.status.tolist() == [2, 2], tag
        assert s.iterations.tolist() == [0, 0], tag
        assert np.array_equal(bits(s.X), bits(X0)), tag
    # B = 0: converged at once whatever tol, tol = 0 included
    s = _solve(lap, B=np.zeros((M, 2)), X0=X0, tol=0.0)[0]
    assert s.status.tolist() == [0, 0] and s.iterations.tolist() == [0, 0]
    # maxit = 0: running columns answer 1 with X untouched and rr = b1
    s = _solve(lap, B=B, X0=X0, maxit=0)[0]
    assert s.status.tolist() == [1, 1] and s.iterations.tolist() == [0, 0]
    assert np.array_equal(bits(s.rr), bits(s.pp))
    assert np.array_equal(bits(s.X), bits(X0))
