"""BiCGStab on the device (spmv_*_bicgstab, spmv_bicgstab_work_bytes;
spmv_engine.h): what can be checked without a GPU -- the declared surface, the
ctypes signatures, the dead-handle answers, the argument checks of the Python
wrapper, and the numpy restatement of the solver (tests/_bicgstab.py) run with
the CPU oracle's product: that the loop of the contract solves nonsymmetric
systems, what Jacobi buys on row-scaled ones, and the edge rules.  The kernels
themselves: tests/test_gpu_bicgstab.py."""
import ctypes as C
import errno

import numpy as np
import pytest

import _bicgstab as BI
import _cg as G
import _oracle as O
import _pcg as PG
import spmv_scpa_amd as S

NEW = ["spmv_csr_bicgstab", "spmv_hll_bicgstab", "spmv_bicgstab_work_bytes"]
TOL = 1e-8


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_the_headers_declare_the_bicgstab_entry_points():
    declared = S.declared_symbols()
    for name in NEW:
        assert name in declared, name
        assert hasattr(S._lib, name), name
    assert S.check_symbols()
    # the feature is detected by the symbol, not by the version string
    assert S.version() == "spmv_scpa_amd 0.7 gfx950"


def test_the_twin_signature_comes_from_the_shared_list():
    names = [t[0] for t in S._TWINS]
    assert names.count("bicgstab") == 1
    for fmt in ("csr", "hll"):
        fn = getattr(S._lib, "spmv_%s_bicgstab" % fmt)
        assert fn.restype is C.c_int
        assert fn.argtypes == [C.c_void_p, C.POINTER(S.LaunchOpts), C.c_int,
                               C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                               C.c_void_p, C.c_double, C.c_int, C.c_int,
                               C.c_void_p, C.c_size_t, C.POINTER(S.CgInfo),
                               C.c_void_p]
    assert S._lib.spmv_bicgstab_work_bytes.restype is C.c_int64
    assert S._lib.spmv_bicgstab_work_bytes.argtypes == [C.c_int, C.c_int]


def test_work_bytes_answers_its_errors_and_grows_with_the_vectors():
    einval = -errno.EINVAL
    assert S._lib.spmv_bicgstab_work_bytes(-1, 1) == einval
    for k in (0, 9, -1):
        assert S._lib.spmv_bicgstab_work_bytes(10, k) == einval
        with pytest.raises(OSError) as ei:
            S.bicgstab_work_bytes(10, k)
        assert ei.value.errno == errno.EINVAL
    base = S.bicgstab_work_bytes(0, 1)
    assert base > 0 and base % 8 == 0
    for k in range(1, 9):
        assert S.bicgstab_work_bytes(0, k) == base
        # six vectors of M x k doubles: R, Rh, P, V, T, Z
        assert S.bicgstab_work_bytes(1000, k) == base + 6 * 8 * 1000 * k
    # no 32-bit overflow
    assert S.bicgstab_work_bytes(2**31 - 1, 8) == \
        base + 6 * 8 * (2**31 - 1) * 8


def test_dead_handles_are_refused():
    x = C.create_string_buffer(64)
    px = C.cast(x, C.c_void_p)
    junk = C.create_string_buffer(512)  # never a handle of the library
    pj = C.cast(junk, C.c_void_p)
    info = (S.CgInfo * 8)()
    dead = -errno.EBADF if S.device_count() > 0 else -errno.ENODEV
    for fmt in ("csr", "hll"):
        solve = getattr(S._lib, "spmv_%s_bicgstab" % fmt)
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
            fake.bicgstab(1, 2, **kw)
    assert not calls
    # a good call does reach the library: k, B, ldb, X, ldx, minv, tol, maxit,
    # check_every, work, work_bytes
    got = fake.bicgstab(1, 2, 4, d_minv=3, tol=1e-6, maxit=17, check_every=3,
                        ldb=6)
    assert len(calls) == 1 and calls[0][0] == "bicgstab"
    assert calls[0][2:13] == (4, 1, 6, 2, 0, 3, 1e-6, 17, 3, None, 0)
    assert type(calls[0][8]) is float
    assert len(calls[0][13]) == 4  # k records for the library to fill
    assert got == [S.CgResult(0, 0, 0.0, 0.0)] * 4
    fake.bicgstab(1, 2)  # one system, no preconditioner, the defaults
    assert calls[1][2] == 1 and calls[1][7:11] == (None, 1e-8, 1000, 0)

    class Work:
        ptr, nbytes = 4096, 777
    fake.bicgstab(1, 2, 2, work=Work)
    assert calls[2][11:13] == (4096, 777)


# ------------------------------------------------------ the restatement
def _solve(mat, minv=None, tol=TOL, maxit=200, B=None, X0=None, k=4):
    M, IRP, JA, AS = mat
    if B is None:
        B, X0 = G.common_inputs(M, k)
    product, residual0 = G.dense_product(IRP, JA, AS, O.csr_spmv)
    s = BI.restate(product, residual0(B, X0), B, X0, minv, tol, maxit)
    return s, G.true_residual(IRP, JA, AS, O.csr_spmv, B, s.X), B, X0


MATRICES = {
    "convdiff(15,17,.5,.5)": lambda: BI.convdiff(15, 17, 0.5, 0.5),
    "convdiff(37,29,.5,.5)": lambda: BI.convdiff(37, 29, 0.5, 0.5),
    "arrow2(2051,3)": lambda: BI.arrow2(2051, 3),
    "arrow2(4099,3)": lambda: BI.arrow2(4099, 3),
}


@pytest.mark.parametrize("name", list(MATRICES))
def test_the_restatement_solves_the_test_matrices(name):
    mat = MATRICES[name]()
    s, res, B, X0 = _solve(mat)
    assert s.status.tolist() == [0, 0, 0, 0], name
    print(name, "iterations", s.iterations, "true residual", res)
    assert np.all(res <= TOL), (name, res)
    # the zero column: converged before the first iteration, X untouched
    assert s.iterations[1] == 0 and s.bb[1] == 0.0 and s.rr[1] == 0.0
    assert np.array_equal(bits(s.X[:, 1]), bits(X0[:, 1]))
    assert np.all(s.iterations[[0, 2, 3]] > 0)
    if name == "convdiff(37,29,.5,.5)":
        assert s.iterations.tolist() == [32, 0, 33, 30]
    # stopped early, a column keeps what it had: maxit = 3
    s3, _, _, _ = _solve(mat, maxit=3)
    assert s3.status.tolist() == [1, 0, 1, 1], name
    assert s3.iterations.tolist() == [3, 0, 3, 3], name


def test_the_generators_give_the_stated_nonsymmetric_matrices():
    def dense(mat):
        M, IRP, JA, AS = mat
        D = np.zeros((M, M))
        for r in range(M):
            assert np.all(np.diff(JA[IRP[r]:IRP[r + 1]]) > 0)  # sorted columns
            D[r, JA[IRP[r]:IRP[r + 1]]] = AS[IRP[r]:IRP[r + 1]]
        return D
    D = dense(BI.convdiff(5, 4, 0.5, 0.25))
    assert D.shape == (20, 20) and np.all(np.diag(D) == 4.5)
    assert D[6, 7] == -0.75 and D[6, 5] == -1.25       # east, west
    assert D[6, 1] == -1.0 and D[6, 11] == -1.0        # south, north
    assert D[4, 5] == 0.0 and D[5, 4] == 0.0           # no wrap between lines
    assert np.count_nonzero(D) == 20 + 2 * (4 * 4 + 5 * 3)
    D = dense(BI.arrow2(40, 3))
    assert not np.array_equal(D, D.T)
    assert np.all(D[0, 1:] != 0) and np.all(D[1:, 0] != 0)
    off = np.abs(D).sum(axis=1) - np.abs(np.diag(D))
    assert np.all(np.diag(D) > off)                    # row diagonal dominance
    assert np.count_nonzero(D) == 3 * 40 - 2
    M, IRP, JA, AS = BI.arrow2(2051, 3)
    assert IRP[1] == 2051 > 2048      # the CSR long-row kernel, a wide block
    base = BI.convdiff(5, 4, 0.5, 0.25)
    scaled = BI.rowscale(base, 5)
    f = 2.0 ** np.random.default_rng(5).uniform(0, 6, 20)
    assert np.all((1.0 <= f) & (f <= 64.0)) and f.max() > 4 * f.min()
    assert np.array_equal(dense(scaled), dense(base) * f[:, None])
    D = dense(BI.skew2(6))
    assert np.array_equal(D, -D.T) and D[0, 1] == 1.0 and D[1, 0] == -1.0
    assert np.count_nonzero(D) == 6
    assert np.array_equal(dense(BI.diagm([1.0, 2.0, 3.0])),
                          np.diag([1.0, 2.0, 3.0]))


@pytest.mark.parametrize("name", ["convdiff(15,17,.5,.5)",
                                  "convdiff(37,29,.5,.5)"])
def test_jacobi_undoes_a_row_scaling(name):
    mat = BI.rowscale(MATRICES[name](), 5)
    minv = 1.0 / PG.diag_of(*mat)
    plain, res0, _, _ = _solve(mat, maxit=400)
    pre, res1, _, _ = _solve(mat, minv=minv, maxit=400)
    print(name, "iterations: jacobi", pre.iterations, "none", plain.iterations)
    assert plain.status.tolist() == [0, 0, 0, 0]
    assert pre.status.tolist() == [0, 0, 0, 0]
    assert np.all(res0 <= TOL) and np.all(res1 <= TOL), (res0, res1)
    for j in (0, 2, 3):
        assert 0 < pre.iterations[j] < plain.iterations[j], (name, j)
    assert pre.iterations[1] == 0 and plain.iterations[1] == 0


# ------------------------------------------------------------ the edge rules
def _edge(mat, B, minv=None, maxit=200):
    M = mat[0]
    return _solve(mat, minv=minv, maxit=maxit, B=B, X0=np.zeros((M, 2)))


def test_an_identity_is_solved_by_the_tt_equals_zero_rule():
    B = np.random.default_rng(2).uniform(-1, 1, (70, 2))
    s, _, _, X0 = _edge(BI.diagm(np.ones(70)), B)
    # S = R - 1 * R = 0 exactly: tt = 0, omega = 0, R = 0
    assert s.status.tolist() == [0, 0]
    assert s.iterations.tolist() == [1, 1]
    assert s.rr.tolist() == [0.0, 0.0]
    assert np.array_equal(bits(s.X), bits(B))


def test_rv_equal_to_zero_is_a_breakdown_before_the_first_step():
    B = np.random.default_rng(2).uniform(-1, 1, (70, 2))
    B[1::2] = 0.0
    s, _, _, X0 = _edge(BI.skew2(70), B)
    assert s.status.tolist() == [2, 2]
    assert s.iterations.tolist() == [0, 0]
    assert np.array_equal(bits(s.X), bits(X0))


def test_an_overflowing_tt_is_a_breakdown_before_the_first_step():
    v = np.ones(70)
    v[1::2] = 1e200
    s, _, _, X0 = _edge(BI.diagm(v), np.ones((70, 2)))
    assert s.status.tolist() == [2, 2]
    assert s.iterations.tolist() == [0, 0]
    assert np.array_equal(bits(s.X), bits(X0))


def test_a_nonfinite_right_hand_side_stops_its_own_column_only():
    mat = BI.convdiff(15, 17, 0.5, 0.5)
    B, X0 = G.common_inputs(mat[0])
    clean, _, _, _ = _solve(mat, B=B, X0=X0)
    Bi = B.copy()
    Bi[7, 0] = np.inf
    s, _, _, _ = _solve(mat, B=Bi, X0=X0)
    assert s.status.tolist() == [2, 0, 0, 0]
    assert s.iterations[0] == 0
    assert np.array_equal(bits(s.X[:, 0]), bits(X0[:, 0]))
    assert np.array_equal(bits(s.X[:, 1:]), bits(clean.X[:, 1:]))
    assert s.iterations[1:].tolist() == clean.iterations[1:].tolist()
    assert np.array_equal(bits(s.rr[1:]), bits(clean.rr[1:]))


@pytest.mark.parametrize("name", ["convdiff(37,29,.5,.5)", "arrow2(2051,3)"])
def test_a_preconditioner_of_ones_has_the_bits_of_none(name):
    mat = MATRICES[name]()
    for maxit in (200, 3):
        none, _, _, _ = _solve(mat, maxit=maxit)
        ones, _, _, _ = _solve(mat, minv=np.ones(mat[0]), maxit=maxit)
        assert np.array_equal(bits(ones.X), bits(none.X))
        assert ones.status.tolist() == none.status.tolist()
        assert ones.iterations.tolist() == none.iterations.tolist()
        assert np.array_equal(bits(ones.rr), bits(none.rr))
        assert np.array_equal(bits(ones.bb), bits(none.bb))
