"""Conjugate gradients on the device (spmv_*_cg, spmv_cg_work_bytes;
spmv_engine.h): what can be checked without a GPU -- the declared surface, the
ctypes signatures, the dead-handle answers, the argument checks of the Python
wrapper, and the numpy restatement of the solver (tests/_cg.py) run with the
CPU oracle's product.  The kernels themselves: tests/test_gpu_cg.py."""
import ctypes as C
import errno

import numpy as np
import pytest

import _cg as G
import _oracle as O
import spmv_scpa_amd as S

NEW = ["spmv_csr_cg", "spmv_hll_cg", "spmv_cg_work_bytes", "spmv_cg_dot_shape"]
TOL = 1e-8


def test_the_headers_declare_the_cg_entry_points():
    declared = S.declared_symbols()
    for name in NEW:
        assert name in declared, name
        assert hasattr(S._lib, name), name
    assert S.check_symbols()
    # the feature is detected by the symbol, not by the version string
    assert S.version() == "spmv_scpa_amd 0.7 gfx950"


def test_the_twin_signature_comes_from_the_shared_list():
    names = [t[0] for t in S._TWINS]
    assert names.count("cg") == 1
    for fmt in ("csr", "hll"):
        fn = getattr(S._lib, "spmv_%s_cg" % fmt)
        assert fn.restype is C.c_int
        assert fn.argtypes == [C.c_void_p, C.POINTER(S.LaunchOpts), C.c_int,
                               C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                               C.c_double, C.c_int, C.c_int, C.c_void_p,
                               C.c_size_t, C.POINTER(S.CgInfo), C.c_void_p]
    assert S._lib.spmv_cg_work_bytes.restype is C.c_int64
    assert S._lib.spmv_cg_work_bytes.argtypes == [C.c_int, C.c_int]
    # spmv_cg_info: two ints and two doubles, no padding
    assert C.sizeof(S.CgInfo) == 24
    assert [f[0] for f in S.CgInfo._fields_] == ["status", "iterations", "rr",
                                                 "bb"]


def test_the_dot_shape_is_exported_and_two_powers_of_two():
    nwg, t = S.CG_DOT_SHAPE
    assert nwg >= 1 and t >= 1
    assert nwg & (nwg - 1) == 0 and t & (t - 1) == 0  # halving trees


def test_work_bytes_answers_its_errors_and_grows_with_the_vectors():
    einval = -errno.EINVAL
    assert S._lib.spmv_cg_work_bytes(-1, 1) == einval
    for k in (0, 9, -1):
        assert S._lib.spmv_cg_work_bytes(10, k) == einval
        with pytest.raises(OSError) as ei:
            S.cg_work_bytes(10, k)
        assert ei.value.errno == errno.EINVAL
    base = S.cg_work_bytes(0, 1)
    assert base > 0 and base % 8 == 0
    for k in range(1, 9):
        assert S.cg_work_bytes(0, k) == base
        # three vectors of M x k doubles: R, P, Q
        assert S.cg_work_bytes(1000, k) == base + 3 * 8 * 1000 * k
    # no 32-bit overflow
    assert S.cg_work_bytes(2**31 - 1, 8) == base + 3 * 8 * (2**31 - 1) * 8


def test_dead_handles_are_refused():
    x = C.create_string_buffer(64)
    px = C.cast(x, C.c_void_p)
    junk = C.create_string_buffer(512)  # never a handle of the library
    pj = C.cast(junk, C.c_void_p)
    info = (S.CgInfo * 8)()
    dead = -errno.EBADF if S.device_count() > 0 else -errno.ENODEV
    for fmt in ("csr", "hll"):
        cg = getattr(S._lib, "spmv_%s_cg" % fmt)
        multi = getattr(S._lib, "spmv_%s_launch_multi" % fmt)
        args = (None, 1, px, 1, px, 1, 1e-8, 10, 0, None, 0, info, None)
        assert cg(None, *args) == -errno.EINVAL
        assert cg(pj, *args) == dead
        # one function checks the handle for all three: the same answers
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
            fake.cg(1, 2, **kw)
    assert not calls
    # a good call does reach the library: k, B, ldb, X, ldx, tol, maxit,
    # check_every, work, work_bytes
    got = fake.cg(1, 2, 4, tol=1e-6, maxit=17, check_every=3, ldb=6)
    assert len(calls) == 1 and calls[0][0] == "cg"
    assert calls[0][2:12] == (4, 1, 6, 2, 0, 1e-6, 17, 3, None, 0)
    assert type(calls[0][7]) is float
    assert len(calls[0][12]) == 4  # k records for the library to fill
    assert got == [S.CgResult(0, 0, 0.0, 0.0)] * 4
    fake.cg(1, 2)  # one system, the defaults
    assert calls[1][2] == 1 and calls[1][7:10] == (1e-8, 1000, 0)

    class Work:
        ptr, nbytes = 4096, 777
    fake.cg(1, 2, 2, work=Work)
    assert calls[2][10:12] == (4096, 777)


# ------------------------------------------------------ the restatement
def test_the_dot_is_a_sum_in_the_documented_order():
    """against a scalar loop over slots, on shapes small enough for one:
    several sweeps, a ragged last sweep, fewer elements than slots"""
    rng = np.random.default_rng(11)
    for (nwg, T), M in (((4, 8), 1), ((4, 8), 7), ((4, 8), 32), ((4, 8), 33),
                        ((4, 8), 100), ((2, 2), 9)):
        U, V = rng.uniform(-1, 1, (M, 2)), rng.uniform(-1, 1, (M, 2))
        for j in range(2):
            slot = [0.0] * (nwg * T)
            for i in range(M):
                slot[i % (nwg * T)] = slot[i % (nwg * T)] + U[i, j] * V[i, j]
            wsum = []
            for w in range(nwg):
                s = slot[w * T:(w + 1) * T]
                h = T // 2
                while h:
                    for t in range(h):
                        s[t] = s[t] + s[t + h]
                    h //= 2
                wsum.append(s[0])
            h = nwg // 2
            while h:
                for t in range(h):
                    wsum[t] = wsum[t] + wsum[t + h]
                h //= 2
            got = G.dot(U, V, (nwg, T))[j]
            assert np.float64(wsum[0]).tobytes() == got.tobytes(), (nwg, T, M)


def _solve(mat, tol=TOL, maxit=200, B=None, X0=None):
    M, IRP, JA, AS = mat
    if B is None:
        B, X0 = G.common_inputs(M)
    product, residual0 = G.dense_product(IRP, JA, AS, O.csr_spmv)
    s = G.restate(product, residual0(B, X0), B, X0, tol, maxit)
    return s, G.true_residual(IRP, JA, AS, O.csr_spmv, B, s.X), B, X0


@pytest.mark.parametrize("name,mat", [
    ("lap2d(15,17,0.5)", G.lap2d(15, 17, 0.5)),
    ("lap2d(37,29,0.5)", G.lap2d(37, 29, 0.5)),
    ("arrow(2051,3)", G.arrow(2051, 3)),
    ("arrow(4099,3)", G.arrow(4099, 3))])
def test_the_restatement_solves_the_test_matrices(name, mat):
    s, res, B, X0 = _solve(mat)
    assert s.status.tolist() == [0, 0, 0, 0], name
    assert np.all(res <= 1.0e-8), (name, res)
    # the zero column: converged before the first iteration, X untouched
    assert s.iterations[1] == 0 and s.bb[1] == 0.0 and s.rr[1] == 0.0
    assert np.all(s.X[:, 1] == 0.0)
    assert np.all(s.iterations[[0, 2, 3]] > 0)
    if name == "lap2d(37,29,0.5)":
        assert s.iterations.tolist() == [36, 0, 36, 38]
    # stopped early, a column keeps what it had: maxit = 7
    s7, _, _, _ = _solve(mat, maxit=7)
    assert s7.status.tolist() == [1, 0, 1, 1], name
    assert s7.iterations.tolist() == [7, 0, 7, 7], name


def test_the_generators_give_symmetric_matrices_of_the_stated_shape():
    for mat in (G.lap2d(5, 4, 0.5), G.arrow(40, 3)):
        M, IRP, JA, AS = mat
        D = np.zeros((M, M))
        for r in range(M):
            D[r, JA[IRP[r]:IRP[r + 1]]] = AS[IRP[r]:IRP[r + 1]]
            assert np.all(np.diff(JA[IRP[r]:IRP[r + 1]]) > 0)
        assert np.array_equal(D, D.T)
        assert np.all(np.linalg.eigvalsh(D) > 0)
    M, IRP, JA, AS = G.arrow(2051, 3)
    assert IRP[1] == 2051 > 2048      # the CSR long-row kernel, a wide block
    M, IRP, JA, AS = G.lap2d(5, 4, 0.5)
    assert M == 20 and np.all(AS[JA == np.repeat(np.arange(M), np.diff(IRP))]
                              == 4.5)


def test_an_indefinite_matrix_is_a_breakdown_not_a_solution():
    # diagonal -5: p.Ap < 0 at once
    s, _, B, X0 = _solve(G.lap2d(15, 17, -9))
    assert s.status.tolist() == [2, 0, 2, 2]
    assert s.iterations.tolist() == [0, 0, 0, 0]
    assert np.array_equal(s.X.view(np.uint64), X0.view(np.uint64))
    # diagonal 2: indefinite, found after one and after two updates
    s, _, _, _ = _solve(G.lap2d(15, 17, -2))
    assert s.status.tolist() == [2, 0, 2, 2]
    assert s.iterations.tolist() == [1, 0, 1, 2]


def test_a_nonfinite_right_hand_side_stops_its_own_column_only():
    mat = G.lap2d(15, 17, 0.5)
    B, X0 = G.common_inputs(mat[0])
    clean, _, _, _ = _solve(mat, B=B, X0=X0)
    Bi = B.copy()
    Bi[7, 0] = np.inf
    s, _, _, _ = _solve(mat, B=Bi, X0=X0)
    assert s.status.tolist() == [2, 0, 0, 0]
    assert s.iterations[0] == 0
    assert np.array_equal(s.X[:, 1:].view(np.uint64),
                          clean.X[:, 1:].view(np.uint64))
    assert s.iterations[1:].tolist() == clean.iterations[1:].tolist()
