"""Preconditioned CG and the diagonal of a handle (spmv_*_pcg, spmv_*_diag,
spmv_pcg_work_bytes; spmv_engine.h): what can be checked without a GPU -- the
declared surface, the ctypes signatures, the dead-handle answers, the argument
checks of the Python wrapper, and the numpy restatement (tests/_pcg.py) run
with the CPU oracle's product.  The kernels: tests/test_gpu_pcg.py."""
import ctypes as C
import errno

import numpy as np
import pytest

import _cg as G
import _oracle as O
import _pcg as PG
import spmv_scpa_amd as S

NEW = ["spmv_csr_diag", "spmv_hll_diag", "spmv_pcg_work_bytes",
       "spmv_csr_pcg", "spmv_hll_pcg"]
TOL = 1e-8


def test_the_headers_declare_the_five_entry_points():
    declared = S.declared_symbols()
    for name in NEW:
        assert name in declared, name
        assert hasattr(S._lib, name), name
    assert S.check_symbols()
    # detected by the symbol, not by the version string
    assert S.version() == "spmv_scpa_amd 0.7 gfx950"


def test_the_twin_signatures_come_from_the_shared_list():
    names = [t[0] for t in S._TWINS]
    assert names.count("pcg") == 1 and names.count("diag") == 1
    for fmt in ("csr", "hll"):
        fn = getattr(S._lib, "spmv_%s_pcg" % fmt)
        assert fn.restype is C.c_int
        # cg's arguments with d_minv behind ldx
        cg = getattr(S._lib, "spmv_%s_cg" % fmt).argtypes
        assert fn.argtypes == cg[:7] + [C.c_void_p] + cg[7:]
        fn = getattr(S._lib, "spmv_%s_diag" % fmt)
        assert fn.restype is C.c_int
        assert fn.argtypes == [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    assert S._lib.spmv_pcg_work_bytes.restype is C.c_int64
    assert S._lib.spmv_pcg_work_bytes.argtypes == [C.c_int, C.c_int]


def test_work_bytes_is_cg_s_and_one_more_set_of_partial_sums():
    einval = -errno.EINVAL
    assert S._lib.spmv_pcg_work_bytes(-1, 1) == einval
    for k in (0, 9, -1):
        assert S._lib.spmv_pcg_work_bytes(10, k) == einval
        with pytest.raises(OSError) as ei:
            S.pcg_work_bytes(10, k)
        assert ei.value.errno == errno.EINVAL
    nwg, _ = S.CG_DOT_SHAPE
    part = nwg * 8 * 8  # one sum per workgroup and column, 8 columns
    for M in (0, 1000, 2**31 - 1):
        for k in range(1, 9):
            assert S.pcg_work_bytes(M, k) == S.cg_work_bytes(M, k) + part


def test_dead_handles_are_refused():
    x = C.create_string_buffer(64)
    px = C.cast(x, C.c_void_p)
    junk = C.create_string_buffer(512)  # never a handle of the library
    pj = C.cast(junk, C.c_void_p)
    info = (S.CgInfo * 8)()
    dead = -errno.EBADF if S.device_count() > 0 else -errno.ENODEV
    for fmt in ("csr", "hll"):
        pcg = getattr(S._lib, "spmv_%s_pcg" % fmt)
        diag = getattr(S._lib, "spmv_%s_diag" % fmt)
        args = (None, 1, px, 1, px, 1, px, 1e-8, 10, 0, None, 0, info, None)
        assert pcg(None, *args) == -errno.EINVAL
        assert pcg(pj, *args) == dead
        assert diag(None, px, 0, None) == -errno.EINVAL
        assert diag(pj, px, 0, None) == dead
        assert diag(pj, None, 1, None) == dead  # the handle first


@pytest.mark.parametrize("cls", [S.CsrDevice, S.HllDevice])
def test_the_wrapper_checks_k_and_the_strides_before_anything_is_called(cls):
    fake = object.__new__(cls)  # a wrapper around no handle
    fake.h = None
    calls = []
    fake._call = lambda *a: calls.append(a)
    for kw in (dict(k=0), dict(k=9), dict(k=-1), dict(k=4, ldb=3),
               dict(k=4, ldx=2), dict(k=8, ldb=7, ldx=8)):
        with pytest.raises(ValueError):
            fake.pcg(1, 2, 3, **kw)
    assert not calls
    # k, B, ldb, X, ldx, minv, tol, maxit, check_every, work, work_bytes
    got = fake.pcg(1, 2, 3, 4, tol=1e-6, maxit=17, check_every=3, ldb=6)
    assert len(calls) == 1 and calls[0][0] == "pcg"
    assert calls[0][2:13] == (4, 1, 6, 2, 0, 3, 1e-6, 17, 3, None, 0)
    assert type(calls[0][8]) is float
    assert len(calls[0][13]) == 4  # k records for the library to fill
    assert got == [S.CgResult(0, 0, 0.0, 0.0)] * 4
    fake.pcg(1, 2, 3)  # one system, the defaults
    assert calls[1][2] == 1 and calls[1][8:11] == (1e-8, 1000, 0)

    class Work:
        ptr, nbytes = 4096, 777
    fake.pcg(1, 2, 3, 2, work=Work)
    assert calls[2][11:13] == (4096, 777)
    # diag: d_out, invert as 0 / 1, stream
    fake.diag(5)
    fake.diag(5, invert=True, stream=9)
    assert calls[3] == ("diag", 5, 0, None) and calls[4] == ("diag", 5, 1, 9)


# ------------------------------------------------------ the restatement
def _solves(mat, minv, tol=TOL, maxit=200, k=4):
    M, IRP, JA, AS = mat
    B, X0 = G.common_inputs(M, k)
    product, residual0 = G.dense_product(IRP, JA, AS, O.csr_spmv)
    return (PG.restate(product, residual0(B, X0), B, X0, minv, tol, maxit),
            G.restate(product, residual0(B, X0), B, X0, tol, maxit), B)


@pytest.mark.parametrize("name,mat", [
    ("lap2d(15,17,0.5)", G.lap2d(15, 17, 0.5)),
    ("arrow(2051,3)", G.arrow(2051, 3))])
def test_a_preconditioner_of_ones_gives_the_bits_of_plain_cg(name, mat):
    for maxit in (200, 7):
        pre, plain, _ = _solves(mat, np.ones(mat[0]), maxit=maxit)
        assert pre.status.tolist() == plain.status.tolist(), (name, maxit)
        assert pre.iterations.tolist() == plain.iterations.tolist(), name
        for a, b in ((pre.X, plain.X), (pre.rr, plain.rr), (pre.bb, plain.bb)):
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), name
    assert plain.status.tolist() == [1, 0, 1, 1]  # maxit = 7 stopped them


def test_jacobi_needs_a_quarter_of_the_iterations_on_the_scaled_stencil():
    """guards the fixture (numpy measured 36-37 against 565-572), not the
    device"""
    mat = PG.scaled_lap2d(15, 17, 0.5, 6, 7)
    M, IRP, JA, AS = mat
    d = PG.diag_of(*mat)
    assert np.all(d > 0) and d.max() / d.min() > 2.0 ** 10
    pre, plain, B = _solves(mat, 1.0 / d, maxit=2000)
    print("jacobi", pre.iterations.tolist(), "plain", plain.iterations.tolist())
    assert pre.status.tolist() == [0, 0, 0, 0]
    assert plain.status.tolist() == [0, 0, 0, 0]
    assert pre.iterations[1] == 0 and np.all(pre.X[:, 1] == 0.0)
    for j in (0, 2, 3):
        assert 0 < 4 * pre.iterations[j] <= plain.iterations[j], j
    res = G.true_residual(IRP, JA, AS, O.csr_spmv, B, pre.X)
    assert np.all(res <= 2 * TOL), res


def test_the_scaled_stencil_is_symmetric_and_diag_of_reads_its_diagonal():
    M, IRP, JA, AS = PG.scaled_lap2d(5, 4, 0.5, 6, 7)
    D = np.zeros((M, M))
    for r in range(M):
        D[r, JA[IRP[r]:IRP[r + 1]]] = AS[IRP[r]:IRP[r + 1]]
    assert np.array_equal(D, D.T)
    assert np.all(np.linalg.eigvalsh(D) > 0)
    assert np.array_equal(PG.diag_of(M, IRP, JA, AS), np.diag(D))
    s = 2.0 ** np.random.default_rng(7).uniform(0, 6, M)
    assert np.array_equal(np.diag(D), 4.5 * (s * s))
    # duplicates add up, a missing diagonal is 0.0, rows beyond N are left out
    IRP = np.array([0, 3, 4, 4, 6], np.int32)
    JA = np.array([0, 1, 0, 0, 3, 3], np.int32)
    AS = np.array([0.5, 9.0, 2.0, 7.0, 0.25, 0.25])
    assert PG.diag_of(4, IRP, JA, AS).tolist() == [2.5, 0.0, 0.0, 0.5]
    assert PG.diag_of(4, IRP, JA, AS, N=3).tolist() == [2.5, 0.0, 0.0]


def test_a_preconditioner_that_is_not_positive_is_a_breakdown():
    mat = G.lap2d(15, 17, 0.5)
    pre, _, _ = _solves(mat, -np.ones(mat[0]))
    assert pre.status.tolist() == [2, 0, 2, 2]
    assert pre.iterations.tolist() == [0, 0, 0, 0]
    inf = np.ones(mat[0])
    inf[9] = np.inf
    pre, _, _ = _solves(mat, inf)
    # the zero column too: inf * 0 is NaN, and a non-finite r.z comes first
    assert pre.status.tolist() == [2, 2, 2, 2]
    assert pre.iterations.tolist() == [0, 0, 0, 0]
