"""CGLS on the device (spmv_*_cgls, spmv_cgls_work_bytes; spmv_engine.h): what
can be checked without a GPU -- the declared surface, the ctypes signatures,
the dead-handle answers, the argument checks of the Python wrapper, and the
numpy restatement of the solver (tests/_cgls.py) run with the CPU oracle's
product: that the loop of the contract solves rectangular least-squares
problems (tall, wide, rank deficient, damped), that it agrees with dense
solves, and the edge rules.  The kernels themselves: tests/test_gpu_cgls.py."""
import ctypes as C
import errno

import numpy as np
import pytest

import _bicgstab as BI
import _cgls as LS
import _oracle as O
import spmv_scpa_amd as S

NEW = ["spmv_csr_cgls", "spmv_hll_cgls", "spmv_cgls_work_bytes"]
TOL = 1e-8
#: the record of a column nothing was done for (and, at import, the proof that
#: the binding has the solver at all: nothing in this file means anything
#: without it)
ZERO = S.CglsResult(0, 0, 0.0, 0.0, 0.0)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_the_headers_declare_the_cgls_entry_points():
    declared = S.declared_symbols()
    for name in NEW:
        assert name in declared, name
        assert hasattr(S._lib, name), name
    assert S.check_symbols()
    # the feature is detected by the symbol, not by the version string
    assert S.version() == "spmv_scpa_amd 0.7 gfx950"


def test_the_twin_signature_comes_from_the_shared_list():
    names = [t[0] for t in S._TWINS]
    assert names.count("cgls") == 1
    for fmt in ("csr", "hll"):
        fn = getattr(S._lib, "spmv_%s_cgls" % fmt)
        assert fn.restype is C.c_int
        assert fn.argtypes == [C.c_void_p, C.c_void_p, C.POINTER(S.LaunchOpts),
                               C.c_int, C.c_void_p, C.c_int64, C.c_void_p,
                               C.c_int64, C.c_double, C.c_double, C.c_int,
                               C.c_int, C.c_void_p, C.c_size_t,
                               C.POINTER(S.CglsInfo), C.c_void_p]
    assert S._lib.spmv_cgls_work_bytes.restype is C.c_int64
    assert S._lib.spmv_cgls_work_bytes.argtypes == [C.c_int, C.c_int, C.c_int]
    # the record: two ints and three doubles, as the header declares it
    assert [f[0] for f in S.CglsInfo._fields_] == \
        ["status", "iterations", "ss", "atb", "rr"]
    assert C.sizeof(S.CglsInfo) == 32
    assert S.CglsResult._fields == ("status", "iterations", "ss", "atb", "rr")


def test_work_bytes_answers_its_errors_and_grows_with_the_vectors():
    einval = -errno.EINVAL
    assert S._lib.spmv_cgls_work_bytes(-1, 1, 1) == einval
    assert S._lib.spmv_cgls_work_bytes(1, -1, 1) == einval
    for k in (0, 9, -1):
        assert S._lib.spmv_cgls_work_bytes(10, 10, k) == einval
        with pytest.raises(OSError) as ei:
            S.cgls_work_bytes(10, 10, k)
        assert ei.value.errno == errno.EINVAL
    base = S.cgls_work_bytes(0, 0, 1)
    assert base > 0 and base % 8 == 0
    for k in range(1, 9):
        assert S.cgls_work_bytes(0, 0, k) == base
        # R, Q of M rows and S, P of N rows
        assert S.cgls_work_bytes(1000, 0, k) == base + 8 * k * 2 * 1000
        assert S.cgls_work_bytes(0, 1000, k) == base + 8 * k * 2 * 1000
        assert S.cgls_work_bytes(1000, 37, k) == \
            base + 8 * k * (2 * 1000 + 2 * 37)
    # no 32-bit overflow
    big = 2**31 - 1
    assert S.cgls_work_bytes(big, big, 8) == base + 8 * 8 * (2 * big + 2 * big)


def test_dead_handles_are_refused_in_either_position():
    x = C.create_string_buffer(64)
    px = C.cast(x, C.c_void_p)
    junk = C.create_string_buffer(512)  # never a handle of the library
    pj = C.cast(junk, C.c_void_p)
    info = (S.CglsInfo * 8)()
    dead = -errno.EBADF if S.device_count() > 0 else -errno.ENODEV
    args = (None, 1, px, 1, px, 1, 0.0, 1e-8, 10, 0, None, 0, info, None)
    for fmt in ("csr", "hll"):
        solve = getattr(S._lib, "spmv_%s_cgls" % fmt)
        multi = getattr(S._lib, "spmv_%s_launch_multi" % fmt)
        # A is checked first, then AT, each with launch_multi's answers
        assert solve(None, None, *args) == -errno.EINVAL
        assert solve(None, pj, *args) == -errno.EINVAL
        assert solve(pj, pj, *args) == dead
        assert solve(pj, None, *args) == dead
        assert multi(None, None, 1, px, 1, px, 1, None) == -errno.EINVAL
        assert multi(pj, None, 1, px, 1, px, 1, None) == dead
    # (a live A with a dead or NULL AT: tests/test_gpu_cgls.py)


@pytest.mark.parametrize("cls", [S.CsrDevice, S.HllDevice])
def test_the_wrapper_checks_its_arguments_before_anything_is_called(cls):
    def fake_of(c, h):
        f = object.__new__(c)  # a wrapper around no handle
        f.h = h
        f.release = lambda: None  # ... so there is nothing to release
        return f
    fake, fake_t = fake_of(cls, None), fake_of(cls, 77)
    calls = []
    fake._call = lambda *a: calls.append(a)
    for kw in (dict(k=0), dict(k=9), dict(k=-1), dict(k=4, ldb=3),
               dict(k=4, ldx=2), dict(k=8, ldb=7, ldx=8)):
        with pytest.raises(ValueError):
            fake.cgls(fake_t, 1, 2, **kw)
    other = S.HllDevice if cls is S.CsrDevice else S.CsrDevice
    for bad in (fake_of(other, 77), None, 77, object()):
        with pytest.raises(TypeError):
            fake.cgls(bad, 1, 2)
    assert not calls
    # a good call does reach the library: AT, opts, k, B, ldb, X, ldx, damp,
    # tol, maxit, check_every, work, work_bytes, info, stream
    got = fake.cgls(fake_t, 1, 2, 4, damp=1, tol=1e-6, maxit=17,
                    check_every=3, ldb=6)
    assert len(calls) == 1 and calls[0][0] == "cgls" and calls[0][1] == 77
    assert calls[0][3:14] == (4, 1, 6, 2, 0, 1.0, 1e-6, 17, 3, None, 0)
    assert type(calls[0][8]) is float and type(calls[0][9]) is float
    assert len(calls[0][14]) == 4  # k records for the library to fill
    assert got == [ZERO] * 4
    fake.cgls(fake_t, 1, 2)  # one problem, no damping, the defaults
    assert calls[1][3] == 1 and calls[1][8:12] == (0.0, 1e-8, 1000, 0)

    class Work:
        ptr, nbytes = 4096, 777
    fake.cgls(fake_t, 1, 2, 2, work=Work)
    assert calls[2][12:14] == (4096, 777)


# ------------------------------------------------------ the restatement
def _solve(mat, damp=0.0, tol=TOL, maxit=2000, B=None, X0=None, k=4, **kw):
    if B is None:
        B, X0 = LS.inputs(mat, k)
    product, product_t, residual0 = LS.cpu_products(mat, O.csr_spmv)
    s = LS.restate(product, product_t, residual0(B, X0), B, X0, damp, tol,
                   maxit, **kw)
    return s, LS.normal_residual(mat, O.csr_spmv, B, s.X, damp), B, X0


MATRICES = {
    "stacked(24,20,0,.5,1)": lambda: LS.stacked(24, 20, 0.0, 0.5, 1.0),
    "stacked(33,31,0,.3,.5)": lambda: LS.stacked(33, 31, 0.0, 0.3, 0.5),
    "diff1d(300)": lambda: LS.diff1d(300),
    "wide(700,1500,3,5)": lambda: LS.wide(700, 1500, 3, 5),
    "arrow_rect(5000,3000,7)": lambda: LS.arrow_rect(5000, 3000, 7),
    "convdiff(40,37,.2,.4)":
        lambda: LS.square(BI.convdiff(40, 37, 0.2, 0.4)),
    "stacked(24,20,0,.5,1) less column 17":
        lambda: LS.without_column(LS.stacked(24, 20, 0.0, 0.5, 1.0), 17),
    "long(600000,257,2,9)":
        lambda: LS.transpose(LS.wide(257, 600000, 2, 9)),
}
SHAPES = {
    "stacked(24,20,0,.5,1)": (960, 480),
    "stacked(33,31,0,.3,.5)": (2046, 1023),
    "diff1d(300)": (301, 300),
    "wide(700,1500,3,5)": (700, 1500),
    "arrow_rect(5000,3000,7)": (5000, 3000),
    "convdiff(40,37,.2,.4)": (1480, 1480),
    "stacked(24,20,0,.5,1) less column 17": (960, 480),
    "long(600000,257,2,9)": (600000, 257),
}
#: iterations of the four columns with the CPU oracle's product, damp 0 / 0.5
PINNED = {
    "stacked(24,20,0,.5,1)": ([69, 0, 69, 74], [62, 0, 63, 66]),
    "stacked(33,31,0,.3,.5)": ([134, 0, 135, 136], [98, 0, 97, 101]),
    "diff1d(300)": ([300, 0, 300, 300], [36, 0, 36, 37]),
    "wide(700,1500,3,5)": ([24, 0, 24, 25], [22, 0, 22, 27]),
    "arrow_rect(5000,3000,7)": ([30, 0, 29, 29], [26, 0, 25, 26]),
    "convdiff(40,37,.2,.4)": ([277, 0, 280, 270], [124, 0, 123, 130]),
    "stacked(24,20,0,.5,1) less column 17":
        ([70, 0, 69, 74], [63, 0, 63, 76]),
    "long(600000,257,2,9)": ([6, 0, 6, 7], [6, 0, 6, 7]),
}


@pytest.mark.parametrize("damp", [0.0, 0.5])
@pytest.mark.parametrize("name", list(MATRICES))
def test_the_restatement_solves_the_test_matrices(name, damp):
    mat = MATRICES[name]()
    assert mat[:2] == SHAPES[name]
    s, res, B, X0 = _solve(mat, damp)
    print(name, damp, "iterations", s.iterations.tolist(), "normal residual",
          res)
    assert s.status.tolist() == [0, 0, 0, 0], name
    # the recurrence's own test is <= tol; the recomputed residual stayed
    # below 1.0 tol in the experiment of the issue, the factor 2 is the gap
    assert np.all(res <= 2 * TOL), (name, res)
    assert np.all(s.ss <= TOL * TOL * s.atb)
    # the zero column: A^T b = 0 and, with X0 = 0, s = 0: converged at once
    assert s.iterations[1] == 0 and s.atb[1] == 0.0 and s.ss[1] == 0.0
    assert s.rr[1] == 0.0
    assert np.array_equal(bits(s.X[:, 1]), bits(X0[:, 1]))
    assert np.all(s.iterations[[0, 2, 3]] > 0)
    assert s.iterations.tolist() == PINNED[name][damp != 0], (name, damp)
    # stopped early, a column keeps what it had: maxit = 3
    s3, _, _, _ = _solve(mat, damp, maxit=3)
    assert s3.status.tolist() == [1, 0, 1, 1], name
    assert s3.iterations.tolist() == [3, 0, 3, 3], name


def test_the_generators_give_the_stated_matrices():
    def sorted_rows(mat):
        M, N, IRP, JA, AS = mat
        assert len(IRP) == M + 1 and IRP[-1] == len(JA) == len(AS)
        assert JA.min() >= 0 and JA.max() < N
        for r in range(0, M, max(1, M // 50)):  # strictly increasing columns
            assert np.all(np.diff(JA[IRP[r]:IRP[r + 1]]) > 0)
    conv = LS.dense(LS.square(BI.convdiff(5, 4, 0.0, 0.5)))
    st = LS.stacked(5, 4, 0.0, 0.5, 0.25)
    sorted_rows(st)
    D = LS.dense(st)
    assert D.shape == (40, 20)
    assert np.array_equal(D[:20], conv)
    assert np.array_equal(D[20:], 0.25 * np.eye(20))
    D17 = LS.dense(LS.without_column(st, 17))
    assert np.all(D17[:, 17] == 0)
    D17[:, 17] = D[:, 17]
    assert np.array_equal(D17, D)
    assert np.linalg.matrix_rank(LS.dense(LS.without_column(st, 17))) == 19
    D = LS.dense(LS.diff1d(6))
    assert D.shape == (7, 6)
    assert np.array_equal(D, np.eye(7, 6) - np.eye(7, 6, k=-1))
    w = LS.wide(40, 100, 3, 5)
    sorted_rows(w)
    D = LS.dense(w)
    assert D.shape == (40, 100)
    d = np.diag(D[:, :40])
    assert np.array_equal(D[:, :40], np.diag(d)) and np.all((1 <= d) & (d < 2))
    assert np.all(np.count_nonzero(D[:, 40:], axis=0) == 3)  # per column
    assert np.all(np.abs(D[:, 40:]) < 1)
    a = LS.arrow_rect(50, 30, 7)
    sorted_rows(a)
    D = LS.dense(a)
    assert D.shape == (50, 30)
    assert np.all(D[0] != 0) and np.all(D[:, 0] != 0)
    assert np.count_nonzero(D) == 30 + 49 + 29
    assert np.all(np.diag(D)[1:] >= 1)
    t = LS.transpose(a)
    sorted_rows(t)
    assert np.array_equal(LS.dense(t), D.T)
    M, N, IRP, JA, AS = MATRICES["arrow_rect(5000,3000,7)"]()
    assert IRP[1] == 3000 > 2048      # the CSR long-row kernel, a wide block
    M, N, IRP, JA, AS = MATRICES["long(600000,257,2,9)"]()
    sorted_rows((M, N, IRP, JA, AS))
    assert IRP[-1] == 257 + 2 * (600000 - 257)
    # dot_M takes three sweeps of the slots, dot_N two workgroups with a tail
    nwg, T = S.CG_DOT_SHAPE
    assert 2 * nwg * T < M <= 3 * nwg * T and N == T + 1


@pytest.mark.parametrize("damp", [0.0, 0.5])
def test_the_minimum_norm_solution_of_a_wide_system(damp):
    mat = MATRICES["wide(700,1500,3,5)"]()
    M, N = mat[:2]
    B, _ = LS.inputs(mat)
    s, _, _, _ = _solve(mat, damp, B=B, X0=np.zeros((N, 4)))
    assert s.status.tolist() == [0, 0, 0, 0]
    D = LS.dense(mat)
    if damp:
        want = np.linalg.solve(D.T @ D + damp * damp * np.eye(N), D.T @ B)
    else:
        want = np.linalg.lstsq(D, B, rcond=None)[0]  # the minimum norm
    err = np.linalg.norm(s.X - want, axis=0) / \
        np.maximum(np.linalg.norm(want, axis=0), 1e-300)
    print("wide, damp", damp, "relative error", err)
    assert np.all(err <= 1e-6), err


@pytest.mark.parametrize("name", ["stacked(24,20,0,.5,1)", "diff1d(300)",
                                  "stacked(24,20,0,.5,1) less column 17"])
def test_a_damped_solve_agrees_with_the_dense_normal_equations(name):
    mat = MATRICES[name]()
    M, N = mat[:2]
    damp = 0.5
    s, _, B, X0 = _solve(mat, damp)
    assert s.status.tolist() == [0, 0, 0, 0]
    D = LS.dense(mat)
    want = np.linalg.solve(D.T @ D + damp * damp * np.eye(N), D.T @ B)
    err = np.linalg.norm(s.X - want, axis=0) / \
        np.maximum(np.linalg.norm(want, axis=0), 1e-300)
    print(name, "relative error", err)
    assert np.all(err[[0, 2, 3]] <= 1e-6), err
    # the zero column starts from X0 and the unique minimiser is 0: column 1
    # of X0 is zero, so nothing moved
    assert np.all(s.X[:, 1] == 0.0)


def test_damp_zero_has_no_d2_term():
    mat = MATRICES["stacked(24,20,0,.5,1)"]()
    for maxit in (200, 3):
        a, _, _, _ = _solve(mat, 0.0, maxit=maxit)
        b, _, _, _ = _solve(mat, 0.0, maxit=maxit, d2_path=False)
        for f in ("X", "ss", "atb", "rr"):
            assert np.array_equal(bits(getattr(a, f)), bits(getattr(b, f)))
        assert a.iterations.tolist() == b.iterations.tolist()
    # and damping is not a no-op
    c, _, _, _ = _solve(mat, 0.5, maxit=3)
    d, _, _, _ = _solve(mat, 0.0, maxit=3)
    assert not np.array_equal(bits(c.X), bits(d.X))


# ------------------------------------------------------------ the edge rules
def _edge(mat, B, damp=0.0, maxit=200):
    return _solve(mat, damp, maxit=maxit, B=B,
                  X0=np.zeros((mat[1], B.shape[1])))


def test_twice_the_identity_is_solved_in_one_step():
    B = np.random.default_rng(2).uniform(-1, 1, (70, 2))
    s, _, _, _ = _edge(LS.diagm(np.full(70, 2.0)), B)
    # ss = 4 b.b and delta = 16 b.b exactly: alpha = 1/4, X = B/2, R = 0
    assert s.status.tolist() == [0, 0]
    assert s.iterations.tolist() == [1, 1]
    assert s.ss.tolist() == [0.0, 0.0] and s.rr.tolist() == [0.0, 0.0]
    assert np.array_equal(bits(s.X), bits(B / 2))


def test_b_orthogonal_to_the_range_is_converged_at_once():
    mat = LS._rect(2, 1, [0, 1], [0, 0], [1.0, 1.0])
    B = np.array([[1.0], [-1.0]])
    X0 = np.array([[0.0]])
    s, _, _, _ = _solve(mat, B=B, X0=X0)
    assert s.atb.tolist() == [0.0] and s.ss.tolist() == [0.0]
    assert s.status.tolist() == [0] and s.iterations.tolist() == [0]
    assert np.array_equal(bits(s.X), bits(X0))
    assert s.rr.tolist() == [2.0]


def test_a_nan_in_b_is_a_breakdown_before_the_first_step():
    mat = MATRICES["stacked(24,20,0,.5,1)"]()
    B, X0 = LS.inputs(mat)
    clean, _, _, _ = _solve(mat, B=B, X0=X0)
    Bn = B.copy()
    Bn[7, 0] = np.nan
    s, _, _, _ = _solve(mat, B=Bn, X0=X0)
    assert s.status.tolist() == [2, 0, 0, 0]
    assert s.iterations[0] == 0
    assert np.array_equal(bits(s.X[:, 0]), bits(X0[:, 0]))
    # ... of its own column only
    assert np.array_equal(bits(s.X[:, 1:]), bits(clean.X[:, 1:]))
    assert s.iterations[1:].tolist() == clean.iterations[1:].tolist()
    assert np.array_equal(bits(s.ss[1:]), bits(clean.ss[1:]))
    assert np.array_equal(bits(s.rr[1:]), bits(clean.rr[1:]))


def test_an_infinite_atb_is_a_breakdown():
    s, _, _, X0 = _edge(LS.diagm(np.full(70, 1e200)), np.ones((70, 2)))
    assert np.all(np.isinf(s.atb))
    assert s.status.tolist() == [2, 2] and s.iterations.tolist() == [0, 0]
    assert np.array_equal(bits(s.X), bits(X0))


def test_a_delta_that_underflows_to_zero_is_a_breakdown():
    s, _, _, X0 = _edge(LS.diagm(np.full(70, 1e-120)), np.full((70, 2), 1e40))
    # S = 1e-80, ss = atb > 0: running; Q = 1e-200, Q.Q underflows to 0
    assert np.all(s.ss > 0) and np.array_equal(bits(s.ss), bits(s.atb))
    assert s.status.tolist() == [2, 2] and s.iterations.tolist() == [0, 0]
    assert np.array_equal(bits(s.X), bits(X0))
