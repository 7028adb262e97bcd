"""Conjugate gradients on the device (spmv_*_cg, spmv_engine.h) on the GPU: CSR
and column-major HLL handles, f64 and f32 values, 1-8 interleaved systems.

The expected values come from the numpy restatement of the solver
(tests/_cg.py), with Q = A P taken from the SAME handle's launch_multi and the
initial residual from its launch_axpby, both with the same opts.  numpy rounds
every operation once, which is the contract, so the uint64 views of X are
compared, and iterations, status and the bits of rr / bb.  No tolerance
appears anywhere except the sanity line of the first test: the true residual
of the device's X, computed on the host, is at most 2 tol (the restatement
reaches 0.99 tol on these inputs; the factor 2 only keeps a wrong contract
that still "matches itself" from passing).

Common inputs (tests/_cg.py, common_inputs): B = uniform(-1, 1), seed 1,
k = 4; column 1 all zero; column 2 scaled by 1e-3; X0 zero except column 3.

Every test runs under a time limit of its own (LIMIT_S): a test that exceeds
it ends the whole process, so nothing else is started on the device.
"""
import ctypes as C
import errno
import faulthandler

import numpy as np
import pytest

import _cg as G
import _oracle as O
import spmv_scpa_amd as S
from test_gpu_f32_values import round32
from test_gpu_multi_vector import FILL, PAST, bits, handles

pytestmark = pytest.mark.gpu

LIMIT_S = 240
TOL = 1e-8
NWG, T = S.CG_DOT_SHAPE
#: one grid just above one full sweep of the dot's slots (523 x 502 with the
#: 1024 x 256 shape): every slot holds an element and the first 402 hold two
BIG_NX = 523
BIG_NY = -(-(NWG * T + 1) // BIG_NX)
MATRICES = {
    "lap2d(1,1,0.5)": lambda: G.lap2d(1, 1, 0.5),
    "lap2d(15,17,0.5)": lambda: G.lap2d(15, 17, 0.5),   # below one workgroup
    "lap2d(37,29,0.5)": lambda: G.lap2d(37, 29, 0.5),   # M = 1073, odd
    "arrow(2051,3)": lambda: G.arrow(2051, 3),
    "arrow(4099,3)": lambda: G.arrow(4099, 3),
    "lap2d(big)": lambda: G.lap2d(BIG_NX, BIG_NY, 1.0),
}


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def fill(buf):
    S._check(S._lib.spmv_dev_memset(buf.ptr, 0xFF, buf.nbytes, None),
             "spmv_dev_memset")


def put(ptr, a):
    a = np.ascontiguousarray(a, np.float64)
    S.stream_sync()
    S._check(S._lib.spmv_copy_h2d(ptr, a.ctypes.data, a.nbytes),
             "spmv_copy_h2d")


class CgBench:
    """device buffers of one M: B and X of the solver (sized for strides up
    to 8 + 3, PAST rows beyond M and an 8-byte shift), and the P / Q pair the
    restatement multiplies with"""

    def __init__(self, M):
        self.M = M
        n = (M + PAST) * (8 + 3) * 8 + 8
        self.B, self.X = S.DevBuffer(n), S.DevBuffer(n)
        self.P, self.Q = S.DevBuffer(M * 8 * 8), S.DevBuffer(M * 8 * 8)

    def callables(self, m, B, X0, **opts):
        """-> (product, residual0) on handle m, for restate()"""
        M, k = B.shape

        def product(P):
            put(self.P.ptr, P)
            m.launch_multi(self.P.ptr, self.Q.ptr, k, **opts)
            S.stream_sync()
            return self.Q.to_numpy(np.float64, M * k).reshape(M, k)

        def residual0():
            put(self.P.ptr, X0)
            put(self.Q.ptr, B)
            m.launch_axpby(-1.0, 1.0, self.P.ptr, self.Q.ptr, k, **opts)
            S.stream_sync()
            return self.Q.to_numpy(np.float64, M * k).reshape(M, k)
        return product, residual0

    def want(self, m, B, X0, tol=TOL, maxit=200, **opts):
        product, residual0 = self.callables(m, B, X0, **opts)
        return G.restate(product, residual0, B, X0, tol, maxit)

    def solve(self, m, B, X0, ldb=0, ldx=0, shift=0, **kw):
        """-> (records, whole X buffer as (M + PAST, ldx), whole B buffer as
        (M + PAST, ldb)): padding columns of B are NaN, those of X and the
        rows beyond M of both hold the 0xFF fill"""
        M, k = B.shape
        lb, lx = ldb or k, ldx or k
        Bh = np.full((M + PAST, lb), np.nan)
        bits(Bh)[M:] = FILL
        Bh[:M, :k] = B
        Xh = np.empty((M + PAST, lx))
        bits(Xh)[:] = FILL
        Xh[:M, :k] = X0
        fill(self.B)
        fill(self.X)
        put(self.B.ptr, Bh)
        put(self.X.ptr + shift, Xh)
        rec = m.cg(self.B.ptr, self.X.ptr + shift, k, ldb=ldb, ldx=ldx, **kw)
        S.stream_sync()
        Xf = self.X.to_numpy(np.float64, (M + PAST) * lx + shift // 8)
        Bf = self.B.to_numpy(np.float64, (M + PAST) * lb)
        assert np.array_equal(bits(Bf), bits(Bh.ravel())), "B was written"
        return rec, Xf[shift // 8:].reshape(M + PAST, lx), Bh

    def free(self):
        for b in (self.B, self.X, self.P, self.Q):
            b.free()


def same_solve(rec, X, want, tag):
    """a device solve against a restatement (or two device solves): bits"""
    k = len(rec)
    print(tag, "status", [r.status for r in rec], "iterations",
          [r.iterations for r in rec])
    assert [r.status for r in rec] == list(want.status), tag
    assert [r.iterations for r in rec] == list(want.iterations), tag
    for name in ("rr", "bb"):
        got = np.array([getattr(r, name) for r in rec])
        assert np.array_equal(bits(got), bits(getattr(want, name))), \
            (tag, name, got, getattr(want, name))
    same = bits(X[:, :k]) == bits(want.X)
    assert np.all(same), (tag, "elements of X that differ",
                          int(np.sum(~same)), np.argwhere(~same)[:4].tolist())


def as_solve(rec, X):
    k = len(rec)
    return G.Solve(X[:, :k].copy(), [r.status for r in rec],
                   [r.iterations for r in rec],
                   np.array([r.rr for r in rec]),
                   np.array([r.bb for r in rec]))


def neighbours_kept(Xf, M, k, tag):
    assert np.all(bits(Xf[:M, k:]) == FILL), (tag, "columns beyond k")
    assert np.all(bits(Xf[M:]) == FILL), (tag, "rows beyond M")


def upload(mat, values):
    M, IRP, JA, AS = mat
    A = S.csr_from_arrays("cg", M, M, IRP, JA, AS)
    hs = handles(A, values)
    S.csr_free(A)
    return hs


# -------------------------------------------------------------------- 1. bits
@pytest.mark.parametrize("values", ["f64", "f32"])
@pytest.mark.parametrize("name", list(MATRICES))
def test_a_solve_has_the_bits_of_the_restatement(name, values):
    mat = MATRICES[name]()
    M, IRP, JA, AS = mat
    if name == "lap2d(big)":
        assert NWG * T < M <= NWG * T + BIG_NX
    if name.startswith("arrow"):
        assert IRP[1] == M > 2048   # the CSR long-row kernel, a wide block
    stored = round32(AS) if values == "f32" else AS
    B, X0 = G.common_inputs(M)
    bench = CgBench(M)
    hs = upload(mat, values)
    for fmt, m in hs.items():
        tag = (name, values, fmt)
        want = bench.want(m, B, X0)
        rec, Xf, _ = bench.solve(m, B, X0, tol=TOL, maxit=200)
        same_solve(rec, Xf[:M], want, tag)
        neighbours_kept(Xf, M, 4, tag)
        assert [r.status for r in rec] == [0, 0, 0, 0], tag
        # the zero column: converged at once, X untouched
        assert rec[1].iterations == 0 and rec[1].bb == 0.0, tag
        assert np.array_equal(bits(Xf[:M, 1]), bits(X0[:, 1])), tag
        # the sanity line: the true residual of the device's X
        res = G.true_residual(IRP, JA, stored, O.csr_spmv, B, Xf[:M, :4])
        print(tag, "true residual", res)
        assert np.all(res <= 2 * TOL), (tag, res)
        # stopped by maxit: every non-zero column after exactly 7 updates
        want7 = bench.want(m, B, X0, maxit=7)
        rec, Xf, _ = bench.solve(m, B, X0, tol=TOL, maxit=7)
        same_solve(rec, Xf[:M], want7, tag + ("maxit 7",))
        if M > 1:  # a 1 x 1 system is solved by its first update
            assert [r.status for r in rec] == [1, 0, 1, 1], tag
            assert [r.iterations for r in rec] == [7, 0, 7, 7], tag
        assert np.array_equal(bits(Xf[:M, 1]), bits(X0[:, 1])), tag
    for m in hs.values():
        m.release()
    bench.free()


# ------------------------------------------------------------ 2. independence
@pytest.mark.parametrize("name", ["lap2d(37,29,0.5)", "arrow(4099,3)"])
def test_the_result_depends_on_the_system_alone(name):
    mat = MATRICES[name]()
    M = mat[0]
    B, X0 = G.common_inputs(M)
    bench = CgBench(M)
    hs = upload(mat, "f64")
    work = S.DevBuffer(S.cg_work_bytes(M, 8))
    for fmt, m in hs.items():
        rec, Xf, _ = bench.solve(m, B, X0, tol=TOL, maxit=200)
        base = as_solve(rec, Xf[:M])
        assert base.status == [0, 0, 0, 0]
        for kw in (dict(check_every=1), dict(check_every=7),
                   dict(check_every=0), dict(work=work),
                   dict(waves_per_block=1), dict(waves_per_block=8)):
            rec, Xf, _ = bench.solve(m, B, X0, tol=TOL, maxit=200, **kw)
            same_solve(rec, Xf[:M], base, (name, fmt, kw))
        # column j of the k = 4 solve is the k = 1 solve of that column
        for j in range(4):
            rec, Xf, _ = bench.solve(m, B[:, j:j + 1], X0[:, j:j + 1],
                                     tol=TOL, maxit=200)
            one = G.Solve(base.X[:, j:j + 1], base.status[j:j + 1],
                          base.iterations[j:j + 1], base.rr[j:j + 1],
                          base.bb[j:j + 1])
            same_solve(rec, Xf[:M], one, (name, fmt, "column", j))
        # other widths against the restatement
        for k in (3, 8):
            Bk, Xk = G.common_inputs(M, k)
            want = bench.want(m, Bk, Xk)
            rec, Xf, _ = bench.solve(m, Bk, Xk, tol=TOL, maxit=200)
            same_solve(rec, Xf[:M], want, (name, fmt, "k", k))
            neighbours_kept(Xf, M, k, (name, fmt, "k", k))
    work.free()
    for m in hs.values():
        m.release()
    bench.free()


# ----------------------------------------------------------------- 3. strides
class _Exactly:
    """`work` of exactly n bytes at the head of a larger allocation"""

    def __init__(self, buf, n):
        self.ptr, self.nbytes = buf.ptr, n


@pytest.mark.parametrize("values", ["f64", "f32"])
def test_strides_an_unaligned_X_and_the_neighbours(values):
    mat = MATRICES["arrow(2051,3)"]()
    M = mat[0]
    k = 4
    B, X0 = G.common_inputs(M)
    bench = CgBench(M)
    hs = upload(mat, values)
    need = S.cg_work_bytes(M, k)
    guard = 4096
    work = S.DevBuffer(need + guard)
    for fmt, m in hs.items():
        tag = (values, fmt)
        want = bench.want(m, B, X0)
        S._check(S._lib.spmv_dev_memset(work.ptr, 0xA5, work.nbytes, None),
                 "spmv_dev_memset")
        # ldx = k + 1: a column of X that is not the solver's; ldb = k + 3:
        # NaN padding in B; X 8 bytes off 16; rows beyond M of both
        rec, Xf, _ = bench.solve(m, B, X0, ldb=k + 3, ldx=k + 1, shift=8,
                                 tol=TOL, maxit=200,
                                 work=_Exactly(work, need))
        same_solve(rec, Xf[:M], want, tag)
        neighbours_kept(Xf, M, k, tag)
        tail = work.to_numpy(np.uint8, need + guard)[need:]
        assert np.all(tail == 0xA5), (tag, "bytes behind the work buffer")
    work.free()
    for m in hs.values():
        m.release()
    bench.free()


# --------------------------------------------------------------- 4. breakdown
def test_a_breakdown_is_a_status_not_a_fault():
    M = 15 * 17
    B, X0 = G.common_inputs(M)
    bench = CgBench(M)
    # diagonal -5: p.Ap < 0 before the first update
    hs = upload(G.lap2d(15, 17, -9), "f64")
    for fmt, m in hs.items():
        rec, Xf, _ = bench.solve(m, B, X0, tol=TOL, maxit=200)
        assert [r.status for r in rec] == [2, 0, 2, 2], fmt
        assert [r.iterations for r in rec] == [0, 0, 0, 0], fmt
        assert np.array_equal(bits(Xf[:M]), bits(X0)), fmt
        same_solve(rec, Xf[:M], bench.want(m, B, X0), ("-9", fmt))
        m.release()
    # diagonal 2: indefinite, found after one and after two updates
    hs = upload(G.lap2d(15, 17, -2), "f64")
    for fmt, m in hs.items():
        want = bench.want(m, B, X0)
        assert list(want.status) == [2, 0, 2, 2]
        assert list(want.iterations) == [1, 0, 1, 2]
        rec, Xf, _ = bench.solve(m, B, X0, tol=TOL, maxit=200)
        same_solve(rec, Xf[:M], want, ("-2", fmt))
        m.release()
    # one inf in column 0 of B: that column stops, the others never notice
    hs = upload(G.lap2d(15, 17, 0.5), "f64")
    Bi = B.copy()
    Bi[7, 0] = np.inf
    for fmt, m in hs.items():
        rec, Xf, _ = bench.solve(m, B, X0, tol=TOL, maxit=200)
        clean = as_solve(rec, Xf[:M])
        for ce in (1, 0):
            rec, Xf, _ = bench.solve(m, Bi, X0, tol=TOL, maxit=200,
                                     check_every=ce)
            assert rec[0].status == 2, (fmt, rec)
            assert [r.status for r in rec[1:]] == [0, 0, 0], (fmt, rec)
            assert ([r.iterations for r in rec[1:]]
                    == clean.iterations[1:]), fmt
            assert np.array_equal(bits(Xf[:M, 1:4]), bits(clean.X[:, 1:])), fmt
            for j in (1, 2, 3):
                assert bits(rec[j].rr) == bits(clean.rr[j]), (fmt, j)
            same_solve(rec, Xf[:M], bench.want(m, Bi, X0), ("inf", fmt))
        m.release()
    bench.free()


# ---------------------------------------------------------------- 5. refusals
def _rc(m, k, B, ldb, X, ldx, tol=TOL, maxit=10, check_every=0, work=None,
        work_bytes=0, info=True, opts=None, stream=None):
    rec = (S.CgInfo * 8)()
    return m._fn("cg")(m.h, opts, k, B, ldb, X, ldx, tol, maxit, check_every,
                       work, work_bytes, rec if info else None, stream), rec


def test_refusals_on_live_handles():
    mat = G.lap2d(37, 29, 0.5)
    M = mat[0]
    k = 4
    B, X0 = G.common_inputs(M)
    bench = CgBench(M)
    live = S._lib.spmv_live_handles()
    hs = upload(mat, "f64")
    d, cm = hs["csr"], hs["hll"]
    rm = d.to_hll(False)
    compact = cm.to_index16()
    # 1073 x 1074: the same rows, one more (empty) column
    A1 = S.csr_from_arrays("wide", M, M + 1, mat[1], mat[2], mat[3])
    d1 = S.CsrDevice.upload(A1)
    h1 = d1.to_hll(True)
    A0 = S.csr_from_arrays("norows", 0, 0, np.zeros(1, np.int32),
                           np.zeros(0, np.int32), np.zeros(0))
    d0 = S.CsrDevice.upload(A0)
    h0 = d0.to_hll(True)
    made = S._lib.spmv_live_handles()
    assert made == live + 8
    rec, Xf, _ = bench.solve(d, B, X0, tol=TOL, maxit=200)  # buffers filled
    good = as_solve(rec, Xf[:M])
    Bp, Xp = bench.B.ptr, bench.X.ptr
    einval = -errno.EINVAL
    need = S.cg_work_bytes(M, k)
    work = S.DevBuffer(need)
    for m in (d, cm):
        put(Xp, np.vstack([X0, np.zeros((PAST, k))]))
        assert _rc(m, k, Bp, 0, Xp, 0)[0] == 0  # opts may be NULL
        for bad in (0, 9):
            assert _rc(m, bad, Bp, 0, Xp, 0)[0] == einval
        assert _rc(m, k, Bp, 3, Xp, 0)[0] == einval
        assert _rc(m, k, Bp, 0, Xp, 3)[0] == einval
        assert _rc(m, k, None, 0, Xp, 0)[0] == einval
        assert _rc(m, k, Bp, 0, None, 0)[0] == einval
        assert _rc(m, k, Bp, 0, Xp, 0, info=False)[0] == einval
        for tol in (-1e-8, float("nan")):
            assert _rc(m, k, Bp, 0, Xp, 0, tol=tol)[0] == einval
        assert _rc(m, k, Bp, 0, Xp, 0, maxit=-1)[0] == einval
        assert _rc(m, k, Bp, 0, Xp, 0, check_every=-1)[0] == einval
        for bad in (dict(variant=1), dict(waves_per_block=17)):
            o = S._opts(**bad)
            assert _rc(m, k, Bp, 0, Xp, 0, opts=C.byref(o))[0] == einval, bad
        # a work buffer that is too short, or not 8-byte aligned
        assert _rc(m, k, Bp, 0, Xp, 0, work=work.ptr,
                   work_bytes=need - 1)[0] == einval
        assert _rc(m, k, Bp, 0, Xp, 0, work=work.ptr + 4,
                   work_bytes=need)[0] == einval
        assert S._lib.spmv_live_handles() == made
    assert _rc(compact, k, Bp, 0, Xp, 0)[0] == -errno.ENOTSUP
    assert _rc(rm, k, Bp, 0, Xp, 0)[0] == einval
    for m in (d1, h1):  # M != N
        assert _rc(m, k, Bp, 0, Xp, 0)[0] == einval
    # no rows: 0, every record zero
    for m in (d0, h0):
        rc, rec = _rc(m, k, Bp, 0, Xp, 0)
        assert rc == 0
        assert [(r.status, r.iterations, r.rr, r.bb) for r in rec[:k]] == \
            [(0, 0, 0.0, 0.0)] * k

    # maxit = 0: the first classification only, X untouched
    for m in (d, cm):
        rec, Xf, _ = bench.solve(m, B, X0, tol=TOL, maxit=0)
        assert [r.status for r in rec] == [1, 0, 1, 1]
        assert [r.iterations for r in rec] == [0, 0, 0, 0]
        assert np.array_equal(bits(Xf[:M]), bits(X0))
        assert [bits(r.bb) for r in rec] == [bits(b) for b in good.bb]

    # a capturing stream: -EBUSY, nothing enqueued, the capture ends cleanly
    side = S.Stream()
    for m in (d, cm):
        put(Xp, np.vstack([X0, np.zeros((PAST, k))]))
        S._check(S._lib.spmv_graph_begin_capture(side.ptr), "begin_capture")
        rc, _ = _rc(m, k, Bp, 0, Xp, 0, stream=side.ptr)
        rc_null, _ = _rc(m, k, Bp, 0, Xp, 0, work=work.ptr, work_bytes=need,
                         stream=side.ptr)
        g = C.c_void_p()
        end = S._lib.spmv_graph_end_capture(side.ptr, C.byref(g))
        if end == 0:
            S._check(S._lib.spmv_graph_destroy(g), "spmv_graph_destroy")
        assert rc == -errno.EBUSY and rc_null == -errno.EBUSY
        assert end == 0, "the capture was invalidated"
        got = bench.X.to_numpy(np.float64, M * k).reshape(M, k)
        assert np.array_equal(bits(got), bits(X0)), "something was enqueued"
        # ... and the stream solves afterwards
        rc, rec = _rc(m, k, Bp, 0, Xp, 0, maxit=200, stream=side.ptr)
        assert rc == 0 and [r.status for r in rec[:k]] == [0, 0, 0, 0]
    side.sync()

    # a solve that allocates its own work buffer gives it back
    S.device_sync()
    free0 = S.dev_mem_info()[0]
    put(Xp, np.vstack([X0, np.zeros((PAST, k))]))
    assert _rc(d, k, Bp, 0, Xp, 0, maxit=200)[0] == 0
    S.device_sync()
    assert S.dev_mem_info()[0] == free0

    # only the blocked copy left: no source arrays to multiply with
    for m in (d, cm):
        m.build_panels()
        m.release_source()
        assert _rc(m, k, Bp, 0, Xp, 0)[0] == -errno.ENODATA
        with pytest.raises(OSError) as ei:
            m.cg(Bp, Xp, k)
        assert ei.value.errno == errno.ENODATA
    S.stream_sync()
    for m in (d, cm, rm, compact, d1, h1, d0, h0):
        m.release()
    assert S._lib.spmv_csr_cg(C.c_void_p(1 << 20), None, k, Bp, 0, Xp, 0, TOL,
                              10, 0, None, 0, (S.CgInfo * 8)(),
                              None) == -errno.EBADF
    assert S._lib.spmv_live_handles() == live
    work.free()
    bench.free()
    S.csr_free(A0)
    S.csr_free(A1)
