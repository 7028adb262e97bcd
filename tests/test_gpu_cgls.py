"""CGLS on the device (spmv_*_cgls, spmv_engine.h) on the GPU: CSR pairs and
column-major HLL pairs (A, AT), AT from transpose(), f64 and f32 values, 1-8
interleaved problems, with and without damping.

The expected values come from the numpy restatement of the solver
(tests/_cgls.py), with Q = A P from A's launch_multi, S = AT R from AT's
launch_multi and the initial residual from A's launch_axpby, all with the same
opts.  numpy rounds every operation once, which is the contract, so the uint64
views of X are compared, and iterations, status and the bits of ss / atb / rr.
Every matrix but one is rectangular: B, R, Q have M rows and X, P, S have N
rows, so a kernel launched over the wrong length cannot pass.  The one
tolerance is the sanity line of test_gpu_cg: the true normal-equations residual
of the device's X, computed on the host, is at most 2 tol for a converged
column (the restatement reaches 0.99 tol on these inputs with the CPU oracle's
product; the factor 2 only keeps a wrong contract that still "matches itself"
from passing).

Inputs: tests/_cgls.py inputs (column 1 of B all zero, column 2 scaled by
1e-3, X0 zero except column 3).  Every test runs under a time limit of its own
(LIMIT_S): a test that exceeds it ends the whole process, so nothing else is
started on the device.
"""
import ctypes as C
import errno
import faulthandler

import numpy as np
import pytest

import _cgls as LS
import _oracle as O
import spmv_scpa_amd as S
from test_cgls import MATRICES
from test_gpu_cg import NWG, T, TOL, fill, put
from test_gpu_f32_values import round32
from test_gpu_multi_vector import FILL, PAST, bits

pytestmark = pytest.mark.gpu

LIMIT_S = 240
FIELDS = ("ss", "atb", "rr")


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def upload(mat, values="f64"):
    """-> {"csr": (A, AT), "hll": (A, AT)}: AT = A.transpose() on the device,
    the HLL pair made from the CSR pair (column-major)"""
    M, N, IRP, JA, AS = mat
    A = S.csr_from_arrays("cgls", M, N, IRP, JA, AS)
    d = S.CsrDevice.upload(A, values=values)
    S.csr_free(A)
    dt = d.transpose()
    assert (d.M, d.N, dt.M, dt.N) == (M, N, N, M)
    return {"csr": (d, dt), "hll": (d.to_hll(True), dt.to_hll(True))}


def release(hs):
    for pair in hs.values():
        for m in pair:
            m.release()


class LsBench:
    """device buffers of one M x N: B (M rows) and X (N rows) of the solver
    (sized for strides up to 8 + 3, PAST rows beyond the end and an 8-byte
    shift), and the vectors of both lengths the restatement multiplies with"""

    def __init__(self, M, N):
        self.M, self.N = M, N
        self.B = S.DevBuffer((M + PAST) * (8 + 3) * 8 + 8)
        self.X = S.DevBuffer((N + PAST) * (8 + 3) * 8 + 8)
        self.Vm, self.Vn = S.DevBuffer(M * 8 * 8), S.DevBuffer(N * 8 * 8)

    def callables(self, a, at, B, X0, **opts):
        """-> (product, product_t, residual0) on the pair, for restate()"""
        M, N, k = self.M, self.N, B.shape[1]

        def product(P):
            put(self.Vn.ptr, P)
            a.launch_multi(self.Vn.ptr, self.Vm.ptr, k, **opts)
            S.stream_sync()
            return self.Vm.to_numpy(np.float64, M * k).reshape(M, k)

        def product_t(R):
            put(self.Vm.ptr, R)
            at.launch_multi(self.Vm.ptr, self.Vn.ptr, k, **opts)
            S.stream_sync()
            return self.Vn.to_numpy(np.float64, N * k).reshape(N, k)

        def residual0():
            put(self.Vn.ptr, X0)
            put(self.Vm.ptr, B)
            a.launch_axpby(-1.0, 1.0, self.Vn.ptr, self.Vm.ptr, k, **opts)
            S.stream_sync()
            return self.Vm.to_numpy(np.float64, M * k).reshape(M, k)
        return product, product_t, residual0

    def want(self, a, at, B, X0, damp=0.0, tol=TOL, maxit=200, d2_path=True,
             **opts):
        product, product_t, residual0 = self.callables(a, at, B, X0, **opts)
        return LS.restate(product, product_t, residual0, B, X0, damp, tol,
                          maxit, d2_path=d2_path)

    def solve(self, a, at, B, X0, ldb=0, ldx=0, shift=0, **kw):
        """-> (records, whole X buffer as (N + PAST, ldx)): padding columns of
        B are NaN, those of X and the rows beyond the end of both hold the
        0xFF fill.  Asserts that B was not written"""
        M, N, k = self.M, self.N, B.shape[1]
        assert B.shape == (M, k) and X0.shape == (N, k)
        lb, lx = ldb or k, ldx or k
        Bh = np.full((M + PAST, lb), np.nan)
        bits(Bh)[M:] = FILL
        Bh[:M, :k] = B
        Xh = np.empty((N + PAST, lx))
        bits(Xh)[:] = FILL
        Xh[:N, :k] = X0
        fill(self.B)
        fill(self.X)
        put(self.B.ptr, Bh)
        put(self.X.ptr + shift, Xh)
        rec = a.cgls(at, self.B.ptr, self.X.ptr + shift, k, ldb=ldb, ldx=ldx,
                     **kw)
        S.stream_sync()
        Xf = self.X.to_numpy(np.float64, (N + PAST) * lx + shift // 8)
        Bf = self.B.to_numpy(np.float64, (M + PAST) * lb)
        assert np.array_equal(bits(Bf), bits(Bh.ravel())), "B was written"
        return rec, Xf[shift // 8:].reshape(N + PAST, lx)

    def free(self):
        for b in (self.B, self.X, self.Vm, self.Vn):
            b.free()


def same_solve(rec, X, want, tag):
    """a device solve against a restatement (or two device solves): bits"""
    k = len(rec)
    print(tag, "status", [r.status for r in rec], "iterations",
          [r.iterations for r in rec])
    assert [r.status for r in rec] == list(want.status), tag
    assert [r.iterations for r in rec] == list(want.iterations), tag
    for name in FIELDS:
        got = np.array([getattr(r, name) for r in rec])
        assert np.array_equal(bits(got), bits(getattr(want, name))), \
            (tag, name, got, getattr(want, name))
    same = bits(X[:, :k]) == bits(want.X)
    assert np.all(same), (tag, "elements of X that differ",
                          int(np.sum(~same)), np.argwhere(~same)[:4].tolist())


def as_solve(rec, X):
    k = len(rec)
    return LS.Solve(X[:, :k].copy(), [r.status for r in rec],
                    [r.iterations for r in rec],
                    *(np.array([getattr(r, f) for r in rec]) for f in FIELDS))


def column(base, j):
    return LS.Solve(base.X[:, j:j + 1], base.status[j:j + 1],
                    base.iterations[j:j + 1], base.ss[j:j + 1],
                    base.atb[j:j + 1], base.rr[j:j + 1])


def neighbours_kept(Xf, N, k, tag):
    assert np.all(bits(Xf[:N, k:]) == FILL), (tag, "columns beyond k")
    assert np.all(bits(Xf[N:]) == FILL), (tag, "rows beyond N")


# -------------------------------------------------------------------- 1. bits
#: the matrices of tests/test_cgls.py, and `long` in the other role: the pair
#: (AT, A) is the 257 x 600000 problem
CASES = [(name, values, False) for name in MATRICES for values in
         (("f64", "f32") if name in ("stacked(24,20,0,.5,1)",
                                     "wide(700,1500,3,5)",
                                     "arrow_rect(5000,3000,7)",
                                     "long(600000,257,2,9)") else ("f64",))]
CASES += [("long(600000,257,2,9)", "f64", True),
          ("arrow_rect(5000,3000,7)", "f64", True)]


@pytest.mark.parametrize("name,values,swap", CASES)
def test_a_solve_has_the_bits_of_the_restatement(name, values, swap):
    mat = MATRICES[name]()
    hs = upload(mat, values)
    if swap:  # the transpose is the matrix, the matrix its transpose
        mat = LS.transpose(mat)
        hs = {fmt: (at, a) for fmt, (a, at) in hs.items()}
    M, N, IRP, JA, AS = mat
    if name.startswith("long"):
        big, small = max(M, N), min(M, N)
        # one dot takes three sweeps of the slots, the other has two
        # workgroups with a one-row tail
        assert 2 * NWG * T < big <= 3 * NWG * T and small == T + 1
    stored = (M, N, IRP, JA, round32(AS) if values == "f32" else AS)
    B, X0 = LS.inputs(mat)
    bench = LsBench(M, N)
    for fmt, (a, at) in hs.items():
        for damp in (0.0, 0.5):
            tag = (name, values, swap, fmt, damp)
            want = bench.want(a, at, B, X0, damp)
            rec, Xf = bench.solve(a, at, B, X0, damp=damp, tol=TOL, maxit=200)
            same_solve(rec, Xf[:N], want, tag)
            neighbours_kept(Xf, N, 4, tag)
            # the zero column: converged at once, X untouched
            assert rec[1].status == 0 and rec[1].iterations == 0, tag
            assert rec[1].atb == 0.0 and rec[1].rr == 0.0, tag
            assert np.array_equal(bits(Xf[:N, 1]), bits(X0[:, 1])), tag
            assert all(r.iterations > 0 for r in (rec[0], rec[2], rec[3])), tag
            # the sanity line: the true residual of the converged columns
            res = LS.normal_residual(stored, O.csr_spmv, B, Xf[:N, :4], damp)
            print(tag, "normal residual", res)
            done = np.array([r.status == 0 for r in rec])
            assert np.all(res[done] <= 2 * TOL), (tag, res)
            if not name.startswith(("diff1d", "convdiff")) or damp:
                assert done.all(), tag   # (those two need more than 200)
            # stopped by maxit: every non-zero column after exactly 3 steps
            want3 = bench.want(a, at, B, X0, damp, maxit=3)
            rec, Xf = bench.solve(a, at, B, X0, damp=damp, tol=TOL, maxit=3)
            same_solve(rec, Xf[:N], want3, tag + ("maxit 3",))
            assert [r.status for r in rec] == [1, 0, 1, 1], tag
            assert [r.iterations for r in rec] == [3, 0, 3, 3], tag
            assert np.array_equal(bits(Xf[:N, 1]), bits(X0[:, 1])), tag
    release(hs)
    bench.free()


# ------------------------------------------------------------ 2. independence
@pytest.mark.parametrize("damp", [0.0, 0.5])
@pytest.mark.parametrize("name", ["stacked(33,31,0,.3,.5)",
                                  "wide(700,1500,3,5)"])
def test_the_result_depends_on_the_problem_alone(name, damp):
    mat = MATRICES[name]()
    M, N = mat[:2]
    B, X0 = LS.inputs(mat)
    bench = LsBench(M, N)
    hs = upload(mat)
    work = S.DevBuffer(S.cgls_work_bytes(M, N, 8))
    for fmt, (a, at) in hs.items():
        rec, Xf = bench.solve(a, at, B, X0, damp=damp, tol=TOL, maxit=200)
        base = as_solve(rec, Xf[:N])
        assert base.status == [0, 0, 0, 0]
        for kw in (dict(check_every=1), dict(check_every=5),
                   dict(check_every=8), dict(work=work),
                   dict(waves_per_block=1), dict(waves_per_block=4),
                   dict(waves_per_block=16)):
            rec, Xf = bench.solve(a, at, B, X0, damp=damp, tol=TOL, maxit=200,
                                  **kw)
            same_solve(rec, Xf[:N], base, (name, fmt, kw))
        # column j of the k = 4 solve is the k = 1 solve of that column
        for j in range(4):
            rec, Xf = bench.solve(a, at, B[:, j:j + 1], X0[:, j:j + 1],
                                  damp=damp, tol=TOL, maxit=200)
            same_solve(rec, Xf[:N], column(base, j), (name, fmt, "column", j))
            neighbours_kept(Xf, N, 1, (name, fmt, "column", j))
        # k = 8, columns 4-7 copies of columns 0-3, and the first k of them
        B8, X8 = np.hstack([B, B]), np.hstack([X0, X0])
        for k in (3, 5, 7, 8):
            rec, Xf = bench.solve(a, at, B8[:, :k], X8[:, :k], damp=damp,
                                  tol=TOL, maxit=200)
            neighbours_kept(Xf, N, k, (name, fmt, "k", k))
            for j in range(k):
                same_solve(rec[j:j + 1], Xf[:N, j:j + 1], column(base, j % 4),
                           (name, fmt, "k", k, "column", j))
    work.free()
    release(hs)
    bench.free()


# ----------------------------------------------------------------- 3. strides
class _Exactly:
    """`work` of exactly n bytes at the head of a larger allocation"""

    def __init__(self, buf, n):
        self.ptr, self.nbytes = buf.ptr, n


@pytest.mark.parametrize("damp", [0.0, 0.5])
@pytest.mark.parametrize("name", ["stacked(24,20,0,.5,1)",
                                  "wide(700,1500,3,5)"])
def test_strides_an_unaligned_X_and_the_neighbours(name, damp):
    mat = MATRICES[name]()
    M, N = mat[:2]
    k = 4
    B, X0 = LS.inputs(mat)
    bench = LsBench(M, N)
    hs = upload(mat)
    need = S.cgls_work_bytes(M, N, k)
    guard = 4096
    work = S.DevBuffer(need + guard)
    for fmt, (a, at) in hs.items():
        tag = (name, damp, fmt)
        want = bench.want(a, at, B, X0, damp)
        S._check(S._lib.spmv_dev_memset(work.ptr, 0xA5, work.nbytes, None),
                 "spmv_dev_memset")
        # ldx = k + 1: a column of X that is not the solver's; ldb = k + 3:
        # NaN padding in B; X 8 bytes off 16; rows beyond the end of both;
        # solve() checks that B keeps its bits
        rec, Xf = bench.solve(a, at, B, X0, ldb=k + 3, ldx=k + 1, shift=8,
                              damp=damp, tol=TOL, maxit=200,
                              work=_Exactly(work, need))
        same_solve(rec, Xf[:N], want, tag)
        assert [r.status for r in rec] == [0, 0, 0, 0], tag
        neighbours_kept(Xf, N, k, tag)
        tail = work.to_numpy(np.uint8, need + guard)[need:]
        assert np.all(tail == 0xA5), (tag, "bytes behind the work buffer")
    work.free()
    release(hs)
    bench.free()


# ----------------------------------------------------------------- 4. damping
@pytest.mark.parametrize("name", ["stacked(24,20,0,.5,1)",
                                  "wide(700,1500,3,5)"])
def test_damp_zero_has_no_d2_term(name):
    mat = MATRICES[name]()
    M, N = mat[:2]
    B, X0 = LS.inputs(mat)
    bench = LsBench(M, N)
    hs = upload(mat)
    for fmt, (a, at) in hs.items():
        for maxit in (200, 3):
            # the loop written without the term, whatever `damp` says
            want = bench.want(a, at, B, X0, 0.5, maxit=maxit, d2_path=False)
            rec, Xf = bench.solve(a, at, B, X0, damp=0.0, tol=TOL,
                                  maxit=maxit)
            same_solve(rec, Xf[:N], want, (name, fmt, maxit))
        # ... and the damped solve is another one
        rec5, Xf5 = bench.solve(a, at, B, X0, damp=0.5, tol=TOL, maxit=3)
        assert not np.array_equal(bits(Xf5[:N, 0]), bits(Xf[:N, 0]))
    release(hs)
    bench.free()


# ---------------------------------------------------------------- 5. statuses
def test_a_breakdown_is_a_status_not_a_fault():
    good = MATRICES["stacked(24,20,0,.5,1)"]()
    Mg, Ng = good[:2]
    Bg, Xg = LS.inputs(good)
    gbench = LsBench(Mg, Ng)
    ghs = upload(good)
    clean = {}
    for fmt, (a, at) in ghs.items():
        rec, Xf = gbench.solve(a, at, Bg, Xg, tol=TOL, maxit=200)
        clean[fmt] = as_solve(rec, Xf[:Ng])
        assert clean[fmt].status == [0, 0, 0, 0]

    def still_solves(tag):
        for fmt, (a, at) in ghs.items():
            rec, Xf = gbench.solve(a, at, Bg, Xg, tol=TOL, maxit=200)
            same_solve(rec, Xf[:Ng], clean[fmt], (tag, "clean solve", fmt))

    # the rules at 70 x 70, k = 2, X0 = 0
    n = 70
    Br = np.random.default_rng(2).uniform(-1, 1, (n, 2))
    orth = LS._rect(2, 1, [0, 1], [0, 0], [1.0, 1.0])
    for tag, mat, B, status, iters in (
            # ss = 4 b.b, delta = 16 b.b: alpha = 1/4, X = B / 2, R = 0
            ("2 I", LS.diagm(np.full(n, 2.0)), Br, [0, 0], [1, 1]),
            # b orthogonal to the range: atb = 0, converged at once
            ("orthogonal", orth, np.array([[1.0, 2.0], [-1.0, -2.0]]),
             [0, 0], [0, 0]),
            # atb overflows
            ("1e200 I", LS.diagm(np.full(n, 1e200)), np.ones((n, 2)),
             [2, 2], [0, 0]),
            # Q.Q underflows to 0: delta == 0
            ("1e-120 I", LS.diagm(np.full(n, 1e-120)), np.full((n, 2), 1e40),
             [2, 2], [0, 0])):
        M, N = mat[:2]
        X0 = np.zeros((N, 2))
        bench = LsBench(M, N)
        hs = upload(mat)
        for fmt, (a, at) in hs.items():
            want = bench.want(a, at, B, X0)
            assert list(want.status) == status, (tag, fmt)
            assert list(want.iterations) == iters, (tag, fmt)
            for ce in (0, 1):
                rec, Xf = bench.solve(a, at, B, X0, tol=TOL, maxit=200,
                                      check_every=ce)
                same_solve(rec, Xf[:N], want, (tag, fmt, ce))
                neighbours_kept(Xf, N, 2, (tag, fmt, ce))
                if tag == "2 I":
                    assert [r.ss for r in rec] == [0.0, 0.0], fmt
                    assert [r.rr for r in rec] == [0.0, 0.0], fmt
                    assert np.array_equal(bits(Xf[:N]), bits(B / 2)), fmt
                else:
                    assert np.array_equal(bits(Xf[:N]), bits(X0)), (tag, fmt)
                if tag == "orthogonal":
                    assert [r.atb for r in rec] == [0.0, 0.0], fmt
                    assert [r.rr for r in rec] == [2.0, 8.0], fmt
                if tag == "1e200 I":
                    assert all(np.isinf(r.atb) for r in rec), fmt
        release(hs)
        bench.free()
        still_solves(tag)

    # one NaN in column 0 of B: that column stops before its first step and
    # keeps its X, the others never notice
    Bn = Bg.copy()
    Bn[7, 0] = np.nan
    for fmt, (a, at) in ghs.items():
        for damp in (0.0, 0.5):
            cl, Xc = gbench.solve(a, at, Bg, Xg, damp=damp, tol=TOL, maxit=200)
            cl = as_solve(cl, Xc[:Ng])
            for ce in (1, 0):
                rec, Xf = gbench.solve(a, at, Bn, Xg, damp=damp, tol=TOL,
                                       maxit=200, check_every=ce)
                assert rec[0].status == 2 and rec[0].iterations == 0, (fmt, rec)
                assert np.array_equal(bits(Xf[:Ng, 0]), bits(Xg[:, 0])), fmt
                for j in (1, 2, 3):
                    same_solve(rec[j:j + 1], Xf[:Ng, j:j + 1], column(cl, j),
                               ("nan", fmt, damp, ce, j))
            # (the sums of column 0 are NaN: which NaN is not compared)
            assert all(np.isnan(v) for v in (rec[0].ss, rec[0].atb, rec[0].rr))
            want = gbench.want(a, at, Bn, Xg, damp)
            assert want.status[0] == 2 and want.iterations[0] == 0
            for j in (1, 2, 3):
                same_solve(rec[j:j + 1], Xf[:Ng, j:j + 1], column(want, j),
                           ("nan", fmt, damp, "restatement", j))
    still_solves("nan in B")
    release(ghs)
    gbench.free()


# ---------------------------------------------------------------- 6. refusals
def _rc(a, at, k, B, ldb, X, ldx, damp=0.0, tol=TOL, maxit=10, check_every=0,
        work=None, work_bytes=0, info=True, opts=None, stream=None):
    rec = (S.CglsInfo * 8)()
    ath = at.h if isinstance(at, S._Device) else at
    return a._fn("cgls")(a.h, ath, opts, k, B, ldb, X, ldx, damp, tol, maxit,
                         check_every, work, work_bytes,
                         rec if info else None, stream), rec


def test_refusals_on_live_handles():
    mat = MATRICES["stacked(24,20,0,.5,1)"]()
    M, N = mat[:2]
    k = 4
    B, X0 = LS.inputs(mat)
    bench = LsBench(M, N)
    live = S._lib.spmv_live_handles()
    hs = upload(mat)
    (d, dt), (cm, cmt) = hs["csr"], hs["hll"]
    rm, rmt = d.to_hll(False), dt.to_hll(False)
    compact, compact_t = cm.to_index16(), cmt.to_index16()
    # 960 x 481: the same rows, one more (empty) column
    A1 = S.csr_from_arrays("wider", M, N + 1, mat[2], mat[3], mat[4])
    d1 = S.CsrDevice.upload(A1)
    h1 = d1.to_hll(True)
    S.csr_free(A1)
    empty = np.zeros(0, np.int32), np.zeros(0)
    A0 = S.csr_from_arrays("norows", 0, 0, np.zeros(1, np.int32), *empty)
    d0 = S.CsrDevice.upload(A0)
    h0 = d0.to_hll(True)
    S.csr_free(A0)
    A05 = S.csr_from_arrays("0 x 5", 0, 5, np.zeros(1, np.int32), *empty)
    d05 = S.CsrDevice.upload(A05)
    d50 = d05.transpose()
    S.csr_free(A05)
    extra = (rm, rmt, compact, compact_t, d1, h1, d0, h0, d05, d50)
    made = S._lib.spmv_live_handles()
    assert made == live + 4 + len(extra)
    rec, Xf = bench.solve(d, dt, B, X0, tol=TOL, maxit=200)
    assert [r.status for r in rec] == [0, 0, 0, 0]   # the buffers are filled
    Bp, Xp = bench.B.ptr, bench.X.ptr
    einval = -errno.EINVAL
    need = S.cgls_work_bytes(M, N, k)
    work = S.DevBuffer(need)
    for a, at in ((d, dt), (cm, cmt)):
        put(Xp, np.vstack([X0, np.zeros((PAST, k))]))
        assert _rc(a, at, k, Bp, 0, Xp, 0)[0] == 0  # opts may be NULL
        for bad in (0, 9):
            assert _rc(a, at, bad, Bp, 0, Xp, 0)[0] == einval
        assert _rc(a, at, k, Bp, 3, Xp, 0)[0] == einval
        assert _rc(a, at, k, Bp, 0, Xp, 3)[0] == einval
        assert _rc(a, at, k, None, 0, Xp, 0)[0] == einval
        assert _rc(a, at, k, Bp, 0, None, 0)[0] == einval
        assert _rc(a, at, k, Bp, 0, Xp, 0, info=False)[0] == einval
        for bad in (-1e-8, float("nan")):
            assert _rc(a, at, k, Bp, 0, Xp, 0, tol=bad)[0] == einval
            assert _rc(a, at, k, Bp, 0, Xp, 0, damp=bad)[0] == einval
        assert _rc(a, at, k, Bp, 0, Xp, 0, maxit=-1)[0] == einval
        assert _rc(a, at, k, Bp, 0, Xp, 0, check_every=-1)[0] == einval
        for bad in (dict(variant=1), dict(waves_per_block=17)):
            o = S._opts(**bad)
            assert _rc(a, at, k, Bp, 0, Xp, 0, opts=C.byref(o))[0] == einval
        # a work buffer one byte short, or not 8-byte aligned
        assert _rc(a, at, k, Bp, 0, Xp, 0, work=work.ptr,
                   work_bytes=need - 1)[0] == einval
        assert _rc(a, at, k, Bp, 0, Xp, 0, work=work.ptr + 4,
                   work_bytes=need)[0] == einval
        assert _rc(a, at, k, Bp, 0, Xp, 0, work=work.ptr,
                   work_bytes=need)[0] == 0
        # the shapes: the matrix or the transpose in both places (the
        # swapped pair (AT, A) is a valid problem of its own: test 1)
        assert _rc(a, a, k, Bp, 0, Xp, 0)[0] == einval
        assert _rc(at, at, k, Bp, 0, Xp, 0)[0] == einval
        # the second handle: NULL, and a pointer that is no handle
        assert _rc(a, None, k, Bp, 0, Xp, 0)[0] == einval
        assert _rc(a, C.c_void_p(1 << 20), k, Bp, 0, Xp, 0)[0] == -errno.EBADF
        assert S._lib.spmv_live_handles() == made
    # 960 x 481 against 480 x 960
    assert _rc(d1, dt, k, Bp, 0, Xp, 0)[0] == einval
    assert _rc(dt, d1, k, Bp, 0, Xp, 0)[0] == einval
    assert _rc(h1, cmt, k, Bp, 0, Xp, 0)[0] == einval
    # a compact or a row-major handle, in either position
    assert _rc(compact, cmt, k, Bp, 0, Xp, 0)[0] == -errno.ENOTSUP
    assert _rc(cm, compact_t, k, Bp, 0, Xp, 0)[0] == -errno.ENOTSUP
    assert _rc(rm, cmt, k, Bp, 0, Xp, 0)[0] == einval
    assert _rc(cm, rmt, k, Bp, 0, Xp, 0)[0] == einval
    # the wrapper: a CSR matrix with an HLL transpose
    with pytest.raises(TypeError):
        d.cgls(cmt, Bp, Xp, k)
    # no rows or no columns: 0, every record zero, nothing enqueued
    put(Xp, np.vstack([X0, np.zeros((PAST, k))]))
    for a, at in ((d0, d0), (h0, h0), (d05, d50), (d50, d05)):
        rc, rec = _rc(a, at, k, Bp, 0, Xp, 0)
        assert rc == 0
        assert [(r.status, r.iterations, r.ss, r.atb, r.rr)
                for r in rec[:k]] == [(0, 0, 0.0, 0.0, 0.0)] * k
    S.stream_sync()
    got = bench.X.to_numpy(np.float64, N * k).reshape(N, k)
    assert np.array_equal(bits(got), bits(X0)), "something was enqueued"
    assert S._lib.spmv_live_handles() == made

    # a capturing stream: -EBUSY, nothing enqueued, the capture ends cleanly
    side = S.Stream()
    for a, at in ((d, dt), (cm, cmt)):
        put(Xp, np.vstack([X0, np.zeros((PAST, k))]))
        S._check(S._lib.spmv_graph_begin_capture(side.ptr), "begin_capture")
        rc, _ = _rc(a, at, k, Bp, 0, Xp, 0, stream=side.ptr)
        rc_own, _ = _rc(a, at, k, Bp, 0, Xp, 0, damp=0.5, work=work.ptr,
                        work_bytes=need, stream=side.ptr)
        g = C.c_void_p()
        end = S._lib.spmv_graph_end_capture(side.ptr, C.byref(g))
        if end == 0:
            S._check(S._lib.spmv_graph_destroy(g), "spmv_graph_destroy")
        assert rc == -errno.EBUSY and rc_own == -errno.EBUSY
        assert end == 0, "the capture was invalidated"
        got = bench.X.to_numpy(np.float64, N * k).reshape(N, k)
        assert np.array_equal(bits(got), bits(X0)), "something was enqueued"
        # ... and the stream solves afterwards
        rc, rec = _rc(a, at, k, Bp, 0, Xp, 0, maxit=200, stream=side.ptr)
        assert rc == 0 and [r.status for r in rec[:k]] == [0, 0, 0, 0]
    side.sync()

    # only the blocked copy left in one of the two: no source arrays to read
    for a, at in ((d, dt), (cmt, cm)):
        a.build_panels()
        a.release_source()
        assert _rc(a, at, k, Bp, 0, Xp, 0)[0] == -errno.ENODATA
        assert _rc(at, a, k, Bp, 0, Xp, 0)[0] == -errno.ENODATA
        with pytest.raises(OSError) as ei:
            at.cgls(a, Bp, Xp, k)
        assert ei.value.errno == errno.ENODATA
    S.stream_sync()
    assert S._lib.spmv_live_handles() == made
    release(hs)
    for m in extra:
        m.release()
    assert S._lib.spmv_csr_cgls(C.c_void_p(1 << 20), C.c_void_p(1 << 20),
                                None, k, Bp, 0, Xp, 0, 0.0, TOL, 10, 0, None,
                                0, (S.CglsInfo * 8)(), None) == -errno.EBADF
    assert S._lib.spmv_live_handles() == live
    work.free()
    bench.free()
