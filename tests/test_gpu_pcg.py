"""Preconditioned CG and the diagonal of a handle (spmv_*_pcg, spmv_*_diag;
spmv_engine.h) on the GPU: CSR and column-major HLL handles, f64 and f32
values, 1-8 interleaved systems.

Everything is compared as uint64: the diagonal against tests/_pcg.py diag_of,
a solve against the numpy restatement (tests/_pcg.py restate) fed with Q = A P
from the SAME handle's launch_multi, the initial residual from its launch_axpby
and minv from its diag(invert=True); a solve with minv = 1 against cg() on the
same handle.  The one tolerance is the sanity line of test_gpu_cg: the true
residual of the device's X, computed on the host, is at most 2 tol (numpy
reached 0.99 tol on these inputs).

Inputs: tests/_cg.py common_inputs (column 1 all zero, column 2 scaled by 1e-3,
X0 zero except column 3).  Every test runs under a time limit of its own
(LIMIT_S): a test that exceeds it ends the whole process, so nothing else is
started on the device.
"""
import ctypes as C
import errno
import faulthandler

import numpy as np
import pytest

import _cg as G
import _oracle as O
import _pcg as PG
import spmv_scpa_amd as S
from test_gpu_cg import (BIG_NX, BIG_NY, MATRICES, NWG, T, TOL, CgBench,
                         as_solve, fill, neighbours_kept, put, same_solve,
                         upload)
from test_gpu_f32_values import round32
from test_gpu_multi_vector import FILL, PAST, bits, handles

pytestmark = pytest.mark.gpu

LIMIT_S = 240
SCALED = {
    "scaled(15,17)": lambda: PG.scaled_lap2d(15, 17, 0.5, 6, 7),
    "scaled(37,29)": lambda: PG.scaled_lap2d(37, 29, 0.5, 6, 7),
    "arrow(4099,3)": lambda: G.arrow(4099, 3),
    "scaled(big)": lambda: PG.scaled_lap2d(BIG_NX, BIG_NY, 0.5, 6, 7),
}


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


class PcgBench(CgBench):
    """CgBench and a minv buffer (M + PAST doubles)"""

    def __init__(self, M):
        CgBench.__init__(self, M)
        self.minv = S.DevBuffer((M + PAST) * 8)

    def set_minv(self, v):
        """minv = v (M values), the PAST doubles behind it the 0xFF fill"""
        h = np.empty(self.M + PAST)
        bits(h)[:] = FILL
        h[:self.M] = v
        put(self.minv.ptr, h)
        return h[:self.M].copy()

    def jacobi(self, m):
        """minv = diag(invert=True) of handle m -> its values"""
        fill(self.minv)
        m.diag(self.minv.ptr, invert=True)
        S.stream_sync()
        return self.minv.to_numpy(np.float64, self.M)

    def want(self, m, B, X0, minv, tol=TOL, maxit=200, **opts):
        product, residual0 = self.callables(m, B, X0, **opts)
        return PG.restate(product, residual0, B, X0, minv, tol, maxit)

    def solve(self, m, B, X0, ldb=0, ldx=0, shift=0, plain=False, **kw):
        """as CgBench.solve, through pcg() with the minv buffer as it stands
        (plain=True: through cg()); asserts that minv was not written"""
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
        before = self.minv.to_numpy(np.uint64, M + PAST)
        if plain:
            rec = m.cg(self.B.ptr, self.X.ptr + shift, k, ldb=ldb, ldx=ldx,
                       **kw)
        else:
            rec = m.pcg(self.B.ptr, self.X.ptr + shift, self.minv.ptr, k,
                        ldb=ldb, ldx=ldx, **kw)
        S.stream_sync()
        Xf = self.X.to_numpy(np.float64, (M + PAST) * lx + shift // 8)
        Bf = self.B.to_numpy(np.float64, (M + PAST) * lb)
        assert np.array_equal(bits(Bf), bits(Bh.ravel())), "B was written"
        assert np.array_equal(self.minv.to_numpy(np.uint64, M + PAST),
                              before), "minv was written"
        return rec, Xf[shift // 8:].reshape(M + PAST, lx), Bh

    def free(self):
        CgBench.free(self)
        self.minv.free()


# ---------------------------------------------------------------- 1. diagonal
def hand_made(N=70):
    """70 x N: rows 3, 20, 33 store no diagonal; rows 5, 37 store it twice
    (0.25, 0.5), rows 11, 64 three times (0.5, 2.0, 0.25) -- sums that are
    exact in any order; row 40 holds nine off-diagonals only; row 50 is empty;
    in a 70 x 50 matrix the rows from 50 on have no diagonal to store"""
    M = 70
    rng = np.random.default_rng(5)
    rows, cols, vals = [], [], []
    for r in range(M):
        if r == 50:
            continue
        offs = ((r + 1 + np.arange(9) * 5) % N if r == 40
                else np.array([(r + 1) % N, (r + 7) % N]))
        offs = offs[offs != r]
        dg = ([] if r in (3, 20, 33, 40) or r >= N
              else [0.25, 0.5] if r in (5, 37)
              else [0.5, 2.0, 0.25] if r in (11, 64)
              else [0.75 * (r % 5 + 1)])
        rows += [r] * (len(offs) + len(dg))
        cols += list(offs) + [r] * len(dg)
        vals += list(rng.uniform(-1.0, 1.0, len(offs))) + dg
    rows, cols, vals = np.array(rows), np.array(cols), np.array(vals)
    order = np.argsort(rows * N + cols, kind="stable")  # duplicates in order
    IRP = np.zeros(M + 1, np.int32)
    IRP[1:] = np.cumsum(np.bincount(rows, minlength=M))
    return (M, IRP, np.ascontiguousarray(cols[order], np.int32),
            np.ascontiguousarray(vals[order]))


DIAG_CASES = {
    "lap2d(1,1,0.5)": lambda: G.lap2d(1, 1, 0.5) + (1,),
    "lap2d(37,29,0.5)": lambda: G.lap2d(37, 29, 0.5) + (1073,),
    "arrow(4099,3)": lambda: G.arrow(4099, 3) + (4099,),
    "hand-made 70x70": lambda: hand_made(70) + (70,),
    "hand-made 70x50": lambda: hand_made(50) + (50,),
}


@pytest.mark.parametrize("values", ["f64", "f32"])
@pytest.mark.parametrize("name", list(DIAG_CASES))
def test_the_diagonal_has_the_bits_of_the_host_s(name, values):
    M, IRP, JA, AS, N = DIAG_CASES[name]()
    n = min(M, N)
    stored = round32(AS) if values == "f32" else AS
    d = PG.diag_of(M, IRP, JA, stored, N)
    with np.errstate(divide="ignore"):
        inv = 1.0 / d
    if name.startswith("arrow"):
        assert IRP[1] == M > 2048   # a CSR long row, a wide hack block
    if name.startswith("hand-made"):
        assert np.sum(d == 0.0) == (5 if N == 70 else 4) and n == N
        assert d[5] == 0.75 and d[11] == 2.75 and np.isinf(inv[3])
        assert IRP[51] == IRP[50] and IRP[41] - IRP[40] == 9
    A = S.csr_from_arrays("diag", M, N, IRP, JA, AS)
    hs = handles(A, values)
    out = S.DevBuffer((M + PAST) * 8)
    side = S.Stream()
    for fmt, m in hs.items():
        for invert, want in ((False, d), (True, inv)):
            tag = (name, values, fmt, invert)
            fill(out)
            m.diag(out.ptr, invert=invert)
            S.stream_sync()
            got = out.to_numpy(np.float64, M + PAST)
            same = bits(got[:n]) == bits(want)
            assert np.all(same), (tag, "rows that differ",
                                  np.flatnonzero(~same)[:8].tolist(),
                                  got[:n][~same][:4], want[~same][:4])
            assert np.all(bits(got[n:]) == FILL), (tag, "beyond min(M, N)")
            # captured into a graph and replayed: the same bits
            with side.capture() as g:
                m.diag(out.ptr, invert=invert, stream=side.ptr)
            for rep in range(2):
                S._check(S._lib.spmv_dev_memset(out.ptr, 0xFF, out.nbytes,
                                                side.ptr), "spmv_dev_memset")
                g.launch(side.ptr)
                side.sync()
                again = out.to_numpy(np.float64, M + PAST)
                assert np.array_equal(bits(again), bits(got)), (tag, rep)
            g.destroy()
    for m in hs.values():
        m.release()
    out.free()
    S.csr_free(A)


# ------------------------------------------------------------ 2. minv = 1: cg
@pytest.mark.parametrize("name", list(MATRICES))
def test_a_preconditioner_of_ones_returns_the_bits_of_cg(name):
    mat = MATRICES[name]()
    M = mat[0]
    B, X0 = G.common_inputs(M)
    bench = PcgBench(M)
    bench.set_minv(np.ones(M))
    hs = upload(mat, "f64")
    for fmt, m in hs.items():
        for maxit in (200, 7):
            rec, Xf, _ = bench.solve(m, B, X0, tol=TOL, maxit=maxit,
                                     plain=True)
            plain = as_solve(rec, Xf[:M])
            rec, Xf, _ = bench.solve(m, B, X0, tol=TOL, maxit=maxit)
            same_solve(rec, Xf[:M], plain, (name, fmt, maxit))
            neighbours_kept(Xf, M, 4, (name, fmt, maxit))
    for m in hs.values():
        m.release()
    bench.free()


# ------------------------------------------------------------------ 3. Jacobi
@pytest.mark.parametrize("values", ["f64", "f32"])
@pytest.mark.parametrize("name", list(SCALED))
def test_a_jacobi_solve_has_the_bits_of_the_restatement(name, values):
    mat = SCALED[name]()
    M, IRP, JA, AS = mat
    if name == "scaled(big)":
        assert NWG * T < M <= NWG * T + BIG_NX
    stored = round32(AS) if values == "f32" else AS
    B, X0 = G.common_inputs(M)
    bench = PcgBench(M)
    hs = upload(mat, values)
    with np.errstate(divide="ignore"):
        inv = 1.0 / PG.diag_of(M, IRP, JA, stored)
    for fmt, m in hs.items():
        tag = (name, values, fmt)
        minv = bench.jacobi(m)
        assert np.array_equal(bits(minv), bits(inv)), tag
        want = bench.want(m, B, X0, minv)
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
        pre_iters = [r.iterations for r in rec]
        # stopped by maxit
        want5 = bench.want(m, B, X0, minv, maxit=5)
        rec, Xf, _ = bench.solve(m, B, X0, tol=TOL, maxit=5)
        same_solve(rec, Xf[:M], want5, tag + ("maxit 5",))
        if name.startswith("scaled"):
            # (Jacobi leaves the arrow three distinct eigenvalues: it is
            # solved before the fifth update)
            assert [r.status for r in rec] == [1, 0, 1, 1], tag
            assert [r.iterations for r in rec] == [5, 0, 5, 5], tag
        if name == "scaled(37,29)":
            # what the preconditioner is for: a quarter of cg()'s iterations
            rec, Xf, _ = bench.solve(m, B, X0, tol=TOL, maxit=2000,
                                     plain=True)
            plain_iters = [r.iterations for r in rec]
            print(tag, "iterations: pcg", pre_iters, "cg", plain_iters)
            assert [r.status for r in rec] == [0, 0, 0, 0], tag
            for j in (0, 2, 3):
                assert 0 < 4 * pre_iters[j] <= plain_iters[j], (tag, j)
    for m in hs.values():
        m.release()
    bench.free()


# ------------------------------------------------------------ 4. independence
@pytest.mark.parametrize("name", ["scaled(37,29)", "arrow(4099,3)"])
def test_the_result_depends_on_the_system_alone(name):
    mat = SCALED[name]()
    M = mat[0]
    bench = PcgBench(M)
    hs = upload(mat, "f64")
    work = S.DevBuffer(S.pcg_work_bytes(M, 8))
    for fmt, m in hs.items():
        bench.jacobi(m)
        for k in (4, 8, 3):
            B, X0 = G.common_inputs(M, k)
            rec, Xf, _ = bench.solve(m, B, X0, tol=TOL, maxit=200)
            base = as_solve(rec, Xf[:M])
            neighbours_kept(Xf, M, k, (name, fmt, "k", k))
            assert base.status == [0] * k
            if k == 4:
                for kw in (dict(check_every=1), dict(check_every=3),
                           dict(check_every=0), dict(work=work),
                           dict(waves_per_block=1), dict(waves_per_block=8)):
                    rec, Xf, _ = bench.solve(m, B, X0, tol=TOL, maxit=200,
                                             **kw)
                    same_solve(rec, Xf[:M], base, (name, fmt, kw))
            # column j of the k-column solve is the k = 1 solve of that column
            for j in range(k):
                rec, Xf, _ = bench.solve(m, B[:, j:j + 1], X0[:, j:j + 1],
                                         tol=TOL, maxit=200)
                one = G.Solve(base.X[:, j:j + 1], base.status[j:j + 1],
                              base.iterations[j:j + 1], base.rr[j:j + 1],
                              base.bb[j:j + 1])
                same_solve(rec, Xf[:M], one, (name, fmt, "k", k, "column", j))
    work.free()
    for m in hs.values():
        m.release()
    bench.free()


# ----------------------------------------------------------------- 5. strides
class _Exactly:
    """`work` of exactly n bytes at the head of a larger allocation"""

    def __init__(self, buf, n):
        self.ptr, self.nbytes = buf.ptr, n


@pytest.mark.parametrize("values", ["f64", "f32"])
def test_strides_an_unaligned_X_and_the_neighbours(values):
    mat = SCALED["scaled(37,29)"]()
    M = mat[0]
    k = 4
    B, X0 = G.common_inputs(M)
    bench = PcgBench(M)
    hs = upload(mat, values)
    need = S.pcg_work_bytes(M, k)
    guard = 4096
    work = S.DevBuffer(need + guard)
    for fmt, m in hs.items():
        tag = (values, fmt)
        minv = bench.jacobi(m)
        want = bench.want(m, B, X0, minv)
        S._check(S._lib.spmv_dev_memset(work.ptr, 0xA5, work.nbytes, None),
                 "spmv_dev_memset")
        # ldx = k + 2: columns of X that are not the solver's; ldb = k + 3:
        # NaN padding in B; X 8 bytes off 16; rows beyond M of both; solve()
        # checks that B and minv (and the fill behind minv) keep their bits
        rec, Xf, _ = bench.solve(m, B, X0, ldb=k + 3, ldx=k + 2, shift=8,
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


# ---------------------------------------------------------------- 6. statuses
def test_a_breakdown_is_a_status_not_a_fault():
    M, IRP, JA, AS = G.lap2d(15, 17, 0.5)
    B, X0 = G.common_inputs(M)
    bench = PcgBench(M)
    # row 9 stores no diagonal: minv[9] = inf, r.z is inf or (the zero column:
    # inf * 0) NaN -- every column breaks down before the first update
    rows = np.repeat(np.arange(M), np.diff(IRP))
    keep = ~((rows == 9) & (JA == 9))
    IRP0 = np.zeros(M + 1, np.int32)
    IRP0[1:] = np.cumsum(np.bincount(rows[keep], minlength=M))
    hs = upload((M, IRP0, JA[keep], AS[keep]), "f64")
    for fmt, m in hs.items():
        minv = bench.jacobi(m)
        assert np.isinf(minv[9]) and np.sum(np.isinf(minv)) == 1, fmt
        rec, Xf, _ = bench.solve(m, B, X0, tol=TOL, maxit=200)
        assert [r.status for r in rec] == [2, 2, 2, 2], fmt
        assert [r.iterations for r in rec] == [0, 0, 0, 0], fmt
        assert np.array_equal(bits(Xf[:M]), bits(X0)), fmt
        same_solve(rec, Xf[:M], bench.want(m, B, X0, minv), ("inf", fmt))
        m.release()
    hs = upload((M, IRP, JA, AS), "f64")
    Bn = B.copy()
    Bn[7, 0] = np.nan
    for fmt, m in hs.items():
        # minv = -1 everywhere: r.z < 0 at the start
        minv = bench.set_minv(-np.ones(M))
        rec, Xf, _ = bench.solve(m, B, X0, tol=TOL, maxit=200)
        assert [r.status for r in rec] == [2, 0, 2, 2], fmt
        assert [r.iterations for r in rec] == [0, 0, 0, 0], fmt
        assert np.array_equal(bits(Xf[:M]), bits(X0)), fmt
        same_solve(rec, Xf[:M], bench.want(m, B, X0, minv), ("-1", fmt))
        # one NaN in column 0 of B: that column stops, the others never notice
        minv = bench.jacobi(m)
        rec, Xf, _ = bench.solve(m, B, X0, tol=TOL, maxit=200)
        clean = as_solve(rec, Xf[:M])
        assert clean.status == [0, 0, 0, 0]
        for ce in (1, 0):
            rec, Xf, _ = bench.solve(m, Bn, X0, tol=TOL, maxit=200,
                                     check_every=ce)
            assert rec[0].status == 2 and rec[0].iterations == 0, (fmt, rec)
            assert [r.status for r in rec[1:]] == [0, 0, 0], (fmt, rec)
            assert ([r.iterations for r in rec[1:]]
                    == clean.iterations[1:]), fmt
            assert np.array_equal(bits(Xf[:M, 1:4]), bits(clean.X[:, 1:])), fmt
            for j in (1, 2, 3):
                assert bits(rec[j].rr) == bits(clean.rr[j]), (fmt, j)
            same_solve(rec, Xf[:M], bench.want(m, Bn, X0, minv), ("nan", fmt))
        m.release()
    # indefinite matrices: p.Ap <= 0, at once (diagonal -5) and after one and
    # two updates (diagonal 2), as test_gpu_cg -- under Jacobi's uniform 1/2,
    # and under minv = 1
    hs = upload(G.lap2d(15, 17, -9), "f64")
    for fmt, m in hs.items():
        minv = bench.set_minv(np.ones(M))
        rec, Xf, _ = bench.solve(m, B, X0, tol=TOL, maxit=200)
        assert [r.status for r in rec] == [2, 0, 2, 2], fmt
        assert [r.iterations for r in rec] == [0, 0, 0, 0], fmt
        assert np.array_equal(bits(Xf[:M]), bits(X0)), fmt
        same_solve(rec, Xf[:M], bench.want(m, B, X0, minv), ("-9", fmt))
        m.release()
    hs = upload(G.lap2d(15, 17, -2), "f64")
    for fmt, m in hs.items():
        for minv in (bench.jacobi(m), bench.set_minv(np.ones(M))):
            want = bench.want(m, B, X0, minv)
            assert list(want.status) == [2, 0, 2, 2]
            assert list(want.iterations) == [1, 0, 1, 2]
            rec, Xf, _ = bench.solve(m, B, X0, tol=TOL, maxit=200)
            same_solve(rec, Xf[:M], want, ("-2", fmt, minv[0]))
        m.release()
    bench.free()


# ---------------------------------------------------------------- 7. refusals
def _rc(m, k, B, ldb, X, ldx, minv, tol=TOL, maxit=10, check_every=0,
        work=None, work_bytes=0, info=True, opts=None, stream=None):
    rec = (S.CgInfo * 8)()
    return m._fn("pcg")(m.h, opts, k, B, ldb, X, ldx, minv, tol, maxit,
                        check_every, work, work_bytes, rec if info else None,
                        stream), rec


def test_refusals_on_live_handles():
    mat = G.lap2d(37, 29, 0.5)
    M = mat[0]
    k = 4
    B, X0 = G.common_inputs(M)
    bench = PcgBench(M)
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
    bench.jacobi(d)
    rec, Xf, _ = bench.solve(d, B, X0, tol=TOL, maxit=200)  # buffers filled
    assert [r.status for r in rec] == [0, 0, 0, 0]
    Bp, Xp, Dp = bench.B.ptr, bench.X.ptr, bench.minv.ptr
    einval = -errno.EINVAL
    need = S.pcg_work_bytes(M, k)
    work = S.DevBuffer(need)
    for m in (d, cm):
        put(Xp, np.vstack([X0, np.zeros((PAST, k))]))
        assert _rc(m, k, Bp, 0, Xp, 0, Dp)[0] == 0  # opts may be NULL
        for bad in (0, 9):
            assert _rc(m, bad, Bp, 0, Xp, 0, Dp)[0] == einval
        assert _rc(m, k, Bp, 3, Xp, 0, Dp)[0] == einval
        assert _rc(m, k, Bp, 0, Xp, 3, Dp)[0] == einval
        assert _rc(m, k, None, 0, Xp, 0, Dp)[0] == einval
        assert _rc(m, k, Bp, 0, None, 0, Dp)[0] == einval
        assert _rc(m, k, Bp, 0, Xp, 0, None)[0] == einval  # NULL minv
        assert _rc(m, k, Bp, 0, Xp, 0, Dp, info=False)[0] == einval
        for tol in (-1e-8, float("nan")):
            assert _rc(m, k, Bp, 0, Xp, 0, Dp, tol=tol)[0] == einval
        assert _rc(m, k, Bp, 0, Xp, 0, Dp, maxit=-1)[0] == einval
        assert _rc(m, k, Bp, 0, Xp, 0, Dp, check_every=-1)[0] == einval
        for bad in (dict(variant=1), dict(waves_per_block=17)):
            o = S._opts(**bad)
            assert _rc(m, k, Bp, 0, Xp, 0, Dp,
                       opts=C.byref(o))[0] == einval, bad
        # a work buffer that is too short (cg's size is), or not 8-byte aligned
        assert _rc(m, k, Bp, 0, Xp, 0, Dp, work=work.ptr,
                   work_bytes=need - 1)[0] == einval
        assert _rc(m, k, Bp, 0, Xp, 0, Dp, work=work.ptr,
                   work_bytes=S.cg_work_bytes(M, k))[0] == einval
        assert _rc(m, k, Bp, 0, Xp, 0, Dp, work=work.ptr + 4,
                   work_bytes=need)[0] == einval
        assert m._fn("diag")(m.h, None, 0, None) == einval
        assert S._lib.spmv_live_handles() == made
    assert _rc(compact, k, Bp, 0, Xp, 0, Dp)[0] == -errno.ENOTSUP
    assert compact._fn("diag")(compact.h, Dp, 1, None) == -errno.ENOTSUP
    assert _rc(rm, k, Bp, 0, Xp, 0, Dp)[0] == einval
    assert rm._fn("diag")(rm.h, Dp, 1, None) == einval
    for m in (d1, h1):  # M != N: no solve, but a diagonal
        assert _rc(m, k, Bp, 0, Xp, 0, Dp)[0] == einval
        assert m._fn("diag")(m.h, Dp, 1, None) == 0
    # no rows: 0, every record zero
    for m in (d0, h0):
        rc, rec = _rc(m, k, Bp, 0, Xp, 0, Dp)
        assert rc == 0
        assert [(r.status, r.iterations, r.rr, r.bb) for r in rec[:k]] == \
            [(0, 0, 0.0, 0.0)] * k
        assert m._fn("diag")(m.h, Dp, 0, None) == 0
    S.stream_sync()
    bench.jacobi(d)

    # a capturing stream: -EBUSY, nothing enqueued, the capture ends cleanly
    side = S.Stream()
    for m in (d, cm):
        put(Xp, np.vstack([X0, np.zeros((PAST, k))]))
        S._check(S._lib.spmv_graph_begin_capture(side.ptr), "begin_capture")
        rc, _ = _rc(m, k, Bp, 0, Xp, 0, Dp, stream=side.ptr)
        rc_own, _ = _rc(m, k, Bp, 0, Xp, 0, Dp, work=work.ptr,
                        work_bytes=need, stream=side.ptr)
        g = C.c_void_p()
        end = S._lib.spmv_graph_end_capture(side.ptr, C.byref(g))
        if end == 0:
            S._check(S._lib.spmv_graph_destroy(g), "spmv_graph_destroy")
        assert rc == -errno.EBUSY and rc_own == -errno.EBUSY
        assert end == 0, "the capture was invalidated"
        got = bench.X.to_numpy(np.float64, M * k).reshape(M, k)
        assert np.array_equal(bits(got), bits(X0)), "something was enqueued"
        # ... and the stream solves afterwards
        rc, rec = _rc(m, k, Bp, 0, Xp, 0, Dp, maxit=200, stream=side.ptr)
        assert rc == 0 and [r.status for r in rec[:k]] == [0, 0, 0, 0]
    side.sync()

    # only the blocked copy left: no source arrays to read
    for m in (d, cm):
        m.build_panels()
        m.release_source()
        assert _rc(m, k, Bp, 0, Xp, 0, Dp)[0] == -errno.ENODATA
        assert m._fn("diag")(m.h, Dp, 1, None) == -errno.ENODATA
        with pytest.raises(OSError) as ei:
            m.pcg(Bp, Xp, Dp, k)
        assert ei.value.errno == errno.ENODATA
        with pytest.raises(OSError) as ei:
            m.diag(Dp)
        assert ei.value.errno == errno.ENODATA
    S.stream_sync()
    for m in (d, cm, rm, compact, d1, h1, d0, h0):
        m.release()
    assert S._lib.spmv_csr_pcg(C.c_void_p(1 << 20), None, k, Bp, 0, Xp, 0, Dp,
                               TOL, 10, 0, None, 0, (S.CgInfo * 8)(),
                               None) == -errno.EBADF
    assert S._lib.spmv_csr_diag(C.c_void_p(1 << 20), Dp, 0,
                                None) == -errno.EBADF
    assert S._lib.spmv_live_handles() == live
    work.free()
    bench.free()
    S.csr_free(A0)
    S.csr_free(A1)
