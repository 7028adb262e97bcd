"""Restarted GMRES on the device (spmv_*_gmres, spmv_*_gmres_trsv;
spmv_engine.h) on the GPU: CSR and column-major HLL handles, f64 and f32
values, 1-8 interleaved systems, restart 1 / 3 / 30 / 64, without a
preconditioner, with a diagonal and with triangular plans.

The expected values come from the numpy restatement (tests/_gmres.py) with the
product of every step taken from the SAME handle's launch_multi and the
residual of every cycle's start from its launch_axpby.  numpy rounds every
operation once, which is the contract, so the uint64 views of X are compared,
and status, iterations, restarts and the bits of rr / est / bb.  The one
tolerance is the sanity line of test_gpu_cg: the true residual of the device's
X, computed on the host, is at most 2 tol.

A launch of the multi-vector dot takes min(16, 32 // k) basis vectors, so the
restart = 30 cycles at k = 8 cross seven chunk boundaries (one at k = 1), the
53 steps of restart = 64 three at k = 1.
Inputs: tests/_cg.py common_inputs (column 1 all zero, column 2 scaled by 1e-3,
X0 zero except column 3), so the columns stop at different steps, some in
mid-cycle.  Every test runs under a time limit of its own (LIMIT_S).
"""
import ctypes as C
import errno
import faulthandler

import numpy as np
import pytest

import _bicgstab as BI
import _cg as G
import _gmres as GM
import _ilu0 as IL
import _oracle as O
import _pcg as PG
import _pcg_trsv as PT
import spmv_scpa_amd as S
from test_gpu_bicgstab_trsv import (GROUP, Precond, device_diagonal,
                                    device_ilu0, device_sgs)
from test_gpu_cg import (BIG_NX, BIG_NY, NWG, T, TOL, fill, neighbours_kept,
                         put, upload)
from test_gpu_f32_values import round32
from test_gpu_multi_vector import FILL, PAST, bits
from test_gpu_pcg import PcgBench

pytestmark = pytest.mark.gpu

LIMIT_S = 240
MATRICES = {
    "convdiff(1,1)": lambda: BI.convdiff(1, 1, 0.5, 0.5),
    "convdiff(15,17)": lambda: BI.convdiff(15, 17, 0.5, 0.5),  # < a workgroup
    "convdiff(37,29)": lambda: BI.convdiff(37, 29, 0.5, 0.5),  # M = 1073, odd
    "arrow2(2051,3)": lambda: BI.arrow2(2051, 3),   # the long-row kernel
}


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def chunk(k):
    """basis vectors one launch of the multi-vector dot takes"""
    return min(16, 32 // k)


class GmBench(PcgBench):
    """PcgBench (B, X, P / Q of the restatement, a minv buffer) solving
    through gmres() / gmres_trsv()"""

    def want(self, m, B, X0, restart, z=None, tol=TOL, maxit=200, trace=None,
             **opts):
        M, k = B.shape
        product, _ = self.callables(m, B, X0, **opts)

        def residual(X):
            put(self.P.ptr, X)
            put(self.Q.ptr, B)
            m.launch_axpby(-1.0, 1.0, self.P.ptr, self.Q.ptr, k, **opts)
            S.stream_sync()
            return self.Q.to_numpy(np.float64, M * k).reshape(M, k)
        return GM.restate(product, residual, B, X0, restart, tol, maxit, z=z,
                          trace=trace)

    def solve(self, m, B, X0, restart, ldb=0, ldx=0, shift=0, pre=None, **kw):
        """-> (records, whole X buffer as (M + PAST, ldx)): padding columns of
        B are NaN, those of X and the rows beyond M of both hold the 0xFF
        fill.  pre: None, "minv" (the minv buffer as it stands) or a Precond.
        Asserts that B, minv and the scale of the plans were not written"""
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
        plans = isinstance(pre, Precond)
        scale = (pre.scale.to_numpy(np.uint64, M)
                 if plans and pre.scale is not None else None)
        if plans:
            rec = m.gmres_trsv(self.B.ptr, self.X.ptr + shift, k=k,
                               restart=restart, ldb=ldb, ldx=ldx, **pre.kw,
                               **kw)
        else:
            rec = m.gmres(self.B.ptr, self.X.ptr + shift, k, restart,
                          d_minv=self.minv.ptr if pre == "minv" else None,
                          ldb=ldb, ldx=ldx, **kw)
        S.stream_sync()
        Xf = self.X.to_numpy(np.float64, (M + PAST) * lx + shift // 8)
        Bf = self.B.to_numpy(np.float64, (M + PAST) * lb)
        assert np.array_equal(bits(Bf), bits(Bh.ravel())), "B was written"
        assert np.array_equal(self.minv.to_numpy(np.uint64, M + PAST),
                              before), "minv was written"
        if scale is not None:
            assert np.array_equal(pre.scale.to_numpy(np.uint64, M), scale)
        return rec, Xf[shift // 8:].reshape(M + PAST, lx)


def same(rec, X, want, tag):
    """a device solve against a restatement (or two device solves): bits"""
    k = len(rec)
    print(tag, "status", [r.status for r in rec], "iterations",
          [r.iterations for r in rec], "restarts", [r.restarts for r in rec])
    for name in ("status", "iterations", "restarts"):
        assert [getattr(r, name) for r in rec] == list(getattr(want, name)), \
            (tag, name, list(getattr(want, name)))
    for name in ("rr", "est", "bb"):
        got = np.array([getattr(r, name) for r in rec])
        assert np.array_equal(bits(got), bits(getattr(want, name))), \
            (tag, name, got, getattr(want, name))
    eq = bits(X[:, :k]) == bits(want.X)
    assert np.all(eq), (tag, "elements of X that differ", int(np.sum(~eq)),
                        np.argwhere(~eq)[:4].tolist())


def as_want(rec, X):
    k = len(rec)
    return GM.Solve(X[:, :k].copy(), *([getattr(r, f) for r in rec]
                                       for f in ("status", "iterations",
                                                 "restarts")),
                    *(np.array([getattr(r, f) for r in rec])
                      for f in ("rr", "est", "bb")))


def column(base, j):
    return GM.Solve(base.X[:, j:j + 1], *(getattr(base, f)[j:j + 1]
                                          for f in GM.Solve._fields[1:]))


def release(hs, bench, *more):
    for h in more:
        h.release() if hasattr(h, "release") else h.free()
    for m in hs.values():
        m.release()
    bench.free()


# -------------------------------------------------------------------- 1. bits
@pytest.mark.parametrize("values", ["f64", "f32"])
@pytest.mark.parametrize("name", list(MATRICES))
def test_a_solve_has_the_bits_of_the_restatement(name, values):
    mat = MATRICES[name]()
    M, IRP, JA, AS = mat
    if name.startswith("arrow2"):
        assert IRP[1] == M > 2048
    stored = round32(AS) if values == "f32" else AS
    B, X0 = G.common_inputs(M)
    bench = GmBench(M)
    fill(bench.minv)
    hs = upload(mat, values)
    for fmt, m in hs.items():
        tag = (name, values, fmt)
        want = bench.want(m, B, X0, 30)
        rec, Xf = bench.solve(m, B, X0, 30, tol=TOL, maxit=200)
        same(rec, Xf[:M], want, tag)
        neighbours_kept(Xf, M, 4, tag)
        assert [r.status for r in rec] == [0, 0, 0, 0], tag
        # the zero column: converged at once, X untouched
        assert rec[1].iterations == 0 and rec[1].bb == 0.0, tag
        assert np.array_equal(bits(Xf[:M, 1]), bits(X0[:, 1])), tag
        res = G.true_residual(IRP, JA, stored, O.csr_spmv, B, Xf[:M, :4])
        print(tag, "true residual", res)
        assert np.all(res <= 2 * TOL), (tag, res)
        # maxit = restart + 2: the solve ends in mid-cycle and its two steps
        # are applied
        want5 = bench.want(m, B, X0, 3, maxit=5)
        rec, Xf = bench.solve(m, B, X0, 3, tol=TOL, maxit=5)
        same(rec, Xf[:M], want5, tag + ("restart 3, maxit 5",))
        if M > 17:
            assert [(r.status, r.iterations, r.restarts) for r in rec] == \
                [(1, 5, 1), (0, 0, 0), (1, 5, 1), (1, 5, 1)], tag
        assert np.array_equal(bits(Xf[:M, 1]), bits(X0[:, 1])), tag
    release(hs, bench)


@pytest.mark.parametrize("restart", [1, 3, 30, 64])
@pytest.mark.parametrize("k", [1, 8])
def test_every_restart_length_and_chunking(restart, k):
    """k = 8: four basis vectors a launch of the multi-dot, k = 1: sixteen;
    restart = 30 runs a full cycle across 7 (k = 8) or 1 (k = 1) chunk
    boundaries and restarts, restart = 64 does not restart.  The restatement
    on the CPU oracle's product takes 52-55 steps at restart = 30 here"""
    mat = MATRICES["convdiff(37,29)"]()
    M = mat[0]
    B, X0 = G.common_inputs(M, 8)
    if k == 1:
        B, X0 = B[:, :1].copy(), X0[:, :1].copy()
    bench = GmBench(M)
    fill(bench.minv)
    hs = upload(mat, "f64")
    maxit = 60 if restart == 1 else 200
    for fmt, m in hs.items():
        tag = (restart, k, fmt)
        trace = []
        want = bench.want(m, B, X0, restart, maxit=maxit, trace=trace)
        rec, Xf = bench.solve(m, B, X0, restart, tol=TOL, maxit=maxit)
        same(rec, Xf[:M], want, tag)
        neighbours_kept(Xf, M, k, tag)
        if restart == 30:
            if k == 8:  # a full cycle across two chunk boundaries and more
                assert restart + 1 > 2 * chunk(k)
            assert all(r.restarts >= 1 for j, r in enumerate(rec) if j != 1)
            assert [r.status for r in rec] == [0] * k, tag
        if restart == 64:
            assert [r.restarts for r in rec] == [0] * k, tag
        if restart == 1:
            assert rec[0].restarts == rec[0].iterations == 60, tag
        # est never grows within a cycle
        for (_, p, e0), (_, p1, e1) in zip(trace, trace[1:]):
            if p1 == p + 1:
                assert np.all(e1 <= e0), tag
        if k == 8 and restart > 1:  # columns stop at different steps
            assert len({r.iterations for r in rec}) > 2, tag
    release(hs, bench)


def test_one_full_sweep_of_the_slots_and_a_bit_more():
    mat = BI.convdiff(BIG_NX, BIG_NY, 1.0, 0.5)
    M = mat[0]
    assert NWG * T < M <= NWG * T + BIG_NX
    B, X0 = G.common_inputs(M, 8)
    bench = GmBench(M)
    fill(bench.minv)
    hs = upload(mat, "f64")
    for fmt, m in hs.items():
        # restart + 2 steps: one full cycle, a restart, two steps applied at
        # the end
        want = bench.want(m, B, X0, 4, maxit=6)
        rec, Xf = bench.solve(m, B, X0, 4, tol=TOL, maxit=6)
        same(rec, Xf[:M], want, ("big", fmt))
        neighbours_kept(Xf, M, 8, ("big", fmt))
        assert [(r.status, r.iterations, r.restarts) for r in rec] == \
            [(1, 6, 1), (0, 0, 0)] + [(1, 6, 1)] * 6, fmt
    release(hs, bench)


# ------------------------------------------------------------------ 2. Jacobi
@pytest.mark.parametrize("values", ["f64", "f32"])
def test_a_jacobi_solve_has_the_bits_of_the_restatement(values):
    mat = BI.rowscale(BI.convdiff(37, 29, 0.5, 0.5), 5)
    M, IRP, JA, AS = mat
    stored = round32(AS) if values == "f32" else AS
    B, X0 = G.common_inputs(M, 5)
    bench = GmBench(M)
    hs = upload(mat, values)
    inv = 1.0 / PG.diag_of(M, IRP, JA, stored)
    for fmt, m in hs.items():
        tag = (values, fmt)
        minv = bench.jacobi(m)
        assert np.array_equal(bits(minv), bits(inv)), tag
        want = bench.want(m, B, X0, 7, z=lambda U: minv[:, None] * U)
        rec, Xf = bench.solve(m, B, X0, 7, pre="minv", tol=TOL, maxit=200,
                              ldb=8, ldx=6, shift=8)
        same(rec, Xf[:M], want, tag)
        neighbours_kept(Xf, M, 5, tag)
        assert [r.status for r in rec] == [0] * 5, tag
        assert min(r.restarts for j, r in enumerate(rec) if j != 1) >= 1
        res = G.true_residual(IRP, JA, stored, O.csr_spmv, B, Xf[:M, :5])
        print(tag, "true residual", res)
        assert np.all(res <= 2 * TOL), (tag, res)
    release(hs, bench)


# --------------------------------------------------------------- 3. the plans
@pytest.mark.parametrize("which", ["ilu0", "sgs"])
def test_a_solve_with_plans_has_the_bits_of_the_restatement(which):
    mat = IL.MATRICES["convdiff(37,29)"]()
    M, IRP, JA, AS = mat
    pc = {"sgs": PT.sgs, "ilu0": IL.ilu0}[which](mat)
    z = PT.plans_apply(*pc, GROUP)
    bench = GmBench(M)
    fill(bench.minv)
    hs = upload(mat, "f64")
    pre = {"sgs": device_sgs, "ilu0": device_ilu0}[which](hs["csr"])
    for fmt, m in hs.items():
        for k, restart in ((3, 5), (8, 30)):
            tag = (which, fmt, k, restart)
            B, X0 = G.common_inputs(M, k)
            want = bench.want(m, B, X0, restart, z=z)
            stride = dict(ldb=k + 2, ldx=k + 1, shift=8) if k == 3 else {}
            rec, Xf = bench.solve(m, B, X0, restart, pre=pre, tol=TOL,
                                  maxit=200, **stride)
            same(rec, Xf[:M], want, tag)
            neighbours_kept(Xf, M, k, tag)
            assert [r.status for r in rec] == [0] * k, tag
            res = G.true_residual(IRP, JA, AS, O.csr_spmv, B, Xf[:M, :k])
            assert np.all(res <= 2 * TOL), (tag, res)
    if which == "sgs":  # the documented call
        B, X0 = G.common_inputs(M, 2)
        d_B, d_X = S.DevBuffer.from_numpy(B), S.DevBuffer.from_numpy(X0)
        sg = hs["csr"].sgs()
        rec = hs["csr"].gmres_trsv(d_B.ptr, d_X.ptr, *sg.args, k=2)
        assert [r.status for r in rec] == [0, 0]
        for h in (sg, d_B, d_X):
            h.release() if hasattr(h, "release") else h.free()
    pre.release()
    release(hs, bench)


def test_ones_and_an_identity_plan_are_none_and_a_power_of_two_plan_its_minv():
    mat = MATRICES["convdiff(37,29)"]()
    M = mat[0]
    B, X0 = G.common_inputs(M)
    bench = GmBench(M)
    hs = upload(mat, "f64")
    d = 2.0 ** np.random.default_rng(3).integers(-6, 7, M)
    ident = device_diagonal(np.ones(M))
    unit = device_diagonal(np.full(M, 7.0), unit=True)
    pow2 = device_diagonal(d)
    for fmt, m in hs.items():
        for maxit in (200, 12):   # converged; cut short in the second cycle
            fill(bench.minv)
            rec, Xf = bench.solve(m, B, X0, 10, tol=TOL, maxit=maxit)
            none = as_want(rec, Xf[:M])
            bench.set_minv(np.ones(M))
            rec, Xf = bench.solve(m, B, X0, 10, pre="minv", tol=TOL,
                                  maxit=maxit)
            same(rec, Xf[:M], none, (fmt, "ones", maxit))
            for nm, pre in (("identity", ident), ("unit", unit)):
                rec, Xf = bench.solve(m, B, X0, 10, pre=pre, tol=TOL,
                                      maxit=maxit)
                same(rec, Xf[:M], none, (fmt, nm, maxit))
            bench.set_minv(1.0 / d)
            rec, Xf = bench.solve(m, B, X0, 10, pre="minv", tol=TOL,
                                  maxit=maxit)
            diag = as_want(rec, Xf[:M])
            rec, Xf = bench.solve(m, B, X0, 10, pre=pow2, tol=TOL,
                                  maxit=maxit)
            same(rec, Xf[:M], diag, (fmt, "2^n", maxit))
            if maxit == 200:
                assert list(none.status) == [0, 0, 0, 0]
            else:
                assert list(none.iterations) == [12, 0, 12, 12]
    for pre in (ident, unit, pow2):
        pre.release()
    release(hs, bench)


def test_ilu0_plans_of_a_coloured_and_permuted_handle_converge():
    mat = MATRICES["convdiff(37,29)"]()
    M = mat[0]
    B, X0 = G.common_inputs(M, 2)
    hs = upload(mat, "f64")
    col = hs["csr"].colour()
    dP = hs["csr"].permute(col, col)
    host = dP.download()
    IRP, JA, AS = S.csr_arrays(host)
    LU, info = dP.ilu0()
    lo, up = LU.trsv_analyse("lower", unit=True), LU.trsv_analyse("upper")
    d_B, d_X = S.DevBuffer.from_numpy(B), S.DevBuffer.from_numpy(X0)
    rec = dP.gmres_trsv(d_B.ptr, d_X.ptr, lo, up, k=2, restart=20, tol=TOL,
                        maxit=200)
    X = d_X.to_numpy(np.float64, M * 2).reshape(M, 2)
    res = G.true_residual(IRP, JA, AS, O.csr_spmv, B, X)
    print("coloured ilu0", rec, res)
    assert [r.status for r in rec] == [0, 0] and np.all(res <= 2 * TOL)
    assert 0 < rec[0].iterations < 54   # fewer steps than without
    S.csr_free(host)
    for h in (lo, up, LU, dP, col, *hs.values()):
        h.release()
    d_B.free()
    d_X.free()


# ------------------------------------------------------------ 4. independence
def test_the_result_depends_on_the_system_alone():
    mat = MATRICES["convdiff(37,29)"]()
    M = mat[0]
    B, X0 = G.common_inputs(M)
    bench = GmBench(M)
    fill(bench.minv)
    hs = upload(mat, "f64")
    restart, maxit = 7, 200
    work = S.DevBuffer(S.gmres_work_bytes(M, 8, restart))
    for fmt, m in hs.items():
        rec, Xf = bench.solve(m, B, X0, restart, tol=TOL, maxit=maxit)
        base = as_want(rec, Xf[:M])
        assert base.status == [0, 0, 0, 0]
        # some column stops in mid-cycle
        assert any(i % restart for i in base.iterations), base.iterations
        for kw in (dict(check_every=1), dict(check_every=7),
                   dict(check_every=0), dict(check_every=maxit + 1),
                   dict(work=work), dict(waves_per_block=1),
                   dict(waves_per_block=16)):
            rec, Xf = bench.solve(m, B, X0, restart, ldx=6, tol=TOL,
                                  maxit=maxit, **kw)
            same(rec, Xf[:M], base, (fmt, kw))
            neighbours_kept(Xf, M, 4, (fmt, kw))
        # column j of the k = 4 solve is the k = 1 solve of that column
        for j in range(4):
            rec, Xf = bench.solve(m, B[:, j:j + 1], X0[:, j:j + 1], restart,
                                  tol=TOL, maxit=maxit)
            same(rec, Xf[:M], column(base, j), (fmt, "column", j))
            neighbours_kept(Xf, M, 1, (fmt, "column", j))
        # the other widths: the first k of the four columns twice
        B8, X8 = np.hstack([B, B]), np.hstack([X0, X0])
        for k in (2, 3, 5, 6, 7, 8):
            rec, Xf = bench.solve(m, B8[:, :k], X8[:, :k], restart, tol=TOL,
                                  maxit=maxit)
            neighbours_kept(Xf, M, k, (fmt, "k", k))
            for j in range(k):
                same(rec[j:j + 1], Xf[:M, j:j + 1], column(base, j % 4),
                     (fmt, "k", k, "column", j))
        # the same, stopped by maxit in mid-cycle
        rec, Xf = bench.solve(m, B, X0, restart, tol=TOL, maxit=restart + 2)
        cut = as_want(rec, Xf[:M])
        assert cut.iterations == [9, 0, 9, 9] and cut.restarts == [1, 0, 1, 1]
        for kw in (dict(check_every=1), dict(check_every=100)):
            rec, Xf = bench.solve(m, B, X0, restart, tol=TOL,
                                  maxit=restart + 2, **kw)
            same(rec, Xf[:M], cut, (fmt, "cut", kw))
    release(hs, bench, work)


class _Exactly:
    """`work` of exactly n bytes at the head of a larger allocation"""

    def __init__(self, buf, n):
        self.ptr, self.nbytes = buf.ptr, n


def test_the_work_buffer_is_used_and_not_overrun():
    mat = MATRICES["convdiff(15,17)"]()
    M = mat[0]
    B, X0 = G.common_inputs(M, 8)
    bench = GmBench(M)
    fill(bench.minv)
    hs = upload(mat, "f64")
    guard = 4096
    for restart in (1, 64):
        need = S.gmres_work_bytes(M, 8, restart)
        work = S.DevBuffer(need + guard)
        for fmt, m in hs.items():
            rec, Xf = bench.solve(m, B, X0, restart, tol=TOL, maxit=70)
            own = as_want(rec, Xf[:M])
            S._check(S._lib.spmv_dev_memset(work.ptr, 0xA5, work.nbytes,
                                            None), "spmv_dev_memset")
            rec, Xf = bench.solve(m, B, X0, restart, tol=TOL, maxit=70,
                                  work=_Exactly(work, need))
            same(rec, Xf[:M], own, (restart, fmt))
            tail = work.to_numpy(np.uint8, need + guard)[need:]
            assert np.all(tail == 0xA5), "bytes behind the work buffer"
        work.free()
    release(hs, bench)


# ---------------------------------------------------------------- 5. statuses
def test_a_breakdown_is_a_status_not_a_fault():
    good = MATRICES["convdiff(15,17)"]()
    M = good[0]
    B, X0 = G.common_inputs(M)
    bench = GmBench(M)
    fill(bench.minv)
    # every stored value 0.0: d == 0 in the first step
    zero = (M, good[1], good[2], np.zeros_like(good[3]))
    hs = upload(zero, "f64")
    for fmt, m in hs.items():
        want = bench.want(m, B, X0, 5)
        rec, Xf = bench.solve(m, B, X0, 5, tol=TOL, maxit=200)
        same(rec, Xf[:M], want, ("zero", fmt))
        assert [(r.status, r.iterations) for r in rec] == \
            [(2, 0), (0, 0), (2, 0), (2, 0)], fmt
        assert np.array_equal(bits(Xf[:M, :4]), bits(X0)), fmt
    for m in hs.values():
        m.release()
    hs = upload(good, "f64")
    # a zero pivot in row 0 leaves inf / NaN in the factor of the plans
    bad = upload(IL.with_zero_pivot(good, 0), "f64")
    pre = device_ilu0(bad["csr"])
    for m in bad.values():
        m.release()
    for fmt, m in hs.items():
        rec, Xf = bench.solve(m, B, X0, 5, tol=TOL, maxit=200)
        clean = as_want(rec, Xf[:M])
        assert clean.status == [0, 0, 0, 0]
        # a NaN in minv, and in the factor of a plan
        d = np.ones(M)
        d[9] = np.nan
        minv = bench.set_minv(d)
        want = bench.want(m, B, X0, 5, z=lambda U: minv[:, None] * U)
        for p in ("minv", pre):
            rec, Xf = bench.solve(m, B, X0, 5, pre=p, tol=TOL, maxit=200)
            assert [(r.status, r.iterations) for r in rec] == \
                [(2, 0), (0, 0), (2, 0), (2, 0)], fmt
            assert np.array_equal(bits(Xf[:M, :4]), bits(X0)), fmt
            if p == "minv":
                same(rec, Xf[:M], want, ("nan", fmt))
        # one inf in column 0 of B: that column stops, the others never notice
        Bi = B.copy()
        Bi[7, 0] = np.inf
        rec, Xf = bench.solve(m, Bi, X0, 5, tol=TOL, maxit=200)
        assert rec[0].status == 2 and rec[0].iterations == 0, fmt
        assert np.array_equal(bits(Xf[:M, 0]), bits(X0[:, 0])), fmt
        for j in (1, 2, 3):
            got = as_want(rec[j:j + 1], Xf[:M, j:j + 1])
            same(rec[j:j + 1], Xf[:M, j:j + 1], column(clean, j), ("inf", j))
            assert got.status == [0]
        # ... and the handle still solves
        rec, Xf = bench.solve(m, B, X0, 5, tol=TOL, maxit=200)
        same(rec, Xf[:M], clean, ("after", fmt))
    pre.release()
    release(hs, bench)


# ---------------------------------------------------------------- 6. refusals
def _rc(m, k, B, X, minv, restart=5, tol=TOL, maxit=10, check_every=0,
        work=None, work_bytes=0, info=True, opts=None, stream=None, ldb=0,
        ldx=0):
    rec = (S.GmresInfo * 8)()
    return m._fn("gmres")(m.h, opts, k, B, ldb, X, ldx, minv, restart, tol,
                          maxit, check_every, work, work_bytes,
                          rec if info else None, stream), rec


def _rc_trsv(m, k, B, X, first, second, scale, restart=5):
    rec = (S.GmresInfo * 8)()
    return m._fn("gmres_trsv")(m.h, None, k, B, 0, X, 0, first, second, scale,
                               restart, TOL, 3, 0, None, 0, rec, None)


def test_refusals_on_live_handles():
    mat = MATRICES["convdiff(37,29)"]()
    M = mat[0]
    k = 4
    B, X0 = G.common_inputs(M)
    bench = GmBench(M)
    hs = upload(mat, "f64")
    d, cm = hs["csr"], hs["hll"]
    compact = cm.to_index16()
    A1 = S.csr_from_arrays("wide", M, M + 1, mat[1], mat[2], mat[3])
    d1 = S.CsrDevice.upload(A1)
    A0 = S.csr_from_arrays("norows", 0, 0, np.zeros(1, np.int32),
                           np.zeros(0, np.int32), np.zeros(0))
    d0 = S.CsrDevice.upload(A0)
    made = S._lib.spmv_live_handles()
    bench.jacobi(d)
    rec, Xf = bench.solve(d, B, X0, 5, pre="minv", tol=TOL, maxit=200)
    assert [r.status for r in rec] == [0, 0, 0, 0]   # the buffers are filled
    Bp, Xp, Dp = bench.B.ptr, bench.X.ptr, bench.minv.ptr
    einval = -errno.EINVAL
    need = S.gmres_work_bytes(M, k, 5)
    assert need < S.gmres_work_bytes(M, k, 6)
    work = S.DevBuffer(need)
    for m in (d, cm):
        for minv in (Dp, None):
            put(Xp, np.vstack([X0, np.zeros((PAST, k))]))
            assert _rc(m, k, Bp, Xp, minv)[0] == 0
            for bad in (0, 9):
                assert _rc(m, bad, Bp, Xp, minv)[0] == einval
            for bad in (0, -1, 65):
                assert _rc(m, k, Bp, Xp, minv, restart=bad)[0] == einval
            assert _rc(m, k, Bp, Xp, minv, restart=64, maxit=2)[0] == 0
            assert _rc(m, k, Bp, Xp, minv, ldb=3)[0] == einval
            assert _rc(m, k, Bp, Xp, minv, ldx=3)[0] == einval
            assert _rc(m, k, None, Xp, minv)[0] == einval
            assert _rc(m, k, Bp, None, minv)[0] == einval
            assert _rc(m, k, Bp, Xp, minv, info=False)[0] == einval
            for tol in (-1e-8, float("nan")):
                assert _rc(m, k, Bp, Xp, minv, tol=tol)[0] == einval
            assert _rc(m, k, Bp, Xp, minv, maxit=-1)[0] == einval
            assert _rc(m, k, Bp, Xp, minv, check_every=-1)[0] == einval
            o = S._opts(waves_per_block=17)
            assert _rc(m, k, Bp, Xp, minv, opts=C.byref(o))[0] == einval
            # a work buffer one byte short (the size of restart 5 does not
            # hold restart 6), or not 8-byte aligned
            assert _rc(m, k, Bp, Xp, minv, work=work.ptr,
                       work_bytes=need - 1)[0] == einval
            assert _rc(m, k, Bp, Xp, minv, restart=6, work=work.ptr,
                       work_bytes=need)[0] == einval
            assert _rc(m, k, Bp, Xp, minv, work=work.ptr + 4,
                       work_bytes=need)[0] == einval
            assert _rc(m, k, Bp, Xp, minv, work=work.ptr,
                       work_bytes=need)[0] == 0
        with pytest.raises(ValueError):
            m.gmres(Bp, Xp, k, restart=65)
    assert _rc(compact, k, Bp, Xp, Dp)[0] == -errno.ENOTSUP
    assert _rc(d1, k, Bp, Xp, Dp)[0] == einval        # M != N
    rc, rec = _rc(d0, k, Bp, Xp, Dp)                  # no rows
    assert rc == 0 and [(r.status, r.iterations, r.restarts, r.rr, r.est,
                         r.bb) for r in rec[:k]] == [(0, 0, 0, 0.0, 0.0,
                                                      0.0)] * k

    # the plans: bicgstab_trsv's checks behind restart's
    lower = d.trsv_analyse("lower")
    dead = d.trsv_analyse("upper")
    dead_h = dead.h
    dead.release()
    small = device_diagonal(np.ones(M - 1))
    for m in (d, cm):
        assert _rc_trsv(m, k, Bp, Xp, lower.h, None, None) == 0
        assert _rc_trsv(m, k, Bp, Xp, lower.h, None, None, restart=0) == einval
        assert _rc_trsv(m, k, Bp, Xp, None, None, None) == einval
        assert _rc_trsv(m, k, Bp, Xp, lower.h, None, Dp) == einval
        assert _rc_trsv(m, k, Bp, Xp, dead_h, None, None) == -errno.EBADF
        assert _rc_trsv(m, k, Bp, Xp, lower.h, dead_h, None) == -errno.EBADF
        assert _rc_trsv(m, k, Bp, Xp, small.first.h, None, None) == einval
        # restart is looked at first
        assert _rc_trsv(m, k, Bp, Xp, dead_h, None, None, restart=65) == einval
    assert _rc_trsv(compact, k, Bp, Xp, lower.h, None, None) == -errno.ENOTSUP
    small.release()
    lower.release()

    # a capturing stream: -EBUSY, nothing enqueued, the capture ends cleanly
    side = S.Stream()
    for m in (d, cm):
        put(Xp, np.vstack([X0, np.zeros((PAST, k))]))
        S._check(S._lib.spmv_graph_begin_capture(side.ptr), "begin_capture")
        rc, _ = _rc(m, k, Bp, Xp, Dp, stream=side.ptr)
        rc_own, _ = _rc(m, k, Bp, Xp, None, work=work.ptr, work_bytes=need,
                        stream=side.ptr)
        g = C.c_void_p()
        end = S._lib.spmv_graph_end_capture(side.ptr, C.byref(g))
        if end == 0:
            S._check(S._lib.spmv_graph_destroy(g), "spmv_graph_destroy")
        assert rc == -errno.EBUSY and rc_own == -errno.EBUSY
        assert end == 0, "the capture was invalidated"
        got = bench.X.to_numpy(np.float64, M * k).reshape(M, k)
        assert np.array_equal(bits(got), bits(X0)), "something was enqueued"
        rc, rec = _rc(m, k, Bp, Xp, Dp, maxit=200, stream=side.ptr)
        assert rc == 0 and [r.status for r in rec[:k]] == [0, 0, 0, 0]
    side.sync()
    S.stream_sync()
    assert S._lib.spmv_live_handles() == made
    for m in (d, cm, compact, d1, d0):
        m.release()
    work.free()
    bench.free()
    S.csr_free(A0)
    S.csr_free(A1)
