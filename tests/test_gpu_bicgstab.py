"""BiCGStab on the device (spmv_*_bicgstab, spmv_engine.h) on the GPU: CSR and
column-major HLL handles, f64 and f32 values, 1-8 interleaved systems, with
and without a diagonal preconditioner.

The expected values come from the numpy restatement of the solver
(tests/_bicgstab.py), with both products of an iteration taken from the SAME
handle's launch_multi and the initial residual from its launch_axpby, both
with the same opts.  numpy rounds every operation once, which is the contract,
so the uint64 views of X are compared, and iterations, status and the bits of
rr / bb.  The one tolerance is the sanity line of test_gpu_cg: the true
residual of the device's X, computed on the host, is at most 2 tol (the
restatement reaches 0.98 tol on these inputs with the CPU oracle's product;
the factor 2 only keeps a wrong contract that still "matches itself" from
passing).

Inputs: tests/_cg.py common_inputs (column 1 all zero, column 2 scaled by
1e-3, X0 zero except column 3).  Every test runs under a time limit of its own
(LIMIT_S): a test that exceeds it ends the whole process, so nothing else is
started on the device.
"""
import ctypes as C
import errno
import faulthandler

import numpy as np
import pytest

import _bicgstab as BI
import _cg as G
import _oracle as O
import _pcg as PG
import spmv_scpa_amd as S
from test_gpu_cg import (BIG_NX, BIG_NY, NWG, T, TOL, as_solve, fill,
                         neighbours_kept, put, same_solve, upload)
from test_gpu_f32_values import round32
from test_gpu_multi_vector import FILL, PAST, bits
from test_gpu_pcg import PcgBench

pytestmark = pytest.mark.gpu

LIMIT_S = 240
MATRICES = {
    "convdiff(1,1)": lambda: BI.convdiff(1, 1, 0.5, 0.5),
    "convdiff(15,17)": lambda: BI.convdiff(15, 17, 0.5, 0.5),  # < a workgroup
    "convdiff(37,29)": lambda: BI.convdiff(37, 29, 0.5, 0.5),  # M = 1073, odd
    "arrow2(2051,3)": lambda: BI.arrow2(2051, 3),
    "arrow2(4099,3)": lambda: BI.arrow2(4099, 3),
    # one grid just above one full sweep of the dot's slots
    "convdiff(big)": lambda: BI.convdiff(BIG_NX, BIG_NY, 1.0, 0.5),
}
SCALED = {
    "rowscale convdiff(15,17)":
        lambda: BI.rowscale(BI.convdiff(15, 17, 0.5, 0.5), 5),
    "rowscale convdiff(37,29)":
        lambda: BI.rowscale(BI.convdiff(37, 29, 0.5, 0.5), 5),
    "rowscale arrow2(2051,3)": lambda: BI.rowscale(BI.arrow2(2051, 3), 5),
}


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


class BiBench(PcgBench):
    """PcgBench (B, X, P / Q of the restatement, a minv buffer) solving
    through bicgstab()"""

    def want(self, m, B, X0, minv=None, tol=TOL, maxit=200, **opts):
        product, residual0 = self.callables(m, B, X0, **opts)
        return BI.restate(product, residual0, B, X0, minv, tol, maxit)

    def solve(self, m, B, X0, ldb=0, ldx=0, shift=0, pre=False, **kw):
        """-> (records, whole X buffer as (M + PAST, ldx), whole B buffer):
        padding columns of B are NaN, those of X and the rows beyond M of
        both hold the 0xFF fill.  pre: with the minv buffer as it stands.
        Asserts that neither B nor minv was written"""
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
        rec = m.bicgstab(self.B.ptr, self.X.ptr + shift, k,
                         d_minv=self.minv.ptr if pre else None, ldb=ldb,
                         ldx=ldx, **kw)
        S.stream_sync()
        Xf = self.X.to_numpy(np.float64, (M + PAST) * lx + shift // 8)
        Bf = self.B.to_numpy(np.float64, (M + PAST) * lb)
        assert np.array_equal(bits(Bf), bits(Bh.ravel())), "B was written"
        assert np.array_equal(self.minv.to_numpy(np.uint64, M + PAST),
                              before), "minv was written"
        return rec, Xf[shift // 8:].reshape(M + PAST, lx), Bh


# -------------------------------------------------------------------- 1. bits
@pytest.mark.parametrize("values", ["f64", "f32"])
@pytest.mark.parametrize("name", list(MATRICES))
def test_a_solve_has_the_bits_of_the_restatement(name, values):
    mat = MATRICES[name]()
    M, IRP, JA, AS = mat
    if name == "convdiff(big)":
        assert NWG * T < M <= NWG * T + BIG_NX
    if name.startswith("arrow2"):
        assert IRP[1] == M > 2048   # the CSR long-row kernel, a wide block
    stored = round32(AS) if values == "f32" else AS
    B, X0 = G.common_inputs(M)
    bench = BiBench(M)
    fill(bench.minv)
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
        # stopped by maxit: every non-zero column after exactly 3 steps
        want3 = bench.want(m, B, X0, maxit=3)
        rec, Xf, _ = bench.solve(m, B, X0, tol=TOL, maxit=3)
        same_solve(rec, Xf[:M], want3, tag + ("maxit 3",))
        if M > 1:  # a 1 x 1 system is solved by its first step
            assert [r.status for r in rec] == [1, 0, 1, 1], tag
            assert [r.iterations for r in rec] == [3, 0, 3, 3], tag
        assert np.array_equal(bits(Xf[:M, 1]), bits(X0[:, 1])), tag
    for m in hs.values():
        m.release()
    bench.free()


# ------------------------------------------------------------------ 2. Jacobi
@pytest.mark.parametrize("values", ["f64", "f32"])
@pytest.mark.parametrize("name", list(SCALED))
def test_a_jacobi_solve_has_the_bits_of_the_restatement(name, values):
    mat = SCALED[name]()
    M, IRP, JA, AS = mat
    stored = round32(AS) if values == "f32" else AS
    B, X0 = G.common_inputs(M)
    bench = BiBench(M)
    hs = upload(mat, values)
    inv = 1.0 / PG.diag_of(M, IRP, JA, stored)
    for fmt, m in hs.items():
        tag = (name, values, fmt)
        minv = bench.jacobi(m)
        assert np.array_equal(bits(minv), bits(inv)), tag
        want = bench.want(m, B, X0, minv)
        rec, Xf, _ = bench.solve(m, B, X0, pre=True, tol=TOL, maxit=200)
        same_solve(rec, Xf[:M], want, tag)
        neighbours_kept(Xf, M, 4, tag)
        assert [r.status for r in rec] == [0, 0, 0, 0], tag
        assert rec[1].iterations == 0 and rec[1].bb == 0.0, tag
        assert np.array_equal(bits(Xf[:M, 1]), bits(X0[:, 1])), tag
        res = G.true_residual(IRP, JA, stored, O.csr_spmv, B, Xf[:M, :4])
        print(tag, "true residual", res)
        assert np.all(res <= 2 * TOL), (tag, res)
        pre_iters = [r.iterations for r in rec]
        # stopped by maxit
        want2 = bench.want(m, B, X0, minv, maxit=2)
        rec, Xf, _ = bench.solve(m, B, X0, pre=True, tol=TOL, maxit=2)
        same_solve(rec, Xf[:M], want2, tag + ("maxit 2",))
        if "convdiff" in name:
            # (Jacobi makes the arrow nearly a rank-two change of the
            # identity: it may be solved by then)
            assert [r.status for r in rec] == [1, 0, 1, 1], tag
            assert [r.iterations for r in rec] == [2, 0, 2, 2], tag
        if name == "rowscale convdiff(37,29)":
            # what the preconditioner is for
            rec, Xf, _ = bench.solve(m, B, X0, tol=TOL, maxit=400)
            plain_iters = [r.iterations for r in rec]
            print(tag, "iterations: jacobi", pre_iters, "none", plain_iters)
            assert [r.status for r in rec] == [0, 0, 0, 0], tag
            for j in (0, 2, 3):
                assert 0 < pre_iters[j] < plain_iters[j], (tag, j)
    for m in hs.values():
        m.release()
    bench.free()


# --------------------------------------------------------- 3. minv = 1: none
@pytest.mark.parametrize("name", ["convdiff(15,17)", "convdiff(37,29)",
                                  "arrow2(4099,3)"])
def test_a_preconditioner_of_ones_has_the_bits_of_none(name):
    mat = MATRICES[name]()
    M = mat[0]
    B, X0 = G.common_inputs(M)
    bench = BiBench(M)
    bench.set_minv(np.ones(M))
    hs = upload(mat, "f64")
    for fmt, m in hs.items():
        for maxit in (200, 3):
            rec, Xf, _ = bench.solve(m, B, X0, tol=TOL, maxit=maxit)
            none = as_solve(rec, Xf[:M])
            rec, Xf, _ = bench.solve(m, B, X0, pre=True, tol=TOL, maxit=maxit)
            same_solve(rec, Xf[:M], none, (name, fmt, maxit))
            neighbours_kept(Xf, M, 4, (name, fmt, maxit))
    for m in hs.values():
        m.release()
    bench.free()


# ------------------------------------------------------------ 4. independence
def column(base, j):
    return G.Solve(base.X[:, j:j + 1], base.status[j:j + 1],
                   base.iterations[j:j + 1], base.rr[j:j + 1],
                   base.bb[j:j + 1])


@pytest.mark.parametrize("name", ["convdiff(37,29)", "arrow2(4099,3)"])
def test_the_result_depends_on_the_system_alone(name):
    mat = MATRICES[name]()
    M = mat[0]
    B, X0 = G.common_inputs(M)
    bench = BiBench(M)
    fill(bench.minv)
    hs = upload(mat, "f64")
    work = S.DevBuffer(S.bicgstab_work_bytes(M, 8))
    for fmt, m in hs.items():
        rec, Xf, _ = bench.solve(m, B, X0, tol=TOL, maxit=200)
        base = as_solve(rec, Xf[:M])
        assert base.status == [0, 0, 0, 0]
        for kw in (dict(check_every=1), dict(check_every=0),
                   dict(check_every=5), dict(work=work),
                   dict(waves_per_block=1), dict(waves_per_block=4),
                   dict(waves_per_block=16)):
            rec, Xf, _ = bench.solve(m, B, X0, tol=TOL, maxit=200, **kw)
            same_solve(rec, Xf[:M], base, (name, fmt, kw))
        # column j of the k = 4 solve is the k = 1 solve of that column
        for j in range(4):
            rec, Xf, _ = bench.solve(m, B[:, j:j + 1], X0[:, j:j + 1],
                                     tol=TOL, maxit=200)
            same_solve(rec, Xf[:M], column(base, j), (name, fmt, "column", j))
            neighbours_kept(Xf, M, 1, (name, fmt, "column", j))
        # k = 8, columns 4-7 copies of columns 0-3: the k = 4 bits twice
        B8, X8 = np.hstack([B, B]), np.hstack([X0, X0])
        rec, Xf, _ = bench.solve(m, B8, X8, tol=TOL, maxit=200)
        neighbours_kept(Xf, M, 8, (name, fmt, "k", 8))
        for j in range(8):
            same_solve(rec[j:j + 1], Xf[:M, j:j + 1], column(base, j % 4),
                       (name, fmt, "k", 8, "column", j))
        # the odd widths: the first k of those eight columns
        if name == "convdiff(37,29)":
            for k in (3, 5, 7):
                rec, Xf, _ = bench.solve(m, B8[:, :k], X8[:, :k], tol=TOL,
                                         maxit=200)
                neighbours_kept(Xf, M, k, (name, fmt, "k", k))
                for j in range(k):
                    same_solve(rec[j:j + 1], Xf[:M, j:j + 1],
                               column(base, j % 4),
                               (name, fmt, "k", k, "column", j))
    work.free()
    for m in hs.values():
        m.release()
    bench.free()


# ----------------------------------------------------------------- 5. strides
class _Exactly:
    """`work` of exactly n bytes at the head of a larger allocation"""

    def __init__(self, buf, n):
        self.ptr, self.nbytes = buf.ptr, n


@pytest.mark.parametrize("pre", [False, True])
def test_strides_an_unaligned_X_and_the_neighbours(pre):
    mat = SCALED["rowscale convdiff(37,29)"]()
    M = mat[0]
    k = 4
    B, X0 = G.common_inputs(M)
    bench = BiBench(M)
    hs = upload(mat, "f64")
    need = S.bicgstab_work_bytes(M, k)
    guard = 4096
    work = S.DevBuffer(need + guard)
    for fmt, m in hs.items():
        tag = (pre, fmt)
        minv = bench.jacobi(m)
        want = bench.want(m, B, X0, minv if pre else None, maxit=400)
        S._check(S._lib.spmv_dev_memset(work.ptr, 0xA5, work.nbytes, None),
                 "spmv_dev_memset")
        # ldx = k + 1: a column of X that is not the solver's; ldb = k + 3:
        # NaN padding in B; X 8 bytes off 16; rows beyond M of both; solve()
        # checks that B and minv (and the fill behind minv) keep their bits
        rec, Xf, _ = bench.solve(m, B, X0, ldb=k + 3, ldx=k + 1, shift=8,
                                 pre=pre, tol=TOL, maxit=400,
                                 work=_Exactly(work, need))
        same_solve(rec, Xf[:M], want, tag)
        assert [r.status for r in rec] == [0, 0, 0, 0], tag
        neighbours_kept(Xf, M, k, tag)
        tail = work.to_numpy(np.uint8, need + guard)[need:]
        assert np.all(tail == 0xA5), (tag, "bytes behind the work buffer")
    work.free()
    for m in hs.values():
        m.release()
    bench.free()


# ---------------------------------------------------------------- 6. statuses
def test_a_breakdown_is_a_status_not_a_fault():
    good = BI.convdiff(15, 17, 0.5, 0.5)
    Mg = good[0]
    Bg, Xg = G.common_inputs(Mg)
    gbench = BiBench(Mg)
    fill(gbench.minv)
    ghs = upload(good, "f64")
    clean = {}
    for fmt, m in ghs.items():
        rec, Xf, _ = gbench.solve(m, Bg, Xg, tol=TOL, maxit=200)
        clean[fmt] = as_solve(rec, Xf[:Mg])
        assert clean[fmt].status == [0, 0, 0, 0]

    def still_solves(tag):
        for fmt, m in ghs.items():
            rec, Xf, _ = gbench.solve(m, Bg, Xg, tol=TOL, maxit=200)
            same_solve(rec, Xf[:Mg], clean[fmt], (tag, "clean solve", fmt))

    # the three rules at M = 70, k = 2, X0 = 0
    M = 70
    bench = BiBench(M)
    fill(bench.minv)
    X0 = np.zeros((M, 2))
    Br = np.random.default_rng(2).uniform(-1, 1, (M, 2))
    Bodd = Br.copy()
    Bodd[1::2] = 0.0
    v = np.ones(M)
    v[1::2] = 1e200
    for tag, mat, B, status, iters in (
            # S = 0 exactly: tt = 0, omega = 0, R = 0, X = B
            ("identity", BI.diagm(np.ones(M)), Br, [0, 0], [1, 1]),
            # rv = 0 exactly
            ("skew2", BI.skew2(M), Bodd, [2, 2], [0, 0]),
            # tt overflows
            ("1e200", BI.diagm(v), np.ones((M, 2)), [2, 2], [0, 0])):
        hs = upload(mat, "f64")
        for fmt, m in hs.items():
            want = bench.want(m, B, X0)
            assert list(want.status) == status, (tag, fmt)
            assert list(want.iterations) == iters, (tag, fmt)
            for ce in (0, 1):
                rec, Xf, _ = bench.solve(m, B, X0, tol=TOL, maxit=200,
                                         check_every=ce)
                same_solve(rec, Xf[:M], want, (tag, fmt, ce))
                neighbours_kept(Xf, M, 2, (tag, fmt, ce))
                if tag == "identity":
                    assert [r.rr for r in rec] == [0.0, 0.0], fmt
                    assert np.array_equal(bits(Xf[:M]), bits(B)), fmt
                else:
                    assert np.array_equal(bits(Xf[:M]), bits(X0)), (tag, fmt)
            m.release()
        still_solves(tag)
    bench.free()

    # a NaN in minv: every product is NaN in that row, rv is NaN
    for fmt, m in ghs.items():
        d = np.ones(Mg)
        d[9] = np.nan
        minv = gbench.set_minv(d)
        rec, Xf, _ = gbench.solve(m, Bg, Xg, pre=True, tol=TOL, maxit=200)
        assert [r.status for r in rec] == [2, 0, 2, 2], fmt
        assert [r.iterations for r in rec] == [0, 0, 0, 0], fmt
        assert np.array_equal(bits(Xf[:Mg]), bits(Xg)), fmt
        same_solve(rec, Xf[:Mg], gbench.want(m, Bg, Xg, minv), ("nan", fmt))
    still_solves("nan in minv")

    # one inf in column 0 of B: that column stops, the others never notice
    Bi = Bg.copy()
    Bi[7, 0] = np.inf
    for fmt, m in ghs.items():
        for ce in (1, 0):
            rec, Xf, _ = gbench.solve(m, Bi, Xg, tol=TOL, maxit=200,
                                      check_every=ce)
            assert rec[0].status == 2 and rec[0].iterations == 0, (fmt, rec)
            assert np.array_equal(bits(Xf[:Mg, 0]), bits(Xg[:, 0])), fmt
            for j in (1, 2, 3):
                same_solve(rec[j:j + 1], Xf[:Mg, j:j + 1],
                           column(clean[fmt], j), ("inf", fmt, ce, j))
            same_solve(rec, Xf[:Mg], gbench.want(m, Bi, Xg), ("inf", fmt))
    still_solves("inf in B")
    for m in ghs.values():
        m.release()
    gbench.free()


# ---------------------------------------------------------------- 7. refusals
def _rc(m, k, B, ldb, X, ldx, minv, tol=TOL, maxit=10, check_every=0,
        work=None, work_bytes=0, info=True, opts=None, stream=None):
    rec = (S.CgInfo * 8)()
    return m._fn("bicgstab")(m.h, opts, k, B, ldb, X, ldx, minv, tol, maxit,
                             check_every, work, work_bytes,
                             rec if info else None, stream), rec


def test_refusals_on_live_handles():
    mat = BI.convdiff(37, 29, 0.5, 0.5)
    M = mat[0]
    k = 4
    B, X0 = G.common_inputs(M)
    bench = BiBench(M)
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
    rec, Xf, _ = bench.solve(d, B, X0, pre=True, tol=TOL, maxit=200)
    assert [r.status for r in rec] == [0, 0, 0, 0]   # the buffers are filled
    Bp, Xp, Dp = bench.B.ptr, bench.X.ptr, bench.minv.ptr
    einval = -errno.EINVAL
    need = S.bicgstab_work_bytes(M, k)
    work = S.DevBuffer(need)
    for m in (d, cm):
        for minv in (Dp, None):  # with and without: the same checks
            put(Xp, np.vstack([X0, np.zeros((PAST, k))]))
            assert _rc(m, k, Bp, 0, Xp, 0, minv)[0] == 0  # opts may be NULL
            for bad in (0, 9):
                assert _rc(m, bad, Bp, 0, Xp, 0, minv)[0] == einval
            assert _rc(m, k, Bp, 3, Xp, 0, minv)[0] == einval
            assert _rc(m, k, Bp, 0, Xp, 3, minv)[0] == einval
            assert _rc(m, k, None, 0, Xp, 0, minv)[0] == einval
            assert _rc(m, k, Bp, 0, None, 0, minv)[0] == einval
            assert _rc(m, k, Bp, 0, Xp, 0, minv, info=False)[0] == einval
            for tol in (-1e-8, float("nan")):
                assert _rc(m, k, Bp, 0, Xp, 0, minv, tol=tol)[0] == einval
            assert _rc(m, k, Bp, 0, Xp, 0, minv, maxit=-1)[0] == einval
            assert _rc(m, k, Bp, 0, Xp, 0, minv, check_every=-1)[0] == einval
            for bad in (dict(variant=1), dict(waves_per_block=17)):
                o = S._opts(**bad)
                assert _rc(m, k, Bp, 0, Xp, 0, minv,
                           opts=C.byref(o))[0] == einval, bad
            # a work buffer one byte short, or not 8-byte aligned
            assert _rc(m, k, Bp, 0, Xp, 0, minv, work=work.ptr,
                       work_bytes=need - 1)[0] == einval
            assert _rc(m, k, Bp, 0, Xp, 0, minv, work=work.ptr + 4,
                       work_bytes=need)[0] == einval
            assert _rc(m, k, Bp, 0, Xp, 0, minv, work=work.ptr,
                       work_bytes=need)[0] == 0
        assert S._lib.spmv_live_handles() == made
    assert _rc(compact, k, Bp, 0, Xp, 0, Dp)[0] == -errno.ENOTSUP
    assert _rc(rm, k, Bp, 0, Xp, 0, Dp)[0] == einval
    for m in (d1, h1):  # M != N
        assert _rc(m, k, Bp, 0, Xp, 0, Dp)[0] == einval
    # no rows: 0, every record zero
    for m in (d0, h0):
        rc, rec = _rc(m, k, Bp, 0, Xp, 0, Dp)
        assert rc == 0
        assert [(r.status, r.iterations, r.rr, r.bb) for r in rec[:k]] == \
            [(0, 0, 0.0, 0.0)] * k
    S.stream_sync()
    assert S._lib.spmv_live_handles() == made

    # a capturing stream: -EBUSY, nothing enqueued, the capture ends cleanly
    side = S.Stream()
    for m in (d, cm):
        put(Xp, np.vstack([X0, np.zeros((PAST, k))]))
        S._check(S._lib.spmv_graph_begin_capture(side.ptr), "begin_capture")
        rc, _ = _rc(m, k, Bp, 0, Xp, 0, Dp, stream=side.ptr)
        rc_own, _ = _rc(m, k, Bp, 0, Xp, 0, None, work=work.ptr,
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
        with pytest.raises(OSError) as ei:
            m.bicgstab(Bp, Xp, k, d_minv=Dp)
        assert ei.value.errno == errno.ENODATA
    S.stream_sync()
    assert S._lib.spmv_live_handles() == made
    for m in (d, cm, rm, compact, d1, h1, d0, h0):
        m.release()
    assert S._lib.spmv_csr_bicgstab(C.c_void_p(1 << 20), None, k, Bp, 0, Xp, 0,
                                    Dp, TOL, 10, 0, None, 0,
                                    (S.CgInfo * 8)(), None) == -errno.EBADF
    assert S._lib.spmv_live_handles() == live
    work.free()
    bench.free()
    S.csr_free(A0)
    S.csr_free(A1)
