"""Smoothed-aggregation AMG on the device (spmv_csr_aggregate,
spmv_csr_amg_setup, spmv_amg_apply, spmv_*_pcg_amg; spmv_engine.h) against the
numpy restatement of tests/_amg.py.

The aggregation and its info are compared as integers, at two seeds, twice.
Every level of a hierarchy (A_l, P, PT, w, rho, omega) is compared as uint64.
A cycle is compared as uint64 with the restated cycle fed by launch_multi of
handles uploaded from the RESTATED levels (the same arrays, so the same lane
group and the same bits as the hierarchy's own handles); a solve with
tests/_pcg_trsv.py restate around that cycle.  There is no tolerance in this
file.

The shapes are the smallest on which the kernels can go wrong: 40 x 40 (more
than one workgroup, ten rounds), a 27-point grid, a hub row, an anisotropic
grid at theta 0.25 (line aggregates), a bidiagonal matrix whose edges are
stored on one side, a diagonal matrix, explicit zeros and a NaN, no rows and
one row; the hierarchy of 64 x 64 has four levels.

Every test runs under a time limit of its own (LIMIT_S): a test that exceeds
it ends the whole process, so nothing else is started on the device.
"""
import ctypes as C
import errno
import faulthandler

import numpy as np
import pytest

import _amg as AM
import _cg as G
import _pcg_trsv as PT
import spmv_scpa_amd as S
from test_gpu_cg import TOL, CgBench, as_solve, fill, put, same_solve
from test_gpu_multi_vector import FILL, PAST, bits
from test_gpu_pcg_trsv import Bench as TrsvBench
from test_gpu_pcg_trsv import GROUP, device_sgs

pytestmark = pytest.mark.gpu

LIMIT_S = 240
SENTINEL = -77


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def upload(mat, N=None, values="f64"):
    if len(mat) == 5:
        M, N, IRP, JA, AS = mat
    else:
        M, IRP, JA, AS = mat
    A = S.csr_from_arrays("amg", M, M if N is None else N,
                          np.asarray(IRP, np.int32), np.asarray(JA, np.int32),
                          AS)
    d = S.CsrDevice.upload(A, values=values)
    S.csr_free(A)
    return d


def ints(buf, n):
    return buf.to_numpy(np.int32, n) if n else np.zeros(0, np.int32)


def raw_aggregate(d, theta, seed, cap, d_agg, info=None):
    return S._lib.spmv_csr_aggregate(d.h, theta, seed, cap,
                                     d_agg.ptr if d_agg else None,
                                     C.byref(info) if info else None)


def numbers(info):
    return (info.aggregates, info.roots, info.rounds, info.widest,
            info.singletons)


# ------------------------------------------------------------ 1. aggregation
@pytest.mark.parametrize("name", list(AM.AGG))
def test_the_aggregation_has_the_integers_of_the_restatement(name):
    for seed in (0, 1):
        mat, theta, ref = AM.reference(name, seed)
        M = mat[0]
        want = (ref.aggregates, ref.roots, ref.rounds, ref.widest,
                ref.singletons)
        tag = (name, seed)
        d = upload(mat)
        live = S._lib.spmv_live_handles()
        for _ in range(2):  # the same integers from two calls
            ag = d.aggregate(theta=theta, seed=seed)
            got = (ag.aggregates, ag.roots, ag.rounds, ag.widest,
                   ag.singletons)
            print(tag, "aggregates, roots, rounds, widest, singletons", got)
            assert got == want, tag
            assert np.array_equal(ints(ag.agg, M), ref.agg), tag
            assert ag in S.live_objects()
            ag.release()
            assert ag not in S.live_objects()
        # the array or the info may be NULL; nothing past M is written
        a = S.DevBuffer.from_numpy(np.full(max(M, 4), SENTINEL, np.int32))
        info = S.AggregateInfo()
        assert raw_aggregate(d, theta, seed, 0, a, None) == 0, tag
        assert np.array_equal(ints(a, M), ref.agg), tag
        assert ints(a, max(M, 4))[M:].tolist() == [SENTINEL] * (max(M, 4) - M)
        assert raw_aggregate(d, theta, seed, 0, None, info) == 0, tag
        assert numbers(info) == want, tag
        assert S._lib.spmv_live_handles() == live, tag
        a.free()
        d.release()


# -------------------------------------------------------------- 2. hierarchy
def same_matrix(got, want, tag):
    assert got[0] == want[0] and got[1] == want[1], tag
    assert np.array_equal(got[2], want[2]), (tag, "IRP")
    assert np.array_equal(got[3], want[3]), (tag, "JA")
    assert np.array_equal(bits(got[4]), bits(want[4])), (tag, "AS")


def test_every_level_has_the_bits_of_the_restatement():
    levels = AM.reference_hierarchy(64)
    mat = levels[0].A
    d = upload(mat)
    live = S._lib.spmv_live_handles()
    for _ in range(2):
        H = d.amg()
        info = H.info
        print("hierarchy", info, S.amg_last_phases())
        assert H in S.live_objects()
        assert info["levels"] == len(levels) == 4
        assert info["rows"] == [l.A[0] for l in levels]
        assert info["entries"] == [len(l.A[2]) for l in levels]
        assert info["rounds"] == [l.agg.rounds if l.agg else 0
                                  for l in levels]
        assert info["aggregates"] == [l.agg.aggregates if l.agg else 0
                                      for l in levels]
        assert np.array_equal(bits(info["rho"]),
                              bits([l.rho for l in levels]))
        assert np.array_equal(bits(info["omega"]),
                              bits([l.omega for l in levels]))
        assert info["complexity"] == AM.complexity(levels)
        for l, want in enumerate(levels):
            got = H.level(l)
            M = want.A[0]
            same_matrix(got.A, (M, M) + want.A[1:], (l, "A"))
            assert np.array_equal(bits(got.w), bits(want.w)), (l, "w")
            if want.P is None:
                assert got.P is None and got.PT is None
            else:
                same_matrix(got.P, want.P, (l, "P"))
                same_matrix(got.PT, want.PT, (l, "PT"))
        # the hierarchy, and three handles per level below the coarsest
        assert S._lib.spmv_live_handles() == \
            live + 1 + 3 * (len(levels) - 1)
        H.release()
        assert H not in S.live_objects()
        assert S._lib.spmv_live_handles() == live
    d.release()


# ------------------------------------------------------------------ 3. apply
class Cycle:
    """the restated cycle on device products: handles uploaded from the
    restated levels, launch_multi through two buffers"""

    def __init__(self, levels, k):
        self.levels, self.k = levels, k
        self.h = []
        big = max(l.A[0] for l in levels) * k * 8
        self.X, self.Y = S.DevBuffer(big), S.DevBuffer(big)
        for l in levels:
            M = l.A[0]
            self.h.append((upload((M, M) + l.A[1:]),
                           upload(l.P) if l.P is not None else None,
                           upload(l.PT) if l.PT is not None else None))

    def product(self, h, **opts):
        def mul(X):
            k = X.shape[1]
            put(self.X.ptr, X)
            h.launch_multi(self.X.ptr, self.Y.ptr, k, **opts)
            S.stream_sync()
            return self.Y.to_numpy(np.float64, h.M * k).reshape(h.M, k)
        return mul

    def apply(self, sweeps=1, coarse_sweeps=8, **opts):
        prods = [tuple(self.product(h, **opts) if h is not None else None
                       for h in hs) for hs in self.h]
        return AM.cycle(self.levels, prods, sweeps, coarse_sweeps)

    def release(self):
        for hs in self.h:
            for h in hs:
                if h is not None:
                    h.release()
        self.X.free()
        self.Y.free()


def device_apply(H, R, ldr=0, ldz=0, **kw):
    """-> Z (M, k) and the whole buffer, padding and guard rows filled"""
    M, k = R.shape
    lr, lz = ldr or k, ldz or k
    Rh = np.full((M + PAST, lr), np.nan)
    Rh[:M, :k] = R
    Zh = np.empty((M + PAST, lz))
    bits(Zh)[:] = FILL
    dR, dZ = S.DevBuffer.from_numpy(Rh), S.DevBuffer.from_numpy(Zh)
    H.apply(dR.ptr, dZ.ptr, k, ldr=ldr, ldz=ldz, **kw)
    S.stream_sync()
    Zf = dZ.to_numpy(np.float64, (M + PAST) * lz).reshape(M + PAST, lz)
    assert np.array_equal(bits(dR.to_numpy(np.float64, (M + PAST) * lr)),
                          bits(Rh.ravel())), "R was written"
    assert np.all(bits(Zf[:M, k:]) == FILL) and np.all(bits(Zf[M:]) == FILL)
    dR.free()
    dZ.free()
    return Zf[:M, :k]


@pytest.mark.parametrize("sweeps,max_levels", [(1, 16), (2, 16), (1, 1)])
def test_a_cycle_has_the_bits_of_the_restatement(sweeps, max_levels):
    levels = AM.reference_hierarchy(64, max_levels=max_levels)
    assert len(levels) == (4 if max_levels > 1 else 1)
    mat = levels[0].A
    M = mat[0]
    R8 = np.random.default_rng(3).standard_normal((M, 8))
    R8[:, 5] = 0.0
    d = upload(mat)
    H = d.amg(sweeps=sweeps, max_levels=max_levels)
    cyc = Cycle(levels, 8)
    want8 = cyc.apply(sweeps)(R8)
    # the fused sweep (one launch a sweep) and the composition it replaces
    # (a product and a vector kernel): the same bits.  Mode 1 is the rule:
    # fused from k = 4 on; the launch count is that of k = kmax = 8
    for mode, fine, coarse in ((2, 2 * sweeps + 3, 8), (1, 2 * sweeps + 3, 8),
                               (0, 4 * sweeps + 3, 15)):
        assert S.amg_set_fused(mode) in (0, 1, 2)
        assert H.info["launches"] == (3 * fine + coarse if max_levels > 1
                                      else coarse)
        for k in (1, 2, 3, 4, 5, 6, 7, 8):
            got = device_apply(H, R8[:, :k], ldr=k + 2 if k < 8 else 0,
                               ldz=k + 1 if k < 8 else 0)
            assert np.array_equal(bits(got), bits(want8[:, :k])), \
                (mode, sweeps, k)
    assert S.amg_set_fused(1) == 0
    with pytest.raises(OSError):
        S.amg_set_fused(3)
    # a column does not depend on k or on its neighbours
    for j in (0, 5, 7):
        one = device_apply(H, R8[:, j:j + 1])
        assert np.array_equal(bits(one[:, 0]), bits(want8[:, j])), j
    # nor on the workgroup size
    for waves in (1, 8):
        got = device_apply(H, R8[:, :3], waves_per_block=waves)
        assert np.array_equal(bits(got), bits(want8[:, :3])), waves
    # a captured graph replayed twice
    dR = S.DevBuffer.from_numpy(R8[:, :3].copy())
    dZ = S.DevBuffer(M * 3 * 8)
    st = S.Stream()
    with st.capture() as graph:
        H.apply(dR.ptr, dZ.ptr, 3, stream=st.ptr)
    for _ in range(2):
        fill(dZ)
        S.stream_sync()
        graph.launch(st.ptr)
        st.sync()
        Z = dZ.to_numpy(np.float64, M * 3).reshape(M, 3)
        assert np.array_equal(bits(Z), bits(want8[:, :3]))
    graph.destroy()
    for h in (dR, dZ):
        h.free()
    cyc.release()
    H.release()
    d.release()


def test_a_level_with_a_long_row_sweeps_by_the_composition():
    """row 0 of the arrow matrix holds more than 2048 entries: not the fused
    kernel's; the cycle has the bits of the restatement all the same"""
    mat = AM.int32(G.arrow(2100, 3))
    assert mat[1][1] > 2048
    levels = AM.hierarchy(mat)
    assert [l.A[0] for l in levels] == [2100, 1]
    M = mat[0]
    R = np.random.default_rng(4).standard_normal((M, 3))
    d = upload(mat)
    H = d.amg(sweeps=2)
    assert H.info["rows"] == [2100, 1]
    assert H.info["launches"] == (4 * 2 + 3) + 8   # composed, fused
    cyc = Cycle(levels, 3)
    want = cyc.apply(2)(R)
    got = device_apply(H, R, ldr=5, ldz=4)
    assert np.array_equal(bits(got), bits(want))
    cyc.release()
    H.release()
    d.release()


# ---------------------------------------------------------------- 4. pcg_amg
class AmgBench(CgBench):
    def solve(self, m, B, X0, H, ldb=0, ldx=0, shift=0, **kw):
        """as CgBench.solve, through pcg_amg() with the hierarchy H"""
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
        rec = m.pcg_amg(self.B.ptr, self.X.ptr + shift, H, k=k, ldb=ldb,
                        ldx=ldx, **kw)
        S.stream_sync()
        Xf = self.X.to_numpy(np.float64, (M + PAST) * lx + shift // 8)
        Bf = self.B.to_numpy(np.float64, (M + PAST) * lb)
        assert np.array_equal(bits(Bf), bits(Bh.ravel())), "B was written"
        return rec, Xf[shift // 8:].reshape(M + PAST, lx), Bh


def test_a_solve_has_the_bits_of_the_restatement():
    levels = AM.reference_hierarchy(64)
    mat = levels[0].A
    M = mat[0]
    k = 4
    B, X0 = G.common_inputs(M, k)
    bench = AmgBench(M)
    d = upload(mat)
    hs = {"csr": d, "hll": d.to_hll(True)}
    live = S._lib.spmv_live_handles()
    H = d.amg()
    cyc = Cycle(levels, k)
    work = S.DevBuffer(S.pcg_trsv_work_bytes(M, k))
    for fmt, m in hs.items():
        product, residual0 = bench.callables(m, B, X0)
        want = AM.pcg_amg(product, residual0, B, X0, cyc.apply(), TOL, 200)
        rec, Xf, _ = bench.solve(m, B, X0, H, ldb=k + 2, ldx=k + 1, shift=8,
                                 tol=TOL, maxit=200)
        same_solve(rec, Xf[:M], want, fmt)
        assert [r.status for r in rec] == [0] * k, fmt
        # the zero column converged at once, the others far below Jacobi
        assert rec[1].iterations == 0 and rec[1].bb == 0.0
        assert np.array_equal(bits(Xf[:M, 1]), bits(X0[:, 1]))
        assert 0 < max(r.iterations for r in rec) <= 40, fmt
        # a converged column is frozen: the columns stop at different counts
        # and the solve stopped by maxit keeps the bits of the converged ones
        base = as_solve(rec, Xf[:M])
        for kw in (dict(check_every=1), dict(check_every=7),
                   dict(work=work), dict(waves_per_block=8)):
            rec2, Xf2, _ = bench.solve(m, B, X0, H, tol=TOL, maxit=200, **kw)
            same_solve(rec2, Xf2[:M], base, (fmt, kw))
        its = [r.iterations for r in rec]
        few = min(i for i in its if i)
        assert few < max(its)
        want5 = AM.pcg_amg(product, residual0, B, X0, cyc.apply(), TOL, few)
        rec5, Xf5, _ = bench.solve(m, B, X0, H, tol=TOL, maxit=few)
        same_solve(rec5, Xf5[:M], want5, (fmt, "maxit", few))
        # the slowest column was stopped by maxit, the others had converged
        assert sorted(r.status for r in rec5) == [0, 0, 0, 1], fmt
        for j, r in enumerate(rec5):
            if r.status == 0:
                assert np.array_equal(bits(Xf5[:M, j]), bits(Xf[:M, j])), j
    work.free()
    cyc.release()
    H.release()
    assert S._lib.spmv_live_handles() == live
    # pcg_trsv on the same matrix keeps its bits
    tb = TrsvBench(M)
    pre = device_sgs(d)
    B3, X3 = G.common_inputs(M, 3)
    for fmt, m in hs.items():
        want = tb.want(m, B3, X3, PT.sgs(mat))
        rec, Xf, _ = tb.solve(m, B3, X3, pre, tol=TOL, maxit=200)
        same_solve(rec, Xf[:M], want, ("pcg_trsv", fmt))
    pre.release()
    for m in hs.values():
        m.release()
    bench.free()
    tb.free()


# ----------------------------------------------------------------- 5. errors
def test_refusals_in_their_order_leave_nothing_behind():
    mat = AM.lap2d(12, 11)
    M = mat[0]
    d = upload(mat)
    f32 = upload(mat, values="f32")
    rect = upload(mat, N=M + 1)
    JA = mat[2].copy()
    JA[[0, 1]] = JA[[1, 0]]                     # row 0 descending
    unsorted = upload((M, mat[1], JA, mat[3]))
    keep = np.ones(len(mat[2]), bool)
    keep[mat[1][3]:mat[1][4]] = mat[2][mat[1][3]:mat[1][4]] != 3
    IRP = np.concatenate([[0], np.cumsum(np.bincount(
        AM.rows_of(M, mat[1])[keep], minlength=M))]).astype(np.int32)
    nodiag = upload((M, IRP, mat[2][keep], mat[3][keep]))
    AS = mat[3].copy()
    AS[AM.rows_of(M, mat[1]) == mat[2]] = 0.0
    zerod = upload((M, mat[1], mat[2], AS))     # rho is not finite
    other = upload(AM.lap2d(5, 5))
    JA2 = mat[2].copy()
    JA2[-1] = M + 3                             # a column outside [0, M)
    outside = upload((M, mat[1], JA2, mat[3]))
    nosrc = upload(mat)
    try:
        S.set_panel_schedule("chain")
        nosrc.build_panels(0)
        nosrc.release_source()
    finally:
        S.set_panel_schedule("sweep")
    dead = upload(mat)
    dead_h = dead.h
    dead.release()
    live = S._lib.spmv_live_handles()
    a = S.DevBuffer.from_numpy(np.full(M, SENTINEL, np.int32))
    info = S.AggregateInfo(5, 5, 5, 5, 5)
    E = errno
    for rc, args in (
            (E.EINVAL, (None, 0.0, 0, 0)), (E.EINVAL, (d.h, -1.0, 0, 0)),
            (E.EINVAL, (d.h, float("nan"), 0, 0)),
            (E.EINVAL, (d.h, 0.0, 0, -1)), (E.EBADF, (dead_h, 0.0, 0, 0)),
            (E.EINVAL, (rect.h, 0.0, 0, 0)), (E.ENOTSUP, (f32.h, 0.0, 0, 0)),
            (E.ENODATA, (nosrc.h, 0.0, 0, 0)),
            (E.EDOM, (outside.h, 0.0, 0, 0)),
            (E.EINVAL, (unsorted.h, 0.0, 0, 0)),
            (E.EINVAL, (nodiag.h, 0.0, 0, 0)), (E.E2BIG, (d.h, 0.0, 0, 1))):
        assert S._lib.spmv_csr_aggregate(*args, a.ptr, C.byref(info)) == -rc, \
            (rc, args)
        assert numbers(info) == (5, 5, 5, 5, 5)
        assert set(ints(a, M).tolist()) == {SENTINEL}
        assert S._lib.spmv_live_handles() == live
    h = C.c_void_p(77)

    def setup(A, theta=0.0, sweeps=1, coarse=8, min_rows=32, levels=16,
              kmax=8):
        return S._lib.spmv_csr_amg_setup(A, theta, sweeps, coarse, min_rows,
                                         levels, 0, kmax, C.byref(h))
    for rc, kw in ((E.EINVAL, dict(A=None)), (E.EINVAL, dict(A=d.h, sweeps=0)),
                   (E.EINVAL, dict(A=d.h, coarse=65)),
                   (E.EINVAL, dict(A=d.h, min_rows=0)),
                   (E.EINVAL, dict(A=d.h, levels=33)),
                   (E.EINVAL, dict(A=d.h, kmax=9)),
                   (E.EBADF, dict(A=dead_h)), (E.EINVAL, dict(A=rect.h)),
                   (E.ENOTSUP, dict(A=f32.h)), (E.ENODATA, dict(A=nosrc.h)),
                   (E.EDOM, dict(A=outside.h)),
                   (E.EINVAL, dict(A=unsorted.h)),
                   (E.EINVAL, dict(A=nodiag.h)), (E.EDOM, dict(A=zerod.h))):
        h.value = 77
        assert setup(**kw) == -rc, (rc, kw)
        assert h.value is None, kw
        assert S._lib.spmv_live_handles() == live
    # the cycle and the solver
    H = d.amg(kmax=4, min_rows=16)
    Ho = other.amg()
    assert H.info["levels"] > 1
    Z = S.DevBuffer.from_numpy(np.full(8 * M, -77.0))
    R = S.DevBuffer.from_numpy(np.ones(8 * M))
    o = S.LaunchOpts()
    bad = S.LaunchOpts(group=4)
    ap = S._lib.spmv_amg_apply
    for rc, args in ((E.EINVAL, (None, o, 1, R.ptr, 0, Z.ptr, 0)),
                     (E.EBADF, (dead_h, o, 1, R.ptr, 0, Z.ptr, 0)),
                     (E.EINVAL, (H.h, o, 0, R.ptr, 0, Z.ptr, 0)),
                     (E.EINVAL, (H.h, o, 5, R.ptr, 0, Z.ptr, 0)),
                     (E.EINVAL, (H.h, o, 2, R.ptr, 1, Z.ptr, 0)),
                     (E.EINVAL, (H.h, o, 2, R.ptr, 0, Z.ptr, 1)),
                     (E.EINVAL, (H.h, o, 1, None, 0, Z.ptr, 0)),
                     (E.EINVAL, (H.h, o, 1, R.ptr, 0, None, 0)),
                     (E.EINVAL, (H.h, o, 1, R.ptr, 0, R.ptr, 0)),
                     (E.EINVAL, (H.h, bad, 1, R.ptr, 0, Z.ptr, 0))):
        got = ap(args[0], C.byref(args[1]), *args[2:], None)
        assert got == -rc, (rc, args[2:])
    rec = (S.CgInfo * 8)()

    def solve(m, Hh, k=2, X=Z.ptr):
        return m._fn("pcg_amg")(m.h, None, k, R.ptr, 0, X, 0, Hh, TOL, 10, 0,
                                None, 0, rec, None)
    hll = d.to_hll(True)
    for m in (d, hll):
        assert solve(m, H.h, k=9) == -E.EINVAL       # pcg's own checks first
        assert solve(m, H.h, X=None) == -E.EINVAL
        assert solve(m, None) == -E.EINVAL
        assert solve(m, dead_h) == -E.EBADF
        assert solve(m, Ho.h) == -E.EINVAL           # another M
        assert solve(m, H.h, k=5) == -E.EINVAL       # k > kmax
    S.stream_sync()
    assert set(Z.to_numpy(np.float64, 8 * M).tolist()) == {-77.0}
    with pytest.raises(ValueError):
        H.apply(R.ptr, Z.ptr, 5)
    with pytest.raises(ValueError):
        d.pcg_amg(R.ptr, Z.ptr, None)
    # a hierarchy whose fine handle was released
    lone = upload(mat)
    Hl = lone.amg()
    lone.release()
    assert ap(Hl.h, C.byref(o), 1, R.ptr, 0, Z.ptr, 0, None) == -E.EBADF
    assert solve(d, Hl.h) == -E.EBADF
    # ... also when the allocator hands its address to a newer handle
    again = [upload(AM.lap2d(5, 5)) for _ in range(8)]
    assert ap(Hl.h, C.byref(o), 1, R.ptr, 0, Z.ptr, 0, None) == -E.EBADF
    assert Hl.info["levels"] >= 1
    for x in again:
        x.release()
    for x in (Hl, H, Ho, hll):
        x.release()
    assert S._lib.spmv_live_handles() == live
    for x in (Z, R, a, d, f32, rect, unsorted, nodiag, zerod, other, outside,
              nosrc):
        x.free() if isinstance(x, S.DevBuffer) else x.release()
