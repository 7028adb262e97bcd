"""BiCGStab preconditioned by triangular plans (spmv_*_bicgstab_trsv;
spmv_engine.h) on the GPU: CSR and column-major HLL handles, ILU(0) and
symmetric Gauss-Seidel, 1-8 interleaved systems.

Everything is compared as uint64: a solve against the numpy restatement
(tests/_ilu0.py restate) fed with both products from the SAME handle's
launch_multi, the initial residual from its launch_axpby and Z = apply(U) from
the restated plans (tests/_trsv.py; the factor from tests/_ilu0.py).  An
identity plan against bicgstab() and a power-of-two diagonal plan against
bicgstab(d_minv) on the same handle.  The one tolerance is the sanity line of
test_gpu_cg: the true residual of the device's X, computed on the host, is at
most 2 tol.

The matrices are the stencils of tests/test_gpu_ilu0.py: 1073 rows, the natural
order (the chain kernels alone) and the red-black order (the wide kernels
alone).  Every test runs under a time limit of its own (LIMIT_S).
"""
import ctypes as C
import errno
import faulthandler

import numpy as np
import pytest

import _cg as G
import _ilu0 as IL
import _oracle as O
import _pcg_trsv as PT
import _trsv as TV
import spmv_scpa_amd as S
from test_gpu_cg import (TOL, CgBench, as_solve, fill, neighbours_kept, put,
                         same_solve, upload)
from test_gpu_multi_vector import FILL, PAST, bits

pytestmark = pytest.mark.gpu

LIMIT_S = 240
GROUP = S.trsv_shape()["group"]
STENCILS = ["convdiff(37,29)", "red-black convdiff(37,29)"]


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


class Precond:
    """the device side of one preconditioner: (first, second, d_scale) and
    what to release"""

    def __init__(self, first, second=None, scale=None, own=()):
        self.first, self.second, self.scale = first, second, scale
        self.own = list(own)

    @property
    def kw(self):
        return dict(first=self.first, second=self.second,
                    d_scale=self.scale.ptr if self.scale is not None
                    else None)

    def release(self):
        for h in self.own:
            (h.free if isinstance(h, S.DevBuffer) else h.release)()


def device_sgs(csr):
    sg = csr.sgs()
    return Precond(*sg.args[:2], scale=sg.diag, own=[sg])


def device_ilu0(csr, shift=0.0):
    LU, info = csr.ilu0(shift=shift)
    lo, up = LU.trsv_analyse("lower", unit=True), LU.trsv_analyse("upper")
    LU.release()    # the plans own what they need
    return Precond(lo, up, own=[lo, up])


def device_diagonal(d, unit=False):
    """the lower plan of diag(d)"""
    M = len(d)
    A = S.csr_from_arrays("diag", M, M, np.arange(M + 1), np.arange(M), d)
    h = S.CsrDevice.upload(A)
    S.csr_free(A)
    plan = h.trsv_analyse("lower", unit=unit)
    h.release()
    return Precond(plan, own=[plan])


DEVICE = {"sgs": device_sgs, "ilu0": device_ilu0}
HOST = {"sgs": PT.sgs, "ilu0": IL.ilu0}


class Bench(CgBench):
    def want(self, m, B, X0, pc, tol=TOL, maxit=200, **opts):
        product, residual0 = self.callables(m, B, X0, **opts)
        return IL.restate(product, residual0, B, X0,
                          PT.plans_apply(*pc, GROUP), tol, maxit)

    def solve(self, m, B, X0, pre, ldb=0, ldx=0, shift=0, **kw):
        """as CgBench.solve, through bicgstab_trsv() with the Precond `pre`;
        asserts that the scale was not written"""
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
        before = (pre.scale.to_numpy(np.uint64, M)
                  if pre.scale is not None else None)
        rec = m.bicgstab_trsv(self.B.ptr, self.X.ptr + shift, k=k, ldb=ldb,
                              ldx=ldx, **pre.kw, **kw)
        S.stream_sync()
        Xf = self.X.to_numpy(np.float64, (M + PAST) * lx + shift // 8)
        Bf = self.B.to_numpy(np.float64, (M + PAST) * lb)
        assert np.array_equal(bits(Bf), bits(Bh.ravel())), "B was written"
        if pre.scale is not None:
            assert np.array_equal(pre.scale.to_numpy(np.uint64, M), before)
        return rec, Xf[shift // 8:].reshape(M + PAST, lx), Bh

    def plain(self, m, B, X0, minv=None, **kw):
        """bicgstab() on the same buffers -> _cg.Solve"""
        M, k = B.shape
        put(self.B.ptr, B)
        put(self.X.ptr, X0)
        rec = m.bicgstab(self.B.ptr, self.X.ptr, k,
                         d_minv=minv.ptr if minv is not None else None, **kw)
        S.stream_sync()
        return as_solve(rec, self.X.to_numpy(np.float64, M * k).reshape(M, k))


# -------------------------------------------------------------------- 1. bits
@pytest.mark.parametrize("which", ["ilu0", "sgs"])
@pytest.mark.parametrize("name", STENCILS)
def test_a_solve_has_the_bits_of_the_restatement(name, which):
    mat = IL.MATRICES[name]()
    M, IRP, JA, AS = mat
    pc = HOST[which](mat)
    bench = Bench(M)
    hs = upload(mat, "f64")
    live = S._lib.spmv_live_handles()
    pre = DEVICE[which](hs["csr"])
    for fmt, m in hs.items():
        for k in (1, 3, 8):
            tag = (name, which, fmt, k)
            B, X0 = G.common_inputs(M, k)
            want = bench.want(m, B, X0, pc)
            # ldx > k once: at k = 3, with an unaligned X as well
            stride = dict(ldb=k + 2, ldx=k + 1, shift=8) if k == 3 else {}
            rec, Xf, _ = bench.solve(m, B, X0, pre, tol=TOL, maxit=200,
                                     **stride)
            same_solve(rec, Xf[:M], want, tag)
            neighbours_kept(Xf, M, k, tag)
            assert [r.status for r in rec] == [0] * k, tag
            if k > 1:  # the zero column: converged at once, X untouched
                assert rec[1].iterations == 0 and rec[1].bb == 0.0, tag
                assert np.array_equal(bits(Xf[:M, 1]), bits(X0[:, 1])), tag
            # the sanity line: the true residual of the device's X
            res = G.true_residual(IRP, JA, AS, O.csr_spmv, B, Xf[:M, :k])
            print(tag, "true residual", res)
            assert np.all(res <= 2 * TOL), (tag, res)
        # stopped by maxit
        B, X0 = G.common_inputs(M, 3)
        want3 = bench.want(m, B, X0, pc, maxit=3)
        rec, Xf, _ = bench.solve(m, B, X0, pre, tol=TOL, maxit=3)
        same_solve(rec, Xf[:M], want3, (name, which, fmt, "maxit 3"))
        assert [r.status for r in rec] == [1, 0, 1], (name, which, fmt)
    pre.release()
    assert S._lib.spmv_live_handles() == live
    for m in hs.values():
        m.release()
    bench.free()


def test_ilu0_takes_fewer_iterations_than_jacobi_on_the_device():
    mat = IL.MATRICES["convdiff(37,29)"]()
    M = mat[0]
    B, X0 = G.common_inputs(M, 1)
    bench = Bench(M)
    hs = upload(mat, "f64")
    m = hs["csr"]
    minv = S.DevBuffer(M * 8)
    m.diag(minv.ptr, invert=True)
    jacobi = bench.plain(m, B, X0, minv, tol=TOL, maxit=1000)
    pre = device_ilu0(m)
    rec, _, _ = bench.solve(m, B, X0, pre, tol=TOL, maxit=1000)
    print("ilu0", rec[0].iterations, "jacobi", jacobi.iterations)
    assert rec[0].status == 0 and jacobi.status == [0]
    assert rec[0].iterations < jacobi.iterations[0]
    pre.release()
    minv.free()
    for h in hs.values():
        h.release()
    bench.free()


# ----------------------------------------------- 2. properties of the contract
def test_an_identity_plan_is_bicgstab_and_a_power_of_two_diagonal_its_minv():
    mat = IL.MATRICES["convdiff(37,29)"]()
    M = mat[0]
    B, X0 = G.common_inputs(M)
    bench = Bench(M)
    hs = upload(mat, "f64")
    d = 2.0 ** np.random.default_rng(3).integers(-6, 7, M)
    minv = S.DevBuffer.from_numpy(1.0 / d)
    ident = device_diagonal(np.ones(M))
    unit = device_diagonal(np.full(M, 7.0), unit=True)
    pow2 = device_diagonal(d)
    for fmt, m in hs.items():
        for maxit in (40, 7):   # converged (33 steps at the most), cut short
            plain = bench.plain(m, B, X0, tol=TOL, maxit=maxit)
            for nm, pre in (("identity", ident), ("unit", unit)):
                rec, Xf, _ = bench.solve(m, B, X0, pre, tol=TOL, maxit=maxit)
                same_solve(rec, Xf[:M], plain, (fmt, nm, maxit))
            diag = bench.plain(m, B, X0, minv, tol=TOL, maxit=maxit)
            rec, Xf, _ = bench.solve(m, B, X0, pow2, tol=TOL, maxit=maxit)
            same_solve(rec, Xf[:M], diag, (fmt, "2^n", maxit))
            if maxit == 40:  # the random scaling itself does not converge
                assert list(plain.status) == [0, 0, 0, 0]
                assert list(diag.iterations) == [40, 0, 40, 40]
    for pre in (ident, unit, pow2):
        pre.release()
    minv.free()
    for m in hs.values():
        m.release()
    bench.free()


# ------------------------------------------------------------ 3. independence
@pytest.mark.parametrize("name", STENCILS)
def test_the_result_depends_on_the_system_alone(name):
    mat = IL.MATRICES[name]()
    M, IRP, JA, AS = mat
    B, X0 = G.common_inputs(M)
    # column 2 starts six digits from its solution: it stops long before
    # columns 0 and 3, and has to keep its bits while they go on
    X0[:, 2] = np.linalg.solve(IL.dense_of(*mat), B[:, 2]) * (
        1.0 + 1e-6 * np.random.default_rng(4).uniform(-1.0, 1.0, M))
    bench = Bench(M)
    hs = upload(mat, "f64")
    work = S.DevBuffer(S.bicgstab_trsv_work_bytes(M, 8))
    pre = device_ilu0(hs["csr"])
    for fmt, m in hs.items():
        rec, Xf, _ = bench.solve(m, B, X0, pre, tol=TOL, maxit=200)
        base = as_solve(rec, Xf[:M])
        assert base.status == [0, 0, 0, 0]
        assert base.iterations[1] == 0
        assert 0 < base.iterations[2] < min(base.iterations[0],
                                            base.iterations[3])
        for kw in (dict(check_every=1), dict(check_every=7),
                   dict(work=work), dict(waves_per_block=16)):
            rec, Xf, _ = bench.solve(m, B, X0, pre, ldx=6, tol=TOL,
                                     maxit=200, **kw)
            same_solve(rec, Xf[:M], base, (name, fmt, kw))
            neighbours_kept(Xf, M, 4, (name, fmt, kw))
        # column j of the k = 4 solve is the k = 1 solve of that column: a
        # column frozen early kept its bits while the others went on
        for j in range(4):
            rec, Xf, _ = bench.solve(m, B[:, j:j + 1], X0[:, j:j + 1], pre,
                                     tol=TOL, maxit=200)
            assert rec[0].status == base.status[j]
            assert rec[0].iterations == base.iterations[j]
            assert bits(np.array([rec[0].rr]))[0] == bits(base.rr)[j]
            assert np.array_equal(bits(Xf[:M, 0]), bits(base.X[:, j])), \
                (name, fmt, j)
    pre.release()
    work.free()
    for m in hs.values():
        m.release()
    bench.free()


# ---------------------------------------------------------------- 4. breakdown
def test_a_nan_factor_is_a_breakdown_and_not_a_fault():
    """a zero pivot in row 0 of the stencil leaves inf / NaN in the factor, so
    Z = z(P) is NaN and rv with it: the columns that run break down at their
    first rv, with 0 iterations and X untouched.

    No running column can escape that, whatever its right-hand side: a plan
    solves all k columns, and a row of the factor that holds an inf or a NaN
    multiplies it with the column's z even where that is 0.0 (0 * inf is NaN),
    the product A Z carries the NaN into V, and rv = Rh . V sums 0 * NaN.  So
    the columns that end converged beside a poisoned factor are those that do
    not run: the zero column, and column 2, which starts AT its solution with
    a right-hand side that is not zero -- their X keeps its bits although
    their Z is NaN like everybody's"""
    mat = IL.with_zero_pivot(IL.MATRICES["convdiff(37,29)"](), 0)
    M = mat[0]
    B, X0 = G.common_inputs(M)
    X0[:, 2] = np.linalg.solve(IL.dense_of(*mat), B[:, 2])
    pc = IL.ilu0(mat)
    bench = Bench(M)
    hs = upload(mat, "f64")
    LU, info = hs["csr"].ilu0()
    assert info.bad_pivots > 1
    LU.release()
    pre = device_ilu0(hs["csr"])
    for fmt, m in hs.items():
        want = bench.want(m, B, X0, pc, maxit=50)
        rec, Xf, _ = bench.solve(m, B, X0, pre, tol=TOL, maxit=50)
        same_solve(rec, Xf[:M], want, fmt)
        assert [(r.status, r.iterations) for r in rec] == \
            [(2, 0), (0, 0), (0, 0), (2, 0)], fmt
        assert rec[2].bb > 0.0 and np.any(X0[:, 2] != 0.0), fmt
        assert np.array_equal(bits(Xf[:M, :4]), bits(X0)), fmt
    pre.release()
    # with a healthy factor of the neighbouring matrix the same systems
    # converge: the preconditioner need not belong to A
    near = upload(IL.MATRICES["convdiff(37,29)"](), "f64")
    pre = device_ilu0(near["csr"])
    rec, _, _ = bench.solve(hs["csr"], B, X0, pre, tol=TOL, maxit=200)
    assert [r.status for r in rec] == [0, 0, 0, 0]
    pre.release()
    for m in list(hs.values()) + list(near.values()):
        m.release()
    bench.free()


# --------------------------------------------------------------- 5. refusals
def _rc(m, k, Bp, Xp, first, second, scale, tol=TOL, maxit=3, check_every=0,
        work=None, work_bytes=0, stream=None, ldb=0, ldx=0):
    info = (S.CgInfo * 8)()
    o = S._opts()
    rc = m._fn("bicgstab_trsv")(m.h, C.byref(o), k, Bp, ldb, Xp, ldx, first,
                                second, scale, tol, maxit, check_every, work,
                                work_bytes, info, stream)
    return rc, info


def test_the_refusals_and_a_capturing_stream():
    mat = IL.MATRICES["convdiff(37,29)"]()
    M = mat[0]
    k = 4
    B, X0 = G.common_inputs(M)
    bench = Bench(M)
    hs = upload(mat, "f64")
    sg = hs["csr"].sgs()
    lo, up, Dp = sg.lower.h, sg.upper.h, sg.diag.ptr
    small = device_diagonal(np.ones(M - 1))  # a plan of another size
    junk = C.cast(C.create_string_buffer(512), C.c_void_p)
    Bp, Xp = bench.B.ptr, bench.X.ptr
    put(Bp, B)
    put(Xp, X0)
    need = S.bicgstab_trsv_work_bytes(M, k)
    work = S.DevBuffer(need)
    einval = -errno.EINVAL
    live = S._lib.spmv_live_handles()
    for m in hs.values():
        # bicgstab's checks first ...
        assert _rc(m, 0, Bp, Xp, lo, up, Dp)[0] == einval
        assert _rc(m, 9, Bp, Xp, lo, up, Dp)[0] == einval
        assert _rc(m, k, None, Xp, lo, up, Dp)[0] == einval
        assert _rc(m, k, Bp, Xp, lo, up, Dp, ldx=3)[0] == einval
        assert _rc(m, k, Bp, Xp, lo, up, Dp, tol=-1.0)[0] == einval
        assert _rc(m, k, Bp, Xp, lo, up, Dp, maxit=-1)[0] == einval
        # ... a bad tol outranks a dead plan, a missing plan outranks a dead
        # one, and a dead plan its size
        assert _rc(m, k, Bp, Xp, junk, up, Dp, tol=-1.0)[0] == einval
        assert _rc(m, k, Bp, Xp, None, up, Dp)[0] == einval
        assert _rc(m, k, Bp, Xp, lo, None, Dp)[0] == einval   # scale alone
        assert _rc(m, k, Bp, Xp, junk, None, Dp)[0] == einval
        assert _rc(m, k, Bp, Xp, junk, up, Dp)[0] == -errno.EBADF
        assert _rc(m, k, Bp, Xp, lo, junk, Dp)[0] == -errno.EBADF
        assert _rc(m, k, Bp, Xp, small.first.h, junk, None)[0] == -errno.EBADF
        assert _rc(m, k, Bp, Xp, small.first.h, up, Dp)[0] == einval
        assert _rc(m, k, Bp, Xp, lo, small.first.h, None)[0] == einval
        # the work buffer: bicgstab's size is one vector short
        assert _rc(m, k, Bp, Xp, lo, up, Dp, work=work.ptr,
                   work_bytes=S.bicgstab_work_bytes(M, k))[0] == einval
        assert _rc(m, k, Bp, Xp, lo, up, Dp, work=work.ptr + 4,
                   work_bytes=need)[0] == einval
        assert S._lib.spmv_live_handles() == live
        got = bench.X.to_numpy(np.float64, M * k).reshape(M, k)
        assert np.array_equal(bits(got), bits(X0)), "something was enqueued"
    # a capturing stream: -EBUSY, nothing enqueued, the capture ends cleanly
    side = S.Stream()
    for m in hs.values():
        S._check(S._lib.spmv_graph_begin_capture(side.ptr), "begin_capture")
        rc, _ = _rc(m, k, Bp, Xp, lo, up, Dp, stream=side.ptr)
        rc_own, _ = _rc(m, k, Bp, Xp, lo, up, Dp, work=work.ptr,
                        work_bytes=need, stream=side.ptr)
        g = C.c_void_p()
        end = S._lib.spmv_graph_end_capture(side.ptr, C.byref(g))
        if end == 0:
            S._check(S._lib.spmv_graph_destroy(g), "spmv_graph_destroy")
        assert rc == -errno.EBUSY and rc_own == -errno.EBUSY
        assert end == 0, "the capture was invalidated"
        got = bench.X.to_numpy(np.float64, M * k).reshape(M, k)
        assert np.array_equal(bits(got), bits(X0)), "something was enqueued"
        # ... and the stream solves afterwards, in the caller's buffer
        rc, rec = _rc(m, k, Bp, Xp, lo, up, Dp, maxit=200, work=work.ptr,
                      work_bytes=need, stream=side.ptr)
        assert rc == 0 and [r.status for r in rec[:k]] == [0, 0, 0, 0]
        put(Xp, X0)
    side.sync()
    # a released plan is a dead plan; no rows: 0 and zero records
    sg.release()
    assert _rc(hs["csr"], k, Bp, Xp, lo, None, None)[0] == -errno.EBADF
    e = S.CsrDevice.upload(S.csr_from_arrays("e", 0, 0, *TV.empty()[1:]))
    p0 = e.trsv_analyse("lower")
    rc, rec = _rc(e, k, Bp, Xp, p0.h, None, None)
    assert rc == 0
    assert [(r.status, r.iterations, r.rr, r.bb) for r in rec[:k]] == \
        [(0, 0, 0.0, 0.0)] * k
    for h in (p0, e, small, work):
        (h.free if isinstance(h, S.DevBuffer) else h.release)()
    for m in hs.values():
        m.release()
    bench.free()
