"""Sweep plans (spmv_csr_trsv_analyse_sweeps; spmv_engine.h) as the
preconditioner of the solvers that take plans, on the GPU: spmv_*_pcg_trsv
with IC(0) and symmetric Gauss-Seidel, spmv_*_bicgstab_trsv and
spmv_*_gmres_trsv with ILU(0), on a CSR handle and on its HLL handle.

Everything is compared as uint64, against the numpy restatements of the
solvers (tests/_pcg_trsv.py, tests/_ilu0.py, tests/_gmres.py) fed with the
product and the residual of the SAME handle, as the existing solver tests do,
and with Z = apply(R) from the restated sweeps (tests/_trsv_sweeps.py).  The
one tolerance is the sanity line of test_gpu_cg: the true residual of the
device's X is at most 2 tol.  Every test runs under a time limit of its own.
"""
import ctypes as C
import errno
import faulthandler

import numpy as np
import pytest

import _bicgstab as BI
import _cg as G
import _ilu0 as IL
import _oracle as O
import _pcg_trsv as PT
import _trsv_sweeps as SW
import spmv_scpa_amd as S
from test_gpu_bicgstab_trsv import Bench as BiBench, Precond
from test_gpu_cg import (TOL, as_solve, fill, neighbours_kept, put, same_solve,
                         upload)
from test_gpu_gmres import GmBench, same as same_gmres
from test_gpu_multi_vector import bits
from test_gpu_pcg_trsv import Bench as CgBench

pytestmark = pytest.mark.gpu

LIMIT_S = 240
GROUP = S.trsv_shape()["group"]


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def device_sgs(csr, sweeps, kmax=8):
    sg = csr.sgs(sweeps=sweeps, kmax=kmax)
    assert (sg.lower.sweeps, sg.upper.sweeps) == (sweeps, sweeps)
    return Precond(*sg.args[:2], scale=sg.diag, own=[sg])


def device_ic0(csr, sweeps, kmax=8):
    L, _ = csr.ic0()
    LT = L.transpose()
    lo = L.trsv_analyse("lower", sweeps=sweeps, kmax=kmax)
    up = LT.trsv_analyse("upper", sweeps=sweeps, kmax=kmax)
    L.release()    # the plans own what they need
    LT.release()
    return Precond(lo, up, own=[lo, up])


def device_ilu0(csr, sweeps, kmax=8):
    LU, _ = csr.ilu0()
    lo = LU.trsv_analyse("lower", unit=True, sweeps=sweeps, kmax=kmax)
    up = LU.trsv_analyse("upper", sweeps=sweeps, kmax=kmax)
    LU.release()
    return Precond(lo, up, own=[lo, up])


def device_diagonal(d, sweeps):
    M = len(d)
    A = S.csr_from_arrays("diag", M, M, np.arange(M + 1), np.arange(M), d)
    h = S.CsrDevice.upload(A)
    S.csr_free(A)
    plan = h.trsv_analyse("lower", sweeps=sweeps)
    h.release()
    return Precond(plan, own=[plan])


# ------------------------------------------------------------------ 1. CG
@pytest.mark.parametrize("which,sweeps", [("ic0", 3), ("sgs", 2)])
def test_pcg_trsv_has_the_bits_of_the_restatement(which, sweeps):
    mat = G.lap2d(37, 29, 0.01)
    M, IRP, JA, AS = mat
    apply = SW.sweeps_apply(*getattr(PT, which)(mat), GROUP, sweeps)
    bench = CgBench(M)
    hs = upload(mat, "f64")
    live = S._lib.spmv_live_handles()
    pre = {"ic0": device_ic0, "sgs": device_sgs}[which](hs["csr"], sweeps)
    for fmt, m in hs.items():
        for k in (1, 3, 8):
            tag = (which, sweeps, fmt, k)
            B, X0 = G.common_inputs(M, k)
            product, residual0 = bench.callables(m, B, X0)
            want = PT.restate(product, residual0, B, X0, apply, TOL, 300)
            rec, Xf, _ = bench.solve(m, B, X0, pre, ldb=k + 2, ldx=k + 1,
                                     shift=8, tol=TOL, maxit=300)
            same_solve(rec, Xf[:M], want, tag)
            neighbours_kept(Xf, M, k, tag)
            assert [r.status for r in rec] == [0] * k, tag
            res = G.true_residual(IRP, JA, AS, O.csr_spmv, B, Xf[:M, :k])
            print(tag, "iterations", [r.iterations for r in rec],
                  "true residual", res)
            assert np.all(res <= 2 * TOL), (tag, res)
    pre.release()
    assert S._lib.spmv_live_handles() == live
    for m in hs.values():
        m.release()
    bench.free()


def test_a_diagonal_sweep_plan_is_cg_and_pcg():
    """no strict entries: every sweep is x = D^-1 b -- the identity gives the
    bits of cg(), powers of two those of pcg()"""
    mat = G.lap2d(37, 29, 0.01)
    M = mat[0]
    B, X0 = G.common_inputs(M)
    bench = CgBench(M)
    hs = upload(mat, "f64")
    d = 2.0 ** np.random.default_rng(3).integers(-6, 7, M)
    minv = S.DevBuffer.from_numpy(1.0 / d)
    ident = device_diagonal(np.ones(M), 3)
    pow2 = device_diagonal(d, 3)
    for fmt, m in hs.items():
        put(bench.B.ptr, B)
        put(bench.X.ptr, X0)
        rec = m.cg(bench.B.ptr, bench.X.ptr, 4, tol=TOL, maxit=200)
        plain = as_solve(rec, bench.X.to_numpy(np.float64,
                                               M * 4).reshape(M, 4))
        rec, Xf, _ = bench.solve(m, B, X0, ident, tol=TOL, maxit=200)
        same_solve(rec, Xf[:M], plain, (fmt, "identity"))
        put(bench.X.ptr, X0)
        rec = m.pcg(bench.B.ptr, bench.X.ptr, minv.ptr, 4, tol=TOL, maxit=200)
        diag = as_solve(rec, bench.X.to_numpy(np.float64,
                                              M * 4).reshape(M, 4))
        rec, Xf, _ = bench.solve(m, B, X0, pow2, tol=TOL, maxit=200)
        same_solve(rec, Xf[:M], diag, (fmt, "2^n"))
    for pre in (ident, pow2):
        pre.release()
    minv.free()
    for m in hs.values():
        m.release()
    bench.free()


# ------------------------------------------------- 2. BiCGStab and GMRES
def test_bicgstab_trsv_has_the_bits_of_the_restatement():
    mat = BI.convdiff(37, 29, 0.5, 0.5)
    M, IRP, JA, AS = mat
    apply = SW.sweeps_apply(*IL.ilu0(mat), GROUP, 3)
    bench = BiBench(M)
    hs = upload(mat, "f64")
    pre = device_ilu0(hs["csr"], 3)
    for fmt, m in hs.items():
        for k in (1, 3, 8):
            tag = ("bicgstab", fmt, k)
            B, X0 = G.common_inputs(M, k)
            product, residual0 = bench.callables(m, B, X0)
            want = IL.restate(product, residual0, B, X0, apply, TOL, 200)
            stride = dict(ldb=k + 2, ldx=k + 1, shift=8) if k == 3 else {}
            rec, Xf, _ = bench.solve(m, B, X0, pre, tol=TOL, maxit=200,
                                     **stride)
            same_solve(rec, Xf[:M], want, tag)
            neighbours_kept(Xf, M, k, tag)
            assert [r.status for r in rec] == [0] * k, tag
            res = G.true_residual(IRP, JA, AS, O.csr_spmv, B, Xf[:M, :k])
            print(tag, "iterations", [r.iterations for r in rec],
                  "true residual", res)
            assert np.all(res <= 2 * TOL), (tag, res)
    pre.release()
    for m in hs.values():
        m.release()
    bench.free()


def test_gmres_trsv_has_the_bits_of_the_restatement():
    mat = BI.convdiff(37, 29, 0.5, 0.5)
    M, IRP, JA, AS = mat
    z = SW.sweeps_apply(*IL.ilu0(mat), GROUP, 3)
    bench = GmBench(M)
    fill(bench.minv)
    hs = upload(mat, "f64")
    pre = device_ilu0(hs["csr"], 3)
    for fmt, m in hs.items():
        for k in (1, 3, 8):
            tag = ("gmres(5)", fmt, k)
            B, X0 = G.common_inputs(M, k)
            want = bench.want(m, B, X0, 5, z=z)
            stride = dict(ldb=k + 2, ldx=k + 1, shift=8) if k == 3 else {}
            rec, Xf = bench.solve(m, B, X0, 5, pre=pre, tol=TOL, maxit=200,
                                  **stride)
            same_gmres(rec, Xf[:M], want, tag)
            neighbours_kept(Xf, M, k, tag)
            assert [r.status for r in rec] == [0] * k, tag
            assert rec[0].restarts > 0, tag
            res = G.true_residual(IRP, JA, AS, O.csr_spmv, B, Xf[:M, :k])
            assert np.all(res <= 2 * TOL), (tag, res)
    pre.release()
    for m in hs.values():
        m.release()
    bench.free()


# ------------------------------------------------------------ 3. refusals
def test_the_solvers_refuse_a_plan_with_fewer_columns_than_k():
    mat = BI.convdiff(17, 13, 0.5, 0.5)
    M = mat[0]
    k = 4
    B, X0 = G.common_inputs(M, k)
    hs = upload(mat, "f64")
    d = hs["csr"]
    exact = d.trsv_analyse("lower")
    narrow = d.trsv_analyse("lower", sweeps=2, kmax=3)
    enough = d.trsv_analyse("upper", sweeps=2, kmax=4)
    others = upload(BI.convdiff(17, 12, 0.5, 0.5), "f64")
    small = others["csr"].trsv_analyse("lower", sweeps=2, kmax=8)  # another M
    d_B, d_X = S.DevBuffer.from_numpy(B), S.DevBuffer.from_numpy(X0)
    einval = -errno.EINVAL
    o = S._opts()
    for m in hs.values():
        for name, tail, info in (
                ("pcg_trsv", (TOL, 3, 0, None, 0), (S.CgInfo * 8)()),
                ("bicgstab_trsv", (TOL, 3, 0, None, 0), (S.CgInfo * 8)()),
                ("gmres_trsv", (5, TOL, 3, 0, None, 0),
                 (S.GmresInfo * 8)())):
            def rc(kk, first, second):
                return m._fn(name)(m.h, C.byref(o), kk, d_B.ptr, 0, d_X.ptr,
                                   0, first, second, None, *tail, info, None)
            assert rc(k, narrow.h, None) == einval, name
            assert rc(k, exact.h, narrow.h) == einval, name
            assert rc(k, enough.h, narrow.h) == einval, name
            assert rc(k, small.h, None) == einval, name
            S.stream_sync()
            got = d_X.to_numpy(np.float64, M * k).reshape(M, k)
            assert np.array_equal(bits(got), bits(X0)), "something was enqueued"
            assert rc(3, narrow.h, enough.h) == 0, name  # k == kmax
            assert rc(k, enough.h, exact.h) == 0, name
            S.stream_sync()
            put(d_X.ptr, X0)
    for h in (exact, narrow, enough, small, *others.values(), d_B, d_X):
        (h.free if isinstance(h, S.DevBuffer) else h.release)()
    for m in hs.values():
        m.release()
