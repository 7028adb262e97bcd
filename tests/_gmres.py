"""Restarted GMRES (spmv_*_gmres, spmv_*_gmres_trsv; spmv_engine.h) restated
in numpy.  No GPU here.

As tests/_cg.py: numpy rounds every operation once and fuses nothing, and its
division and square root are correctly rounded, so `restate` with the products
and the residuals the device gives must reproduce a device solve BIT FOR BIT.
The vector statements are whole-array numpy; the dense arithmetic of a column
(rotations, ladder, back substitution) is written out scalar by scalar on
np.float64, one rounding each, in the order of the contract.  The matrices are
those of tests/_bicgstab.py (convdiff, arrow2, rowscale), the inputs
_cg.common_inputs.
"""
import collections

import numpy as np

import _bicgstab as BI  # noqa: F401  (the matrices, for the users of this file)
import _cg as G

RUNNING = G.RUNNING
Solve = collections.namedtuple(
    "Solve", "X status iterations restarts rr est bb")
F = np.float64


def _finite(v):
    return bool(np.isfinite(v))


class _Column:
    """the rotated Hessenberg factor, the rotations and g of one column"""

    def __init__(self, m):
        self.r = np.zeros((m, m))
        self.cs = np.zeros(m)
        self.sn = np.zeros(m)
        self.g = np.zeros(m + 1)

    def step(self, p, a, c, nn):
        """position p with the sums a[0..p], c[0..p] of the two passes and
        nn = dot(W, W) -> None on a breakdown, else (est, h_{p+1})"""
        h = np.zeros(p + 2)
        ok = _finite(nn)
        for i in range(p + 1):
            h[i] = F(a[i]) + F(c[i])
            ok = ok and _finite(h[i])
        h[p + 1] = np.sqrt(F(nn))
        if not ok:
            return None
        for i in range(p):
            t = F(self.cs[i] * h[i]) + F(self.sn[i] * h[i + 1])
            h[i + 1] = F(self.cs[i] * h[i + 1]) - F(self.sn[i] * h[i])
            h[i] = t
        a_, b_ = F(h[p]), F(h[p + 1])
        d = np.sqrt(F(a_ * a_) + F(b_ * b_))
        if not _finite(d) or d == 0.0:
            return None
        c_ = a_ / d
        s_ = b_ / d
        self.r[:p, p] = h[:p]
        self.r[p, p] = F(c_ * a_) + F(s_ * b_)
        self.cs[p] = c_
        self.sn[p] = s_
        gp = F(self.g[p])
        self.g[p + 1] = -F(s_ * gp)
        self.g[p] = F(c_ * gp)
        est = F(self.g[p + 1]) * F(self.g[p + 1])
        return est, b_

    def back(self, q):
        y = np.zeros(q)
        for i in range(q - 1, -1, -1):
            s = F(0.0)
            for l in range(i + 1, q):
                s = s + F(self.r[i, l] * y[l])
            y[i] = F(self.g[i] - s) / F(self.r[i, i])
        return y


def restate(product, residual0, B, X0, restart, tol, maxit, z=None,
            shape=None, trace=None):
    """the loop of spmv_engine.h (spmv_*_gmres).  product(Z) -> A Z as (M, k);
    residual0(X) -> B - A X as (M, k), asked for at the start, at every
    restart and for the true rr at the end; z(U) -> the preconditioned (M, k)
    array, None: U itself (a diagonal: lambda U: minv[:, None] * U; plans:
    _pcg_trsv.plans_apply); trace: a list that receives (step, position, est
    copy) after every step.  -> Solve"""
    M, k = B.shape
    m = int(restart)
    if z is None:
        def z(U):
            return U.copy()
    X = np.array(X0, np.float64)
    tol2 = F(tol) * F(tol)
    status = np.full(k, RUNNING, np.int64)
    iters = np.zeros(k, np.int64)
    restarts = np.zeros(k, np.int64)
    q = np.zeros(k, np.int64)
    rr = np.zeros(k)
    est = np.zeros(k)
    scale = np.zeros(k)
    cols = [_Column(m) for _ in range(k)]
    V = [np.zeros((M, k)) for _ in range(m + 1)]

    def begin(first):
        look = np.ones(k, bool) if first else status == RUNNING
        V[0] = np.array(residual0(X), np.float64)
        r0 = G.dot(V[0], V[0], shape)
        for j in np.flatnonzero(look):
            if not first:
                restarts[j] += 1
            rr[j] = est[j] = r0[j]
            if not (_finite(r0[j]) and _finite(bb[j])):
                status[j] = 2
            elif r0[j] <= tol2 * bb[j]:
                status[j] = 0
            else:
                status[j] = RUNNING
                beta = np.sqrt(F(r0[j]))
                cols[j].g[0] = beta
                V[0][:, j] = V[0][:, j] / beta

    def update():
        U = np.zeros((M, k))
        todo = np.flatnonzero(q > 0)
        if not todo.size:
            return
        for j in todo:
            y = cols[j].back(int(q[j]))
            u = y[0] * V[0][:, j]
            for i in range(1, int(q[j])):
                u = u + y[i] * V[i][:, j]
            U[:, j] = u
        ZU = np.asarray(z(U), np.float64)
        X[:, todo] = X[:, todo] + ZU[:, todo]
        q[todo] = 0

    with np.errstate(all="ignore"):
        bb = G.dot(B, B, shape)
        begin(True)
        for step in range(1, maxit + 1):
            if not (status == RUNNING).any():
                break
            p = (step - 1) % m
            run = status == RUNNING
            W = np.array(product(z(V[p])), np.float64)
            sums = []
            for _ in range(2):
                s = [G.dot(V[i], W, shape) for i in range(p + 1)]
                for i in range(p + 1):
                    W[:, run] = W[:, run] - s[i][run] * V[i][:, run]
                sums.append(s)
            nn = G.dot(W, W, shape)
            for j in np.flatnonzero(run):
                got = cols[j].step(p, [s[j] for s in sums[0]],
                                   [s[j] for s in sums[1]], nn[j])
                if got is None:
                    status[j] = 2
                    continue
                iters[j] += 1
                q[j] += 1
                est[j] = got[0]
                if est[j] <= tol2 * bb[j]:
                    status[j] = 0
                else:
                    scale[j] = got[1]
            if trace is not None:
                trace.append((step, p, est.copy()))
            if p + 1 < m:
                run = status == RUNNING
                V[p + 1] = W.copy()
                V[p + 1][:, run] = W[:, run] / scale[run]
            else:
                update()
                begin(False)
        update()
        R = np.array(residual0(X), np.float64)
        rr = G.dot(R, R, shape)
    status[status == RUNNING] = 1
    return Solve(X, status, iters, restarts, rr, est, bb)


def oracle_callables(mat, spmv, B):
    """(product, residual0) of the CPU stand-ins: _cg.dense_product with the
    residual as a function of X"""
    M, IRP, JA, AS = mat
    product, _ = G.dense_product(IRP, JA, AS, spmv)
    return product, lambda X: -1.0 * product(X) + 1.0 * B
