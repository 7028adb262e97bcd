"""Conjugate gradients preconditioned by triangular plans (spmv_*_pcg_trsv,
spmv_engine.h) restated in numpy.  No GPU here.

restate         tests/_pcg.py restate with the STORED Z = apply(R) where that
                has minv * R
plans_apply     apply(R) of two reference plans (tests/_trsv.py): the first
                solve, then the second in place with its row scale
level_solve     tests/_trsv.py reference_solve with the rows of a level taken
                together (they never meet): the same operations on the same
                operands, so the same bits, in a fraction of the time
sgs / ic0       the two preconditioners as (first, second, scale)
"""
import numpy as np

import _cg as G
import _ic0 as IC
import _trsv as TV

RUNNING = G.RUNNING


def restate(product, residual0, B, X0, apply, tol, maxit, shape=None):
    """the loop of spmv_engine.h (spmv_*_pcg_trsv).  product(P) -> Q = A P as
    (M, k); residual0() -> B - A X0 as (M, k); apply(R) -> Z as (M, k), all
    columns.  -> _cg.Solve"""
    M, k = B.shape
    X = np.array(X0, np.float64)
    R = np.array(residual0(), np.float64)
    tol2 = np.float64(tol) * np.float64(tol)
    iters = np.zeros(k, np.int64)
    with np.errstate(all="ignore"):
        Z = apply(R)
        P = Z.copy()
        bb = G.dot(B, B, shape)
        rr = G.dot(R, R, shape)
        rz = G.dot(R, Z, shape)
        finite = np.isfinite(rr) & np.isfinite(bb) & np.isfinite(rz)
        status = np.where(~finite, 2,
                          np.where(rr <= tol2 * bb, 0,
                                   np.where(~(rz > 0), 2, RUNNING)))
        for _ in range(maxit):
            run = status == RUNNING
            if not run.any():
                break
            Q = product(P)
            pq = G.dot(P, Q, shape)
            status[run & ~((pq > 0) & np.isfinite(pq))] = 2
            run = status == RUNNING
            alpha = rz[run] / pq[run]
            X[:, run] = X[:, run] + alpha * P[:, run]
            R[:, run] = R[:, run] - alpha * Q[:, run]
            iters[run] += 1
            rn = G.dot(R, R, shape)
            Z = apply(R)
            zn = G.dot(R, Z, shape)
            conv = run & (rn <= tol2 * bb)
            status[conv] = 0
            rr[conv] = rn[conv]
            status[run & ~conv
                   & (~np.isfinite(rn) | ~((zn > 0) & np.isfinite(zn)))] = 2
            run = status == RUNNING
            beta = zn[run] / rz[run]
            P[:, run] = Z[:, run] + beta * P[:, run]
            rr[run] = rn[run]
            rz[run] = zn[run]
    status[status == RUNNING] = 1
    return G.Solve(X, status.astype(np.int64), iters, rr, bb)


def level_solve(plan, B, scale, group, unit=False):
    """TV.reference_solve, one level at a time"""
    order, rowptr, ja, vals = (plan[n] for n in ("order", "rowptr", "ja", "as"))
    diag, level_ptr = plan["diag"], plan["level_ptr"]
    B = np.asarray(B, np.float64)
    M, k = B.shape
    X = np.zeros((M, k))
    with np.errstate(all="ignore"):
        for l in range(len(level_ptr) - 1):
            ps = np.arange(level_ptr[l], level_ptr[l + 1])
            rows = order[ps]
            beg = rowptr[ps].astype(np.int64)
            n = rowptr[ps + 1] - rowptr[ps]
            slot = np.zeros((len(ps), group, k))
            for q in range(int(n.max()) if len(n) else 0):
                act = np.flatnonzero(n > q)
                e = beg[act] + q
                g = q % group
                slot[act, g] = slot[act, g] + vals[e][:, None] * X[ja[e]]
            h = group // 2
            while h >= 1:
                slot[:, :h] = slot[:, :h] + slot[:, h:2 * h]
                h //= 2
            rhs = B[rows] if scale is None else scale[rows][:, None] * B[rows]
            t = rhs - slot[:, 0]
            X[rows] = t if unit else t / diag[rows][:, None]
    return X


def plans_apply(first, second, scale, group, solve=level_solve):
    """apply(R) of spmv_*_pcg_trsv: first and second are (plan, unit) with a
    plan of TV.reference_plan; second may be None"""
    def apply(R):
        Z = solve(first[0], R, None, group, first[1])
        if second is not None:
            Z = solve(second[0], Z, scale, group, second[1])
        return Z
    return apply


def int32(mat):
    M, IRP, JA, AS = mat
    return M, IRP.astype(np.int32), JA.astype(np.int32), AS


def sgs(mat):
    """-> (first, second, scale): the lower and upper plan of A and diag(A)"""
    M, IRP, JA, AS = int32(mat)
    lo = TV.reference_plan(IRP, JA, AS, "lower")
    up = TV.reference_plan(IRP, JA, AS, "upper")
    return (lo, False), (up, False), lo["diag"].copy()


def transposed(M, IRP, JA, AS):
    """A^T with each row's entries in the order of A's rows (the stable order
    by column of spmv_csr_transpose)"""
    rows = np.repeat(np.arange(M), np.diff(IRP))
    order = np.argsort(JA, kind="stable")
    TIRP = np.zeros(M + 1, np.int32)
    TIRP[1:] = np.cumsum(np.bincount(JA, minlength=M))
    return (M, TIRP, np.ascontiguousarray(rows[order], np.int32),
            np.ascontiguousarray(AS[order]))


def ic0(mat, shift=0.0):
    """-> (first, second, None): the lower plan of L = reference_ic0(A) and
    the upper plan of L^T"""
    M = mat[0]
    F = IC.reference_ic0(*mat, shift=shift)
    lo = TV.reference_plan(F.IRP, F.JA, F.AS, "lower")
    up = TV.reference_plan(*transposed(M, F.IRP, F.JA, F.AS)[1:], "upper")
    return (lo, False), (up, False), None
