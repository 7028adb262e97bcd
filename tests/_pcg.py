"""The preconditioned conjugate-gradient solver (spmv_*_pcg, spmv_engine.h)
restated in numpy, the scaled test matrix and the diagonal of CSR arrays.  No
GPU here.

As tests/_cg.py: numpy rounds every operation once and fuses nothing, so
`restate` with the product and the initial residual the device gives must
reproduce a device solve BIT FOR BIT.  z(R) = minv[:, None] * R is recomputed
wherever it is used, as on the device (a product of the same two doubles has
the same bits wherever it is formed).
"""
import numpy as np

import _cg as G

RUNNING = G.RUNNING


def restate(product, residual0, B, X0, minv, tol, maxit, shape=None):
    """the loop of spmv_engine.h (spmv_*_pcg).  product(P) -> Q = A P as
    (M, k); residual0() -> B - A X0 as (M, k); minv: (M,).  -> _cg.Solve"""
    M, k = B.shape
    d = np.asarray(minv, np.float64).reshape(M, 1)
    X = np.array(X0, np.float64)
    R = np.array(residual0(), np.float64)
    tol2 = np.float64(tol) * np.float64(tol)
    iters = np.zeros(k, np.int64)
    with np.errstate(all="ignore"):
        P = d * R
        bb = G.dot(B, B, shape)
        rr = G.dot(R, R, shape)
        rz = G.dot(R, d * R, shape)
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
            zn = G.dot(R, d * R, shape)
            conv = run & (rn <= tol2 * bb)
            status[conv] = 0
            rr[conv] = rn[conv]
            status[run & ~conv
                   & (~np.isfinite(rn) | ~((zn > 0) & np.isfinite(zn)))] = 2
            run = status == RUNNING
            beta = zn[run] / rz[run]
            P[:, run] = d * R[:, run] + beta * P[:, run]
            rr[run] = rn[run]
            rz[run] = zn[run]
    status[status == RUNNING] = 1
    return G.Solve(X, status.astype(np.int64), iters, rr, bb)


def scaled_lap2d(nx, ny, shift, span, seed):
    """_cg.lap2d(nx, ny, shift) with entry (r, c) multiplied by s_r * s_c,
    s = 2 ** uniform(0, span): SPD, symmetric, the diagonal spread over
    2 ** (2 span).  The entry is a * rn(s_r * s_c): a product commutes, so the
    matrix is symmetric to the bit"""
    M, IRP, JA, AS = G.lap2d(nx, ny, shift)
    s = 2.0 ** np.random.default_rng(seed).uniform(0, span, M)
    rows = np.repeat(np.arange(M), np.diff(IRP))
    return M, IRP, JA, np.ascontiguousarray(AS * (s[rows] * s[JA]))


def diag_of(M, IRP, JA, AS, N=None):
    """-> d[min(M, N)]: the sum, from 0.0 in stored order, of the entries of
    row r whose column is r (what spmv_*_diag stores when a row holds its
    diagonal at most once, or sums that are exact in any order)"""
    n = M if N is None else min(M, N)
    d = np.zeros(n)
    rows = np.repeat(np.arange(M), np.diff(IRP))
    for k in np.flatnonzero((rows == JA) & (rows < n)):
        d[rows[k]] = d[rows[k]] + AS[k]
    return d
