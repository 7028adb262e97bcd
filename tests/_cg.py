"""The conjugate-gradient solver (spmv_*_cg, spmv_engine.h) restated in numpy,
and the symmetric test matrices.  No GPU here.

numpy rounds every operation once and fuses nothing, which is the solver's
contract, so `restate` with the product and the initial residual the device
gives (launch_multi, launch_axpby) must reproduce X, the iteration counts, the
statuses and rr / bb of a device solve BIT FOR BIT; with the CPU oracle's
product it is an ordinary CG, for the tests that need no GPU.
"""
import collections

import numpy as np

import spmv_scpa_amd as S

RUNNING = 3  # the status only the loop sees
Solve = collections.namedtuple("Solve", "X status iterations rr bb")


def dot(U, V, shape=None):
    """the solver's dot product per column of two (M, k) arrays -> (k,).

    With (NWG, T) = shape: element i belongs to slot i mod (NWG * T); a slot
    starts at 0.0 and adds rn(u_i * v_i) in increasing i; the T slots of a
    workgroup are combined by the halving tree s[t] += s[t + h], h = T/2 .. 1,
    and the NWG workgroup sums by the same tree.  The order depends on M and
    on nothing else."""
    nwg, T = shape or S.CG_DOT_SHAPE
    M, k = U.shape
    with np.errstate(all="ignore"):
        prod = U * V
        used = min(nwg, -(-M // T))        # workgroups that hold an element
        slots = np.zeros((used * T, k))
        for first in range(0, M, nwg * T):  # one sweep over the slots
            chunk = prod[first:first + nwg * T]
            slots[:len(chunk)] = slots[:len(chunk)] + chunk
        s = slots.reshape(used, T, k)
        h = T // 2
        while h:
            s[:, :h] = s[:, :h] + s[:, h:2 * h]
            h //= 2
        w = np.zeros((nwg, k))             # the other workgroups: 0.0
        w[:used] = s[:, 0]
        h = nwg // 2
        while h:
            w[:h] = w[:h] + w[h:2 * h]
            h //= 2
    return w[0].copy()


def restate(product, residual0, B, X0, tol, maxit, shape=None):
    """the loop of spmv_engine.h.  product(P) -> Q = A P as (M, k);
    residual0() -> B - A X0 as (M, k).  -> Solve"""
    M, k = B.shape
    X = np.array(X0, np.float64)
    R = np.array(residual0(), np.float64)
    P = R.copy()
    tol2 = np.float64(tol) * np.float64(tol)
    iters = np.zeros(k, np.int64)
    with np.errstate(all="ignore"):
        bb = dot(B, B, shape)
        rr = dot(R, R, shape)
        status = np.where(~(np.isfinite(rr) & np.isfinite(bb)), 2,
                          np.where(rr <= tol2 * bb, 0, RUNNING))
        for _ in range(maxit):
            run = status == RUNNING
            if not run.any():
                break
            Q = product(P)
            pq = dot(P, Q, shape)
            status[run & ~((pq > 0) & np.isfinite(pq))] = 2
            run = status == RUNNING
            alpha = rr[run] / pq[run]
            X[:, run] = X[:, run] + alpha * P[:, run]
            R[:, run] = R[:, run] - alpha * Q[:, run]
            iters[run] += 1
            rn = dot(R, R, shape)
            conv = run & (rn <= tol2 * bb)
            status[conv] = 0
            rr[conv] = rn[conv]
            status[run & ~conv & ~np.isfinite(rn)] = 2
            run = status == RUNNING
            beta = rn[run] / rr[run]
            P[:, run] = R[:, run] + beta * P[:, run]
            rr[run] = rn[run]
    status[status == RUNNING] = 1
    return Solve(X, status.astype(np.int64), iters, rr, bb)


# ------------------------------------------------------------------ matrices
def lap2d(nx, ny, shift):
    """5-point stencil on an nx x ny grid as CSR arrays (M, IRP, JA, AS):
    diagonal 4 + shift, off-diagonals -1; SPD for shift > 0"""
    M = nx * ny
    idx = np.arange(M).reshape(ny, nx)
    rows = [idx.ravel()]
    cols = [idx.ravel()]
    vals = [np.full(M, 4.0 + shift)]
    for a, b in ((idx[:, :-1], idx[:, 1:]), (idx[:-1, :], idx[1:, :])):
        for r, c in ((a, b), (b, a)):
            rows.append(r.ravel())
            cols.append(c.ravel())
            vals.append(np.full(r.size, -1.0))
    return _csr(M, np.concatenate(rows), np.concatenate(cols),
                np.concatenate(vals))


def arrow(M, seed):
    """row and column 0 dense with a_i = uniform(-1, 1), A[0][0] = sum |a_i|
    + 1, A[i][i] = |a_i| + 1 + uniform(0, 1): SPD by diagonal dominance.  Row
    0 is a long row of the CSR kernels and makes hack block 0 M columns wide"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.0, 1.0, M - 1)
    d = np.abs(a) + 1.0 + rng.uniform(0.0, 1.0, M - 1)
    i = np.arange(1, M)
    z = np.zeros(M - 1, np.int64)
    rows = np.concatenate(([0], z, i, i))
    cols = np.concatenate(([0], i, z, i))
    vals = np.concatenate(([np.abs(a).sum() + 1.0], a, a, d))
    return _csr(M, rows, cols, vals)


def _csr(M, rows, cols, vals):
    order = np.lexsort((cols, rows))
    IRP = np.zeros(M + 1, np.int32)
    IRP[1:] = np.cumsum(np.bincount(rows, minlength=M))
    return (M, IRP, np.ascontiguousarray(cols[order], np.int32),
            np.ascontiguousarray(vals[order], np.float64))


def common_inputs(M, k=4, seed=1):
    """B = uniform(-1, 1) with column 1 all zero and column 2 scaled by 1e-3;
    X0 zero except column 3 = uniform(-1, 1) (for k < 4: what exists)"""
    rng = np.random.default_rng(seed)
    B = rng.uniform(-1.0, 1.0, (M, k))
    X0 = np.zeros((M, k))
    if k > 1:
        B[:, 1] = 0.0
    if k > 2:
        B[:, 2] *= 1e-3
    if k > 3:
        X0[:, 3] = rng.uniform(-1.0, 1.0, M)
    return B, X0


def dense_product(IRP, JA, AS, spmv):
    """-> (product, residual0 maker) from a single-vector SpMV
    spmv(IRP, JA, AS, x): the CPU stand-ins for launch_multi / launch_axpby"""
    def product(P):
        return np.stack([spmv(IRP, JA, AS, np.ascontiguousarray(P[:, j]))
                         for j in range(P.shape[1])], axis=1)

    def residual0(B, X0):
        return lambda: -1.0 * product(X0) + 1.0 * B
    return product, residual0


def true_residual(IRP, JA, AS, spmv, B, X):
    """||B - A X|| / ||B|| per column on the host (0 / 0 = 0)"""
    product, _ = dense_product(IRP, JA, AS, spmv)
    with np.errstate(invalid="ignore"):
        r = np.linalg.norm(B - product(X), axis=0)
        b = np.linalg.norm(B, axis=0)
        return np.where(b > 0, r / np.where(b > 0, b, 1.0), r)
