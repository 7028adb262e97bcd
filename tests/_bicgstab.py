"""The BiCGStab solver (spmv_*_bicgstab, spmv_engine.h) restated in numpy, and
the nonsymmetric test matrices.  No GPU here.

As tests/_cg.py: numpy rounds every operation once and fuses nothing, so
`restate` with the products and the initial residual the device gives must
reproduce a device solve BIT FOR BIT.  z(U) = minv[:, None] * U is formed
wherever it is used (a product of the same two doubles has the same bits
wherever it is formed); without minv it is U itself.
"""
import numpy as np

import _cg as G

RUNNING = G.RUNNING


def restate(product, residual0, B, X0, minv, tol, maxit, shape=None):
    """the loop of spmv_engine.h (spmv_*_bicgstab).  product(Z) -> A Z as
    (M, k); residual0() -> B - A X0 as (M, k); minv: (M,) or None.
    -> _cg.Solve"""
    M, k = B.shape
    if minv is None:
        def z(U):
            return U.copy()
    else:
        d = np.asarray(minv, np.float64).reshape(M, 1)

        def z(U):
            return d * U
    X = np.array(X0, np.float64)
    R = np.array(residual0(), np.float64)
    Rh = R.copy()
    P = R.copy()
    tol2 = np.float64(tol) * np.float64(tol)
    iters = np.zeros(k, np.int64)
    alpha = np.zeros(k)
    omega = np.zeros(k)
    with np.errstate(all="ignore"):
        bb = G.dot(B, B, shape)
        rr = G.dot(R, R, shape)
        rho = rr.copy()
        status = np.where(~(np.isfinite(rr) & np.isfinite(bb)), 2,
                          np.where(rr <= tol2 * bb, 0, RUNNING))
        for _ in range(maxit):
            run = status == RUNNING
            if not run.any():
                break
            Z = z(P)
            V = np.asarray(product(Z), np.float64)
            rv = G.dot(Rh, V, shape)
            status[run & ~((rv != 0) & np.isfinite(rv))] = 2
            run = status == RUNNING
            alpha[run] = rho[run] / rv[run]
            S = R.copy()
            S[:, run] = R[:, run] - alpha[run] * V[:, run]
            Zs = z(S)
            T = np.asarray(product(Zs), np.float64)
            ts = G.dot(T, S, shape)
            tt = G.dot(T, T, shape)
            status[run & ~(np.isfinite(ts) & np.isfinite(tt))] = 2
            run = status == RUNNING
            omega[run] = np.where(tt[run] > 0, ts[run] / tt[run], 0.0)
            X[:, run] = ((X[:, run] + alpha[run] * Z[:, run])
                         + omega[run] * Zs[:, run])
            R[:, run] = S[:, run] - omega[run] * T[:, run]
            iters[run] += 1
            rn = G.dot(R, R, shape)
            rhon = G.dot(Rh, R, shape)
            conv = run & (rn <= tol2 * bb)
            status[conv] = 0
            rr[conv] = rn[conv]
            status[run & ~conv & ~np.isfinite(rn)] = 2
            run = status == RUNNING
            beta = (rhon[run] / rho[run]) * (alpha[run] / omega[run])
            P[:, run] = R[:, run] + beta * (P[:, run] - omega[run] * V[:, run])
            rho[run] = rhon[run]
            rr[run] = rn[run]
    status[status == RUNNING] = 1
    return G.Solve(X, status.astype(np.int64), iters, rr, bb)


# ------------------------------------------------------------------ matrices
def convdiff(nx, ny, shift, c):
    """5-point convection-diffusion stencil on an nx x ny grid as CSR arrays
    (M, IRP, JA, AS): diagonal 4 + shift, east -1 + c, west -1 - c, north and
    south -1; nonsymmetric for c != 0"""
    M = nx * ny
    idx = np.arange(M).reshape(ny, nx)
    w, e = idx[:, :-1].ravel(), idx[:, 1:].ravel()
    s, n = idx[:-1, :].ravel(), idx[1:, :].ravel()
    rows = np.concatenate((idx.ravel(), w, e, s, n))
    cols = np.concatenate((idx.ravel(), e, w, n, s))
    vals = np.concatenate((np.full(M, 4.0 + shift),
                           np.full(w.size, -1.0 + c),    # east of row w
                           np.full(e.size, -1.0 - c),    # west of row e
                           np.full(s.size + n.size, -1.0)))
    return G._csr(M, rows, cols, vals)


def arrow2(M, seed):
    """row 0 dense with a_i, column 0 dense with b_i, both uniform(-1, 1),
    A[i][i] = |a_i| + |b_i| + 1 + uniform(0, 1), A[0][0] = sum |a| + sum |b|
    + 1: nonsymmetric, diagonally dominant.  Row 0 is a long row of the CSR
    kernels and makes hack block 0 M columns wide"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.0, 1.0, M - 1)
    b = rng.uniform(-1.0, 1.0, M - 1)
    d = np.abs(a) + np.abs(b) + 1.0 + rng.uniform(0.0, 1.0, M - 1)
    i = np.arange(1, M)
    z = np.zeros(M - 1, np.int64)
    rows = np.concatenate(([0], z, i, i))
    cols = np.concatenate(([0], i, z, i))
    vals = np.concatenate(([np.abs(a).sum() + np.abs(b).sum() + 1.0], a, b, d))
    return G._csr(M, rows, cols, vals)


def rowscale(mat, seed):
    """row i of `mat` times 2 ** uniform(0, 6): what Jacobi undoes"""
    M, IRP, JA, AS = mat
    s = 2.0 ** np.random.default_rng(seed).uniform(0, 6, M)
    rows = np.repeat(np.arange(M), np.diff(IRP))
    return M, IRP, JA, np.ascontiguousarray(AS * s[rows])


def skew2(M):
    """M even: A[i][i ^ 1] = +1 for even i, -1 for odd i -- skew-symmetric,
    no diagonal"""
    assert M % 2 == 0
    i = np.arange(M)
    return G._csr(M, i, i ^ 1, np.where(i % 2 == 0, 1.0, -1.0))


def diagm(v):
    v = np.asarray(v, np.float64)
    i = np.arange(v.size)
    return G._csr(v.size, i, i, v)
