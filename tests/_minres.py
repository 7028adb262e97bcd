"""The MINRES solver (spmv_*_minres, spmv_engine.h) restated in numpy, and the
symmetric indefinite test matrices.  No GPU here.

As tests/_cg.py: numpy rounds every operation once and fuses nothing, and
np.sqrt is the correctly rounded square root, so `restate` with the products
and the residuals the device gives must reproduce a device solve BIT FOR BIT.
z(U) = minv[:, None] * U is formed wherever it is used (a product of the same
two doubles has the same bits wherever it is formed); without minv it is U
itself.
"""
import collections

import numpy as np

import _cg as G

RUNNING = G.RUNNING
Solve = collections.namedtuple("Solve", "X status iterations pp bn2 rr bb")


def restate(product, residual0, B, X0, minv, tol, maxit, shape=None,
            residual=None):
    """the loop of spmv_engine.h (spmv_*_minres).  product(V) -> A V as
    (M, k); residual0() -> B - A X0 as (M, k); minv: (M,) or None;
    residual(X) -> B - A X for the closing rr (None: -1.0 * product(X) +
    1.0 * B, what launch_axpby computes from launch_multi's sums).  -> Solve"""
    M, k = B.shape
    if minv is None:
        def z(U):
            return U
    else:
        d = np.asarray(minv, np.float64).reshape(M, 1)

        def z(U):
            return d * U
    X = np.array(X0, np.float64)
    R2 = np.array(residual0(), np.float64)
    R1 = np.zeros((M, k))
    W1 = np.zeros((M, k))
    W2 = np.zeros((M, k))
    tol2 = np.float64(tol) * np.float64(tol)
    iters = np.zeros(k, np.int64)
    oldb = np.zeros(k)
    dbar = np.zeros(k)
    epsln = np.zeros(k)
    cs = np.full(k, -1.0)
    sn = np.zeros(k)
    with np.errstate(all="ignore"):
        bb = G.dot(B, B, shape)
        bn2 = G.dot(B, z(B), shape)
        b1 = G.dot(R2, z(R2), shape)
        bad = ~((b1 >= 0) & np.isfinite(b1)) | ~((bn2 >= 0) & np.isfinite(bn2))
        status = np.where(bad, 2, np.where(b1 <= tol2 * bn2, 0, RUNNING))
        pp = b1.copy()
        beta = np.where(status == RUNNING, np.sqrt(b1), 0.0)
        phibar = beta.copy()
        for i in range(1, maxit + 1):
            run = status == RUNNING
            if not run.any():
                break
            s = 1.0 / beta
            V = s * z(R2)
            Q = np.array(product(V), np.float64)
            if i >= 2:
                Q = Q - (beta / oldb) * R1
            alfa = G.dot(V, Q, shape)
            status[run & ~np.isfinite(alfa)] = 2
            run = status == RUNNING
            Rn = Q - (alfa / beta) * R2
            bnew = G.dot(Rn, z(Rn), shape)
            R1, R2 = R2, Rn
            status[run & ~((bnew >= 0) & np.isfinite(bnew))] = 2
            run = status == RUNNING
            oldb_n = beta
            beta_n = np.sqrt(bnew)
            oldeps = epsln
            delta = cs * dbar + sn * alfa
            gbar = sn * dbar - cs * alfa
            epsln_n = sn * beta_n
            dbar_n = -(cs * beta_n)
            gamma = np.sqrt(gbar * gbar + beta_n * beta_n)
            status[run & ~((gamma > 0) & np.isfinite(gamma))] = 2
            run = status == RUNNING
            cs_n = gbar / gamma
            sn_n = beta_n / gamma
            phi = cs_n * phibar
            phibar_n = sn_n * phibar
            Wn = ((V - oldeps * W1) - delta * W2) / gamma
            W1, W2 = W2, Wn
            X[:, run] = X[:, run] + phi[run] * Wn[:, run]
            iters[run] += 1
            # the scalars of a frozen column stay what they were
            oldb = np.where(run, oldb_n, oldb)
            beta = np.where(run, beta_n, beta)
            epsln = np.where(run, epsln_n, epsln)
            dbar = np.where(run, dbar_n, dbar)
            cs = np.where(run, cs_n, cs)
            sn = np.where(run, sn_n, sn)
            phibar = np.where(run, phibar_n, phibar)
            pp = np.where(run, phibar * phibar, pp)
            conv = run & (pp <= tol2 * bn2)
            status[conv] = 0
            status[run & ~conv & ~np.isfinite(pp)] = 2
        status[status == RUNNING] = 1
        if residual is None:
            R = -1.0 * np.array(product(X), np.float64) + 1.0 * B
        else:
            R = np.array(residual(X), np.float64)
        rr = G.dot(R, R, shape)
    return Solve(X, status.astype(np.int64), iters, pp, bn2, rr, bb)


# ------------------------------------------------------------------ matrices
def shifted_lap1d(M, sigma):
    """tridiag(-1, 2 - sigma, -1) as CSR arrays (M, IRP, JA, AS): indefinite
    for 0 < sigma < 4 once M is large enough"""
    i = np.arange(M)
    rows = np.concatenate((i, i[:-1], i[1:]))
    cols = np.concatenate((i, i[1:], i[:-1]))
    vals = np.concatenate((np.full(M, 2.0 - sigma), np.full(2 * (M - 1), -1.0)))
    return G._csr(M, rows, cols, vals)


def shifted_lap2d(nx, ny, sigma):
    """5-point stencil on an nx x ny grid, diagonal 4 - sigma, off-diagonals
    -1 (the Helmholtz-like shift of _cg.lap2d)"""
    return G.lap2d(nx, ny, -float(sigma))


def saddle(n, m, seed):
    """[[K, C^T], [C, 0]], n + m rows: K = tridiag(-1, 2.5, -1) (SPD), C
    m x n with C[i][i] = 1 + uniform(0, 1) (full row rank, m <= n) and one
    more uniform(-1, 1) entry per row.  The last m rows store no diagonal"""
    assert m <= n
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    rows = [i, i[:-1], i[1:]]
    cols = [i, i[1:], i[:-1]]
    vals = [np.full(n, 2.5), np.full(n - 1, -1.0), np.full(n - 1, -1.0)]
    r = np.arange(m)
    c2 = (r + 1 + rng.integers(0, n - 1, m)) % n     # never the diagonal one
    cr = np.concatenate((r, r))
    cc = np.concatenate((r, c2))
    cv = np.concatenate((1.0 + rng.uniform(0, 1, m), rng.uniform(-1, 1, m)))
    rows += [n + cr, cc]
    cols += [cc, n + cr]
    vals += [cv, cv]
    return G._csr(n + m, np.concatenate(rows), np.concatenate(cols),
                  np.concatenate(vals))


def sym_arrow(M, seed):
    """_cg.arrow with the corner negated: row and column 0 dense, A[0][0] =
    -(sum |a_i| + 1), the other diagonal entries positive -- one negative
    eigenvalue, M - 1 positive.  Row 0 is a long row of the CSR kernels and
    makes hack block 0 M columns wide"""
    Mm, IRP, JA, AS = G.arrow(M, seed)
    AS = AS.copy()
    assert JA[0] == 0
    AS[0] = -AS[0]
    return Mm, IRP, JA, AS


def symscale(mat, seed):
    """entry (r, c) of `mat` times s_r * s_c, s = 2 ** uniform(0, 6):
    symmetric still, and what Jacobi undoes"""
    M, IRP, JA, AS = mat
    s = 2.0 ** np.random.default_rng(seed).uniform(0, 6, M)
    rows = np.repeat(np.arange(M), np.diff(IRP))
    return M, IRP, JA, np.ascontiguousarray(AS * s[rows] * s[JA])


def diagm(v):
    v = np.asarray(v, np.float64)
    i = np.arange(v.size)
    return G._csr(v.size, i, i, v)


def dense(mat):
    M, IRP, JA, AS = mat
    A = np.zeros((M, M))
    rows = np.repeat(np.arange(M), np.diff(IRP))
    np.add.at(A, (rows, JA), AS)
    return A


def abs_inverse_diag(mat):
    """1 / |d| of the stored diagonal, 1 where d == 0 (or is not stored): the
    preconditioner of a saddle-point caller"""
    M, IRP, JA, AS = mat
    rows = np.repeat(np.arange(M), np.diff(IRP))
    d = np.zeros(M)
    np.add.at(d, rows[rows == JA], AS[rows == JA])
    return np.where(d == 0, 1.0, 1.0 / np.where(d == 0, 1.0, np.abs(d)))
