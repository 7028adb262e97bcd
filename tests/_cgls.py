"""The CGLS solver (spmv_*_cgls, spmv_engine.h) restated in numpy, and the
rectangular test matrices.  No GPU here.

As tests/_cg.py: numpy rounds every operation once and fuses nothing, so
`restate` with the products and the initial residual the device gives (A's
launch_multi and launch_axpby, AT's launch_multi) must reproduce a device solve
BIT FOR BIT; with the CPU oracle's product it is an ordinary CGLS, for the tests
that need no GPU.  The vectors have two lengths: B, R, Q have M rows, X, P, S
have N rows, and a dot takes its order from the length of its operands.

A matrix here is (M, N, IRP, JA, AS).
"""
import collections

import numpy as np

import _bicgstab as BI
import _cg as G

RUNNING = G.RUNNING
Solve = collections.namedtuple("Solve", "X status iterations ss atb rr")


def restate(product, product_t, residual0, B, X0, damp, tol, maxit,
            shape=None, d2_path=True):
    """the loop of spmv_engine.h (spmv_*_cgls).  product(P) -> A P as (M, k);
    product_t(R) -> AT R as (N, k); residual0() -> B - A X0 as (M, k).
    d2_path=False: the loop written without any d2 term (what damp == 0 must
    be), whatever `damp` says.  -> Solve"""
    M, k = B.shape
    X = np.array(X0, np.float64)
    tol2 = np.float64(tol) * np.float64(tol)
    d2 = np.float64(damp) * np.float64(damp)
    damped = d2_path and damp != 0
    iters = np.zeros(k, np.int64)
    with np.errstate(all="ignore"):
        R = np.array(residual0(), np.float64)
        W = np.asarray(product_t(B), np.float64)
        atb = G.dot(W, W, shape)
        S = np.array(product_t(R), np.float64)
        if damped:
            S = S - d2 * X
        P = S.copy()
        ss = G.dot(S, S, shape)
        status = np.where(~(np.isfinite(ss) & np.isfinite(atb)), 2,
                          np.where(ss <= tol2 * atb, 0, RUNNING))
        for _ in range(maxit):
            run = status == RUNNING
            if not run.any():
                break
            Q = np.asarray(product(P), np.float64)
            delta = G.dot(Q, Q, shape)
            if damped:
                delta = delta + d2 * G.dot(P, P, shape)
            status[run & ~((delta > 0) & np.isfinite(delta))] = 2
            run = status == RUNNING
            alpha = ss[run] / delta[run]
            X[:, run] = X[:, run] + alpha * P[:, run]
            R[:, run] = R[:, run] - alpha * Q[:, run]
            iters[run] += 1
            S = np.array(product_t(R), np.float64)
            if damped:
                S = S - d2 * X
            sn = G.dot(S, S, shape)
            conv = run & (sn <= tol2 * atb)
            status[conv] = 0
            ss[conv] = sn[conv]
            status[run & ~conv & ~np.isfinite(sn)] = 2
            run = status == RUNNING
            beta = sn[run] / ss[run]
            P[:, run] = S[:, run] + beta * P[:, run]
            ss[run] = sn[run]
        rr = G.dot(R, R, shape)
    status[status == RUNNING] = 1
    return Solve(X, status.astype(np.int64), iters, ss, atb, rr)


# ------------------------------------------------------------------ matrices
def _rect(M, N, rows, cols, vals):
    _, IRP, JA, AS = G._csr(M, np.asarray(rows, np.int64),
                            np.asarray(cols, np.int64),
                            np.asarray(vals, np.float64))
    return M, N, IRP, JA, AS


def coo(mat):
    """-> (rows, cols, vals) of a matrix"""
    M, N, IRP, JA, AS = mat
    return np.repeat(np.arange(M), np.diff(IRP)), JA.astype(np.int64), AS


def transpose(mat):
    """the N x M transpose on the host, entries sorted by (row, column)"""
    M, N, IRP, JA, AS = mat
    rows, cols, vals = coo(mat)
    return _rect(N, M, cols, rows, vals)


def dense(mat):
    M, N, IRP, JA, AS = mat
    D = np.zeros((M, N))
    rows, cols, vals = coo(mat)
    np.add.at(D, (rows, cols), vals)
    return D


def square(mat4):
    """a square (M, IRP, JA, AS) of tests/_cg.py as (M, M, IRP, JA, AS)"""
    M, IRP, JA, AS = mat4
    return M, M, IRP, JA, AS


def stacked(nx, ny, shift, c, lam):
    """[convdiff(nx, ny, shift, c); lam * I]: 2 n x n with n = nx ny, full
    column rank"""
    n, IRP, JA, AS = BI.convdiff(nx, ny, shift, c)
    rows, cols, vals = coo((n, n, IRP, JA, AS))
    i = np.arange(n)
    return _rect(2 * n, n, np.concatenate((rows, n + i)),
                 np.concatenate((cols, i)),
                 np.concatenate((vals, np.full(n, float(lam)))))


def without_column(mat, c):
    """`mat` with the entries of column c removed: rank deficient"""
    M, N, IRP, JA, AS = mat
    rows, cols, vals = coo(mat)
    keep = cols != c
    return _rect(M, N, rows[keep], cols[keep], vals[keep])


def diff1d(n):
    """first differences, (n + 1) x n: row i holds +1 in column i (i < n) and
    -1 in column i - 1 (i > 0)"""
    i = np.arange(n)
    return _rect(n + 1, n, np.concatenate((i, i + 1)), np.concatenate((i, i)),
                 np.concatenate((np.ones(n), -np.ones(n))))


def wide(M, N, per, seed):
    """[D | random], M x N with N > M: D = diag(uniform(1, 2)), and every
    column c >= M holds `per` entries uniform(-1, 1) in distinct random rows"""
    rng = np.random.default_rng(seed)
    d = rng.uniform(1.0, 2.0, M)
    nc = N - M
    # `per` distinct rows per column: a random start and a random odd stride
    # below M would repeat for small M; draw and re-draw the duplicates
    r = rng.integers(0, M, (nc, per))
    for _ in range(64):
        r.sort(axis=1)
        dup = np.zeros(r.shape, bool)
        dup[:, 1:] = r[:, 1:] == r[:, :-1]
        if not dup.any():
            break
        r[dup] = rng.integers(0, M, int(dup.sum()))
    assert not dup.any()
    v = rng.uniform(-1.0, 1.0, (nc, per))
    c = np.repeat(np.arange(M, N), per)
    i = np.arange(M)
    return _rect(M, N, np.concatenate((i, r.ravel())),
                 np.concatenate((i, c)), np.concatenate((d, v.ravel())))


def arrow_rect(M, N, seed):
    """M x N, M > N: row 0 dense with a_j, column 0 dense with b_i, both
    uniform(-1, 1), A[j][j] = 1 + uniform(0, 1) for 0 < j < N and
    A[0][0] = 2.  Row 0 is a long row of the CSR kernels; in the transpose
    row 0 has M entries"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.0, 1.0, N - 1)
    b = rng.uniform(-1.0, 1.0, M - 1)
    d = 1.0 + rng.uniform(0.0, 1.0, N - 1)
    j = np.arange(1, N)
    i = np.arange(1, M)
    rows = np.concatenate(([0], np.zeros(N - 1, np.int64), i, j))
    cols = np.concatenate(([0], j, np.zeros(M - 1, np.int64), j))
    return _rect(M, N, rows, cols, np.concatenate(([2.0], a, b, d)))


def diagm(v):
    return square(BI.diagm(v))


def inputs(mat, k=4, seed=1):
    """B (M rows) and X0 (N rows) with the columns of _cg.common_inputs:
    column 1 of B zero, column 2 scaled by 1e-3, column 3 of X0 random"""
    M, N = mat[0], mat[1]
    B, _ = G.common_inputs(M, k, seed)
    _, X0 = G.common_inputs(N, k, seed)
    return B, X0


def cpu_products(mat, spmv):
    """-> (product, product_t, residual0 maker) from a single-vector SpMV:
    the CPU stand-ins for the launches"""
    _, _, IRP, JA, AS = mat
    _, _, IRPt, JAt, ASt = transpose(mat)
    product, residual0 = G.dense_product(IRP, JA, AS, spmv)
    product_t, _ = G.dense_product(IRPt, JAt, ASt, spmv)
    return product, product_t, residual0


def normal_residual(mat, spmv, B, X, damp):
    """||A^T (b - A x) - damp^2 x|| / ||A^T b|| per column on the host
    (0 / 0 = 0)"""
    product, product_t, _ = cpu_products(mat, spmv)
    with np.errstate(invalid="ignore"):
        s = product_t(B - product(X)) - (damp * damp) * X
        r = np.linalg.norm(s, axis=0)
        b = np.linalg.norm(product_t(B), axis=0)
        return np.where(b > 0, r / np.where(b > 0, b, 1.0), r)
