"""Zero-fill incomplete LU (spmv_csr_ilu0; spmv_engine.h) restated in numpy,
straight from the definition in the header, the BiCGStab that takes its z(.)
from triangular plans (spmv_*_bicgstab_trsv), and the matrices their tests
run.  No GPU here.

reference_ilu0  plain Python loops over float64 scalars: numpy rounds every
                operation once, as the device does
dense_lu        LU without pivoting on a dense array, the same roundings: where
                the pattern has no fill it must give the bits of reference_ilu0
                (every extra operation of the dense loop acts on an exact zero)
pattern_ratio   on the pattern, L U is A: the residual over its derived bound
restate         tests/_bicgstab.py restate with Z = apply(U) where that has
                minv * U
ilu0            the preconditioner as (first, second, scale) for
                tests/_pcg_trsv.py plans_apply

A matrix is (M, IRP, JA, AS) with int32 index arrays and float64 values, every
row strictly ascending by column, every diagonal stored.
"""
import collections

import numpy as np

import _bicgstab as BI
import _cg as G
import _ic0 as IC
import _trsv as TV

RUNNING = G.RUNNING
Factor = collections.namedtuple("Factor", "IRP JA AS bad_pivots bad_rows")


def diag_positions(M, IRP, JA):
    rows = np.repeat(np.arange(M), np.diff(IRP))
    at = np.flatnonzero(JA == rows)
    assert len(at) == M and np.array_equal(rows[at], np.arange(M)), \
        "a row stores no diagonal, or stores it twice"
    return at


def reference_ilu0(M, IRP, JA, AS, shift=0.0):
    """-> Factor: L (strictly below the diagonal, its unit diagonal implied)
    and U (on and above it) in A's pattern, the number of rows whose final u_ii
    is 0 or not finite, and those rows"""
    W = np.array(AS, np.float64)
    shift = np.float64(shift)
    dpos = diag_positions(M, IRP, JA) if M else np.zeros(0, np.int64)
    bad = []
    with np.errstate(all="ignore"):
        for i in range(M):
            b, e, d = IRP[i], IRP[i + 1], dpos[i]
            assert np.all(np.diff(JA[b:e]) > 0), "row %d not ascending" % i
            W[d] = W[d] + shift * W[d]
            for t in range(b, d):
                j = JA[t]
                dj, ej = dpos[j], IRP[j + 1]
                l = W[t] / W[dj]
                W[t] = l
                # the columns above j stored in both rows: each w_m once
                _, ia, ib = np.intersect1d(JA[t + 1:e], JA[dj + 1:ej],
                                           assume_unique=True,
                                           return_indices=True)
                for x, y in zip(ia, ib):
                    W[t + 1 + x] = W[t + 1 + x] - l * W[dj + 1 + y]
            if not (W[d] != 0 and np.isfinite(W[d])):
                bad.append(i)
    return Factor(np.asarray(IRP), np.asarray(JA), W, len(bad),
                  np.array(bad, np.int64))


def dense_of(M, IRP, JA, AS):
    D = np.zeros((M, M))
    D[np.repeat(np.arange(M), np.diff(IRP)), JA] = AS
    return D


def dense_lu(D):
    """L (strict, unit diagonal implied) and U of D in one array: row by row,
    l = rn(w_k / u_kk), w_m = rn(w_m - rn(l * u_km)) for EVERY m > k.  A zero
    w_k is skipped: its l is an exact zero and its updates change nothing"""
    W = np.array(D, np.float64)
    M = len(W)
    with np.errstate(all="ignore"):
        for i in range(M):
            for k in np.flatnonzero(W[i, :i]):
                l = W[i, k] / W[k, k]
                W[i, k] = l
                W[i, k + 1:] = W[i, k + 1:] - l * W[k, k + 1:]
    return W


def nonfinite_rows(F):
    """mask of the rows of a Factor that hold an inf or a NaN"""
    M = len(F.IRP) - 1
    rows = np.repeat(np.arange(M), np.diff(F.IRP))
    return np.bincount(rows[~np.isfinite(F.AS)], minlength=M) > 0


def pattern_ratio(mat, F, shift=0.0):
    """the largest |sum_m l_im u_mj - a_ij| / ((n + 3) u sum_m |l_im u_mj|)
    over the stored entries (i, j), in the sense of _ic0.pattern_ratio: the sum
    runs over m <= min(i, j) with l_ii = 1, n = the products below min(i, j)
    whose two factors are both stored, u = 2^-53, the sums in extended
    precision.  For the diagonal the shifted a_ii is used.  n products and
    subtractions, one division (or the two operations of the shift)"""
    E = np.longdouble
    M, IRP, JA, AS = mat
    dpos = diag_positions(M, IRP, JA)
    at = [dict(zip(JA[IRP[i]:IRP[i + 1]].tolist(),
                   range(IRP[i], IRP[i + 1]))) for i in range(M)]
    worst = 0.0
    for i in range(M):
        for e in range(IRP[i], IRP[i + 1]):
            j = int(JA[e])
            prods = []
            for t in range(IRP[i], dpos[i]):
                m = int(JA[t])
                if m >= j:
                    break
                p = at[m].get(j)
                if p is not None:
                    prods.append(E(F.AS[t]) * E(F.AS[p]))
            n = len(prods)
            if j < i:
                prods.append(E(F.AS[e]) * E(F.AS[dpos[j]]))
            else:
                prods.append(E(F.AS[e]))
            prods = np.array(prods, E)
            a = E(AS[e])
            if j == i:
                a = a + E(shift) * a
            bound = (n + 3) * E(2.0) ** -53 * np.abs(prods).sum()
            worst = max(worst, float(abs(prods.sum() - a) / bound))
    return worst


# ------------------------------------------------------------- the solver
def restate(product, residual0, B, X0, apply, tol, maxit, shape=None):
    """the loop of spmv_engine.h (spmv_*_bicgstab_trsv): _bicgstab.restate
    with the STORED Zp = apply(P) and Zs = apply(S), all columns.
    -> _cg.Solve"""
    M, k = B.shape
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
            Z = np.asarray(apply(P), np.float64)
            V = np.asarray(product(Z), np.float64)
            rv = G.dot(Rh, V, shape)
            status[run & ~((rv != 0) & np.isfinite(rv))] = 2
            run = status == RUNNING
            alpha[run] = rho[run] / rv[run]
            S = R.copy()
            S[:, run] = R[:, run] - alpha[run] * V[:, run]
            Zs = np.asarray(apply(S), np.float64)
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


def ilu0(mat, shift=0.0):
    """-> (first, second, None): the unit lower plan and the upper plan of
    LU = reference_ilu0(A), both from the one array"""
    F = reference_ilu0(*mat, shift=shift)
    IRP, JA = F.IRP.astype(np.int32), F.JA.astype(np.int32)
    lo = TV.reference_plan(IRP, JA, F.AS, "lower", unit=True)
    up = TV.reference_plan(IRP, JA, F.AS, "upper")
    return (lo, True), (up, False), None


# ------------------------------------------------------------------ matrices
def reversed_order(M):
    return np.arange(M - 1, -1, -1)


def layered(sizes=(3, 140, 5, 131), seed=17, extra=4):
    """_ic0.layered_spd made nonsymmetric: rows numbered level by level; a row
    of level l > 0 has every column of level 0, one entry in level l - 1 and up
    to `extra` more in any earlier level; every entry is mirrored into the
    upper triangle with a value of its own.  The diagonal outweighs its row
    strictly.  Every two rows share the columns of level 0, and a row of level
    0 holds every later column, so the update loop has work in both triangles"""
    rng = np.random.default_rng(seed)
    first = np.concatenate(([0], np.cumsum(sizes)))
    M = int(first[-1])
    entries = {}
    for l in range(1, len(sizes)):
        for i in range(first[l], first[l + 1]):
            cols = set(range(first[1]))
            cols.add(int(rng.integers(first[l - 1], first[l])))
            cols |= set(rng.integers(0, first[l],
                                     int(rng.integers(0, extra + 1))).tolist())
            for c in sorted(cols):
                entries[(i, c)] = float(rng.uniform(-1.0, 1.0))
                entries[(c, i)] = float(rng.uniform(-1.0, 1.0))
    weight = np.ones(M)
    for (i, _), v in entries.items():
        weight[i] += abs(v)
    weight += rng.uniform(0.0, 1.0, M)
    r = [i for i, _ in entries] + list(range(M))
    c = [c for _, c in entries] + list(range(M))
    v = list(entries.values()) + list(weight)
    return G._csr(M, np.array(r), np.array(c), np.array(v))


def with_zero_pivot(mat, row):
    """`mat` with the diagonal of `row` set to 0.0"""
    M, IRP, JA, AS = mat
    AS = AS.copy()
    AS[diag_positions(M, IRP, JA)[row]] = 0.0
    return M, IRP, JA, AS


#: name -> matrix: at most 1073 rows, the smallest that reach each kernel
MATRICES = {
    # 65 thin levels: the chain kernel alone
    "convdiff(37,29)": lambda: BI.convdiff(37, 29, 0.5, 0.5),
    # levels of 537 and 536 rows: the wide kernel alone
    "red-black convdiff(37,29)": lambda: IC.permuted(
        BI.convdiff(37, 29, 0.5, 0.5), IC.red_black_order(37, 29)),
    # one thin and one wide level; the dense row 0 is the tail every other
    # row searches
    "arrow2(600,3)": lambda: BI.arrow2(600, 3),
    # the same with the dense row and column last: a row of 599 strict lower
    # entries, far longer than a group of lanes, and no fill
    "arrow2(600,3) reversed": lambda: IC.permuted(BI.arrow2(600, 3),
                                                  reversed_order(600)),
    "layered": layered,
}


def tridiagonal(M=40):
    M_, IRP, JA, AS = TV.chain(M)      # diagonal first in each row: sort
    rows = np.repeat(np.arange(M), np.diff(IRP))
    return G._csr(M, rows, JA.astype(np.int64), AS)
