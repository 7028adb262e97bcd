"""Smoothed-aggregation AMG (spmv_csr_aggregate, spmv_csr_amg_setup,
spmv_amg_apply, spmv_*_pcg_amg; spmv_engine.h) restated in numpy, straight
from the definitions in the header, and the matrices its tests run.  No GPU
here.

strong_edges    the strong entries of every row, in stored order
mis2            the distance-2 independent set by parallel rounds
aggregate       roots, the three passes, the info
gershgorin      rho and w of one level
prolongator     T, A T and P = T - diag(w) A T
hierarchy       every level: A_l, P, PT, w, rho, omega, rounds
cycle           V(sweeps, sweeps) with any product (the device's launch_multi
                for the bits, the CPU oracle's for the properties)
pcg_amg         tests/_pcg_trsv.py restate with apply = the cycle

A square matrix is (M, IRP, JA, AS) with int32 index arrays; the products and
the transposition take the (M, N, IRP, JA, AS) of tests/_spgemm.py.
"""
import collections

import numpy as np

import _cg as G
import _colour as CO
import _pcg_trsv as PT
import _spgemm as SG
import _transpose as TR
import _trsv as TV

Aggregation = collections.namedtuple(
    "Aggregation", "agg aggregates roots rounds widest singletons root_mask")
Level = collections.namedtuple("Level", "A P PT w rho omega agg")


def int32(mat):
    M, IRP, JA, AS = mat
    return (M, np.asarray(IRP, np.int32), np.asarray(JA, np.int32),
            np.asarray(AS, np.float64))


def rows_of(M, IRP):
    return np.repeat(np.arange(M, dtype=np.int64), np.diff(IRP))


def diagonal(mat):
    """d[i]: the stored (i, i); every row holds it once"""
    M, IRP, JA, AS = mat
    rows = rows_of(M, IRP)
    d = np.zeros(M)
    on = rows == JA
    d[rows[on]] = AS[on]
    return d


def well_formed(mat):
    """rows strictly ascending, every column inside, the diagonal stored"""
    M, IRP, JA, AS = mat
    rows = rows_of(M, IRP)
    if len(JA) and (JA.min() < 0 or JA.max() >= M):
        return False
    inner = np.ones(len(JA), bool)
    inner[IRP[:-1][np.diff(IRP) > 0]] = False     # the first of every row
    if np.any(inner[1:] & (JA[1:] <= JA[:-1])):
        return False
    return int(np.sum(rows == JA)) == M


def strong_edges(mat, theta):
    """-> (row, column, |a|, position) of the strong entries, stored order:
    (i, j), j != i, is strong iff rn(a a) >= rn(theta^2 |rn(d_i d_j)|); a
    comparison with a NaN is false"""
    M, IRP, JA, AS = mat
    rows = rows_of(M, IRP)
    d = diagonal(mat)
    theta2 = np.float64(theta) * np.float64(theta)
    with np.errstate(all="ignore"):
        lhs = AS * AS
        rhs = theta2 * np.abs(d[rows] * d[JA])
        strong = (JA != rows) & (lhs >= rhs)
    pos = np.flatnonzero(strong)
    return rows[pos], JA[pos].astype(np.int64), np.abs(AS[pos]), pos


def mis2(M, er, ec, seed):
    """-> (root mask, rounds).  Every row carries (state, fmix32(row ^ seed),
    row) with out < undecided < root; a round takes the maximum over the strong
    neighbours twice and decides: an undecided row that is its own distance-2
    maximum becomes a root, one whose maximum is a root becomes out"""
    h = CO.priority(M, seed).astype(np.int64)
    order = np.lexsort((np.arange(M), h))
    rank = np.empty(M, np.int64)
    rank[order] = np.arange(M)          # the order of (hash, row)
    state = np.ones(M, np.int64)        # 0 out, 1 undecided, 2 root
    rounds = 0
    while np.any(state == 1):
        key = state * M + rank
        t1 = key.copy()
        np.maximum.at(t1, er, key[ec])
        t2 = t1.copy()
        np.maximum.at(t2, er, t1[ec])
        und = state == 1
        root = und & (t2 == key)
        out = und & ~root & (t2 // M == 2)
        state[root] = 2
        state[out] = 0
        rounds += 1
    return state == 2, rounds


def _pick(rows, absv, pos):
    """per row the candidate of the greatest |a|, the first in stored order
    among equals -> (rows, indices into the candidate arrays)"""
    order = np.lexsort((pos, -absv, rows))
    r = rows[order]
    first = np.ones(len(r), bool)
    first[1:] = r[1:] != r[:-1]
    return r[first], order[first]


def aggregate(mat, theta=0.0, seed=0):
    mat = int32(mat)
    M = mat[0]
    if M == 0:
        return Aggregation(np.zeros(0, np.int32), 0, 0, 0, 0, 0,
                           np.zeros(0, bool))
    er, ec, ea, ep = strong_edges(mat, theta)
    root, rounds = mis2(M, er, ec, seed)
    nroots = int(root.sum())
    rid = np.cumsum(root) - root        # the exclusive scan
    agg1 = np.where(root, rid, -1)
    c = root[ec] & ~root[er]
    r, i = _pick(er[c], ea[c], ep[c])
    agg1[r] = rid[ec[c][i]]
    agg2 = agg1.copy()
    c = (agg1[er] < 0) & (agg1[ec] >= 0)
    r, i = _pick(er[c], ea[c], ep[c])
    agg2[r] = agg1[ec[c][i]]
    single = agg2 < 0
    agg = agg2.copy()
    agg[single] = nroots + np.cumsum(single)[single] - 1
    n = nroots + int(single.sum())
    return Aggregation(agg.astype(np.int32), n, nroots, rounds,
                       int(np.bincount(agg, minlength=n).max()),
                       int(single.sum()), root)


def gershgorin(mat):
    """-> (rho, omega, w): rho = max_i rn(S_i / |d_i|), S_i the sequential sum
    of |a_ij| in stored order from 0.0; omega = (4/3) / rho; w = omega / d"""
    M, IRP, JA, AS = mat
    d = diagonal(mat)
    lens = np.diff(IRP)
    S = np.zeros(M)
    a = np.abs(AS)
    with np.errstate(all="ignore"):
        for q in range(int(lens.max()) if M else 0):
            sel = np.flatnonzero(lens > q)
            S[sel] = S[sel] + a[IRP[sel].astype(np.int64) + q]
        q = S / np.abs(d)
        rho = np.float64(np.nan) if np.any(np.isnan(q)) else q.max()
        omega = np.float64(4.0 / 3.0) / rho
        w = omega / d
    return rho, omega, w


def prolongator(mat, agg, n, w):
    """-> P as (M, n, IRP, JA, AS): the pattern of A T, p = rn(t - rn(w_i at))"""
    M, IRP, JA, AS = mat
    A = (M, M, IRP, JA, AS)
    T = (M, n, np.arange(M + 1, dtype=np.int32), agg.astype(np.int32),
         np.ones(M))
    pi, pj, pv = SG.reference(A, T)
    rows = rows_of(M, pi)
    with np.errstate(all="ignore"):
        t = np.where(pj == agg[rows], 1.0, 0.0)
        pv = t - w[rows] * pv
    return (M, n, pi, pj, pv)


def transposed(Pm):
    M, N, IRP, JA, AS = Pm
    ti, tj, tv = TR.reference(IRP, JA, AS, N)
    return (N, M, ti, tj.astype(np.int32), tv)


def hierarchy(mat, theta=0.0, min_rows=32, max_levels=16, seed=0):
    """-> [Level]: the last one has P, PT and agg None"""
    mat = int32(mat)
    levels = []
    while True:
        M = mat[0]
        rho, omega, w = gershgorin(mat)
        if not (np.isfinite(rho) and rho > 0):
            raise FloatingPointError("rho = %r" % (rho,))
        if M <= min_rows or len(levels) + 1 == max_levels:
            levels.append(Level(mat, None, None, w, rho, omega, None))
            return levels
        ag = aggregate(mat, theta, seed)
        if ag.aggregates == M:
            levels.append(Level(mat, None, None, w, rho, omega, None))
            return levels
        P = prolongator(mat, ag.agg, ag.aggregates, w)
        PTm = transposed(P)
        A5 = (M, M) + mat[1:]
        ci, cj, cv = SG.reference(PTm, (M, ag.aggregates) + SG.reference(A5, P))
        levels.append(Level(mat, P, PTm, w, rho, omega, ag))
        mat = (ag.aggregates, ci, cj, cv)


def complexity(levels):
    return sum(len(l.A[2]) for l in levels) / len(levels[0].A[2])


def oracle_products(levels, spmv):
    """the CPU stand-ins: -> products[l] = (A, P, PT) callables on (rows, k)"""
    def of(IRP, JA, AS):
        return G.dense_product(IRP, JA, AS, spmv)[0]
    return [(of(*l.A[1:]),
             of(*l.P[2:]) if l.P is not None else None,
             of(*l.PT[2:]) if l.PT is not None else None) for l in levels]


def cycle(levels, products, sweeps=1, coarse_sweeps=8):
    """-> apply(R) -> Z, the V cycle of spmv_amg_apply.  products[l] = (A, P,
    PT): callables X (rows, k) -> the product with the bits of launch_multi"""
    def smooth(l, x, b, n):
        w = levels[l].w[:, None]
        for _ in range(n):
            x = x + w * (b - products[l][0](x))
        return x

    def level(l, b):
        w = levels[l].w[:, None]
        x = w * b
        if l == len(levels) - 1:
            return smooth(l, x, b, coarse_sweeps - 1)
        x = smooth(l, x, b, sweeps - 1)
        r = b - products[l][0](x)
        xc = level(l + 1, products[l][2](r))
        x = x + products[l][1](xc)
        return smooth(l, x, b, sweeps)

    def apply(R):
        with np.errstate(all="ignore"):
            return level(0, np.asarray(R, np.float64))
    return apply


def pcg_amg(product, residual0, B, X0, apply, tol, maxit, shape=None):
    return PT.restate(product, residual0, B, X0, apply, tol, maxit, shape)


# ------------------------------------------------------------------ matrices
def lap2d(nx, ny=None, diag=4.01):
    return int32(G.lap2d(nx, ny or nx, diag - 4.0))


def anisotropic(nx, ny, weak=0.01):
    """5-point, -1 along x and -weak along y, the diagonal outweighs the row"""
    idx = np.arange(nx * ny).reshape(ny, nx)
    rows, cols, vals = [idx.ravel()], [idx.ravel()], \
        [np.full(nx * ny, 2.0 + 2.0 * weak + 0.01)]
    for (a, b), v in (((idx[:, :-1], idx[:, 1:]), -1.0),
                      ((idx[:-1, :], idx[1:, :]), -weak)):
        for r, c in ((a, b), (b, a)):
            rows.append(r.ravel())
            cols.append(c.ravel())
            vals.append(np.full(r.size, v))
    return int32(G._csr(nx * ny, np.concatenate(rows), np.concatenate(cols),
                        np.concatenate(vals)))


def zeros_and_nan(nx=9, ny=7):
    """lap2d with an explicit zero in every third row's first off-diagonal and
    one NaN off-diagonal (stored on one side): the zero is strong at theta 0,
    the NaN never is"""
    M, IRP, JA, AS = lap2d(nx, ny)
    AS = AS.copy()
    rows = rows_of(M, IRP)
    off = np.flatnonzero(rows != JA)
    AS[off[::7]] = 0.0
    AS[off[5]] = np.nan
    return M, IRP, JA, AS


#: name -> (matrix maker, theta): the shapes of the issue
AGG = {
    "lap2d(40,40)": (lambda: lap2d(40, 40), 0.0),
    "stencil27(8)": (lambda: int32(CO.stencil27(8)), 0.0),
    "arrow(600,3)": (lambda: int32(G.arrow(600, 3)), 0.0),
    "anisotropic(33,21)": (lambda: anisotropic(33, 21), 0.25),
    "lower_bidiagonal(300)": (lambda: int32(CO.lower_bidiagonal(300)), 0.0),
    "diagonal": (lambda: int32(TV.diagonal()), 0.0),
    "zeros and a NaN": (zeros_and_nan, 0.0),
    "M = 0": (lambda: int32(TV.empty()), 0.0),
    "M = 1": (lambda: int32(TV.single()), 0.0),
}

_cache = {}


def reference(name, seed):
    """(mat, theta, Aggregation) of a named matrix, computed once and shared:
    treat the arrays as read-only"""
    if (name, seed) not in _cache:
        make, theta = AGG[name]
        mat = make()
        _cache[name, seed] = (mat, theta, aggregate(mat, theta, seed))
    return _cache[name, seed]


def reference_hierarchy(nx=64, **kw):
    key = ("H", nx, tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = hierarchy(lap2d(nx, nx), **kw)
    return _cache[key]
