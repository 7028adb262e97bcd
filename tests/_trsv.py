"""The level-scheduled triangular solve (spmv_csr_trsv_analyse,
spmv_trsv_solve; spmv_engine.h) restated in numpy, straight from the
definitions in the header, and the shapes its tests run.

reference_plan      level, order, level_ptr, rowptr, ja, as, diag of a triangle
reference_solve     a plain Python loop: G slots per row, the halving tree,
                    rn(rhs - s), a division -- numpy's float64 operations are
                    rounded once each, as the device's are
segments            the launch list of trsv_plan.h
shapes(L)           name -> (M, IRP, JA, AS); L = small_rows of trsv_shape()

A matrix is (M, IRP, JA, AS) with int32 index arrays and float64 values; every
shape stores BOTH triangles, so both `uplo` have something to do.
"""
import numpy as np

import _cg as G

WIDE, CHAIN = 0, 1


def irp_of(lens):
    IRP = np.zeros(len(lens) + 1, np.int32)
    IRP[1:] = np.cumsum(lens)
    return IRP


def from_rows(rows):
    """rows[i] = list of (column, value) in the order they are stored"""
    M = len(rows)
    IRP = irp_of([len(r) for r in rows])
    JA = np.array([c for r in rows for c, _ in r], np.int32)
    AS = np.array([v for r in rows for _, v in r], np.float64)
    return M, IRP, JA, AS


# ------------------------------------------------------------- the reference
def reference_plan(IRP, JA, AS, uplo, unit=False):
    """uplo "lower" / "upper".  `unit` changes nothing here: the plan's diag
    is the sum of the stored diagonal either way, only the solve ignores it"""
    M = len(IRP) - 1
    upper = uplo == "upper"
    level = np.zeros(M, np.int32)
    diag = np.zeros(M, np.float64)
    strict = [None] * M
    for i in (range(M - 1, -1, -1) if upper else range(M)):
        cols = JA[IRP[i]:IRP[i + 1]]
        vals = AS[IRP[i]:IRP[i + 1]]
        d = np.float64(0.0)
        for v in vals[cols == i]:
            d = d + v  # in stored order
        diag[i] = d
        keep = cols > i if upper else cols < i
        strict[i] = (cols[keep], vals[keep])
        if keep.any():
            level[i] = 1 + level[cols[keep]].max()
    order = np.argsort(level, kind="stable").astype(np.int32)
    levels = int(level.max()) + 1 if M else 0
    level_ptr = irp_of(np.bincount(level, minlength=levels)[:levels])
    rowptr = irp_of([len(strict[r][0]) for r in order])
    ja = (np.concatenate([strict[r][0] for r in order]) if M
          else np.zeros(0)).astype(np.int32)
    vals = (np.concatenate([strict[r][1] for r in order]) if M
            else np.zeros(0)).astype(np.float64)
    return dict(level=level, order=order, level_ptr=level_ptr, rowptr=rowptr,
                ja=ja, diag=diag, **{"as": vals})


def reference_solve(plan, B, scale, G, unit=False):
    """X (M, k) from B (M, k): the contract of spmv_trsv_solve, one rounding
    per operation, all k columns at once (they never meet)"""
    order, rowptr, ja, vals = (plan[n] for n in ("order", "rowptr", "ja", "as"))
    diag = plan["diag"]
    B = np.asarray(B, np.float64)
    M, k = B.shape
    X = np.zeros((M, k))
    with np.errstate(all="ignore"):
        for p in range(M):
            i = order[p]
            slot = np.zeros((G, k))
            for e in range(rowptr[p], rowptr[p + 1]):
                g = (e - rowptr[p]) % G
                slot[g] = slot[g] + vals[e] * X[ja[e]]
            h = G // 2
            while h >= 1:
                slot[:h] = slot[:h] + slot[h:2 * h]
                h //= 2
            rhs = B[i] if scale is None else scale[i] * B[i]
            t = rhs - slot[0]
            X[i] = t if unit else t / diag[i]
    return X


def segments(level_ptr, small_rows):
    """[(kind, first_level, last_level)]: a level of more than small_rows rows
    is a WIDE launch of its own, a maximal run of the others one CHAIN"""
    out, run = [], None
    for l, rows in enumerate(np.diff(level_ptr)):
        if rows <= small_rows:
            run = l if run is None else run
            continue
        if run is not None:
            out.append((CHAIN, run, l - 1))
            run = None
        out.append((WIDE, l, l))
    if run is not None:
        out.append((CHAIN, run, len(level_ptr) - 2))
    return out


def reachable(plan, r):
    """mask of the rows whose value depends on row r (r included)"""
    M = len(plan["order"])
    hit = np.zeros(M, bool)
    hit[r] = True
    for p in range(M):  # in level order: dependencies come first
        i = plan["order"][p]
        if hit[plan["ja"][plan["rowptr"][p]:plan["rowptr"][p + 1]]].any():
            hit[i] = True
    return hit


def row_bound(plan, X, unit=False):
    """(n_i + 3) u sum_c |T_ic| |x_c| per row and column, u = 2^-53: n_i
    products and sums, one subtraction and one division"""
    M, k = X.shape
    out = np.zeros((M, k))
    for p in range(M):
        i = plan["order"][p]
        e = slice(plan["rowptr"][p], plan["rowptr"][p + 1])
        d = 1.0 if unit else abs(plan["diag"][i])
        s = d * np.abs(X[i]) + (np.abs(plan["as"][e])[:, None]
                                * np.abs(X[plan["ja"][e]])).sum(axis=0)
        out[i] = (e.stop - e.start + 3) * 2.0 ** -53 * s
    return out


def residual(plan, B, X, unit=False):
    """|b - T x| per row and column in extended precision"""
    L = np.longdouble
    M, k = X.shape
    out = np.zeros((M, k), L)
    for p in range(M):
        i = plan["order"][p]
        e = slice(plan["rowptr"][p], plan["rowptr"][p + 1])
        d = L(1.0) if unit else L(plan["diag"][i])
        acc = d * X[i].astype(L)
        acc = acc + (plan["as"][e].astype(L)[:, None]
                     * X[plan["ja"][e]].astype(L)).sum(axis=0)
        out[i] = np.abs(B[i].astype(L) - acc)
    return out


def dense_of(plan, unit=False):
    """the triangle as a dense matrix (duplicates summed)"""
    M = len(plan["order"])
    T = np.zeros((M, M))
    for p in range(M):
        i = plan["order"][p]
        for e in range(plan["rowptr"][p], plan["rowptr"][p + 1]):
            T[i, plan["ja"][e]] += plan["as"][e]
        T[i, i] = 1.0 if unit else plan["diag"][i]
    return T


def dense_solve(T, B, upper):
    """forward / back substitution, row by row"""
    M = len(T)
    X = np.zeros_like(B)
    for i in (range(M - 1, -1, -1) if upper else range(M)):
        X[i] = (B[i] - T[i] @ X) / T[i, i]  # X[i] is still zero
    return X


# ------------------------------------------------------------------ shapes
def empty():
    return 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0)


def single():
    return from_rows([[(0, 2.5)]])


def diagonal(M=40):
    return from_rows([[(i, 1.0 + 0.25 * i)] for i in range(M)])


def chain(M=300):
    """tridiagonal: M levels either way, one chain segment"""
    rows = []
    for i in range(M):
        r = [(i, 3.0 + (i % 5) * 0.125)]
        if i > 0:
            r.append((i - 1, -1.0 - (i % 3) * 0.25))
        if i + 1 < M:
            r.append((i + 1, 0.5 + (i % 7) * 0.0625))
        rows.append(r)
    return from_rows(rows)


def lap(nx, ny, shift=0.5):
    M, IRP, JA, AS = G.lap2d(nx, ny, shift)
    return M, IRP.astype(np.int32), JA.astype(np.int32), AS


def random_triangle(M=5000, seed=11, dominant=False):
    """0-12 strict lower entries per row (columns below i / 8 + 1, so that
    levels of both kinds appear at M = 5000), unsorted, with duplicates and
    explicit zeros; 0-3 entries in the other triangle; rows without a
    diagonal and rows that store it twice (dominant=True: every row stores a
    diagonal that outweighs the rest of the row in both triangles)"""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(M):
        n = int(rng.integers(0, 13)) if i else 0
        # dependencies reach far back: few levels, some of them wide
        cols = rng.integers(0, i // 8 + 1, n).tolist() if n else []
        if n >= 4:
            cols[1] = cols[0]  # a duplicate
        up = rng.integers(i + 1, M, int(rng.integers(0, 4))).tolist() \
            if i + 1 < M else []
        r = [(c, float(rng.uniform(-1.0, 1.0))) for c in cols + up]
        if n >= 2:
            r[0] = (r[0][0], 0.0)  # an explicit zero: still a dependency
        weight = sum(abs(v) for _, v in r) + 1.0
        kind = 1 if dominant else int(rng.integers(0, 6))
        if kind == 0:
            dg = []  # no stored diagonal
        elif kind == 5 or (dominant and i % 7 == 3):
            dg = [(i, 0.75 * weight), (i, 0.5 * weight)]  # stored twice
        else:
            dg = [(i, weight)]
        r = r + dg
        rows.append([r[j] for j in rng.permutation(len(r))])
    return from_rows(rows)


def layered(sizes, seed=5, extra=3):
    """rows numbered level by level: a row of level l > 0 has one entry in
    level l - 1 and up to `extra` more in any earlier level, stored unsorted;
    every entry is mirrored into the upper triangle with another value"""
    rng = np.random.default_rng(seed)
    first = np.concatenate(([0], np.cumsum(sizes)))
    rows = [[] for _ in range(first[-1])]
    for l, n in enumerate(sizes):
        for i in range(first[l], first[l + 1]):
            cols = []
            if l > 0:
                cols.append(int(rng.integers(first[l - 1], first[l])))
                cols += rng.integers(0, first[l],
                                     int(rng.integers(0, extra + 1))).tolist()
            for c in cols:
                rows[i].append((c, float(rng.uniform(-1.0, 1.0))))
                rows[c].append((i, float(rng.uniform(-1.0, 1.0))))
            rows[i].append((i, 4.0 + float(rng.uniform(0.0, 1.0))))
    rows = [[r[j] for j in rng.permutation(len(r))] for r in rows]
    return from_rows(rows)


def arrow(n=4500):
    """the last row holds 2 n = 9000 strict entries (every column twice): a row
    far longer than the lane group; level 0 is n rows wide"""
    rng = np.random.default_rng(3)
    rows = [[(i, 2.0 + 0.001 * i)] for i in range(n)]
    cols = np.concatenate((rng.permutation(n), rng.permutation(n)))
    last = [(int(c), float(rng.uniform(-1.0, 1.0)) / n) for c in cols]
    rows.append(last[:n] + [(n, 3.0)] + last[n:])
    return from_rows(rows)


FANS = ("L-1", "L", "L+1", "3L+5")


def fan_rows(L, which):
    return {"L-1": L - 1, "L": L, "L+1": L + 1, "3L+5": 3 * L + 5}[which]


def shapes(L):
    """name -> matrix.  L = small_rows of trsv_shape()"""
    out = {"empty": empty(), "single": single(), "diagonal": diagonal(),
           "chain300": chain(300), "lap2d": lap(17, 13),
           "random": random_triangle(), "arrow": arrow(),
           # thin, thin, WIDE, thin, thin: chain / wide / chain
           "sandwich": layered([3, 2, L + 7, 4, 1], seed=9)}
    for which in FANS:
        out["fan " + which] = layered([5, fan_rows(L, which)], seed=21,
                                      extra=2)
    return out
