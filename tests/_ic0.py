"""Zero-fill incomplete Cholesky (spmv_csr_ic0; spmv_engine.h) restated in
numpy, straight from the definition in the header, and the matrices its tests
run.  No GPU here.

reference_ic0   plain Python loops over float64 scalars: numpy rounds every
                operation once, as the device does
red_black       lap2d with the grid points of one colour numbered first: two
                levels, both wide
layered_spd     rows that share strict columns, so that the sums of the
                definition are not empty (a 5-point stencil has no fill to
                drop: no two of its rows share a column below both)

A matrix is (M, IRP, JA, AS) with int32 index arrays and float64 values, every
row ascending by column.
"""
import collections

import numpy as np

import _cg as G
import _pcg as PG

Factor = collections.namedtuple("Factor", "IRP JA AS bad_pivots bad_rows")


def lower_of(M, IRP, JA, AS):
    """the stored-lower-only copy: entries with column <= row"""
    rows = np.repeat(np.arange(M), np.diff(IRP))
    keep = JA <= rows
    LIRP = np.zeros(M + 1, np.int32)
    LIRP[1:] = np.cumsum(np.bincount(rows[keep], minlength=M))
    return (M, LIRP, np.ascontiguousarray(JA[keep], np.int32),
            np.ascontiguousarray(AS[keep], np.float64))


def reference_ic0(M, IRP, JA, AS, shift=0.0):
    """-> Factor: L in the pattern of the lower triangle (the diagonal last in
    each row), the number of rows whose pivot was not > 0, and those rows"""
    _, LIRP, LJA, L = lower_of(M, IRP, JA, AS)
    L = L.copy()
    shift = np.float64(shift)
    bad = []
    with np.errstate(all="ignore"):
        for i in range(M):
            b, d = LIRP[i], LIRP[i + 1] - 1
            assert d >= b and LJA[d] == i, "row %d stores no diagonal" % i
            assert np.all(np.diff(LJA[b:d + 1]) > 0), "row %d not ascending" % i
            for t in range(b, d):
                j = LJA[t]
                bj, dj = LIRP[j], LIRP[j + 1] - 1
                # the columns below j stored in both rows, in increasing order
                _, ia, ib = np.intersect1d(LJA[b:t], LJA[bj:dj],
                                           assume_unique=True,
                                           return_indices=True)
                s = np.float64(0.0)
                for x, y in zip(ia, ib):
                    s = s + L[b + x] * L[bj + y]
                L[t] = (L[t] - s) / L[dj]
            s = np.float64(0.0)
            for t in range(b, d):
                s = s + L[t] * L[t]
            piv = (L[d] + shift * L[d]) - s
            L[d] = np.sqrt(piv)
            if not piv > 0:
                bad.append(i)
    return Factor(LIRP, LJA, L, len(bad), np.array(bad, np.int64))


def nan_rows(F):
    """mask of the rows of a Factor that hold a NaN"""
    M = len(F.IRP) - 1
    rows = np.repeat(np.arange(M), np.diff(F.IRP))
    return np.bincount(rows[np.isnan(F.AS)], minlength=M) > 0


def pattern_ratio(mat, F, shift=0.0):
    """the largest |sum_m L_im L_jm - a_ij| / ((n + 3) u sum_m |L_im L_jm|)
    over the stored lower entries (i, j), n = the common columns below j,
    u = 2^-53; the sums in extended precision.  On the pattern L L^T is A (+
    shift diag(A))"""
    E = np.longdouble
    M, IRP, JA, AS = lower_of(*mat)
    worst = 0.0
    for i in range(M):
        b, d = F.IRP[i], F.IRP[i + 1] - 1
        for t in range(b, d + 1):
            j = F.JA[t]
            bj, dj = F.IRP[j], F.IRP[j + 1] - 1
            _, ia, ib = np.intersect1d(F.JA[b:t], F.JA[bj:dj],
                                       assume_unique=True, return_indices=True)
            prods = F.AS[b + ia].astype(E) * F.AS[bj + ib].astype(E)
            prods = np.append(prods, E(F.AS[t]) * E(F.AS[dj]))
            a = E(AS[t])
            if j == i:
                a = a + E(shift) * a
            bound = (len(ia) + 3) * E(2.0) ** -53 * np.abs(prods).sum()
            worst = max(worst, float(abs(prods.sum() - a) / bound))
    return worst


# ------------------------------------------------------------------ matrices
def permuted(mat, new_of_old):
    """P A P^T: row and column r of `mat` become new_of_old[r]; rows ascending"""
    M, IRP, JA, AS = mat
    rows = np.repeat(np.arange(M), np.diff(IRP))
    return G._csr(M, new_of_old[rows], new_of_old[JA], AS)


def red_black_order(nx, ny):
    """new_of_old for an nx x ny grid: the points with x + y even first"""
    y, x = np.divmod(np.arange(nx * ny), nx)
    old_of_new = np.argsort((x + y) % 2, kind="stable")
    new_of_old = np.empty(nx * ny, np.int64)
    new_of_old[old_of_new] = np.arange(nx * ny)
    return new_of_old


def red_black(nx, ny, shift):
    """_cg.lap2d in red-black order: every strict lower entry of a black row is
    a red column, so the lower triangle has 2 levels"""
    return permuted(G.lap2d(nx, ny, shift), red_black_order(nx, ny))


def layered_spd(sizes=(3, 140, 5, 131), seed=13, extra=4):
    """rows numbered level by level; a row of level l > 0 has every column of
    level 0, one entry in level l - 1 and up to `extra` more in any earlier
    level.  Symmetric, the diagonal outweighs its row: SPD.  Every two rows
    share the columns of level 0, so the sums of the factorisation have
    terms"""
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
            for c in cols:
                entries[(i, c)] = float(rng.uniform(-1.0, 1.0))
    weight = np.ones(M)
    for (i, c), v in entries.items():
        weight[i] += abs(v)
        weight[c] += abs(v)
    r = [i for i, _ in entries] + [c for _, c in entries] + list(range(M))
    c = [c for _, c in entries] + [i for i, _ in entries] + list(range(M))
    v = list(entries.values()) * 2 + list(weight)
    return G._csr(M, np.array(r), np.array(c), np.array(v))


#: the matrices of the issue, and one whose rows share columns
MATRICES = {
    "lap2d(37,29,0.01)": lambda: G.lap2d(37, 29, 0.01),
    "red-black(37,29,0.01)": lambda: red_black(37, 29, 0.01),
    "arrow(600,3)": lambda: G.arrow(600, 3),
    "scaled(37,29,0.01)": lambda: PG.scaled_lap2d(37, 29, 0.01, 3, 5),
    "layered": layered_spd,
}
