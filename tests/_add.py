"""The sparse sum C = alpha A + beta B of two CSR matrices as spmv_csr_add
defines it (include/spmv_engine.h): `reference`, the contract in numpy, and
`model`, the size class of every row restated from the numbers of
S.add_shape().  Also the shapes the GPU tests run (tests/test_gpu_sparse_add.py), so
that the CPU test (tests/test_add.py) can hold them to what they are for.

A matrix is the tuple (M, N, IRP, JA, AS) of tests/_transpose.py."""
import functools

import numpy as np

import _spgemm as SG
import _transpose as TR

irp_of = TR.irp_of
from_rows = SG.from_rows
random_sorted = SG.random_sorted
dense = SG.dense
WIDE_N = SG.WIDE_N


def keys_of(A):
    M, N, IRP, JA, _ = A
    rows = np.repeat(np.arange(M, dtype=np.int64),
                     np.diff(np.asarray(IRP, np.int64)))
    return rows * max(N, 1) + np.asarray(JA, np.int64)


def reference(alpha, A, beta, B):
    """-> (IRP_C, JA_C, AS_C): the union of the two patterns, ascending;
    ta = rn(alpha a) where only A stores the column, tb = rn(beta b) where
    only B does, rn(ta + tb) where both do.  numpy rounds every product and
    every sum on its own"""
    M, N = A[0], A[1]
    assert (M, N) == (B[0], B[1])
    ka, kb = keys_of(A), keys_of(B)
    assert np.all(np.diff(ka) > 0) and np.all(np.diff(kb) > 0)
    keys = np.union1d(ka, kb)
    ia, ib = np.searchsorted(keys, ka), np.searchsorted(keys, kb)
    in_a, in_b = np.zeros(len(keys), bool), np.zeros(len(keys), bool)
    in_a[ia], in_b[ib] = True, True
    with np.errstate(all="ignore"):
        ta = np.float64(alpha) * np.asarray(A[4], np.float64)
        tb = np.float64(beta) * np.asarray(B[4], np.float64)
        V, W = np.zeros(len(keys)), np.zeros(len(keys))
        V[ia], W[ib] = ta, tb
        both = in_a & in_b
        V[~in_a] = W[~in_a]
        V[both] = V[both] + W[both]
    IRP = irp_of(np.bincount(keys // max(N, 1), minlength=M)[:M]
                 if M else [])
    return IRP, (keys % max(N, 1)).astype(np.int32), V


def matched(A, B):
    return len(np.intersect1d(keys_of(A), keys_of(B)))


def lens(A, B):
    """len_A(r) + len_B(r), int64"""
    return (np.diff(np.asarray(A[2], np.int64))
            + np.diff(np.asarray(B[2], np.int64)))


def pick_group(A, B, shape):
    """the smallest width that is not below the mean (nzA + nzB) / M"""
    M, entries = A[0], len(A[3]) + len(B[3])
    for w in shape["widths"]:
        if M <= 0 or w * M >= entries:
            return w
    return shape["widths"][-1]


def rows_in_bin(A, B, shape, mode=0):
    n = len(lens(A, B))
    if mode == 1:
        return (n, 0)
    if mode == 2:
        return (0, n)
    wide = int(np.count_nonzero(lens(A, B) > shape["edge"]))
    return (n - wide, wide)


def transpose(A):
    return SG.transpose(A)


def with_values(A, vals):
    return A[:4] + (np.asarray(vals, np.float64),)


def empty(M, N):
    return (M, N, irp_of([0] * M), np.zeros(0, np.int32), np.zeros(0))


# ---------------------------------------------------------- partial overlap
def overlap():
    """(A, B): 300 x 257, 0..9 entries a row, rows empty in A only (every
    7th), in B only (every 5th) and in both (every 35th)"""
    return (random_sorted(300, 257, 9, 50, empty_every=7),
            random_sorted(300, 257, 9, 51, empty_every=5))


def disjoint(M=200, N=301, seed=52):
    """(A, B): A holds even columns only, B odd ones"""
    rng = np.random.default_rng(seed)
    a, b = [], []
    for r in range(M):
        a.append((2 * np.sort(rng.choice(N // 2, int(rng.integers(0, 9)),
                                         replace=False))).tolist())
        b.append((2 * np.sort(rng.choice(N // 2, int(rng.integers(0, 9)),
                                         replace=False)) + 1).tolist())
    return from_rows(N, a, rng=rng), from_rows(N, b, rng=rng)


def degenerate():
    """name -> (A, B)"""
    out = {}
    out["A empty"] = (empty(7, 9), random_sorted(7, 9, 4, 53))
    out["B empty"] = (random_sorted(7, 9, 4, 54), empty(7, 9))
    out["both empty"] = (empty(7, 9), empty(7, 9))
    out["M = 0"] = (empty(0, 6), empty(0, 6))
    out["M = 1"] = (random_sorted(1, 40, 30, 55), random_sorted(1, 40, 30, 56))
    rng = np.random.default_rng(57)
    out["N = 1"] = (from_rows(1, [[0], [], [0], []], rng=rng),
                    from_rows(1, [[0], [0], [], []], rng=rng))
    out["N = 0"] = (empty(5, 0), empty(5, 0))
    return out


# --------------------------------------------------------------- the edges
WAYS = ("none", "all", "first", "last")
BIG = 5000  # the shared last column; every other column is below it


def row_pair(la, lb, way):
    """two ascending column lists of la and lb entries whose common columns
    are: none; all of the shorter list; only the first column of each; only
    the last column of each"""
    if way == "all":
        long_, short = max(la, lb), min(la, lb)
        cols = np.arange(long_) * 3
        # distinct places, the first and the last among them
        sub = cols[np.arange(short) * (long_ - 1) // max(short - 1, 1)]
        return (cols, sub) if la >= lb else (sub, cols)
    a, b = 2 * np.arange(la) + 2, 2 * np.arange(lb) + 3
    if way == "first" and la and lb:
        a[0] = b[0] = 0
    if way == "last" and la and lb:
        a[-1] = b[-1] = BIG
    return a, b


def edge_lengths(shape, w):
    """len_A + len_B one below, at and one above: the width and twice the
    width, 64 and 128 (a wavefront), the workgroup and the class edge"""
    marks = sorted({w, 2 * w, 64, 128, shape["threads"], shape["edge"]})
    return sorted({m + d for m in marks for d in (-1, 0, 1)})


@functools.lru_cache(maxsize=None)
def edges(w, seed=58):
    """(A, B, what) whose mean len_A + len_B selects the group width w: for
    every length of edge_lengths and both splits of it (halves; all but two
    against two) a row for each of the four placements of the matches, then
    filler rows of w - 1 entries (1 for w = 2) in A alone until the mean is at
    most w.  what[r] = (la, lb, way) of the first rows"""
    import spmv_scpa_amd as S
    shape = S.add_shape()
    rng = np.random.default_rng(seed + w)
    a, b, what = [], [], []
    for L in edge_lengths(shape, w):
        for la in sorted({L // 2, max(L - 2, 0)}):
            for way in WAYS:
                ra, rb = row_pair(la, L - la, way)
                a.append(ra.tolist())
                b.append(rb.tolist())
                what.append((la, L - la, way))
    S_, R = sum(len(x) + len(y) for x, y in zip(a, b)), len(a)
    f = max(w - 1, 1)
    F = max(0, S_ - w * R) + 1
    A, B = from_rows(BIG + 1, a, rng=rng), from_rows(BIG + 1, b, rng=rng)
    # the filler rows as arrays (tens of thousands of them): row r holds the
    # columns r % 7 .. r % 7 + f - 1 in A and nothing in B
    cols = (np.arange(F)[:, None] % 7 + np.arange(f)[None, :]).astype(np.int32)
    A = (R + F, BIG + 1, irp_of(np.concatenate([np.diff(A[2]), np.full(F, f)])),
         np.concatenate([A[3], cols.ravel()]),
         np.concatenate([A[4], rng.uniform(-2, 2, F * f)]))
    B = (R + F, BIG + 1, irp_of(np.concatenate([np.diff(B[2]), np.zeros(F, np.int64)])),
         B[3], B[4])
    return A, B, what


@functools.lru_cache(maxsize=None)
def edges_reference(w):
    A, B, _ = edges(w)
    return reference(1.5, A, -0.75, B)


# ---------------------------------------------------------------- long rows
def long_against_one():
    """(A, B): three copies of a row of 3000 entries against a one-entry row
    that holds its first column, its last column, and a column it lacks"""
    rng = np.random.default_rng(59)
    long_row = (5 * np.arange(3000) + 5).tolist()
    A = from_rows(15006, [long_row] * 3, rng=rng)
    B = from_rows(15006, [[5], [15000], [7]], rng=rng)
    return A, B


@functools.lru_cache(maxsize=None)
def wide_n():
    """(A, B): two 4 x (2^24 + 1) matrices of the product's wide_n maker: a
    row of 5000 entries over all of [0, N), short rows that reach the last
    column, an empty row.  The two long rows share four columns at least"""
    return SG.wide_n(seed=24)[1], SG.wide_n(seed=60)[1]


# ------------------------------------------------------------------- values
def special():
    """(alpha, A, beta, B) cases, 1 x 8 each, by name"""
    inf, nan, sub = np.inf, np.nan, 2.0 ** -1070
    cols = [0, 1, 2, 3, 4, 5]
    out = {}
    # a lone -0.0 in A (column 0) and in B (column 1), a pair of them
    # (column 2: -0.0 + -0.0 = -0.0), -0.0 + 0.0 = +0.0 (column 3)
    out["zeros"] = (1.0, from_rows(8, [[0, 2, 3]], [-0.0, -0.0, -0.0]),
                    1.0, from_rows(8, [[1, 2, 3]], [-0.0, -0.0, 0.0]))
    out["inf - inf"] = (1.0, from_rows(8, [cols], [inf, 1, 2, -inf, 4, 5]),
                        -1.0, from_rows(8, [[0, 3, 5]], [inf, inf, 1.0]))
    out["alpha = 0"] = (0.0, from_rows(8, [cols], [inf, 1, -2, -inf, 4, 5]),
                        2.0, from_rows(8, [[0, 1, 7]], [1.0, 1.0, 1.0]))
    out["subnormal"] = (0.5, from_rows(8, [cols], [sub, 3 * sub, -sub,
                                                   2.0 ** -1074, 1.0, 0.0]),
                        1.0, from_rows(8, [[0, 2, 3]], [sub, sub,
                                                        2.0 ** -1074]))
    out["nan"] = (1.0, from_rows(8, [cols], [1, nan, 3, 4, 5, 6]),
                  1.0, from_rows(8, [[0, 1, 6]], [1.0, 1.0, 1.0]))
    return out


def shifted_stencil(n=40, sigma=1.3):
    """(A, want): the five-point stencil on n^2 and A - sigma I built on the
    host (the diagonal is stored in every row: one rounded sum per row)"""
    import _cg as G
    M, IRP, JA, AS = G.lap2d(n, n, 0.0)
    rows = np.repeat(np.arange(M), np.diff(IRP))
    V = AS.copy()
    d = JA == rows
    V[d] = AS[d] + np.float64(-sigma) * 1.0
    return (M, M, IRP, JA, AS), (IRP, JA, V)
