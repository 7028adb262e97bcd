"""The sparse product C = A B of two CSR matrices as spmv_csr_spgemm defines it
(include/spmv_engine.h): `reference`, the contract in numpy, and `model`, the
size class of every row restated from the numbers of S.spgemm_shape().  Also
the shapes the GPU tests run (tests/test_gpu_spgemm.py), so that the CPU test
(tests/test_spgemm.py) can hold them to what they are for.

A matrix is the tuple (M, N, IRP, JA, AS) of tests/_transpose.py."""
import functools

import numpy as np

import _cg as G
import _transpose as TR

irp_of = TR.irp_of


def reference(A, B):
    """-> (IRP_C, JA_C, AS_C).  The walk is expanded product by product (for
    row r: A's entries p in stored order, for each the entries q of B's row
    JA_A[p] in stored order), sorted stably by (row, column) -- which keeps
    the walk order inside a column -- and summed sequentially: the first
    product of a column initialises its sum, every further one is ONE rounded
    addition"""
    M, K, IA, JA, VA = A
    K2, N, IB, JB, VB = B
    assert K == K2
    IA, IB = np.asarray(IA, np.int64), np.asarray(IB, np.int64)
    JA, JB = np.asarray(JA, np.int64), np.asarray(JB, np.int64)
    VA, VB = np.asarray(VA, np.float64), np.asarray(VB, np.float64)
    rows_a = np.repeat(np.arange(M, dtype=np.int64), np.diff(IA))
    per_p = np.diff(IB)[JA] if len(JA) else np.zeros(0, np.int64)
    P = int(per_p.sum())
    p_of = np.repeat(np.arange(len(JA), dtype=np.int64), per_p)
    first_of_p = np.cumsum(per_p) - per_p
    q_of = IB[JA][p_of] + (np.arange(P, dtype=np.int64) - first_of_p[p_of])
    row, col = rows_a[p_of], JB[q_of]
    with np.errstate(all="ignore"):
        t = VA[p_of] * VB[q_of]
    order = np.lexsort((np.arange(P), col, row))  # (row, column, walk index)
    row, col, t = row[order], col[order], t[order]
    new = np.ones(P, bool)
    new[1:] = (row[1:] != row[:-1]) | (col[1:] != col[:-1])
    starts = np.flatnonzero(new)
    lens = np.diff(np.append(starts, P))
    s = t[starts].copy()
    with np.errstate(all="ignore"):
        for j in range(1, int(lens.max()) if len(lens) else 0):
            sel = lens > j
            s[sel] = s[sel] + t[starts[sel] + j]
    IRP_C = np.concatenate(
        [[0], np.cumsum(np.bincount(row[starts], minlength=M))])
    return IRP_C.astype(np.int32), col[starts].astype(np.int32), s


def upper_bounds(A, B):
    """ub[r] = sum over the entries (r, k) of A of len(row k of B), int64"""
    M, K, IA, JA, _ = A
    per_p = np.diff(np.asarray(B[2], np.int64))[np.asarray(JA, np.int64)] \
        if len(JA) else np.zeros(0, np.int64)
    rows = np.repeat(np.arange(M), np.diff(np.asarray(IA, np.int64)))
    return np.bincount(rows, weights=per_p, minlength=M).astype(np.int64)


def model(A, B, shape):
    """the size class of every row: the first class whose edge holds its ub,
    len(edges) (the fallback) beyond the last"""
    return np.searchsorted(np.asarray(shape["edges"], np.int64),
                           upper_bounds(A, B), side="left")


def rows_in_bin(A, B, shape):
    return tuple(np.bincount(model(A, B, shape),
                             minlength=len(shape["edges"]) + 1).tolist())


def transpose(A):
    M, N, IRP, JA, AS = A
    return (N, M) + TR.reference(IRP, JA, AS, N)


def identity(n):
    return (n, n, irp_of(np.ones(n, np.int64)), np.arange(n, dtype=np.int32),
            np.ones(n))


def dense(A):
    M, N, IRP, JA, AS = A
    D = np.zeros((M, N))
    rows = np.repeat(np.arange(M), np.diff(IRP))
    np.add.at(D, (rows, JA), AS)
    return D


def from_rows(N, rows, vals=None, rng=None):
    """rows: a list of column lists -> matrix with random values"""
    lens = [len(r) for r in rows]
    JA = np.array([c for r in rows for c in r], np.int32)
    if vals is None:
        vals = rng.uniform(-2, 2, len(JA))
    return len(rows), N, irp_of(lens), JA, np.asarray(vals, np.float64)


def random_sorted(M, N, per_row, seed, empty_every=0):
    """M x N, strictly ascending rows of up to per_row entries"""
    rng = np.random.default_rng(seed)
    rows = []
    for r in range(M):
        n = int(rng.integers(0, min(per_row, N) + 1))
        if empty_every and r % empty_every == 0:
            n = 0
        rows.append(np.sort(rng.choice(N, n, replace=False)).tolist())
    return from_rows(N, rows, rng=rng)


def random_unsorted(M, N, per_row, seed):
    """M x N, rows in random order with duplicates and explicit zeros"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, per_row + 1, M)
    JA = rng.integers(0, N, lens.sum()).astype(np.int32)
    AS = rng.uniform(-2, 2, lens.sum())
    AS[rng.integers(0, max(len(AS), 1), len(AS) // 10)] = 0.0
    return M, N, irp_of(lens), JA, AS


# ------------------------------------------------------------ class edges
BLOCKS = [1000] * 4 + [500, 250, 125, 64, 32, 16, 8, 4, 2, 1]


def block_b(seed=11):
    """B for rows of a chosen ub: row 0 holds ONE entry (column 5); rows
    1..len(BLOCKS) hold blocks of BLOCKS[j] consecutive columns, all disjoint
    (from column 10 on); the last row is empty"""
    rng = np.random.default_rng(seed)
    rows, at = [[5]], 10
    for n in BLOCKS:
        rows.append(list(range(at, at + n)))
        at += n
    rows.append([])
    return from_rows(at, rows, rng=rng)


def blocks_for(ub):
    """rows of block_b() whose lengths sum to ub (greedy; ub <= 5002)"""
    out = []
    for j, n in enumerate(BLOCKS):
        if n <= ub:
            out.append(j + 1)
            ub -= n
    assert ub == 0
    return out


def class_edges(shape, seed=12):
    """(A, B, what): for every class edge e, rows with ub = e - 1, e, e + 1,
    each once with all columns distinct (nnz = ub, A's entries shuffled) and
    once with all products on one column (nnz = 1: ub copies of (r, 0));
    between them empty rows and rows that point at B's empty row only.
    what[r] = (ub, nnz) of row r"""
    rng = np.random.default_rng(seed)
    B = block_b()
    empty = B[0] - 1
    rows, what = [], []
    for e in shape["edges"]:
        for ub in (e - 1, e, e + 1):
            rows.append(rng.permutation(blocks_for(ub)).tolist())
            what.append((ub, ub))
            rows.append([0] * ub)
            what.append((ub, 1))
            rows.append([] if len(rows) % 4 else [empty, empty])
            what.append((0, 0))
    return from_rows(B[0], rows, rng=rng), B, what


# ------------------------------------------------- one row in every class
PAD_COL = 7000


def padded(shape, seed=13):
    """(A, B, pads): the SAME logical row -- entries in a fixed shuffled order
    with duplicates, one column of which collects [2^53, 1, 1, -2^53] -- stored
    len(pads) times, copy i with pads[i] more entries (spread through the row)
    that point at a B row holding only PAD_COL: ub grows, nothing else
    changes, and the copies land in every class in turn"""
    rng = np.random.default_rng(seed)
    b_rows = [sorted(rng.choice(6000, 2, replace=False).tolist())
              for _ in range(5)]
    b_rows += [[6500], [PAD_COL]]  # row 5: the order column, row 6: padding
    B = from_rows(PAD_COL + 1, b_rows, rng=rng)
    B[4][B[2][5]] = 1.0
    base_cols = [0, 5, 3, 1, 5, 0, 2, 5, 4, 5, 1]
    base_vals = rng.uniform(-2, 2, len(base_cols))
    base_vals[[1, 4, 7, 9]] = [2.0 ** 53, 1.0, 1.0, -2.0 ** 53]
    edges = shape["edges"]
    pads = [0, edges[0], edges[1], edges[2]]
    rows, vals = [], []
    for n in pads:
        cols, v = list(base_cols), list(base_vals)
        for at in sorted(rng.integers(0, len(cols) + 1, n).tolist(),
                         reverse=True):
            cols.insert(at, 6)
            v.insert(at, rng.uniform(-2, 2))
        rows.append(cols)
        vals += v
    return from_rows(7, rows, vals), B, pads


# -------------------------------------------------------- hash collisions
def collisions(shape):
    """(A, B): row c of B holds edges[c] columns that are ALL congruent
    modulo tables[c] (3 + tables[c] * i): every key of the row has the same
    home slot, and the row fills its table to ub exactly.  Row c of A is the
    one entry (c, c)"""
    rng = np.random.default_rng(14)
    rows = [(3 + t * np.arange(e, dtype=np.int64)).tolist()
            for e, t in zip(shape["edges"], shape["tables"])]
    N = max(r[-1] for r in rows) + 1
    B = from_rows(N, rows, rng=rng)
    A = from_rows(len(rows), [[c] for c in range(len(rows))], rng=rng)
    return A, B


# ------------------------------------------------------------------ order
def sums3(v):
    """sequential, reversed and pairwise sum of four numbers"""
    seq = ((v[0] + v[1]) + v[2]) + v[3]
    rev = ((v[3] + v[2]) + v[1]) + v[0]
    pair = (v[0] + v[1]) + (v[2] + v[3])
    return seq, rev, pair


def order():
    """(A, B): every row of A stores a permutation of {2^53, 1, 1, -2^53} *
    2^e for which the sequential, the reversed and the pairwise sum are three
    different numbers; B is K x 1, all ones, so C[r, 0] is the sum of row r in
    whatever order the product adds"""
    import itertools
    base = [2.0 ** 53, 1.0, 1.0, -2.0 ** 53]
    perms = sorted(set(itertools.permutations(base)))
    rows, vals = [], []
    rng = np.random.default_rng(15)
    for e in (-60, 0, 1, 400):
        for p in perms:
            v = [x * 2.0 ** e for x in p]
            if len(set(sums3(v))) == 3:
                rows.append(rng.permutation(4).tolist())
                vals += v
    A = from_rows(4, rows, vals)
    B = (4, 1, irp_of([1] * 4), np.zeros(4, np.int32), np.ones(4))
    return A, B


# -------------------------------------------------------------- structure
def structure():
    """name -> (A, B)"""
    rng = np.random.default_rng(16)
    out = {}
    out["duplicates"] = (TR.duplicates(), random_sorted(6, 40, 7, 17))
    Bh = from_rows(9, [[], [1, 4], [], [0, 8], []], rng=rng)
    out["only empty rows of B"] = (
        from_rows(5, [[0, 2], [4], [], [2, 2, 0]], rng=rng), Bh)
    out["empty rows"] = (random_sorted(30, 12, 3, 18, empty_every=3),
                         random_sorted(12, 25, 4, 19, empty_every=2))
    e = np.zeros(0, np.int32), np.zeros(0)
    out["0 x K"] = ((0, 6, irp_of([])) + e, random_sorted(6, 9, 3, 20))
    out["M x 0"] = (random_sorted(7, 6, 3, 21), (6, 0, irp_of([0] * 6)) + e)
    out["K = 0"] = ((5, 0, irp_of([0] * 5)) + e, (0, 8, irp_of([])) + e)
    out["A empty"] = ((5, 6, irp_of([0] * 5)) + e, random_sorted(6, 9, 3, 22))
    out["B empty"] = (random_sorted(7, 6, 3, 23), (6, 9, irp_of([0] * 6)) + e)
    out["1 x 1"] = ((1, 1, irp_of([1]), np.zeros(1, np.int32),
                     np.array([2.5])),
                    (1, 1, irp_of([1]), np.zeros(1, np.int32),
                     np.array([-3.0])))
    return out


WIDE_N = 2 ** 24 + 1


def wide_n(rows=10, seed=24):
    """(A, B): N = 2^24 + 1.  B: a few short rows that reach the last column,
    and one row of 5000 entries spread over all of [0, N).  A: `rows` rows
    that hold the long row (the fallback: each allocates N doubles, so there
    are few of them -- but more than one batch) and a few short ones"""
    rng = np.random.default_rng(seed)
    long_row = np.unique(np.concatenate(
        [rng.integers(0, WIDE_N, 5000), [0, 31, 32, WIDE_N - 1]])).tolist()
    b_rows = [[0, WIDE_N - 1], [65535, 65536, 2 ** 24], [], long_row]
    B = from_rows(WIDE_N, b_rows, rng=rng)
    a_rows = [[3, 0], [1, 0]] + [[3] + rng.integers(0, 3, 2).tolist()
                                 for _ in range(rows - 1)] + [[2], [1]]
    return from_rows(4, a_rows, rng=rng), B


# --------------------------------------------------------- special values
def special():
    """(A, B): 8 x 6 times 6 x 5.
    C[0, 0] = 3 * 2 + (-6) * 1: cancellation stores +0.0
    C[1, 1] = (-0.0) * 1 alone: -0.0 keeps its sign
    C[2, 2] = inf * 0: a NaN there, C[2, 3] = inf * 2 = inf
    row 3 meets B's NaN (at (4, 1)) through column 4 only: C[3, 1] is NaN,
    C[3, 0] is not; row 4 does not meet it at all
    row 5: subnormal products, 2^-1060 * 2^-10 and the sum of two of them
    row 6: (-0.0) * 2 + 0.0 * 1 = +0.0 (two products of one column)
    row 7: an explicit zero of A: 0.0 * 2 stores +0.0"""
    inf, nan = np.inf, np.nan
    A = from_rows(6, [[0, 1], [2], [3], [4, 0], [0, 1], [5, 5], [0, 1], [0]],
                  [3.0, -6.0, -0.0, inf, 1.5, 2.5, 1.0, 1.0, 2.0 ** -10,
                   2.0 ** -10, -0.0, 0.0, 0.0])
    B = from_rows(5, [[0], [0], [1], [2, 3], [1], [4]],
                  [2.0, 1.0, 1.0, 0.0, 2.0, nan, 2.0 ** -1060])
    return A, B


# ---------------------------------------------------------------- fallback
def dedup(A):
    """drop the later copies of a stored (row, column)"""
    M, N, IRP, JA, AS = A
    rows = np.repeat(np.arange(M, dtype=np.int64), np.diff(IRP))
    _, keep = np.unique(rows * N + JA, return_index=True)
    keep = np.sort(keep)
    return (M, N, irp_of(np.bincount(rows[keep], minlength=M)), JA[keep],
            AS[keep])


def hublike(M=3000, seed=25):
    """the shape of tests/golden/hub96.mtx, larger: three random entries a
    row, a hub ROW (41) of 2000 entries and a hub COLUMN (8) in every sixth
    row, in random order, no duplicates.  In A A^T the hub row meets about
    2000 * 3.5 products (the fallback), the rows of the hub column M / 6 each"""
    rng = np.random.default_rng(seed)
    rows = []
    for r in range(M):
        n = 2000 if r == 41 else 3
        c = rng.choice(M, n, replace=False).tolist()
        if r % 6 == 0 and 8 not in c:
            c[int(rng.integers(0, n))] = 8
        rows.append(c)
    return from_rows(M, rows, rng=rng)


def hub_cut(rows=4200, take=40):
    """(A, B): B = H^T of H = hub() of tests/_transpose.py cut to `rows` rows
    (duplicates dropped), whose row 7 holds every row of H; A = the first
    `take` rows of H, each of which holds column 7: `take` rows of H H^T"""
    M, N, IRP, JA, AS = TR.hub(M=rows)
    H = dedup((M, N, IRP, JA, AS))
    e = int(H[2][take])
    return (take, N, H[2][:take + 1], H[3][:e], H[4][:e]), transpose(H)


# ---------------------------------------------------------------- galerkin
def aggregates(nx, ny, bx=2, by=2):
    """P: (nx ny) x (nx ny / (bx by)), one 1.0 per row at the row's aggregate"""
    j, i = np.divmod(np.arange(nx * ny), nx)
    agg = (j // by) * (nx // bx) + i // bx
    n = (nx // bx) * (ny // by)
    return (nx * ny, n, irp_of(np.ones(nx * ny, np.int64)),
            agg.astype(np.int32), np.ones(nx * ny))


def galerkin_case(n=64):
    """(A, P): the five-point stencil on n^2 and 2 x 2 aggregates"""
    M, IRP, JA, AS = G.lap2d(n, n, 0.0)
    return (M, M, IRP, JA, AS), aggregates(n, n)


def galerkin_reference(A, P):
    return reference(transpose(P), (A[0], P[1]) + reference(A, P))


# ---------------------------------------------------------------- overflow
OVERFLOW_N = 46341  # 46341^2 = 2 147 488 281 > INT32_MAX


def overflow_case():
    n = OVERFLOW_N
    A = (n, 1, irp_of(np.ones(n, np.int64)), np.zeros(n, np.int32),
         np.ones(n))
    B = (1, n, irp_of([n]), np.arange(n, dtype=np.int32), np.ones(n))
    return A, B


@functools.lru_cache(maxsize=None)
def cached_reference(name):
    """reference of a named heavy case, computed once a process"""
    A, B = CASES[name]()
    return A, B, reference(A, B)


CASES = {
    "hublike": lambda: (lambda H: (H, transpose(H)))(hublike()),
    "hub cut": hub_cut,
    "wide n": wide_n,
}
