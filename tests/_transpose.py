"""Transposition of a CSR matrix as spmv_csr_transpose defines it
(include/spmv_engine.h): `reference`, the contract in four numpy lines, and
`model`, a numpy restatement of the device algorithm (transpose_kernels.hip)
that uses the numbers of the plan (S.transpose_plan): per-tile digit
histograms, a digit-major exclusive scan, the stable rank inside a tile,
composed over the passes.  Also the shapes the GPU tests run
(tests/test_gpu_transpose.py), so that the CPU test can check that the model
equals the reference on each of them and that they are what they are for."""
import numpy as np


def reference(IRP, JA, AS, N):
    """-> (IRP_T, JA_T, AS_T): the stable counting sort of the entries, in
    stored order, by column"""
    IRP = np.asarray(IRP, np.int64)
    JA = np.asarray(JA, np.int32)
    AS = np.asarray(AS)
    M = len(IRP) - 1
    rows = np.repeat(np.arange(M, dtype=np.int32), np.diff(IRP))
    order = np.argsort(JA, kind="stable")
    IRP_T = np.concatenate(
        [[0], np.cumsum(np.bincount(JA, minlength=N))]).astype(np.int32)
    return IRP_T, rows[order], AS[order]


def row_sorted(IRP, JA, AS):
    """the matrix with every row stably ordered by column: (A^T)^T"""
    IRP = np.asarray(IRP, np.int64)
    JA = np.asarray(JA, np.int32)
    M = len(IRP) - 1
    rows = np.repeat(np.arange(M, dtype=np.int64), np.diff(IRP))
    order = np.lexsort((np.arange(len(JA)), JA, rows))
    return IRP.astype(np.int32), JA[order], np.asarray(AS)[order]


def model_sort(JA, plan, stats=None):
    """the sorted positions as the device computes them: `passes` counting
    sorts on digits of `digit_bits` bits over tiles of `tile` keys.
    stats (a dict) receives what the shapes are chosen for"""
    keys = np.asarray(JA, np.int64)
    NZ = len(keys)
    pos = np.arange(NZ, dtype=np.int64)
    tile, bits, wgs = plan["tile"], plan["digit_bits"], plan["workgroups"]
    radix = 1 << bits
    assert wgs * tile >= NZ > (wgs - 1) * tile
    most_tiles = 0
    for p in range(plan["passes"]):
        digit = (keys >> (p * bits)) & (radix - 1)
        # 1. counter[digit][workgroup]
        hist = np.zeros((radix, wgs), np.int64)
        for w in range(wgs):
            hist[:, w] = np.bincount(digit[w * tile:(w + 1) * tile],
                                     minlength=radix)
        most_tiles = max(most_tiles, int((hist > 0).sum(axis=1).max())
                         if wgs else 0)
        # 2. exclusive scan over the flattened (digit-major) counters
        flat = hist.ravel()
        base = (np.cumsum(flat) - flat).reshape(radix, wgs)
        # 3. base[digit][workgroup] + stable rank inside the tile
        out_k, out_p = np.empty_like(keys), np.empty_like(pos)
        for w in range(wgs):
            d = digit[w * tile:(w + 1) * tile]
            order = np.argsort(d, kind="stable")
            rank = np.empty(len(d), np.int64)
            first = np.concatenate(
                [[0], np.cumsum(np.bincount(d, minlength=radix))])
            rank[order] = np.arange(len(d)) - first[d[order]]
            at = base[d, w] + rank
            out_k[at] = keys[w * tile:(w + 1) * tile]
            out_p[at] = pos[w * tile:(w + 1) * tile]
        keys, pos = out_k, out_p
    if stats is not None:
        stats.update(tiles=wgs, last_tile=NZ - (wgs - 1) * tile if wgs else 0,
                     passes=plan["passes"], bucket_tiles=most_tiles)
    return pos


def model(IRP, JA, AS, N, plan, stats=None):
    """-> (IRP_T, JA_T, AS_T) by the device algorithm"""
    IRP = np.asarray(IRP, np.int64)
    JA = np.asarray(JA, np.int32)
    pos = model_sort(JA, plan, stats)
    # the gather: the row that holds position p, by a search in IRP
    rows = (np.searchsorted(IRP, pos, side="right") - 1).astype(np.int32)
    IRP_T = np.concatenate(
        [[0], np.cumsum(np.bincount(JA, minlength=N))]).astype(np.int32)
    return IRP_T, rows, np.asarray(AS)[pos]


# ------------------------------------------------------------------ shapes
def irp_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def values(rng, n):
    """distinct-looking finite values: the position shows in the bits"""
    return rng.uniform(-1, 1, n) + np.arange(n)


def random_nz(NZ, N=300, M=41, seed=1):
    """NZ entries dealt to M rows at random, random columns below N"""
    rng = np.random.default_rng(seed + NZ)
    lens = np.bincount(rng.integers(0, M, NZ), minlength=M)
    JA = rng.integers(0, N, NZ).astype(np.int32)
    return M, N, irp_of(lens), JA, values(rng, NZ)


def digit_edges(N, M=50, nz=5000, seed=2):
    """about nz entries in M rows, the columns drawn at both ends of [0, N)
    and around every digit boundary below N"""
    rng = np.random.default_rng(seed + N)
    marks = {0, 1, N - 1, N - 2, N // 2}
    for b in (8, 16, 24):
        for k in (-2, -1, 0, 1):
            marks.add((1 << b) + k)
            marks.add(3 * (1 << b) + k)
    marks = np.array(sorted(c for c in marks if 0 <= c < N), np.int64)
    JA = np.concatenate([rng.choice(marks, nz - nz // 4),
                         rng.integers(0, N, nz // 4)]).astype(np.int32)
    rng.shuffle(JA)
    lens = np.bincount(rng.integers(0, M, len(JA)), minlength=M)
    return M, N, irp_of(lens), JA, values(rng, len(JA))


def hub(M=70000, N=1000, seed=3):
    """every row holds column 7 and two random others, in a random order"""
    rng = np.random.default_rng(seed)
    JA = rng.integers(0, N, (M, 3)).astype(np.int32)
    JA[np.arange(M), rng.integers(0, 3, M)] = 7
    return M, N, irp_of(np.full(M, 3)), JA.ravel(), values(rng, 3 * M)


def duplicates():
    """5 x 6, rows unsorted; (1, 4) stored three times with three values,
    (3, 0) twice; an explicit zero at (2, 2); row 4 empty"""
    lens = [3, 5, 2, 3, 0]
    JA = np.array([5, 0, 2, 4, 1, 4, 0, 4, 2, 3, 0, 5, 0], np.int32)
    AS = np.array([1.0, 2.0, 3.0, 10.0, 4.0, 20.0, 5.0, 30.0, 0.0, 6.0, 7.0,
                   8.0, 9.0])
    return 5, 6, irp_of(lens), JA, AS


def plain_shapes():
    """name -> (M, N, IRP, JA, AS): the empty and the thin ones"""
    rng = np.random.default_rng(4)
    out = {}
    out["0 x 5"] = (0, 5, irp_of([]), np.zeros(0, np.int32), np.zeros(0))
    out["7 x 9 empty"] = (7, 9, irp_of([0] * 7), np.zeros(0, np.int32),
                          np.zeros(0))
    out["1 x 1"] = (1, 1, irp_of([1]), np.zeros(1, np.int32), np.array([2.5]))
    c = np.sort(rng.choice(500, 77, replace=False)).astype(np.int32)
    out["1 x 500"] = (1, 500, irp_of([77]), c, values(rng, 77))
    lens = rng.integers(0, 2, 500)
    out["500 x 1"] = (500, 1, irp_of(lens), np.zeros(lens.sum(), np.int32),
                      values(rng, lens.sum()))
    for name, (M, N) in (("90 x 700", (90, 700)), ("700 x 90", (700, 90))):
        lens = rng.integers(0, 9, M)
        out[name] = (M, N, irp_of(lens),
                     rng.integers(0, N, lens.sum()).astype(np.int32),
                     values(rng, lens.sum()))
    return out


NZ_EDGES = lambda tile: [1, 63, 64, 65, tile - 1, tile, tile + 1,  # noqa: E731
                         3 * tile + 17]
N_EDGES = [1, 255, 256, 257, 65536, 65537, 2**24 + 1]


def gpu_shapes(tile):
    """every synthetic shape of the GPU tests: name -> (M, N, IRP, JA, AS)"""
    out = {}
    for nz in NZ_EDGES(tile):
        out["nz=%d" % nz] = random_nz(nz)
    for n in N_EDGES:
        out["n=%d" % n] = digit_edges(n)
    out["hub"] = hub()
    out["duplicates"] = duplicates()
    out.update(plain_shapes())
    return out
