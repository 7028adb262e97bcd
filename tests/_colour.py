"""The colouring and the permutation of a handle (spmv_csr_colour,
spmv_csr_permute; spmv_engine.h) restated in numpy, straight from the
definitions in the header, and the matrices their tests run.  No GPU here.

fmix32              the finaliser of murmur3 on uint32 arrays
reference_colour    the plain greedy loop: rows in decreasing priority, the
                    smallest colour no neighbour of higher priority has
reference_permute   two stable argsorts: by new column, then by new row
clique(n)           every row stores every column: n colours in n rounds
lower_bidiagonal(n) stores (i, i) and (i, i - 1) only: every edge is visible
                    from one side, so adjacency read from A alone is wrong

A matrix is (M, IRP, JA, AS) with int32 index arrays; a rectangular one is
given its column count on the side.
"""
import numpy as np

import _cg as G
import _ic0 as IC
import _trsv as TV


def fmix32(h):
    h = np.array(h, dtype=np.uint32)
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85ebca6b)   # wraps: 32-bit arithmetic
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xc2b2ae35)
    h ^= h >> np.uint32(16)
    return h


def priority(M, seed):
    with np.errstate(over="ignore"):
        return fmix32(np.arange(M, dtype=np.uint32) ^ np.uint32(seed))


def neighbours(M, IRP, JA):
    """list of sets: i ~ j iff i != j and (i, j) or (j, i) is stored"""
    adj = [set() for _ in range(M)]
    for i in range(M):
        for j in JA[IRP[i]:IRP[i + 1]].tolist():
            if j != i:
                adj[i].add(j)
                adj[j].add(i)
    return adj


def reference_colour(M, IRP, JA, seed, adjacency=neighbours):
    """-> (colour, round, new_of_old), int32 each"""
    h = priority(M, seed)
    adj = adjacency(M, IRP, JA)
    colour = np.full(M, -1, np.int32)
    rnd = np.zeros(M, np.int32)
    for i in np.argsort(h)[::-1].tolist():   # distinct: no tie to break
        higher = [j for j in adj[i] if h[j] > h[i]]
        taken = {int(colour[j]) for j in higher}
        c = 0
        while c in taken:
            c += 1
        colour[i] = c
        rnd[i] = 1 + max([int(rnd[j]) for j in higher], default=0)
    old_of_new = np.argsort(colour, kind="stable")
    new_of_old = np.empty(M, np.int32)
    new_of_old[old_of_new] = np.arange(M, dtype=np.int32)
    return colour, rnd, new_of_old


def one_sided(M, IRP, JA):
    """the WRONG adjacency: what row i stores, and nothing of A^T"""
    return [set(JA[IRP[i]:IRP[i + 1]].tolist()) - {i} for i in range(M)]


def reference_permute(mat, p=None, q=None, N=None):
    """-> (M, IRP, JA, AS) of P A Q^T; N: the columns of a rectangular mat"""
    M, IRP, JA, AS = mat
    N = M if N is None else N
    p = np.arange(M) if p is None else np.asarray(p)
    q = np.arange(N) if q is None else np.asarray(q)
    rows = np.repeat(np.arange(M), np.diff(IRP))
    first = np.argsort(q[JA], kind="stable")
    order = first[np.argsort(p[rows][first], kind="stable")]
    NIRP = np.zeros(M + 1, np.int32)
    NIRP[1:] = np.cumsum(np.bincount(p[rows], minlength=M))
    return (M, NIRP, np.ascontiguousarray(q[JA][order], np.int32),
            np.ascontiguousarray(AS[order]))   # moved: the bits, the dtype


def same_colour_edges(M, IRP, JA, colour):
    """stored off-diagonal entries that join two rows of one colour"""
    rows = np.repeat(np.arange(M), np.diff(IRP))
    return int(np.sum((rows != JA) & (colour[rows] == colour[JA])))


def max_degree(M, IRP, JA):
    return max([len(a) for a in neighbours(M, IRP, JA)], default=0)


# ------------------------------------------------------------------ matrices
def clique(n):
    return TV.from_rows([[(j, 1.0 + (i == j) * n) for j in range(n)]
                         for i in range(n)])


def lower_bidiagonal(n):
    return TV.from_rows([([(i - 1, -1.0)] if i else []) + [(i, 2.0)]
                         for i in range(n)])


def stencil27(n):
    """the 27-point stencil on an n^3 grid"""
    idx = np.arange(n ** 3).reshape(n, n, n)
    rows, cols = [], []

    def cut(d):     # the points that have a neighbour at offset d
        return slice(max(0, -d), n - max(0, d))

    def shift(d):   # those neighbours
        return slice(max(0, d), n + min(0, d))
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                rows.append(idx[cut(dz), cut(dy), cut(dx)].ravel())
                cols.append(idx[shift(dz), shift(dy), shift(dx)].ravel())
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    return G._csr(n ** 3, rows, cols, np.where(rows == cols, 26.5, -1.0))


def unsorted_duplicates(M=700):
    """tests/_trsv.py random_triangle: unsorted rows, duplicates, explicit
    zeros, rows without a diagonal, a pattern that is not symmetric"""
    return TV.random_triangle(M, seed=11)


#: the matrices of the issue
MATRICES = {
    "lap2d(37,29)": lambda: G.lap2d(37, 29, 0.01),
    "stencil27(7)": lambda: stencil27(7),
    "arrow(600,3)": lambda: G.arrow(600, 3),
    "layered": IC.layered_spd,
    "clique(70)": lambda: clique(70),
    "lower_bidiagonal(300)": lambda: lower_bidiagonal(300),
    "unsorted, duplicates, zeros": unsorted_duplicates,
}

#: no rows, one row, no edges
SMALL = {
    "M = 0": TV.empty,
    "M = 1": TV.single,
    "diagonal": TV.diagonal,
}

_cache = {}


def reference(name, seed):
    """(mat, colour, round, new_of_old) of a named matrix, computed once and
    shared: treat the arrays as read-only"""
    if (name, seed) not in _cache:
        mat = (MATRICES.get(name) or SMALL[name])()
        mat = (mat[0], mat[1].astype(np.int32), mat[2].astype(np.int32),
               mat[3])
        _cache[name, seed] = (mat,) + reference_colour(mat[0], mat[1], mat[2],
                                                       seed)
    return _cache[name, seed]
