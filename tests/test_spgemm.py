"""The sparse product's contract and test shapes on the CPU
(tests/_spgemm.py; the device side: tests/test_gpu_spgemm.py): the numpy
reference against dense integer arithmetic, the shapes held to what they are
for, the identities of the contract, and the symbols of the C ABI."""
import numpy as np

import _spgemm as SG
import _transpose as TR
import spmv_scpa_amd as S

SHAPE = S.spgemm_shape()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same(got, want):
    return (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            and np.array_equal(bits(got[2]), bits(want[2])))


def integer_valued(mat, seed):
    rng = np.random.default_rng(seed)
    return mat[:4] + (rng.integers(-9, 10, len(mat[4])).astype(np.float64),)


def test_symbols_and_shape():
    assert S.check_symbols()
    for name in ("spmv_csr_spgemm", "spmv_spgemm_shape", "spmv_csr_galerkin"):
        assert name in S.declared_symbols()
    edges, tables = SHAPE["edges"], SHAPE["tables"]
    assert len(edges) == len(tables) == len(SHAPE["teams"]) == 3
    assert edges == sorted(set(edges))
    # a table is strictly larger than any ub it serves, a power of two
    assert all(t > e and t & (t - 1) == 0 for e, t in zip(edges, tables))
    assert max(SHAPE["lds_bytes"]) <= 160 * 1024 - 256
    assert SHAPE["fallback_batch"] >= 1 and SHAPE["fallback_bytes"] > 0


def test_reference_equals_dense_integer_products():
    cases = [(SG.random_unsorted(13, 9, 6, 1), SG.random_sorted(9, 11, 5, 2)),
             (SG.random_unsorted(40, 30, 12, 3),
              SG.random_sorted(30, 7, 7, 4, empty_every=4)),
             SG.structure()["duplicates"], SG.structure()["empty rows"]]
    for k, (A, B) in enumerate(cases):
        A, B = integer_valued(A, 10 + k), integer_valued(B, 20 + k)
        I, J, V = SG.reference(A, B)
        want = SG.dense(A) @ SG.dense(B)
        got = SG.dense((A[0], B[1], I, J, V))
        assert np.array_equal(got, want)  # small integers: exact in any order
        rows = np.repeat(np.arange(A[0]), np.diff(I))
        # every column once, ascending; an entry wherever a product exists
        assert np.all((np.diff(J) > 0) | (np.diff(rows) > 0))
        pattern = (np.abs(SG.dense(A[:4] + (np.ones(len(A[4])),)))
                   @ np.abs(SG.dense(B[:4] + (np.ones(len(B[4])),)))) > 0
        assert np.array_equal(SG.dense((A[0], B[1], I, J, np.ones(len(J)))) > 0,
                              pattern)


def test_class_edges_sit_at_their_edges():
    A, B, what = SG.class_edges(SHAPE)
    assert 25 <= A[0] <= 45
    ub = SG.upper_bounds(A, B)
    assert ub.tolist() == [w[0] for w in what]
    C = SG.reference(A, B)
    assert np.diff(C[0]).tolist() == [w[1] for w in what]
    cls = SG.model(A, B, SHAPE)
    for c, e in enumerate(SHAPE["edges"]):
        for u, want in ((e - 1, c), (e, c), (e + 1, c + 1)):
            hit = cls[ub == u]
            assert len(hit) == 2 and np.all(hit == want)
    assert all(n > 0 for n in SG.rows_in_bin(A, B, SHAPE))


def test_padded_rows_land_in_every_class():
    A, B, pads = SG.padded(SHAPE)
    assert SG.model(A, B, SHAPE).tolist() == [0, 1, 2, 3]
    I, J, V = SG.reference(A, B)
    real = [(J[I[r]:I[r + 1]], V[I[r]:I[r + 1]]) for r in range(4)]
    keep = [j != SG.PAD_COL for j, _ in real]
    assert [int((~k).sum()) for k in keep] == [0, 1, 1, 1]
    for r in range(1, 4):
        assert np.array_equal(real[r][0][keep[r]], real[0][0])
        assert np.array_equal(bits(real[r][1][keep[r]]), bits(real[0][1]))
    # the order column holds the sequential sum of [2^53, 1, 1, -2^53]
    assert real[0][1][real[0][0] == 6500].tolist() == [0.0]


def test_collision_rows_share_one_home_slot_and_fill_to_ub():
    A, B = SG.collisions(SHAPE)
    assert SG.upper_bounds(A, B).tolist() == SHAPE["edges"]
    assert SG.model(A, B, SHAPE).tolist() == [0, 1, 2]
    for c, t in enumerate(SHAPE["tables"]):
        cols = B[3][B[2][c]:B[2][c + 1]]
        assert len(np.unique(cols % t)) == 1 and len(cols) == SHAPE["edges"][c]
    assert np.diff(SG.reference(A, B)[0]).tolist() == SHAPE["edges"]


def test_the_three_orders_differ_in_every_row():
    A, B = SG.order()
    M = A[0]
    assert M >= 8 and np.all(np.diff(A[2]) == 4)
    seqs = []
    for r in range(M):
        v = A[4][4 * r:4 * r + 4]
        assert sorted(np.abs(v / np.abs(v).min())) == [1, 1, 2.0 ** 53,
                                                       2.0 ** 53]
        seq, rev, pair = SG.sums3(v)
        assert len({seq, rev, pair}) == 3
        seqs.append(seq)
    I, J, V = SG.reference(A, B)
    assert np.array_equal(bits(V), bits(np.array(seqs))) and not J.any()
    # the first row is the permutation of the contract: 0, 2 and 1
    first = [2.0 ** 53, 1.0, 1.0, -2.0 ** 53]
    assert SG.sums3(first) == (0.0, 2.0, 1.0)


def test_structure_and_special_values():
    st = SG.structure()
    for name, (A, B) in st.items():
        I, J, V = SG.reference(A, B)
        assert len(I) == A[0] + 1 and I[-1] == len(J) == len(V), name
    assert SG.reference(*st["only empty rows of B"])[0][-1] == 0
    A, B = st["duplicates"]
    assert len(A[3]) > len(np.unique(
        np.repeat(np.arange(A[0]), np.diff(A[2])) * A[1] + A[3]))
    A, B = SG.special()
    I, J, V = SG.reference(A, B)

    def at(r, c):
        k = np.flatnonzero(J[I[r]:I[r + 1]] == c)
        assert len(k) == 1
        return V[I[r] + k[0]]

    neg0 = 0x8000_0000_0000_0000
    assert bits(at(0, 0)) == 0 and bits(at(1, 1)) == neg0
    assert np.isnan(at(2, 2)) and at(2, 3) == np.inf
    assert np.isnan(at(3, 1)) and at(3, 0) == 5.0
    assert np.count_nonzero(np.isnan(V)) == 2
    assert at(5, 4) == 2.0 ** -1069 and bits(at(6, 0)) == 0
    assert bits(at(7, 0)) == 0


def test_identities_hold_for_the_reference():
    A = SG.random_unsorted(50, 40, 8, 30)
    A = SG.dedup(A)
    A[4][::7] = np.inf
    A[4][3::11] = -np.inf
    M, K = A[0], A[1]
    assert same(SG.reference(A, SG.identity(K)), TR.row_sorted(*A[2:]))
    B = SG.random_sorted(40, 33, 6, 31)
    assert same(SG.reference(SG.identity(40), B), B[2:])
    # (A B)^T == B^T A^T when A's rows are strictly ascending
    As = SG.random_sorted(50, 40, 8, 32)
    AB = (50, 33) + SG.reference(As, B)
    assert same(SG.transpose(AB)[2:],
                SG.reference(SG.transpose(B), SG.transpose(As)))
    sq = SG.random_sorted(40, 40, 6, 33)
    assert SG.reference(sq, sq)[0][-1] > 0


def test_fallback_and_galerkin_shapes():
    A, B, C = SG.cached_reference("hublike")
    bins = SG.rows_in_bin(A, B, SHAPE)
    assert all(n > 0 for n in bins) and SG.model(A, B, SHAPE)[41] == 3
    A, B, C = SG.cached_reference("hub cut")
    assert SG.rows_in_bin(A, B, SHAPE) == (0, 0, 0, A[0])
    A, B, C = SG.cached_reference("wide n")
    assert B[1] == 2 ** 24 + 1 and C[1].max() == 2 ** 24
    assert SG.rows_in_bin(A, B, SHAPE)[3] == 10
    A, P = SG.galerkin_case()
    I, J, V = SG.galerkin_reference(A, P)
    assert len(J) == 4992 and np.diff(I).max() == 5
    assert V[:3].tolist() == [8.0, -2.0, -2.0] and J[:3].tolist() == [0, 1, 32]
    A, B = SG.overflow_case()
    assert int(SG.upper_bounds(A, B).sum()) == 46341 ** 2 > 2 ** 31 - 1
