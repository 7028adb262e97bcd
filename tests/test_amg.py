"""Smoothed-aggregation AMG (spmv_csr_aggregate, spmv_csr_amg_setup,
spmv_amg_apply, spmv_*_pcg_amg; spmv_engine.h): what can be checked without a
GPU -- the declared surface, and the properties of the numpy restatement
(tests/_amg.py) with the CPU oracle's product: the aggregates partition the
rows, the roots are a maximal independent set of distance 2, P holds T and
keeps the row sums, the cycle is symmetric and positive, and the iteration
counts fall the way multigrid promises.  The device: tests/test_gpu_amg.py."""
import numpy as np
import pytest

import _amg as AM
import _cg as G
import _oracle as O
import _pcg as PG
import spmv_scpa_amd as S

NEW = ["spmv_csr_aggregate", "spmv_csr_amg_setup", "spmv_amg_info",
       "spmv_amg_level", "spmv_amg_last_phases", "spmv_amg_release",
       "spmv_amg_release_checked", "spmv_amg_apply", "spmv_csr_pcg_amg",
       "spmv_hll_pcg_amg"]
TOL = 1e-8
U = 2.0 ** -53


def test_the_headers_declare_the_entry_points():
    declared = S.declared_symbols()
    for name in NEW:
        assert name in declared and hasattr(S._lib, name), name
    assert S.check_symbols()
    assert S.version() == "spmv_scpa_amd 0.7 gfx950"
    for cls in ("Aggregation", "AmgHierarchy"):
        assert hasattr(S, cls)
    for method in ("aggregate", "amg", "pcg_amg"):
        assert hasattr(S.CsrDevice, method)
    assert hasattr(S.HllDevice, "pcg_amg")


def test_null_arguments_are_refused_before_anything_else():
    import ctypes as C
    import errno
    h = C.c_void_p(5)
    assert S._lib.spmv_csr_aggregate(None, 0.0, 0, 0, None, None) == \
        -errno.EINVAL
    assert S._lib.spmv_csr_amg_setup(None, 0.0, 1, 8, 32, 16, 0, 8,
                                     C.byref(h)) == -errno.EINVAL
    assert h.value is None
    assert S._lib.spmv_amg_info(None, None) == -errno.EINVAL
    assert S._lib.spmv_amg_apply(None, None, 1, None, 0, None, 0, None) == \
        -errno.EINVAL
    S._lib.spmv_amg_release(None)
    S._lib.spmv_amg_release_checked(None, 1)


# ---------------------------------------------------------------- aggregates
@pytest.mark.parametrize("name", list(AM.AGG))
def test_every_row_is_in_exactly_one_aggregate(name):
    for seed in (0, 1):
        mat, theta, ag = AM.reference(name, seed)
        M = mat[0]
        assert AM.well_formed(mat)
        assert ag.agg.shape == (M,)
        if M == 0:
            assert ag.aggregates == 0
            continue
        sizes = np.bincount(ag.agg, minlength=ag.aggregates)
        assert ag.agg.min() >= 0 and len(sizes) == ag.aggregates
        assert sizes.min() >= 1 and sizes.max() == ag.widest
        assert ag.aggregates == ag.roots + ag.singletons
        # the roots are numbered in row order, each in its own aggregate
        assert np.array_equal(ag.agg[ag.root_mask], np.arange(ag.roots))


def test_every_row_of_the_stencil_is_in_one_aggregate_of_a_root():
    mat, theta, ref = AM.reference("lap2d(40,40)", 0)
    assert ref.rounds > 3 and mat[0] > 4 * 256   # rounds, workgroups
    assert ref.singletons == 0 and ref.aggregates == ref.roots
    assert sorted(set(ref.agg.tolist())) == list(range(ref.aggregates))
    line = AM.reference("anisotropic(33,21)", 0)[2]
    # line aggregates: the weak direction is never strong at theta 0.25
    rows = np.arange(33 * 21) // 33
    for a in range(line.aggregates):
        assert len(set(rows[line.agg == a].tolist())) == 1


def strong_sets(mat, theta):
    er, ec, _, _ = AM.strong_edges(mat, theta)
    adj = [set() for _ in range(mat[0])]
    for r, c in zip(er.tolist(), ec.tolist()):
        adj[r].add(c)
    return adj


@pytest.mark.parametrize("name", ["lap2d(40,40)", "stencil27(8)",
                                  "arrow(600,3)", "anisotropic(33,21)"])
def test_the_roots_are_a_maximal_independent_set_of_distance_two(name):
    """on a symmetric strength graph"""
    mat, theta, ag = AM.reference(name, 0)
    adj = strong_sets(mat, theta)
    assert all(i in adj[j] for i in range(mat[0]) for j in adj[i])
    roots = set(np.flatnonzero(ag.root_mask).tolist())
    for i in range(mat[0]):
        within2 = set(adj[i])
        for j in adj[i]:
            within2 |= adj[j]
        within2.discard(i)
        if i in roots:   # more than distance 2 apart
            assert not (within2 & roots), i
        else:            # maximal: a root within distance 2
            assert within2 & roots, i


def test_a_nan_is_never_strong_and_a_zero_is_at_theta_zero():
    mat, theta, _ = AM.reference("zeros and a NaN", 0)
    M, IRP, JA, AS = mat
    er, ec, _, pos = AM.strong_edges(mat, theta)
    rows = AM.rows_of(M, IRP)
    off = rows != JA
    assert np.isnan(AS).sum() == 1 and (AS[off] == 0).sum() > 3
    assert set(pos.tolist()) == set(np.flatnonzero(off & ~np.isnan(AS)))


# ----------------------------------------------------------------- hierarchy
@pytest.fixture(scope="module")
def levels64():
    return AM.reference_hierarchy(64)


def test_the_levels_of_the_stencil(levels64):
    assert [l.A[0] for l in levels64] == [4096, 585, 38, 4]
    assert 1.2 < AM.complexity(levels64) < 1.4
    for l in levels64:
        assert AM.well_formed(l.A) and 1.0 < l.rho <= 2.0
        assert l.omega == (4.0 / 3.0) / l.rho


def test_p_holds_t_and_keeps_the_row_sums(levels64):
    for l in levels64[:-1]:
        M, IRP, JA, AS = l.A
        _, n, pi, pj, pv = l.P
        rows = AM.rows_of(M, pi)
        own = pj == l.agg.agg[rows]
        assert np.array_equal(np.bincount(rows[own], minlength=M),
                              np.ones(M, np.int64))      # T's pattern
        rs = np.add.reduceat(AS, IRP[:-1])
        S_abs = np.add.reduceat(np.abs(AS), IRP[:-1])
        got = np.add.reduceat(pv, pi[:-1])
        want = 1.0 - l.w * rs
        # a row of P sums the row of A: each of its len(row) products and
        # sums is rounded once, on terms of size w_i |a_ij| and 1
        bound = 4 * (np.diff(IRP) + 3) * U * (1.0 + np.abs(l.w) * S_abs)
        assert np.all(np.abs(got - want) <= bound)
        # PT is P transposed, entry for entry
        assert l.PT[0] == n and l.PT[1] == M
        assert sorted(zip(rows.tolist(), pj.tolist(), pv.tolist())) == sorted(
            zip(l.PT[3].tolist(), AM.rows_of(n, l.PT[2]).tolist(),
                l.PT[4].tolist()))


@pytest.mark.parametrize("sweeps", [1, 2])
def test_the_cycle_is_symmetric_and_positive(levels64, sweeps):
    M = levels64[0].A[0]
    V = AM.cycle(levels64, AM.oracle_products(levels64, O.csr_spmv), sweeps)
    rng = np.random.default_rng(11)
    W = rng.standard_normal((M, 20))
    VW = np.concatenate([V(W[:, :8]), V(W[:, 8:16]), V(W[:, 16:])], axis=1)
    for j in range(20):
        assert W[:, j] @ VW[:, j] > 0, j
    # symmetric to 1e-12 relative.  An inner product is only as accurate as
    # its terms are large: for vectors of mixed sign u . V(v) cancels (it is
    # ~0.1 where sum |u_i| |V(v)_i| is ~50), so "relative" is relative to
    # that sum; for positive vectors nothing cancels (V(v) is positive as
    # A^-1 v is) and it is relative to the value itself
    for i, j in ((0, 1), (2, 3), (4, 19), (7, 12)):
        a, b = W[:, i] @ VW[:, j], W[:, j] @ VW[:, i]
        scale = max(np.abs(W[:, i]) @ np.abs(VW[:, j]),
                    np.abs(W[:, j]) @ np.abs(VW[:, i]))
        print(sweeps, i, j, a, b, abs(a - b) / scale)
        assert abs(a - b) <= 1e-12 * scale, (i, j, a, b)
        # what the reference gives is 7e-17 at most: held to ten times that
        assert abs(a - b) <= 1e-15 * scale, (i, j, a, b)
    Pv = rng.uniform(0.5, 1.5, (M, 4))
    VP = V(Pv)
    assert np.all(VP > 0)
    for i, j in ((0, 1), (2, 3), (0, 3)):
        a, b = Pv[:, i] @ VP[:, j], Pv[:, j] @ VP[:, i]
        print(sweeps, "positive", i, j, a, b, abs(a - b) / max(a, b))
        assert abs(a - b) <= 1e-12 * max(a, b), (i, j, a, b)


# ---------------------------------------------------------- iteration counts
def solves(nx):
    mat = AM.lap2d(nx, nx)
    M, IRP, JA, AS = mat
    levels = AM.reference_hierarchy(nx)
    B = np.random.default_rng(5).uniform(-1, 1, (M, 1))
    X0 = np.zeros((M, 1))
    product, residual0 = G.dense_product(IRP, JA, AS, O.csr_spmv)
    V = AM.cycle(levels, AM.oracle_products(levels, O.csr_spmv))
    amg = AM.pcg_amg(product, residual0(B, X0), B, X0, V, TOL, 500)
    jac = PG.restate(product, residual0(B, X0), B, X0,
                     1.0 / PG.diag_of(*mat), TOL, 1000)
    assert amg.status[0] == 0 and jac.status[0] == 0
    res = G.true_residual(IRP, JA, AS, O.csr_spmv, B, amg.X)
    assert np.all(res <= 2 * TOL), res
    return int(amg.iterations[0]), int(jac.iterations[0])


def test_the_iteration_counts_fall_and_do_not_grow_with_the_mesh():
    amg32, jac32 = solves(32)
    amg64, jac64 = solves(64)
    print("5-point, diagonal 4.01, tol 1e-8: 32^2 amg %d jacobi %d; "
          "64^2 amg %d jacobi %d" % (amg32, jac32, amg64, jac64))
    assert 4 * amg64 <= jac64
    assert amg64 <= amg32 + 4
