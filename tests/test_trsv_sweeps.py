"""Sweep plans (spmv_csr_trsv_analyse_sweeps, spmv_trsv_sweeps; spmv_engine.h):
what can be checked without a GPU -- the declared surface, the binding's
argument checks, and the numpy restatement of tests/_trsv_sweeps.py: `levels`
sweeps are the exact solve to the bit, a NaN travels one dependency step per
sweep, and more sweeps of IC(0) buy fewer CG iterations.  The device:
tests/test_gpu_trsv_sweeps.py, tests/test_gpu_trsv_sweeps_solvers.py."""
import ctypes as C
import errno

import numpy as np
import pytest

import _cg as G
import _oracle as O
import _pcg as PG
import _pcg_trsv as PT
import _trsv as TV
import _trsv_sweeps as SW
import spmv_scpa_amd as S

GROUP, SMALL = (S.trsv_shape()[n] for n in ("group", "small_rows"))
NEW = ["spmv_csr_trsv_analyse_sweeps", "spmv_trsv_sweeps"]
TOL = 1e-8


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def cpu_shapes():
    """every non-empty shape of _trsv.shapes, the two large ones cut down for
    Python's sake"""
    out = TV.shapes(SMALL)
    del out["empty"]
    out["random"] = TV.random_triangle(600)
    out["arrow"] = TV.arrow(300)
    return out


SHAPES = cpu_shapes()


def rhs(M, k, seed=7):
    B = np.random.default_rng(seed).uniform(-1.0, 1.0, (M, k))
    if M:
        B[M // 2, 0] = -0.0
    return B


def test_the_headers_declare_the_entry_points():
    declared = S.declared_symbols()
    for name in NEW:
        assert name in declared and hasattr(S._lib, name), name
    assert S.check_symbols()
    for name in ("sweeps", "kmax"):
        assert isinstance(getattr(S.TrsvPlan, name), property), name


def test_the_binding_checks_its_arguments():
    fake = object.__new__(S.CsrDevice)  # a wrapper around no handle
    fake.h = None
    for kw in (dict(sweeps=-1), dict(sweeps=4097), dict(sweeps=3, kmax=0),
               dict(sweeps=3, kmax=9), dict(kmax=0), dict(kmax=9)):
        with pytest.raises(ValueError):
            fake.trsv_analyse("lower", **kw)
        with pytest.raises(ValueError):
            fake.sgs(**kw)
    with pytest.raises(OSError) as ei:
        fake.trsv_analyse("lower", sweeps=4096, kmax=8)
    assert ei.value.errno == errno.EINVAL  # the library's answer to NULL


def test_argument_errors_of_the_library():
    fn = S._lib.spmv_csr_trsv_analyse_sweeps
    pj = C.cast(C.create_string_buffer(512), C.c_void_p)
    out = C.c_void_p(5)
    dead = -errno.EBADF if S.device_count() > 0 else -errno.ENODEV
    assert fn(None, 0, 0, 3, 8, C.byref(out)) == -errno.EINVAL
    assert fn(pj, 0, 0, 3, 8, None) == -errno.EINVAL
    for uplo, unit, sweeps, kmax in ((2, 0, 3, 8), (0, -1, 3, 8), (0, 0, 0, 8),
                                     (0, 0, 4097, 8), (0, 0, 3, 0),
                                     (0, 0, 3, 9)):
        assert fn(pj, uplo, unit, sweeps, kmax, C.byref(out)) == -errno.EINVAL
    assert out.value == 5  # the numbers are refused before anything is written
    assert fn(pj, 1, 1, 4096, 1, C.byref(out)) == dead and not out.value
    s, k = C.c_int(7), C.c_int(7)
    assert S._lib.spmv_trsv_sweeps(None, C.byref(s), C.byref(k)) == \
        -errno.EINVAL
    assert S._lib.spmv_trsv_sweeps(pj, C.byref(s), C.byref(k)) == dead
    assert (s.value, k.value) == (7, 7)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_levels_sweeps_are_the_exact_solve(name):
    M, IRP, JA, AS = SHAPES[name]
    B = rhs(M, 2)
    scale = np.random.default_rng(5).uniform(0.5, 2.0, M)
    for uplo in ("lower", "upper"):
        plan = TV.reference_plan(IRP, JA, AS, uplo)
        levels = len(plan["level_ptr"]) - 1
        for unit, sc in ((False, None), (True, scale)):
            want = TV.reference_solve(plan, B, sc, GROUP, unit)
            got = SW.fast_sweeps(plan, B, sc, GROUP, levels, unit)
            assert np.array_equal(bits(got), bits(want)), (uplo, unit)
            if levels > 1:  # a row of level l is final after sweep l + 1
                short = SW.fast_sweeps(plan, B, sc, GROUP, levels - 1, unit)
                shallow = plan["order"][:plan["level_ptr"][levels - 1]]
                assert np.array_equal(bits(short[shallow]),
                                      bits(want[shallow]))


@pytest.mark.parametrize("name", ["lap2d", "sandwich", "random", "chain300"])
def test_the_fast_restatement_is_the_row_loop(name):
    M, IRP, JA, AS = SHAPES[name]
    B = rhs(M, 3)
    B[M // 3, 1] = np.nan
    scale = np.random.default_rng(5).uniform(0.5, 2.0, M)
    for uplo, unit, sc in (("lower", False, None), ("upper", True, scale)):
        plan = TV.reference_plan(IRP, JA, AS, uplo)
        for sweeps in (1, 2, 4):
            slow = SW.reference_sweeps(plan, B, sc, GROUP, sweeps, unit)
            fast = SW.fast_sweeps(plan, B, sc, GROUP, sweeps, unit)
            assert np.array_equal(bits(slow), bits(fast)), (uplo, sweeps)


@pytest.mark.parametrize("name", ["lap2d", "dominant"])
def test_a_nan_travels_one_dependency_step_per_sweep(name):
    # `random` has rows without a diagonal: their inf makes NaN of its own
    M, IRP, JA, AS = (TV.random_triangle(600, dominant=True)
                      if name == "dominant" else SHAPES[name])
    plan = TV.reference_plan(IRP, JA, AS, "lower")
    r = int(plan["order"][0])  # a row of level 0: everything may follow it
    B = rhs(M, 2)
    B[r, 1] = np.nan
    steps = SW.steps_from(plan, r)
    assert (steps >= 2).any()
    for sweeps in (1, 2, 3, 5):
        X = SW.fast_sweeps(plan, B, None, GROUP, sweeps)
        assert not np.isnan(X[:, 0]).any()
        assert np.array_equal(np.isnan(X[:, 1]),
                              (steps >= 0) & (steps < sweeps)), sweeps


def test_more_sweeps_of_ic0_buy_fewer_cg_iterations():
    mat = G.lap2d(24, 24, 0.01)
    M, IRP, JA, AS = mat
    B, X0 = G.common_inputs(M, 2)
    B, X0 = B[:, :1].copy(), X0[:, :1].copy()
    product, residual0 = G.dense_product(IRP, JA, AS, O.csr_spmv)
    with np.errstate(divide="ignore"):
        jacobi = PG.restate(product, residual0(B, X0), B, X0,
                            1.0 / PG.diag_of(*mat), TOL, 1000)
    first, second, scale = PT.ic0(mat)
    counts = [int(jacobi.iterations[0])]
    for sweeps in (2, 3):
        got = PT.restate(product, residual0(B, X0), B, X0,
                         SW.sweeps_apply(first, second, scale, GROUP, sweeps),
                         TOL, 1000)
        assert got.status.tolist() == [0], sweeps
        res = G.true_residual(IRP, JA, AS, O.csr_spmv, B, got.X)
        assert np.all(res <= 2 * TOL), (sweeps, res)
        counts.append(int(got.iterations[0]))
    exact = PT.restate(product, residual0(B, X0), B, X0,
                       PT.plans_apply(first, second, scale, GROUP), TOL, 1000)
    assert jacobi.status.tolist() == [0] and exact.status.tolist() == [0]
    counts.append(int(exact.iterations[0]))
    print("jacobi / IC(0) sweeps=2 / sweeps=3 / exact:", counts)
    assert counts[0] > counts[1] > counts[2] > counts[3], counts
