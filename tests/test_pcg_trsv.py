"""Conjugate gradients preconditioned by triangular plans (spmv_*_pcg_trsv;
spmv_engine.h): what can be checked without a GPU -- the declared surface, the
binding's argument checks, the answers without a device, and the numpy
restatement of tests/_pcg_trsv.py with the CPU oracle's product: its iteration
counts, its true residual, and the two properties of the contract (an identity
plan is cg, a power-of-two diagonal plan is pcg).  The device:
tests/test_gpu_pcg_trsv.py."""
import ctypes as C
import errno

import numpy as np
import pytest

import _cg as G
import _oracle as O
import _pcg as PG
import _pcg_trsv as PT
import _trsv as TV
import spmv_scpa_amd as S

GROUP = S.trsv_shape()["group"]
NEW = ["spmv_csr_pcg_trsv", "spmv_hll_pcg_trsv", "spmv_pcg_trsv_work_bytes"]
TOL = 1e-8


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def test_the_headers_declare_the_entry_points():
    declared = S.declared_symbols()
    for name in NEW:
        assert name in declared and hasattr(S._lib, name), name
    assert S.check_symbols()
    assert S.version() == "spmv_scpa_amd 0.7 gfx950"
    for cls in (S.CsrDevice, S.HllDevice):
        assert callable(cls.pcg_trsv)
    for name in ("args", "release"):
        assert hasattr(S.SgsPreconditioner, name), name


def test_the_work_buffer_is_pcg_s_and_one_vector():
    for M, k in ((0, 1), (1, 1), (1073, 3), (10 ** 7, 8)):
        assert S.pcg_trsv_work_bytes(M, k) == \
            S.pcg_work_bytes(M, k) + 8 * M * k
    for M, k in ((-1, 1), (5, 0), (5, 9)):
        with pytest.raises(OSError) as ei:
            S.pcg_trsv_work_bytes(M, k)
        assert ei.value.errno == errno.EINVAL


def fake_plan():
    plan = object.__new__(S.TrsvPlan)
    plan.h = None
    return plan


@pytest.mark.parametrize("cls", [S.CsrDevice, S.HllDevice])
def test_the_binding_checks_its_arguments(cls):
    fake = object.__new__(cls)  # a wrapper around no handle
    fake.h = None
    plan = fake_plan()
    for kw in (dict(k=0), dict(k=9), dict(k=3, ldb=2), dict(k=3, ldx=2)):
        with pytest.raises(ValueError):
            fake.pcg_trsv(1, 2, plan, **kw)
    with pytest.raises(ValueError):
        fake.pcg_trsv(1, 2, None)              # no first plan
    with pytest.raises(ValueError):
        fake.pcg_trsv(1, 2, plan, second=5)    # not a plan
    with pytest.raises(ValueError):
        fake.pcg_trsv(1, 2, plan, d_scale=8)   # a scale and no second plan
    with pytest.raises(OSError) as ei:
        fake.pcg_trsv(1, 2, plan, plan, 8, k=3, ldb=3, ldx=5)
    assert ei.value.errno == errno.EINVAL  # the library's answer to NULL


@pytest.mark.parametrize("fmt", ["csr", "hll"])
def test_dead_handles_and_argument_errors_of_the_library(fmt):
    fn = getattr(S._lib, "spmv_%s_pcg_trsv" % fmt)
    pj = C.cast(C.create_string_buffer(512), C.c_void_p)
    dead = -errno.EBADF if S.device_count() > 0 else -errno.ENODEV
    o, info = S._opts(), (S.CgInfo * 1)()
    args = (C.byref(o), 1, 8, 0, 8, 0, pj, None, None, 1e-8, 10, 0, None, 0,
            info, None)
    assert fn(None, *args) == -errno.EINVAL
    assert fn(pj, *args) == dead  # the matrix is checked before the plans


# ------------------------------------------------------------ the restatement
@pytest.fixture(scope="module")
def scaled():
    """the scaled stencil, column 0 of the common inputs, the oracle's product,
    and the Jacobi solve every preconditioner is held against"""
    mat = PG.scaled_lap2d(37, 29, 0.01, 3, 5)
    M, IRP, JA, AS = mat
    B, X0 = G.common_inputs(M, 2)
    B, X0 = B[:, :1].copy(), X0[:, :1].copy()
    product, residual0 = G.dense_product(IRP, JA, AS, O.csr_spmv)
    with np.errstate(divide="ignore"):
        jacobi = PG.restate(product, residual0(B, X0), B, X0,
                            1.0 / PG.diag_of(*mat), TOL, 1000)
    return mat, B, X0, product, residual0, jacobi


@pytest.mark.parametrize("which", ["sgs", "ic0"])
def test_the_preconditioners_halve_jacobi_s_iterations(scaled, which):
    mat, B, X0, product, residual0, jacobi = scaled
    M, IRP, JA, AS = mat
    pc = getattr(PT, which)(mat)
    got = PT.restate(product, residual0(B, X0), B, X0,
                     PT.plans_apply(*pc, GROUP), TOL, 1000)
    print(which, "iterations", got.iterations, "jacobi", jacobi.iterations)
    assert got.status.tolist() == [0] and jacobi.status.tolist() == [0]
    assert 2 * got.iterations[0] <= jacobi.iterations[0]
    res = G.true_residual(IRP, JA, AS, O.csr_spmv, B, got.X)
    print(which, "true residual", res)
    assert np.all(res <= 2 * TOL)
    # the level-wise solve is the row-wise reference, bit for bit
    slow = PT.restate(product, residual0(B, X0), B, X0,
                      PT.plans_apply(*pc, GROUP, solve=TV.reference_solve),
                      TOL, 5)
    fast = PT.restate(product, residual0(B, X0), B, X0,
                      PT.plans_apply(*pc, GROUP), TOL, 5)
    assert np.array_equal(bits(slow.X), bits(fast.X))
    assert np.array_equal(bits(slow.rr), bits(fast.rr))


def diagonal_plan(d):
    M = len(d)
    return TV.reference_plan(np.arange(M + 1, dtype=np.int32),
                             np.arange(M, dtype=np.int32),
                             np.asarray(d, np.float64), "lower")


def test_the_two_properties_of_the_contract(scaled):
    mat, _, _, product, residual0, _ = scaled
    M = mat[0]
    B, X0 = G.common_inputs(M, 4)
    # an identity plan, and a unit plan without strict entries: cg
    plain = G.restate(product, residual0(B, X0), B, X0, TOL, 60)
    for first in ((diagonal_plan(np.ones(M)), False),
                  (diagonal_plan(np.full(M, 7.0)), True)):
        got = PT.restate(product, residual0(B, X0), B, X0,
                         PT.plans_apply(first, None, None, GROUP), TOL, 60)
        for name in ("X", "rr", "bb", "status", "iterations"):
            assert np.array_equal(getattr(got, name), getattr(plain, name))
        assert np.array_equal(bits(got.X), bits(plain.X))
    # a diagonal of powers of two: pcg with minv = 1 / d
    d = 2.0 ** np.random.default_rng(3).integers(-6, 7, M)
    pre = PG.restate(product, residual0(B, X0), B, X0, 1.0 / d, TOL, 60)
    got = PT.restate(product, residual0(B, X0), B, X0,
                     PT.plans_apply((diagonal_plan(d), False), None, None,
                                    GROUP), TOL, 60)
    assert np.array_equal(bits(got.X), bits(pre.X))
    assert np.array_equal(bits(got.rr), bits(pre.rr))
    assert got.iterations.tolist() == pre.iterations.tolist()
    assert got.status.tolist() == pre.status.tolist()
