"""Level-scheduled triangular solve (spmv_csr_trsv_analyse, spmv_trsv_solve;
spmv_engine.h): what can be checked without a GPU -- the declared surface, the
binding's argument checks, the answers without a device, the launch list's
arithmetic (also under AddressSanitizer + UBSan, as a stand-alone program over
trsv_plan.h), and the numpy reference of tests/_trsv.py against a dense
substitution on the shapes the GPU tests run.  The kernels themselves:
tests/test_gpu_trsv.py."""
import ctypes as C
import errno
import os
import subprocess
import sys

import numpy as np
import pytest

import _trsv as TV
import spmv_scpa_amd as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["spmv_csr_trsv_analyse", "spmv_trsv_info", "spmv_trsv_download",
       "spmv_trsv_shape", "spmv_trsv_release", "spmv_trsv_release_checked",
       "spmv_trsv_solve", "spmv_graph_end_capture_shape"]
SHAPE = S.trsv_shape()
L, GROUP = SHAPE["small_rows"], SHAPE["group"]


@pytest.fixture(scope="module")
def shapes():
    return TV.shapes(L)


def test_the_headers_declare_the_entry_points():
    declared = S.declared_symbols()
    for name in NEW:
        assert name in declared, name
        assert hasattr(S._lib, name), name
    assert S.check_symbols()
    # the feature is detected by the symbol, not by the version string
    assert S.version() == "spmv_scpa_amd 0.7 gfx950"
    assert callable(S.CsrDevice.trsv_analyse)
    for name in ("info", "download", "solve", "release"):
        assert hasattr(S.TrsvPlan, name), name


def test_the_shape_constants_are_powers_of_two():
    assert set(SHAPE) == {"group", "small_rows", "threads"}
    for name, v in SHAPE.items():
        assert v >= 2 and v & (v - 1) == 0, (name, v)
    assert GROUP <= 64  # inside a wavefront
    assert SHAPE["threads"] % GROUP == 0 and SHAPE["threads"] <= 1024
    # any out-pointer may be NULL
    S._lib.spmv_trsv_shape(None, None, None)


def test_the_binding_checks_its_arguments():
    fake = object.__new__(S.CsrDevice)  # a wrapper around no handle
    fake.h = None
    for kw in (dict(uplo="both"), dict(uplo=0), dict(max_levels=-1)):
        with pytest.raises(ValueError):
            fake.trsv_analyse(**kw)
    with pytest.raises(OSError) as ei:
        fake.trsv_analyse()
    assert ei.value.errno == errno.EINVAL
    plan = object.__new__(S.TrsvPlan)
    plan.h = None
    for kw in (dict(k=0), dict(k=9), dict(k=3, ldb=2), dict(k=3, ldx=2),
               dict(k=8, ldb=7, ldx=8)):
        with pytest.raises(ValueError):
            plan.solve(1, 2, **kw)
    with pytest.raises(OSError) as ei:
        plan.solve(1, 2, k=3, ldb=3, ldx=5)
    assert ei.value.errno == errno.EINVAL  # the library's answer to NULL
    plan.release()  # nothing to release: no call is made


def test_dead_handles_and_argument_errors_of_the_library():
    junk = C.create_string_buffer(512)  # never a handle of the library
    pj = C.cast(junk, C.c_void_p)
    dead = -errno.EBADF if S.device_count() > 0 else -errno.ENODEV
    before = S._lib.spmv_live_handles()
    out = C.c_void_p(1234)
    an = S._lib.spmv_csr_trsv_analyse
    assert an(None, 0, 0, 0, C.byref(out)) == -errno.EINVAL
    assert an(pj, 0, 0, 0, None) == -errno.EINVAL
    for uplo, unit, cap in ((2, 0, 0), (-1, 0, 0), (0, 2, 0), (0, -1, 0),
                            (0, 0, -1)):
        assert an(pj, uplo, unit, cap, C.byref(out)) == -errno.EINVAL
    assert an(pj, 1, 1, 7, C.byref(out)) == dead
    assert out.value is None  # *out is NULL after an error
    i = C.c_int(77)
    assert S._lib.spmv_trsv_info(None, C.byref(i), None, None, None, None,
                                 None, None) == -errno.EINVAL
    assert S._lib.spmv_trsv_info(pj, C.byref(i), None, None, None, None,
                                 None, None) == dead
    assert i.value == 77
    assert S._lib.spmv_trsv_download(pj, None, None, None, None, None, None,
                                     None) == dead
    o = S._opts()
    assert S._lib.spmv_trsv_solve(None, C.byref(o), 1, 8, 0, 8, 0, None,
                                  None) == -errno.EINVAL
    assert S._lib.spmv_trsv_solve(pj, C.byref(o), 1, 8, 0, 8, 0, None,
                                  None) == dead
    ignored = S.ignored_releases()
    S._lib.spmv_trsv_release(None)   # ignored, not counted
    S._lib.spmv_trsv_release(pj)     # not a live plan: ignored AND counted
    assert S.ignored_releases() == ignored + 1
    assert S._lib.spmv_live_handles() == before


def test_without_a_device_the_analysis_answers_enodev():
    if S.device_count() > 0:
        return  # with a device the same calls are test_gpu_trsv.py's
    M, IRP, JA, AS = TV.single()
    A = S.csr_from_arrays("t", M, M, IRP, JA, AS)
    with pytest.raises(OSError) as ei:
        S.CsrDevice.upload(A)
    assert ei.value.errno == errno.ENODEV
    S.csr_free(A)
    out = C.c_void_p(5)
    junk = C.cast(C.create_string_buffer(512), C.c_void_p)
    assert S._lib.spmv_csr_trsv_analyse(junk, 0, 0, 0, C.byref(out)) == \
        -errno.ENODEV
    assert out.value is None


# ------------------------------------------------------------ the launches
def test_the_launch_list_on_the_shapes_it_is_for(shapes):
    want = {"empty": [], "single": [(TV.CHAIN, 0, 0)],
            "diagonal": [(TV.CHAIN, 0, 0)],
            "chain300": [(TV.CHAIN, 0, 299)],
            "lap2d": [(TV.CHAIN, 0, 28)],
            "fan L-1": [(TV.CHAIN, 0, 1)], "fan L": [(TV.CHAIN, 0, 1)],
            "fan L+1": [(TV.CHAIN, 0, 0), (TV.WIDE, 1, 1)],
            "fan 3L+5": [(TV.CHAIN, 0, 0), (TV.WIDE, 1, 1)],
            "sandwich": [(TV.CHAIN, 0, 1), (TV.WIDE, 2, 2), (TV.CHAIN, 3, 4)],
            "arrow": [(TV.WIDE, 0, 0), (TV.CHAIN, 1, 1)]}
    for name, segs in want.items():
        M, IRP, JA, AS = shapes[name]
        plan = TV.reference_plan(IRP, JA, AS, "lower")
        assert TV.segments(plan["level_ptr"], L) == segs, name
    # 29 levels, both ways: the shape is held to what it is for
    M, IRP, JA, AS = shapes["lap2d"]
    for uplo in ("lower", "upper"):
        assert len(TV.reference_plan(IRP, JA, AS, uplo)["level_ptr"]) == 30
    # the random triangle takes both kernels
    M, IRP, JA, AS = shapes["random"]
    kinds = {s[0] for s in TV.segments(
        TV.reference_plan(IRP, JA, AS, "lower")["level_ptr"], L)}
    assert kinds == {TV.WIDE, TV.CHAIN}
    # the arrow's last row is far longer than the lane group
    M, IRP, JA, AS = shapes["arrow"]
    plan = TV.reference_plan(IRP, JA, AS, "lower")
    assert np.diff(plan["rowptr"]).max() == 9000 > 100 * GROUP


def test_the_launch_list_under_asan(tmp_path):
    """trsv_plan.h as a stand-alone program under ASan + UBSan: the edges,
    2000 seeded random level_ptrs, and Kahn + sort + gather restated with the
    kernels' index arithmetic over heap blocks of exactly the planned sizes"""
    exe = str(tmp_path / "trsv_plan_asan")
    subprocess.run(
        ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined",
         "-fno-omit-frame-pointer", "-fno-sanitize-recover=all",
         "-I", os.path.join(ROOT, "spmv_scpa_amd", "csrc"),
         os.path.join(ROOT, "tests", "asan", "trsv_plan_asan.cc"),
         "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    r = subprocess.run([exe, "2000"], capture_output=True, text=True, env=env)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "launch lists hold, levels and copies are the definitions" in r.stdout
    assert "FAILED" not in r.stdout and "ERROR" not in r.stderr


# ------------------------------------------------------------ the reference
def test_the_reference_plan_on_a_matrix_written_out():
    # row 2 stores its diagonal twice and (2, 0) twice; row 3 has no diagonal
    rows = [[(0, 2.0), (3, 9.0)],
            [(1, 4.0)],
            [(2, 1.0), (0, 5.0), (1, 0.0), (2, 0.5), (0, 7.0)],
            [(2, -1.0), (0, 3.0)]]
    M, IRP, JA, AS = TV.from_rows(rows)
    p = TV.reference_plan(IRP, JA, AS, "lower")
    assert p["level"].tolist() == [0, 0, 1, 2]
    assert p["order"].tolist() == [0, 1, 2, 3]
    assert p["level_ptr"].tolist() == [0, 2, 3, 4]
    assert p["rowptr"].tolist() == [0, 0, 0, 3, 5]
    assert p["ja"].tolist() == [0, 1, 0, 2, 0]       # stored order, both (2, 0)
    assert p["as"].tolist() == [5.0, 0.0, 7.0, -1.0, 3.0]
    assert p["diag"].tolist() == [2.0, 4.0, 1.5, 0.0]
    u = TV.reference_plan(IRP, JA, AS, "upper")
    assert u["level"].tolist() == [1, 0, 0, 0]
    assert u["order"].tolist() == [1, 2, 3, 0]
    assert u["ja"].tolist() == [3] and u["as"].tolist() == [9.0]
    # the slots and the tree: 9 entries of one row at G = 4
    rows = [[(i, 1.0)] for i in range(9)]
    rows.append([(c, float(2 ** c)) for c in range(9)] + [(9, 2.0)])
    M, IRP, JA, AS = TV.from_rows(rows)
    p = TV.reference_plan(IRP, JA, AS, "lower")
    B = np.ones((10, 1))
    B[9] = 1023.0
    X = TV.reference_solve(p, B, None, 4)
    assert X[9, 0] == (1023.0 - 511.0) / 2.0


@pytest.mark.parametrize("uplo", ["lower", "upper"])
def test_the_reference_against_a_dense_substitution(shapes, uplo):
    """|b - T x|_i <= (n_i + 3) u sum_c |T_ic| |x_c|: n_i products and sums,
    one subtraction and one division.  The residual is formed in extended
    precision; the dense substitution solves the same systems"""
    M, IRP, JA, AS = TV.random_triangle(700, seed=4, dominant=True)
    rng = np.random.default_rng(8)
    B = rng.uniform(-1.0, 1.0, (M, 3))
    scale = rng.uniform(0.5, 2.0, M)
    plan = TV.reference_plan(IRP, JA, AS, uplo)
    assert plan["rowptr"][-1] > M  # something to sum
    for unit in (False, True):
        for sc in (None, scale):
            X = TV.reference_solve(plan, B, sc, GROUP, unit)
            rhs = B if sc is None else sc[:, None] * B
            res = TV.residual(plan, rhs, X, unit)
            bound = TV.row_bound(plan, X, unit)
            assert np.all(res <= bound), (uplo, unit, float((res / bound).max()))
            Xd = TV.dense_solve(TV.dense_of(plan, unit), rhs, uplo == "upper")
            assert np.allclose(X, Xd, rtol=1e-9, atol=1e-12)
    # column j of a k-column solve is the one-column solve; ones scale nothing
    X3 = TV.reference_solve(plan, B, None, GROUP)
    X1 = TV.reference_solve(plan, B[:, 1:2], np.ones(M), GROUP)
    assert np.array_equal(X3[:, 1].view(np.uint64), X1[:, 0].view(np.uint64))


def test_every_gpu_shape_is_a_valid_matrix(shapes):
    for name, (M, IRP, JA, AS) in shapes.items():
        assert IRP.dtype == JA.dtype == np.int32 and AS.dtype == np.float64
        assert len(IRP) == M + 1 and IRP[-1] == len(JA) == len(AS), name
        assert len(JA) == 0 or (JA.min() >= 0 and JA.max() < M), name
    M, IRP, JA, AS = shapes["random"]
    rows = np.repeat(np.arange(M), np.diff(IRP))
    per_row = np.bincount(rows[JA == rows], minlength=M)
    assert (per_row == 0).any() and (per_row == 2).any()  # none, and twice
    assert (AS[JA < rows] == 0.0).any()                   # explicit zeros
    assert (JA > rows).any()                              # the other triangle
    assert np.any((np.diff(JA) < 0) & (np.diff(rows) == 0))  # unsorted
