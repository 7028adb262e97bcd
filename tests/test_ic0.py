"""Zero-fill incomplete Cholesky (spmv_csr_ic0; spmv_engine.h): what can be
checked without a GPU -- the declared surface, the binding's argument checks,
the answers without a device, and the numpy restatement of tests/_ic0.py
against the definition of an incomplete factor (on the pattern, L L^T is A).
The kernels themselves: tests/test_gpu_ic0.py."""
import ctypes as C
import errno

import numpy as np
import pytest

import _cg as G
import _ic0 as IC
import _pcg_trsv as PT
import _trsv as TV
import spmv_scpa_amd as S

L = S.trsv_shape()["small_rows"]


def test_the_headers_declare_the_entry_point():
    declared = S.declared_symbols()
    assert "spmv_csr_ic0" in declared and hasattr(S._lib, "spmv_csr_ic0")
    assert S.check_symbols()
    # the feature is detected by the symbol, not by the version string
    assert S.version() == "spmv_scpa_amd 0.7 gfx950"
    assert callable(S.CsrDevice.ic0) and callable(S.CsrDevice.sgs)
    assert [f for f, _ in S.Ic0Info._fields_] == \
        ["levels", "launches", "entries", "bad_pivots"]
    assert C.sizeof(S.Ic0Info) == 24


def test_the_binding_checks_its_arguments():
    fake = object.__new__(S.CsrDevice)  # a wrapper around no handle
    fake.h = None
    for kw in (dict(shift=-0.5), dict(shift=float("nan")),
               dict(shift=float("inf")), dict(max_levels=-1)):
        with pytest.raises(ValueError):
            fake.ic0(**kw)
    with pytest.raises(OSError) as ei:
        fake.ic0()
    assert ei.value.errno == errno.EINVAL  # the library's answer to NULL


def test_dead_handles_and_argument_errors_of_the_library():
    junk = C.create_string_buffer(512)  # never a handle of the library
    pj = C.cast(junk, C.c_void_p)
    dead = -errno.EBADF if S.device_count() > 0 else -errno.ENODEV
    before = S._lib.spmv_live_handles()
    out, info = C.c_void_p(1234), S.Ic0Info()
    ic0 = S._lib.spmv_csr_ic0
    assert ic0(None, 0.0, 0, C.byref(out), None) == -errno.EINVAL
    assert ic0(pj, 0.0, 0, None, None) == -errno.EINVAL
    for shift, cap in ((-1.0, 0), (float("nan"), 0), (float("inf"), 0),
                       (0.0, -1)):
        assert ic0(pj, shift, cap, C.byref(out), C.byref(info)) == \
            -errno.EINVAL
    assert ic0(pj, 0.25, 7, C.byref(out), C.byref(info)) == dead
    assert out.value is None  # *out is NULL after an error
    assert S._lib.spmv_live_handles() == before


def test_without_a_device_the_factorisation_answers_enodev():
    if S.device_count() > 0:
        return  # with a device the same calls are test_gpu_ic0.py's
    out = C.c_void_p(5)
    junk = C.cast(C.create_string_buffer(512), C.c_void_p)
    assert S._lib.spmv_csr_ic0(junk, 0.0, 0, C.byref(out), None) == \
        -errno.ENODEV
    assert out.value is None


# ------------------------------------------------------------ the reference
def test_the_reference_on_a_matrix_written_out():
    # A = L L^T with L = [[2], [1, 3], [0.5, -1, 2]]: no fill, so IC(0) is the
    # Cholesky factor; the upper triangle is absent from row 0 and wrong in 1
    rows = [[(0, 4.0)],
            [(0, 2.0), (1, 10.0), (2, 99.0)],
            [(0, 1.0), (1, -2.5), (2, 5.25)]]
    M, IRP, JA, AS = TV.from_rows(rows)
    F = IC.reference_ic0(M, IRP, JA, AS)
    assert F.IRP.tolist() == [0, 1, 3, 6] and F.JA.tolist() == [0, 0, 1, 0, 1, 2]
    assert F.AS.tolist() == [2.0, 1.0, 3.0, 0.5, -1.0, 2.0]
    assert F.bad_pivots == 0
    # shift: the diagonal becomes a_ii + shift * a_ii before the subtraction
    F = IC.reference_ic0(M, IRP, JA, AS, shift=0.5)
    assert F.AS[0] == np.sqrt(6.0) and F.AS[1] == 2.0 / np.sqrt(6.0)


@pytest.mark.parametrize("name", list(IC.MATRICES))
def test_on_the_pattern_the_factor_reproduces_the_matrix(name):
    """|sum_m L_im L_jm - a_ij| <= (n + 3) u sum_m |L_im L_jm| for every
    stored (i, j), n the common columns below j: n products and sums, one
    subtraction and one division or square root"""
    mat = IC.MATRICES[name]()
    F = IC.reference_ic0(*mat)
    assert F.bad_pivots == 0 and np.all(np.isfinite(F.AS))
    ratio = IC.pattern_ratio(mat, F)
    print(name, "largest ratio", ratio)
    assert ratio <= 1.0, (name, ratio)
    # the full matrix and its stored-lower-only copy: the same factor
    F2 = IC.reference_ic0(*IC.lower_of(*mat))
    assert np.array_equal(F.AS.view(np.uint64), F2.AS.view(np.uint64))


def test_the_shapes_take_the_kernels_they_are_for():
    def segs(mat):
        plan = TV.reference_plan(*PT.int32(mat)[1:], "lower")
        return TV.segments(plan["level_ptr"], L), np.diff(plan["level_ptr"])
    s, rows = segs(IC.MATRICES["lap2d(37,29,0.01)"]())
    assert s == [(TV.CHAIN, 0, 64)] and rows.max() <= L   # the chain alone
    s, rows = segs(IC.MATRICES["red-black(37,29,0.01)"]())
    assert s == [(TV.WIDE, 0, 0), (TV.WIDE, 1, 1)]        # the wide alone
    assert rows.tolist() == [537, 536]
    s, rows = segs(IC.MATRICES["arrow(600,3)"]())
    assert s == [(TV.CHAIN, 0, 0), (TV.WIDE, 1, 1)] and rows.tolist() == [1, 599]
    s, rows = segs(IC.MATRICES["layered"]())
    assert s == [(TV.CHAIN, 0, 0), (TV.WIDE, 1, 1), (TV.CHAIN, 2, 2),
                 (TV.WIDE, 3, 3)]
    # ... and the layered rows share columns: the sums have terms
    M, IRP, JA, AS = IC.lower_of(*IC.MATRICES["layered"]())
    terms = 0
    for i in range(M):
        ci = JA[IRP[i]:IRP[i + 1] - 1]
        for j in ci:
            terms += len(np.intersect1d(ci[ci < j], JA[IRP[j]:IRP[j + 1] - 1]))
    assert terms > 100, terms


def test_an_indefinite_stencil_counts_its_bad_pivots():
    mat = G.lap2d(37, 29, -1.3)
    F = IC.reference_ic0(*mat)
    assert F.bad_pivots == 849 and F.bad_rows[0] == 128
    # a NaN reaches exactly the dependent rows: every bad row holds one
    assert np.all(IC.nan_rows(F)[F.bad_rows[1:]])
    assert not IC.nan_rows(F)[:128].any()
    F = IC.reference_ic0(*mat, shift=0.25)
    assert F.bad_pivots == 0 and np.all(np.isfinite(F.AS))
