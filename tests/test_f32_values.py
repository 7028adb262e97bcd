"""fp32-stored matrix values (spmv_engine.h, library 0.7): what can be checked
without a GPU -- the declared surface, the ctypes signatures, the no-device
convention (-ENODEV, never a CPU fallback) and the Python wrappers' argument
checks.  The kernels themselves: tests/test_gpu_f32_values.py."""
import ctypes as C
import errno

import numpy as np
import pytest

import _golden as G
import spmv_scpa_amd as S

NEW = ["spmv_csr_upload_f32", "spmv_hll_upload_f32", "spmv_csr_to_f32",
       "spmv_csr_value_bytes", "spmv_hll_value_bytes"]


def test_the_headers_declare_the_f32_entry_points_and_the_library_has_them():
    declared = S.declared_symbols()
    for name in NEW:
        assert name in declared, name
        assert hasattr(S._lib, name), name
    assert S.check_symbols()
    assert S.version() == "spmv_scpa_amd 0.7 gfx950"


def test_the_twin_signatures_come_from_the_shared_list():
    assert any(t[0] == "value_bytes" for t in S._TWINS)
    for fmt in ("csr", "hll"):
        fn = getattr(S._lib, "spmv_%s_value_bytes" % fmt)
        assert fn.restype is C.c_int and fn.argtypes == [C.c_void_p]


def test_values_argument_is_checked_before_anything_is_uploaded():
    A = S.io_load_csr(G.mtx_path("gen"))
    H = S.csr_to_hll(A, True)
    with pytest.raises(ValueError):
        S.CsrDevice.upload(A, values="f16")
    with pytest.raises(ValueError):
        S.HllDevice.upload(H, True, values=4)
    S.hll_free(H)
    S.csr_free(A)


def test_dead_handles_are_refused_by_the_new_entry_points():
    out = C.c_void_p()
    assert S._lib.spmv_csr_to_f32(None, C.byref(out)) == -errno.EINVAL
    assert S._lib.spmv_csr_value_bytes(None) == -errno.EINVAL
    assert S._lib.spmv_hll_value_bytes(None) == -errno.EINVAL
    junk = C.create_string_buffer(512)  # never a handle of the library
    p = C.cast(junk, C.c_void_p)
    assert S._lib.spmv_csr_value_bytes(p) == -errno.EBADF
    assert S._lib.spmv_hll_value_bytes(p) == -errno.EBADF
    assert S._lib.spmv_csr_upload_f32(None, C.byref(out)) == -errno.EINVAL
    assert S._lib.spmv_hll_upload_f32(None, 1, C.byref(out)) == -errno.EINVAL


def test_without_a_gpu_the_f32_entry_points_answer_enodev():
    if S.device_count() > 0:
        pytest.skip("a GPU is present")
    A = S.io_load_csr(G.mtx_path("gen"))
    H = S.csr_to_hll(A, True)
    live = S._lib.spmv_live_handles()
    out = C.c_void_p()
    assert S._lib.spmv_csr_upload_f32(A, C.byref(out)) == -errno.ENODEV
    assert not out.value
    assert S._lib.spmv_hll_upload_f32(H, 1, C.byref(out)) == -errno.ENODEV
    assert not out.value
    # no handle can exist without a device: whatever pointer comes in
    junk = C.create_string_buffer(512)
    assert S._lib.spmv_csr_to_f32(C.cast(junk, C.c_void_p),
                                  C.byref(out)) == -errno.ENODEV
    assert not out.value
    # ... and the wrappers raise accordingly
    with pytest.raises(OSError) as ei:
        S.CsrDevice.upload(A, values="f32")
    assert ei.value.errno == errno.ENODEV
    with pytest.raises(OSError) as ei:
        S.HllDevice.upload(H, True, values="f32")
    assert ei.value.errno == errno.ENODEV
    fake = object.__new__(S.CsrDevice)  # a wrapper around no handle
    fake.h = C.cast(junk, C.c_void_p)
    with pytest.raises(OSError) as ei:
        fake.to_f32()
    assert ei.value.errno == errno.ENODEV
    fake.h = None  # nothing for its finaliser to release
    assert S._lib.spmv_live_handles() == live
    S.hll_free(H)
    S.csr_free(A)


def test_round_to_nearest_even_is_what_numpy_does_too():
    """the expected values of the GPU tests are AS.astype(float32): numpy's
    cast and the C cast of the library are the same IEEE conversion -- ties go
    to the even mantissa, values below FLT_MIN become subnormals"""
    tie_down = 1.0 + 2.0 ** -24            # halfway between 1 and 1 + 2^-23
    tie_up = 1.0 + 3.0 * 2.0 ** -24        # halfway, odd neighbour below
    with np.errstate(over="ignore"):
        a = np.array([tie_down, tie_up, 1e-40, 1e39, -1e39]).astype(np.float32)
    assert a[0] == np.float32(1.0)
    assert a[1] == np.float32(1.0 + 2.0 ** -22)
    assert 0.0 < float(a[2]) < float(np.finfo(np.float32).tiny)
    assert np.isinf(a[3]) and np.isinf(a[4])
