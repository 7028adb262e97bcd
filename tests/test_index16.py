"""16-bit column offsets on column-major HLL handles (spmv_hll_to_index16,
spmv_engine.h): what can be checked without a GPU -- the declared surface, the
ctypes signatures, the dead-handle contract, the no-device convention
(-ENODEV, never a CPU fallback), the Python wrappers' argument checks, and
that every case of the GPU tests fits the format at all.  The kernels
themselves: tests/test_gpu_index16.py."""
import ctypes as C
import errno

import numpy as np
import pytest

import _index16 as I
import _oracle as O
import spmv_scpa_amd as S

NEW = ["spmv_hll_to_index16", "spmv_hll_index_bytes",
       "spmv_hll_download_index16"]


def test_the_header_declares_the_entry_points_and_the_library_exports_them():
    declared = S.declared_symbols()
    for name in NEW:
        assert name in declared, name
        assert hasattr(S._lib, name), name
    assert S.check_symbols()
    # callers detect the feature by the symbol: the version has not moved
    assert S.version() == "spmv_scpa_amd 0.7 gfx950"
    for name in ("spmv_csr_to_index16", "spmv_csr_index_bytes"):
        assert name not in declared and not hasattr(S._lib, name), name


def test_the_signatures_come_from_the_shared_list():
    assert [t[0] for t in S._HLL_ONLY] == ["to_index16", "index_bytes",
                                           "download_index16"]
    fn = S._lib.spmv_hll_to_index16
    assert fn.restype is C.c_int
    assert fn.argtypes == [C.c_void_p, C.POINTER(C.c_void_p)]
    fn = S._lib.spmv_hll_index_bytes
    assert fn.restype is C.c_int and fn.argtypes == [C.c_void_p]
    fn = S._lib.spmv_hll_download_index16
    assert fn.restype is C.c_int
    assert fn.argtypes == [C.c_void_p, C.POINTER(C.c_int),
                           C.POINTER(C.c_uint16)]


def test_null_and_dead_handles_are_refused():
    out = C.c_void_p(1)
    base = (C.c_int * 4)()
    off16 = (C.c_uint16 * 4)()
    assert S._lib.spmv_hll_to_index16(None, C.byref(out)) == -errno.EINVAL
    assert S._lib.spmv_hll_index_bytes(None) == -errno.EINVAL
    assert S._lib.spmv_hll_download_index16(None, base, off16) == -errno.EINVAL
    junk = C.create_string_buffer(512)  # never a handle of the library
    p = C.cast(junk, C.c_void_p)
    assert S._lib.spmv_hll_to_index16(p, None) == -errno.EINVAL
    # not a live handle: -EBADF, or -ENODEV where no handle can be live at all
    dead = -errno.EBADF if S.device_count() > 0 else -errno.ENODEV
    live = S._lib.spmv_live_handles()
    assert S._lib.spmv_hll_to_index16(p, C.byref(out)) == dead
    assert not out.value  # *out is cleared before anything else happens
    assert S._lib.spmv_hll_index_bytes(p) == dead
    assert S._lib.spmv_hll_download_index16(p, base, off16) == dead
    assert S._lib.spmv_live_handles() == live


def test_without_a_gpu_the_entry_points_answer_enodev():
    if S.device_count() > 0:
        pytest.skip("a GPU is present")
    junk = C.create_string_buffer(512)
    p = C.cast(junk, C.c_void_p)
    out = C.c_void_p()
    live = S._lib.spmv_live_handles()
    assert S._lib.spmv_hll_to_index16(p, C.byref(out)) == -errno.ENODEV
    assert not out.value
    assert S._lib.spmv_hll_index_bytes(p) == -errno.ENODEV
    assert S._lib.spmv_hll_download_index16(p, None, None) == -errno.ENODEV
    # ... and the wrappers raise accordingly
    fake = object.__new__(S.HllDevice)  # a wrapper around no handle
    fake.h = p
    fake.num_blocks, fake.slots = 1, 32
    with pytest.raises(OSError) as ei:
        fake.to_index16()
    assert ei.value.errno == errno.ENODEV
    with pytest.raises(OSError) as ei:
        fake.index_bytes
    assert ei.value.errno == errno.ENODEV
    with pytest.raises(OSError) as ei:
        fake.download_index16()
    assert ei.value.errno == errno.ENODEV
    fake.h = None  # nothing for its finaliser to release
    assert S._lib.spmv_live_handles() == live


def test_the_wrappers_check_their_arguments():
    # a released wrapper holds no handle: the library's NULL check answers
    fake = object.__new__(S.HllDevice)
    fake.h = None
    fake.num_blocks, fake.slots = 0, 0
    for call in (fake.to_index16, fake.download_index16,
                 lambda: fake.index_bytes):
        with pytest.raises(OSError) as ei:
            call()
        assert ei.value.errno == errno.EINVAL
    # the conversion exists for HLL handles only
    assert not hasattr(S.CsrDevice, "to_index16")
    assert isinstance(S.HllDevice.index_bytes, property)


@pytest.mark.parametrize("case", I.CASES)
def test_every_case_of_the_gpu_tests_fits_a_16_bit_window(case):
    """the GPU tests rely on these matrices converting: no hack block wider
    than 512 columns, no block whose valid columns span more than 65 536"""
    M, N, IRP, JA, AS, _ = I.case_arrays(case)
    p = I.pack16(IRP, JA, AS)
    assert I.fits(p) == 0, (case, int(p["width"].max()), int(p["span"].max()))
    ok = ~p["pad"]
    col = p["base"][np.repeat(np.arange(len(p["base"])),
                              np.diff(p["off"]))].astype(np.int64) + p["off16"]
    assert np.array_equal(col[ok], p["ja"][ok])
    assert np.all((col >= 0) & (col < max(N, 1)))


def test_the_packer_refuses_what_the_library_must_refuse():
    M = N = 131_072
    IRP, JA, AS = O.synth_csr(S.SYNTH_RANDOM, M, N, 8, 1 << 30, 42)
    assert I.fits(I.pack16(IRP, JA, AS)) == errno.ERANGE
    IRP = np.array([0, 513], np.int32)  # one row of 513 entries: a wide block
    JA = np.arange(513, dtype=np.int32)
    assert I.fits(I.pack16(IRP, JA, np.ones(513))) == errno.ENOTSUP
