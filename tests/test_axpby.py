"""Y = alpha*A*X + beta*Y launches for 1-8 interleaved vectors
(spmv_*_launch_axpby, spmv_*_axpby_bytes; spmv_engine.h): what can be checked
without a GPU -- the declared surface, the ctypes signatures, the dead-handle
answers and the argument checks of the Python wrapper.  The kernels
themselves: tests/test_gpu_axpby.py."""
import ctypes as C
import errno

import pytest

import spmv_scpa_amd as S

NEW = ["spmv_csr_launch_axpby", "spmv_hll_launch_axpby",
       "spmv_csr_axpby_bytes", "spmv_hll_axpby_bytes"]


def test_the_headers_declare_the_axpby_entry_points():
    declared = S.declared_symbols()
    for name in NEW:
        assert name in declared, name
        assert hasattr(S._lib, name), name
    assert S.check_symbols()
    # the feature is detected by the symbol, not by the version string
    assert S.version() == "spmv_scpa_amd 0.7 gfx950"


def test_the_twin_signatures_come_from_the_shared_list():
    names = [t[0] for t in S._TWINS]
    assert names.count("launch_axpby") == 1 and names.count("axpby_bytes") == 1
    for fmt in ("csr", "hll"):
        fn = getattr(S._lib, "spmv_%s_launch_axpby" % fmt)
        assert fn.restype is C.c_int
        # launch_multi's arguments with alpha, beta (by value) after k
        assert fn.argtypes == [C.c_void_p, C.POINTER(S.LaunchOpts), C.c_int,
                               C.c_double, C.c_double, C.c_void_p, C.c_int64,
                               C.c_void_p, C.c_int64, C.c_void_p]
        fn = getattr(S._lib, "spmv_%s_axpby_bytes" % fmt)
        assert fn.restype is C.c_int64
        assert fn.argtypes == [C.c_void_p, C.c_int, C.c_int]


def test_dead_handles_are_refused():
    x = C.create_string_buffer(64)
    px = C.cast(x, C.c_void_p)
    junk = C.create_string_buffer(512)  # never a handle of the library
    pj = C.cast(junk, C.c_void_p)
    # a pointer that is no handle: -EBADF; without any GPU no handle can be
    # live and -ENODEV is the answer (as spmv_*_launch_multi)
    dead = -errno.EBADF if S.device_count() > 0 else -errno.ENODEV
    for fmt in ("csr", "hll"):
        launch = getattr(S._lib, "spmv_%s_launch_axpby" % fmt)
        multi = getattr(S._lib, "spmv_%s_launch_multi" % fmt)
        assert launch(None, None, 1, 2.0, 1.0, px, 1, px, 1, None) == -errno.EINVAL
        assert launch(pj, None, 1, 2.0, 1.0, px, 1, px, 1, None) == dead
        # one function checks both launches: the same answers
        assert multi(None, None, 1, px, 1, px, 1, None) == -errno.EINVAL
        assert multi(pj, None, 1, px, 1, px, 1, None) == dead
        nbytes = getattr(S._lib, "spmv_%s_axpby_bytes" % fmt)
        for reads_y in (0, 1):
            assert nbytes(None, 1, reads_y) == -errno.EINVAL
            assert nbytes(pj, 1, reads_y) == -errno.EBADF


@pytest.mark.parametrize("cls", [S.CsrDevice, S.HllDevice])
def test_the_wrapper_checks_k_and_the_strides_before_anything_is_launched(cls):
    fake = object.__new__(cls)  # a wrapper around no handle: a call that
    fake.h = None               # reached the library would answer EINVAL too
    calls = []
    fake._call = lambda *a: calls.append(a)
    for kw in (dict(k=0), dict(k=9), dict(k=-1), dict(k=4, ldx=3),
               dict(k=4, ldy=2), dict(k=8, ldx=7, ldy=8)):
        with pytest.raises((ValueError, OSError)) as ei:
            fake.launch_axpby(2.0, 1.0, 1, 2, **kw)
        if isinstance(ei.value, OSError):
            assert ei.value.errno == errno.EINVAL
    assert not calls
    # a good call does reach the library: k, alpha, beta, X, ldx, Y, ldy
    fake.launch_axpby(-1, 1, 1, 2, 4, ldx=6)
    assert len(calls) == 1 and calls[0][0] == "launch_axpby"
    assert calls[0][2:9] == (4, -1.0, 1.0, 1, 6, 2, 0)
    assert all(type(v) is float for v in calls[0][3:5])
    fake.launch_axpby(0.5, 0.0, 1, 2)  # k defaults to one vector
    assert calls[1][2:5] == (1, 0.5, 0.0)


@pytest.mark.parametrize("cls", [S.CsrDevice, S.HllDevice])
def test_axpby_bytes_asks_for_y_only_when_beta_is_not_zero(cls):
    fake = object.__new__(cls)
    fake.h = None
    asked = []
    fake._fn = lambda name: (lambda h, k, reads_y:
                             asked.append((name, k, reads_y)) or 0)
    for beta in (0.0, -0.0, 1.0, -1.7, float("nan")):
        fake.axpby_bytes(4, beta)
    assert asked == [("axpby_bytes", 4, r) for r in (0, 0, 1, 1, 1)]
