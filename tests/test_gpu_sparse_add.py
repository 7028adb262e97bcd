"""The sparse sum of CSR handles on the GPU and its companions (spmv_csr_add,
spmv_csr_from_diag, spmv_csr_scale; spmv_engine.h).

The result is defined to the byte (tests/_add.py reference), so everything is
compared through download() as int32 arrays and uint64 views of the values:
THERE IS NO TOLERANCE here.  Every sum runs in all three modes of
spmv_add_set_class (the rule, lane groups only, workgroups only) and must give
the same bytes.

The shapes are those of tests/_add.py, which the CPU test (tests/test_add.py)
holds to what they are for.  No test provokes a fault: every error case
returns before a launch that could misbehave.  Every test runs under a time
limit of its own (LIMIT_S): a test that exceeds it ends the whole process, so
nothing else is started on the device.

The module's name places it after tests/test_gpu_exit.py in the collection
order on purpose: test_stale_wrapper_cannot_release_a_newer_handle_at_the_
same_address there depends on what the host allocator has seen before it
("every test collected before this one", its docstring), and with this module
collected first it skipped where it had passed.
"""
import ctypes as C
import errno
import faulthandler

import numpy as np
import pytest

import _add as AD
import _bicgstab as BI
import _cg as G
import _oracle as O
import _transpose as TR
import spmv_scpa_amd as S

pytestmark = pytest.mark.gpu

LIMIT_S = 240
SHAPE = S.add_shape()
MODES = (0, 1, 2)
NEG0 = 0x8000_0000_0000_0000


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(LIMIT_S, exit=True)
    was = S.add_set_class(0)
    yield
    S.add_set_class(was)
    faulthandler.cancel_dump_traceback_later()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def upload(mat, values="f64"):
    M, N, IRP, JA, AS = mat
    A = S.csr_from_arrays("t", M, N, IRP, JA, AS)
    d = S.CsrDevice.upload(A, values=values)
    S.csr_free(A)
    return d


def arrays(d):
    """(IRP, JA, AS) of a handle, copied out of its download"""
    p = d.download()
    assert (p.contents.M, p.contents.N, p.contents.NZ) == (d.M, d.N, d.NZ)
    out = tuple(a.copy() for a in S.csr_arrays(p))
    S.csr_free(p)
    return out


def same(got, want):
    return (got[0].dtype == got[1].dtype == np.int32
            and np.array_equal(got[0], want[0])
            and np.array_equal(got[1], want[1])
            and np.array_equal(bits(got[2]), bits(want[2])))


def check_sum(alpha, A, beta, B, want=None, values=("f64", "f64"),
              same_handle=False):
    """upload, add in every mode, compare with the reference -> C's arrays"""
    dA = upload(A, values[0])
    dB = dA if same_handle else upload(B, values[1])
    if want is None:  # the f32 handles' values, widened
        want = AD.reference(alpha, A[:4] + (arrays(dA)[2],),
                            beta, B[:4] + (arrays(dB)[2],))
    live = S._lib.spmv_live_handles()
    got = None
    for mode in MODES:
        S.add_set_class(mode)
        dC = dA.add(dB, alpha, beta)
        assert S._lib.spmv_live_handles() == live + 1
        assert (dC.M, dC.N) == (A[0], A[1]) and dC.value_bytes == 8
        got = arrays(dC)
        info = dC.add_info
        assert same(got, want), mode
        assert info.nz == dC.NZ == len(want[1])
        assert info.matched == len(A[3]) + len(B[3]) - len(want[1])
        L = AD.lens(A, B)
        assert info.widest == (int(L.max()) if len(L) else 0)
        assert info.rows_in_bin == AD.rows_in_bin(A, B, SHAPE, mode)
        dC.release()
    S.add_set_class(0)
    # the operands are unchanged
    assert np.array_equal(arrays(dA)[1], A[3])
    if not same_handle:
        dB.release()
    dA.release()
    assert S._lib.spmv_live_handles() == live - (1 if same_handle else 2)
    return got


def swapped(alpha, A, beta, B):
    """add(alpha, A, beta, B) == add(beta, B, alpha, A) to the byte"""
    got = check_sum(alpha, A, beta, B)
    assert same(check_sum(beta, B, alpha, A), got)
    return got


# ------------------------------------------------------------ 1. the bytes
def test_partial_overlap_with_empty_rows():
    A, B = AD.overlap()
    I, J, V = swapped(1.5, A, -0.75, B)
    assert 0 < AD.matched(A, B) < min(len(A[3]), len(B[3]))


def test_the_same_handle_twice():
    A, _ = AD.overlap()
    I, J, V = check_sum(1.0, A, -1.0, A, same_handle=True)
    assert len(J) == len(A[3]) and not bits(V).any()
    check_sum(2.0, A, 0.5, A, same_handle=True)


def test_disjoint_patterns():
    A, B = AD.disjoint()
    I, J, V = swapped(2.0, A, 3.0, B)
    assert len(J) == len(A[3]) + len(B[3])


@pytest.mark.parametrize("name", list(AD.degenerate()))
def test_degenerate_sizes(name):
    A, B = AD.degenerate()[name]
    I, J, V = check_sum(1.0, A, 1.0, B)
    assert len(I) == A[0] + 1
    if name in ("both empty", "M = 0", "N = 0"):
        assert not I.any() and len(J) == 0


@pytest.mark.parametrize("w", SHAPE["widths"])
def test_the_class_edge_and_the_chunk_edges_of_every_width(w):
    A, B, what = AD.edges(w)
    assert AD.pick_group(A, B, SHAPE) == w
    I, J, V = check_sum(1.5, A, -0.75, B, want=AD.edges_reference(w))
    assert AD.rows_in_bin(A, B, SHAPE)[1] > 0


def test_long_rows():
    arrow = G.arrow(2100, 3)
    A = (arrow[0], arrow[0]) + arrow[1:]
    dA = upload(A)
    dT = dA.transpose()
    want = AD.reference(1.0, A, 1.0, AD.transpose(A))
    for mode in MODES:
        S.add_set_class(mode)
        dC = dA.add(dT)
        assert same(arrays(dC), want), mode
        assert dC.add_info.widest == 2 * 2100
        assert dC.add_info.rows_in_bin == AD.rows_in_bin(A, A, SHAPE, mode)
        dC.release()
    dT.release()
    dA.release()
    A, B = AD.long_against_one()
    I, J, V = swapped(1.0, A, 1.0, B)
    assert np.diff(I).tolist() == [3000, 3000, 3001]


def test_wide_columns():
    A, B = AD.wide_n()
    I, J, V = swapped(1.0, A, -2.0, B)
    assert A[1] == 2 ** 24 + 1 and J.max() == 2 ** 24
    assert AD.matched(A, B) >= 4


@pytest.mark.parametrize("name", list(AD.special()))
def test_special_values(name):
    alpha, A, beta, B = AD.special()[name]
    I, J, V = check_sum(alpha, A, beta, B)
    if name == "zeros":
        assert bits(V).tolist() == [NEG0, NEG0, NEG0, 0]
    if name == "inf - inf":
        assert np.flatnonzero(np.isnan(V)).tolist() == [0]
    if name == "alpha = 0":
        assert np.flatnonzero(np.isnan(V)).tolist() == [0, 3] and len(J) == 7
    if name != "nan" and name != "alpha = 0" and name != "inf - inf":
        assert same(check_sum(beta, B, alpha, A), (I, J, V))


@pytest.mark.parametrize("values", [("f32", "f64"), ("f64", "f32"),
                                    ("f32", "f32")])
def test_f32_operands_are_widened_exactly(values):
    A, B = AD.overlap()
    I, J, V = check_sum(1.5, A, -0.75, B, values=values)
    assert not np.array_equal(bits(V), bits(AD.reference(1.5, A, -0.75, B)[2]))
    A, B = AD.long_against_one()
    check_sum(1.5, A, -0.75, B, values=values)


# ------------------------------------------------- 2. an ordinary handle
def test_the_sum_is_an_ordinary_handle():
    A, B = AD.overlap()
    A = A[:4] + (np.abs(A[4]),)
    want = AD.reference(1.0, A, 2.0, B)
    dA, dB = upload(A), upload(B)
    dC = dA.add(dB, 1.0, 2.0)
    dU = upload((A[0], A[1]) + want)
    assert same(arrays(dC), want)
    x = O.synth_x(7, 0, dC.N)
    X = np.stack([x, 2.0 * x, -x], axis=1)
    d_x, d_X = S.DevBuffer.from_numpy(x), S.DevBuffer.from_numpy(X)
    d_y = S.DevBuffer(dC.M * 8 * 3)

    def run(fn, n):
        S._lib.spmv_dev_memset(d_y.ptr, 0xFF, n * 8, None)
        fn()
        S.stream_sync()
        return bits(d_y.to_numpy(np.float64, n))

    for kernel in range(S.NUM_CSR_KERNELS):
        got = run(lambda: dC.launch(kernel, d_x.ptr, d_y.ptr), dC.M)
        ref = run(lambda: dU.launch(kernel, d_x.ptr, d_y.ptr), dC.M)
        assert np.array_equal(got, ref), kernel
    got = run(lambda: dC.launch_multi(d_X.ptr, d_y.ptr, 3), dC.M * 3)
    ref = run(lambda: dU.launch_multi(d_X.ptr, d_y.ptr, 3), dC.M * 3)
    assert np.array_equal(got, ref)
    tC, tU = dC.transpose(), dU.transpose()
    assert same(arrays(tC), arrays(tU))
    assert same(arrays(tC), AD.transpose((A[0], A[1]) + want)[2:])
    hC, hU = dC.to_hll(True), dU.to_hll(True)
    got = run(lambda: hC.launch(1, d_x.ptr, d_y.ptr), dC.M)
    ref = run(lambda: hU.launch(1, d_x.ptr, d_y.ptr), dC.M)
    assert np.array_equal(got, ref)
    for b in (d_x, d_X, d_y):
        b.free()
    for h in (hU, hC, tU, tC, dU, dC, dB, dA):
        h.release()


# ------------------------------------------------------- 3. the identities
def test_a_shifted_stencil_through_from_diag():
    A, want = AD.shifted_stencil(40, 1.3)
    dA = upload(A)
    dI = S.CsrDevice.from_diag(A[0])
    eye = arrays(dI)
    assert (dI.M, dI.N, dI.NZ) == (A[0], A[0], A[0])
    assert np.array_equal(eye[0], np.arange(A[0] + 1))
    assert np.array_equal(eye[1], np.arange(A[0])) and np.all(eye[2] == 1.0)
    for mode in MODES:
        S.add_set_class(mode)
        dC = dA.add(dI, 1.0, -1.3)
        assert same(arrays(dC), want), mode
        assert dC.add_info.matched == A[0]
        dC.release()
    dI.release()
    dA.release()
    empty = S.CsrDevice.from_diag(0)
    assert (empty.M, empty.NZ) == (0, 0) and arrays(empty)[0].tolist() == [0]
    empty.release()


def test_a_plus_its_transpose_is_symmetric():
    M, IRP, JA, AS = BI.convdiff(37, 29, 0.5, 0.5)
    dA = upload((M, M, IRP, JA, AS))
    assert dA.symmetry() != S.SYM_VALUES
    dT = dA.transpose()
    for mode in MODES:
        S.add_set_class(mode)
        dC = dA.add(dT)
        assert dC.symmetry() == S.SYM_VALUES == 2
        dC.release()
    dT.release()
    dA.release()


def test_from_diag_returns_the_bits_of_its_vector():
    rng = np.random.default_rng(61)
    d = rng.uniform(-2, 2, 1000)
    d[3], d[4], d[5], d[6] = np.nan, 0.0, -0.0, np.inf
    d[7:8].view(np.uint64)[0] = 0x7FF8_0000_0000_BEEF  # a NaN with a payload
    d_d, d_out = S.DevBuffer.from_numpy(d), S.DevBuffer(1000 * 8)
    dD = S.CsrDevice.from_diag(1000, d_d.ptr)
    I, J, V = arrays(dD)
    assert np.array_equal(I, np.arange(1001)) and np.array_equal(
        J, np.arange(1000))
    assert np.array_equal(bits(V), bits(d))
    dD.release()
    # ... and through diag(), whose sum starts from 0.0 by its own contract:
    # a vector without -0.0 and with the default NaN comes back to the bit
    d[5], d[7] = 0.0, np.nan
    S._check(S._lib.spmv_copy_h2d(d_d.ptr, d.ctypes.data, d.nbytes), "h2d")
    dD = S.CsrDevice.from_diag(1000, d_d.ptr)
    dD.diag(d_out.ptr)
    S.stream_sync()
    assert np.array_equal(bits(d_out.to_numpy(np.float64, 1000)), bits(d))
    dD.release()
    d_d.free()
    d_out.free()


def test_scale_keeps_symmetry_and_the_pattern_bytes():
    M, IRP, JA, AS = G.lap2d(40, 40, 0.25)
    rng = np.random.default_rng(62)
    AS = AS * rng.uniform(1, 2, 1)[0]
    s = 2.0 ** rng.integers(-20, 21, M).astype(np.float64)
    rows = np.repeat(np.arange(M), np.diff(IRP))
    d_s = S.DevBuffer.from_numpy(s)
    dA = upload((M, M, IRP, JA, AS))
    dS = dA.scale(d_s.ptr, d_s.ptr)
    assert dS.symmetry() == 2
    assert same(arrays(dS), (IRP, JA, (s[rows] * AS) * s[JA]))
    dS.release()
    dA.release()
    # unsorted rows with duplicates, rectangular, arbitrary factors
    A = AD.SG.random_unsorted(60, 45, 9, 63)
    rows = np.repeat(np.arange(60), np.diff(A[2]))
    l, r = rng.uniform(-2, 2, 60), rng.uniform(-2, 2, 45)
    d_l, d_r = S.DevBuffer.from_numpy(l), S.DevBuffer.from_numpy(r)
    for values in ("f64", "f32"):
        dA = upload(A, values)
        a = arrays(dA)[2]
        for dl, dr, want in ((d_l.ptr, d_r.ptr, (l[rows] * a) * r[A[3]]),
                             (d_l.ptr, None, l[rows] * a),
                             (None, d_r.ptr, a * r[A[3]])):
            dS = dA.scale(dl, dr)
            assert dS.value_bytes == 8
            assert same(arrays(dS), (A[2], A[3], want))
            dS.release()
        dA.release()
    dE = upload(AD.empty(4, 3))
    dS = dE.scale(d_l.ptr, None)
    assert dS.NZ == 0 and not arrays(dS)[0].any()
    for h in (dS, dE):
        h.release()
    for b in (d_s, d_l, d_r):
        b.free()


# --------------------------------------------------------------- 4. errors
def test_every_refusal_in_its_order_creates_nothing():
    A, B = AD.random_sorted(20, 15, 4, 64), AD.random_sorted(20, 15, 4, 65)
    dA, dB = upload(A), upload(B)
    live = S._lib.spmv_live_handles()
    fn = S._lib.spmv_csr_add
    info = S.AddInfo()
    info.nz = -77
    info.matched = -78
    junk = C.cast(C.create_string_buffer(512), C.c_void_p)

    def refused(a, b, err, alpha=1.0, beta=1.0, with_out=True):
        for mode in MODES:
            S.add_set_class(mode)
            before = S._lib.spmv_live_handles()
            out = C.c_void_p(1234)
            rc = fn(alpha, a, beta, b, C.byref(out) if with_out else None,
                    C.byref(info))
            assert rc == -err, (rc, err, mode)
            assert (out.value is None) == with_out
            assert S._lib.spmv_live_handles() == before
            assert (info.nz, info.matched) == (-77, -78)
        S.add_set_class(0)

    refused(None, dB.h, errno.EINVAL)
    refused(dA.h, None, errno.EINVAL)
    refused(dA.h, dB.h, errno.EINVAL, with_out=False)
    refused(junk, dB.h, errno.EINVAL, alpha=np.nan)  # before -EBADF
    refused(dA.h, dB.h, errno.EINVAL, beta=np.inf)
    refused(junk, dB.h, errno.EBADF)
    refused(dA.h, junk, errno.EBADF)
    other = upload(AD.random_sorted(20, 16, 4, 66))
    tall = upload(AD.random_sorted(21, 15, 4, 67))
    refused(dA.h, other.h, errno.EINVAL)
    refused(tall.h, dB.h, errno.EINVAL)
    refused(junk, other.h, errno.EBADF)  # a dead handle before the shapes
    # after release_source: -ENODATA, from either side, before the columns
    gone = upload(B)
    try:
        S.set_panel_schedule("chain")
        gone.build_panels(0)
        gone.release_source()
    finally:
        S.set_panel_schedule("sweep")
    refused(dA.h, gone.h, errno.ENODATA)
    refused(gone.h, dA.h, errno.ENODATA)
    refused(gone.h, other.h, errno.EINVAL)  # the shapes before the source
    # a column outside [0, N), in A and in B; before the order of the rows
    bad = upload((20, 15, TR.irp_of([1, 0, 1] + [0] * 17),
                  np.array([2, 15], np.int32), np.ones(2)))
    refused(bad.h, dB.h, errno.EDOM)
    refused(dA.h, bad.h, errno.EDOM)
    refused(gone.h, bad.h, errno.ENODATA)
    both = upload((20, 15, TR.irp_of([3] + [0] * 19),
                   np.array([5, 4, -1], np.int32), np.ones(3)))
    refused(dA.h, both.h, errno.EDOM)
    unsorted = upload((20, 15, TR.irp_of([3] + [0] * 19),
                       np.array([1, 5, 4], np.int32), np.ones(3)))
    refused(dA.h, unsorted.h, errno.EINVAL)
    refused(unsorted.h, dB.h, errno.EINVAL)
    refused(bad.h, unsorted.h, errno.EDOM)
    dup = upload((20, 15, TR.irp_of([0] * 19 + [3]),
                  np.array([1, 4, 4], np.int32), np.ones(3)))
    refused(dA.h, dup.h, errno.EINVAL)
    refused(dup.h, dup.h, errno.EINVAL)
    # the companions: a refusal leaves *out NULL and no handle behind, also
    # the one that comes after the result was allocated (scale's -EDOM)
    d_v = S.DevBuffer.from_numpy(np.ones(20))
    before = S._lib.spmv_live_handles()
    for err, args in (
            (errno.EBADF, (junk, d_v.ptr, None)),
            (errno.EINVAL, (dA.h, None, None)),
            (errno.ENODATA, (gone.h, d_v.ptr, None)),
            (errno.EDOM, (bad.h, None, d_v.ptr)),
            (errno.EDOM, (both.h, d_v.ptr, d_v.ptr))):
        out = C.c_void_p(1234)
        assert S._lib.spmv_csr_scale(*args, C.byref(out)) == -err, (err, args)
        assert out.value is None
        assert S._lib.spmv_live_handles() == before
    out = C.c_void_p(1234)
    assert S._lib.spmv_csr_from_diag(-1, d_v.ptr,
                                     C.byref(out)) == -errno.EINVAL
    assert out.value is None and S._lib.spmv_live_handles() == before
    assert S._lib.spmv_csr_from_diag(3, d_v.ptr, None) == -errno.EINVAL
    assert S._lib.spmv_live_handles() == before
    d_v.free()
    for h in (dup, unsorted, both, bad, gone, tall, other):
        h.release()
    assert S._lib.spmv_live_handles() == live
    with pytest.raises(TypeError):
        dA.add(B)
    # the operands are unchanged, and a released one is refused
    assert same(arrays(dA), A[2:]) and same(arrays(dB), B[2:])
    for h in (dB, dA):
        h.release()
    with pytest.raises(OSError) as ei:
        dA.add(dA)
    assert ei.value.errno == errno.EINVAL
