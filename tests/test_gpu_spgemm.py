"""The sparse product of CSR handles on the GPU (spmv_csr_spgemm,
spmv_csr_galerkin; spmv_engine.h).

The result is defined to the bit (tests/_spgemm.py reference), so everything
is compared through download() as int32 arrays and uint64 views of the values:
THERE IS NO TOLERANCE here, except where a launch of the result is checked
against the CPU oracle's product of the downloaded arrays (the bound of
tests/test_gpu_parity.py) and where a solve has to reach its tol.

The shapes are those of tests/_spgemm.py, which the CPU test
(tests/test_spgemm.py) holds to what they are for.  No test provokes a fault:
every error case returns before a launch that could misbehave.  Every test
runs under a time limit of its own (LIMIT_S): a test that exceeds it ends the
whole process, so nothing else is started on the device.
"""
import ctypes as C
import errno
import faulthandler

import numpy as np
import pytest

import _cg as G
import _oracle as O
import _spgemm as SG
import _transpose as TR
import spmv_scpa_amd as S
from test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

LIMIT_S = 240
SHAPE = S.spgemm_shape()


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(LIMIT_S, exit=True)
    yield
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


def check_product(A, B, want=None, values=("f64", "f64")):
    """upload, multiply, compare with the reference; -> (C's arrays, info)"""
    dA, dB = upload(A, values[0]), upload(B, values[1])
    live = S._lib.spmv_live_handles()
    dC = dA.matmul(dB)
    assert S._lib.spmv_live_handles() == live + 1
    assert (dC.M, dC.N) == (A[0], B[1]) and dC.value_bytes == 8
    if want is None:  # the f32 handles' values, widened
        want = SG.reference(A[:4] + (arrays(dA)[2],), B[:4] + (arrays(dB)[2],))
    got = arrays(dC)
    info = dC.spgemm_info
    assert same(got, want)
    assert info.nz == dC.NZ == len(want[1])
    ub = SG.upper_bounds(A, B)
    assert info.products == int(ub.sum())
    assert info.widest == (int(ub.max()) if len(ub) else 0)
    assert info.rows_in_bin == SG.rows_in_bin(A, B, SHAPE)
    for h in (dC, dB, dA):
        h.release()
    assert S._lib.spmv_live_handles() == live - 2
    return got, info


# ------------------------------------------------------------ 1. the bits
def test_rows_at_every_class_edge():
    A, B, what = SG.class_edges(SHAPE)
    got, info = check_product(A, B)
    assert np.diff(got[0]).tolist() == [w[1] for w in what]
    assert all(n > 0 for n in info.rows_in_bin)


def test_the_same_row_has_the_same_bits_in_every_class():
    A, B, pads = SG.padded(SHAPE)
    (I, J, V), info = check_product(A, B)
    assert info.rows_in_bin == (1, 1, 1, 1)
    rows = [(J[I[r]:I[r + 1]], V[I[r]:I[r + 1]]) for r in range(4)]
    for j, v in rows[1:]:
        keep = j != SG.PAD_COL
        assert np.array_equal(j[keep], rows[0][0])
        assert np.array_equal(bits(v[keep]), bits(rows[0][1]))


def test_columns_that_share_one_home_slot_and_fill_the_table():
    A, B = SG.collisions(SHAPE)
    (I, J, V), info = check_product(A, B)
    assert np.diff(I).tolist() == SHAPE["edges"]
    assert info.rows_in_bin == (1, 1, 1, 0)


def test_the_sum_is_sequential_in_walk_order():
    A, B = SG.order()
    (I, J, V), _ = check_product(A, B)
    for r in range(A[0]):
        seq, rev, pair = SG.sums3(A[4][4 * r:4 * r + 4])
        assert V[r] == seq and V[r] != rev and V[r] != pair


@pytest.mark.parametrize("name", list(SG.structure()))
def test_structure(name):
    A, B = SG.structure()[name]
    (I, J, V), info = check_product(A, B)
    if name in ("only empty rows of B", "0 x K", "M x 0", "K = 0", "A empty",
                "B empty"):
        assert info.nz == 0 and len(I) == A[0] + 1 and not I.any()


def test_a_wide_n_and_more_than_one_fallback_batch():
    A, B, want = SG.cached_reference("wide n")
    (I, J, V), info = check_product(A, B, want)
    assert B[1] == 2 ** 24 + 1 and J.max() == 2 ** 24
    assert info.rows_in_bin[3] == 10


def test_special_values():
    A, B = SG.special()
    (I, J, V), _ = check_product(A, B)
    assert np.count_nonzero(np.isnan(V)) == 2
    assert bits(V[I[1]:I[2]]).tolist() == [0x8000_0000_0000_0000]
    assert bits(V[I[0]:I[1]]).tolist() == [0]


def test_identities_on_the_device():
    A = SG.dedup(SG.random_unsorted(50, 40, 8, 30))
    A[4][::7] = np.inf
    got, _ = check_product(A, SG.identity(40))
    assert same(got, TR.row_sorted(*A[2:]))
    B = SG.random_sorted(40, 33, 6, 31)
    got, _ = check_product(SG.identity(40), B)
    assert same(got, B[2:])
    # (A B)^T == B^T A^T, every step on the device
    As = SG.random_sorted(50, 40, 8, 32)
    dA, dB = upload(As), upload(B)
    dAB = dA.matmul(dB)
    dABT, dAT, dBT = dAB.transpose(), dA.transpose(), dB.transpose()
    dBTAT = dBT.matmul(dAT)
    assert same(arrays(dABT), arrays(dBTAT))
    # the handle passed twice
    sq = SG.random_sorted(40, 40, 6, 33)
    dS = upload(sq)
    dSS = dS.matmul(dS)
    assert same(arrays(dSS), SG.reference(sq, sq))
    for h in (dSS, dS, dBTAT, dBT, dAT, dABT, dAB, dB, dA):
        h.release()


@pytest.mark.parametrize("values", [("f32", "f64"), ("f64", "f32"),
                                    ("f32", "f32")])
def test_f32_operands_are_widened_exactly(values):
    A, B, _ = SG.class_edges(SHAPE)
    A2, B2, _ = SG.padded(SHAPE)
    for a, b in ((A, B), (A2, B2)):
        (I, J, V), _ = check_product(a, b, values=values)
        if values == ("f32", "f32"):
            assert not np.array_equal(bits(V), bits(SG.reference(a, b)[2]))


@pytest.mark.parametrize("name", ["hublike", "hub cut"])
def test_the_fallback_serves_hub_rows(name):
    A, B, want = SG.cached_reference(name)
    if name == "hublike":  # B = A^T, made on the device
        dA = upload(A)
        dB = dA.transpose()
        dC = dA.matmul(dB)
        assert same(arrays(dC), want)
        info = dC.spgemm_info
        for h in (dC, dB, dA):
            h.release()
    else:
        _, info = check_product(A, B, want)
    assert info.rows_in_bin[3] > 0
    assert info.rows_in_bin == SG.rows_in_bin(A, B, SHAPE)


# ------------------------------------------------------------- 2. galerkin
def test_galerkin_is_the_two_products_and_an_ordinary_handle():
    A, P = SG.galerkin_case()
    want = SG.galerkin_reference(A, P)
    dA, dP = upload(A), upload(P)
    live = S._lib.spmv_live_handles()
    dG = dA.galerkin(dP)
    assert S._lib.spmv_live_handles() == live + 1  # A P and P^T are gone
    gI, gJ, gA = got = arrays(dG)
    assert same(got, want)
    assert dG.NZ == 4992 and np.diff(gI).max() == 5
    assert gA[:3].tolist() == [8.0, -2.0, -2.0]
    dPT = dP.transpose()
    dG2 = dA.galerkin(dP, dPT)
    assert same(arrays(dG2), want)
    composed = dPT.matmul(dA.matmul(dP))  # the intermediate goes with the gc
    assert same(arrays(composed), want)
    # an ordinary handle: launch, and cg to its tol
    x = O.synth_x(7, 0, dG.N)
    d_x, d_y = S.DevBuffer.from_numpy(x), S.DevBuffer(dG.M * 8)
    for kernel in (0, 2):
        S._lib.spmv_dev_memset(d_y.ptr, 0xFF, dG.M * 8, None)
        dG.launch(kernel, d_x.ptr, d_y.ptr)
        S.stream_sync()
        assert_parity(d_y.to_numpy(np.float64, dG.M),
                      O.csr_spmv(gI, gJ, gA, x), O.csr_abs_spmv(gI, gJ, gA, x),
                      ("galerkin", kernel))
    tol = 1e-8
    Bm, X0 = G.common_inputs(dG.M, 2)
    d_B, d_X = S.DevBuffer.from_numpy(Bm), S.DevBuffer.from_numpy(X0)
    rec = dG.cg(d_B.ptr, d_X.ptr, 2, tol=tol, maxit=500)
    X = d_X.to_numpy(np.float64, dG.M * 2).reshape(dG.M, 2)
    res = G.true_residual(gI, gJ, gA, O.csr_spmv, Bm, X)
    print("cg on the coarse operator:", rec, "true residual", res)
    assert [r.status for r in rec] == [0, 0]
    assert all(r.rr <= tol * tol * r.bb for r in rec)
    assert np.all(res <= 2 * tol)  # the sanity line of test_gpu_cg
    for b in (d_x, d_y, d_B, d_X):
        b.free()
    for h in (composed, dG2, dPT, dG, dP, dA):
        h.release()


# --------------------------------------------------------------- 3. errors
def test_errors_in_order_create_nothing():
    A, B = SG.random_sorted(20, 15, 4, 40), SG.random_sorted(15, 9, 4, 41)
    dA, dB = upload(A), upload(B)
    live = S._lib.spmv_live_handles()
    fn = S._lib.spmv_csr_spgemm
    info = S.SpgemmInfo()
    info.nz = -77
    junk = C.cast(C.create_string_buffer(512), C.c_void_p)

    def refused(a, b, err, with_out=True):
        live = S._lib.spmv_live_handles()
        out = C.c_void_p(1234)
        rc = fn(a, b, C.byref(out) if with_out else None, C.byref(info))
        assert rc == -err, (rc, err)
        assert (out.value is None) == with_out
        assert S._lib.spmv_live_handles() == live and info.nz == -77

    refused(None, dB.h, errno.EINVAL)
    refused(dA.h, None, errno.EINVAL)
    refused(dA.h, dB.h, errno.EINVAL, with_out=False)
    refused(junk, dB.h, errno.EBADF)
    refused(dA.h, junk, errno.EBADF)
    refused(dB.h, dA.h, errno.EINVAL)  # 15 x 9 times 20 x 15
    # a column outside its range: A's beyond K, B's beyond N
    bad = upload((3, 15, TR.irp_of([1, 0, 1]), np.array([2, 15], np.int32),
                  np.ones(2)))
    refused(bad.h, dB.h, errno.EDOM)
    badB = upload((15, 9, TR.irp_of([2] + [0] * 14),
                   np.array([1, 9], np.int32), np.ones(2)))
    refused(dA.h, badB.h, errno.EDOM)
    # ... which comes before the order of B's rows
    both = upload((15, 9, TR.irp_of([3] + [0] * 14),
                   np.array([5, 4, -1], np.int32), np.ones(3)))
    refused(dA.h, both.h, errno.EDOM)
    # B unsorted, B with one duplicate
    unsorted = upload((15, 9, TR.irp_of([3] + [0] * 14),
                       np.array([1, 5, 4], np.int32), np.ones(3)))
    refused(dA.h, unsorted.h, errno.EINVAL)
    dup = upload((15, 9, TR.irp_of([0] * 14 + [3]),
                  np.array([1, 4, 4], np.int32), np.ones(3)))
    refused(dA.h, dup.h, errno.EINVAL)
    for h in (dup, unsorted, both, badB, bad):
        h.release()
    assert S._lib.spmv_live_handles() == live
    # after release_source: -ENODATA, from either side
    gone = upload(B)
    try:
        S.set_panel_schedule("chain")
        gone.build_panels(0)
        gone.release_source()
    finally:
        S.set_panel_schedule("sweep")
    refused(dA.h, gone.h, errno.ENODATA)
    sqr = upload(SG.random_sorted(9, 15, 3, 42))
    refused(gone.h, sqr.h, errno.ENODATA)
    live = S._lib.spmv_live_handles()
    # galerkin passes the errors of its calls on
    out = C.c_void_p(1234)
    assert S._lib.spmv_csr_galerkin(dA.h, dA.h, None, C.byref(out),
                                    None) == -errno.EINVAL
    assert out.value is None and S._lib.spmv_live_handles() == live
    # ... from each of them: a handle that is none as A, as P and as P^T, a
    # released source as P, a P^T of the wrong shape (the third and the last
    # after A P was made: it is released)
    dBT = dB.transpose()
    live += 1
    for err, args in ((errno.EBADF, (junk, dB.h, None)),
                      (errno.EBADF, (dA.h, junk, None)),
                      (errno.EBADF, (dA.h, dB.h, junk)),
                      (errno.ENODATA, (dA.h, gone.h, None)),
                      (errno.ENODATA, (dA.h, gone.h, dBT.h)),
                      (errno.EINVAL, (dA.h, dB.h, dB.h))):
        out = C.c_void_p(1234)
        assert S._lib.spmv_csr_galerkin(*args, C.byref(out),
                                        C.byref(info)) == -err, (err, args)
        assert out.value is None and info.nz == -77
        assert S._lib.spmv_live_handles() == live
    dBT.release()
    live -= 1
    with pytest.raises(TypeError):
        dA.matmul(B)
    # the operands are unchanged, and a released one is refused
    assert same(arrays(dA), A[2:]) and same(arrays(dB), B[2:])
    for h in (sqr, gone, dB, dA):
        h.release()
    with pytest.raises(OSError) as ei:
        dA.matmul(dA)
    assert ei.value.errno == errno.EINVAL


def test_more_entries_than_an_int_irp_holds_is_eoverflow():
    """46341 x 1 times 1 x 46341, full: the symbolic fallback runs over every
    row, the product has 46341^2 > INT32_MAX entries, nothing is allocated
    for C"""
    A, B = SG.overflow_case()
    dA, dB = upload(A), upload(B)
    live = S._lib.spmv_live_handles()
    with pytest.raises(OSError) as ei:
        dA.matmul(dB)
    assert ei.value.errno == errno.EOVERFLOW
    assert S._lib.spmv_live_handles() == live
    dB.release()
    dA.release()
