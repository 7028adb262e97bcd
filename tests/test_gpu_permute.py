"""B = P A Q^T on the device and the permutation of vector blocks
(spmv_csr_permute, spmv_permute_vectors; spmv_engine.h) against the numpy
restatement of tests/_colour.py: index arrays as integers, values as uint64,
no tolerance anywhere.  The last test walks the whole route of the README:
colour, permute, ic0, the two plans, the vectors into the new numbering, the
preconditioned solve, the vectors back.

Every test runs under a time limit of its own (LIMIT_S): a test that exceeds
it ends the whole process, so nothing else is started on the device.
"""
import ctypes as C
import errno
import faulthandler

import numpy as np
import pytest

import _cg as G
import _colour as CO
import _ic0 as IC
import _pcg as PG
import _pcg_trsv as PT
import _trsv as TV
import spmv_scpa_amd as S

pytestmark = pytest.mark.gpu

LIMIT_S = 120
GROUP = S.trsv_shape()["group"]


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def upload(mat, values="f64", N=None):
    M, IRP, JA, AS = mat
    A = S.csr_from_arrays("permute", M, M if N is None else N, IRP, JA, AS)
    d = S.CsrDevice.upload(A, values=values)
    S.csr_free(A)
    return d


def arrays(d):
    """(IRP, JA, AS) of a handle, copied out of its download (f32 values
    widened: exact, so equal bits there are equal bits here)"""
    p = d.download()
    assert (p.contents.M, p.contents.N, p.contents.NZ) == (d.M, d.N, d.NZ)
    out = tuple(a.copy() for a in S.csr_arrays(p))
    S.csr_free(p)
    return out


def same_matrix(d, want, tag):
    IRP, JA, AS = arrays(d)
    assert IRP.dtype == JA.dtype == np.int32, tag
    assert np.array_equal(IRP, want[1]) and np.array_equal(JA, want[2]), tag
    assert np.array_equal(bits(AS), bits(want[3])), tag


def perm_buffer(p):
    return S.DevBuffer.from_numpy(np.ascontiguousarray(p, np.int32))


def rectangular(M=50, N=70, seed=4):
    """unsorted rows with duplicates, explicit zeros, -0.0, subnormals of
    both value types and a NaN with a payload; some rows empty"""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(M):
        n = int(rng.integers(0, 12)) if i % 9 else 0
        cols = rng.integers(0, N, n).tolist()
        if n >= 3:
            cols[2] = cols[0]  # a duplicate, apart in the row
        rows.append([(c, float(rng.uniform(-1.0, 1.0))) for c in cols])
    M_, IRP, JA, AS = TV.from_rows(rows)
    AS[3], AS[10], AS[17], AS[23], AS[31] = 0.0, -0.0, 5e-324, 1e-40, np.nan
    AS.view(np.uint64)[31] |= 0x0000123400000000  # survives a round to fp32
    return (M, IRP, JA, AS)


@pytest.mark.parametrize("values", ["f64", "f32"])
def test_the_bytes_of_two_stable_sorts(values):
    M, N = 50, 70
    mat = rectangular(M, N)
    rng = np.random.default_rng(8)
    p, q = rng.permutation(M), rng.permutation(N)
    d = upload(mat, values, N)
    src = (M,) + arrays(d)  # what the handle holds: rounded once for f32
    assert np.isnan(src[3][31]) and np.signbit(src[3][10])
    if values == "f64":
        assert np.array_equal(bits(src[3]), bits(mat[3]))
    d_p, d_q = perm_buffer(p), perm_buffer(q)
    live = S._lib.spmv_live_handles()
    for tag, rows, cols, rp, cq in (
            ("both", d_p, d_q, p, q), ("rows", d_p.ptr, None, p, None),
            ("columns", None, d_q, None, q), ("neither", None, None, None,
                                              None)):
        B = d.permute(rows, cols)
        assert S._lib.spmv_live_handles() == live + 1
        assert (B.M, B.N, B.NZ, B.value_bytes) == (M, N, d.NZ, d.value_bytes)
        same_matrix(B, CO.reference_permute(src, rp, cq, N=N), (values, tag))
        if tag == "neither":  # (A^T)^T
            T = d.transpose()
            TT = T.transpose()
            same_matrix(B, (M,) + arrays(TT), (values, "transposed twice"))
            TT.release()
            T.release()
        if tag == "both":  # an ordinary handle: y = B x
            x = np.random.default_rng(2).uniform(-1.0, 1.0, N)
            keep = np.isfinite(src[3])
            rows_of = np.repeat(np.arange(M), np.diff(src[1]))
            want = np.zeros(M)
            np.add.at(want, p[rows_of[keep]],
                      src[3][keep] * x[q[src[2][keep]]])
            nanrow = p[rows_of[~keep]]
            d_x, d_y = S.DevBuffer.from_numpy(x), S.DevBuffer(M * 8)
            B.launch(2, d_x.ptr, d_y.ptr)
            S.stream_sync()
            y = d_y.to_numpy(np.float64, M)
            assert np.all(np.isnan(y[nanrow]))
            ok = np.ones(M, bool)
            ok[nanrow] = False
            assert np.allclose(y[ok], want[ok], rtol=1e-12, atol=1e-12)
            d_x.free()
            d_y.free()
        B.release()
        assert S._lib.spmv_live_handles() == live
    # there and back: the row-sorted source
    inv_p, inv_q = np.argsort(p), np.argsort(q)
    d_ip, d_iq = perm_buffer(inv_p), perm_buffer(inv_q)
    B = d.permute(d_p, d_q)
    back = B.permute(d_ip, d_iq)
    same_matrix(back, CO.reference_permute(src, N=N), (values, "back"))
    for h in (back, B, d):
        h.release()
    for b in (d_p, d_q, d_ip, d_iq):
        b.free()


def test_no_entries_and_no_rows():
    live = S._lib.spmv_live_handles()
    empty = (3, np.zeros(4, np.int32), np.zeros(0, np.int32), np.zeros(0))
    d = upload(empty, N=4)
    d_p, d_q = perm_buffer([2, 0, 1]), perm_buffer([1, 3, 0, 2])
    for rows, cols in ((d_p, d_q), (None, None)):
        B = d.permute(rows, cols)
        assert (B.M, B.N, B.NZ) == (3, 4, 0)
        assert arrays(B)[0].tolist() == [0, 0, 0, 0]
        B.release()
    d.release()
    d = upload(TV.empty())
    for rows, cols in ((d_p, d_q), (None, None)):  # nothing of them is read
        B = d.permute(rows, cols)
        assert (B.M, B.N, B.NZ) == (0, 0, 0)
        assert arrays(B)[0].tolist() == [0]
        B.release()
    d.release()
    d_p.free()
    d_q.free()
    assert S._lib.spmv_live_handles() == live


def test_the_coloured_stencil_is_the_host_permuted_one_and_factors():
    mat, colour, _, new_of_old = CO.reference("lap2d(37,29)", 0)
    M = mat[0]
    d = upload(mat)
    col = d.colour()
    assert np.array_equal(col.perm.to_numpy(np.int32, M), new_of_old)
    B = d.permute(col, col)
    host = IC.permuted(mat, new_of_old.astype(np.int64))
    same_matrix(B, host, "P A P^T")
    L, info = B.ic0()  # rows strictly ascending, the diagonal stored
    F = IC.reference_ic0(*host)
    assert np.array_equal(bits(arrays(L)[2]), bits(F.AS))
    assert info.bad_pivots == 0 and info.levels <= col.colours
    LT = L.transpose()
    plans = [B.trsv_analyse("lower"), B.trsv_analyse("upper"),
             L.trsv_analyse("lower"), LT.trsv_analyse("upper")]
    for plan in plans:
        print("levels", plan.info["levels"], "colours", col.colours,
              "launches", plan.info["launches"])
        assert plan.info["levels"] <= col.colours == 4
    # against the natural order: 37 + 29 - 1 levels
    natural = d.trsv_analyse("lower")
    assert natural.info["levels"] == 65
    for h in plans + [natural, LT, L, B, col, d]:
        h.release()


def test_what_is_no_permutation_is_refused():
    mat = rectangular(50, 70)
    M, N = 50, 70
    d = upload(mat, N=N)
    good_p, good_q = perm_buffer(np.arange(M)[::-1]), perm_buffer(np.arange(N))
    live = S._lib.spmv_live_handles()
    permute = S._lib.spmv_csr_permute
    out = C.c_void_p(77)

    def refused(rows, cols):
        out.value = 77
        rc = permute(d.h, rows and rows.ptr, cols and cols.ptr, C.byref(out))
        assert out.value is None and S._lib.spmv_live_handles() == live, rc
        return -rc

    for n, which in ((M, "rows"), (N, "columns")):
        def call(buf):
            return refused(buf, good_q) if which == "rows" \
                else refused(good_p, buf)
        p = np.arange(n)
        p[n // 2] = n                      # == its range
        bad = perm_buffer(p)
        assert call(bad) == errno.EDOM, which
        bad.free()
        p[n // 2] = -1
        bad = perm_buffer(p)
        assert call(bad) == errno.EDOM, which
        bad.free()
        p[n // 2] = n - 1                  # twice n - 1, n // 2 is missing
        bad = perm_buffer(p)
        assert call(bad) == errno.EINVAL, which
        bad.free()
    # a column of A outside [0, N) is the transposition's -EDOM
    far = upload((3, np.array([0, 1, 3, 4]), np.array([0, 1, 5, 2]),
                  np.ones(4)))
    live += 1
    out.value = 77
    assert permute(far.h, None, None, C.byref(out)) == -errno.EDOM
    three = perm_buffer([2, 0, 1])
    assert permute(far.h, three.ptr, three.ptr, C.byref(out)) == -errno.EDOM
    assert out.value is None and S._lib.spmv_live_handles() == live
    junk = C.cast(C.create_string_buffer(512), C.c_void_p)
    assert permute(junk, None, None, C.byref(out)) == -errno.EBADF
    gone = upload(G.lap2d(9, 7, 0.5))
    try:
        S.set_panel_schedule("chain")
        gone.build_panels(0)
        gone.release_source()
    finally:
        S.set_panel_schedule("sweep")
    assert permute(gone.h, None, None, C.byref(out)) == -errno.ENODATA
    assert out.value is None
    # and what is refused nowhere
    B = d.permute(good_p, good_q)
    assert (B.M, B.N, B.NZ) == (M, N, d.NZ)
    B.release()
    for h in (gone, far, d):
        h.release()
    for b in (three, good_p, good_q):
        b.free()


@pytest.mark.parametrize("k", [1, 3, 8])
def test_vectors_go_into_the_new_numbering_and_back(k):
    M, pad_rows = 1073, 5
    rng = np.random.default_rng(k)
    p = rng.permutation(M)
    d_p = perm_buffer(p)
    for ld in (k, k + 2):
        src = rng.uniform(-1.0, 1.0, (M + pad_rows, ld))
        src[7, 0], src[11, k - 1], src[M - 1, 0] = np.nan, -0.0, 5e-324
        src.view(np.uint64)[7, 0] |= 0x1234
        fill = np.full((M + pad_rows, ld), -7.5)
        d_in = S.DevBuffer.from_numpy(src)
        d_fw, d_bk = S.DevBuffer.from_numpy(fill), S.DevBuffer.from_numpy(fill)
        S.permute_vectors(d_p, d_in, d_fw, M, k, ldin=ld, ldout=ld)
        S.permute_vectors(d_p.ptr, d_fw.ptr, d_bk.ptr, M, k, inverse=True,
                          ldin=ld, ldout=0 if ld == k else ld)
        S.stream_sync()
        fw = d_fw.to_numpy(np.float64, fill.size).reshape(fill.shape)
        bk = d_bk.to_numpy(np.float64, fill.size).reshape(fill.shape)
        want = fill.copy()
        want[p, :k] = src[:M, :k]
        assert np.array_equal(bits(fw), bits(want)), (k, ld, "forward")
        want = fill.copy()
        want[:M, :k] = src[:M, :k]
        assert np.array_equal(bits(bk), bits(want)), (k, ld, "and back")
        # a captured call replays to the same bytes
        d_g = S.DevBuffer.from_numpy(fill)
        st = S.Stream()
        with st.capture() as g:
            S.permute_vectors(d_p, d_in, d_g, M, k, ldin=ld, ldout=ld,
                              stream=st.ptr)
        g.launch(st.ptr)
        st.sync()
        got = d_g.to_numpy(np.float64, fill.size).reshape(fill.shape)
        assert np.array_equal(bits(got), bits(fw)), (k, ld, "captured")
        g.destroy()
        for b in (d_in, d_fw, d_bk, d_g):
            b.free()
    d_p.free()


def test_the_whole_route_has_the_bits_of_the_restatement():
    k, tol, maxit = 3, 1e-8, 300
    mat = PG.scaled_lap2d(37, 29, 0.01, 3, 5)
    M = mat[0]
    mat = (M, mat[1].astype(np.int32), mat[2].astype(np.int32), mat[3])
    new_of_old = CO.reference_colour(M, mat[1], mat[2], 0)[2]
    host = IC.permuted(mat, new_of_old.astype(np.int64))
    B, X0 = G.common_inputs(M, k)
    Bp = np.empty_like(B)
    Bp[new_of_old] = B
    # the seven lines of the README
    dA = upload(mat)
    d_b, d_pb = S.DevBuffer.from_numpy(B), S.DevBuffer(M * k * 8)
    d_px, d_x = S.DevBuffer.from_numpy(X0), S.DevBuffer(M * k * 8)
    col = dA.colour()
    dB = dA.permute(col, col)
    dL, ic = dB.ic0()
    dLT = dL.transpose()
    lo, up = dL.trsv_analyse("lower"), dLT.trsv_analyse("upper")
    S.permute_vectors(col.perm, d_b, d_pb, M, k)
    info = dB.pcg_trsv(d_pb.ptr, d_px.ptr, lo, up, k=k, tol=tol, maxit=maxit)
    S.permute_vectors(col.perm, d_px, d_x, M, k, inverse=True)
    S.stream_sync()
    assert np.array_equal(col.perm.to_numpy(np.int32, M), new_of_old)
    same_matrix(dB, host, "P A P^T")
    assert np.array_equal(bits(d_pb.to_numpy(np.float64, M * k)),
                          bits(Bp.ravel()))
    # the restatement on the host-permuted matrix, the product from the device
    d_P, d_Q = S.DevBuffer(M * k * 8), S.DevBuffer(M * k * 8)

    def product(P):
        P = np.ascontiguousarray(P)
        S._check(S._lib.spmv_copy_h2d(d_P.ptr, P.ctypes.data, P.nbytes), "h2d")
        dB.launch_multi(d_P.ptr, d_Q.ptr, k)
        S.stream_sync()
        return d_Q.to_numpy(np.float64, M * k).reshape(M, k)

    want = PT.restate(product, lambda: Bp.copy(), Bp, X0,
                      PT.plans_apply(*PT.ic0(host), GROUP), tol, maxit)
    Xp = d_px.to_numpy(np.float64, M * k).reshape(M, k)
    print("iterations", [r.iterations for r in info], "levels",
          lo.info["levels"], up.info["levels"], "colours", col.colours)
    assert [r.status for r in info] == want.status.tolist()
    assert [r.iterations for r in info] == want.iterations.tolist()
    assert max(want.iterations) > 0 and want.status[0] == 0
    assert np.array_equal(bits([r.rr for r in info]), bits(want.rr))
    assert np.array_equal(bits([r.bb for r in info]), bits(want.bb))
    assert np.array_equal(bits(Xp), bits(want.X))
    X = d_x.to_numpy(np.float64, M * k).reshape(M, k)
    assert np.array_equal(bits(X), bits(want.X[new_of_old]))
    assert lo.info["levels"] <= col.colours and \
        up.info["levels"] <= col.colours
    for h in (lo, up, dLT, dL, dB, col, dA):
        h.release()
    for b in (d_b, d_pb, d_px, d_x, d_P, d_Q):
        b.free()
