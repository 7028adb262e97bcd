"""The colouring on the device (spmv_csr_colour; spmv_engine.h) against the
numpy restatement of tests/_colour.py: colour, new_of_old and the four numbers
of the info compared as integers, at two seeds, from an f64 and an f32 handle,
twice.  The shapes are the smallest on which the rounds can go wrong: a stencil
(4 colours, 9 rounds, more than one workgroup), a 27-point grid, a hub row, a
clique of 70 (the second window of 64 colours, one row per round), a
bidiagonal matrix whose edges are stored on one side only, unsorted rows with
duplicates and explicit zeros, no rows, one row and no edges.

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
import spmv_scpa_amd as S

pytestmark = pytest.mark.gpu

LIMIT_S = 120
SENTINEL = -77


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def upload(mat, values="f64", N=None):
    M, IRP, JA, AS = mat
    A = S.csr_from_arrays("colour", M, M if N is None else N, IRP, JA, AS)
    d = S.CsrDevice.upload(A, values=values)
    S.csr_free(A)
    return d


def ints(buf, n):
    return buf.to_numpy(np.int32, n) if n else np.zeros(0, np.int32)


def sentinels(M):
    return S.DevBuffer.from_numpy(np.full(max(M, 4), SENTINEL, np.int32))


def raw(d, seed, cap, d_colour, d_perm, info=None):
    return S._lib.spmv_csr_colour(d.h, seed, cap,
                                  d_colour.ptr if d_colour else None,
                                  d_perm.ptr if d_perm else None,
                                  C.byref(info) if info else None)


def numbers(info):
    return info.colours, info.rounds, info.widest, info.narrowest


@pytest.mark.parametrize("name", list(CO.MATRICES) + list(CO.SMALL))
def test_the_colouring_has_the_integers_of_the_restatement(name):
    for seed in (0, 1):
        mat, colour, rnd, new_of_old = CO.reference(name, seed)
        M = mat[0]
        sizes = np.bincount(colour) if M else np.zeros(1, np.int64)
        want = (len(sizes) if M else 0, int(rnd.max()) if M else 0,
                int(sizes.max()), int(sizes.min()))
        for values in ("f64", "f32"):
            tag = (name, seed, values)
            d = upload(mat, values)
            live = S._lib.spmv_live_handles()
            for _ in range(2):  # the same bytes from two calls
                col = d.colour(seed=seed)
                got = (col.colours, col.rounds, col.widest, col.narrowest)
                print(tag, "colours, rounds, widest, narrowest", got)
                assert got == want, tag
                assert col.M == M
                assert np.array_equal(ints(col.colour, M), colour), tag
                assert np.array_equal(ints(col.perm, M), new_of_old), tag
                assert col in S.live_objects()
                col.release()
                assert col not in S.live_objects()
            # either array, both or the info may be NULL
            a, b, info = sentinels(M), sentinels(M), S.ColourInfo()
            assert raw(d, seed, 0, a, None, info) == 0 and \
                numbers(info) == want, tag
            assert np.array_equal(ints(a, M), colour), tag
            assert raw(d, seed, 0, None, b) == 0, tag
            assert np.array_equal(ints(b, M), new_of_old), tag
            assert raw(d, seed, 0, None, None) == 0, tag
            # nothing past M was written
            assert ints(a, max(M, 4))[M:].tolist() == \
                ints(b, max(M, 4))[M:].tolist() == [SENTINEL] * (max(M, 4) - M)
            assert S._lib.spmv_live_handles() == live, tag
            for h in (a, b, d):
                h.free() if isinstance(h, S.DevBuffer) else h.release()


def test_a_clique_takes_the_second_window_and_meets_the_cap():
    mat, colour, rnd, new_of_old = CO.reference("clique(70)", 0)
    M = mat[0]
    assert int(colour.max()) == 69 and int(rnd.max()) == 70
    d = upload(mat)
    live = S._lib.spmv_live_handles()
    a, b, info = sentinels(M), sentinels(M), S.ColourInfo(5, 5, 5, 5)
    assert raw(d, 0, 69, a, b, info) == -errno.E2BIG
    assert S._lib.spmv_live_handles() == live
    # the outputs are untouched
    assert numbers(info) == (5, 5, 5, 5)
    assert set(ints(a, M).tolist()) == set(ints(b, M).tolist()) == {SENTINEL}
    with pytest.raises(OSError) as ei:
        d.colour(max_rounds=1)
    assert ei.value.errno == errno.E2BIG
    assert raw(d, 0, 70, a, b, info) == 0
    assert numbers(info) == (70, 70, 1, 1)
    assert np.array_equal(ints(a, M), colour)
    assert np.array_equal(ints(b, M), new_of_old)
    assert S._lib.spmv_live_handles() == live
    a.free()
    b.free()
    d.release()


def test_an_edge_stored_on_one_side_is_an_edge():
    """(i, i - 1) is stored and (i - 1, i) is not: adjacency from A alone gives
    another colouring, in which neighbours share a colour"""
    mat, colour, _, _ = CO.reference("lower_bidiagonal(300)", 0)
    M, IRP, JA, _ = mat
    wrong = CO.reference_colour(M, IRP, JA, 0, adjacency=CO.one_sided)[0]
    assert not np.array_equal(wrong, colour)
    d = upload(mat)
    col = d.colour()
    got = ints(col.colour, M)
    assert CO.same_colour_edges(M, IRP, JA, got) == 0
    assert np.array_equal(got, colour)
    col.release()
    d.release()


def test_every_refusal_in_the_stated_order():
    mat = G.lap2d(9, 7, 0.5)
    M = mat[0]
    d = upload(mat)
    junk = C.cast(C.create_string_buffer(512), C.c_void_p)
    rect = upload((2, np.array([0, 1, 2]), np.array([0, 1]), np.ones(2)), N=3)
    gone = upload(mat)
    try:
        S.set_panel_schedule("chain")
        gone.build_panels(0)
        gone.release_source()
    finally:
        S.set_panel_schedule("sweep")
    far = upload((3, np.array([0, 1, 3, 4]), np.array([0, 1, 5, 2]),
                  np.ones(4)))       # a column outside [0, N), unsorted too
    live = S._lib.spmv_live_handles()
    a, b, info = sentinels(M), sentinels(M), S.ColourInfo(5, 5, 5, 5)
    colour = S._lib.spmv_csr_colour

    def refused(h, cap=0):
        rc = colour(h, 0, cap, a.ptr, b.ptr, C.byref(info))
        assert S._lib.spmv_live_handles() == live, rc
        assert numbers(info) == (5, 5, 5, 5), rc
        assert set(ints(a, M).tolist()) == set(ints(b, M).tolist()) == \
            {SENTINEL}, rc
        return -rc

    # the arguments come before everything, a dead handle before its shape
    assert refused(None) == errno.EINVAL
    assert refused(junk, cap=-1) == errno.EINVAL
    assert refused(junk) == errno.EBADF
    assert refused(rect.h) == errno.EINVAL
    assert refused(gone.h) == errno.ENODATA
    assert refused(far.h, cap=1) == errno.EDOM   # before any round is counted
    assert refused(d.h, cap=1) == errno.E2BIG
    assert colour(d.h, 0, 0, a.ptr, b.ptr, C.byref(info)) == 0
    assert info.colours >= 2 and S._lib.spmv_live_handles() == live
    for h in (rect, gone, far, d):
        h.release()
    a.free()
    b.free()
    with pytest.raises(OSError) as ei:
        d.colour()  # released: the binding passes NULL
    assert ei.value.errno == errno.EINVAL
