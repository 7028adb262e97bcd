"""The multicolour ordering (spmv_csr_colour, spmv_csr_permute,
spmv_permute_vectors; spmv_engine.h): what can be checked without a GPU -- the
declared surface, the binding's argument checks, the answers without a device,
and the properties of the numpy restatement of tests/_colour.py that make it a
colouring worth comparing the device with.  The kernels themselves:
tests/test_gpu_colour.py, tests/test_gpu_permute.py."""
import ctypes as C
import errno

import numpy as np
import pytest

import _colour as CO
import _trsv as TV
import spmv_scpa_amd as S

SYMBOLS = ("spmv_csr_colour", "spmv_csr_permute", "spmv_permute_vectors")


def test_the_headers_declare_the_entry_points():
    declared = S.declared_symbols()
    for name in SYMBOLS:
        assert name in declared and hasattr(S._lib, name), name
    assert S.check_symbols()
    # the feature is detected by the symbols, not by the version string
    assert S.version() == "spmv_scpa_amd 0.7 gfx950"
    assert callable(S.CsrDevice.colour) and callable(S.CsrDevice.permute)
    assert callable(S.permute_vectors)
    assert [f for f, _ in S.ColourInfo._fields_] == \
        ["colours", "rounds", "widest", "narrowest"]
    assert C.sizeof(S.ColourInfo) == 16


def test_the_binding_checks_its_arguments():
    fake = object.__new__(S.CsrDevice)  # a wrapper around no handle
    fake.h = None
    for kw in (dict(max_rounds=-1), dict(seed=-1), dict(seed=1 << 32)):
        with pytest.raises(ValueError):
            fake.colour(**kw)
    with pytest.raises(ValueError):
        fake.permute(rows="no pointer")
    with pytest.raises(OSError) as ei:
        fake.permute()
    assert ei.value.errno == errno.EINVAL  # the library's answer to NULL
    # pointers nothing ever follows: every call is refused before the C call
    p, a, b = 4096, 8192, 12288
    for k in (0, 9, -1):
        with pytest.raises(ValueError):
            S.permute_vectors(p, a, b, 5, k=k)
    with pytest.raises(ValueError):
        S.permute_vectors(p, a, a, 5)           # d_in is d_out
    for kw in (dict(ldin=2), dict(ldout=2)):
        with pytest.raises(ValueError):
            S.permute_vectors(p, a, b, 5, k=3, **kw)
    with pytest.raises(ValueError):
        S.permute_vectors(p, a, b, -1)
    for args in ((None, a, b), (p, None, b), (p, a, None)):
        with pytest.raises(ValueError):
            S.permute_vectors(*args, 5)


def test_dead_handles_and_argument_errors_of_the_library():
    junk = C.cast(C.create_string_buffer(512), C.c_void_p)
    dead = -errno.EBADF if S.device_count() > 0 else -errno.ENODEV
    before = S._lib.spmv_live_handles()
    colour, permute = S._lib.spmv_csr_colour, S._lib.spmv_csr_permute
    vectors = S._lib.spmv_permute_vectors
    info, out = S.ColourInfo(7, 7, 7, 7), C.c_void_p(1234)
    assert colour(None, 0, 0, None, None, None) == -errno.EINVAL
    assert colour(junk, 0, -1, None, None, C.byref(info)) == -errno.EINVAL
    assert colour(junk, 0, 0, None, None, C.byref(info)) == dead
    assert (info.colours, info.rounds, info.widest, info.narrowest) == \
        (7, 7, 7, 7)
    assert permute(None, None, None, C.byref(out)) == -errno.EINVAL
    assert permute(junk, None, None, None) == -errno.EINVAL
    assert permute(junk, None, None, C.byref(out)) == dead
    assert out.value is None  # *out is NULL after an error
    # the argument errors of launch_multi, and d_in == d_out, come first
    p, a, b = 4096, 8192, 12288
    for M, k, ldin, ldout, d_in, d_out in (
            (5, 0, 0, 0, a, b), (5, 9, 0, 0, a, b), (5, 3, 2, 0, a, b),
            (5, 3, 0, 2, a, b), (5, 1, 0, 0, None, b), (5, 1, 0, 0, a, None),
            (5, 1, 0, 0, a, a), (-1, 1, 0, 0, a, b)):
        assert vectors(p, M, k, 0, d_in, ldin, d_out, ldout, None) == \
            -errno.EINVAL
    assert vectors(None, 5, 1, 0, a, 0, b, 0, None) == -errno.EINVAL
    if S.device_count() == 0:
        assert vectors(p, 5, 1, 0, a, 0, b, 0, None) == -errno.ENODEV
    assert S._lib.spmv_live_handles() == before


# ------------------------------------------------------------ the reference
def test_fmix32_is_a_bijection_on_16_bits_and_is_murmur3s():
    h = CO.fmix32(np.arange(1 << 16, dtype=np.uint32))
    assert h.dtype == np.uint32 and len(np.unique(h)) == 1 << 16
    # the finaliser written out once in Python integers
    for x in (0, 1, 2, 0xdeadbeef, 0xffffffff):
        y = x
        y ^= y >> 16
        y = (y * 0x85ebca6b) & 0xffffffff
        y ^= y >> 13
        y = (y * 0xc2b2ae35) & 0xffffffff
        y ^= y >> 16
        assert int(CO.fmix32(np.array([x], np.uint32))[0]) == y
    assert int(CO.fmix32(np.array([0], np.uint32))[0]) == 0


@pytest.mark.parametrize("name", list(CO.MATRICES))
@pytest.mark.parametrize("seed", [0, 1])
def test_the_restatement_is_a_colouring_that_bounds_the_levels(name, seed):
    mat, colour, rnd, new_of_old = CO.reference(name, seed)
    M, IRP, JA, AS = mat
    colours = int(colour.max()) + 1
    assert colour.min() == 0 and rnd.min() == 1
    assert CO.same_colour_edges(M, IRP, JA, colour) == 0
    assert colours <= CO.max_degree(M, IRP, JA) + 1
    assert sorted(new_of_old.tolist()) == list(range(M))
    assert np.all(np.diff(colour[np.argsort(new_of_old)]) >= 0)
    B = CO.reference_permute(mat, new_of_old, new_of_old)
    for uplo in ("lower", "upper"):
        plan = TV.reference_plan(B[1], B[2], B[3].astype(np.float64), uplo)
        levels = len(plan["level_ptr"]) - 1
        print(name, seed, uplo, "colours", colours, "rounds", int(rnd.max()),
              "levels", levels)
        assert levels <= colours, (name, seed, uplo)


@pytest.mark.parametrize("seed", [0, 1])
def test_the_figures_of_the_small_stencil_and_the_clique(seed):
    _, colour, rnd, _ = CO.reference("lap2d(37,29)", seed)
    assert (int(colour.max()) + 1, int(rnd.max())) == (4, 9)
    _, colour, rnd, _ = CO.reference("clique(70)", seed)
    assert (int(colour.max()) + 1, int(rnd.max())) == (70, 70)
    assert sorted(colour.tolist()) == list(range(70))


def test_the_seed_changes_the_colouring():
    a = CO.reference("lap2d(37,29)", 0)[1]
    b = CO.reference("lap2d(37,29)", 1)[1]
    assert not np.array_equal(a, b)


def test_one_sided_adjacency_is_not_a_colouring_of_the_bidiagonal():
    """what tests/test_gpu_colour.py relies on: read from A alone, the
    bidiagonal matrix gets another, invalid, colouring"""
    mat, colour, _, _ = CO.reference("lower_bidiagonal(300)", 0)
    M, IRP, JA, _ = mat
    wrong = CO.reference_colour(M, IRP, JA, 0, adjacency=CO.one_sided)[0]
    assert not np.array_equal(wrong, colour)
    assert CO.same_colour_edges(M, IRP, JA, wrong) > 0
    assert int(colour.max()) + 1 <= 3   # a path: degree 2


def test_the_permutation_is_two_stable_sorts():
    # 3 x 4, unsorted, a duplicate (0, 3) and an explicit zero
    mat = (3, np.array([0, 4, 4, 6], np.int32),
           np.array([3, 0, 3, 1, 2, 0], np.int32),
           np.array([1.0, 2.0, 3.0, 0.0, 5.0, 6.0]))
    p, q = np.array([2, 0, 1]), np.array([1, 3, 0, 2])
    M, IRP, JA, AS = CO.reference_permute(mat, p, q, N=4)
    assert IRP.tolist() == [0, 0, 2, 6]
    assert JA.tolist() == [0, 1, 1, 2, 2, 3]
    assert AS.tolist() == [5.0, 6.0, 2.0, 1.0, 3.0, 0.0]
    # neither: the rows stably sorted by column, (A^T)^T
    M, IRP, JA, AS = CO.reference_permute(mat, N=4)
    assert IRP.tolist() == [0, 4, 4, 6] and JA.tolist() == [0, 1, 3, 3, 0, 2]
    assert AS.tolist() == [2.0, 0.0, 1.0, 3.0, 6.0, 5.0]
    # the values keep their type and their bits
    weird = np.array([-0.0, 5e-324, np.nan, 1.0, 2.0, 3.0])
    weird.view(np.uint64)[2] |= 0x1234
    out = CO.reference_permute(mat[:3] + (weird,), p, q, N=4)[3]
    assert sorted(out.view(np.uint64).tolist()) == \
        sorted(weird.view(np.uint64).tolist())
    f32 = CO.reference_permute(mat[:3] + (weird.astype(np.float32),), p, q,
                               N=4)[3]
    assert f32.dtype == np.float32
