"""Sweep plans on the GPU (spmv_csr_trsv_analyse_sweeps, spmv_trsv_sweeps,
spmv_trsv_solve; spmv_engine.h): the triangular solve by a fixed number of
Jacobi sweeps.

The result is defined to the bit (tests/_trsv_sweeps.py: reference_sweeps), so
everything is compared as integer arrays and uint64 views: THERE IS NO
TOLERANCE here.  A NaN has no defined payload: where the reference holds a NaN
the device must hold one, every other value is compared by its bits.  The
central property: with at least as many sweeps as the exact plan of the same
triangle has levels, a sweep plan gives the exact solve's bits.

No test provokes a fault: every error case is an argument check that returns
before any launch.  Every test runs under a time limit of its own (LIMIT_S): a
test that exceeds it ends the whole process, so nothing else is started on the
device.
"""
import ctypes as C
import errno
import faulthandler

import numpy as np
import pytest

import _trsv as TV
import _trsv_sweeps as SW
import spmv_scpa_amd as S

pytestmark = pytest.mark.gpu

LIMIT_S = 240
SHAPE = S.trsv_shape()
L, GROUP = SHAPE["small_rows"], SHAPE["group"]
NAMES = list(TV.shapes(8))  # the names do not depend on L
UPLO = ("lower", "upper")
FILL = 0xFFF8_DEAD_BEEF_0001  # a NaN no solve produces: padding columns
PAST = 0xFFF8_DEAD_BEEF_0002  # and the guard rows behind row M - 1
GUARD = 2


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def shapes():
    return TV.shapes(L)


@pytest.fixture(scope="module")
def small():
    """the shapes held against the row loop in Python"""
    return {"lap": TV.lap(17, 13), "sandwich": TV.layered([3, 2, L + 7, 4, 1],
                                                          seed=9),
            "random": TV.random_triangle(600), "arrow": TV.arrow(300)}


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64).ravel()


def same_bits(got, want):
    """equal bit for bit, except that any NaN stands for any NaN"""
    nan = np.isnan(want)
    return (got.shape == want.shape and np.array_equal(np.isnan(got), nan)
            and np.array_equal(bits(got)[~nan.ravel()],
                               bits(want)[~nan.ravel()]))


def upload(mat, values="f64", N=None):
    M, IRP, JA, AS = mat
    A = S.csr_from_arrays("t", M, N or M, IRP, JA, AS)
    d = S.CsrDevice.upload(A, values=values)
    S.csr_free(A)
    return d


def rhs_of(M, k=8, seed=2):
    B = np.random.default_rng(seed).uniform(-1.0, 1.0, (M, k))
    if M:
        B[M // 2, 0] = -0.0
    return B


def scale_of(M):
    return np.random.default_rng(6).uniform(0.5, 2.0, M)


def padded(V, ld):
    """(M, k) values in an (M + GUARD, ld) array: FILL in the padding columns,
    PAST in the guard rows"""
    M, k = V.shape
    out = np.full((M + GUARD, ld), FILL, np.uint64)
    out[M:] = PAST
    out = out.view(np.float64)
    out[:M, :k] = V
    return out


def run(plan, B, k, ld=None, scale=None, in_place=False, waves=0, stream=None):
    """one solve of the first k columns of B -> X (M, k); the padding and the
    guard rows of X, and all of a B that is not X, must be what they were"""
    M = B.shape[0]
    ld = ld or k
    before = padded(B[:, :k], ld)
    d_B = S.DevBuffer.from_numpy(before)
    d_X = d_B if in_place else S.DevBuffer.from_numpy(
        padded(np.zeros((M, k)), ld))
    d_s = S.DevBuffer.from_numpy(scale) if scale is not None else None
    plan.solve(d_B.ptr, d_X.ptr, k, scale=d_s.ptr if d_s else None, ldb=ld,
               ldx=ld, waves_per_block=waves, stream=stream)
    S.stream_sync(stream)
    X = d_X.to_numpy(np.float64, (M + GUARD) * ld).reshape(M + GUARD, ld)
    assert np.all(bits(X[:M, k:]) == FILL), (k, ld)
    assert np.all(bits(X[M:]) == PAST), (k, ld)
    if not in_place:
        back = d_B.to_numpy(np.float64, (M + GUARD) * ld)
        assert np.array_equal(bits(back), bits(before))
    for b in {d_B, d_X, d_s} - {None}:
        b.free()
    return X[:M, :k].copy()


# ------------------------------- 1. enough sweeps are the exact solve's bits
@pytest.mark.parametrize("uplo", UPLO)
@pytest.mark.parametrize("name", NAMES)
def test_levels_sweeps_give_the_exact_solve_s_bits(shapes, name, uplo):
    mat = shapes[name]
    M = mat[0]
    B, scale = rhs_of(M, 3), scale_of(M)
    d = upload(mat)
    for unit in (False, True):
        exact = d.trsv_analyse(uplo, unit=unit)
        levels = exact.info["levels"]
        if M == 0:
            plan = d.trsv_analyse(uplo, unit=unit, sweeps=3)
            plan.solve(8, 8, 3)  # nothing to do: no pointer is read
            assert plan.info["levels"] == 0 and plan.info["launches"] == 3
            plan.release()
            exact.release()
            continue
        if name == "chain300":
            assert levels == 300
        want = {sc is not None: run(exact, B, 3, scale=sc)
                for sc in (None, scale)}
        for sweeps in (levels, levels + 3):
            plan = d.trsv_analyse(uplo, unit=unit, sweeps=sweeps, kmax=3)
            assert plan.info["launches"] == sweeps
            for sc in (None, scale):
                got = run(plan, B, 3, 4, scale=sc)
                assert same_bits(got, want[sc is not None]), \
                    (unit, sweeps, sc is not None)
            plan.release()
        exact.release()
    d.release()


def test_non_finite_right_hand_sides_keep_the_exact_bits(shapes):
    mat = shapes["sandwich"]
    M = mat[0]
    B = rhs_of(M, 3)
    B[1, 0], B[4, 1], B[M - 1, 2], B[2, 2] = np.nan, np.inf, -np.inf, np.nan
    d = upload(mat)
    for uplo in UPLO:
        exact = d.trsv_analyse(uplo)
        plan = d.trsv_analyse(uplo, sweeps=exact.info["levels"])
        assert same_bits(run(plan, B, 3), run(exact, B, 3)), uplo
        plan.release()
        exact.release()
    d.release()


# --------------------------------------------- 2. against the restatement
@pytest.mark.parametrize("values", ["f64", "f32"])
@pytest.mark.parametrize("name", ["lap", "sandwich", "random", "arrow"])
def test_a_few_sweeps_equal_the_restatement(small, name, values):
    """sweeps 1, 2, 3, 5; k = 1 / 3 / 8 with padded leading dimensions; unit
    and not, with and without scale; waves_per_block 1 / 4 / 16"""
    M, IRP, JA, AS = small[name]
    if values == "f32":
        AS = AS.astype(np.float32).astype(np.float64)
    B, scale = rhs_of(M), scale_of(M)
    d = upload(small[name], values)
    for uplo, unit, sc in (("lower", False, None), ("upper", False, scale),
                           ("lower", True, scale), ("upper", True, None)):
        rp = TV.reference_plan(IRP, JA, AS, uplo)
        for sweeps in (1, 2, 3, 5):
            want = SW.reference_sweeps(rp, B, sc, GROUP, sweeps, unit)
            plan = d.trsv_analyse(uplo, unit=unit, sweeps=sweeps)
            assert (plan.sweeps, plan.kmax) == (sweeps, 8)
            for k, ld, waves in ((1, 1, 0), (1, 3, 1), (3, 3, 4), (3, 5, 16),
                                 (8, 8, 1), (8, 11, 0)):
                got = run(plan, B, k, ld, scale=sc, waves=waves)
                assert same_bits(got, want[:, :k]), \
                    (uplo, unit, sweeps, k, ld, waves)
            plan.release()
    d.release()


def test_a_nan_lands_on_the_restatement_s_rows():
    mat = TV.random_triangle(600, dominant=True)
    M, IRP, JA, AS = mat
    rp = TV.reference_plan(IRP, JA, AS, "lower")
    r = int(rp["order"][0])
    steps = SW.steps_from(rp, r)
    B = rhs_of(M, 3)
    d = upload(mat)
    for sweeps in (1, 2, 3, 5):
        plan = d.trsv_analyse("lower", sweeps=sweeps)
        clean = run(plan, B, 3)
        B2 = B.copy()
        B2[r, 1] = np.nan
        X = run(plan, B2, 3)
        want = SW.reference_sweeps(rp, B2, None, GROUP, sweeps)
        hit = (steps >= 0) & (steps < sweeps)
        assert np.array_equal(np.isnan(want[:, 1]), hit)
        assert np.array_equal(np.isnan(X[:, 1]), hit), sweeps
        assert same_bits(X, want)
        assert np.array_equal(bits(X[:, [0, 2]]), bits(clean[:, [0, 2]]))
        plan.release()
    d.release()


def test_a_zero_diagonal_is_plain_arithmetic(small):
    M, IRP, JA, AS = small["sandwich"]
    r = 3
    keep = ~((np.repeat(np.arange(M), np.diff(IRP)) == r) & (JA == r))
    lens = np.diff(IRP)
    lens[r] -= 1
    mat = (M, TV.irp_of(lens), JA[keep], AS[keep])
    rp = TV.reference_plan(*mat[1:], "lower")
    assert rp["diag"][r] == 0.0
    B = rhs_of(M, 2)
    d = upload(mat)
    plan = d.trsv_analyse("lower", sweeps=3)
    assert plan.info["zero_diag"] == 1
    X = run(plan, B, 2)
    assert same_bits(X, SW.reference_sweeps(rp, B, None, GROUP, 3))
    assert not np.isfinite(X[r]).any() and np.isfinite(X).any()
    plan.release()
    d.release()


# ------------------------------------------------- 3. buffers and reuse
def test_in_place_equals_out_of_place(small):
    mat = small["random"]
    M = mat[0]
    B, scale = rhs_of(M), scale_of(M)
    d = upload(mat)
    for uplo in UPLO:
        for sweeps in (1, 2, 3, 4):
            plan = d.trsv_analyse(uplo, sweeps=sweeps)
            for k, ld, sc in ((1, 1, None), (3, 5, scale), (8, 8, scale)):
                out = run(plan, B, k, ld, scale=sc)
                inp = run(plan, B, k, ld, scale=sc, in_place=True)
                assert same_bits(inp, out), (uplo, sweeps, k)
            plan.release()
    d.release()


def test_one_plan_solves_k_1_then_8_then_3(small):
    M, IRP, JA, AS = small["lap"]
    B = rhs_of(M)
    rp = TV.reference_plan(IRP, JA, AS, "lower")
    want = SW.reference_sweeps(rp, B, None, GROUP, 4)
    d = upload(small["lap"])
    plan = d.trsv_analyse("lower", sweeps=4)
    for k in (1, 8, 3):
        assert same_bits(run(plan, B, k), want[:, :k]), k
    plan.release()
    d.release()


def test_a_captured_solve_replays_the_eager_bits(small):
    M, IRP, JA, AS = small["sandwich"]
    B = rhs_of(M, 3)
    want = SW.reference_sweeps(TV.reference_plan(IRP, JA, AS, "lower"), B,
                               None, GROUP, 3)
    d = upload(small["sandwich"])
    plan = d.trsv_analyse("lower", sweeps=3)
    side = S.Stream()
    d_B = S.DevBuffer.from_numpy(B)
    d_X = S.DevBuffer.from_numpy(np.zeros((M, 3)))
    plan.solve(d_B.ptr, d_X.ptr, 3, stream=side.ptr)  # one eager run
    side.sync()
    eager = d_X.to_numpy(np.float64, M * 3).reshape(M, 3)
    assert same_bits(eager, want)
    with side.capture(shape=True) as g:
        plan.solve(d_B.ptr, d_X.ptr, 3, stream=side.ptr)
    # the sweeps, one after the other: a single chain of nodes
    assert g.shape == dict(nodes=3, edges=2, roots=1, max_fanout=1)
    for _ in range(2):
        S._lib.spmv_dev_memset(d_X.ptr, 0xFF, M * 3 * 8, side.ptr)
        g.launch(side.ptr)
        side.sync()
        again = d_X.to_numpy(np.float64, M * 3).reshape(M, 3)
        assert np.array_equal(bits(again), bits(eager))
    g.destroy()
    for b in (d_B, d_X):
        b.free()
    plan.release()
    d.release()


# ----------------------------------------------- 4. what the plan reports
@pytest.mark.parametrize("values", ["f64", "f32"])
def test_info_download_and_sweeps(shapes, values):
    mat = shapes["random"]
    M, IRP, JA, AS = mat
    if values == "f32":
        AS = AS.astype(np.float32).astype(np.float64)
    d = upload(mat, values)
    exact = d.trsv_analyse("upper")
    assert (exact.sweeps, exact.kmax) == (0, 0)
    ex, base = exact.download(), exact.info
    exact.release()
    live = S._lib.spmv_live_handles()
    seen = {}
    for sweeps, kmax in ((1, 8), (2, 5), (3, 5), (7, 1)):
        plan = d.trsv_analyse("upper", sweeps=sweeps, kmax=kmax)
        assert S._lib.spmv_live_handles() == live + 1
        assert (plan.sweeps, plan.kmax) == (sweeps, kmax)
        info = plan.info
        assert info["M"] == M and info["levels"] == 1
        assert info["widest_level"] == M and info["launches"] == sweeps
        assert info["entries"] == base["entries"]
        assert info["zero_diag"] == base["zero_diag"]
        seen[sweeps] = info["bytes"] - min(sweeps - 1, 2) * 8 * kmax * M
        got = plan.download()
        assert not got["level"].any()
        assert np.array_equal(got["order"], np.arange(M))
        assert got["level_ptr"].tolist() == [0, M]
        assert np.array_equal(bits(got["diag"]), bits(ex["diag"]))
        # the strict entries of every row, in stored order, as the exact plan
        # holds them at the row's position
        pos = np.empty(M, np.int64)
        pos[ex["order"]] = np.arange(M)
        assert np.array_equal(np.diff(got["rowptr"]),
                              np.diff(ex["rowptr"])[pos])
        take = np.concatenate([np.arange(ex["rowptr"][p], ex["rowptr"][p + 1])
                               for p in pos])
        assert np.array_equal(got["ja"], ex["ja"][take])
        assert np.array_equal(bits(got["as"]), bits(ex["as"][take]))
        plan.release()
        assert S._lib.spmv_live_handles() == live
    assert len(set(seen.values())) == 1  # the rest does not depend on sweeps
    d.release()


# ------------------------------------------------------------ 5. refusals
def test_refusals(small):
    mat = small["sandwich"]
    M = mat[0]
    d = upload(mat)
    wide = upload(mat, N=M + 1)
    live = S._lib.spmv_live_handles()
    an = S._lib.spmv_csr_trsv_analyse_sweeps
    out = C.c_void_p(99)
    for sweeps, kmax in ((0, 8), (4097, 8), (-1, 8), (3, 0), (3, 9)):
        assert an(d.h, 0, 0, sweeps, kmax, C.byref(out)) == -errno.EINVAL
    assert out.value == 99  # refused before anything is written
    assert an(wide.h, 0, 0, 3, 8, C.byref(out)) == -errno.EINVAL  # M != N
    assert out.value is None
    junk = C.cast(C.create_string_buffer(512), C.c_void_p)
    assert an(junk, 0, 0, 3, 8, C.byref(out)) == -errno.EBADF
    assert S._lib.spmv_live_handles() == live
    wide.release()

    plan = d.trsv_analyse("lower", sweeps=3, kmax=4)
    buf = S.DevBuffer.from_numpy(np.zeros(M * 8))
    sol = S._lib.spmv_trsv_solve
    o = S._opts()
    assert sol(plan.h, C.byref(o), 5, buf.ptr, 5, buf.ptr, 5, None,
               None) == -errno.EINVAL  # k > kmax
    assert sol(plan.h, C.byref(o), 9, buf.ptr, 9, buf.ptr, 9, None,
               None) == -errno.EINVAL
    assert sol(plan.h, C.byref(o), 4, buf.ptr, 3, buf.ptr, 4, None,
               None) == -errno.EINVAL
    assert sol(plan.h, C.byref(o), 4, buf.ptr, 4, buf.ptr, 4, None, None) == 0
    S.stream_sync()
    h = plan.h
    plan.release()  # a dead plan
    s, k = C.c_int(7), C.c_int(7)
    assert S._lib.spmv_trsv_sweeps(h, C.byref(s), C.byref(k)) == -errno.EBADF
    assert (s.value, k.value) == (7, 7)
    assert sol(h, C.byref(o), 4, buf.ptr, 4, buf.ptr, 4, None,
               None) == -errno.EBADF
    buf.free()
    # after release_source: -ENODATA, as the exact analysis
    T = upload(mat)
    try:
        S.set_panel_schedule("chain")
        T.build_panels(0)
        T.release_source()
    finally:
        S.set_panel_schedule("sweep")
    with pytest.raises(OSError) as ei:
        T.trsv_analyse(sweeps=2)
    assert ei.value.errno == errno.ENODATA
    T.release()
    d.release()


# -------------------------------------------------- 6. a deep chain is fine
def test_a_tridiagonal_matrix_gets_a_usable_plan():
    mat = TV.chain(5000)
    M, IRP, JA, AS = mat
    d = upload(mat)
    with pytest.raises(OSError) as ei:
        d.trsv_analyse("lower", max_levels=100)
    assert ei.value.errno == errno.E2BIG
    plan = d.trsv_analyse("lower", max_levels=100, sweeps=4)
    assert plan.info["launches"] == 4 and plan.info["levels"] == 1
    B = rhs_of(M, 2)
    got = run(plan, B, 2)
    want = SW.fast_sweeps(TV.reference_plan(IRP, JA, AS, "lower"), B, None,
                          GROUP, 4)
    assert same_bits(got, want)
    plan.release()
    d.release()
