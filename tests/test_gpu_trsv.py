"""Level-scheduled triangular solve on the GPU (spmv_csr_trsv_analyse,
spmv_trsv_solve; spmv_engine.h).

The plan is defined to the byte and the solve to the bit (tests/_trsv.py:
reference_plan, reference_solve), so everything is compared as integer arrays
and uint64 views: THERE IS NO TOLERANCE here.  The one bound, in the accuracy
test, is derived from the operation count and not measured.  A NaN has no
defined payload: where the reference holds a NaN the device must hold one,
every other value is compared by its bits.

The shapes are those of tests/_trsv.py (shapes), which the CPU test holds to
what they are for.  No test provokes a fault: every error case is an argument
check that returns before any launch.  Every test runs under a time limit of
its own (LIMIT_S): a test that exceeds it ends the whole process, so nothing
else is started on the device.
"""
import ctypes as C
import errno
import faulthandler
import itertools

import numpy as np
import pytest

import _oracle as O
import _trsv as TV
import spmv_scpa_amd as S

pytestmark = pytest.mark.gpu

LIMIT_S = 240
SHAPE = S.trsv_shape()
L, GROUP = SHAPE["small_rows"], SHAPE["group"]
NAMES = list(TV.shapes(8))  # the names do not depend on L
UPLO = ("lower", "upper")
PAD = 0xFFF8_DEAD_BEEF_0001  # a NaN no solve produces


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def shapes():
    return TV.shapes(L)


_plans = {}


def ref_plan(shapes, name, uplo, values="f64"):
    """the reference plan, computed once per (shape, uplo, value type)"""
    key = (name, uplo, values)
    if key not in _plans:
        M, IRP, JA, AS = shapes[name]
        if values == "f32":
            AS = AS.astype(np.float32).astype(np.float64)
        _plans[key] = TV.reference_plan(IRP, JA, AS, uplo)
    return _plans[key]


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
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (M, k))


def scale_of(M):
    return np.random.default_rng(6).uniform(0.5, 2.0, M)


def padded(V, ld):
    """(M, k) values in an (M, ld) array whose padding holds PAD"""
    M, k = V.shape
    out = np.full((M, ld), PAD, np.uint64).view(np.float64)
    out[:, :k] = V
    return out


def run(plan, B, k, ld=None, scale=None, in_place=False, waves=0, stream=None):
    """one solve of the first k columns of B -> the (M, ld) array that holds
    X, padding included (B's own buffer when in place)"""
    M = B.shape[0]
    ld = ld or k
    d_B = S.DevBuffer.from_numpy(padded(B[:, :k], ld))
    d_X = d_B if in_place else S.DevBuffer.from_numpy(
        padded(np.zeros((M, k)), ld))
    d_s = S.DevBuffer.from_numpy(scale) if scale is not None else None
    plan.solve(d_B.ptr, d_X.ptr, k, scale=d_s.ptr if d_s else None, ldb=ld,
               ldx=ld, waves_per_block=waves, stream=stream)
    S.stream_sync(stream)
    X = d_X.to_numpy(np.float64, M * ld).reshape(M, ld)
    if not in_place:  # B is read only: its bytes are what they were
        back = d_B.to_numpy(np.float64, M * ld)
        assert np.array_equal(bits(back), bits(padded(B[:, :k], ld)))
    for b in {d_B, d_X, d_s} - {None}:
        b.free()
    return X


def check_solve(plan, want, B, k, ld=None, **kw):
    ld = ld or k
    X = run(plan, B, k, ld, **kw)
    assert same_bits(X[:, :k], want[:, :k]), (k, ld, kw)
    assert np.all(bits(X[:, k:]) == PAD), (k, ld, kw)  # padding untouched


# ------------------------------------------------------ 1. bytes of the plan
@pytest.mark.parametrize("values", ["f64", "f32"])
@pytest.mark.parametrize("uplo", UPLO)
@pytest.mark.parametrize("name", NAMES)
def test_the_plan_is_the_reference_byte_for_byte(shapes, name, uplo, values):
    mat = shapes[name]
    want = ref_plan(shapes, name, uplo, values)
    d = upload(mat, values)
    live = S._lib.spmv_live_handles()
    plan = d.trsv_analyse(uplo)
    assert S._lib.spmv_live_handles() == live + 1
    got = plan.download()
    for key in ("level", "order", "level_ptr", "rowptr", "ja"):
        assert got[key].dtype == np.int32
        assert np.array_equal(got[key], want[key]), (name, key)
    for key in ("as", "diag"):
        assert np.array_equal(bits(got[key]), bits(want[key])), (name, key)
    info = plan.info
    widths = np.diff(want["level_ptr"])
    assert info["M"] == mat[0]
    assert info["levels"] == len(widths)
    assert info["entries"] == len(want["ja"])
    assert info["widest_level"] == (widths.max() if len(widths) else 0)
    assert info["zero_diag"] == np.count_nonzero(want["diag"] == 0.0)
    assert info["launches"] == len(TV.segments(want["level_ptr"], L))
    assert info["bytes"] >= 4 * (len(widths) + 1) + 20 * mat[0] + \
        (4 + d.value_bytes) * len(want["ja"])
    if name == "lap2d":
        assert info["levels"] == 29
    # a unit plan holds the same bytes: only the solve ignores the diagonal
    if name in ("sandwich", "single"):
        unit = d.trsv_analyse(uplo, unit=True).download()
        assert all(np.array_equal(unit[n], got[n]) for n in
                   ("level", "order", "level_ptr", "rowptr", "ja"))
        assert np.array_equal(bits(unit["diag"]), bits(got["diag"]))
    plan.release()
    d.release()


def test_three_analyses_give_identical_bytes(shapes):
    d = upload(shapes["random"])
    first = d.trsv_analyse("lower")
    want = first.download()
    for _ in range(2):
        again = d.trsv_analyse("lower")
        got = again.download()
        assert all(np.array_equal(got[n], want[n]) for n in
                   ("level", "order", "level_ptr", "rowptr", "ja"))
        assert np.array_equal(bits(got["as"]), bits(want["as"]))
        again.release()
    first.release()
    d.release()


# ------------------------------------------------------ 2. bits of the solve
GRID = list(itertools.product((1, 3, 8), (0, 3), (False, True), (False, True),
                              (0, 1, 16)))


@pytest.mark.parametrize("uplo", UPLO)
@pytest.mark.parametrize("name", ["lap2d", "sandwich", "fan 3L+5"])
def test_every_combination_equals_the_reference(shapes, name, uplo):
    """k, leading dimension, scale, in place, waves_per_block; unit and not"""
    mat = shapes[name]
    M = mat[0]
    B, scale = rhs_of(M), scale_of(M)
    d = upload(mat)
    rp = ref_plan(shapes, name, uplo)
    for unit in (False, True):
        plan = d.trsv_analyse(uplo, unit=unit)
        want = {s is not None: TV.reference_solve(rp, B, s, GROUP, unit)
                for s in (None, scale)}
        for k, extra, scaled, in_place, waves in GRID:
            check_solve(plan, want[scaled], B, k, k + extra,
                        scale=scale if scaled else None, in_place=in_place,
                        waves=waves)
        plan.release()
    d.release()


@pytest.mark.parametrize("values", ["f64", "f32"])
@pytest.mark.parametrize("uplo", UPLO)
@pytest.mark.parametrize("name", NAMES)
def test_every_shape_solves_to_the_bit(shapes, name, uplo, values):
    mat = shapes[name]
    M = mat[0]
    B, scale = rhs_of(M, 3), scale_of(M)
    rp = ref_plan(shapes, name, uplo, values)
    d = upload(mat, values)
    plan = d.trsv_analyse(uplo)
    d.release()  # the plan owns its data
    want = TV.reference_solve(rp, B, scale, GROUP)
    if M == 0:
        plan.solve(8, 8, 3)  # nothing to do: no pointer is read
    else:
        check_solve(plan, want, B, 3, 4, scale=scale)
        check_solve(plan, want, B, 2, 2, scale=scale, in_place=True, waves=2)
    plan.release()


def test_columns_do_not_meet_and_ones_scale_nothing(shapes):
    mat = shapes["random"]
    M = mat[0]
    B = rhs_of(M)
    d = upload(mat)
    plan = d.trsv_analyse("lower")
    X8 = run(plan, B, 8)
    for j in (0, 5, 7):
        X1 = run(plan, B[:, j:j + 1], 1)
        assert same_bits(X1[:, 0], X8[:, j]), j  # rows without a diagonal: NaN
    ones = run(plan, B, 8, scale=np.ones(M))
    assert same_bits(ones, X8)
    # the other columns may hold anything
    B2 = B.copy()
    B2[:, 3] = np.inf
    B2[7, 4] = np.nan
    X2 = run(plan, B2, 8)
    keep = [0, 1, 2, 5, 6, 7]
    assert same_bits(X2[:, keep], X8[:, keep])
    assert np.isfinite(X8).any() and np.isnan(X8).any()
    plan.release()
    d.release()


# ------------------------------------------------------------ 3. accuracy
@pytest.mark.parametrize("uplo", UPLO)
def test_the_residual_meets_the_derived_bound(uplo):
    """|b - T x|_i <= (n_i + 3) u sum_c |T_ic| |x_c|, u = 2^-53: n_i products
    and sums, one subtraction and one division; evaluated from the DOWNLOADED
    plan, the residual in extended precision"""
    mat = TV.random_triangle(5000, seed=17, dominant=True)
    M = mat[0]
    B = rhs_of(M, 2)
    d = upload(mat)
    plan = d.trsv_analyse(uplo)
    got = plan.download()
    assert plan.info["zero_diag"] == 0
    X = run(plan, B, 2)
    res = TV.residual(got, B, X)
    bound = TV.row_bound(got, X)
    print("largest residual / bound:", float((res / bound).max()))
    assert np.all(np.isfinite(X)) and np.all(res <= bound)
    plan.release()
    d.release()


# ------------------------------------------------------- 4. special values
def test_a_nan_reaches_its_dependents_and_nothing_else():
    mat = TV.random_triangle(5000, seed=17, dominant=True)
    M, IRP, JA, AS = mat
    rp = TV.reference_plan(IRP, JA, AS, "lower")
    r = 40
    reach = TV.reachable(rp, r)
    assert 10 < reach.sum() < M - 10  # explicit zeros are dependencies too
    B = rhs_of(M, 3)
    d = upload(mat)
    plan = d.trsv_analyse("lower")
    clean = run(plan, B, 3)
    B[r, 1] = np.nan
    X = run(plan, B, 3)
    assert np.array_equal(np.isnan(X[:, 1]), reach)
    assert np.array_equal(bits(X[~reach, 1]), bits(clean[~reach, 1]))
    assert np.array_equal(bits(X[:, [0, 2]]), bits(clean[:, [0, 2]]))
    plan.release()
    d.release()


def test_a_zero_diagonal_is_plain_arithmetic(shapes):
    M, IRP, JA, AS = shapes["sandwich"]
    r = 3  # a row of level 1: the wide level hangs on it
    keep = ~((np.repeat(np.arange(M), np.diff(IRP)) == r) & (JA == r))
    lens = np.diff(IRP)
    lens[r] -= 1
    mat = (M, TV.irp_of(lens), JA[keep], AS[keep])
    rp = TV.reference_plan(*mat[1:], "lower")
    assert rp["diag"][r] == 0.0 and rp["level"][r] == 1
    reach = TV.reachable(rp, r)
    assert 2 < reach.sum() < M
    B = rhs_of(M, 2)
    want = TV.reference_solve(rp, B, None, GROUP)
    d = upload(mat)
    plan = d.trsv_analyse("lower")
    assert plan.info["zero_diag"] == 1
    X = run(plan, B, 2)
    assert same_bits(X, want)
    assert not np.isfinite(X[reach]).any() and np.isfinite(X[~reach]).all()
    plan.release()
    d.release()


# ----------------------------------------------------------- 5. max_levels
def test_the_level_cap(shapes):
    d = upload(shapes["chain300"])
    d.trsv_analyse("lower").release()  # the kernels' code is resident now
    live = S._lib.spmv_live_handles()
    free0 = S.dev_mem_info()[0]
    for uplo in UPLO:
        with pytest.raises(OSError) as ei:
            d.trsv_analyse(uplo, max_levels=299)
        assert ei.value.errno == errno.E2BIG
        assert S._lib.spmv_live_handles() == live
    out = C.c_void_p(99)
    assert S._lib.spmv_csr_trsv_analyse(d.h, 0, 0, 1, C.byref(out)) == \
        -errno.E2BIG
    assert out.value is None
    assert S.dev_mem_info()[0] >= free0  # the scratch went with the error
    plan = d.trsv_analyse("lower", max_levels=300)
    assert plan.info["levels"] == 300 and plan.info["launches"] == 1
    plan.release()
    d.release()


# ------------------------------------------------- 6. errors and lifetime
def test_errors_and_lifetime(shapes):
    mat = shapes["sandwich"]
    M = mat[0]
    d = upload(mat)
    wide = upload((M, mat[1], mat[2], mat[3]), N=M + 1)
    live = S._lib.spmv_live_handles()
    out = C.c_void_p(99)
    an = S._lib.spmv_csr_trsv_analyse
    # every error is an argument check: nothing is created, nothing launched
    assert an(wide.h, 0, 0, 0, C.byref(out)) == -errno.EINVAL  # not square
    assert out.value is None
    assert an(d.h, 2, 0, 0, C.byref(out)) == -errno.EINVAL
    assert an(d.h, 0, 0, -1, C.byref(out)) == -errno.EINVAL
    assert an(d.h, 0, 0, 0, None) == -errno.EINVAL
    junk = C.cast(C.create_string_buffer(512), C.c_void_p)
    assert an(junk, 0, 0, 0, C.byref(out)) == -errno.EBADF
    assert S._lib.spmv_live_handles() == live
    wide.release()
    live -= 1

    warm = d.trsv_analyse("lower")  # the kernels' code is resident after this
    run(warm, rhs_of(M, 3), 3)
    warm.release()
    S.stream_sync()
    free0 = S.dev_mem_info()[0]
    plan = d.trsv_analyse("lower")
    assert S._lib.spmv_live_handles() == live + 1
    buf = S.DevBuffer.from_numpy(np.zeros(M * 11))
    sol = S._lib.spmv_trsv_solve
    o = S._opts()
    ok = (plan.h, C.byref(o), 3, buf.ptr, 3, buf.ptr, 3, None, None)

    def with_(**kw):
        names = ("P", "opts", "k", "B", "ldb", "X", "ldx", "scale", "stream")
        a = dict(zip(names, ok))
        a.update(kw)
        return sol(*(a[n] for n in names))

    for bad in (dict(k=0), dict(k=9), dict(k=-1), dict(ldb=2), dict(ldx=2),
                dict(B=None), dict(X=None), dict(P=None)):
        assert with_(**bad) == -errno.EINVAL, bad
    assert with_(P=junk) == -errno.EBADF
    for field, v in (("waves_per_block", 17), ("waves_per_block", -1),
                     ("group", 2), ("variant", 1)):
        o2 = S._opts()
        setattr(o2, field, v)
        assert with_(opts=C.byref(o2)) == -errno.EINVAL, field
    o2 = S._opts()
    o2.reserved[4] = 1
    assert with_(opts=C.byref(o2)) == -errno.EINVAL
    assert with_(opts=None) == 0  # NULL opts: the defaults
    S.stream_sync()

    # the plan still solves after the source handle is released
    B = rhs_of(M, 3)
    want = TV.reference_solve(ref_plan(shapes, "sandwich", "lower"), B, None,
                              GROUP)
    d.release()
    assert S._lib.spmv_live_handles() == live
    check_solve(plan, want, B, 3)
    buf.free()
    plan.release()
    plan.release()  # a second release of the wrapper makes no call
    assert S._lib.spmv_live_handles() == live - 1
    assert S.dev_mem_info()[0] >= free0
    # after release_source: -ENODATA, and nothing is created
    T = upload(mat)
    try:
        S.set_panel_schedule("chain")
        T.build_panels(0)
        T.release_source()
    finally:
        S.set_panel_schedule("sweep")
    live = S._lib.spmv_live_handles()
    with pytest.raises(OSError) as ei:
        T.trsv_analyse()
    assert ei.value.errno == errno.ENODATA
    assert S._lib.spmv_live_handles() == live
    T.release()


# ------------------------------------------------------- 7. graph capture
def test_a_captured_solve_replays_the_eager_bits(shapes):
    mat = shapes["sandwich"]
    M = mat[0]
    B = rhs_of(M, 3)
    want = TV.reference_solve(ref_plan(shapes, "sandwich", "lower"), B, None,
                              GROUP)
    d = upload(mat)
    plan = d.trsv_analyse("lower")
    assert plan.info["launches"] == 3  # chain, wide, chain
    side = S.Stream()
    d_B = S.DevBuffer.from_numpy(B)
    d_X = S.DevBuffer.from_numpy(np.zeros((M, 3)))
    plan.solve(d_B.ptr, d_X.ptr, 3, stream=side.ptr)  # one eager run
    side.sync()
    eager = d_X.to_numpy(np.float64, M * 3).reshape(M, 3)
    assert same_bits(eager, want)
    with side.capture(shape=True) as g:
        plan.solve(d_B.ptr, d_X.ptr, 3, stream=side.ptr)
    # the launches of the plan, one after the other: a single chain of nodes
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


# ------------------------------------------------------------------ 8. use
def test_gauss_seidel_sweeps_and_symmetric_gauss_seidel():
    """x <- x + (D+L)^-1 (b - A x) from launch_axpby and plan.solve against the
    same loop in numpy with the device's product A x, to the bit, 50 sweeps;
    then z = (D+U)^-1 D (D+L)^-1 r as two solves through scale = diag"""
    Mg, IRP, JA, AS = TV.lap(24, 24)
    d = upload((Mg, IRP, JA, AS))
    eye = upload(TV.from_rows([[(i, 1.0)] for i in range(Mg)]))
    low, up = d.trsv_analyse("lower"), d.trsv_analyse("upper")
    rl = TV.reference_plan(IRP, JA, AS, "lower")
    ru = TV.reference_plan(IRP, JA, AS, "upper")
    b = rhs_of(Mg, 1, seed=12)
    d_b = S.DevBuffer.from_numpy(b)
    d_x = S.DevBuffer.from_numpy(np.zeros((Mg, 1)))
    d_r, d_z, d_s = (S.DevBuffer(Mg * 8) for _ in range(3))
    x = np.zeros((Mg, 1))
    norms = [np.linalg.norm(b)]
    for sweep in range(50):
        # the device: r = b; r = -A x + r; z = (D+L)^-1 r; x = z + x
        eye.launch_axpby(1.0, 0.0, d_b.ptr, d_r.ptr)
        d.launch_axpby(-1.0, 1.0, d_x.ptr, d_r.ptr)
        low.solve(d_r.ptr, d_z.ptr)
        eye.launch_axpby(1.0, 1.0, d_z.ptr, d_x.ptr)
        # numpy, with the device's product of ITS x
        d_t = S.DevBuffer.from_numpy(x)
        d.launch_multi(d_t.ptr, d_s.ptr, 1)
        S.stream_sync()
        s = d_s.to_numpy(np.float64, Mg).reshape(Mg, 1)
        d_t.free()
        r = -1.0 * s + 1.0 * b
        z = TV.reference_solve(rl, r, None, GROUP)
        x = 1.0 * z + 1.0 * x
        got = d_x.to_numpy(np.float64, Mg).reshape(Mg, 1)
        assert np.array_equal(bits(got), bits(x)), sweep
        norms.append(np.linalg.norm(
            b[:, 0] - O.csr_spmv(IRP, JA, AS, np.ascontiguousarray(x[:, 0]))))
    print("residual norms:", norms[0], norms[1], norms[-1])
    assert all(b_ < a_ for a_, b_ in zip(norms, norms[1:]))
    # symmetric Gauss-Seidel of the last residual
    d_d = S.DevBuffer(Mg * 8)
    d.diag(d_d.ptr)
    S.stream_sync()
    dg = d_d.to_numpy(np.float64, Mg)
    assert np.array_equal(bits(dg), bits(rl["diag"]))
    low.solve(d_r.ptr, d_z.ptr)
    up.solve(d_z.ptr, d_z.ptr, scale=d_d.ptr)  # in place
    S.stream_sync()
    r = d_r.to_numpy(np.float64, Mg).reshape(Mg, 1)
    want = TV.reference_solve(ru, TV.reference_solve(rl, r, None, GROUP), dg,
                              GROUP)
    assert np.array_equal(bits(d_z.to_numpy(np.float64, Mg)), bits(want))
    for h in (d_b, d_x, d_r, d_z, d_s, d_d):
        h.free()
    for h in (low, up, eye, d):
        h.release()
