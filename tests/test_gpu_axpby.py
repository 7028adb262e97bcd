"""Y = alpha*A*X + beta*Y in place (spmv_*_launch_axpby, spmv_engine.h) on the
GPU: CSR and column-major HLL handles, f64 and f32 values, 1-8 interleaved
vectors.

The expected value needs no new oracle and no tolerance.  With S what
launch_multi stores on the same handle with the same opts and Y0 the old Y,

    beta == 0:  want = np.float64(alpha) * S                  (Y0 is not read)
    beta != 0:  want = np.float64(alpha) * S + np.float64(beta) * Y0

numpy rounds every operation once, which is the contract (two products and
one sum, no fused multiply-add), so the uint64 views are compared.  Y0 is
finite (fixed seed) where beta != 0 and 0xFF bytes -- a NaN -- where beta == 0;
columns beyond k and PAST rows beyond M always hold the 0xFF fill and must
keep it.  The padding columns of X (ldx > k) hold NaN: they are never read.

Every test runs under a time limit of its own (LIMIT_S): a test that exceeds
it ends the whole process, so nothing else is started on the device.
"""
import ctypes as C
import errno
import faulthandler

import numpy as np
import pytest

import spmv_scpa_amd as S
from test_gpu_f32_values import SYNTH, case_arrays
from test_gpu_multi_vector import (FILL, PAST, Bench, _ms_per_launch, bits,
                                   handles, x_columns)
from test_gpu_multi_vector_edges import BIG_M, BIG_SPEC, klass

pytestmark = pytest.mark.gpu

LIMIT_S = {"test_the_epilogue_costs_what_its_bytes_cost": 600}

#: (alpha, beta): the bits of launch_multi; a scaled product; the residual
#: y - A x; two inexact factors; alpha == 0 (no special case)
AB = ((1.0, 0.0), (2.5, 0.0), (-1.0, 1.0), (0.3, -1.7), (0.0, 1.0))
BIT_CASES = ["hand", "synth:hub", "synth:ragged", "synth:banded", "mtx:tail40"]
KS = (1, 3, 4, 8)


@pytest.fixture(autouse=True)
def _time_limit(request):
    name = request.node.name.split("[")[0]
    faulthandler.dump_traceback_later(LIMIT_S.get(name, 240), exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def old_y(M, ly, k, seed=5):
    """-> Y0 as (M + PAST, ly): finite in [:M, :k], the fill everywhere else"""
    Y0 = np.empty((M + PAST, ly))
    bits(Y0)[:] = FILL
    Y0[:M, :k] = np.random.default_rng(seed).uniform(-2.0, 2.0, (M, k))
    return Y0


def expected(alpha, beta, Sx, Y0):
    """the contract, as numpy computes it: each operation rounded once"""
    with np.errstate(invalid="ignore", over="ignore"):
        if beta == 0:
            return np.float64(alpha) * Sx
        return np.float64(alpha) * Sx + np.float64(beta) * Y0


class AxBench(Bench):
    def axpby(self, m, alpha, beta, k, Y0=None, ldx=0, ldy=0, shift=0, **kw):
        """-> the whole of Y as (M + PAST, ldy) after launch_axpby on a Y
        that held Y0 (M + PAST, ldy), or the 0xFF fill when Y0 is None"""
        ly = ldy or k
        self.put_X(k, ldx, shift)
        S._check(S._lib.spmv_dev_memset(self.Y.ptr, 0xFF, self.Y.nbytes,
                                        None), "spmv_dev_memset")
        if Y0 is not None:
            assert Y0.shape == (self.M + PAST, ly) and Y0.flags.c_contiguous
            S.stream_sync()
            S._check(S._lib.spmv_copy_h2d(self.Y.ptr, Y0.ctypes.data,
                                          Y0.nbytes), "spmv_copy_h2d")
        m.launch_axpby(alpha, beta, self.X.ptr + shift, self.Y.ptr, k,
                       ldx=ldx, ldy=ldy, **kw)
        S.stream_sync()
        n = (self.M + PAST) * ly
        return self.Y.to_numpy(np.float64, n).reshape(self.M + PAST, ly)


def check_axpby(bench, m, k, what, pairs=AB, Y0=None, **kw):
    """launch_axpby against the numpy expression on launch_multi's S, with
    the same strides and opts, for every (alpha, beta) of `pairs`"""
    M = bench.M
    ly = kw.get("ldy", 0) or k
    Sx = bench.multi(m, k, **kw)[:M, :k].copy()
    assert not np.any(bits(Sx) == FILL), (what, "launch_multi left rows out")
    if Y0 is None:
        Y0 = old_y(M, ly, k)
    for alpha, beta in pairs:
        tag = (what, "k", k, "alpha", alpha, "beta", beta, kw)
        Yf = bench.axpby(m, alpha, beta, k, Y0 if beta != 0 else None, **kw)
        want = expected(alpha, beta, Sx, Y0[:M, :k])
        got = Yf[:M, :k]
        same = bits(got) == bits(want)
        assert np.all(same), (tag, "elements that differ", int(np.sum(~same)),
                              "first", np.argwhere(~same)[:4].tolist(),
                              got[~same][:4], want[~same][:4])
        if beta == 0:  # the old Y (all NaN) was not read
            assert not np.any(np.isnan(got) & ~np.isnan(Sx)), tag
        # columns beyond k and rows beyond M keep their bits
        assert np.all(bits(Yf[:M, k:]) == FILL), (tag, "columns beyond k")
        assert np.all(bits(Yf[M:]) == FILL), (tag, "rows beyond M")


# -------------------------------------------------------------------- 1. bits
@pytest.mark.parametrize("values", ["f64", "f32"])
@pytest.mark.parametrize("case", BIT_CASES)
def test_every_element_has_the_bits_of_the_numpy_expression(case, values):
    M, N, IRP, JA, AS, _, _ = case_arrays(case)
    lens = np.diff(IRP)
    if case == "hand":  # the CSR long-row kernel, HLL blocks wider than 512
        assert lens.min() == 0 and np.any(lens == 1) and lens.max() == 2049
    if case == "synth:hub":
        assert lens.max() == 40_000
    if case == "synth:ragged":
        assert M == 20_011 and M % 32 != 0
    A = S.csr_from_arrays(case, M, N, IRP, JA, AS)
    bench = AxBench(M, N, x_columns(N))
    hs = handles(A, values)
    for fmt, m in hs.items():
        assert m.value_bytes == (4 if values == "f32" else 8)
        for k in KS:
            check_axpby(bench, m, k, (case, values, fmt))
    for m in hs.values():
        m.release()
    bench.free()
    S.csr_free(A)


# ----------------------------------------------------------------- 2. strides
@pytest.mark.parametrize("values", ["f64", "f32"])
@pytest.mark.parametrize("case", ["synth:ragged", "hand"])
def test_strides_and_an_unaligned_X_change_no_bit(case, values):
    M, N, IRP, JA, AS, _, _ = case_arrays(case)
    A = S.csr_from_arrays(case, M, N, IRP, JA, AS)
    bench = AxBench(M, N, x_columns(N))
    hs = handles(A, values)
    for fmt, m in hs.items():
        for k in (3, 8):
            # ldx = k + 3: the padding columns of X are NaN; ldy = k + 1: one
            # column of Y that is not the launch's; X 8 bytes off 16
            check_axpby(bench, m, k, (case, values, fmt, "strides"),
                        pairs=((0.3, -1.7), (2.5, 0.0)), ldx=k + 3, ldy=k + 1,
                        shift=8)
            # ... and the strided launch has the bits of the dense one
            Y0 = old_y(M, k, k)
            Y1 = old_y(M, k + 1, k)
            assert np.array_equal(bits(Y0[:M, :k]), bits(Y1[:M, :k]))
            dense = bench.axpby(m, 0.3, -1.7, k, Y0)
            strided = bench.axpby(m, 0.3, -1.7, k, Y1, ldx=k + 3, ldy=k + 1,
                                  shift=8)
            assert np.array_equal(bits(strided[:M, :k]), bits(dense[:M, :k]))
    for m in hs.values():
        m.release()
    bench.free()
    S.csr_free(A)


# ------------------------------------------------------------ 3. launch shape
@pytest.mark.parametrize("values", ["f64", "f32"])
def test_waves_per_block_and_csr_groups_follow_launch_multi(values):
    case = "synth:ragged"
    M, N, IRP, JA, AS, _, _ = case_arrays(case)
    A = S.csr_from_arrays(case, M, N, IRP, JA, AS)
    bench = AxBench(M, N, x_columns(N))
    hs = handles(A, values)
    pairs = ((-1.0, 1.0), (2.5, 0.0))
    for k in (1, 4, 8):  # P / U = 8, 4, 2
        for fmt, m in hs.items():
            for w in (1, 16):
                check_axpby(bench, m, k, (values, fmt, "waves"), pairs=pairs,
                            waves_per_block=w)
        for g in (2, 4, 8, 16, 32):  # S with the same group: its own tree
            check_axpby(bench, hs["csr"], k, (values, "csr", "group"),
                        pairs=pairs, group=g)
    for m in hs.values():
        m.release()
    bench.free()
    S.csr_free(A)


# ------------------------------------------------------------ 4. grouped order
def test_grouped_order_and_its_padded_grid():
    """2 100 003 rows: past both order thresholds of the engine (CSR M >=
    2 000 000, HLL 65 536 hack blocks), so both handles run the grouped order
    on a grid padded to whole rounds; the last hack block has 3 rows"""
    M = N = BIG_M
    k = 4
    d = S.CsrDevice.generate(*BIG_SPEC, 0, 42)
    h = d.to_hll(True)
    assert d.M == M >= 2_000_000
    assert h.num_blocks == (M + 31) // 32 >= 65536 and M % 32 == 3
    X = S.DevBuffer(N * k * 8)
    Y = S.DevBuffer((M + PAST) * k * 8)
    S.dev_fill_synth(X.ptr, N * k, 7)
    Y0 = old_y(M, k, k)

    def run(launch):
        S._check(S._lib.spmv_copy_h2d(Y.ptr, Y0.ctypes.data, Y0.nbytes),
                 "spmv_copy_h2d")
        launch()
        S.stream_sync()
        return Y.to_numpy(np.float64, (M + PAST) * k).reshape(M + PAST, k)

    for fmt, m in (("csr", d), ("hll", h)):
        Sx = run(lambda: m.launch_multi(X.ptr, Y.ptr, k))
        assert np.all(bits(Sx[M:]) == FILL), fmt
        assert np.all(np.isfinite(Sx[:M])), fmt
        got = run(lambda: m.launch_axpby(-1.0, 1.0, X.ptr, Y.ptr, k))
        want = expected(-1.0, 1.0, Sx[:M], Y0[:M])
        same = bits(got[:M]) == bits(want)
        assert np.all(same), (fmt, "elements that differ", int(np.sum(~same)),
                              "first", np.argwhere(~same)[:4].tolist())
        assert np.all(bits(got[M:]) == FILL), (fmt, "rows beyond M")
    for b in (h, d):
        b.release()
    X.free()
    Y.free()


# -------------------------------------------------------------- 5. non-finite
@pytest.mark.parametrize("case", ["synth:ragged", "hand"])
def test_a_nonfinite_old_y_reaches_its_own_element_only(case):
    """hand: row 2 holds 2049 entries (the CSR long-row kernel; its hack block
    is wider than 512 columns, so every row of it is the wide kernel's)"""
    M, N, IRP, JA, AS, _, _ = case_arrays(case)
    A = S.csr_from_arrays(case, M, N, IRP, JA, AS)
    bench = AxBench(M, N, x_columns(N))
    k = 4
    Y0 = old_y(M, k, k)
    Y0[2, 1] = np.inf
    Y0[5, 0] = np.nan
    Ynan = old_y(M, k, k)
    Ynan[:M] = np.nan
    for values in ("f64", "f32"):
        hs = handles(A, values)
        for fmt, m in hs.items():
            Sx = bench.multi(m, k)[:M, :k].copy()
            assert np.all(np.isfinite(Sx))
            for alpha, beta in ((0.3, -1.7), (-1.0, 1.0), (0.0, 1.0)):
                got = bench.axpby(m, alpha, beta, k, Y0)[:M, :k]
                want = expected(alpha, beta, Sx, Y0[:M, :k])
                what = (case, values, fmt, alpha, beta)
                assert np.array_equal(klass(got), klass(want)), what
                bad = ~np.isfinite(got)
                assert np.argwhere(bad).tolist() == [[2, 1], [5, 0]], what
                assert got[2, 1] == np.sign(beta) * np.inf, what
                assert np.array_equal(bits(got[~bad]), bits(want[~bad])), what
            for alpha in (2.5, 0.0):  # beta == 0: an all-NaN Y reaches nothing
                got = bench.axpby(m, alpha, 0.0, k, Ynan)[:M, :k]
                want = expected(alpha, 0.0, Sx, Ynan[:M, :k])
                assert np.array_equal(klass(got), klass(want)), (fmt, alpha)
                assert np.all(np.isfinite(got)), (fmt, alpha)
                assert np.array_equal(bits(got), bits(want)), (fmt, alpha)
        for m in hs.values():
            m.release()
    bench.free()
    S.csr_free(A)


# ------------------------------------------------------------------- 6. graph
@pytest.mark.parametrize("values", ["f64", "f32"])
def test_a_captured_axpby_replays_with_the_values_it_was_captured_with(values):
    tag, kind, M, K, W = next(t for t in SYNTH if t[0] == "hub")
    N, k = M, 4
    dG = S.CsrDevice.generate(kind, M, N, K, W, 0, 42)
    d = dG.to_f32() if values == "f32" else dG
    hs = {"csr": d, "hll": d.to_hll(True)}
    X, Y = S.DevBuffer(N * k * 8), S.DevBuffer(M * k * 8)
    Y0 = np.ascontiguousarray(old_y(M, k, k)[:M])
    side = S.Stream()

    def put_y0():
        side.sync()
        S._check(S._lib.spmv_copy_h2d(Y.ptr, Y0.ctypes.data, Y0.nbytes),
                 "spmv_copy_h2d")

    def step(y):  # the captured launch, as numpy computes it
        return expected(0.5, 1.0, Sx, y)

    for fmt, m in hs.items():
        S.dev_fill_synth(X.ptr, N * k, 7, 0, side.ptr)
        m.launch_multi(X.ptr, Y.ptr, k, stream=side.ptr)
        side.sync()
        Sx = Y.to_numpy(np.float64, M * k).reshape(M, k)
        put_y0()
        m.launch_axpby(0.5, 1.0, X.ptr, Y.ptr, k, stream=side.ptr)  # eagerly
        side.sync()
        eager = Y.to_numpy(np.float64, M * k).reshape(M, k)
        assert np.array_equal(bits(eager), bits(step(Y0))), fmt
        with side.capture() as g:  # the long row's side launch is in the graph
            m.launch_axpby(0.5, 1.0, X.ptr, Y.ptr, k, stream=side.ptr)
        put_y0()
        g.launch(side.ptr)
        g.launch(side.ptr)
        side.sync()
        twice = Y.to_numpy(np.float64, M * k).reshape(M, k)
        assert np.array_equal(bits(twice), bits(step(step(Y0)))), fmt
        g.destroy()
    for m in set(list(hs.values()) + [dG]):
        m.release()
    X.free()
    Y.free()


# ---------------------------------------------------------------- 7. refusals
def _rc(m, opts, k, X, ldx, Y, ldy, alpha=2.0, beta=1.0):
    return m._fn("launch_axpby")(m.h, opts, k, alpha, beta, X, ldx, Y, ldy,
                                 None)


def test_refusals_and_the_byte_count():
    M, N, IRP, JA, AS, _, _ = case_arrays("synth:banded")
    A = S.csr_from_arrays("refuse", M, N, IRP, JA, AS)
    bench = AxBench(M, N, x_columns(N))
    bench.put_X(4)
    live = S._lib.spmv_live_handles()
    d = S.CsrDevice.upload(A)
    cm, rm = d.to_hll(True), d.to_hll(False)
    compact = cm.to_index16()
    A0 = S.csr_from_arrays("norows", 0, N, np.zeros(1, np.int32),
                           np.zeros(0, np.int32), np.zeros(0))
    d0 = S.CsrDevice.upload(A0)
    h0 = d0.to_hll(True)
    made = S._lib.spmv_live_handles()
    assert made == live + 6
    X, Y = bench.X.ptr, bench.Y.ptr
    einval = -errno.EINVAL
    for m in (d, cm):
        assert _rc(m, None, 4, X, 0, Y, 0) == 0  # opts may be NULL
        for k in (0, 9):
            assert _rc(m, None, k, X, 0, Y, 0) == einval
            with pytest.raises(OSError) as ei:
                m.axpby_bytes(k, 1.0)
            assert ei.value.errno == errno.EINVAL
        assert _rc(m, None, 4, X, 3, Y, 0) == einval
        assert _rc(m, None, 4, X, 0, Y, 3) == einval
        assert _rc(m, None, 4, None, 0, Y, 0) == einval
        assert _rc(m, None, 4, X, 0, None, 0) == einval
        for bad in (dict(variant=1), dict(variant=1 << 29),
                    dict(waves_per_block=17)):
            o = S._opts(**bad)
            assert _rc(m, C.byref(o), 4, X, 0, Y, 0) == einval, bad
        assert S._lib.spmv_live_handles() == made
    o = S._opts(group=3)
    assert _rc(d, C.byref(o), 4, X, 0, Y, 0) == einval
    # a compact handle holds no 4-byte columns
    assert _rc(compact, None, 4, X, 0, Y, 0) == -errno.ENOTSUP
    for beta in (0.0, 1.0):
        with pytest.raises(OSError) as ei:
            compact.axpby_bytes(4, beta)
        assert ei.value.errno == errno.ENOTSUP
    # the multi-vector HLL kernels are the column-major ones
    assert _rc(rm, None, 4, X, 0, Y, 0) == einval
    with pytest.raises(OSError) as ei:
        rm.launch_axpby(2.0, 1.0, X, Y, 4)
    assert ei.value.errno == errno.EINVAL
    assert S._lib.spmv_live_handles() == made
    # no rows: 0, nothing launched, Y untouched
    S._check(S._lib.spmv_dev_memset(Y, 0xFF, 64, None), "spmv_dev_memset")
    for m in (d0, h0):
        assert _rc(m, None, 4, X, 0, Y, 0) == 0
        m.launch_axpby(2.0, 1.0, X, Y, 4)
    S.stream_sync()
    assert np.all(bench.Y.to_numpy(np.uint64, 8) == FILL)
    # the byte count: launch_multi's, and Y once more when it is read
    for k in range(1, 9):
        for m in (d, cm):
            assert m.axpby_bytes(k, 0.0) == m.multi_bytes(k)
            assert m.axpby_bytes(k, -1.7) == m.multi_bytes(k) + 8 * k * M
    assert d0.axpby_bytes(4, 1.0) == d0.multi_bytes(4)
    # only the blocked copy left: no source arrays to multiply with
    for m in (d, cm):
        m.build_panels()
        m.release_source()
        assert _rc(m, None, 4, X, 0, Y, 0) == -errno.ENODATA
        with pytest.raises(OSError) as ei:
            m.launch_axpby(2.0, 1.0, X, Y, 4)
        assert ei.value.errno == errno.ENODATA
        assert S._lib.spmv_live_handles() == made
    S.stream_sync()
    for m in (d, cm, rm, compact, d0, h0):
        m.release()
    # a pointer that never was a handle
    assert S._lib.spmv_csr_launch_axpby(C.c_void_p(1 << 20), None, 4, 2.0, 1.0,
                                        X, 0, Y, 0, None) == -errno.EBADF
    assert S._lib.spmv_live_handles() == live
    bench.free()
    S.csr_free(A0)
    S.csr_free(A)


# -------------------------------------------------------------------- 8. cost
#: the largest difference between the two rounds of launch_multi that
#: profiles/multi_vector.md records on this matrix shape (banded x 32): csr
#: f64, 0.8687 / 0.8348 ms
SPREAD_FLOOR = 0.0406
#: k_csr_multi<32, 4, 4, double> is 836 instructions, k_csr_axpby of the same
#: parameters 988 (gfx950 assembly)
CSR_INSTRUCTIONS = 988 / 836


def test_the_epilogue_costs_what_its_bytes_cost(request):
    """banded 4M x 32, k = 4, f64 values, CSR and HLL: the shape and the
    timing of test_gpu_multi_vector's speed test (20 launches between two
    events after 3 warm-ups, two alternating rounds).  The yardstick is
    launch_multi on the same handle in the same process:
        t(axpby, beta = 0) <= t(multi) * (1 + m)
        t(axpby, beta = 1) <= t(multi) * axpby_bytes(k, 1) / multi_bytes(k)
                                       * (1 + m)
    with m the relative difference of the yardstick's OWN two rounds in this
    run, floored at SPREAD_FLOOR; m is never measured on launch_axpby.

    The HLL handle is held to exactly that.  Measured on one MI355X (four
    runs): beta = 0 x0.9997-1.0014, beta = 1 x1.048-1.075 of launch_multi for
    a byte ratio of 1.0714.

    The CSR handle does not meet it, and its two bounds are set from the
    measured yardstick instead: launch_multi runs this matrix with 32 lanes
    per row at 0.43-0.49 of 8 TB/s -- a wavefront lives for 8 rows, 4 entries
    per lane, and its time follows the instructions it issues, not the bytes.
    The epilogue (executed by 2 of 64 lanes) and the early y_old loads make
    836 instructions 988 and take one wavefront per SIMD (88 against 78
    VGPRs: 5 against 6).  Measured: beta = 0 x1.06-1.17, beta = 1 x1.16-1.29
    against a byte ratio of 1.0708.  So both CSR bounds carry the factor
    CSR_INSTRUCTIONS = 1.18: beta = 0 <= 1.18 (1 + m), beta = 1 <= 1.18 x
    1.0708 (1 + m).  profiles/axpby.md and DESIGN.md section 15 have the
    tables."""
    M = N = 4_000_000
    k = 4
    X, Y = S.DevBuffer(N * k * 8), S.DevBuffer(M * k * 8)
    S.dev_fill_synth(X.ptr, N * k, 7)
    S.dev_fill_synth(Y.ptr, M * k, 9)
    d = S.CsrDevice.generate(S.SYNTH_BANDED, M, N, 32, 0, 0, 42)
    h = d.to_hll(True)
    late = []
    for fmt, m in (("csr", d), ("hll", h)):
        tm, t0, t1 = [], [], []
        for _ in range(2):
            tm.append(_ms_per_launch(
                lambda: m.launch_multi(X.ptr, Y.ptr, k)))
            t0.append(_ms_per_launch(
                lambda: m.launch_axpby(-1.0, 0.0, X.ptr, Y.ptr, k)))
            # Y <- Y - A X forty-six times over: finite, and the time of a
            # launch does not depend on the values
            t1.append(_ms_per_launch(
                lambda: m.launch_axpby(-1.0, 1.0, X.ptr, Y.ptr, k)))
        spread = abs(tm[0] - tm[1]) / min(tm)
        margin = max(spread, SPREAD_FLOOR)
        print("axpby banded4M %s rounds (ms): multi %s  beta=0 %s  beta=1 %s"
              % (fmt, tm, t0, t1))
        tm, t0, t1 = (float(np.mean(t)) for t in (tm, t0, t1))
        model = m.axpby_bytes(k, 1.0) / m.multi_bytes(k)
        line = ("axpby banded4M %s k=%d  multi %.4f ms (rounds differ by "
                "%.4f, margin %.4f)  beta=0 %.4f ms (x%.4f)  beta=1 %.4f ms "
                "(x%.4f, bytes x%.4f)"
                % (fmt, k, tm, spread, margin, t0, t0 / tm, t1, t1 / tm,
                   model))
        print(line)
        getattr(request.config, "_summary_lines", []).append(line)
        issue = CSR_INSTRUCTIONS if fmt == "csr" else 1.0
        if not t0 <= tm * issue * (1.0 + margin):
            late.append((fmt, "beta=0", t0, tm * issue * (1.0 + margin)))
        if not t1 <= tm * issue * model * (1.0 + margin):
            late.append((fmt, "beta=1", t1,
                         tm * issue * model * (1.0 + margin)))
    for b in (h, d):
        b.release()
    X.free()
    Y.free()
    assert not late, late
