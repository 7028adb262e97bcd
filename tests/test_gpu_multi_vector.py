"""Y = A X launches for 1-8 interleaved vectors (spmv_*_launch_multi,
spmv_engine.h) on the GPU, CSR and column-major HLL handles, f64 and f32
values.

The expected result needs no new oracle: column j of Y is, BIT FOR BIT, the y
of a launch the library already has on the same handle with the contiguous
vector x_j = X[:, j] -- the sub-wave kernel (CSR kernel 2, same group) or the
thread-per-row kernel (HLL kernel 1) -- on every row of at most 2048 entries
(CSR) / every hack block of at most 512 columns (HLL).  Longer rows and wider
blocks are summed by one workgroup each in a fixed order of their own: they,
and all other rows as well, are held to the project's parity bound (1e-12 of
the row scale sum_c |a_rc x_c|) against the CPU oracle, applied to the rounded
values on an f32 handle.

Y is filled with 0xFF bytes before every launch, X[:, j] = synth_x(7 + j), and
the padding columns of X (ldx > k) hold NaN: they must never be read.

Every test runs under a time limit of its own (LIMIT_S): a test that exceeds
it ends the whole process, so nothing else is started on the device.
"""
import ctypes as C
import errno
import faulthandler

import numpy as np
import pytest

import _oracle as O
import spmv_scpa_amd as S
from test_gpu_f32_values import CASES, SYNTH, case_arrays, round32

pytestmark = pytest.mark.gpu

TIGHT = 1e-12        # the project's parity bound (of the row scale)
PEAK = 8.0e12
MAXK = 8
LONG_ROW = 2048      # STREAM_NNZ: CSR rows beyond it are summed by a workgroup
WIDE_BLOCK = 512     # HLL_WIDE: hack blocks beyond it likewise
PAST = 3             # rows of Y allocated (and checked) beyond row M
FILL = np.uint64(0xFFFFFFFFFFFFFFFF)
LIMIT_S = {"test_one_multi_launch_is_not_slower_than_the_launches_it_replaces":
           600}


@pytest.fixture(autouse=True)
def _time_limit(request):
    name = request.node.name.split("[")[0]
    faulthandler.dump_traceback_later(LIMIT_S.get(name, 240), exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def x_columns(N):
    """X[:, j] = synth_x(7 + j), j = 0..7 (the same for every k)"""
    return np.stack([O.synth_x(7 + j, 0, N) for j in range(MAXK)], axis=1)


class Bench:
    """device buffers of one matrix shape: x / y of the single-vector
    launches, X / Y of the multi-vector ones (sized for ldx, ldy <= 8 + 3 and
    PAST rows of Y beyond M, + 8 bytes for a deliberately misaligned X)"""

    def __init__(self, M, N, Xc):
        self.M, self.N, self.Xc = M, N, Xc
        self.x = S.DevBuffer(max(N, 1) * 8)
        self.y = S.DevBuffer(max(M, 1) * 8)
        self.X = S.DevBuffer(max(N, 1) * (MAXK + 3) * 8 + 8)
        self.Y = S.DevBuffer((M + PAST) * (MAXK + 3) * 8)

    def single(self, m, kernel, j, **kw):
        """y of launch(kernel) with x = X[:, j]"""
        xj = np.ascontiguousarray(self.Xc[:, j])
        S._check(S._lib.spmv_copy_h2d(self.x.ptr, xj.ctypes.data, xj.nbytes),
                 "spmv_copy_h2d")
        S._check(S._lib.spmv_dev_memset(self.y.ptr, 0xFF, max(self.M, 1) * 8,
                                        None), "spmv_dev_memset")
        m.launch(kernel, self.x.ptr, self.y.ptr, **kw)
        S.stream_sync()
        return self.y.to_numpy(np.float64, self.M)

    def put_X(self, k, ldx=0, shift=0):
        lx = ldx or k
        Xh = np.full((self.N, lx), np.nan)
        Xh[:, :k] = self.Xc[:, :k]
        S._check(S._lib.spmv_copy_h2d(self.X.ptr + shift, Xh.ctypes.data,
                                      Xh.nbytes), "spmv_copy_h2d")

    def multi(self, m, k, ldx=0, ldy=0, shift=0, **kw):
        """-> the whole of Y as (M + PAST, ldy) after launch_multi: rows
        beyond M and columns beyond k must still hold the fill"""
        ly = ldy or k
        self.put_X(k, ldx, shift)
        S._check(S._lib.spmv_dev_memset(self.Y.ptr, 0xFF, self.Y.nbytes,
                                        None), "spmv_dev_memset")
        m.launch_multi(self.X.ptr + shift, self.Y.ptr, k, ldx=ldx, ldy=ldy,
                       **kw)
        S.stream_sync()
        n = (self.M + PAST) * ly
        return self.Y.to_numpy(np.float64, n).reshape(self.M + PAST, ly)

    def free(self):
        for b in (self.x, self.y, self.X, self.Y):
            b.free()


def only_k_columns_written(Yf, M, k, what):
    assert np.all(bits(Yf[:M, k:]) == FILL), (what, "columns beyond k")
    assert np.all(bits(Yf[M:]) == FILL), (what, "rows beyond M")


def exact_rows(IRP, M, fmt):
    """rows under the bit rule: CSR rows of <= 2048 entries; HLL rows of hack
    blocks (32 rows) of <= 512 columns"""
    lens = np.diff(IRP)
    if fmt == "csr":
        return lens <= LONG_ROW
    nb = (M + 31) // 32
    padded = np.zeros(nb * 32, np.int64)
    padded[:M] = lens
    width = padded.reshape(nb, 32).max(axis=1)
    return np.repeat(width <= WIDE_BLOCK, 32)[:M]


def handles(A, values):
    """-> {"csr": CSR handle, "hll": column-major HLL handle}"""
    d = S.CsrDevice.upload(A, values=values)
    return {"csr": d, "hll": d.to_hll(True)}


SINGLE = {"csr": 2, "hll": 1}  # the kernel whose bits launch_multi repeats


def check_bits_and_bound(bench, m, fmt, IRP, y_ref, scale, tag, ks, **kw):
    """launch_multi(k) for k in ks against launch(SINGLE[fmt]) on x_j (bits,
    on the rows of the bit rule) and against the oracle (all rows)"""
    M = bench.M
    exact = exact_rows(IRP, M, fmt)
    single = [bench.single(m, SINGLE[fmt], j, **kw) for j in range(max(ks))]
    for k in ks:
        Yf = bench.multi(m, k, **kw)
        only_k_columns_written(Yf, M, k, (tag, fmt, k))
        for j in range(k):
            got = Yf[:M, j]
            same = bits(got)[exact] == bits(single[j])[exact]
            assert np.all(same), (tag, fmt, kw, "k", k, "column", j,
                                  "rows that differ", int(np.sum(~same)))
            err = (np.max(np.abs(got - y_ref[j]) / np.maximum(scale[j], 1e-300))
                   if M else 0.0)
            assert err <= TIGHT, (tag, fmt, kw, "k", k, "column", j, err)


def oracle_columns(IRP, JA, vals, Xc):
    y = [O.csr_spmv(IRP, JA, vals, np.ascontiguousarray(Xc[:, j]))
         for j in range(MAXK)]
    s = [O.csr_abs_spmv(IRP, JA, vals, np.ascontiguousarray(Xc[:, j]))
         for j in range(MAXK)]
    return y, s


# -------------------------------------------------------------------- 1. bits
@pytest.mark.parametrize("values", ["f64", "f32"])
@pytest.mark.parametrize("case", CASES)
def test_every_column_has_the_bits_of_the_single_vector_launch(case, values):
    M, N, IRP, JA, AS, _, _ = case_arrays(case)
    Xc = x_columns(N)
    y_ref, scale = oracle_columns(IRP, JA, round32(AS) if values == "f32"
                                  else AS, Xc)
    A = S.csr_from_arrays(case, M, N, IRP, JA, AS)
    bench = Bench(M, N, Xc)
    hs = handles(A, values)
    for fmt, m in hs.items():
        assert m.value_bytes == (4 if values == "f32" else 8)
        check_bits_and_bound(bench, m, fmt, IRP, y_ref, scale, case,
                             range(1, MAXK + 1))
    for m in hs.values():
        m.release()
    bench.free()
    S.csr_free(A)


@pytest.mark.parametrize("values", ["f64", "f32"])
@pytest.mark.parametrize("case", ["synth:ragged", "synth:stencil27"])
def test_csr_groups_have_the_bits_of_the_sub_wave_kernel_of_that_group(
        case, values):
    M, N, IRP, JA, AS, _, _ = case_arrays(case)
    Xc = x_columns(N)
    y_ref, scale = oracle_columns(IRP, JA, round32(AS) if values == "f32"
                                  else AS, Xc)
    A = S.csr_from_arrays(case, M, N, IRP, JA, AS)
    bench = Bench(M, N, Xc)
    d = S.CsrDevice.upload(A, values=values)
    for g in (2, 4, 8, 16, 32):
        check_bits_and_bound(bench, d, "csr", IRP, y_ref, scale, case,
                             range(1, MAXK + 1), group=g)
    # the waves per workgroup never change a result either
    base = bench.multi(d, 5)
    for w in (1, 3, 16):
        assert np.array_equal(bits(bench.multi(d, 5, waves_per_block=w)),
                              bits(base)), w
    d.release()
    bench.free()
    S.csr_free(A)


# ----------------------------------------------------------------- 2. strides
@pytest.mark.parametrize("values", ["f64", "f32"])
@pytest.mark.parametrize("case", ["synth:ragged", "synth:hub", "hand",
                                  "mtx:tail40"])
def test_strides_change_no_bit_and_only_k_columns_are_written(case, values):
    M, N, IRP, JA, AS, _, _ = case_arrays(case)
    A = S.csr_from_arrays(case, M, N, IRP, JA, AS)
    bench = Bench(M, N, x_columns(N))
    hs = handles(A, values)
    for fmt, m in hs.items():
        for k in (3, 8):
            dense = bench.multi(m, k)
            only_k_columns_written(dense, M, k, (case, fmt, k))
            # ldx = k + 1: 9 is odd (8-byte loads), 4 is even (16-byte loads
            # of an odd number of vectors); shift = 8: an even ldx on a base
            # that is not 16-byte aligned
            for ldx, ldy, shift in ((k + 1, k + 3, 0), (k + 1, k + 3, 8),
                                    (k + 2, k, 8), (k, k + 1, 8)):
                Yf = bench.multi(m, k, ldx=ldx, ldy=ldy, shift=shift)
                what = (case, fmt, k, ldx, ldy, shift)
                only_k_columns_written(Yf, M, k, what)
                assert np.array_equal(bits(Yf[:M, :k]), bits(dense[:M, :k])), what
    for m in hs.values():
        m.release()
    bench.free()
    S.csr_free(A)


# ------------------------------------------------------------ 3. reproducible
@pytest.mark.parametrize("values", ["f64", "f32"])
def test_two_launches_give_the_same_bits_in_every_row(values):
    M, N, IRP, JA, AS, _, _ = case_arrays("synth:hub")
    assert np.diff(IRP).max() > 8192  # the long row / the wide block is there
    A = S.csr_from_arrays("hub", M, N, IRP, JA, AS)
    bench = Bench(M, N, x_columns(N))
    hs = handles(A, values)
    for fmt, m in hs.items():
        for k in (1, 4, 8):
            a, b = bench.multi(m, k), bench.multi(m, k)
            assert np.array_equal(bits(a), bits(b)), (fmt, k)
            assert not np.any(np.isnan(a[:M, :k])), (fmt, k)
    for m in hs.values():
        m.release()
    bench.free()
    S.csr_free(A)


# ---------------------------------------------------------- 4. special values
def test_a_nan_stays_in_its_column_and_empty_rows_give_exactly_zero():
    """One NaN at X[1, 1]: it stays in column 1 of Y, in exactly the rows that
    hold matrix column 1.  For the HLL handle that is a property of THIS
    input: the NaN is not on column 0, and no row holding column 1 is followed
    by a pad (each is as wide as its hack block), so no pad carries it to
    another row.  A non-finite x[0], or one on the last valid column of a
    padded row, reaches more rows of a direct HLL launch --
    test_gpu_multi_vector_edges.py pins that down against the padded oracle."""
    rows = [[(0, 1.0), (1, 2.0)], [], [(2, 1.0)], [(1, 0.5), (3, -1.0)],
            [(4, 0.0), (5, 0.0)]]
    rows += [[] for _ in range(40)] + [[(0, 0.0)], [(1, 3.0)]]
    N = 8
    IRP = np.zeros(len(rows) + 1, np.int32)
    IRP[1:] = np.cumsum([len(r) for r in rows])
    JA = np.array([c for r in rows for c, _ in r], np.int32)
    AS = np.array([v for r in rows for _, v in r], np.float64)
    M = len(rows)
    Xc = np.arange(1.0, 1.0 + N * MAXK).reshape(N, MAXK)
    Xc[1, 1] = np.nan
    holds_col_1 = np.array([any(c == 1 for c, _ in r) for r in rows])
    empty = np.diff(IRP) == 0
    A = S.csr_from_arrays("special", M, N, IRP, JA, AS)
    bench = Bench(M, N, Xc)
    for values in ("f64", "f32"):
        hs = handles(A, values)
        for fmt, m in hs.items():
            for k in (2, 3, 8):
                Y = bench.multi(m, k)[:M, :k]
                what = (values, fmt, k)
                assert np.array_equal(np.isnan(Y[:, 1]), holds_col_1), what
                assert not np.any(np.isnan(np.delete(Y, 1, axis=1))), what
                assert np.all(bits(Y[empty]) == 0), what  # +0.0, every column
                assert Y[0, 0] == 1.0 * Xc[0, 0] + 2.0 * Xc[1, 0], what
        for m in hs.values():
            m.release()
    bench.free()
    S.csr_free(A)


# -------------------------------------------------------------- 5. refusals
def _rc(m, opts, k, X, ldx, Y, ldy):
    return m._fn("launch_multi")(m.h, opts, k, X, ldx, Y, ldy, None)


def test_refusals_on_the_device_and_the_byte_count():
    M, N, IRP, JA, AS, _, _ = case_arrays("synth:banded")
    A = S.csr_from_arrays("refuse", M, N, IRP, JA, AS)
    bench = Bench(M, N, x_columns(N))
    bench.put_X(4)
    live = S._lib.spmv_live_handles()
    d = S.CsrDevice.upload(A)
    cm, rm = d.to_hll(True), d.to_hll(False)
    d32 = d.to_f32()
    X, Y = bench.X.ptr, bench.Y.ptr
    einval = -errno.EINVAL
    for m in (d, cm, d32):
        assert _rc(m, None, 4, X, 0, Y, 0) == 0  # opts may be NULL
        for k in (0, 9, -1):
            assert _rc(m, None, k, X, 0, Y, 0) == einval
        assert _rc(m, None, 4, X, 3, Y, 0) == einval
        assert _rc(m, None, 4, X, 0, Y, 3) == einval
        assert _rc(m, None, 4, None, 0, Y, 0) == einval
        assert _rc(m, None, 4, X, 0, None, 0) == einval
        for bad in (dict(variant=1), dict(variant=1 << 29),
                    dict(waves_per_block=17), dict(waves_per_block=-1)):
            o = S._opts(**bad)
            assert _rc(m, C.byref(o), 4, X, 0, Y, 0) == einval, bad
        o = S._opts()
        o.reserved[4] = 1
        assert _rc(m, C.byref(o), 4, X, 0, Y, 0) == einval
    for g in (1, 3, 64, -2):
        o = S._opts(group=g)
        assert _rc(d, C.byref(o), 4, X, 0, Y, 0) == einval, g
    # the multi-vector HLL kernel is the column-major one
    assert _rc(rm, None, 4, X, 0, Y, 0) == einval
    with pytest.raises(OSError) as ei:
        rm.launch_multi(X, Y, 4)
    assert ei.value.errno == errno.EINVAL
    S.stream_sync()
    # the byte count: the matrix once, k vectors read, k written
    for k in range(1, MAXK + 1):
        assert d.multi_bytes(k) == (12 * d.NZ + 4 * (M + 1) + 8 * k * M
                                    + 8 * k * N)
        assert d32.multi_bytes(k) == (8 * d.NZ + 4 * (M + 1) + 8 * k * M
                                      + 8 * k * N)
        assert cm.multi_bytes(k) == (12 * cm.slots + 12 * cm.num_blocks
                                     + 8 * k * M + 8 * k * N)
    assert d.multi_bytes(1) == d.algorithmic_bytes
    assert cm.multi_bytes(1) == cm.algorithmic_bytes
    for k in (0, 9):
        with pytest.raises(OSError) as ei:
            d.multi_bytes(k)
        assert ei.value.errno == errno.EINVAL
    # only the blocked copy left: no source arrays to multiply with
    for m in (d, cm):
        m.build_panels()
        m.release_source()
        with pytest.raises(OSError) as ei:
            m.launch_multi(X, Y, 4)
        assert ei.value.errno == errno.ENODATA
    for m in (d, cm, rm, d32):
        m.release()
    # a pointer that never was a handle
    assert S._lib.spmv_csr_launch_multi(C.c_void_p(1 << 20), None, 4, X, 0, Y,
                                        0, None) == -errno.EBADF
    assert S._lib.spmv_live_handles() == live
    bench.free()
    S.csr_free(A)


# ------------------------------------------------------------------- 6. graph
@pytest.mark.parametrize("values", ["f64", "f32"])
def test_a_captured_multi_launch_replays_with_a_changed_X(values):
    tag, kind, M, K, W = next(t for t in SYNTH if t[0] == "hub")
    N, k = M, 4
    dG = S.CsrDevice.generate(kind, M, N, K, W, 0, 42)
    d = dG.to_f32() if values == "f32" else dG
    hs = {"csr": d, "hll": d.to_hll(True)}
    X, Y = S.DevBuffer(N * k * 8), S.DevBuffer(M * k * 8)
    side = S.Stream()
    for fmt, m in hs.items():
        S.dev_fill_synth(X.ptr, N * k, 7, 0, side.ptr)
        m.launch_multi(X.ptr, Y.ptr, k, stream=side.ptr)  # eagerly once, first
        side.sync()
        with side.capture() as g:  # the long row's side launch is in the graph
            m.launch_multi(X.ptr, Y.ptr, k, stream=side.ptr)
        for seed in (8, 9):  # the graph reads X where it lives
            S.dev_fill_synth(X.ptr, N * k, seed, 0, side.ptr)
            S._check(S._lib.spmv_dev_memset(Y.ptr, 0xFF, M * k * 8, side.ptr),
                     "spmv_dev_memset")
            g.launch(side.ptr)
            side.sync()
            replayed = Y.to_numpy(np.float64, M * k)
            S._check(S._lib.spmv_dev_memset(Y.ptr, 0xFF, M * k * 8, side.ptr),
                     "spmv_dev_memset")
            m.launch_multi(X.ptr, Y.ptr, k, stream=side.ptr)
            side.sync()
            eager = Y.to_numpy(np.float64, M * k)
            assert np.array_equal(bits(replayed), bits(eager)), (fmt, seed)
            assert not np.any(bits(eager) == FILL), (fmt, seed)
        g.destroy()
    for m in set(list(hs.values()) + [dG]):
        m.release()
    X.free()
    Y.free()


# ------------------------------------------------------------------- 7. speed
def _ms_per_launch(launch, warmup=3, iters=20):
    for _ in range(warmup):
        launch()
    e0, e1 = S.Event(), S.Event()
    e0.record()
    for _ in range(iters):
        launch()
    e1.record()
    return e0.elapsed_ms(e1) / iters


def test_one_multi_launch_is_not_slower_than_the_launches_it_replaces(request):
    """banded 4M x 32 (1.5 GB of matrix: beyond the Infinity Cache, no flush)
    at k = 4, and random 2M x 32 with W = 2N (columns anywhere: gather-bound)
    at k = 8.  The yardstick is the single-vector kernel of the same order on
    the same handle in the same process (CSR kernel 2, HLL kernel 1): 20
    launches between two events after 3 warm-ups, two alternating rounds, the
    median.  Asserted: t_multi < k * t_single, nothing else -- by bytes alone
    the banded ratio would be 0.28; what is measured goes to the terminal
    summary (tools/multi_vector_report.py writes profiles/multi_vector.md)."""
    slower = []
    for tag, kind, M, W, k in (("banded4M", S.SYNTH_BANDED, 4_000_000, 0, 4),
                               ("random2M_W2N", S.SYNTH_RANDOM, 2_000_000,
                                4_000_000, 8)):
        N = M
        x, y = S.DevBuffer(N * 8), S.DevBuffer(M * 8)
        X, Y = S.DevBuffer(N * k * 8), S.DevBuffer(M * k * 8)
        S.dev_fill_synth(x.ptr, N, 7)
        S.dev_fill_synth(X.ptr, N * k, 7)
        d = S.CsrDevice.generate(kind, M, N, 32, W, 0, 42)
        h = d.to_hll(True)
        for fmt, m in (("csr", d), ("hll", h)):
            t1, tk = [], []
            for _ in range(2):
                t1.append(_ms_per_launch(
                    lambda: m.launch(SINGLE[fmt], x.ptr, y.ptr)))
                tk.append(_ms_per_launch(
                    lambda: m.launch_multi(X.ptr, Y.ptr, k)))
            t1, tk = float(np.median(t1)), float(np.median(tk))
            model = m.multi_bytes(k) / (k * m.multi_bytes(1))
            line = ("multi-vector %-13s %s k=%d  single %.4f ms  multi %.4f ms "
                    "(%.4f per vector, %.3f of 8 TB/s)  ratio to k singles "
                    "%.3f (bytes: %.3f)"
                    % (tag, fmt, k, t1, tk, tk / k,
                       m.multi_bytes(k) / (tk * 1e-3) / PEAK, tk / (k * t1),
                       model))
            print(line)
            getattr(request.config, "_summary_lines", []).append(line)
            if not tk < k * t1:
                slower.append((tag, fmt, k, tk, k * t1))
        for b in (h, d):
            b.release()
        for b in (x, y, X, Y):
            b.free()
    assert not slower, slower
