"""Compact column-major HLL handles on the GPU: one base column per hack block
and a 16-bit offset per slot (spmv_hll_to_index16, hll_kernels.hip).

The expected result needs no oracle and no tolerance: for finite x a compact
handle gives THE BITS of launch(1) on its 4-byte source handle -- either
kernel id, every workgroup order, every waves_per_block, both value types.
The source's own result is held to the project's parity bound (1e-12 of the
row scale) against the CPU oracle once per case, so a wrong source cannot
hide a wrong copy.

Every test runs under a time limit of its own: a test that exceeds it ends
the whole process, so nothing else is started on the device.
"""
import errno
import faulthandler

import numpy as np
import pytest

import _index16 as I
import _oracle as O
import spmv_scpa_amd as S

pytestmark = pytest.mark.gpu

TIGHT = 1e-12  # the project's parity bound (of the row scale)
CHUNK = 8      # columns per staged chunk of kernel 1 (CH, hll_kernels.hip)
ORDERS = (1, 2, 4)  # variant bit: hardware / XCD ranges / grouped


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(240, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


class Runner:
    """launches on device-resident x / y; y is NaN before every launch"""

    def __init__(self, M, x):
        self.M = M
        self.x = S.DevBuffer.from_numpy(np.ascontiguousarray(x, np.float64))
        self.y = S.DevBuffer(max(M, 1) * 8)

    def run(self, m, kernel, **kw):
        S._check(S._lib.spmv_dev_memset(self.y.ptr, 0xFF, max(self.M, 1) * 8,
                                        None), "spmv_dev_memset")
        m.launch(kernel, self.x.ptr, self.y.ptr, **kw)
        S.stream_sync()
        return self.y.to_numpy(np.float64, self.M)

    def free(self):
        self.x.free()
        self.y.free()


def sources(M, N, IRP, JA, AS, name="t"):
    """-> {8: f64 col-major HLL handle, 4: f32 one} by device conversion"""
    A = S.csr_from_arrays(name, M, N, np.asarray(IRP, np.int32),
                          np.asarray(JA, np.int32), np.asarray(AS, np.float64))
    d64 = S.CsrDevice.upload(A)
    d32 = d64.to_f32()
    out = {8: d64.to_hll(True), 4: d32.to_hll(True)}
    d32.release()
    d64.release()
    S.csr_free(A)
    return out


def from_rows(rows, N, seed=5):
    """rows: list of column lists -> (M, N, IRP, JA, AS), values in +-[1, 2)"""
    rng = np.random.default_rng(seed)
    IRP = np.zeros(len(rows) + 1, np.int32)
    IRP[1:] = np.cumsum([len(r) for r in rows])
    JA = np.array([c for r in rows for c in sorted(r)], np.int32)
    AS = rng.uniform(1.0, 2.0, len(JA)) * rng.choice([-1.0, 1.0], len(JA))
    return len(rows), N, IRP, JA, AS


def check_against_packer(C, IRP, JA, AS):
    p = I.pack16(IRP, JA, AS)
    base, off16 = C.download_index16()
    assert base.dtype == np.int32 and off16.dtype == np.uint16
    assert len(base) == C.num_blocks and len(off16) == C.slots
    assert np.array_equal(base, p["base"])
    ok = ~p["pad"]
    blk = np.repeat(np.arange(C.num_blocks), np.diff(p["off"]))
    col = base[blk].astype(np.int64) + off16
    assert np.array_equal(col[ok], p["ja"][ok])
    # the pads too: the previous valid column, or offset 0 for an empty row
    assert np.array_equal(off16, p["off16"])
    return p


def check_identity(M, N, IRP, JA, AS, x, tag, waves=(1, 4, 8, 16)):
    """both value types: conversion, stored form, and the bits of y for
    kernels 1 / 2 x three orders x `waves`.  -> y of the f64 source"""
    src = sources(M, N, IRP, JA, AS)
    run = Runner(M, x)
    y64 = None
    for vb, H in src.items():
        y_ref = run.run(H, 1)
        if vb == 8:
            y64 = y_ref
            # once per case: the source itself is right
            want = O.csr_spmv(IRP, JA, AS, x)
            scale = O.csr_abs_spmv(IRP, JA, AS, x)
            err = (np.max(np.abs(y_ref - want) / np.maximum(scale, 1e-300))
                   if M else 0.0)
            assert err <= TIGHT, (tag, err)
        C = H.to_index16()
        assert C.index_bytes == 2 and H.index_bytes == 4
        assert C.value_bytes == vb and C.col_major
        assert (C.M, C.N, C.NZ, C.num_blocks, C.slots) == (
            H.M, H.N, H.NZ, H.num_blocks, H.slots)
        check_against_packer(C, IRP, JA, AS)
        assert np.array_equal(bits(run.run(C, 1)), bits(y_ref)), (tag, vb)
        for k in (1, 2):
            for order in ORDERS:
                for w in waves:
                    y = run.run(C, k, variant=order, waves_per_block=w)
                    assert np.array_equal(bits(y), bits(y_ref)), (
                        tag, vb, k, order, w)
        # the source is untouched and outlives the copy
        C.release()
        assert np.array_equal(bits(run.run(H, 1)), bits(y_ref)), (tag, vb)
        H.release()
    run.free()
    return y64


# ------------------------------------------------- 1. + 3. the project's cases
@pytest.mark.parametrize("case", I.CASES)
def test_same_bits_as_the_source_on_every_kernel_order_and_width(case):
    M, N, IRP, JA, AS, x = I.case_arrays(case)
    check_identity(M, N, IRP, JA, AS, x, case)


# ------------------------------------------------------- 2. hand-made shapes
def _rand_rows(M, N, maxlen, seed):
    rng = np.random.default_rng(seed)
    return [sorted(rng.choice(N, rng.integers(0, maxlen + 1), replace=False))
            for _ in range(M)]


@pytest.mark.parametrize("M", [0, 1, 31, 33, 65])
def test_few_rows(M):
    N = 200
    M, N, IRP, JA, AS = from_rows(_rand_rows(M, N, 5, M + 1), N)
    y = check_identity(M, N, IRP, JA, AS, O.synth_x(7, 0, N), ("rows", M),
                       waves=(1, 8))
    assert len(y) == M


def test_a_block_of_width_zero_between_non_empty_blocks():
    N = 300
    rows = _rand_rows(32, N, 6, 1) + [[] for _ in range(32)] + \
        _rand_rows(32, N, 6, 2) + [[] for _ in range(32)] + _rand_rows(7, N, 6, 3)
    M, N, IRP, JA, AS = from_rows(rows, N)
    y = check_identity(M, N, IRP, JA, AS, O.synth_x(7, 0, N), "width 0",
                       waves=(1, 8))
    assert np.array_equal(bits(y[32:64]), bits(np.zeros(32)))
    assert np.array_equal(bits(y[96:128]), bits(np.zeros(32)))
    src = sources(M, N, IRP, JA, AS)
    C = src[8].to_index16()
    base, _ = C.download_index16()
    assert base[1] == 0 and base[3] == 0  # a block without entries: base 0
    for h in (C, src[8], src[4]):
        h.release()


@pytest.mark.parametrize("wA,wB", [(1, 1), (CHUNK - 1, CHUNK - 1),
                                   (CHUNK, CHUNK), (CHUNK + 1, CHUNK + 1),
                                   (2 * CHUNK + 3, 2 * CHUNK + 3),
                                   (3, 2 * CHUNK + 3), (2 * CHUNK + 3, 3),
                                   (CHUNK, 0), (0, CHUNK + 1)])
def test_widths_around_the_chunk_and_pairs_of_unequal_width(wA, wB):
    """one pair of blocks (+ a third, alone in its pair): every row of block A
    has wA entries, of block B wB; some rows one entry fewer (pads)"""
    N = 500
    rng = np.random.default_rng(wA * 100 + wB)
    rows = []
    for w in (wA, wB, CHUNK + 2):
        for i in range(32):
            n = w - 1 if (w > 0 and i % 5 == 4) else w
            rows.append(sorted(rng.choice(N, n, replace=False)))
    M, N, IRP, JA, AS = from_rows(rows, N)
    check_identity(M, N, IRP, JA, AS, O.synth_x(7, 0, N), ("widths", wA, wB),
                   waves=(1, 8))


def test_empty_rows_in_a_block_whose_columns_start_far_right():
    """the pad re-pointing case: the column-0 pads of the empty rows lie
    outside [base, base + 65535] and are stored as offset 0"""
    N = 200_000
    rng = np.random.default_rng(9)
    rows = []
    for i in range(70):
        rows.append([] if i % 3 == 1 else
                    sorted(100_000 + rng.choice(5000, 1 + i % 4, replace=False)))
    M, N, IRP, JA, AS = from_rows(rows, N)
    x = O.synth_x(7, 0, N)
    y = check_identity(M, N, IRP, JA, AS, x, "far right", waves=(1, 8))
    empty = np.array([i % 3 == 1 for i in range(70)])
    src = sources(M, N, IRP, JA, AS)
    run = Runner(M, x)
    for vb, H in src.items():
        C = H.to_index16()
        base, off16 = C.download_index16()
        assert np.all(base >= 100_000)
        for k in (1, 2):
            y = run.run(C, k)
            assert np.array_equal(bits(y[empty]), bits(np.zeros(empty.sum())))
        C.release()
        H.release()
    run.free()


def _two_column_block(c0, gap):
    """33 rows: row 0 holds {c0, c0 + gap}, the others one column between"""
    rows = [[c0, c0 + gap]] + [[c0 + 1 + i] for i in range(32)]
    return from_rows(rows, c0 + gap + 10)


def test_a_span_of_exactly_65535_converts():
    c0 = 1234
    M, N, IRP, JA, AS = _two_column_block(c0, 65535)
    check_identity(M, N, IRP, JA, AS, O.synth_x(7, 0, N), "span 65535",
                   waves=(1, 8))
    src = sources(M, N, IRP, JA, AS)
    C = src[8].to_index16()
    base, off16 = C.download_index16()
    assert base[0] == c0 and off16.max() == 65535
    assert int(np.sum(off16 == 65535)) == 1
    for h in (C, src[8], src[4]):
        h.release()


def test_a_span_of_65536_is_erange_and_leaks_nothing():
    M, N, IRP, JA, AS = _two_column_block(1234, 65536)
    src = sources(M, N, IRP, JA, AS)
    for H in src.values():  # the one-off allocations of a first use
        with pytest.raises(OSError):
            H.to_index16()
    S.device_sync()
    live, free0 = S._lib.spmv_live_handles(), S.dev_mem_info()[0]
    for H in src.values():
        with pytest.raises(OSError) as ei:
            H.to_index16()
        assert ei.value.errno == errno.ERANGE
    S.device_sync()
    assert S._lib.spmv_live_handles() == live
    assert S.dev_mem_info()[0] == free0
    assert sorted(S.live_objects(), key=id) == sorted(src.values(), key=id)
    for H in src.values():
        H.release()


def test_random_columns_anywhere_are_erange():
    d = S.CsrDevice.generate(S.SYNTH_RANDOM, 131_072, 131_072, 8, 1 << 30, 0, 42)
    H = d.to_hll(True)
    live = S._lib.spmv_live_handles()
    with pytest.raises(OSError) as ei:
        H.to_index16()
    assert ei.value.errno == errno.ERANGE
    assert S._lib.spmv_live_handles() == live
    H.release()
    d.release()


def test_a_hack_block_wider_than_512_columns_is_enotsup():
    rows = _rand_rows(40, 2000, 4, 3)
    rows[17] = list(range(100, 700))  # 600 entries: a wide block
    M, N, IRP, JA, AS = from_rows(rows, 2000)
    src = sources(M, N, IRP, JA, AS)
    live = S._lib.spmv_live_handles()
    for H in src.values():
        with pytest.raises(OSError) as ei:
            H.to_index16()
        assert ei.value.errno == errno.ENOTSUP
        H.release()
    assert S._lib.spmv_live_handles() == live - 2


# ------------------------------------------------------------ 4. launch_blocks
@pytest.mark.parametrize("case", ["synth:banded", "synth:ragged"])
def test_launch_blocks_on_proper_sub_ranges(case):
    M, N, IRP, JA, AS, x = I.case_arrays(case)
    src = sources(M, N, IRP, JA, AS)
    run = Runner(M, x)
    for vb, H in src.items():
        y_ref = run.run(H, 1)
        C = H.to_index16()
        nb = C.num_blocks
        # even and odd first block; the last range ends at the (ragged) end
        for b0, b1 in ((nb // 3 & ~1, nb - nb // 4), (nb // 3 | 1, nb - 7),
                       (1, nb), (nb - 1, nb), (4, 5)):
            for k in (1, 2):
                for order in ORDERS:
                    y = run.run(C, k, blocks=(b0, b1), variant=order)
                    r0, r1 = b0 * 32, min(b1 * 32, M)
                    assert np.array_equal(bits(y[r0:r1]), bits(y_ref[r0:r1])), (
                        case, vb, k, order, b0, b1)
                    assert np.all(np.isnan(y[:r0])) and np.all(np.isnan(y[r1:]))
        C.release()
        H.release()
    run.free()


# ------------------------------------------------------------- 5. graph replay
def test_a_captured_launch_replays_with_a_changed_x():
    M, N, IRP, JA, AS, _ = I.case_arrays("synth:ragged")
    src = sources(M, N, IRP, JA, AS)
    x, y = S.DevBuffer(N * 8), S.DevBuffer(M * 8)
    side = S.Stream()
    for vb, H in src.items():
        C = H.to_index16()
        for k in (1, 2):
            S.dev_fill_synth(x.ptr, N, 7, 0, side.ptr)
            C.launch(k, x.ptr, y.ptr, stream=side.ptr)  # eagerly once, first
            side.sync()
            with side.capture() as g:
                C.launch(k, x.ptr, y.ptr, stream=side.ptr)
            for seed in (7, 8):  # the graph reads x where it lives
                S.dev_fill_synth(x.ptr, N, seed, 0, side.ptr)
                H.launch(1, x.ptr, y.ptr, stream=side.ptr)
                side.sync()
                y_ref = y.to_numpy(np.float64, M)
                S._check(S._lib.spmv_dev_memset(y.ptr, 0xFF, M * 8, side.ptr),
                         "spmv_dev_memset")
                g.launch(side.ptr)
                side.sync()
                assert np.array_equal(bits(y.to_numpy(np.float64, M)),
                                      bits(y_ref)), (vb, k, seed)
            g.destroy()
        C.release()
        H.release()
    x.free()
    y.free()


# ------------------------------------------------------------------ 6. autotune
def test_autotune_times_kernels_1_and_2_and_skips_the_blocked_path():
    M, N, IRP, JA, AS, x = I.case_arrays("synth:random_narrow")
    src = sources(M, N, IRP, JA, AS)
    run = Runner(M, x)
    for vb, H in src.items():
        y_ref = run.run(H, 1)
        C = H.to_index16()
        best, ms = C.autotune(run.x.ptr, run.y.ptr, allow_panels=True)
        assert best in (1, 2) and ms > 0.0, (best, ms)
        log = C.tune_log()
        assert "blocked path: skipped" in log, log
        t = C.tune_times()
        assert t[1] > 0.0 and t[2] > 0.0 and t[0] == 0.0 and t[3] == 0.0
        assert t[S.HLL_KERNEL_PANELS] == 0.0 and C.panels_info() is None
        assert np.array_equal(bits(run.run(C, best)), bits(y_ref)), (vb, best)
        ts = C.time(best, run.x.ptr, run.y.ptr, 1, 3)
        assert len(ts) == 3 and np.all(ts > 0.0)
        C.release()
        H.release()
    run.free()


# ------------------------------------------------------------------ 7. refusals
def test_what_a_compact_handle_refuses_and_nothing_leaks():
    M, N, IRP, JA, AS, xs = I.case_arrays("mtx:ragged100")
    A = S.csr_from_arrays("refuse", M, N, IRP, JA, AS)
    d = S.CsrDevice.upload(A)
    H, Hrow = d.to_hll(True), d.to_hll(False)
    C = H.to_index16()
    x, y = S.DevBuffer.from_numpy(np.tile(xs, 8)), S.DevBuffer(M * 8 * 8)
    live = S._lib.spmv_live_handles()

    def refused(code, call):
        with pytest.raises(OSError) as ei:
            call()
        assert ei.value.errno == code, (ei.value, code)

    refused(errno.ENOTSUP, C.build_panels)
    refused(errno.ENOTSUP, lambda: C.build_panels(0, "chain", 4096))
    refused(errno.ENOTSUP, lambda: C.launch_multi(x.ptr, y.ptr, 2))
    refused(errno.ENOTSUP, lambda: C.multi_bytes(2))
    refused(errno.EINVAL, C.to_index16)       # already compact
    refused(errno.EINVAL, Hrow.to_index16)    # row-major source
    refused(errno.EINVAL, H.download_index16)  # a 4-byte handle has none
    for k in (0, 3, S.HLL_KERNEL_PANELS, 5, -1):
        refused(errno.EINVAL, lambda: C.launch(k, x.ptr, y.ptr))
    refused(errno.EINVAL, lambda: C.launch(1, x.ptr, y.ptr, variant=8))
    refused(errno.ENOENT, C.release_source)   # no blocked copy to keep
    assert C.panels_info() is None
    # a source that kept only its blocked copy has no columns to convert
    H.build_panels(1024)
    H.release_source()
    refused(errno.ENODATA, H.to_index16)
    assert S._lib.spmv_live_handles() == live
    # ... and the copy made before does not depend on it
    H.release()
    C.launch(2, x.ptr, y.ptr)
    S.stream_sync()
    want = O.csr_spmv(IRP, JA, AS, xs)
    scale = O.csr_abs_spmv(IRP, JA, AS, xs)
    err = np.max(np.abs(y.to_numpy(np.float64, M) - want) /
                 np.maximum(scale, 1e-300))
    assert err <= TIGHT, err
    for h in (C, Hrow, d):
        h.release()
    x.free()
    y.free()
    S.csr_free(A)


# --------------------------------------------------------------- 8. byte counts
def test_byte_counts_follow_the_formula():
    M, N, IRP, JA, AS, _ = I.case_arrays("synth:ragged")
    src = sources(M, N, IRP, JA, AS)
    for vb, H in src.items():
        C = H.to_index16()
        nb, slots = C.num_blocks, C.slots
        want = (2 + vb) * slots + 4 * nb + 12 * nb + 8 * M + 8 * N
        assert C.algorithmic_bytes == want
        for k in (1, 2):
            assert C.kernel_bytes(k) == want
        assert H.algorithmic_bytes == (4 + vb) * slots + 12 * nb + 8 * M + 8 * N
        assert H.algorithmic_bytes - C.algorithmic_bytes == 2 * slots - 4 * nb
        C.release()
        H.release()
