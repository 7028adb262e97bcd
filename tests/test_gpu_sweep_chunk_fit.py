"""The sweep kernel with chunks of 4608 slots (576 lanes x 2 groups, 384 x 3)
and the plan rule that takes such a shape where the COUNTED steps fall by
10 % (panel_launch.h "Chunk fit").

Bucket lengths at every edge of a chunk -- 0, 1, CH - 1, CH, CH + 1, 2 CH and
2 CH + 1 entries for CH = 4608 and for the built-in 4096 -- in a first tile,
in a last tile shorter than tile_rows, beside a last panel narrower than the
panel width; every shape in ordered and in arrival-order mode against the
oracle's row sums; the ordered arms bit for bit over 200 launches and after a
rebuild from the layout string.  The geometry is the same on every device:
reserve_cus leaves the sweep eight compute units, one per XCD.
"""
import numpy as np
import pytest

import _oracle as O
import spmv_scpa_amd as S

pytestmark = pytest.mark.gpu

REL_TOL = 1e-6   # tests/test_gpu_parity.py: relative, fp64 ...
TIGHT = 1e-12    # ... plus this much of the row scale sum_j |a_ij x_j|

FIT_CH, BUILTIN_CH = 4608, 4096
FIT_576, FIT_384, BUILTIN = 1 << 16, 2 << 16, 3 << 16  # variant bits 16-17
EIGHT_CUS = 100000  # reserve_cus: the build keeps one CU per XCD

TILE_ROWS, PANEL_COLS = 384, 1024
M = 7 * TILE_ROWS + 327       # eight tiles, the last one 327 rows
SIZES = [0, 1]
for _ch in (FIT_CH, BUILTIN_CH):
    SIZES += [_ch - 1, _ch, _ch + 1, 2 * _ch, 2 * _ch + 1]
N = len(SIZES) * PANEL_COLS + 300  # ... and a last panel of 300 columns
PANELS = len(SIZES) + 1


def _steps(lengths, ch):
    # what k_tiles_sweep walks: ceil(n / ch) chunks, one for an empty bucket
    return int(sum(max(1, -(-int(n) // ch)) for n in lengths))


@pytest.fixture(scope="module")
def edges():
    """CSR arrays whose (tile, panel) buckets have prescribed lengths, x, the
    oracle's y and row scale: computed once, read only"""
    rng = np.random.default_rng(4608)
    want = np.zeros((8, PANELS), dtype=np.int64)
    want[0, :len(SIZES)] = SIZES
    want[0, -1] = 1                      # one entry in the narrow panel
    want[7, :len(SIZES)] = SIZES[::-1]   # the short tile: the other order
    want[7, -1] = FIT_CH + 1             # ... and a narrow panel of two chunks
    want[1:7] = rng.integers(0, 40, (6, PANELS))
    want[3, 2] = 0
    rows, cols = [], []
    for t in range(8):
        h = min(TILE_ROWS, M - t * TILE_ROWS)
        for p in range(PANELS):
            w = min(PANEL_COLS, N - p * PANEL_COLS)
            assert want[t, p] <= h * w
            cell = rng.choice(h * w, int(want[t, p]), replace=False)
            rows.append(t * TILE_ROWS + cell // w)
            cols.append(p * PANEL_COLS + cell % w)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    IRP = np.zeros(M + 1, dtype=np.int32)
    np.add.at(IRP, rows + 1, 1)
    IRP = np.cumsum(IRP, dtype=np.int64).astype(np.int32)
    JA = cols.astype(np.int32)
    AS = rng.uniform(-1.0, 1.0, len(JA))
    x = rng.uniform(-1.0, 1.0, N)
    y = O.csr_spmv(IRP, JA, AS, x)
    scale = O.csr_abs_spmv(IRP, JA, AS, x)
    for a in (IRP, JA, AS, x, y, scale):
        a.setflags(write=False)
    return dict(IRP=IRP, JA=JA, AS=AS, x=x, y=y, scale=scale,
                lengths=want.reshape(-1))


def _close(y, e):
    err = np.abs(y - e["y"])
    bound = REL_TOL * np.abs(e["y"]) + TIGHT * e["scale"]
    worst = int(np.argmax(err / np.maximum(bound, 1e-300)))
    print("largest error against its bound: %.3e at row %d (bound %.3e)"
          % (err[worst], worst, bound[worst]))
    return bool(np.all(err <= bound))


def _upload(e):
    A = S.csr_from_arrays("chunk_fit", M, N, e["IRP"], e["JA"], e["AS"])
    dA = S.CsrDevice.upload(A)
    return A, dA


def _build(dA, ordered):
    dA.build_panels(PANEL_COLS, "sweep", sweep_wgs_per_cu=1,
                    reserve_cus=EIGHT_CUS, deterministic=ordered)
    assert dA.panels_tile_rows() == TILE_ROWS, dA.panels_describe()
    assert dA.panels_info()["tiles"] == 8
    assert dA.panels_info()["panels"] == PANELS


@pytest.mark.parametrize("ordered", [True, False],
                         ids=["ordered", "arrival"])
@pytest.mark.parametrize("variant,shape", [(FIT_576, (576, 2)),
                                           (FIT_384, (384, 3)),
                                           (BUILTIN, (512, 2))],
                         ids=["576x2", "384x3", "512x2"])
def test_buckets_at_every_chunk_edge(edges, variant, shape, ordered):
    e = edges
    A, dA = _upload(e)
    d_x, d_y = S.DevBuffer.from_numpy(e["x"]), S.DevBuffer(M * 8)
    try:
        _build(dA, ordered)
        assert dA.panels_info()["entries"] == len(e["JA"])
        assert dA.panels_plan(variant=variant) == shape + (int(ordered),)
        # the device's count of steps is the host's, for both chunks
        assert dA.panels_fit_steps() == (_steps(e["lengths"], BUILTIN_CH),
                                         _steps(e["lengths"], FIT_CH))
        # NaNs: every row must be written
        S._check(S._lib.spmv_dev_memset(d_y.ptr, 0xFF, M * 8, None),
                 "spmv_dev_memset")
        dA.launch(S.CSR_KERNEL_PANELS, d_x.ptr, d_y.ptr, variant=variant)
        S.stream_sync()
        y0 = d_y.to_numpy(np.float64, M)
        assert _close(y0, e)
        if not ordered:
            return
        for it in range(200):
            dA.launch(S.CSR_KERNEL_PANELS, d_x.ptr, d_y.ptr, variant=variant)
            if it % 50 == 49:
                S.stream_sync()
                assert np.array_equal(
                    d_y.to_numpy(np.float64, M).view(np.uint64),
                    y0.view(np.uint64)), it
        # rebuilt from its layout string: the same order, the same bits
        pin = dA.panels_pin()
        assert "chunk_fit=1" in pin
        dA.build_panels_pinned(pin)
        assert dA.panels_pin() == pin
        dA.launch(S.CSR_KERNEL_PANELS, d_x.ptr, d_y.ptr, variant=variant)
        S.stream_sync()
        assert np.array_equal(d_y.to_numpy(np.float64, M).view(np.uint64),
                              y0.view(np.uint64))
    finally:
        dA.release()
        S.csr_free(A)
        d_x.free()
        d_y.free()


# the headline's geometry on eight compute units: 19 552-row tiles, panels of
# 2^17 columns and 32 entries per 10^7 columns, so that a full bucket holds
# 19552 * 4 * 2^17 / 1.25e6 = 8200.7 entries on average: 2 * 4096 + 8.7
HM, HN, HK, HW = 8 * 19531, 1_250_000, 4, 1 << 30


@pytest.fixture(scope="module")
def headline():
    A = S.CsrDevice.generate(S.SYNTH_RANDOM, HM, HN, HK, HW, 0, 42)
    d_x, d_y = S.DevBuffer(HN * 8), S.DevBuffer(HM * 8)
    S.dev_fill_synth(d_x.ptr, HN, 7)
    rows = np.random.default_rng(3).integers(0, HM, 200)
    want = [O.synth_row_dot(S.SYNTH_RANDOM, HM, HN, HK, HW, 0, 42, 7, int(r))
            for r in rows]
    # the same matrix on the host: the length of every (tile, panel) bucket
    IRP, JA, _ = O.synth_csr(S.SYNTH_RANDOM, HM, HN, HK, HW, 42)
    tile = np.repeat(np.arange(HM), np.diff(IRP)) // 19552
    lengths = np.bincount(tile * 10 + (JA >> 17), minlength=80)
    yield A, d_x, d_y, rows, want, lengths
    A.release()
    d_x.free()
    d_y.free()


def _headline_rows_ok(A, d_x, d_y, rows, want):
    A.launch(S.CSR_KERNEL_PANELS, d_x.ptr, d_y.ptr)
    S.stream_sync()
    y = d_y.to_numpy(np.float64, HM)
    return all(abs(y[r] - w) <= REL_TOL * abs(w) + TIGHT * sc
               for r, (w, sc) in zip(rows, want))


def test_headline_geometry_plans_a_4608_slot_shape(headline):
    A, d_x, d_y, rows, want, lengths = headline
    A.build_panels(1 << 17, "sweep", reserve_cus=EIGHT_CUS)
    print(A.panels_describe())
    assert A.panels_tile_rows() == 19552
    assert "(1 wg/cu" in A.panels_describe()
    builtin, fit = A.panels_fit_steps()
    print("steps: %d with 4096-slot chunks, %d with 4608" % (builtin, fit))
    assert len(lengths) == 80 and lengths.sum() == HM * HK
    full = lengths.reshape(8, 10)[:, :9]
    print("full buckets: mean %.1f, %d of 72 above 8192, longest %d"
          % (full.mean(), int((full > 2 * BUILTIN_CH).sum()), full.max()))
    assert (builtin, fit) == (_steps(lengths, BUILTIN_CH),
                              _steps(lengths, FIT_CH))
    # 72 full buckets at 8200.7 +- 90 entries: two chunks of 4608 each; about
    # half of them a third chunk of 4096
    assert full.max() <= 2 * FIT_CH and fit <= 8 * (9 * 2 + 2)
    assert fit * 100 <= builtin * 90
    threads, groups, ordered = A.panels_plan()
    assert threads * groups * 4 == FIT_CH and ordered == 1
    assert _headline_rows_ok(A, d_x, d_y, rows, want)
    # an explicit request keeps its meaning
    assert A.panels_plan(waves_per_block=8) == (512, 2, 1)
    assert A.panels_plan(waves_per_block=16) == (1024, 1, 1)
    assert A.panels_plan(variant=BUILTIN) == (512, 2, 1)


def test_zeroed_field_plans_the_builtin_shape(headline):
    A, d_x, d_y, rows, want, lengths = headline
    A.build_panels(1 << 17, "sweep", reserve_cus=EIGHT_CUS)
    assert A.panels_plan()[0] * A.panels_plan()[1] * 4 == FIT_CH
    A.panels_set_fit_steps(0, 0)
    assert A.panels_fit_steps() == (0, 0)
    assert A.panels_plan() == (512, 2, 1)
    assert _headline_rows_ok(A, d_x, d_y, rows, want)
    # a layout string without the field -- every string written before the
    # field existed -- rebuilds such a copy; one with it, the counted one
    pin = A.panels_pin()
    assert "chunk_fit" not in pin
    A.build_panels_pinned(pin)
    assert A.panels_fit_steps() == (0, 0) and A.panels_plan() == (512, 2, 1)
    A.build_panels_pinned(pin + ",chunk_fit=1")
    assert A.panels_fit_steps()[1] == _steps(lengths, FIT_CH)
    assert A.panels_plan()[0] * A.panels_plan()[1] * 4 == FIT_CH
