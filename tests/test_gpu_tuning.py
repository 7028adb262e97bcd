"""Tuning expectations of the measured selector and of the blocked copy's
geometry, kept apart from the parity tests: a change of heuristics may turn
these red without saying anything about correctness.
They state what the committed profiles/ and DESIGN.md claim."""
import numpy as np
import pytest

import spmv_scpa_amd as S

pytestmark = pytest.mark.gpu


def test_sweep_geometry_for_config3():
    """10M x 10M, columns anywhere: the sweep schedule holds one row tile per
    workgroup and round -- 2 rounds of 256 tiles of <= 20448 rows with
    2^17-column panels, or of 512 tiles of <= 10208 rows with 2^18."""
    M = N = 10_000_000
    dA = S.CsrDevice.generate(S.SYNTH_RANDOM, M, N, 32, 1 << 30, 0, 42)
    dH = dA.to_hll(True)
    dA.release()
    try:
        dH.build_panels(0, "sweep")
        info = dH.panels_info()
        assert info["steps"] == 1
        assert (info["tiles"], info["panels"]) in ((512, 77), (1022, 39))
        # leaving CUs to a neighbour kernel shrinks the grid, not the coverage
        dH.build_panels(0, "sweep", reserve_cus=16)
        info2 = dH.panels_info()
        assert info2["entries"] == info["entries"] and info2["steps"] == 1
        assert info2["tiles"] >= info["tiles"]
    finally:
        dH.release()


def test_autotune_picks_the_blocked_path_when_columns_are_anywhere():
    """one rank's shard of config 5 (80M columns): ~6 ms direct vs ~3 ms
    blocked -- the selector must see that.  WHICH blocked schedule wins is a
    timing outcome (sweep 3.0 vs chain 3.4 ms here, within noise of each
    other at 10M columns): the property is the pick and its time, not the
    schedule's name."""
    M, N = 10_000_000, 80_000_000
    dA = S.CsrDevice.generate(S.SYNTH_RANDOM, M, N, 32, 1 << 30, 3 * M, 42)
    dH = dA.to_hll(True)
    dA.release()
    d_x, d_y = S.DevBuffer(N * 8), S.DevBuffer(M * 8)
    try:
        S.dev_fill_synth(d_x.ptr, N, 7)
        best, ms = dH.autotune(d_x.ptr, d_y.ptr)
        assert best == S.HLL_KERNEL_PANELS
        assert dH.panels_schedule() in ("sweep", "chain")
        direct = float(np.median(dH.time(1, d_x.ptr, d_y.ptr, 1, 3)))
        assert ms < 0.7 * direct, (ms, direct)
    finally:
        dH.release()
        d_x.free()
        d_y.free()


def test_autotune_times_small_matrices_out_of_the_infinity_cache():
    """config 2 (212 MB working set < 256 MB Infinity Cache): the selector
    flushes between launches, so its time is the HBM-regime time the bench
    reports, within noise of an explicitly flushed timing of its pick."""
    M = N = 1_000_000
    dA = S.CsrDevice.generate(S.SYNTH_BANDED, M, N, 16, 0, 0, 42)
    d_x, d_y = S.DevBuffer(N * 8), S.DevBuffer(M * 8)
    try:
        S.dev_fill_synth(d_x.ptr, N, 7)
        best, ms = dA.autotune(d_x.ptr, d_y.ptr)
        flushed = float(np.median(dA.time(best, d_x.ptr, d_y.ptr, warmup=2,
                                          iters=10, flush_bytes=1 << 30)))
        cached = float(np.median(dA.time(best, d_x.ptr, d_y.ptr, warmup=2,
                                         iters=10, flush_bytes=0)))
        assert abs(ms - flushed) <= 0.25 * flushed + 0.01, (ms, flushed, cached)
    finally:
        dA.release()
        d_x.free()
        d_y.free()


@pytest.mark.parametrize("kind,M,K,W", [
    (S.SYNTH_POWERLAW, 2_000_000, 3, 1 << 30),   # webbase / amazon class
    (S.SYNTH_HUB, 1_000_000, 6, 4096),           # dc1 class
], ids=["powerlaw", "hub"])
def test_selector_on_the_reference_s_irregular_classes(kind, M, K, W):
    """on very short rows the selector MEASURES the
    thread-per-row kernel (the reference's plots show it winning on roadNet /
    amazon, cuda_csr.cu:19-31), and the block-per-row kernel when one row is
    far longer than the rest -- and neither wins on wave64: the pick is the
    stream kernel or the blocked copy, several times faster.  A hub row of
    131 072 entries must not serialise the launch (stream kernel: segments;
    blocked copy: the row beside it)."""
    dA = S.CsrDevice.generate(kind, M, M, K, W, 0, 42)
    d_x, d_y = S.DevBuffer(M * 8), S.DevBuffer(M * 8)
    dH = None
    try:
        S.dev_fill_synth(d_x.ptr, M, 7)
        best, ms = dA.autotune(d_x.ptr, d_y.ptr)
        t = dA.tune_times()
        assert best in (4, S.CSR_KERNEL_PANELS), (best, t)
        assert t[4] > 0 and t[2] > 0          # always candidates
        if dA.NZ / dA.M < 6:
            assert t[0] > 0, t                # thread_row was measured ...
            # ... and lost by > 2x (3.5-6x measured, with four loads in flight
            # per lane; 9-15x with one)
            assert ms < 0.5 * t[0], (ms, t)
        if kind == S.SYNTH_HUB:
            assert t[3] > 0, t                # block_row measured, and lost
            assert ms < 0.5 * t[3], (ms, t)
            # the hub row (131 072 entries) is spread over workgroups: the
            # stream kernel runs within 3x of the blocked pick, not 8x off
            assert t[4] < 3.0 * ms + 0.02, (ms, t)
            dH = dA.to_hll(True)
            bh, mh = dH.autotune(d_x.ptr, d_y.ptr)
            assert bh == S.HLL_KERNEL_PANELS     # the format pads 2.3x
            assert "long row(s) beside" in dH.panels_describe()
            assert mh < 2.0 * ms + 0.02, (mh, ms)   # was 4x the CSR time
            # the blocked copy stores no padding: priced on the true entries,
            # or a padded format would read > 100 % of the roofline
            assert dH.kernel_bytes(bh) < dH.algorithmic_bytes
            assert dH.kernel_bytes(bh) / (mh * 1e6) / 8000.0 < 1.0
        log = dA.tune_log()
        assert "direct kernels" in log and "total" in log
    finally:
        if dH is not None:
            dH.release()
        dA.release()
        d_x.free()
        d_y.free()


# ---- the build side of the blocked path (panel_build.h, panels_build) ----
def _csr(M, N, lens, start, step):
    """row r holds lens[r] distinct columns (start[r] + k * step) mod N,
    ascending; values are small binary fractions, never zero"""
    lens = np.asarray(lens, dtype=np.int64)
    IRP = np.zeros(M + 1, dtype=np.int64)
    np.cumsum(lens, out=IRP[1:])
    rows = np.repeat(np.arange(M, dtype=np.int64), lens)
    k = np.arange(IRP[-1], dtype=np.int64) - IRP[rows]
    JA = (np.asarray(start, dtype=np.int64)[rows] + k * step) % max(N, 1)
    AS = ((rows * 31 + k * 17) % 13 - 6) / 8.0 + 0.0625
    order = np.lexsort((JA, rows))
    return (IRP.astype(np.int32), JA[order].astype(np.int32),
            AS[order].astype(np.float64))


def _geometry_matrices():
    """the smallest shapes at which the build can go wrong: name -> (M, N,
    IRP, JA, AS)"""
    r33, r100 = np.arange(33), np.arange(100)
    ragged33 = 1 + r33 % 5
    ragged33[17] = 0
    long_lens = 1 + r100 % 7
    long_lens[50] = 16400
    m = {
        # one partial tile of 32-row tiles, one empty row
        "partial": (33, 5) + _csr(33, 5, ragged33, r33 * 3, 2),
        # 5 panels of 4096 columns; ragged rows: an HLL source pads
        "ragged": (100, 20000) + _csr(100, 20000, (r100 * 7) % 33,
                                      r100 * 977, 613),
        # every row 32 entries: an HLL source pads nothing
        "const32": (100, 20000) + _csr(100, 20000, np.full(100, 32),
                                       r100 * 977, 613),
        # a band: a 32-row tile touches 2-3 of the 5 panels
        "band": (100, 20000) + _csr(100, 20000, 8 + r100 % 33, r100 * 190, 3),
        # one row of 16400 entries: 17 segments beside the copy
        "long": (100, 20000) + _csr(100, 20000, long_lens, r100 * 977, 613),
        # 8 CUs left of 256: 25000 entries per bucket take one workgroup per
        # CU, 16 tiles in two full rounds of 8 (two per CU: 32 in rounds of 16)
        "rounds": (200000, 1000) + _csr(200000, 1000, np.full(200000, 2),
                                        np.arange(200000) * 7, 501),
        # 8 CUs x 8 workgroups: 126 tiles of 1568 rows, rounds of 64 and 62
        "ragged_round": (196736, 1000) + _csr(196736, 1000,
                                              np.full(196736, 2),
                                              np.arange(196736) * 7, 501),
        "nz0": (64, 64) + _csr(64, 64, np.zeros(64), np.zeros(64), 1),
        "m0": (0, 64) + _csr(0, 64, np.zeros(0), np.zeros(0), 1),
    }
    return m


# (matrix, sources, builds): a build is (tag, keyword arguments of
# build_panels, SPMV_BUCKET_ORDER or None)
_S3 = ("steps", "chain", "sweep")
_GEOMETRY_CASES = [
    ("partial", ("csr",),
     [(s, dict(sched=s, tile_rows=32), None) for s in _S3]),
    ("ragged", ("csr", "hll_row", "hll_col"),
     [(s, dict(panel_cols=4096, sched=s, tile_rows=32), None)
      for s in ("steps", "sweep")]),
    ("const32", ("csr", "hll_row", "hll_col"),
     [(s, dict(panel_cols=4096, sched=s, tile_rows=32), None)
      for s in ("steps", "sweep")]),
    ("band", ("csr",),
     [("chain32", dict(panel_cols=4096, sched="chain", tile_rows=32), None),
      ("chain32 ascending", dict(panel_cols=4096, sched="chain", tile_rows=32),
       "1")]),
    ("ragged", ("csr",),   # columns anywhere: every tile touches every panel
     [("chain32", dict(panel_cols=4096, sched="chain", tile_rows=32), None)]),
    ("long", ("csr", "hll_col"),
     [(s, dict(sched=s), None) for s in ("steps", "sweep")]),
    ("rounds", ("csr",),
     [("sweep reserve 248", dict(sched="sweep", reserve_cus=248), None),
      ("sweep reserve 248 tile-major",
       dict(sched="sweep", reserve_cus=248, sweep_layout=0), None),
      ("sweep reserve 248 2 wg/cu",
       dict(sched="sweep", reserve_cus=248, sweep_wgs_per_cu=2), None)]),
    ("ragged_round", ("csr",),
     [("sweep reserve 248 8 wg/cu",
       dict(sched="sweep", reserve_cus=248, sweep_wgs_per_cu=8), None),
      ("sweep reserve 248 8 wg/cu tile-major",
       dict(sched="sweep", reserve_cus=248, sweep_wgs_per_cu=8,
            sweep_layout=0), None)]),
    ("nz0", ("csr", "hll_col"), [(s, dict(sched=s), None) for s in _S3]),
    ("m0", ("csr",), [(s, dict(sched=s), None) for s in _S3]),
]


def _geometry_rows():
    """build every case, default summation order and deterministic=True ->
    [(key, panels_describe() text, panels_info() as a tuple, SHA-256 of y's
    bytes for the deterministic build or None)]; an OSError of the library is
    recorded as the text "errno N" """
    import hashlib
    import os
    mats = _geometry_matrices()
    rows = []
    env_before = os.environ.get("SPMV_BUCKET_ORDER")
    for name, sources, builds in _GEOMETRY_CASES:
        M, N, IRP, JA, AS = mats[name]
        A = S.csr_from_arrays(name, M, N, IRP, JA, AS)
        d_x, d_y = S.DevBuffer(max(N, 1) * 8), S.DevBuffer(max(M, 1) * 8)
        S.dev_fill_synth(d_x.ptr, N, 7)
        dA = S.CsrDevice.upload(A)
        handles = {"csr": (dA, S.CSR_KERNEL_PANELS)}
        if "hll_row" in sources:
            handles["hll_row"] = (dA.to_hll(False), S.HLL_KERNEL_PANELS)
        if "hll_col" in sources:
            handles["hll_col"] = (dA.to_hll(True), S.HLL_KERNEL_PANELS)
        try:
            for tag, kw, bucket_order in builds:
                for src in sources:
                    m, kid = handles[src]
                    for det in (None, True):
                        key = "%s / %s / %s%s" % (name, src, tag,
                                                  " / det" if det else "")
                        if bucket_order is None:
                            os.environ.pop("SPMV_BUCKET_ORDER", None)
                        else:
                            os.environ["SPMV_BUCKET_ORDER"] = bucket_order
                        try:
                            m.build_panels(deterministic=det, **kw)
                            text = m.panels_describe()
                            info = m.panels_info()
                            info = (info["steps"], info["tiles"],
                                    info["panels"], info["entries"])
                            sha = None
                            if det:
                                S._lib.spmv_dev_memset(d_y.ptr, 0xFF,
                                                       max(M, 1) * 8, None)
                                m.launch(kid, d_x.ptr, d_y.ptr)
                                S.stream_sync()
                                y = d_y.to_numpy(np.float64, M)
                                sha = hashlib.sha256(y.tobytes()).hexdigest()
                        except OSError as e:
                            text, info, sha = "errno %d" % e.errno, None, None
                        rows.append((key, text, info, sha))
        finally:
            os.environ.pop("SPMV_BUCKET_ORDER", None)
            if env_before is not None:
                os.environ["SPMV_BUCKET_ORDER"] = env_before
            for m, _ in handles.values():
                m.release()
            S.csr_free(A)
            d_x.free()
            d_y.free()
    return rows


# What the commit before the build was split into stages (e1024be) answered on
# an MI355X, recorded twice; every hash repeated.  key -> (panels_describe(),
# panels_info() as (steps, tiles, panels, entries), SHA-256 of y or None)
_GEOMETRY_RECORDED = {
    'partial / csr / steps': (
        'steps tiles=2 x 32 rows, panels=1 x 2^18 cols, <=1 buckets per tile '
        '(span 1, ascending order), tile order 0, waves=0',
        (1, 2, 1, 93),
        None),
    'partial / csr / steps / det': (
        'steps tiles=2 x 32 rows, panels=1 x 2^18 cols, <=1 buckets per tile '
        '(span 1, ascending order), tile order 0, waves=0, deterministic',
        (1, 2, 1, 93),
        '3dfc90f90278101f3a16b2b37f92f5549fd953f43a74259cf293132be7a9f4e3'),
    'partial / csr / chain': (
        'chain tiles=2 x 32 rows, panels=1 x 2^18 cols, <=1 buckets per tile '
        '(span 1, ascending order), tile order 0, waves=0',
        (1, 2, 1, 93),
        None),
    'partial / csr / chain / det': (
        'chain tiles=2 x 32 rows, panels=1 x 2^18 cols, <=1 buckets per tile '
        '(span 1, ascending order), tile order 0, waves=0, deterministic',
        (1, 2, 1, 93),
        '3dfc90f90278101f3a16b2b37f92f5549fd953f43a74259cf293132be7a9f4e3'),
    'partial / csr / sweep': (
        'sweep tiles=2 x 32 rows, panels=1 x 2^18 cols, grid=2 (2 wg/cu, '
        'reserve 0), buckets panel-major, waves=0, deterministic',
        (1, 2, 1, 93),
        None),
    'partial / csr / sweep / det': (
        'sweep tiles=2 x 32 rows, panels=1 x 2^18 cols, grid=2 (2 wg/cu, '
        'reserve 0), buckets panel-major, waves=0, deterministic',
        (1, 2, 1, 93),
        '3dfc90f90278101f3a16b2b37f92f5549fd953f43a74259cf293132be7a9f4e3'),
    'ragged / csr / steps': (
        'steps tiles=4 x 32 rows, panels=5 x 2^12 cols, <=5 buckets per tile '
        '(span 5, ascending order), tile order 0, waves=0',
        (5, 4, 5, 1584),
        None),
    'ragged / csr / steps / det': (
        'steps tiles=4 x 32 rows, panels=5 x 2^12 cols, <=5 buckets per tile '
        '(span 5, ascending order), tile order 0, waves=0, deterministic',
        (5, 4, 5, 1584),
        'b2e9686f48f37b8b8fbaaeb61ecfb48e199a6cea14e477b1096228cd1d814f0f'),
    'ragged / hll_row / steps': (
        'steps tiles=4 x 32 rows, panels=5 x 2^12 cols, <=5 buckets per tile '
        '(span 5, ascending order), tile order 0, waves=0',
        (5, 4, 5, 1584),
        None),
    'ragged / hll_row / steps / det': (
        'steps tiles=4 x 32 rows, panels=5 x 2^12 cols, <=5 buckets per tile '
        '(span 5, ascending order), tile order 0, waves=0, deterministic',
        (5, 4, 5, 1584),
        'b2e9686f48f37b8b8fbaaeb61ecfb48e199a6cea14e477b1096228cd1d814f0f'),
    'ragged / hll_col / steps': (
        'steps tiles=4 x 32 rows, panels=5 x 2^12 cols, <=5 buckets per tile '
        '(span 5, ascending order), tile order 0, waves=0',
        (5, 4, 5, 1584),
        None),
    'ragged / hll_col / steps / det': (
        'steps tiles=4 x 32 rows, panels=5 x 2^12 cols, <=5 buckets per tile '
        '(span 5, ascending order), tile order 0, waves=0, deterministic',
        (5, 4, 5, 1584),
        'b2e9686f48f37b8b8fbaaeb61ecfb48e199a6cea14e477b1096228cd1d814f0f'),
    'ragged / csr / sweep': (
        'sweep tiles=4 x 32 rows, panels=5 x 2^12 cols, grid=4 (2 wg/cu, '
        'reserve 0), buckets panel-major, waves=0, deterministic',
        (1, 4, 5, 1584),
        None),
    'ragged / csr / sweep / det': (
        'sweep tiles=4 x 32 rows, panels=5 x 2^12 cols, grid=4 (2 wg/cu, '
        'reserve 0), buckets panel-major, waves=0, deterministic',
        (1, 4, 5, 1584),
        'b2e9686f48f37b8b8fbaaeb61ecfb48e199a6cea14e477b1096228cd1d814f0f'),
    'ragged / hll_row / sweep': (
        'sweep tiles=4 x 32 rows, panels=5 x 2^12 cols, grid=4 (2 wg/cu, '
        'reserve 0), buckets panel-major, waves=0, deterministic',
        (1, 4, 5, 1584),
        None),
    'ragged / hll_row / sweep / det': (
        'sweep tiles=4 x 32 rows, panels=5 x 2^12 cols, grid=4 (2 wg/cu, '
        'reserve 0), buckets panel-major, waves=0, deterministic',
        (1, 4, 5, 1584),
        'b2e9686f48f37b8b8fbaaeb61ecfb48e199a6cea14e477b1096228cd1d814f0f'),
    'ragged / hll_col / sweep': (
        'sweep tiles=4 x 32 rows, panels=5 x 2^12 cols, grid=4 (2 wg/cu, '
        'reserve 0), buckets panel-major, waves=0, deterministic',
        (1, 4, 5, 1584),
        None),
    'ragged / hll_col / sweep / det': (
        'sweep tiles=4 x 32 rows, panels=5 x 2^12 cols, grid=4 (2 wg/cu, '
        'reserve 0), buckets panel-major, waves=0, deterministic',
        (1, 4, 5, 1584),
        'b2e9686f48f37b8b8fbaaeb61ecfb48e199a6cea14e477b1096228cd1d814f0f'),
    'const32 / csr / steps': (
        'steps tiles=4 x 32 rows, panels=5 x 2^12 cols, <=5 buckets per tile '
        '(span 5, ascending order), tile order 0, waves=0',
        (5, 4, 5, 3200),
        None),
    'const32 / csr / steps / det': (
        'steps tiles=4 x 32 rows, panels=5 x 2^12 cols, <=5 buckets per tile '
        '(span 5, ascending order), tile order 0, waves=0, deterministic',
        (5, 4, 5, 3200),
        'd4d5840fbb422c9cc94ee02e2e25a847bb6cd992f572cdb04e7f6a163d87163d'),
    'const32 / hll_row / steps': (
        'steps tiles=4 x 32 rows, panels=5 x 2^12 cols, <=5 buckets per tile '
        '(span 5, ascending order), tile order 0, waves=0',
        (5, 4, 5, 3200),
        None),
    'const32 / hll_row / steps / det': (
        'steps tiles=4 x 32 rows, panels=5 x 2^12 cols, <=5 buckets per tile '
        '(span 5, ascending order), tile order 0, waves=0, deterministic',
        (5, 4, 5, 3200),
        'd4d5840fbb422c9cc94ee02e2e25a847bb6cd992f572cdb04e7f6a163d87163d'),
    'const32 / hll_col / steps': (
        'steps tiles=4 x 32 rows, panels=5 x 2^12 cols, <=5 buckets per tile '
        '(span 5, ascending order), tile order 0, waves=0',
        (5, 4, 5, 3200),
        None),
    'const32 / hll_col / steps / det': (
        'steps tiles=4 x 32 rows, panels=5 x 2^12 cols, <=5 buckets per tile '
        '(span 5, ascending order), tile order 0, waves=0, deterministic',
        (5, 4, 5, 3200),
        'd4d5840fbb422c9cc94ee02e2e25a847bb6cd992f572cdb04e7f6a163d87163d'),
    'const32 / csr / sweep': (
        'sweep tiles=4 x 32 rows, panels=5 x 2^12 cols, grid=4 (2 wg/cu, '
        'reserve 0), buckets panel-major, waves=0, deterministic',
        (1, 4, 5, 3200),
        None),
    'const32 / csr / sweep / det': (
        'sweep tiles=4 x 32 rows, panels=5 x 2^12 cols, grid=4 (2 wg/cu, '
        'reserve 0), buckets panel-major, waves=0, deterministic',
        (1, 4, 5, 3200),
        'd4d5840fbb422c9cc94ee02e2e25a847bb6cd992f572cdb04e7f6a163d87163d'),
    'const32 / hll_row / sweep': (
        'sweep tiles=4 x 32 rows, panels=5 x 2^12 cols, grid=4 (2 wg/cu, '
        'reserve 0), buckets panel-major, waves=0, deterministic',
        (1, 4, 5, 3200),
        None),
    'const32 / hll_row / sweep / det': (
        'sweep tiles=4 x 32 rows, panels=5 x 2^12 cols, grid=4 (2 wg/cu, '
        'reserve 0), buckets panel-major, waves=0, deterministic',
        (1, 4, 5, 3200),
        'd4d5840fbb422c9cc94ee02e2e25a847bb6cd992f572cdb04e7f6a163d87163d'),
    'const32 / hll_col / sweep': (
        'sweep tiles=4 x 32 rows, panels=5 x 2^12 cols, grid=4 (2 wg/cu, '
        'reserve 0), buckets panel-major, waves=0, deterministic',
        (1, 4, 5, 3200),
        None),
    'const32 / hll_col / sweep / det': (
        'sweep tiles=4 x 32 rows, panels=5 x 2^12 cols, grid=4 (2 wg/cu, '
        'reserve 0), buckets panel-major, waves=0, deterministic',
        (1, 4, 5, 3200),
        'd4d5840fbb422c9cc94ee02e2e25a847bb6cd992f572cdb04e7f6a163d87163d'),
    'band / csr / chain32': (
        'chain tiles=4 x 32 rows, panels=5 x 2^12 cols, <=3 buckets per tile '
        '(span 3, residue order), tile order 0, waves=0',
        (1, 4, 5, 2384),
        None),
    'band / csr / chain32 / det': (
        'chain tiles=4 x 32 rows, panels=5 x 2^12 cols, <=3 buckets per tile '
        '(span 3, residue order), tile order 0, waves=0, deterministic',
        (1, 4, 5, 2384),
        '4f90dd11ce5f7a7639f303c8cce413d88997457c829fee63040ae154e6dc330e'),
    'band / csr / chain32 ascending': (
        'chain tiles=4 x 32 rows, panels=5 x 2^12 cols, <=3 buckets per tile '
        '(span 3, ascending order), tile order 0, waves=0',
        (1, 4, 5, 2384),
        None),
    'band / csr / chain32 ascending / det': (
        'chain tiles=4 x 32 rows, panels=5 x 2^12 cols, <=3 buckets per tile '
        '(span 3, ascending order), tile order 0, waves=0, deterministic',
        (1, 4, 5, 2384),
        '4f90dd11ce5f7a7639f303c8cce413d88997457c829fee63040ae154e6dc330e'),
    'ragged / csr / chain32': (
        'chain tiles=4 x 32 rows, panels=5 x 2^12 cols, <=5 buckets per tile '
        '(span 5, ascending order), tile order 0, waves=0',
        (1, 4, 5, 1584),
        None),
    'ragged / csr / chain32 / det': (
        'chain tiles=4 x 32 rows, panels=5 x 2^12 cols, <=5 buckets per tile '
        '(span 5, ascending order), tile order 0, waves=0, deterministic',
        (1, 4, 5, 1584),
        'b2e9686f48f37b8b8fbaaeb61ecfb48e199a6cea14e477b1096228cd1d814f0f'),
    'long / csr / steps': (
        'steps tiles=1 x 4096 rows, panels=1 x 2^18 cols, <=1 buckets per '
        'tile (span 1, ascending order), tile order 0, waves=0; 1 long row(s)'
        ' beside the copy (16400 entries, 17 segments)',
        (1, 1, 1, 16793),
        None),
    'long / csr / steps / det': (
        'steps tiles=1 x 4096 rows, panels=1 x 2^18 cols, <=1 buckets per '
        'tile (span 1, ascending order), tile order 0, waves=0, '
        'deterministic; 1 long row(s) beside the copy (16400 entries, 17 '
        'segments)',
        (1, 1, 1, 16793),
        'e72a1bc05cc6c6643402087e83edc63a63554fb52345bcdcd0503ad9f1150d63'),
    'long / hll_col / steps': (
        'steps tiles=1 x 4096 rows, panels=1 x 2^18 cols, <=1 buckets per '
        'tile (span 1, ascending order), tile order 0, waves=0; 1 long row(s)'
        ' beside the copy (16400 entries, 17 segments)',
        (1, 1, 1, 16793),
        None),
    'long / hll_col / steps / det': (
        'steps tiles=1 x 4096 rows, panels=1 x 2^18 cols, <=1 buckets per '
        'tile (span 1, ascending order), tile order 0, waves=0, '
        'deterministic; 1 long row(s) beside the copy (16400 entries, 17 '
        'segments)',
        (1, 1, 1, 16793),
        'e72a1bc05cc6c6643402087e83edc63a63554fb52345bcdcd0503ad9f1150d63'),
    'long / csr / sweep': (
        'sweep tiles=4 x 32 rows, panels=1 x 2^18 cols, grid=4 (1 wg/cu, '
        'reserve 0), buckets panel-major, waves=0, deterministic; 1 long '
        'row(s) beside the copy (16400 entries, 17 segments)',
        (1, 4, 1, 16793),
        None),
    'long / csr / sweep / det': (
        'sweep tiles=4 x 32 rows, panels=1 x 2^18 cols, grid=4 (1 wg/cu, '
        'reserve 0), buckets panel-major, waves=0, deterministic; 1 long '
        'row(s) beside the copy (16400 entries, 17 segments)',
        (1, 4, 1, 16793),
        'e72a1bc05cc6c6643402087e83edc63a63554fb52345bcdcd0503ad9f1150d63'),
    'long / hll_col / sweep': (
        'sweep tiles=4 x 32 rows, panels=1 x 2^18 cols, grid=4 (1 wg/cu, '
        'reserve 0), buckets panel-major, waves=0, deterministic; 1 long '
        'row(s) beside the copy (16400 entries, 17 segments)',
        (1, 4, 1, 16793),
        None),
    'long / hll_col / sweep / det': (
        'sweep tiles=4 x 32 rows, panels=1 x 2^18 cols, grid=4 (1 wg/cu, '
        'reserve 0), buckets panel-major, waves=0, deterministic; 1 long '
        'row(s) beside the copy (16400 entries, 17 segments)',
        (1, 4, 1, 16793),
        'e72a1bc05cc6c6643402087e83edc63a63554fb52345bcdcd0503ad9f1150d63'),
    'rounds / csr / sweep reserve 248': (
        'sweep tiles=16 x 12512 rows, panels=1 x 2^18 cols, grid=8 (1 wg/cu, '
        'reserve 248), buckets panel-major, waves=0, deterministic',
        (1, 16, 1, 400000),
        None),
    'rounds / csr / sweep reserve 248 / det': (
        'sweep tiles=16 x 12512 rows, panels=1 x 2^18 cols, grid=8 (1 wg/cu, '
        'reserve 248), buckets panel-major, waves=0, deterministic',
        (1, 16, 1, 400000),
        '8bcd4356a865107d822a610acdfe1af76516ad6f1d2588fcb918d6fa6099eab3'),
    'rounds / csr / sweep reserve 248 tile-major': (
        'sweep tiles=16 x 12512 rows, panels=1 x 2^18 cols, grid=8 (1 wg/cu, '
        'reserve 248), buckets tile-major, waves=0, deterministic',
        (1, 16, 1, 400000),
        None),
    'rounds / csr / sweep reserve 248 tile-major / det': (
        'sweep tiles=16 x 12512 rows, panels=1 x 2^18 cols, grid=8 (1 wg/cu, '
        'reserve 248), buckets tile-major, waves=0, deterministic',
        (1, 16, 1, 400000),
        '8bcd4356a865107d822a610acdfe1af76516ad6f1d2588fcb918d6fa6099eab3'),
    'rounds / csr / sweep reserve 248 2 wg/cu': (
        'sweep tiles=32 x 6272 rows, panels=1 x 2^18 cols, grid=16 (2 wg/cu, '
        'reserve 248), buckets panel-major, waves=0, deterministic',
        (1, 32, 1, 400000),
        None),
    'rounds / csr / sweep reserve 248 2 wg/cu / det': (
        'sweep tiles=32 x 6272 rows, panels=1 x 2^18 cols, grid=16 (2 wg/cu, '
        'reserve 248), buckets panel-major, waves=0, deterministic',
        (1, 32, 1, 400000),
        '8bcd4356a865107d822a610acdfe1af76516ad6f1d2588fcb918d6fa6099eab3'),
    'ragged_round / csr / sweep reserve 248 8 wg/cu': (
        'sweep tiles=126 x 1568 rows, panels=1 x 2^18 cols, grid=64 (8 wg/cu,'
        ' reserve 248), buckets panel-major, waves=0, deterministic',
        (1, 126, 1, 393472),
        None),
    'ragged_round / csr / sweep reserve 248 8 wg/cu / det': (
        'sweep tiles=126 x 1568 rows, panels=1 x 2^18 cols, grid=64 (8 wg/cu,'
        ' reserve 248), buckets panel-major, waves=0, deterministic',
        (1, 126, 1, 393472),
        '1e1f9ec74517d9dd6372fef678fccab573eb2a40051fc1a777ad89b887541d38'),
    'ragged_round / csr / sweep reserve 248 8 wg/cu tile-major': (
        'sweep tiles=126 x 1568 rows, panels=1 x 2^18 cols, grid=64 (8 wg/cu,'
        ' reserve 248), buckets tile-major, waves=0, deterministic',
        (1, 126, 1, 393472),
        None),
    'ragged_round / csr / sweep reserve 248 8 wg/cu tile-major / det': (
        'sweep tiles=126 x 1568 rows, panels=1 x 2^18 cols, grid=64 (8 wg/cu,'
        ' reserve 248), buckets tile-major, waves=0, deterministic',
        (1, 126, 1, 393472),
        '1e1f9ec74517d9dd6372fef678fccab573eb2a40051fc1a777ad89b887541d38'),
    'nz0 / csr / steps': (
        'steps tiles=1 x 4096 rows, panels=1 x 2^18 cols, <=0 buckets per '
        'tile (span 0, ascending order), tile order 0, waves=0',
        (0, 1, 1, 0),
        None),
    'nz0 / csr / steps / det': (
        'steps tiles=1 x 4096 rows, panels=1 x 2^18 cols, <=0 buckets per '
        'tile (span 0, ascending order), tile order 0, waves=0, deterministic',
        (0, 1, 1, 0),
        '076a27c79e5ace2a3d47f9dd2e83e4ff6ea8872b3c2218f66c92b89b55f36560'),
    'nz0 / hll_col / steps': (
        'steps tiles=1 x 4096 rows, panels=1 x 2^18 cols, <=0 buckets per '
        'tile (span 0, ascending order), tile order 0, waves=0',
        (0, 1, 1, 0),
        None),
    'nz0 / hll_col / steps / det': (
        'steps tiles=1 x 4096 rows, panels=1 x 2^18 cols, <=0 buckets per '
        'tile (span 0, ascending order), tile order 0, waves=0, deterministic',
        (0, 1, 1, 0),
        '076a27c79e5ace2a3d47f9dd2e83e4ff6ea8872b3c2218f66c92b89b55f36560'),
    'nz0 / csr / chain': (
        'chain tiles=1 x 4096 rows, panels=1 x 2^18 cols, <=0 buckets per '
        'tile (span 0, ascending order), tile order 0, waves=0',
        (1, 1, 1, 0),
        None),
    'nz0 / csr / chain / det': (
        'chain tiles=1 x 4096 rows, panels=1 x 2^18 cols, <=0 buckets per '
        'tile (span 0, ascending order), tile order 0, waves=0, deterministic',
        (1, 1, 1, 0),
        '076a27c79e5ace2a3d47f9dd2e83e4ff6ea8872b3c2218f66c92b89b55f36560'),
    'nz0 / hll_col / chain': (
        'chain tiles=1 x 4096 rows, panels=1 x 2^18 cols, <=0 buckets per '
        'tile (span 0, ascending order), tile order 0, waves=0',
        (1, 1, 1, 0),
        None),
    'nz0 / hll_col / chain / det': (
        'chain tiles=1 x 4096 rows, panels=1 x 2^18 cols, <=0 buckets per '
        'tile (span 0, ascending order), tile order 0, waves=0, deterministic',
        (1, 1, 1, 0),
        '076a27c79e5ace2a3d47f9dd2e83e4ff6ea8872b3c2218f66c92b89b55f36560'),
    'nz0 / csr / sweep': (
        'sweep tiles=2 x 32 rows, panels=1 x 2^18 cols, grid=2 (2 wg/cu, '
        'reserve 0), buckets panel-major, waves=0, deterministic',
        (1, 2, 1, 0),
        None),
    'nz0 / csr / sweep / det': (
        'sweep tiles=2 x 32 rows, panels=1 x 2^18 cols, grid=2 (2 wg/cu, '
        'reserve 0), buckets panel-major, waves=0, deterministic',
        (1, 2, 1, 0),
        '076a27c79e5ace2a3d47f9dd2e83e4ff6ea8872b3c2218f66c92b89b55f36560'),
    'nz0 / hll_col / sweep': (
        'sweep tiles=2 x 32 rows, panels=1 x 2^18 cols, grid=2 (2 wg/cu, '
        'reserve 0), buckets panel-major, waves=0, deterministic',
        (1, 2, 1, 0),
        None),
    'nz0 / hll_col / sweep / det': (
        'sweep tiles=2 x 32 rows, panels=1 x 2^18 cols, grid=2 (2 wg/cu, '
        'reserve 0), buckets panel-major, waves=0, deterministic',
        (1, 2, 1, 0),
        '076a27c79e5ace2a3d47f9dd2e83e4ff6ea8872b3c2218f66c92b89b55f36560'),
    'm0 / csr / steps': (
        'steps tiles=0 x 4096 rows, panels=1 x 2^18 cols, <=0 buckets per '
        'tile (span 0, ascending order), tile order 0, waves=0',
        (0, 0, 1, 0),
        None),
    'm0 / csr / steps / det': (
        'steps tiles=0 x 4096 rows, panels=1 x 2^18 cols, <=0 buckets per '
        'tile (span 0, ascending order), tile order 0, waves=0, deterministic',
        (0, 0, 1, 0),
        'e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855'),
    'm0 / csr / chain': (
        'chain tiles=0 x 4096 rows, panels=1 x 2^18 cols, <=0 buckets per '
        'tile (span 0, ascending order), tile order 0, waves=0',
        (1, 0, 1, 0),
        None),
    'm0 / csr / chain / det': (
        'chain tiles=0 x 4096 rows, panels=1 x 2^18 cols, <=0 buckets per '
        'tile (span 0, ascending order), tile order 0, waves=0, deterministic',
        (1, 0, 1, 0),
        'e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855'),
    'm0 / csr / sweep': (
        'sweep tiles=0 x 32 rows, panels=1 x 2^18 cols, grid=1 (2 wg/cu, '
        'reserve 0), buckets panel-major, waves=0, deterministic',
        (1, 0, 1, 0),
        None),
    'm0 / csr / sweep / det': (
        'sweep tiles=0 x 32 rows, panels=1 x 2^18 cols, grid=1 (2 wg/cu, '
        'reserve 0), buckets panel-major, waves=0, deterministic',
        (1, 0, 1, 0),
        'e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855'),
}


def test_build_geometry_matches_the_recorded_table():
    """the build side of the blocked path -- geometry (panel_build.h), keep
    list, keys, sort, bucket tables, compacted lists, placement, long rows --
    on the smallest shapes that reach each of its paths: description, sizes
    and, for deterministic copies, the bits of y are those recorded before
    the build was restructured"""
    rows = _geometry_rows()
    got = {key: (text, info, sha) for key, text, info, sha in rows}
    assert len(got) == len(rows) and set(got) == set(_GEOMETRY_RECORDED)
    for key, text, info, sha in rows:
        print(key, "|", text, info, sha)
    for key, want in _GEOMETRY_RECORDED.items():
        assert got[key] == want, key
    # a CSR handle and both HLL layouts of one matrix give one copy
    for name in ("ragged", "const32"):
        for tag in ("steps", "steps / det", "sweep", "sweep / det"):
            three = {got["%s / %s / %s" % (name, src, tag)]
                     for src in ("csr", "hll_row", "hll_col")}
            assert len(three) == 1, (name, tag, three)
