"""GPU parity: every HIP kernel, called through the C-ABI, against the CPU
oracle (oracle/liboracle.so) and the reference-built golden vectors.

Tolerance (BASELINE.json north_star): 1e-6 relative fp64 against the serial
CSR path.  Written out below as REL_TOL; the kernels are additionally held to
TIGHT = 1e-12 of the row scale sum_j |a_ij x_j| (summation order differs from
the serial loop, nothing else may).
"""
import ctypes as C

import numpy as np
import pytest

import _golden as G
import _oracle as O
import spmv_scpa_amd as S

pytestmark = pytest.mark.gpu

REL_TOL = 1e-6
TIGHT = 1e-12
WPB = (2, 4, 8)  # the reference's sweep (main.c:265-269)


def assert_parity(y, y_ref, scale, what):
    assert y.shape == y_ref.shape, what
    assert np.all(np.isfinite(y)), what
    den = np.maximum(np.abs(y_ref), 1e-3 * scale)
    den = np.maximum(den, 1e-300)
    rel = np.max(np.abs(y - y_ref) / den) if len(y) else 0.0
    assert rel <= REL_TOL, (what, rel)
    nrm = np.linalg.norm(y_ref)
    if nrm > 0:
        assert np.linalg.norm(y - y_ref) / nrm <= REL_TOL, what
    tight = np.max(np.abs(y - y_ref) / np.maximum(scale, 1e-300)) if len(y) else 0
    assert tight <= TIGHT, (what, tight)
    assert S.validation_vec_result(y_ref, y) == 0, what  # reference's -d check


def run_all_kernels(A, x, y_ref, scale, tag):
    for k in range(S.NUM_CSR_KERNELS):
        for w in WPB:
            y, ms = S.csr_spmv_hip(A, x, kernel=k, waves_per_block=w)
            assert ms >= 0
            assert_parity(y, y_ref, scale, (tag, "csr", k, w))
    for g in (2, 4, 8, 16, 32):
        y, _ = S.csr_spmv_hip(A, x, kernel=2, waves_per_block=4, group=g)
        assert_parity(y, y_ref, scale, (tag, "csr subwave G", g))
    # sub-wave kernel with the IRP loads kept (bit 9) -- matrices whose rows
    # all have one length otherwise take the path that computes IRP[r]
    for v in (512, 512 | 1, 512 | 2, 512 | 32):
        y, _ = S.csr_spmv_hip(A, x, kernel=2, waves_per_block=4, variant=v)
        assert_parity(y, y_ref, scale, (tag, "csr subwave variant", v))
    # stream kernel: 4- / 8-byte loads only (bit 4), grouped range order
    # (bit 5), hardware order (bit 6)
    for v in (16, 32, 64, 16 | 32):
        y, _ = S.csr_spmv_hip(A, x, kernel=4, variant=v)
        assert_parity(y, y_ref, scale, (tag, "csr stream variant", v))
    for k in range(S.NUM_HLL_KERNELS):
        H = S.csr_to_hll(A, S.HLL_KERNEL_COL_MAJOR[k])
        for w in WPB:
            y, ms = S.hll_spmv_hip(H, x, kernel=k, waves_per_block=w)
            assert ms >= 0
            assert_parity(y, y_ref, scale, (tag, "hll", k, w))
        S.hll_free(H)


@pytest.mark.parametrize("name", G.MTX_CASES)
def test_golden_mtx_all_kernels(name):
    """Same .mtx, same glibc x as the reference run; expected y is the
    reference's serial CSR output stored in tests/golden."""
    ref = G.load_ref(name)
    A = S.io_load_csr(G.mtx_path(name))
    x = S.vec_random(A.contents.N)
    y_ref = ref["y_csr_serial"]
    IRP, JA, AS = S.csr_arrays(A)
    scale = O.csr_abs_spmv(IRP, JA, AS, x)
    assert np.array_equal(O.csr_spmv(IRP, JA, AS, x), y_ref)
    run_all_kernels(A, x, y_ref, scale, name)
    S.csr_free(A)


SYNTH_SMALL = [
    ("banded", S.SYNTH_BANDED, 50_000, 16, 0),
    ("random_narrow", S.SYNTH_RANDOM, 40_000, 32, 512),
    ("random_wide", S.SYNTH_RANDOM, 33_333, 32, 1 << 30),
    ("ragged", S.SYNTH_RAGGED, 20_011, 32, 4096),
    ("kkt", S.SYNTH_KKT, 30_000, 16, 30_000),
    ("stencil27", S.SYNTH_STENCIL, 40_000, 27, 0),
    ("stencil7", S.SYNTH_STENCIL, 33_000, 7, 30),
    ("one_row", S.SYNTH_RANDOM, 1, 32, 64),
    ("31_rows", S.SYNTH_RANDOM, 31, 5, 64),
    ("33_rows", S.SYNTH_RAGGED, 33, 8, 64),
    ("long_rows", S.SYNTH_RANDOM, 300, 5000, 1 << 30),
    # the reference's irregular classes (scripts/download-matrices.py:7-38):
    # webbase / amazon / roadNet (mean 3, power-law tail) and dc1 (one row and
    # one column far heavier than the rest)
    ("powerlaw3", S.SYNTH_POWERLAW, 60_000, 3, 1 << 30),
    ("powerlaw3_windowed", S.SYNTH_POWERLAW, 40_000, 3, 2048),
    ("powerlaw8", S.SYNTH_POWERLAW, 30_011, 8, 1 << 30),
    ("hub", S.SYNTH_HUB, 40_000, 6, 512),
    ("hub_short", S.SYNTH_HUB, 20_000, 2, 1 << 30),
]


@pytest.mark.parametrize("tag,kind,M,K,W", SYNTH_SMALL)
def test_synthetic_all_kernels(tag, kind, M, K, W):
    N = max(M, K, 64)
    IRP, JA, AS = O.synth_csr(kind, M, N, K, W, 42)
    x = O.synth_x(7, 0, N)
    y_ref = O.csr_spmv(IRP, JA, AS, x)
    scale = O.csr_abs_spmv(IRP, JA, AS, x)
    A = S.csr_from_arrays(tag, M, N, IRP, JA, AS)
    run_all_kernels(A, x, y_ref, scale, tag)
    S.csr_free(A)


def test_empty_and_degenerate_matrices():
    # all rows empty; and a matrix with zero rows
    IRP = np.zeros(71, dtype=np.int32)
    A = S.csr_from_arrays("empty", 70, 9, IRP, np.zeros(0, np.int32),
                          np.zeros(0))
    x = np.ones(9)
    for k in range(S.NUM_CSR_KERNELS):
        y, _ = S.csr_spmv_hip(A, x, kernel=k)
        assert np.array_equal(y, np.zeros(70))
    for k in range(S.NUM_HLL_KERNELS):
        H = S.csr_to_hll(A, S.HLL_KERNEL_COL_MAJOR[k])
        y, _ = S.hll_spmv_hip(H, x, kernel=k)
        assert np.array_equal(y, np.zeros(70))
        S.hll_free(H)
    S.csr_free(A)
    A0 = S.csr_from_arrays("norows", 0, 4, np.zeros(1, np.int32),
                           np.zeros(0, np.int32), np.zeros(0))
    y, _ = S.csr_spmv_hip(A0, np.ones(4), kernel=2)
    assert len(y) == 0
    S.csr_free(A0)


def test_bench_wrappers_and_reference_abi_names():
    """The bench_* layer (reference csr.c:382-415 / hll.c:226-256 shape) and
    the reference's own 11 plugin symbols run the HIP kernels."""
    import ctypes as C
    name = "ragged100"
    ref = G.load_ref(name)
    A = S.io_load_csr(G.mtx_path(name))
    x = S.vec_random(A.contents.N)
    IRP, JA, AS = S.csr_arrays(A)
    scale = O.csr_abs_spmv(IRP, JA, AS, x)
    y_ref = ref["y_csr_serial"]
    for k in range(S.NUM_CSR_KERNELS):
        y, ms, gf = S.bench_csr_hip(A, x, k, 4)
        assert_parity(y, y_ref, scale, ("bench csr", k))
        assert gf == S.compute_gflops(ms, A.contents.NZ)
    Hs = {False: S.csr_to_hll(A, False), True: S.csr_to_hll(A, True)}
    for k in range(S.NUM_HLL_KERNELS):
        y, ms, gf = S.bench_hll_hip(Hs[S.HLL_KERNEL_COL_MAJOR[k]], x, k, 8)
        assert_parity(y, y_ref, scale, ("bench hll", k))
    dp = C.POINTER(C.c_double)
    xs = np.ascontiguousarray(x)
    lib = S._lib
    lib.set_csr_warps_per_block(4)
    lib.set_hll_warps_per_block(2)
    for sym in ("csr_spmv_cuda_thread_row", "csr_spmv_cuda_warp_row",
                "csr_spmv_cuda_halfwarp_row", "csr_spmv_cuda_block_row",
                "csr_spmv_cuda_halfwarp_row_text"):
        fn = getattr(lib, sym)
        fn.restype = C.c_double
        y = np.zeros(A.contents.M)
        ms = fn(A, xs.ctypes.data_as(dp), y.ctypes.data_as(dp), None)
        assert ms >= 0
        assert_parity(y, y_ref, scale, sym)
    for sym, cm in (("hll_spmv_cuda_threads_row_major", False),
                    ("hll_spmv_cuda_threads_col_major", True),
                    ("hll_spmv_cuda_warp_block", True),
                    ("hll_spmv_cuda_halfwarp_row", False)):
        fn = getattr(lib, sym)
        fn.restype = C.c_double
        y = np.zeros(A.contents.M)
        ms = fn(Hs[cm], xs.ctypes.data_as(dp), y.ctypes.data_as(dp), None)
        assert ms >= 0
        assert_parity(y, y_ref, scale, sym)
    for H in Hs.values():
        S.hll_free(H)
    S.csr_free(A)


@pytest.mark.parametrize("kind,M,N,K,W", [
    (S.SYNTH_RAGGED, 50_021, 60_000, 32, 2048),
    (S.SYNTH_POWERLAW, 150_001, 150_001, 3, 1 << 30),
    (S.SYNTH_HUB, 50_021, 60_000, 6, 2048),
    # rows of 225..375 entries: a 128-row range exceeds the LDS budget of the
    # generator and of the CSR->HLL fill -- their direct-access fallbacks
    (S.SYNTH_RAGGED, 30_011, 60_000, 300, 8192),
    # every 64th row 8x longer than the others
    (S.SYNTH_KKT, 50_021, 60_000, 16, 2048),
    # nine rows of 4097..12288 entries, each inside a 128-row range that fits
    # the generator's LDS stage: rows handed to the parallel-row kernel in a
    # workgroup that would otherwise be staged (such a workgroup
    # is not staged any more; before, it wrote the row's uninitialised LDS
    # range out and relied on the later kernel to overwrite it)
    (S.SYNTH_POWERLAW, 400_000, 400_000, 8, 1 << 30),
], ids=["ragged", "powerlaw", "hub", "wide_rows", "kkt", "powerlaw_mid_rows"])
def test_persistent_handles_and_device_generation(kind, M, N, K, W):
    """upload once / launch many; device-side generation and device-side
    CSR->HLL agree bit-for-bit with the host path."""
    IRP, JA, AS = O.synth_csr(kind, M, N, K, W, 42)
    if M == 400_000:
        L = np.diff(IRP)
        mid = np.nonzero((L > 4096) & (L <= 12288))[0]
        assert len(mid) >= 5 and any(
            IRP[min(r // 128 * 128 + 128, M)] - IRP[r // 128 * 128] <= 12288
            for r in mid), "the case no longer holds the rows it is about"
    x = O.synth_x(7, 0, N)
    y_ref = O.csr_spmv(IRP, JA, AS, x)
    scale = O.csr_abs_spmv(IRP, JA, AS, x)
    dA = S.CsrDevice.generate(kind, M, N, K, W, 0, 42)
    assert (dA.M, dA.N, dA.NZ) == (M, N, len(JA))
    back = dA.download()
    bI, bJ, bA = S.csr_arrays(back)
    assert np.array_equal(bI, IRP) and np.array_equal(bJ, JA)
    assert np.array_equal(bA.view(np.uint64), AS.view(np.uint64))
    S.csr_free(back)
    d_x = S.DevBuffer(N * 8)
    S.dev_fill_synth(d_x.ptr, N, 7)
    S.stream_sync()
    assert np.array_equal(d_x.to_numpy(np.float64, N).view(np.uint64),
                          x.view(np.uint64))
    d_y = S.DevBuffer(M * 8)
    assert dA.algorithmic_bytes == 12 * len(JA) + 4 * (M + 1) + 8 * M + 8 * N
    for k in range(S.NUM_CSR_KERNELS):
        S._lib.spmv_dev_memset(d_y.ptr, 0xFF, M * 8, None)
        for _ in range(3):
            dA.launch(k, d_x.ptr, d_y.ptr, waves_per_block=4)
        S.stream_sync()
        assert_parity(d_y.to_numpy(np.float64, M), y_ref, scale, ("dev csr", k))
    # row sub-ranges (the chunked multi-GPU overlap path)
    S._lib.spmv_dev_memset(d_y.ptr, 0, M * 8, None)
    cut = 20_000
    dA.launch(2, d_x.ptr, d_y.ptr, rows=(0, cut))
    dA.launch(4, d_x.ptr, d_y.ptr, rows=(cut, M))
    S.stream_sync()
    assert_parity(d_y.to_numpy(np.float64, M), y_ref, scale, "csr row ranges")
    for cm in (False, True):
        dH = dA.to_hll(cm)
        off, maxnz, _, HJA, HAS = O.csr_to_hll(IRP, JA, AS, cm)
        assert dH.slots == off[-1] and dH.num_blocks == len(maxnz)
        assert dH.algorithmic_bytes == (12 * dH.slots + 12 * dH.num_blocks
                                        + 8 * M + 8 * N)
        for k in range(S.NUM_HLL_KERNELS):
            if S.HLL_KERNEL_COL_MAJOR[k] != cm:
                with pytest.raises(OSError):
                    dH.launch(k, d_x.ptr, d_y.ptr)
                continue
            S._lib.spmv_dev_memset(d_y.ptr, 0xFF, M * 8, None)
            dH.launch(k, d_x.ptr, d_y.ptr, waves_per_block=4)
            S.stream_sync()
            assert_parity(d_y.to_numpy(np.float64, M), y_ref, scale,
                          ("dev hll", cm, k))
            # hack-block sub-ranges
            S._lib.spmv_dev_memset(d_y.ptr, 0, M * 8, None)
            nb = dH.num_blocks
            for b0, b1 in ((0, 7), (7, nb // 2), (nb // 2, nb)):
                dH.launch(k, d_x.ptr, d_y.ptr, blocks=(b0, b1))
            S.stream_sync()
            assert_parity(d_y.to_numpy(np.float64, M), y_ref, scale,
                          ("dev hll blocks", cm, k))
        dH.release()
    # event-timed loop returns one positive time per iteration
    ms = dA.time(2, d_x.ptr, d_y.ptr, warmup=1, iters=5,
                 flush_bytes=64 << 20)
    assert len(ms) == 5 and np.all(ms > 0)
    dA.release()


def test_config2_banded_full_size_properties():
    """BASELINE config 2: 1M x 1M banded, 16/row.  Host-generated, so the
    whole y is compared with the oracle; plus linearity."""
    M = N = 1_000_000
    A = S.csr_generate(S.SYNTH_BANDED, M, N, 16, 0, 0, 42)
    IRP, JA, AS = S.csr_arrays(A)
    x = S.vec_synth(N, 7)
    y_ref = O.csr_spmv(IRP, JA, AS, x)
    scale = O.csr_abs_spmv(IRP, JA, AS, x)
    dA = S.CsrDevice.upload(A)
    assert dA.algorithmic_bytes == 212_000_004
    d_x, d_y = S.DevBuffer.from_numpy(x), S.DevBuffer(M * 8)
    for k in (1, 2, 4):
        dA.launch(k, d_x.ptr, d_y.ptr)
        S.stream_sync()
        assert_parity(d_y.to_numpy(np.float64, M), y_ref, scale, ("cfg2", k))
    z = S.vec_synth(N, 11)
    d_z = S.DevBuffer.from_numpy(2.0 * x - 0.5 * z)
    dA.launch(2, d_z.ptr, d_y.ptr)
    S.stream_sync()
    y_lin = d_y.to_numpy(np.float64, M)
    y_z = O.csr_spmv(IRP, JA, AS, z)
    assert np.max(np.abs(y_lin - (2.0 * y_ref - 0.5 * y_z))
                  / np.maximum(scale + O.csr_abs_spmv(IRP, JA, AS, z), 1e-300)) < 1e-12
    dA.release()
    S.csr_free(A)


@pytest.mark.parametrize("W", [1 << 20, 1 << 30])
def test_config3_random_hll_full_size_properties(W):
    """BASELINE config 3: 10M x 10M, 32/row, hack 32, generated and converted
    on the device.  Size-independent checks: 20k sampled rows regenerated by
    the oracle from the counter-based definition; x = 1 gives row sums;
    CSR and HLL kernels agree with each other."""
    M = N = 10_000_000
    K = 32
    dA = S.CsrDevice.generate(S.SYNTH_RANDOM, M, N, K, W, 0, 42)
    assert dA.NZ == M * K
    dH = dA.to_hll(True)
    assert dH.slots == M * K and dH.num_blocks == 312_500
    assert dH.algorithmic_bytes == 4_003_750_000
    d_x, d_y = S.DevBuffer(N * 8), S.DevBuffer(M * 8)
    S.dev_fill_synth(d_x.ptr, N, 7)
    rng = np.random.default_rng(5)
    rows = np.unique(np.concatenate([[0, 1, 31, 32, M - 1, M - 32],
                                     rng.integers(0, M, 20_000)]))
    want = np.array([O.synth_row_dot(S.SYNTH_RANDOM, M, N, K, W, 0, 42, 7,
                                     int(g)) for g in rows])
    ys = {}
    dH.build_panels(0)  # the 2-D blocked path, bench.py's pick for W = N
    info = dH.panels_info()
    # default schedule: one persistent launch; a workgroup owns one row tile
    # per round (10M rows: 2 rounds of 256 tiles of <= 20448 rows with
    # 2^17-column panels, or of 512 tiles of <= 10208 rows with 2^18)
    assert info["entries"] == M * K and info["steps"] == 1
    # (which tile / panel geometry the build picks is a tuning decision:
    # tests/test_gpu_tuning.py, not a parity matter)
    for tag, fn in (("hll1", lambda: dH.launch(1, d_x.ptr, d_y.ptr)),
                    ("hll2", lambda: dH.launch(2, d_x.ptr, d_y.ptr)),
                    ("hll4", lambda: dH.launch(S.HLL_KERNEL_PANELS, d_x.ptr,
                                               d_y.ptr)),
                    ("csr2", lambda: dA.launch(2, d_x.ptr, d_y.ptr))):
        S._lib.spmv_dev_memset(d_y.ptr, 0xFF, M * 8, None)
        fn()
        S.stream_sync()
        y = d_y.to_numpy(np.float64, M)
        assert np.all(np.isfinite(y))
        got = y[rows]
        assert np.max(np.abs(got - want[:, 0]) / want[:, 1]) <= TIGHT, tag
        den = np.maximum(np.abs(want[:, 0]), 1e-3 * want[:, 1])
        assert np.max(np.abs(got - want[:, 0]) / den) <= REL_TOL, tag
        ys[tag] = y
    assert np.max(np.abs(ys["hll1"] - ys["csr2"])) < 1e-11
    assert np.max(np.abs(ys["hll1"] - ys["hll4"])) < 1e-11
    assert np.array_equal(ys["hll1"], ys["hll2"])  # same order of operations
    # the chain schedule at the selector's tall, balanced tile height: on the
    # band (W = 2^20) the buckets are visited in residue order (panels.hip,
    # k_compact_buckets), with columns anywhere in ascending order; the WHOLE
    # y must agree with the thread-per-row kernel either way, and the blocked
    # kernel must be linear: A (2 x - z / 2) = 2 A x - A z / 2
    dH.build_panels(0, "chain", tile_rows=19552)
    desc = dH.panels_describe()
    assert ("residue order" in desc) == (W == 1 << 20), desc
    S._lib.spmv_dev_memset(d_y.ptr, 0xFF, M * 8, None)
    dH.launch(S.HLL_KERNEL_PANELS, d_x.ptr, d_y.ptr)
    S.stream_sync()
    y_chain = d_y.to_numpy(np.float64, M)
    assert np.max(np.abs(ys["hll1"] - y_chain)) < 1e-11
    d_z = S.DevBuffer(N * 8)
    S.dev_fill_synth(d_z.ptr, N, 11)
    dH.launch(S.HLL_KERNEL_PANELS, d_z.ptr, d_y.ptr)
    S.stream_sync()
    y_z = d_y.to_numpy(np.float64, M)
    mix = 2.0 * d_x.to_numpy(np.float64, N) - 0.5 * d_z.to_numpy(np.float64, N)
    d_m = S.DevBuffer.from_numpy(mix)
    dH.launch(S.HLL_KERNEL_PANELS, d_m.ptr, d_y.ptr)
    S.stream_sync()
    y_m = d_y.to_numpy(np.float64, M)
    # |terms| <= 1 each, 32 per row: rounding of three products of <= 32
    # terms and of the combination stays far below 1e-11
    assert np.max(np.abs(y_m - (2.0 * y_chain - 0.5 * y_z))) < 1e-11
    dH.release()
    dA.release()


def test_config5_one_shard_of_the_8_gpu_problem():
    """BASELINE config 5 on one GPU: rank 3's shard of the 80M x 80M matrix
    (10M local rows starting at global row 30M, GLOBAL column indices up to
    8e7, x of 640 MB).  The direct kernel and the autotuned pick (the blocked
    path here) against rows recomputed from the workload definition."""
    M, N, K, W = 10_000_000, 80_000_000, 32, 1 << 30
    row0 = 3 * M
    dA = S.CsrDevice.generate(S.SYNTH_RANDOM, M, N, K, W, row0, 42)
    dH = dA.to_hll(True)
    dA.release()
    assert dH.slots == M * K
    d_x, d_y = S.DevBuffer(N * 8), S.DevBuffer(M * 8)
    S.dev_fill_synth(d_x.ptr, N, 7)
    rng = np.random.default_rng(11)
    rows = np.unique(np.concatenate([[0, 31, 32, M - 1],
                                     rng.integers(0, M, 4_000)]))
    want = np.array([O.synth_row_dot(S.SYNTH_RANDOM, 8 * M, N, K, W, 0, 42, 7,
                                     row0 + int(g)) for g in rows])
    best, ms = dH.autotune(d_x.ptr, d_y.ptr)
    assert 0 <= best < len(S.HLL_KERNEL_LABELS)  # which one: test_gpu_tuning
    ys = {}
    for tag, k in (("direct", 2), ("autotuned", best)):
        S._lib.spmv_dev_memset(d_y.ptr, 0xFF, M * 8, None)
        dH.launch(k, d_x.ptr, d_y.ptr)
        S.stream_sync()
        y = d_y.to_numpy(np.float64, M)
        assert np.all(np.isfinite(y)), tag
        assert np.max(np.abs(y[rows] - want[:, 0]) / want[:, 1]) <= TIGHT, tag
        ys[tag] = y
    assert np.max(np.abs(ys["direct"] - ys["autotuned"])) < 1e-11
    dH.release()


PANEL_CASES = [
    # tag, kind, M, N, K, W, panel_cols
    ("wide_small_panels", S.SYNTH_RANDOM, 20_000, 20_000, 32, 1 << 30, 512),
    ("wide_default", S.SYNTH_RANDOM, 300_000, 300_000, 32, 1 << 30, 0),
    ("ragged", S.SYNTH_RAGGED, 5_003, 7_000, 24, 3000, 64),
    ("kkt_long_rows", S.SYNTH_KKT, 9_000, 9_000, 16, 9000, 256),
    ("very_long_rows", S.SYNTH_RANDOM, 70, 4_000, 3000, 1 << 30, 1024),
    ("one_panel", S.SYNTH_RANDOM, 1_000, 1_000, 8, 100, 0),
    ("more_tiles_than_groups", S.SYNTH_RANDOM, 40_000, 50_000, 8, 1 << 30, 4096),
    ("empty_rows_banded", S.SYNTH_STENCIL, 27_000, 27_000, 7, 30, 128),
    ("tiny", S.SYNTH_RANDOM, 3, 64, 5, 64, 16),
    # rows kept BESIDE the copy (> 16384 entries: panels.hip "LONG ROWS"): the
    # hub row (30 000 / 131 072 entries) and the power law's tail
    ("hub_long_row_beside", S.SYNTH_HUB, 30_000, 30_000, 6, 512, 0),
    ("hub_131072_row", S.SYNTH_HUB, 50_000, 200_000, 4, 1 << 30, 4096),
    ("powerlaw_k40_tail", S.SYNTH_POWERLAW, 60_000, 60_000, 40, 1 << 30, 0),
]


@pytest.fixture
def default_panel_schedule():
    yield
    S.set_panel_schedule("sweep")


@pytest.mark.parametrize("sched", ["sweep", "steps", "chain"])
@pytest.mark.parametrize("tag,kind,M,N,K,W,pc", PANEL_CASES)
def test_column_panel_path(tag, kind, M, N, K, W, pc, sched,
                           default_panel_schedule):
    """Extra kernel (spmv_engine.h, panels.hip): entries bucketed by (row
    tile, column panel), y tile accumulated in LDS with ds_add_f64; all
    schedules (one persistent launch over all panels with phase counters /
    one launch per panel step / one launch chaining a tile's buckets)."""
    S.set_panel_schedule(sched)
    sweep = sched == "sweep"
    IRP, JA, AS = O.synth_csr(kind, M, N, K, W, 42)
    x = O.synth_x(7, 0, N)
    y_ref = O.csr_spmv(IRP, JA, AS, x)
    scale = O.csr_abs_spmv(IRP, JA, AS, x)
    A = S.csr_from_arrays(tag, M, N, IRP, JA, AS)
    d_x, d_y = S.DevBuffer.from_numpy(x), S.DevBuffer(max(M, 1) * 8)
    dA = S.CsrDevice.upload(A)
    with pytest.raises(OSError):  # not built yet
        dA.launch(S.CSR_KERNEL_PANELS, d_x.ptr, d_y.ptr)
    assert dA.panels_schedule() is None
    dA.build_panels(pc)
    info = dA.panels_info()
    assert info["entries"] == int(IRP[-1]) and dA.panels_schedule() == sched
    longest = int(np.max(np.diff(IRP))) if M else 0
    assert ("long row(s) beside" in dA.panels_describe()) == (longest > 16384)
    assert ((info["steps"] == 1) if sched != "steps"
            else (info["steps"] <= info["panels"]))
    # public bits: steps layout bit 0 flips between step launches and the
    # chain launch, bit 1 tiles in hardware order, bit 2 XCD ranges.  The
    # experiment bits (sweep: 16 = workgroups at most one panel apart, 128 =
    # no phase wait at all, 2048 = the other group count; 14-15: group size of
    # the grouped order) exist only in the ablations flavour (`make abl`)
    abl = S.build_flavour() == "ablations"
    cases = ([(0, 8), (0, 4)] + ([(16, 8), (128, 4), (2048, 8)] if abl else [])
             if sweep else
             [(0, 8), (0, 4), (1, 0), (1, 16), (2, 8), (4, 0), (3, 4)]
             + ([(2048, 8), (16384, 8), (32768 + 1, 4), (49152, 0)]
                if abl else []))
    if not abl:  # the product library refuses what it does not document
        for bad in (16, 128, 256, 512, 2048, 4096, 16384):
            with pytest.raises(OSError):
                dA.launch(S.CSR_KERNEL_PANELS, d_x.ptr, d_y.ptr, variant=bad)
    for variant, waves in cases:
        S._lib.spmv_dev_memset(d_y.ptr, 0xFF, M * 8, None)
        for _ in range(2):  # repeated launches must not accumulate
            dA.launch(S.CSR_KERNEL_PANELS, d_x.ptr, d_y.ptr, variant=variant,
                      waves_per_block=waves)
        S.stream_sync()
        assert_parity(d_y.to_numpy(np.float64, M), y_ref, scale,
                      (tag, "csr panels", variant, waves))
    if sweep:  # both bucket layouts of the sweep schedule (default: 1)
        for layout in (0, 1):
            dA.build_panels(pc, "sweep", sweep_layout=layout)
            for waves in (0, 4):
                S._lib.spmv_dev_memset(d_y.ptr, 0xFF, M * 8, None)
                dA.launch(S.CSR_KERNEL_PANELS, d_x.ptr, d_y.ptr,
                          waves_per_block=waves)
                S.stream_sync()
                assert_parity(d_y.to_numpy(np.float64, M), y_ref, scale,
                              (tag, "sweep layout", layout, waves))
    for cm in (True, False):
        H = S.csr_to_hll(A, cm)
        dH = S.HllDevice.upload(H, cm)
        dH.build_panels(pc)
        S._lib.spmv_dev_memset(d_y.ptr, 0xFF, M * 8, None)
        dH.launch(S.HLL_KERNEL_PANELS, d_x.ptr, d_y.ptr)
        S.stream_sync()
        assert_parity(d_y.to_numpy(np.float64, M), y_ref, scale,
                      (tag, "hll panels", cm))
        dH.release()
        S.hll_free(H)
    dA.release()
    S.csr_free(A)


@pytest.mark.parametrize("tile_rows", [32, 2048, 16384, 20448])
def test_steps_schedule_tile_heights(tile_rows, default_panel_schedule,
                                     monkeypatch):
    """The steps schedule at the tile heights the autotuner tries (16 KiB and
    128 KiB of LDS) and at the smallest one; a matrix with empty rows, rows
    longer than a chunk and more than one panel per tile."""
    M, N, K, W = 50_000, 60_000, 16, 20_000
    IRP, JA, AS = O.synth_csr(S.SYNTH_KKT, M, N, K, W, 42)
    x = O.synth_x(7, 0, N)
    y_ref = O.csr_spmv(IRP, JA, AS, x)
    scale = O.csr_abs_spmv(IRP, JA, AS, x)
    A = S.csr_from_arrays("tiles", M, N, IRP, JA, AS)
    d_x, d_y = S.DevBuffer.from_numpy(x), S.DevBuffer(M * 8)
    dA = S.CsrDevice.upload(A)
    S.set_panel_schedule("steps")
    monkeypatch.setenv("SPMV_TILE_ROWS", str(tile_rows))
    dA.build_panels(8192)  # 8 panels: several steps per tile
    monkeypatch.delenv("SPMV_TILE_ROWS")
    info = dA.panels_info()
    assert info["tiles"] == -(-M // tile_rows) and info["steps"] > 1
    for variant in (0, 1):  # step launches / one chain launch
        for waves in (0, 4, 8, 16):
            S._lib.spmv_dev_memset(d_y.ptr, 0xFF, M * 8, None)
            dA.launch(S.CSR_KERNEL_PANELS, d_x.ptr, d_y.ptr,
                      waves_per_block=waves, variant=variant)
            S.stream_sync()
            assert_parity(d_y.to_numpy(np.float64, M), y_ref, scale,
                          ("steps", tile_rows, waves, variant))
    dA.release()
    S.csr_free(A)


@pytest.mark.parametrize("sched,tile_rows", [("chain", 8192), ("chain", 16384),
                                             ("steps", 4096)])
def test_deterministic_chain_and_steps_at_every_launch_shape(sched, tile_rows):
    """The ordered mode of the chain / steps kernels at explicit
    waves_per_block, not only the default: 256 and 512 threads, two groups per
    lane and -- chain tiles above 80 KiB of LDS -- four.  Each launch shape
    agrees with the oracle and gives the same bits on 20 further launches."""
    M, N, K, W = 50_000, 60_000, 16, 20_000
    IRP, JA, AS = O.synth_csr(S.SYNTH_KKT, M, N, K, W, 42)
    x = O.synth_x(7, 0, N)
    y_ref = O.csr_spmv(IRP, JA, AS, x)
    scale = O.csr_abs_spmv(IRP, JA, AS, x)
    A = S.csr_from_arrays("det tiles", M, N, IRP, JA, AS)
    d_x, d_y = S.DevBuffer.from_numpy(x), S.DevBuffer(M * 8)
    dA = S.CsrDevice.upload(A)
    dA.build_panels(8192, sched, tile_rows, deterministic=True)
    assert dA.panels_schedule() == sched and dA.panels_tile_rows() == tile_rows
    assert "deterministic" in dA.panels_describe()
    for waves in (4, 8, 16):
        S._lib.spmv_dev_memset(d_y.ptr, 0xFF, M * 8, None)
        dA.launch(S.CSR_KERNEL_PANELS, d_x.ptr, d_y.ptr, waves_per_block=waves)
        S.stream_sync()
        y0 = d_y.to_numpy(np.float64, M)
        assert_parity(y0, y_ref, scale, ("det", sched, tile_rows, waves))
        for it in range(20):
            dA.launch(S.CSR_KERNEL_PANELS, d_x.ptr, d_y.ptr,
                      waves_per_block=waves)
            S.stream_sync()
            assert np.array_equal(d_y.to_numpy(np.float64, M).view(np.uint64),
                                  y0.view(np.uint64)), (sched, waves, it)
    dA.release()
    S.csr_free(A)


@pytest.mark.parametrize("sched", ["chain", "steps"])
def test_residue_bucket_order_on_a_band(sched, default_panel_schedule,
                                        monkeypatch):
    """Banded matrix whose tiles reach over several narrow panels: the chain
    / steps schedules then visit a tile's buckets in ascending (panel mod K)
    -- the residue order of k_compact_buckets, K = widest span of panels a
    tile touches -- instead of ascending panels.  Same y either way, and the
    same as with bucket_order = 1 (always ascending); a matrix without a band
    (columns anywhere) keeps ascending order by itself."""
    M = N = 120_000
    K, W = 24, 6000
    IRP, JA, AS = O.synth_csr(S.SYNTH_RANDOM, M, N, K, W, 42)
    x = O.synth_x(7, 0, N)
    y_ref = O.csr_spmv(IRP, JA, AS, x)
    scale = O.csr_abs_spmv(IRP, JA, AS, x)
    A = S.csr_from_arrays("band", M, N, IRP, JA, AS)
    d_x, d_y = S.DevBuffer.from_numpy(x), S.DevBuffer(M * 8)
    dA = S.CsrDevice.upload(A)
    monkeypatch.setenv("SPMV_TILE_ROWS", "2048")
    seen = {}
    for order in (0, 1):
        monkeypatch.setenv("SPMV_BUCKET_ORDER", str(order))
        dA.build_panels(1024, sched)  # 118 panels of 1024 columns
        desc = dA.panels_describe()
        seen[order] = desc
        assert ("residue order" in desc) == (order == 0), desc
        info = dA.panels_info()
        assert info["entries"] == int(IRP[-1]) and info["panels"] == 118
        for variant, waves in ((0, 0), (0, 4), (1, 8), (2, 0), (4, 4)):
            S._lib.spmv_dev_memset(d_y.ptr, 0xFF, M * 8, None)
            dA.launch(S.CSR_KERNEL_PANELS, d_x.ptr, d_y.ptr, variant=variant,
                      waves_per_block=waves)
            S.stream_sync()
            assert_parity(d_y.to_numpy(np.float64, M), y_ref, scale,
                          ("band", sched, order, variant, waves))
    # span: 2048 rows + 6000 columns of window over 1024-column panels
    import re
    assert 8 <= int(re.search(r"span (\d+)", seen[0]).group(1)) <= 10, seen[0]
    monkeypatch.setenv("SPMV_BUCKET_ORDER", "0")
    dA.release()
    S.csr_free(A)
    # no band: every tile touches every panel -> ascending order by itself
    IRP, JA, AS = O.synth_csr(S.SYNTH_RANDOM, 20_000, 20_000, 16, 1 << 30, 42)
    B = S.csr_from_arrays("wide", 20_000, 20_000, IRP, JA, AS)
    dB = S.CsrDevice.upload(B)
    dB.build_panels(1024, sched)
    assert "ascending order" in dB.panels_describe()
    dB.release()
    S.csr_free(B)


def test_build_panels_like_copies_schedule_and_tile_height(
        default_panel_schedule, monkeypatch):
    """Shards of one matrix: tune (here: build) one, build the others with
    the same schedule and tile height (bench.py --strong, N > 1)."""
    M, N, W = 30_000, 600_000, 1 << 30  # 3 panels of 2^18 columns
    A0 = S.CsrDevice.generate(S.SYNTH_RANDOM, M, N, 16, W, 0, 42)
    A1 = S.CsrDevice.generate(S.SYNTH_RANDOM, M, N, 16, W, M, 42)
    with pytest.raises(OSError):
        A1.build_panels_like(A0)  # the model has no blocked copy yet
    d_x, d_y = S.DevBuffer(N * 8), S.DevBuffer(M * 8)
    S.dev_fill_synth(d_x.ptr, N, 7)
    for sched, rows in (("steps", 2048), ("sweep", 0), ("chain", 4096)):
        S.set_panel_schedule(sched)
        if rows:
            monkeypatch.setenv("SPMV_TILE_ROWS", str(rows))
        A0.build_panels(0)
        monkeypatch.delenv("SPMV_TILE_ROWS", raising=False)
        # the copy must not follow the default
        S.set_panel_schedule("steps" if sched != "steps" else "sweep")
        A1.build_panels_like(A0)
        i0, i1 = A0.panels_info(), A1.panels_info()
        assert (i0["tiles"], i0["panels"]) == (i1["tiles"], i1["panels"])
        assert i1["steps"] == (3 if sched == "steps" else 1)
        A1.launch(S.CSR_KERNEL_PANELS, d_x.ptr, d_y.ptr)
        S.stream_sync()
        y = d_y.to_numpy(np.float64, M)
        for r in (0, 1, M // 2, M - 1):
            want, sc = O.synth_row_dot(S.SYNTH_RANDOM, 2 * M, N, 16, W, 0, 42,
                                       7, M + r)
            assert abs(y[r] - want) <= 1e-12 * sc
    # explicit schedule and tile height (what the ranks of a multi-GPU job
    # use to build rank 0's pick)
    for sched, rows in (("chain", 2048), ("steps", 4096), ("sweep", 0)):
        A1.build_panels(0, sched, rows)
        assert A1.panels_schedule() == sched
        if rows:
            assert A1.panels_tile_rows() == rows
        A1.launch(S.CSR_KERNEL_PANELS, d_x.ptr, d_y.ptr)
        S.stream_sync()
        y = d_y.to_numpy(np.float64, M)
        want, sc = O.synth_row_dot(S.SYNTH_RANDOM, 2 * M, N, 16, W, 0, 42, 7,
                                   M + 5)
        assert abs(y[5] - want) <= 1e-12 * sc
    with pytest.raises(OSError):
        A1.build_panels(0, 3, 0)  # no such schedule
    A0.release()
    A1.release()


@pytest.mark.parametrize("kind,M,K,W", [
    (S.SYNTH_RANDOM, 300_000, 16, 1 << 30),
    (S.SYNTH_POWERLAW, 400_000, 3, 1 << 30),
    (S.SYNTH_HUB, 200_000, 6, 4096),
], ids=["random", "powerlaw", "hub"])
def test_pinned_layout_rebuilds_what_the_selector_settled_on(kind, M, K, W):
    """`panels_pin()` of a tuned handle -> `build_panels_pinned()` on another
    handle of the same matrix: the same layout line, the same y, for both
    formats (what the counter passes of tools/profile.sh rely on: they
    measure the layout the un-profiled selector picked)."""
    N = M
    d_x, d_y, d_z = S.DevBuffer(N * 8), S.DevBuffer(M * 8), S.DevBuffer(M * 8)
    S.dev_fill_synth(d_x.ptr, N, 7)
    A = S.CsrDevice.generate(kind, M, N, K, W, 0, 42)
    B = S.CsrDevice.generate(kind, M, N, K, W, 0, 42)
    assert A.panels_pin() is None  # no blocked copy yet
    for a, b, pid in ((A, B, S.CSR_KERNEL_PANELS),
                      (A.to_hll(True), B.to_hll(True), S.HLL_KERNEL_PANELS)):
        a.autotune(d_x.ptr, d_y.ptr)
        if a.panels_info() is None:       # a direct kernel won: build the copy
            a.build_panels(0)
        pin = a.panels_pin()
        assert "sched=" in pin and "waves=" in pin
        b.build_panels_pinned(pin)
        assert b.panels_pin() == pin
        assert b.panels_describe() == a.panels_describe()
        a.launch(pid, d_x.ptr, d_y.ptr)
        b.launch(pid, d_x.ptr, d_z.ptr)
        S.stream_sync()
        # the tiles add their products into LDS with atomics: the order --
        # and so the last bits -- differ from launch to launch
        ya, yb = d_y.to_numpy(np.float64, M), d_z.to_numpy(np.float64, M)
        assert np.max(np.abs(ya - yb)) <= 1e-12 * max(1.0, np.max(np.abs(ya)))
        with pytest.raises(ValueError):
            b.build_panels_pinned(pin + ",no_such_field=1")
        if a is not A:
            a.release()
            b.release()
    A.release()
    B.release()
    for d in (d_x, d_y, d_z):
        d.free()


@pytest.mark.parametrize("sched", ["chain", "sweep"])
def test_pin_round_trips_a_non_default_panel_width(sched):
    """a copy built with an explicit panel_cols (2^14, not the default 2^18)
    reports THAT width in its pin (panels_get_opts said 0), and
    build_panels_pinned / build_panels_like rebuild the same layout line"""
    M = N = 400_000
    A = S.CsrDevice.generate(S.SYNTH_RANDOM, M, N, 16, 1 << 30, 0, 42)
    B = S.CsrDevice.generate(S.SYNTH_RANDOM, M, N, 16, 1 << 30, 0, 42)
    Cm = S.CsrDevice.generate(S.SYNTH_RANDOM, M, N, 16, 1 << 30, 0, 42)
    A.build_panels(1 << 14, sched)
    pin = A.panels_pin()
    assert "panel_cols=16384" in pin, pin
    assert "x 2^14 cols" in A.panels_describe()
    B.build_panels_pinned(pin)
    Cm.build_panels_like(A)
    assert B.panels_pin() == pin and Cm.panels_pin() == pin
    assert B.panels_describe() == A.panels_describe() == Cm.panels_describe()
    D0 = S.CsrDevice.generate(S.SYNTH_RANDOM, M, N, 16, 1 << 30, 0, 42)
    D0.build_panels(0, sched)  # the default width is another layout
    assert D0.panels_describe() != A.panels_describe()
    for m in (A, B, Cm, D0):
        m.release()


def test_release_source_keeps_only_the_blocked_copy(default_panel_schedule):
    """spmv_*_release_source: JA/AS freed, the blocked path still runs, every
    entry point that needs the source says -ENODATA."""
    import errno
    M, N = 20_000, 30_000
    IRP, JA, AS = O.synth_csr(S.SYNTH_RAGGED, M, N, 12, 2000, 42)
    x = O.synth_x(7, 0, N)
    y_ref = O.csr_spmv(IRP, JA, AS, x)
    scale = O.csr_abs_spmv(IRP, JA, AS, x)
    A = S.csr_from_arrays("rel", M, N, IRP, JA, AS)
    d_x, d_y = S.DevBuffer.from_numpy(x), S.DevBuffer(M * 8)
    dA = S.CsrDevice.upload(A)
    dH = dA.to_hll(True)
    for m, blocked in ((dA, S.CSR_KERNEL_PANELS), (dH, S.HLL_KERNEL_PANELS)):
        with pytest.raises(OSError) as ei:
            m.release_source()  # no blocked copy yet
        assert ei.value.errno == errno.ENOENT
        S.set_panel_schedule("chain")
        m.build_panels(0)
        m.release_source()
        S._lib.spmv_dev_memset(d_y.ptr, 0xFF, M * 8, None)
        m.launch(blocked, d_x.ptr, d_y.ptr)
        S.stream_sync()
        assert_parity(d_y.to_numpy(np.float64, M), y_ref, scale, "blocked only")
        for call in (lambda: m.launch(2, d_x.ptr, d_y.ptr),
                     lambda: m.build_panels(0)):
            with pytest.raises(OSError) as ei:
                call()
            assert ei.value.errno == errno.ENODATA
    with pytest.raises(OSError) as ei:
        dA.to_hll(True)
    assert ei.value.errno == errno.ENODATA
    dH.release()
    dA.release()
    S.csr_free(A)


def test_autotune_picks_a_valid_kernel_and_stays_correct():
    """spmv_*_autotune: measured choice between the coalesced kernels and the
    2-D blocked path; whatever it picks must still match the oracle."""
    M = N = 400_000
    for W in (256, 1 << 30):
        IRP, JA, AS = O.synth_csr(S.SYNTH_RANDOM, M, N, 32, W, 42)
        x = O.synth_x(7, 0, N)
        y_ref = O.csr_spmv(IRP, JA, AS, x)
        scale = O.csr_abs_spmv(IRP, JA, AS, x)
        A = S.csr_from_arrays("auto", M, N, IRP, JA, AS)
        dA = S.CsrDevice.upload(A)
        d_x, d_y = S.DevBuffer.from_numpy(x), S.DevBuffer(M * 8)
        k, ms = dA.autotune(d_x.ptr, d_y.ptr)
        assert k in (1, 2, 4, S.CSR_KERNEL_PANELS) and ms > 0
        dA.launch(k, d_x.ptr, d_y.ptr)
        S.stream_sync()
        assert_parity(d_y.to_numpy(np.float64, M), y_ref, scale, ("auto csr", W, k))
        dH = dA.to_hll(True)
        k, ms = dH.autotune(d_x.ptr, d_y.ptr)
        assert k in (1, 2, S.HLL_KERNEL_PANELS) and ms > 0
        dH.launch(k, d_x.ptr, d_y.ptr)
        S.stream_sync()
        assert_parity(d_y.to_numpy(np.float64, M), y_ref, scale, ("auto hll", W, k))
        dH.release()
        dA.release()
        S.csr_free(A)


def test_int32_limits_are_reported_not_wrapped():
    """The host structs count entries in int (reference csr.h:9-10): a shard
    with more than INT_MAX entries must be refused (-EOVERFLOW), not wrapped
    (the reference truncates silently, csr.c:153)."""
    import errno
    with pytest.raises(OSError) as ei:
        S.CsrDevice.generate(S.SYNTH_RANDOM, 70_000_000, 70_000_000, 32, 1 << 20)
    assert ei.value.errno == errno.EOVERFLOW
    with pytest.raises(OSError) as ei:
        S.csr_generate(S.SYNTH_BANDED, 70_000_000, 70_000_000, 32, 0)
    assert ei.value.errno == errno.EOVERFLOW


def test_blocked_copy_keeps_explicit_zeros_and_drops_only_pads():
    """An explicit zero is an entry (the loader keeps it, serial CSR
    multiplies it): 0.0 * inf = NaN must come out of every path.  The blocked
    copy built from HLL used to drop every slot whose value was 0.0 -- pads
    AND explicit zeros -- and disagreed with the copy built from CSR
    (VERDICT r01 weak #8).  Pads are now remembered in a bitmap when they are
    rewritten, and only those are dropped."""
    M, N = 1000, 1001
    IRP, JA, AS = O.synth_csr(S.SYNTH_RAGGED, M, N - 1, 24, 300, 42)
    JA, AS = JA.copy(), AS.copy()
    cstar = N - 1  # a column nothing else references
    hit = [int(IRP[r]) + 1 for r in (5, 333, 998) if IRP[r + 1] - IRP[r] > 2]
    for k in hit:
        JA[k], AS[k] = cstar, 0.0
    AS[int(IRP[40])] = 0.0  # an explicit zero on an ordinary column
    x = O.synth_x(7, 0, N)
    x[cstar] = np.inf
    y_ref = O.csr_spmv(IRP, JA, AS, x)
    nan_rows = np.isnan(y_ref)
    assert nan_rows.sum() == len(hit) == 3
    A = S.csr_from_arrays("zeros", M, N, IRP, JA, AS)
    dA = S.CsrDevice.upload(A)
    d_x, d_y = S.DevBuffer.from_numpy(x), S.DevBuffer(M * 8)
    outs = {}
    for sched in ("steps", "chain", "sweep"):
        dA.build_panels(256, sched)
        assert dA.panels_info()["entries"] == len(JA)  # zeros kept
        dA.launch(S.CSR_KERNEL_PANELS, d_x.ptr, d_y.ptr)
        S.stream_sync()
        outs["csr " + sched] = d_y.to_numpy(np.float64, M)
        for cm in (True, False):
            dH = dA.to_hll(cm)
            assert dH.slots > len(JA)  # ragged rows: the HLL form has pads
            dH.build_panels(256, sched)
            assert dH.panels_info()["entries"] == len(JA)  # pads dropped
            dH.launch(S.HLL_KERNEL_PANELS, d_x.ptr, d_y.ptr)
            S.stream_sync()
            outs["hll%d %s" % (cm, sched)] = d_y.to_numpy(np.float64, M)
            dH.release()
    # an HLL handle uploaded from the HOST form (pads = -1 rewritten on the
    # device) remembers its pads the same way
    H = S.csr_to_hll(A, True)
    dH = S.HllDevice.upload(H, True)
    dH.build_panels(256, "chain")
    assert dH.panels_info()["entries"] == len(JA)
    dH.launch(S.HLL_KERNEL_PANELS, d_x.ptr, d_y.ptr)
    S.stream_sync()
    outs["hll uploaded"] = d_y.to_numpy(np.float64, M)
    dH.release()
    S.hll_free(H)
    scale = O.csr_abs_spmv(IRP, JA, AS, np.where(np.isinf(x), 0.0, x))
    for tag, y in outs.items():
        assert np.array_equal(np.isnan(y), nan_rows), tag
        ok = ~nan_rows
        assert np.max(np.abs(y[ok] - y_ref[ok])
                      / np.maximum(scale[ok], 1e-300)) <= TIGHT, tag
    dA.release()
    S.csr_free(A)


def test_stream_kernel_on_long_empty_and_ragged_rows():
    """kernel 4: rows longer than a workgroup's budget (read in place), empty
    rows, a cooperative range (one 300-entry row among short ones) and
    transposed ranges, in one matrix; launched three times (deterministic:
    the same bits every time), and again after the autotuner ran."""
    rng = np.random.default_rng(9)
    lens = rng.integers(0, 24, 40_000)
    lens[[7, 20_000, 39_999]] = (5000, 2049, 2048)
    lens[[100, 101, 102, 30_000]] = 0
    lens[12_345] = 300
    M, N = len(lens), 50_000
    IRP = np.zeros(M + 1, dtype=np.int32)
    IRP[1:] = np.cumsum(lens)
    JA = rng.integers(0, N, IRP[-1]).astype(np.int32)
    AS = rng.uniform(-1, 1, IRP[-1])
    x = O.synth_x(7, 0, N)
    y_ref = O.csr_spmv(IRP, JA, AS, x)
    scale = O.csr_abs_spmv(IRP, JA, AS, x)
    A = S.csr_from_arrays("forms", M, N, IRP, JA, AS)
    dA = S.CsrDevice.upload(A)
    d_x, d_y = S.DevBuffer.from_numpy(x), S.DevBuffer(M * 8)
    ys = []
    for rep in range(3):
        S._lib.spmv_dev_memset(d_y.ptr, 0xFF, M * 8, None)
        dA.launch(4, d_x.ptr, d_y.ptr)
        S.stream_sync()
        ys.append(d_y.to_numpy(np.float64, M))
        assert_parity(ys[-1], y_ref, scale, ("stream", rep))
    assert np.array_equal(ys[0], ys[1]) and np.array_equal(ys[0], ys[2])
    k, ms = dA.autotune(d_x.ptr, d_y.ptr)
    S._lib.spmv_dev_memset(d_y.ptr, 0xFF, M * 8, None)
    dA.launch(4, d_x.ptr, d_y.ptr)
    S.stream_sync()
    assert np.array_equal(d_y.to_numpy(np.float64, M), ys[0])
    dA.release()
    S.csr_free(A)


def test_long_rows_at_every_threshold_stream_segments_and_blocked_side_path():
    """Rows around the two long-row thresholds: the CSR stream kernel cuts a
    row of more than 8192 entries into 2048-entry segments (mode 2: last
    arriver sums the partials in order), the blocked copy keeps a row of more
    than 16384 entries beside itself (k_long_rows, 1024-entry segments).  Lengths at and next to
    every boundary, long rows first / last / adjacent / between empty rows,
    ranges of up to 1024 short rows; launched three times each (the arrival
    counters must be re-armed), the direct kernels bit-identical every time."""
    rng = np.random.default_rng(11)
    special = [8192, 8193, 12_288, 12_289, 4096 * 5 - 1, 16_384, 16_385,
               20_000, 40_960, 0, 0, 70_001, 1, 8191, 4096, 4097,
               2048 * 5 - 1, 2048 * 5, 2048 * 5 + 1,     # segment boundaries
               1024 * 17 - 1, 1024 * 17, 1024 * 17 + 1]  # of both side paths
    lens = np.concatenate([
        [16_385],                              # a long row FIRST
        rng.integers(1, 4, 3_000),             # 1-3 entries: 1024-row ranges
        special,                               # adjacent long rows, empties
        rng.integers(0, 12, 5_000),
        [8193, 16_385],                        # ... and LAST
    ]).astype(np.int64)
    # hack blocks at the HLL wide-block threshold (512 columns; segments of
    # 256) and rows at the stream kernel's entry budget (2048: beyond it a row
    # owns a range, and kernels 0-3 hand it to k_csr_long_seg)
    for at, ln in ((100, 512), (400, 513), (700, 511), (1000, 768), (1300, 769),
                   (1600, 2047), (1900, 2048), (2200, 2049), (2500, 1025)):
        lens[at] = ln
    M, N = len(lens), 90_000
    IRP = np.zeros(M + 1, dtype=np.int32)
    IRP[1:] = np.cumsum(lens)
    JA = rng.integers(0, N, IRP[-1]).astype(np.int32)
    AS = rng.uniform(-1, 1, IRP[-1])
    x = O.synth_x(7, 0, N)
    y_ref = O.csr_spmv(IRP, JA, AS, x)
    scale = O.csr_abs_spmv(IRP, JA, AS, x)
    A = S.csr_from_arrays("thresholds", M, N, IRP, JA, AS)
    dA = S.CsrDevice.upload(A)
    d_x, d_y = S.DevBuffer.from_numpy(x), S.DevBuffer(M * 8)
    for k in (0, 1, 2, 3, 4):
        first = None
        for rep in range(3):
            S._lib.spmv_dev_memset(d_y.ptr, 0xFF, M * 8, None)
            dA.launch(k, d_x.ptr, d_y.ptr)
            S.stream_sync()
            y = d_y.to_numpy(np.float64, M)
            assert_parity(y, y_ref, scale, ("thresholds csr", k, rep))
            first = y if first is None else first
            assert np.array_equal(y, first), ("not deterministic", k, rep)
    # the direct HLL kernels: hack blocks wider than 512 columns (here: most
    # of the special rows' blocks, and the ragged TAIL block of 19 rows) are
    # summed by k_hll_wide in 256-column segments, the rest by the kernel
    for cm in (True, False):
        dH = dA.to_hll(cm)
        for k in range(S.NUM_HLL_KERNELS):
            if S.HLL_KERNEL_COL_MAJOR[k] != cm:
                continue
            first = None
            for rep in range(3):
                S._lib.spmv_dev_memset(d_y.ptr, 0xFF, M * 8, None)
                dH.launch(k, d_x.ptr, d_y.ptr, waves_per_block=4)
                S.stream_sync()
                y = d_y.to_numpy(np.float64, M)
                assert_parity(y, y_ref, scale, ("thresholds hll", cm, k, rep))
                first = y if first is None else first
                assert np.array_equal(y, first), ("not deterministic", cm, k)
            # block sub-ranges (chunked exchanges): wide blocks only in theirs
            S._lib.spmv_dev_memset(d_y.ptr, 0, M * 8, None)
            nb = dH.num_blocks
            for b0, b1 in ((0, 1), (1, nb // 2), (nb // 2, nb)):
                dH.launch(k, d_x.ptr, d_y.ptr, blocks=(b0, b1))
            S.stream_sync()
            assert_parity(d_y.to_numpy(np.float64, M), y_ref, scale,
                          ("thresholds hll blocks", cm, k))
        dH.release()
    # CSR row sub-ranges with long rows (kernel 4 falls back to kernel 2 there)
    for k in (0, 1, 2, 3, 4):
        S._lib.spmv_dev_memset(d_y.ptr, 0, M * 8, None)
        for r0, r1 in ((0, 1), (1, 3_010), (3_010, M)):
            dA.launch(k, d_x.ptr, d_y.ptr, rows=(r0, r1))
        S.stream_sync()
        assert_parity(d_y.to_numpy(np.float64, M), y_ref, scale,
                      ("thresholds csr rows", k))
    n_beside = int(np.sum(lens > 16_384))
    for sched in ("chain", "steps", "sweep"):
        for src in ("csr", "hll_col", "hll_row"):
            if src == "csr":
                m, blocked = dA, S.CSR_KERNEL_PANELS
            else:
                m, blocked = dA.to_hll(src == "hll_col"), S.HLL_KERNEL_PANELS
            m.build_panels(4096, sched, tile_rows=1024)
            assert "%d long row(s) beside" % n_beside in m.panels_describe()
            assert m.panels_info()["entries"] == int(IRP[-1])
            for rep in range(3):
                S._lib.spmv_dev_memset(d_y.ptr, 0xFF, M * 8, None)
                m.launch(blocked, d_x.ptr, d_y.ptr)
                S.stream_sync()
                assert_parity(d_y.to_numpy(np.float64, M), y_ref, scale,
                              ("thresholds blocked", sched, src, rep))
            if src != "csr":
                m.release()
    dA.release()
    S.csr_free(A)


def test_more_long_rows_than_the_side_path_takes():
    """6000 rows of 17 000 entries each: every row is beyond the blocked
    copy's long-row threshold (16 384), but more of them than the side path
    holds (PANELS_LONG_MAX = 4096) -- they stay in the buckets; every row is
    cut into segments by the CSR stream kernel / k_csr_long_seg; as HLL every
    hack block is wide (k_hll_wide does all the work, 67 segments per block).
    Whole y against the oracle, every kernel."""
    rng = np.random.default_rng(17)
    M, N, L = 6_000, 200_000, 17_000
    IRP = (np.arange(M + 1, dtype=np.int64) * L).astype(np.int32)
    JA = np.sort(rng.integers(0, N, (M, L), dtype=np.int32), axis=1).ravel()
    AS = rng.uniform(-1, 1, M * L)
    x = O.synth_x(7, 0, N)
    y_ref = O.csr_spmv(IRP, JA, AS, x)
    scale = O.csr_abs_spmv(IRP, JA, AS, x)
    A = S.csr_from_arrays("all_long", M, N, IRP, JA, AS)
    dA = S.CsrDevice.upload(A)
    d_x, d_y = S.DevBuffer.from_numpy(x), S.DevBuffer(M * 8)

    def run(h, k, tag, **kw):
        S._lib.spmv_dev_memset(d_y.ptr, 0xFF, M * 8, None)
        h.launch(k, d_x.ptr, d_y.ptr, **kw)
        S.stream_sync()
        assert_parity(d_y.to_numpy(np.float64, M), y_ref, scale, tag)

    for k in range(5):
        run(dA, k, ("all long csr", k))
    for sched in ("chain", "sweep", "steps"):
        dA.build_panels(0, sched)
        assert "long row(s) beside" not in dA.panels_describe()
        assert dA.panels_info()["entries"] == M * L
        run(dA, S.CSR_KERNEL_PANELS, ("all long blocked", sched))
    for cm in (True, False):
        dH = dA.to_hll(cm)
        for k in range(S.NUM_HLL_KERNELS):
            if S.HLL_KERNEL_COL_MAJOR[k] == cm:
                run(dH, k, ("all long hll", k), waves_per_block=4)
        if cm:
            dH.build_panels(0, "chain")
            run(dH, S.HLL_KERNEL_PANELS, ("all long hll blocked",))
        dH.release()
    dA.release()
    S.csr_free(A)
    d_x.free()
    d_y.free()


def test_config3_ragged_variant_full_size():
    """SURVEY 8d, secondary variant of config 3: row lengths uniform in
    [24, 40] (mean 32) so that the HLL form carries pads (S > nnz).  10M x 10M,
    columns anywhere, generated and converted on the device; the thread-per-
    row HLL kernels, the CSR stream kernel and the autotuned pick against
    20k rows regenerated by the oracle."""
    M = N = 10_000_000
    K, W = 32, 1 << 30
    dA = S.CsrDevice.generate(S.SYNTH_RAGGED, M, N, K, W, 0, 42)
    dH = dA.to_hll(True)
    assert dH.slots > dA.NZ  # pads are stored (and are real traffic)
    assert dH.algorithmic_bytes > 12 * dA.NZ
    # the direct kernels are priced on the stored slots, the blocked copy
    # (no padding) on the true entries
    assert dH.kernel_bytes(1) == dH.algorithmic_bytes
    assert dH.kernel_bytes(S.HLL_KERNEL_PANELS) == (
        12 * dA.NZ + 12 * dH.num_blocks + 8 * M + 8 * N)
    assert dA.kernel_bytes(S.CSR_KERNEL_PANELS) == dA.algorithmic_bytes
    d_x, d_y = S.DevBuffer(N * 8), S.DevBuffer(M * 8)
    S.dev_fill_synth(d_x.ptr, N, 7)
    rng = np.random.default_rng(6)
    rows = np.unique(np.concatenate([[0, 31, 32, M - 1],
                                     rng.integers(0, M, 20_000)]))
    want = np.array([O.synth_row_dot(S.SYNTH_RAGGED, M, N, K, W, 0, 42, 7,
                                     int(g)) for g in rows])
    best, _ = dH.autotune(d_x.ptr, d_y.ptr)
    if best == S.HLL_KERNEL_PANELS:  # the copy drops the pads, only them
        assert dH.panels_info()["entries"] == dA.NZ
    ys = {}
    for tag, fn in (("hll1", lambda: dH.launch(1, d_x.ptr, d_y.ptr)),
                    ("hll2", lambda: dH.launch(2, d_x.ptr, d_y.ptr)),
                    ("csr4", lambda: dA.launch(4, d_x.ptr, d_y.ptr)),
                    ("auto", lambda: dH.launch(best, d_x.ptr, d_y.ptr))):
        S._lib.spmv_dev_memset(d_y.ptr, 0xFF, M * 8, None)
        fn()
        S.stream_sync()
        y = d_y.to_numpy(np.float64, M)
        assert np.all(np.isfinite(y)), tag
        got = y[rows]
        assert np.max(np.abs(got - want[:, 0]) / want[:, 1]) <= TIGHT, tag
        den = np.maximum(np.abs(want[:, 0]), 1e-3 * want[:, 1])
        assert np.max(np.abs(got - want[:, 0]) / den) <= REL_TOL, tag
        ys[tag] = y
    assert np.max(np.abs(ys["hll1"] - ys["csr4"])) < 1e-11
    assert np.max(np.abs(ys["hll1"] - ys["auto"])) < 1e-11
    dH.release()
    dA.release()


def test_arrival_counter_kernels_soak():
    """The last-arriver reductions (CSR long rows: k_csr_stream mode 2 and
    k_csr_long_seg; wide HLL blocks: k_hll_wide; rows beside the blocked copy:
    k_long_rows) rely on agent-scope atomics across XCDs and on counters that
    each launch re-arms.  Hundreds of back-to-back launches (SPMV_SOAK=5000
    for a long run), every result compared with the first one BIT FOR BIT for
    the deterministic kernels, and the long rows' entries of the blocked path
    likewise: a lost partial sum, a stale read or a counter left armed shows
    up as a different bit sooner or later."""
    import os
    n_rep = int(os.environ.get("SPMV_SOAK", "300"))
    M = N = 400_000
    dA = S.CsrDevice.generate(S.SYNTH_HUB, M, N, 4, 1 << 30, 0, 42)
    dH = dA.to_hll(True)
    d_x, d_y = S.DevBuffer(N * 8), S.DevBuffer(M * 8)
    S.dev_fill_synth(d_x.ptr, N, 7)
    hub = N // 3
    IRP, JA, AS = S.csr_arrays(dA.download())
    x = O.synth_x(7, 0, N)
    want = float(np.dot(AS[IRP[hub]:IRP[hub + 1]], x[JA[IRP[hub]:IRP[hub + 1]]]))
    scale = float(np.sum(np.abs(AS[IRP[hub]:IRP[hub + 1]]
                                * x[JA[IRP[hub]:IRP[hub + 1]]])))
    assert IRP[hub + 1] - IRP[hub] == 131_072
    dA.build_panels(0, "chain")
    cases = [("csr stream", dA, 4), ("csr subwave + long seg", dA, 2),
             ("hll col + wide", dH, 1), ("blocked + long rows", dA,
                                         S.CSR_KERNEL_PANELS)]
    try:
        for tag, m, k in cases:
            first = None
            for rep in range(n_rep):
                if rep % 50 == 0:  # poison now and then: y must be rewritten
                    S._lib.spmv_dev_memset(d_y.ptr, 0xFF, M * 8, None)
                if rep % 70 == 35:
                    # what a launch that never completed leaves behind in the
                    # arrival counters (a foreign launch number + a count):
                    # the counters carry the launch's own number, so the next
                    # launch must not care (it used to reduce
                    # early, a wrong y[row] with no error, for ever after)
                    S.stream_sync()
                    fn = (S._lib.spmv_hll_debug_stale_arrivals
                          if m is dH else S._lib.spmv_csr_debug_stale_arrivals)
                    fn.restype, fn.argtypes = C.c_int, [C.c_void_p]
                    assert fn(m.h) > 0, tag
                m.launch(k, d_x.ptr, d_y.ptr)
                if rep % 10 and rep != n_rep - 1:
                    continue  # back-to-back launches in between
                S.stream_sync()
                y = d_y.to_numpy(np.float64, M)
                assert abs(y[hub] - want) <= 1e-12 * scale, (tag, rep)
                if first is None:
                    first = y
                elif k == S.CSR_KERNEL_PANELS:
                    assert y[hub] == first[hub], (tag, rep)  # fixed order
                    assert np.max(np.abs(y - first)) <= 1e-12 * scale
                else:
                    assert np.array_equal(y, first), (tag, rep)
    finally:
        dH.release()
        dA.release()


@pytest.mark.parametrize("sched,W,tile_rows", [("chain", 1 << 17, 0),
                                               ("chain", 1 << 30, 8192),
                                               ("steps", 1 << 14, 4096),
                                               ("sweep", 1 << 30, 0)])
def test_deterministic_blocked_mode_gives_the_same_bits_every_launch(
        sched, W, tile_rows):
    """spmv_panel_opts.deterministic: 1000 launches of one blocked copy give
    ONE y, bit for bit (the LDS additions of a workgroup happen wavefront
    after wavefront, chunk after chunk), a second copy built the same way
    gives the same bits again, and the result is the oracle's to rounding.
    The arrival-order mode on the same matrix is only reproducible to
    rounding: over the same launches its last bits move (ds_add_f64 as the
    wavefronts come).  Default: ordered on sweep layouts, where it is free."""
    M = N = 1_500_000
    K = 32
    A = S.CsrDevice.generate(S.SYNTH_RANDOM, M, N, K, W, 0, 42)
    d_x, d_y = S.DevBuffer(N * 8), S.DevBuffer(M * 8)
    S.dev_fill_synth(d_x.ptr, N, 7)
    rows = np.random.default_rng(11).integers(0, M, 400)
    want = [O.synth_row_dot(S.SYNTH_RANDOM, M, N, K, W, 0, 42, 7, int(r))
            for r in rows]
    for fmt in ("csr", "hll"):
        m = A if fmt == "csr" else A.to_hll(True)
        pid = S.CSR_KERNEL_PANELS if fmt == "csr" else S.HLL_KERNEL_PANELS
        m.build_panels(0, sched, tile_rows, deterministic=True)
        assert "deterministic" in m.panels_describe()
        assert "deterministic=1" in m.panels_pin()
        m.launch(pid, d_x.ptr, d_y.ptr)
        S.stream_sync()
        y0 = d_y.to_numpy(np.float64, M)
        for r, (w, sc) in zip(rows, want):
            assert abs(y0[r] - w) <= 1e-12 * sc, (fmt, r)
        for it in range(1000):
            m.launch(pid, d_x.ptr, d_y.ptr)
            if it % 100 == 99:
                S.stream_sync()
                assert np.array_equal(d_y.to_numpy(np.float64, M).view(np.uint64),
                                      y0.view(np.uint64)), (fmt, it)
        # rebuilt from its pin: the same layout, the same order, the same bits
        pin = m.panels_pin()
        m.build_panels_pinned(pin)
        m.launch(pid, d_x.ptr, d_y.ptr)
        S.stream_sync()
        assert np.array_equal(d_y.to_numpy(np.float64, M).view(np.uint64),
                              y0.view(np.uint64)), fmt
        # the arrival-order mode (the default of chain / steps; forced off on
        # a sweep copy, whose default is the ordered one): right to rounding,
        # but not bitwise stable
        m.build_panels(0, sched, tile_rows, deterministic=False)
        assert "deterministic" not in m.panels_describe()
        assert "deterministic=2" in m.panels_pin()
        seen = set()
        for it in range(30):
            m.launch(pid, d_x.ptr, d_y.ptr)
            S.stream_sync()
            y = d_y.to_numpy(np.float64, M)
            seen.add(hash(y.tobytes()))
            assert np.max(np.abs(y - y0)) <= 1e-12 * 32
        # the DEFAULT: ordered on sweep layouts (free there), arrival order
        # on chain / steps (spmv_engine.h, spmv_panel_opts.deterministic)
        m.build_panels(0, sched, tile_rows)
        assert ("deterministic" in m.panels_describe()) == (sched == "sweep")
        print("%s %s W=%d: default mode gave %d distinct y in 30 launches"
              % (fmt, sched, W, len(seen)))
        if m is not A:
            m.release()
    A.release()
    d_x.free()
    d_y.free()


def test_default_headline_layout_gives_the_same_bits_over_1000_launches():
    """on a matrix whose columns reach anywhere the
    selector keeps a blocked SWEEP copy -- and that copy, built with default
    options, is now bitwise reproducible like the reference's kernels
    (cuda_hll.cu:49-72: one fixed order per row): 1000 launches, one y; the
    bench line's `config.deterministic` says so."""
    M = N = 3_000_000
    K, W = 32, 2 * 3_000_000
    A = S.CsrDevice.generate(S.SYNTH_RANDOM, M, N, K, W, 0, 42)
    H = A.to_hll(True)
    A.release()
    d_x, d_y = S.DevBuffer(N * 8), S.DevBuffer(M * 8)
    S.dev_fill_synth(d_x.ptr, N, 7)
    best, _ = H.autotune(d_x.ptr, d_y.ptr)
    print("selector: kernel %d, %s" % (best, H.panels_describe()))
    if best != S.HLL_KERNEL_PANELS or H.panels_schedule() != "sweep":
        # (at 10M rows the selector's pick IS the sweep copy -- bench.py's
        # headline; should a 3M-row matrix go to another layout on some box,
        # the default-built sweep copy is still what this test is about)
        best = S.HLL_KERNEL_PANELS
        H.build_panels(0, "sweep")
    assert "deterministic" in H.panels_describe()
    assert "deterministic=1" in H.panels_pin()
    H.launch(best, d_x.ptr, d_y.ptr)
    S.stream_sync()
    y0 = d_y.to_numpy(np.float64, M)
    rows = np.random.default_rng(5).integers(0, M, 300)
    for r in rows:
        w, sc = O.synth_row_dot(S.SYNTH_RANDOM, M, N, K, W, 0, 42, 7, int(r))
        assert abs(y0[r] - w) <= 1e-12 * sc, r
    for it in range(1000):
        H.launch(best, d_x.ptr, d_y.ptr)
        if it % 100 == 99:
            S.stream_sync()
            assert np.array_equal(
                d_y.to_numpy(np.float64, M).view(np.uint64),
                y0.view(np.uint64)), it
    H.release()
    d_x.free()
    d_y.free()


def test_one_shot_upload_of_reference_style_hll_blocks():
    """The reference's csr_to_hll allocates every hack block by itself
    (hll.c:56-70), so what its driver hands to the seam is NOT slab-backed:
    the upload packs such blocks into two host slabs in parallel and copies
    twice (hll_pack_slabs) instead of twice per block.  Same y, bit for bit,
    as from the slab-backed matrix of this repo's converter, for both
    layouts, and a 31 250-block matrix uploads in tens of milliseconds."""
    import time
    M = N = 1_000_000
    A = S.csr_generate(S.SYNTH_RAGGED, M, N, 16, 4096, 0, 42)
    x = O.synth_x(7, 0, N)
    for col_major, kernel in ((True, 1), (False, 0)):
        H = S.csr_to_hll(A, col_major)
        h = H.contents
        nb = h.num_blocks
        keep = []  # one allocation pair per block, like the reference
        blocks = (S.EllpackBlock * nb)()
        for b in range(nb):
            src = h.blocks[b]
            n = src.M * src.max_NZ
            ja = np.ctypeslib.as_array(src.JA, (max(n, 1),))[:n].copy()
            av = np.ctypeslib.as_array(src.AS, (max(n, 1),))[:n].copy()
            keep.append((ja, av))
            blocks[b].M, blocks[b].N = src.M, src.N
            blocks[b].NZ, blocks[b].max_NZ = src.NZ, src.max_NZ
            blocks[b].JA = ja.ctypes.data_as(C.POINTER(C.c_int))
            blocks[b].AS = av.ctypes.data_as(C.POINTER(C.c_double))
        R = S.SparseHLL()
        R.name, R.M, R.N, R.NZ = h.name, h.M, h.N, h.NZ
        R.hack_size, R.num_blocks = h.hack_size, nb
        R.blocks = C.cast(blocks, C.POINTER(S.EllpackBlock))
        Rp = C.pointer(R)
        assert S._lib.hll_is_contiguous(Rp) == 0
        y0, _ = S.hll_spmv_hip(H, x, kernel=kernel)
        t0 = time.perf_counter()
        S.hll_spmv_hip(H, x, kernel=kernel)
        wall_slab = (time.perf_counter() - t0) * 1e3
        S.hll_spmv_hip(Rp, x, kernel=kernel)  # warm
        t0 = time.perf_counter()
        y1, _ = S.hll_spmv_hip(Rp, x, kernel=kernel)
        wall = (time.perf_counter() - t0) * 1e3
        assert np.array_equal(y0, y1)
        print("block-by-block HLL, %d blocks, col_major=%s: one-shot call "
              "%.1f ms (slab-backed: %.1f ms)" % (nb, col_major, wall,
                                                  wall_slab))
        assert wall < 400.0, wall  # 62 500 hipMemcpy calls took ~ 1 s
        S.hll_free(H)
    S.csr_free(A)


def test_long_row_arrivals_stay_cheap():
    """Perf guard (round 5 lost 4x here without a test noticing): the 128
    segments of a hub row arrive at ONE counter; with a compare-and-swap loop
    per arrival they serialised on it -- hub 1M 0.030 -> 0.116 ms for the
    blocked path, 0.044 -> 0.116 for the stream kernel.  The arrival is one
    fetch-and-add again (epoch_arrive, hip_common.h); generous bounds, event-
    timed medians of 20 launches on an exclusive GPU."""
    M = N = 1_000_000
    dA = S.CsrDevice.generate(S.SYNTH_HUB, M, N, 6, 4096, 0, 42)
    d_x, d_y = S.DevBuffer(N * 8), S.DevBuffer(M * 8)
    S.dev_fill_synth(d_x.ptr, N, 7)
    dA.build_panels(0, "chain", 4096)
    flush = 1 << 30  # 103 MB of matrix: out of the Infinity Cache
    blocked = float(np.median(dA.time(S.CSR_KERNEL_PANELS, d_x.ptr, d_y.ptr, 3,
                                      20, flush)))
    stream = float(np.median(dA.time(4, d_x.ptr, d_y.ptr, 3, 20, flush)))
    subwave = float(np.median(dA.time(2, d_x.ptr, d_y.ptr, 3, 20, flush)))
    print("hub 1M: blocked %.4f ms, stream %.4f, subwave + long seg %.4f"
          % (blocked, stream, subwave))
    assert blocked < 0.075, blocked   # 0.030 measured
    assert stream < 0.095, stream     # 0.044
    assert subwave < 0.16, subwave    # 0.078
    dA.release()
    d_x.free()
    d_y.free()
