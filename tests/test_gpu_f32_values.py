"""fp32-stored matrix values with fp64 products and sums (spmv_engine.h,
library 0.7) on the GPU: every direct kernel of both formats on f32 handles.

The expected result needs no new oracle and no new tolerance: an f32 handle
computes, in fp64 and in the order of the f64 kernels, the product of the
matrix whose values were rounded to fp32 -- so it is held to the project's
parity bound (1e-12 of the row scale sum_j |a_ij x_j|, as smoke() and
tests/test_gpu_parity.py) against the fp64 oracle applied to

    round32(AS) = AS.astype(np.float32).astype(np.float64)

and, bit for bit, to what the f64 handle of that rounded matrix gives.
Against the UN-rounded matrix the bound is derived: every a_ij moves by at
most the fp32 unit roundoff 2^-24 (round to nearest), so a row moves by at
most 2^-24 * sum_j |a_ij x_j|, plus the parity bound.

Every test runs under a time limit of its own (LIMIT_S): a test that exceeds
it ends the whole process, so nothing else is started on the device.
"""
import ctypes as C
import errno
import faulthandler
import glob
import os

import numpy as np
import pytest

import _oracle as O
import spmv_scpa_amd as S

pytestmark = pytest.mark.gpu

TIGHT = 1e-12        # the project's parity bound (of the row scale)
U32 = 2.0 ** -24     # fp32 unit roundoff, round to nearest
PEAK = 8.0e12
LIMIT_S = {"test_f32_is_faster_than_f64_on_the_bandwidth_bound_kernels": 600,
           "test_storage_of_a_generated_4M_x_32_matrix": 300}


@pytest.fixture(autouse=True)
def _time_limit(request):
    name = request.node.name.split("[")[0]
    faulthandler.dump_traceback_later(LIMIT_S.get(name, 240), exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def round32(a):
    with np.errstate(over="ignore"):
        return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _loads(path):
    try:
        S.csr_free(S.io_load_csr(path))
        return True
    except OSError:
        return False


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
#: every .mtx of tests/golden that the loader accepts (the err_* files are
#: the loader's own negative cases)
MTX = sorted(os.path.basename(p)[:-4]
             for p in glob.glob(os.path.join(GOLDEN, "*.mtx")) if _loads(p))

#: tag, kind, M (= N), K, W; None: the generator does not take part
SYNTH = [
    ("banded", S.SYNTH_BANDED, 50_000, 16, 0),
    ("random_narrow", S.SYNTH_RANDOM, 40_000, 32, 512),
    ("random_wide", S.SYNTH_RANDOM, 33_333, 32, 1 << 30),
    ("ragged", S.SYNTH_RAGGED, 20_011, 32, 4096),
    ("powerlaw", S.SYNTH_POWERLAW, 60_000, 3, 1 << 30),
    ("stencil27", S.SYNTH_STENCIL, 40_000, 27, 0),
    # ONE row of 40 000 entries (> 8192: cut into segments, last-arriver sum;
    # a wide hack block in HLL) among rows of 1..12
    ("hub", S.SYNTH_HUB, 40_000, 6, 512),
]
CASES = ["mtx:" + n for n in MTX] + ["synth:" + t[0] for t in SYNTH] + ["hand"]


def hand_made():
    """rows of 0, 1 and 2049 entries (2049: one more than the stream kernel's
    entry budget -- a row with a range of its own)"""
    N = 4096
    lens = [0, 1, 2049, 1, 0, 0, 2049, 1, 1, 0] * 7
    rng = np.random.default_rng(11)
    IRP = np.zeros(len(lens) + 1, np.int32)
    IRP[1:] = np.cumsum(lens)
    JA = np.concatenate([np.sort(rng.choice(N, n, replace=False))
                         for n in lens]).astype(np.int32)
    AS = rng.uniform(-1.0, 1.0, len(JA))
    return len(lens), N, IRP, JA, AS


def case_arrays(case):
    """-> (M, N, IRP, JA, AS, x, generator spec or None)"""
    if case.startswith("mtx:"):
        A = S.io_load_csr(os.path.join(GOLDEN, case[4:] + ".mtx"))
        IRP, JA, AS = (a.copy() for a in S.csr_arrays(A))
        M, N = A.contents.M, A.contents.N
        S.csr_free(A)
        return M, N, IRP, JA, AS, S.vec_random(N), None
    if case == "hand":
        M, N, IRP, JA, AS = hand_made()
        return M, N, IRP, JA, AS, O.synth_x(7, 0, N), None
    tag, kind, M, K, W = next(t for t in SYNTH if t[0] == case[6:])
    N = M
    IRP, JA, AS = O.synth_csr(kind, M, N, K, W, 42)
    return M, N, IRP, JA, AS, O.synth_x(7, 0, N), (kind, M, N, K, W, 0, 42)


class Runner:
    """launches on device-resident x / y; y is NaN before every launch"""

    def __init__(self, M, N, x):
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


def hll_pair(dA):
    """{kernel id: HLL handle of the kernel's layout} by device conversion"""
    cm, rm = dA.to_hll(True), dA.to_hll(False)
    return {k: (cm if S.HLL_KERNEL_COL_MAJOR[k] else rm)
            for k in range(S.NUM_HLL_KERNELS)}, (cm, rm)


def check_rows(y, y_ref, scale, what, rows=None):
    """1e-12 of the row scale on `rows` (a slice; default all); the rows
    outside were not this launch's and must still hold the NaN fill"""
    sl = rows if rows is not None else slice(0, len(y))
    got, want, sc = y[sl], y_ref[sl], scale[sl]
    err = (np.max(np.abs(got - want) / np.maximum(sc, 1e-300))
           if len(got) else 0.0)
    assert err <= TIGHT, (what, err)
    if rows is not None:
        assert np.all(np.isnan(y[:sl.start])) and np.all(np.isnan(y[sl.stop:])), what


def check_every_kernel(run, dA, hll, y_ref, scale, tag):
    """all direct kernel ids, whole matrix and one proper sub-range each"""
    M = run.M
    for k in range(S.NUM_CSR_KERNELS):
        check_rows(run.run(dA, k), y_ref, scale, (tag, "csr", k))
        if M >= 3:
            r0, r1 = M // 3, M - M // 4
            check_rows(run.run(dA, k, rows=(r0, r1)), y_ref, scale,
                       (tag, "csr rows", k), slice(r0, r1))
    for k in range(S.NUM_HLL_KERNELS):
        H = hll[k]
        assert H.value_bytes == 4
        check_rows(run.run(H, k), y_ref, scale, (tag, "hll", k))
        nb = H.num_blocks
        if nb >= 3:
            b0, b1 = nb // 3, nb - nb // 4
            check_rows(run.run(H, k, blocks=(b0, b1)), y_ref, scale,
                       (tag, "hll blocks", k), slice(b0 * 32, min(b1 * 32, M)))


# ------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("case", CASES)
def test_every_kernel_matches_the_oracle_on_the_rounded_matrix(case):
    M, N, IRP, JA, AS, x, spec = case_arrays(case)
    R = round32(AS)
    y_ref = O.csr_spmv(IRP, JA, R, x)
    scale = O.csr_abs_spmv(IRP, JA, R, x)
    A = S.csr_from_arrays(case, M, N, IRP, JA, AS)
    run = Runner(M, N, x)
    made = {"upload_f32": S.CsrDevice.upload(A, values="f32")}
    d64 = S.CsrDevice.upload(A)
    made["to_f32 of an uploaded handle"] = d64.to_f32()
    if spec:
        dG = S.CsrDevice.generate(*spec)
        made["to_f32 of a generated handle"] = dG.to_f32()
        dG.release()
    assert d64.value_bytes == 8
    d64.release()  # the f32 handle does not depend on its source
    for how, d32 in made.items():
        assert d32.value_bytes == 4, how
        assert (d32.M, d32.N, d32.NZ) == (M, N, len(JA)), how
        back = d32.download()
        bI, bJ, bA = S.csr_arrays(back)
        assert np.array_equal(bI, IRP) and np.array_equal(bJ, JA), how
        # bit for bit: round to nearest even on the host AND the device path
        assert np.array_equal(bits(bA), bits(R)), how
        S.csr_free(back)
        hll, handles = hll_pair(d32)
        check_every_kernel(run, d32, hll, y_ref, scale, (case, how))
        for h in handles:
            h.release()
        d32.release()
    # spmv_hll_upload_f32: host HLL in, both layouts
    for cm in (True, False):
        Hh = S.csr_to_hll(A, cm)
        H = S.HllDevice.upload(Hh, cm, values="f32")
        assert H.value_bytes == 4
        for k in range(S.NUM_HLL_KERNELS):
            if S.HLL_KERNEL_COL_MAJOR[k] == cm:
                check_rows(run.run(H, k), y_ref, scale,
                           (case, "hll upload_f32", k))
        H.release()
        S.hll_free(Hh)
    run.free()
    S.csr_free(A)


# ------------------------------------------------------- 2. same order as fp64
@pytest.mark.parametrize("case", CASES)
def test_same_bits_as_the_f64_handle_of_the_rounded_matrix(case):
    M, N, IRP, JA, AS, x, _ = case_arrays(case)
    A = S.csr_from_arrays(case, M, N, IRP, JA, AS)
    AR = S.csr_from_arrays(case + " r", M, N, IRP, JA, round32(AS))
    d32, d64 = S.CsrDevice.upload(A, values="f32"), S.CsrDevice.upload(AR)
    run = Runner(M, N, x)
    h32, k32 = hll_pair(d32)
    h64, k64 = hll_pair(d64)
    csr_opts = {0: [{}], 1: [{}], 3: [{}],
                2: [{}, dict(group=4), dict(group=32), dict(variant=512),
                    dict(waves_per_block=4, variant=1)],
                # the stream kernel: 16-byte loads / 4- and 8-byte loads only
                4: [{}, dict(variant=16), dict(variant=32), dict(variant=64)]}
    for k, optlist in csr_opts.items():
        for kw in optlist:
            a = run.run(d32, k, **kw)
            assert np.array_equal(bits(a), bits(run.run(d64, k, **kw))), (
                case, "csr", k, kw)
            assert np.array_equal(bits(a), bits(run.run(d32, k, **kw))), (
                case, "csr twice", k, kw)
    for k in range(S.NUM_HLL_KERNELS):
        for kw in ({}, dict(waves_per_block=2), dict(waves_per_block=16)):
            a = run.run(h32[k], k, **kw)
            assert np.array_equal(bits(a), bits(run.run(h64[k], k, **kw))), (
                case, "hll", k, kw)
            assert np.array_equal(bits(a), bits(run.run(h32[k], k, **kw))), (
                case, "hll twice", k, kw)
    for h in k32 + k64 + (d32, d64):
        h.release()
    run.free()
    S.csr_free(A)
    S.csr_free(AR)


# ------------------------------------------------------- 3. accuracy contract
@pytest.mark.parametrize("W", [512, 1 << 30], ids=["narrow", "wide"])
def test_accuracy_against_the_unrounded_matrix(W):
    M = N = 40_000
    IRP, JA, AS = O.synth_csr(S.SYNTH_RANDOM, M, N, 32, W, 42)
    x = O.synth_x(7, 0, N)
    y_true = O.csr_spmv(IRP, JA, AS, x)
    scale = O.csr_abs_spmv(IRP, JA, AS, x)
    bound = U32 * scale + TIGHT * scale
    A = S.csr_from_arrays("acc", M, N, IRP, JA, AS)
    d32 = S.CsrDevice.upload(A, values="f32")
    hll, handles = hll_pair(d32)
    run = Runner(M, N, x)
    worst = 0.0
    for m, k, tag in ([(d32, k, "csr") for k in range(S.NUM_CSR_KERNELS)] +
                      [(hll[k], k, "hll") for k in range(S.NUM_HLL_KERNELS)]):
        err = np.abs(run.run(m, k) - y_true)
        worst = max(worst, float(np.max(err / np.maximum(scale, 1e-300))))
        assert np.all(err <= bound), (tag, k, float(np.max(err - bound)))
    print("worst |y_f32 - y| / scale = %.3e (bound %.3e)" % (worst, U32 + TIGHT))
    assert worst > 0.0  # the values really were rounded
    for h in handles + (d32,):
        h.release()
    run.free()
    S.csr_free(A)


# ------------------------------------------------------------ 4. edge values
def _tiny(rows, N=8):
    """rows: list of [(col, value), ...] -> (M, N, IRP, JA, AS)"""
    IRP = np.zeros(len(rows) + 1, np.int32)
    IRP[1:] = np.cumsum([len(r) for r in rows])
    JA = np.array([c for r in rows for c, _ in r], np.int32)
    AS = np.array([v for r in rows for _, v in r], np.float64)
    return len(rows), N, IRP, JA, AS


def _every_kernel_y(M, N, IRP, JA, AS, x):
    """y of all nine direct kernels on f32 handles made both ways"""
    A = S.csr_from_arrays("tiny", M, N, IRP, JA, AS)
    d64 = S.CsrDevice.upload(A)
    run = Runner(M, N, x)
    out = []
    for how, d32 in (("upload_f32", S.CsrDevice.upload(A, values="f32")),
                     ("to_f32", d64.to_f32())):
        hll, handles = hll_pair(d32)
        for k in range(S.NUM_CSR_KERNELS):
            out.append(((how, "csr", k), run.run(d32, k)))
        for k in range(S.NUM_HLL_KERNELS):
            out.append(((how, "hll", k), run.run(hll[k], k)))
        back = d32.download()
        out.append(((how, "download"), S.csr_arrays(back)[2].copy()))
        S.csr_free(back)
        for h in handles + (d32,):
            h.release()
    d64.release()
    run.free()
    S.csr_free(A)
    return out


def test_subnormals_are_kept_not_flushed():
    tiny = float(np.float32(1e-40))
    assert 0.0 < tiny < float(np.finfo(np.float32).tiny) and tiny != 1e-40
    M, N, IRP, JA, AS = _tiny([[(2, 1e-40)], [(1, 0.5)], [(3, -1e-40)]])
    x = np.array([1.0, 2.0, 3.0, 5.0, 0.0, 0.0, 0.0, 0.0])
    want = np.array([tiny * 3.0, 1.0, -tiny * 5.0])
    for what, got in _every_kernel_y(M, N, IRP, JA, AS, x):
        if what[-1] == "download":
            assert np.array_equal(bits(got), bits(round32(AS))), what
        else:
            assert np.array_equal(bits(got), bits(want)), (what, got)


def test_a_finite_value_that_overflows_fp32_is_erange_and_leaks_nothing():
    M, N, IRP, JA, AS = _tiny([[(0, 1.0)], [(1, 1e39)], [(2, 2.0)]] * 20)
    A = S.csr_from_arrays("over", M, N, IRP, JA, AS)
    d64 = S.CsrDevice.upload(A)
    live = S._lib.spmv_live_handles()
    with pytest.raises(OSError) as ei:
        S.CsrDevice.upload(A, values="f32")
    assert ei.value.errno == errno.ERANGE
    with pytest.raises(OSError) as ei:
        d64.to_f32()
    assert ei.value.errno == errno.ERANGE
    for cm in (True, False):
        Hh = S.csr_to_hll(A, cm)
        with pytest.raises(OSError) as ei:
            S.HllDevice.upload(Hh, cm, values="f32")
        assert ei.value.errno == errno.ERANGE
        S.hll_free(Hh)
    assert S._lib.spmv_live_handles() == live
    assert S.live_objects() == [d64]
    # every refusal of to_f32 leaves *out NULL and no handle behind: the one
    # that comes after the result was allocated, a handle that is none, an
    # f32 operand, a released source
    As = S.csr_from_arrays(
        "small", *_tiny([[(0, 1.0)], [(1, 2.0)], [(2, 3.0)]] * 20))
    small = S.CsrDevice.upload(As)
    narrow = small.to_f32()
    try:
        S.set_panel_schedule("chain")
        small.build_panels(0)
        small.release_source()
    finally:
        S.set_panel_schedule("sweep")
    junk = C.cast(C.create_string_buffer(512), C.c_void_p)
    before = S._lib.spmv_live_handles()
    for err, h in ((errno.ERANGE, d64.h), (errno.EBADF, junk),
                   (errno.EINVAL, narrow.h), (errno.ENODATA, small.h)):
        out = C.c_void_p(1234)
        assert S._lib.spmv_csr_to_f32(h, C.byref(out)) == -err, err
        assert out.value is None
        assert S._lib.spmv_live_handles() == before
    narrow.release()
    small.release()
    S.csr_free(As)
    # the largest finite fp32 and a value that rounds DOWN to it still fit
    AS2 = AS.copy()
    AS2[AS2 == 1e39] = float(np.finfo(np.float32).max) * (1.0 + 2.0 ** -26)
    A2 = S.csr_from_arrays("fits", M, N, IRP, JA, AS2)
    d = S.CsrDevice.upload(A2, values="f32")
    d.release()
    d64.release()
    S.csr_free(A)
    S.csr_free(A2)


def test_nan_and_inf_pass_through_and_zero_rows_give_exactly_zero():
    inf, nan = float("inf"), float("nan")
    rows = [[(0, nan), (1, 1.0)], [(1, inf)], [(2, -inf), (3, 1.0)], [],
            [(4, 0.0), (5, 0.0)], [(1, 0.25), (2, 0.5)]]
    rows += [[] for _ in range(40)] + [[(0, 0.0)]]
    M, N, IRP, JA, AS = _tiny(rows)
    x = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0])
    for what, got in _every_kernel_y(M, N, IRP, JA, AS, x):
        if what[-1] == "download":
            assert np.array_equal(bits(got), bits(AS)), what  # all exact in fp32
            continue
        assert np.isnan(got[0]), what
        assert got[1] == inf and got[2] == -inf, (what, got[:3])
        assert got[5] == 2.0, what
        rest = np.concatenate([got[3:5], got[6:]])
        assert np.array_equal(bits(np.abs(rest)), bits(np.zeros(len(rest)))), what


# ----------------------------------------------------------------- 5. storage
def test_storage_of_a_generated_4M_x_32_matrix():
    # the one-off allocations of a first use (code objects, the runtime's own
    # pools) are not the matrix's: made before the first reading
    w = S.CsrDevice.generate(S.SYNTH_BANDED, 4096, 4096, 32, 0, 0, 42)
    w32 = w.to_f32()
    w32.to_hll(True).release()
    w32.release()
    w.release()
    S.device_sync()
    M = N = 4_000_000
    free0 = S.dev_mem_info()[0]
    d64 = S.CsrDevice.generate(S.SYNTH_BANDED, M, N, 32, 0, 0, 42)
    free1 = S.dev_mem_info()[0]
    d32 = d64.to_f32()
    free2 = S.dev_mem_info()[0]
    NZ = d64.NZ
    assert NZ == 32 * M and d32.NZ == NZ
    assert d32.value_bytes == 4 and d64.value_bytes == 8
    assert d32.algorithmic_bytes == 8 * NZ + 4 * (M + 1) + 8 * M + 8 * N
    assert d32.kernel_bytes(4) == d32.algorithmic_bytes
    assert d64.algorithmic_bytes == 12 * NZ + 4 * (M + 1) + 8 * M + 8 * N
    H = d32.to_hll(True)
    assert H.value_bytes == 4
    assert H.algorithmic_bytes == (8 * H.slots + 12 * H.num_blocks + 8 * M
                                   + 8 * N)
    assert H.kernel_bytes(1) == H.algorithmic_bytes
    H.release()
    drop64, drop32 = free0 - free1, free1 - free2
    print("HBM taken: f64 handle %d B, f32 handle %d B, difference %d B "
          "(4 NZ = %d)" % (drop64, drop32, drop64 - drop32, 4 * NZ))
    assert drop64 - drop32 >= 0.9 * 4 * NZ, (drop64, drop32)
    d32.release()
    d64.release()
    S.device_sync()
    # nothing leaked.  The runtime's allocator keeps some freed blocks for
    # itself: free memory moves by ~100 MB either way without any leak
    # (tests/test_gpu_mgpu.py holds its reload test to 256 MiB for that
    # reason); a leaked f32 value array alone would be 4 NZ = 512 MB, a
    # leaked handle 1.1 GB (f32) or 1.6 GB (f64)
    back = free0 - S.dev_mem_info()[0]
    print("free memory after release: %d B below the start" % back)
    assert abs(back) <= (256 << 20), back


# ----------------------------------------------------------------- 6. surface
def test_blocked_path_is_refused_and_autotune_stays_on_the_direct_kernels():
    M = N = 200_000
    spec = (S.SYNTH_RANDOM, M, N, 32, 2 * N, 0, 42)  # columns anywhere: the
    IRP, JA, AS = O.synth_csr(*spec[:5], 42)         # blocked path's matrix
    x = O.synth_x(7, 0, N)
    R = round32(AS)
    y_ref, scale = O.csr_spmv(IRP, JA, R, x), O.csr_abs_spmv(IRP, JA, R, x)
    dG = S.CsrDevice.generate(*spec)
    d32 = dG.to_f32()
    dG.release()
    run = Runner(M, N, x)
    for m, panels, nk in ((d32, S.CSR_KERNEL_PANELS, S.NUM_CSR_KERNELS),
                          (d32.to_hll(True), S.HLL_KERNEL_PANELS,
                           S.NUM_HLL_KERNELS)):
        with pytest.raises(OSError) as ei:
            m.build_panels()
        assert ei.value.errno == errno.ENOTSUP
        with pytest.raises(OSError) as ei:
            m.build_panels(0, "chain", 4096)
        assert ei.value.errno == errno.ENOTSUP
        assert m.panels_info() is None
        with pytest.raises(OSError) as ei:
            m.launch(panels, run.x.ptr, run.y.ptr)
        assert ei.value.errno == errno.EINVAL
        best, ms = m.autotune(run.x.ptr, run.y.ptr, allow_panels=True)
        assert 0 <= best < nk and ms > 0.0, (best, ms)
        log = m.tune_log()
        assert "not available for f32 values" in log, log
        assert m.tune_times()[panels] == 0.0 and m.panels_info() is None
        check_rows(run.run(m, best), y_ref, scale, ("autotune pick", best))
        m.release()
    run.free()


def test_a_captured_launch_replays_with_a_changed_x():
    M = N = 100_000
    spec = (S.SYNTH_HUB, M, N, 6, 4096, 0, 42)  # side launch + arrival counters
    IRP, JA, AS = O.synth_csr(*spec[:5], 42)
    R = round32(AS)
    dG = S.CsrDevice.generate(*spec)
    d32 = dG.to_f32()
    dG.release()
    hll, handles = hll_pair(d32)
    x, y = S.DevBuffer(N * 8), S.DevBuffer(M * 8)
    side = S.Stream()
    cases = ([(d32, k) for k in range(S.NUM_CSR_KERNELS)] +
             [(hll[k], k) for k in range(S.NUM_HLL_KERNELS)])
    for m, k in cases:
        S.dev_fill_synth(x.ptr, N, 7, 0, side.ptr)
        m.launch(k, x.ptr, y.ptr, stream=side.ptr)  # eagerly once, first
        side.sync()
        with side.capture() as g:
            m.launch(k, x.ptr, y.ptr, stream=side.ptr)
        for seed in (7, 8):  # the graph reads x where it lives
            S.dev_fill_synth(x.ptr, N, seed, 0, side.ptr)
            S._check(S._lib.spmv_dev_memset(y.ptr, 0xFF, M * 8, side.ptr),
                     "spmv_dev_memset")
            g.launch(side.ptr)
            side.sync()
            xs = O.synth_x(seed, 0, N)
            check_rows(y.to_numpy(np.float64, M), O.csr_spmv(IRP, JA, R, xs),
                       O.csr_abs_spmv(IRP, JA, R, xs),
                       ("replay", type(m).__name__, k, seed))
        g.destroy()
    for h in handles + (d32,):
        h.release()
    x.free()
    y.free()


# ------------------------------------------------------------------- 7. speed
def test_f32_is_faster_than_f64_on_the_bandwidth_bound_kernels(request):
    """banded 10M x 32, the bench's own size (3.8 GB of matrix: far beyond the
    Infinity Cache, no flush).  The f64 handle of the same matrix in the same
    process is the yardstick: f64 and f32 are timed in turns (two rounds of
    time(warmup=3, iters=20) each, alternating), median over a handle's
    launches.  Asserted: t_f32 < t_f64, nothing else -- by bytes alone the
    ratio would be 0.68; what is measured goes to the terminal summary and to
    profiles/f32_values.md."""
    M = N = 10_000_000
    x, y = S.DevBuffer(N * 8), S.DevBuffer(M * 8)
    S.dev_fill_synth(x.ptr, N, 7)
    d64 = S.CsrDevice.generate(S.SYNTH_BANDED, M, N, 32, 0, 0, 42)
    d32 = d64.to_f32()
    h64, h32 = d64.to_hll(True), d32.to_hll(True)
    slower = []
    for tag, a, b, k in (("csr stream", d64, d32, 4),
                         ("csr subwave_row", d64, d32, 2),
                         ("hll threads_col_major", h64, h32, 1)):
        ms = {8: [], 4: []}
        for _ in range(2):
            for m in (a, b):
                ms[m.value_bytes] += list(m.time(k, x.ptr, y.ptr, 3, 20))
        t64, t32 = float(np.median(ms[8])), float(np.median(ms[4]))
        f64 = a.kernel_bytes(k) / (t64 * 1e-3) / PEAK
        f32 = b.kernel_bytes(k) / (t32 * 1e-3) / PEAK
        line = ("f32 values, banded10M %-22s f64 %.4f ms (%.3f of 8 TB/s)  "
                "f32 %.4f ms (%.3f)  ratio %.3f (bytes: %.3f)"
                % (tag, t64, f64, t32, f32, t32 / t64,
                   b.kernel_bytes(k) / a.kernel_bytes(k)))
        print(line)
        getattr(request.config, "_summary_lines", []).append(line)
        if not t32 < t64:
            slower.append((tag, t32, t64))
    for h in (h64, h32, d32, d64):
        h.release()
    x.free()
    y.free()
    assert not slower, slower
