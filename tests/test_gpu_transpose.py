"""Transposition of CSR handles on the GPU (spmv_csr_transpose,
spmv_csr_symmetry; spmv_engine.h).

The result is defined to the byte (the stable counting sort of the entries, in
stored order, by column: tests/_transpose.py reference), so everything is
compared through download() as integer arrays and uint64 views of the values:
THERE IS NO TOLERANCE here, except where a product of T is checked against
the CPU oracle's product of the downloaded T (the bound of
tests/test_gpu_parity.py) and where a solve has to reach its tol.

The shapes are those of tests/_transpose.py (gpu_shapes), which the CPU test
holds to what they are for.  No test provokes a fault: every error case is an
argument check that returns before any launch.  Every test runs under a time
limit of its own (LIMIT_S): a test that exceeds it ends the whole process, so
nothing else is started on the device.
"""
import ctypes as C
import errno
import faulthandler
import glob
import os

import numpy as np
import pytest

import _bicgstab as BI
import _cg as G
import _oracle as O
import _transpose as TR
import spmv_scpa_amd as S
from test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

LIMIT_S = 240
TILE = S.transpose_plan(1, 1)["tile"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def shapes():
    return TR.gpu_shapes(TILE)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def upload(mat, values="f64"):
    M, N, IRP, JA, AS = mat
    A = S.csr_from_arrays("t", M, N, IRP, JA, AS)
    d = S.CsrDevice.upload(A, values=values)
    S.csr_free(A)
    return d


def arrays(d):
    """(IRP, JA, AS) of a handle, copied out of its download"""
    p = d.download()
    assert (p.contents.M, p.contents.N, p.contents.NZ) == (d.M, d.N, d.NZ)
    out = tuple(a.copy() for a in S.csr_arrays(p))
    S.csr_free(p)
    return out


def same(got, want):
    return (got[0].dtype == got[1].dtype == np.int32
            and np.array_equal(got[0], want[0])
            and np.array_equal(got[1], want[1])
            and np.array_equal(bits(got[2]), bits(want[2])))


def check_transpose(mat, values="f64", d=None):
    """upload, transpose, compare with the reference; -> (d, T, want)"""
    M, N, IRP, JA, AS = mat
    d = d or upload(mat, values)
    live = S._lib.spmv_live_handles()
    T = d.transpose()
    assert S._lib.spmv_live_handles() == live + 1
    assert (T.M, T.N, T.NZ) == (N, M, len(JA))
    assert T.value_bytes == d.value_bytes
    src = arrays(d)  # the f32 handle's values, widened
    want = TR.reference(IRP, JA, src[2], N)
    got = arrays(T)
    assert same(got, want)
    return d, T, want


# ------------------------------------------------------------ 1. the bytes
@pytest.mark.parametrize("nz", TR.NZ_EDGES(TILE))
def test_nz_at_the_strip_wavefront_and_tile_edges(shapes, nz):
    mat = shapes["nz=%d" % nz]
    assert len(mat[3]) == nz and mat[1] == 300
    d, T, _ = check_transpose(mat)
    T.release()
    d.release()


@pytest.mark.parametrize("n", TR.N_EDGES)
def test_n_at_the_digit_edges(shapes, n):
    mat = shapes["n=%d" % n]
    assert mat[1] == n and mat[0] == 50
    d, T, want = check_transpose(mat)
    assert len(want[0]) == n + 1  # all of T's (mostly empty) rows
    T.release()
    d.release()


@pytest.fixture(scope="module")
def hub(shapes):
    mat = shapes["hub"]
    d, T, want = check_transpose(mat)
    yield mat, d, T, want
    T.release()
    d.release()


def test_a_hub_column_keeps_its_rows_in_order_across_the_tiles(hub):
    (M, N, IRP, JA, AS), d, T, want = hub
    beg, end = want[0][7], want[0][8]
    assert end - beg >= M == 70000  # one bucket across every tile
    rows = want[1][beg:end]
    assert np.all(np.diff(rows) >= 0) and len(np.unique(rows)) == M


def test_every_direct_kernel_runs_the_transposed_hub(hub):
    """T holds a row of 70 000 entries, beyond the stream kernel's long-row
    threshold: finish_csr_handle's segment tables.  Kernel ids 0, 1, 3, 4 and
    the sub-wave kernel at its five group sizes, against the CPU oracle's
    product of the DOWNLOADED T at the bound of the parity tests"""
    (M, N, IRP, JA, AS), d, T, want = hub
    tI, tJ, tA = arrays(T)
    assert np.max(np.diff(tI)) >= 70000 > 8192
    x = O.synth_x(7, 0, T.N)
    y_ref = O.csr_spmv(tI, tJ, tA, x)
    scale = O.csr_abs_spmv(tI, tJ, tA, x)
    d_x, d_y = S.DevBuffer.from_numpy(x), S.DevBuffer(T.M * 8)
    runs = [(k, 0) for k in (0, 1, 3, 4)] + [(2, g) for g in (2, 4, 8, 16, 32)]
    assert len(runs) == 9
    for kernel, group in runs:
        S._lib.spmv_dev_memset(d_y.ptr, 0xFF, T.M * 8, None)
        T.launch(kernel, d_x.ptr, d_y.ptr, group=group)
        S.stream_sync()
        assert_parity(d_y.to_numpy(np.float64, T.M), y_ref, scale,
                      ("transposed hub", kernel, group))
    # ... and the four HLL kernels on the handles made of T (a hack block
    # 70 000 columns wide)
    for kernel in range(S.NUM_HLL_KERNELS):
        H = T.to_hll(S.HLL_KERNEL_COL_MAJOR[kernel])
        S._lib.spmv_dev_memset(d_y.ptr, 0xFF, T.M * 8, None)
        H.launch(kernel, d_x.ptr, d_y.ptr)
        S.stream_sync()
        assert_parity(d_y.to_numpy(np.float64, T.M), y_ref, scale,
                      ("transposed hub, hll", kernel))
        H.release()
    d_x.free()
    d_y.free()


def test_three_transpositions_of_the_hub_give_identical_bytes(hub):
    mat, d, T, want = hub
    for _ in range(3):
        again = d.transpose()
        assert same(arrays(again), want)
        again.release()


def loadable_golden():
    out = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, "*.mtx"))):
        try:
            A = S.io_load_csr(path)
        except OSError:
            continue  # the err_*.mtx files: the loader refuses them
        out.append((os.path.basename(path), A))
    return out


def test_golden_matrices_in_file_order_and_stored_duplicates(shapes):
    loaded = loadable_golden()
    assert len(loaded) >= 10
    unsorted = 0
    for name, A in loaded:
        M, N = A.contents.M, A.contents.N
        IRP, JA, AS = (v.copy() for v in S.csr_arrays(A))
        S.csr_free(A)
        rows = np.repeat(np.arange(M), np.diff(IRP))
        unsorted += bool(np.any((np.diff(JA) < 0) & (np.diff(rows) == 0)))
        d, T, _ = check_transpose((M, N, IRP, JA, AS))
        T.release()
        d.release()
    assert unsorted > 0  # the loader keeps file order
    mat = shapes["duplicates"]
    d, T, want = check_transpose(mat)
    # (1, 4) three times: row 4 of T holds source row 1 with 10, 20, 30
    assert want[1][want[0][4]:want[0][5]].tolist() == [1, 1, 1]
    assert want[2][want[0][4]:want[0][5]].tolist() == [10.0, 20.0, 30.0]
    T.release()
    d.release()


def test_special_values_arrive_with_their_bits():
    M, N, IRP, JA, AS = TR.random_nz(500, N=37, M=23)
    AS = AS.copy()
    special = np.array([0x7FF8_0000_DEAD_BEEF, 0xFFF0_0000_0000_0001,
                        0x7FF0_0000_0000_0000, 0xFFF0_0000_0000_0000,
                        0x8000_0000_0000_0000, 0x0000_0000_0000_0001,
                        0x800F_FFFF_FFFF_FFFF, 0], np.uint64)
    at = np.arange(len(special)) * 59 + 3
    bits(AS)[at] = special  # a quiet and a signalling NaN with payloads, ...
    assert np.isnan(AS[at[0]]) and np.isnan(AS[at[1]])
    d, T, want = check_transpose((M, N, IRP, JA, AS))
    got = arrays(T)[2]
    assert sorted(bits(got)[~np.isfinite(got) | (got == 0)
                            | (np.abs(got) < 1e-300)].tolist()) == \
        sorted(special.tolist())
    T.release()
    d.release()
    # f32 handles, made both ways: +-inf, -0.0, the largest finite value
    AS32 = TR.random_nz(500, N=37, M=23)[4]
    fmax = float(np.finfo(np.float32).max)
    AS32[at[:6]] = [np.inf, -np.inf, -0.0, fmax, -fmax, 0.0]
    mat = (M, N, IRP, JA, AS32)
    d64 = upload(mat)
    for d in (upload(mat, "f32"), d64.to_f32()):
        assert d.value_bytes == 4
        _, T, want = check_transpose(mat, d=d)
        assert T.value_bytes == 4
        got = arrays(T)[2]
        assert np.array_equal(got, got.astype(np.float32))  # fp32 values
        assert np.count_nonzero(np.isinf(got)) == 2
        assert np.count_nonzero(bits(got) == 0x8000_0000_0000_0000) == 1
        assert np.count_nonzero(np.abs(got) == fmax) == 2
        T.release()
        d.release()
    d64.release()


@pytest.mark.parametrize("name", list(TR.plain_shapes()))
def test_empty_thin_and_rectangular_shapes(shapes, name):
    mat = shapes[name]
    d, T, want = check_transpose(mat)
    if len(mat[3]) == 0:
        tI = arrays(T)[0]
        assert len(tI) == mat[1] + 1 and not tI.any()  # irp all zero
    T.release()
    d.release()


def test_the_round_trip_is_the_stable_row_sort():
    mat = TR.random_nz(3 * TILE + 17, N=300, M=41)
    M, N, IRP, JA, AS = mat
    d = upload(mat)
    T = d.transpose()
    back = T.transpose()
    assert (back.M, back.N, back.NZ) == (M, N, len(JA))
    want = TR.row_sorted(IRP, JA, AS)
    assert not np.array_equal(want[1], JA)  # the rows were not sorted
    assert same(arrays(back), want)
    for h in (back, T, d):
        h.release()
    # rows already sorted: A itself, byte for byte
    g = S.CsrDevice.generate(S.SYNTH_BANDED, 30011, 30011, 16, 0)
    T = g.transpose()
    back = T.transpose()
    assert same(arrays(back), arrays(g))
    for h in (back, T, g):
        h.release()


# ------------------------------------------------- 2. an ordinary handle
def test_the_result_composes_with_the_rest_of_the_library():
    mat = TR.random_nz(3 * TILE + 17, N=300, M=41)
    d, T, want = check_transpose(mat)
    tI, tJ, tA = want
    x = O.synth_x(7, 0, T.N)
    y_ref = O.csr_spmv(tI, tJ, tA, x)
    scale = O.csr_abs_spmv(tI, tJ, tA, x)
    d_x, d_y = S.DevBuffer.from_numpy(x), S.DevBuffer(T.M * 8 * 3)
    # to_hll
    H = T.to_hll(True)
    H.launch(1, d_x.ptr, d_y.ptr)
    S.stream_sync()
    assert_parity(d_y.to_numpy(np.float64, T.M), y_ref, scale, "to_hll")
    H.release()
    # launch_multi, k = 3: column j has the bits of launch(2) on X[:, j]
    X = np.stack([x, 2.0 * x, -x], axis=1)
    d_X = S.DevBuffer.from_numpy(X)
    T.launch_multi(d_X.ptr, d_y.ptr, 3)
    S.stream_sync()
    Y = d_y.to_numpy(np.float64, T.M * 3).reshape(T.M, 3)
    for j, f in enumerate((1.0, 2.0, -1.0)):
        assert_parity(Y[:, j], f * y_ref, scale * abs(f), ("multi", j))
    # to_f32: the pattern of T, its values rounded
    T32 = T.to_f32()
    got = arrays(T32)
    assert np.array_equal(got[0], tI) and np.array_equal(got[1], tJ)
    assert np.array_equal(got[2], tA.astype(np.float32).astype(np.float64))
    T32.release()
    # autotune
    kernel, ms = T.autotune(d_x.ptr, d_y.ptr)
    assert 0 <= kernel < S.NUM_CSR_KERNELS_ALL and ms > 0
    T.launch(kernel, d_x.ptr, d_y.ptr)
    S.stream_sync()
    assert_parity(d_y.to_numpy(np.float64, T.M), y_ref, scale, "autotuned")
    for b in (d_x, d_y, d_X):
        b.free()
    T.release()
    d.release()


def test_diag_and_bicgstab_on_a_transposed_nonsymmetric_system():
    Mc, IRP, JA, AS = BI.convdiff(37, 29, 0.5, 0.5)
    d, T, want = check_transpose((Mc, Mc, IRP, JA, AS))
    # one stored diagonal entry per row: the same sum on both, bit for bit
    dd, dt = S.DevBuffer(Mc * 8), S.DevBuffer(Mc * 8)
    d.diag(dd.ptr)
    T.diag(dt.ptr)
    S.stream_sync()
    got = dt.to_numpy(np.float64, Mc)
    assert np.array_equal(bits(got), bits(dd.to_numpy(np.float64, Mc)))
    assert np.all(got == 4.5)
    # A^T X = B
    tol = 1e-8
    B, X0 = G.common_inputs(Mc, 2)
    d_B, d_X = S.DevBuffer.from_numpy(B), S.DevBuffer.from_numpy(X0)
    rec = T.bicgstab(d_B.ptr, d_X.ptr, 2, tol=tol, maxit=200)
    X = d_X.to_numpy(np.float64, Mc * 2).reshape(Mc, 2)
    res = G.true_residual(want[0], want[1], want[2], O.csr_spmv, B, X)
    print("bicgstab on the transpose:", rec, "true residual", res)
    assert [r.status for r in rec] == [0, 0]
    assert all(r.rr <= tol * tol * r.bb for r in rec)
    assert np.all(res <= 2 * tol)  # the sanity line of test_gpu_cg
    assert not np.array_equal(want[2], AS)  # nonsymmetric: T is not A
    for b in (dd, dt, d_B, d_X):
        b.free()
    T.release()
    d.release()


# --------------------------------------------------------- 3. ownership
def test_ownership_and_error_paths():
    mat = TR.random_nz(TILE + 1, N=300, M=41)
    M, N, IRP, JA, AS = mat
    d = upload(mat)
    before = arrays(d)
    live = S._lib.spmv_live_handles()
    out = C.c_void_p(1234)
    junk = C.cast(C.create_string_buffer(512), C.c_void_p)
    # every error is an argument check: nothing is created, nothing launched
    assert S._lib.spmv_csr_transpose(None, C.byref(out)) == -errno.EINVAL
    assert S._lib.spmv_csr_transpose(d.h, None) == -errno.EINVAL
    assert S._lib.spmv_live_handles() == live
    assert S._lib.spmv_csr_transpose(junk, C.byref(out)) == -errno.EBADF
    assert out.value is None and S._lib.spmv_live_handles() == live
    sym = C.c_int(7)
    assert S._lib.spmv_csr_symmetry(junk, C.byref(sym)) == -errno.EBADF
    assert sym.value == 0 and S._lib.spmv_live_handles() == live
    # ... but for a column outside [0, N), found after T was allocated
    far = upload((3, 3, np.array([0, 1, 3, 4], np.int32),
                  np.array([0, 1, 5, 2], np.int32), np.ones(4)))
    out = C.c_void_p(1234)
    assert S._lib.spmv_csr_transpose(far.h, C.byref(out)) == -errno.EDOM
    assert out.value is None and S._lib.spmv_live_handles() == live + 1
    far.release()
    T = d.transpose()
    assert S._lib.spmv_live_handles() == live + 1
    assert same(arrays(d), before)  # A is unchanged
    # T owns its arrays: A may go
    want = TR.reference(IRP, JA, AS, N)
    d.release()
    assert S._lib.spmv_live_handles() == live
    x = O.synth_x(7, 0, T.N)
    d_x, d_y = S.DevBuffer.from_numpy(x), S.DevBuffer(T.M * 8)
    T.launch(2, d_x.ptr, d_y.ptr)
    S.stream_sync()
    assert_parity(d_y.to_numpy(np.float64, T.M), O.csr_spmv(*want, x),
                  O.csr_abs_spmv(*want, x), "after the source was released")
    assert same(arrays(T), want)
    # a released handle
    with pytest.raises(OSError) as ei:
        d.transpose()
    assert ei.value.errno == errno.EINVAL
    # after release_source: -ENODATA, and nothing is created
    try:
        S.set_panel_schedule("chain")
        T.build_panels(0)
        T.release_source()
    finally:
        S.set_panel_schedule("sweep")
    live = S._lib.spmv_live_handles()
    for call in (T.transpose, T.symmetry):
        with pytest.raises(OSError) as ei:
            call()
        assert ei.value.errno == errno.ENODATA
        assert S._lib.spmv_live_handles() == live
    T.release()
    d_x.free()
    d_y.free()


# ---------------------------------------------------------- 4. symmetry
def test_symmetry_of_a_laplacian_and_what_breaks_it():
    M, IRP, JA, AS = G.lap2d(37, 29, 0.5)
    live = S._lib.spmv_live_handles()

    def sym(IRP, JA, AS, N=M, values="f64", rows=M):
        d = upload((rows, N, IRP, JA, AS), values)
        got = d.symmetry()
        d.release()
        assert S._lib.spmv_live_handles() == live  # T and C were released
        return got

    assert sym(IRP, JA, AS) == S.SYM_VALUES == 2
    assert sym(IRP, JA, AS, values="f32") == S.SYM_VALUES
    k = int(IRP[100]) + 1  # an off-diagonal of row 100
    assert JA[k] != 100
    changed = AS.copy()
    changed[k] = -1.5
    assert sym(IRP, JA, changed) == S.SYM_PATTERN == 1
    lens = np.diff(IRP)
    lens[100] -= 1
    assert sym(TR.irp_of(lens), np.delete(JA, k), np.delete(AS, k)) == \
        S.SYM_NONE == 0
    # rectangular: one more column, the same entries
    assert sym(IRP, JA, AS, N=M + 1) == S.SYM_NONE
    # a NaN on the diagonal equals nothing, itself included
    diag = np.flatnonzero(JA == np.repeat(np.arange(M), np.diff(IRP)))[5]
    nan = AS.copy()
    nan[diag] = np.nan
    assert sym(IRP, JA, nan) == S.SYM_PATTERN
    # -0.0 == 0.0
    zero = AS.copy()
    mirror = np.flatnonzero((JA == 100) & (np.repeat(np.arange(M),
                                                     np.diff(IRP)) == JA[k]))
    assert len(mirror) == 1
    zero[k], zero[mirror[0]] = 0.0, -0.0
    assert sym(IRP, JA, zero) == S.SYM_VALUES
