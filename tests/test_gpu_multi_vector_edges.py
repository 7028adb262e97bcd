"""Y = A X launches (spmv_*_launch_multi) where tests/test_gpu_multi_vector.py
does not reach: the grouped workgroup order with its padded grid (A), every
boundary between the main kernels and their side kernels (B), and a
non-finite X (C).

No new tolerance: a result is either the bits of a launch the library already
has on the same handle, or within the project's parity bound (1e-12 of the row
scale sum_c |a_rc x_c|) of the CPU oracle, applied to the rounded values on an
f32 handle.  With a non-finite X only the CLASS of an entry of Y (NaN, +inf,
-inf, finite) is compared with the oracle's -- it does not depend on the order
of a sum as long as no finite sum overflows -- and the finite entries are held
to the bound.

Y is filled with 0xFF bytes before every launch.

Every test runs under a time limit of its own (LIMIT_S): a test that exceeds
it ends the whole process, so nothing else is started on the device.
"""
import faulthandler

import numpy as np
import pytest

import _oracle as O
import spmv_scpa_amd as S
from test_gpu_f32_values import case_arrays, round32
from test_gpu_multi_vector import (FILL, MAXK, PAST, SINGLE, TIGHT, Bench,
                                   bits, check_bits_and_bound, exact_rows,
                                   handles, only_k_columns_written,
                                   oracle_columns, x_columns)

pytestmark = pytest.mark.gpu

LIMIT_S = {}


@pytest.fixture(autouse=True)
def _time_limit(request):
    name = request.node.name.split("[")[0]
    faulthandler.dump_traceback_later(LIMIT_S.get(name, 240), exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


# ------------------------------------------------------------ A. grouped order
# engine.hip gives a CSR handle   d->order = M >= 2000000 ? 2 : 1;
#           and an HLL handle     d->order = nb >= 65536 ? 2 : 0;
# (only autotune changes it afterwards, launch_multi takes no variant).  Order
# 2 is xcd_grouped: the grid is padded to a multiple of 8 x 32 workgroups and
# what the surplus workgroups would touch is masked (row < M, t / 32 >= nb).
BIG_M = 2_100_003    # 65 626 hack blocks, the last of 3 rows
BIG_SPEC = (S.SYNTH_RAGGED, BIG_M, BIG_M, 6, 4096)  # rows of 5..7 entries


@pytest.fixture(scope="module")
def big():
    """-> (IRP, JA, AS, Xc, oracle): the host arrays of the big matrix and
    oracle(values) -> (y_ref, scale) per column, each computed once for the
    module and dropped with it"""
    IRP, JA, AS = O.synth_csr(*BIG_SPEC, 42)
    Xc = x_columns(BIG_M)
    for a in (IRP, JA, AS, Xc):
        a.setflags(write=False)
    refs = {}

    def oracle(values):
        if values not in refs:
            refs[values] = oracle_columns(
                IRP, JA, round32(AS) if values == "f32" else AS, Xc)
        return refs[values]

    yield IRP, JA, AS, Xc, oracle
    refs.clear()


class BigBench(Bench):
    """Bench that uploads X only when (k, ldx, shift) changes: nothing writes
    X between two launches, and at this size one upload is 134 MB"""

    on_device = None

    def put_X(self, k, ldx=0, shift=0):
        if self.on_device != (k, ldx, shift):
            super().put_X(k, ldx, shift)
            self.on_device = (k, ldx, shift)


def check_big_launch(Yf, k, single, y_ref, scale, what):
    """bits of the single-vector launch on EVERY row, the oracle's bound, and
    the fill beyond row M and column k (what a wrong mask on the padded grid
    would overwrite)"""
    M = BIG_M
    assert Yf.shape[0] == M + PAST and Yf.shape[1] >= k, what
    only_k_columns_written(Yf, M, k, what)
    for j in range(k):
        got = np.ascontiguousarray(Yf[:M, j])
        same = bits(got) == bits(single[j])
        assert np.all(same), (what, "column", j, "rows that differ",
                              int(np.sum(~same)), "first",
                              int(np.argmin(same)))
        err = np.max(np.abs(got - y_ref[j]) / np.maximum(scale[j], 1e-300))
        assert err <= TIGHT, (what, "column", j, err)


@pytest.mark.parametrize("values", ["f64", "f32"])
def test_grouped_order_and_its_padded_grid_change_no_bit(big, values):
    M = N = BIG_M
    IRP, JA, AS, Xc, oracle = big
    y_ref, scale = oracle(values)
    dG = S.CsrDevice.generate(*BIG_SPEC, 0, 42)
    d = dG.to_f32() if values == "f32" else dG
    h = d.to_hll(True)
    # the premise: both handles carry order 2, and no row is left to a side
    # kernel, so the bit rule covers every row
    assert d.M == M >= 2_000_000 and d.NZ == len(JA)
    assert h.num_blocks == (M + 31) // 32 >= 65536 and M % 32 == 3
    assert d.value_bytes == h.value_bytes == (4 if values == "f32" else 8)
    assert np.all(exact_rows(IRP, M, "csr")) and np.all(exact_rows(IRP, M, "hll"))
    assert len(set(np.diff(IRP).tolist())) >= 3  # ragged: HLL has pads
    bench = BigBench(M, N, Xc)
    csr_groups = (0, 2, 32)
    single = {("csr", g): [bench.single(d, SINGLE["csr"], j, group=g)
                           for j in range(MAXK)] for g in csr_groups}
    single["hll"] = [bench.single(h, SINGLE["hll"], j) for j in range(MAXK)]
    for k in (1, 4, 8):  # P / U = 8, 4, 2: three grids
        for g in csr_groups:
            ldy = k + 1 if g == 32 else 0
            check_big_launch(bench.multi(d, k, ldy=ldy, group=g), k,
                             single["csr", g], y_ref, scale,
                             (values, "csr", k, "group", g, "ldy", ldy))
        ldy = k + 1 if k == 4 else 0
        check_big_launch(bench.multi(h, k, ldy=ldy), k, single["hll"], y_ref,
                         scale, (values, "hll", k, "ldy", ldy))
        if k == 4:  # other workgroup sizes: other grids, other padding
            for w in (1, 16):
                check_big_launch(bench.multi(d, k, waves_per_block=w), k,
                                 single["csr", 0], y_ref, scale,
                                 (values, "csr", k, "waves", w))
                check_big_launch(bench.multi(h, k, waves_per_block=w), k,
                                 single["hll"], y_ref, scale,
                                 (values, "hll", k, "waves", w))
    for m in {h, d, dG}:
        m.release()
    bench.free()


@pytest.mark.parametrize("values", ["f64", "f32"])
def test_autotune_moves_the_order_and_changes_no_bit(values):
    """autotune() may leave the handle in any of the three workgroup orders and
    may build a blocked copy: launch_multi gives the bits it gave before"""
    case = "synth:ragged"
    M, N, IRP, JA, AS, _, _ = case_arrays(case)
    A = S.csr_from_arrays(case, M, N, IRP, JA, AS)
    bench = Bench(M, N, x_columns(N))
    hs = handles(A, values)
    for fmt, m in hs.items():
        before = bench.multi(m, 5)
        only_k_columns_written(before, M, 5, (values, fmt, "before"))
        assert not np.any(bits(before[:M, :5]) == FILL), (values, fmt)
        bench.single(m, SINGLE[fmt], 0)  # x = X[:, 0] for the timed launches
        m.autotune(bench.x.ptr, bench.y.ptr)
        after = bench.multi(m, 5)
        assert np.array_equal(bits(after), bits(before)), (values, fmt,
                                                           m.tune_log())
    for m in hs.values():
        m.release()
    bench.free()
    S.csr_free(A)


# -------------------------------------------------------------- B. thresholds
def threshold_matrix():
    """the recipe of test_gpu_parity.py::test_long_rows_at_every_threshold_
    stream_segments_and_blocked_side_path: rows at and next to 2048 (the entry
    budget of a range: beyond it k_csr_multi_long's row), 8192 (beyond it a
    row owns several ranges) and 16 384 entries, hack blocks at and next to
    512 columns (beyond it k_hll_multi_wide's block)"""
    rng = np.random.default_rng(11)
    special = [8192, 8193, 12_288, 12_289, 4096 * 5 - 1, 16_384, 16_385,
               20_000, 40_960, 0, 0, 70_001, 1, 8191, 4096, 4097,
               2048 * 5 - 1, 2048 * 5, 2048 * 5 + 1,
               1024 * 17 - 1, 1024 * 17, 1024 * 17 + 1]
    lens = np.concatenate([
        [16_385],                              # a long row FIRST
        rng.integers(1, 4, 3_000),
        special,                               # adjacent long rows, empties
        rng.integers(0, 12, 5_000),
        [8193, 16_385],                        # ... and LAST
    ]).astype(np.int64)
    for at, ln in ((100, 512), (400, 513), (700, 511), (1000, 768), (1300, 769),
                   (1600, 2047), (1900, 2048), (2200, 2049), (2500, 1025)):
        lens[at] = ln
    M, N = len(lens), 90_000
    IRP = np.zeros(M + 1, dtype=np.int32)
    IRP[1:] = np.cumsum(lens)
    JA = rng.integers(0, N, IRP[-1]).astype(np.int32)
    AS = rng.uniform(-1, 1, IRP[-1])
    return M, N, IRP, JA, AS


def block_widths(IRP, M):
    nb = (M + 31) // 32
    padded = np.zeros(nb * 32, np.int64)
    padded[:M] = np.diff(IRP)
    return padded.reshape(nb, 32).max(axis=1)


@pytest.mark.parametrize("values", ["f64", "f32"])
def test_every_boundary_between_the_main_and_the_side_kernels(values):
    M, N, IRP, JA, AS = threshold_matrix()
    # the premise, from IRP: a later edit of the recipe cannot drop a boundary
    lens = np.diff(IRP)
    for n in (2047, 2048, 2049, 8191, 8192, 8193, 16_384, 16_385):
        assert np.any(lens == n), n
    width = block_widths(IRP, M)
    for w in (511, 512, 513):
        assert np.any(width == w), w
    assert lens[0] > 2048 and lens[M - 1] > 2048   # a long row first and last
    assert lens[M - 2] > 8192                      # two adjacent, several ranges
    assert M % 32 != 0 and width[-1] > 512         # the ragged tail block is wide
    assert np.any((lens[1:-1] == 0) & (lens[:-2] > 2048))  # long, then empty
    Xc = x_columns(N)
    y_ref, scale = oracle_columns(IRP, JA, round32(AS) if values == "f32"
                                  else AS, Xc)
    A = S.csr_from_arrays("thresholds", M, N, IRP, JA, AS)
    bench = Bench(M, N, Xc)
    hs = handles(A, values)
    ks = range(1, MAXK + 1)
    for fmt, m in hs.items():
        assert m.value_bytes == (4 if values == "f32" else 8)
        for kw in (({}, dict(group=2), dict(group=32)) if fmt == "csr"
                   else ({},)):
            # the bits of the single-vector kernel on the rows of the bit
            # rule, the oracle's bound on all rows
            check_bits_and_bound(bench, m, fmt, IRP, y_ref, scale,
                                 "thresholds", ks, **kw)
            for k in ks:
                a, b = bench.multi(m, k, **kw), bench.multi(m, k, **kw)
                what = (values, fmt, kw, k)
                # a row that no workgroup claims still holds the fill
                unwritten = np.any(bits(a[:M, :k]) == FILL, axis=1)
                assert not np.any(unwritten), (what, "rows never written",
                                               np.flatnonzero(unwritten)[:8],
                                               lens[unwritten][:8])
                assert np.array_equal(bits(a), bits(b)), what
    for m in hs.values():
        m.release()
    bench.free()
    S.csr_free(A)


# ------------------------------------------------------------ C. non-finite X
INF, NAN = float("inf"), float("nan")
NF_N = 8
#: rows of [(column, value), ...]; values exact in fp32.  Hack block 0 (rows
#: 0-31) is 3 columns wide, block 1 (rows 32-63) is empty (width 0), block 2
#: (rows 64-76) is the partial one, 2 columns wide
NF_ROWS = (
    [[(0, 1.0), (1, 2.0)],             # holds column 0, shorter than its block
     [],                               # empty, in a block of non-zero width
     [(2, 1.0)],
     [(1, 0.5), (3, -1.0)],            # short, last valid column 3
     [(3, 2.0)],                       # short, only column 3
     [(1, 1.0), (2, 1.0), (3, 0.25)],  # as wide as the block: no pad
     [(0, 0.0)],                       # its only entry an explicit 0.0
     [(4, 0.0)],                       # ... and one not on column 0
     [(5, 1.0), (6, 1.0)],             # holds both columns of the +inf / -inf pair
     [(5, 2.0)],
     [(6, 1.0), (7, 1.0)],
     [(6, -0.5)],
     [(0, 1.0), (5, 1.0), (6, -1.0)],
     [],
     [(7, 1.0)],
     [(1, -2.0), (7, 0.5)]]
    + [[] for _ in range(16)]
    + [[] for _ in range(32)]
    + [[(0, -1.0)],                    # holds column 0, short
       [],
       [(2, 1.0), (4, 1.0)],
       [(3, 1.0)],                     # short, last valid column 3
       [(5, 0.5), (6, 0.5)]]
    + [[] for _ in range(7)]
    + [[(1, 3.0)]])
#: column j of X -> what is not finite in it; every other column is finite
NF_POISON = {1: {0: INF}, 3: {0: NAN}, 4: {3: INF}, 6: {5: INF, 6: -INF}}


def nonfinite_case():
    rows = NF_ROWS
    M = len(rows)
    IRP = np.zeros(M + 1, np.int32)
    IRP[1:] = np.cumsum([len(r) for r in rows])
    JA = np.array([c for r in rows for c, _ in r], np.int32)
    AS = np.array([v for r in rows for _, v in r], np.float64)
    assert np.array_equal(round32(AS), AS)
    Xc = np.arange(1.0, 1.0 + NF_N * MAXK).reshape(NF_N, MAXK) / 4.0
    for j, at in NF_POISON.items():
        for c, v in at.items():
            Xc[c, j] = v
    return M, NF_N, IRP, JA, AS, Xc


def klass(y):
    """0 NaN, 1 +inf, 2 -inf, 3 finite"""
    y = np.asarray(y, np.float64)
    return np.where(np.isnan(y), 0, np.where(y == INF, 1,
                                             np.where(y == -INF, 2, 3)))


def check_class_and_bound(got, ref, scale, what):
    assert np.array_equal(klass(got), klass(ref)), (
        what, "rows", np.flatnonzero(klass(got) != klass(ref)),
        "got", got[klass(got) != klass(ref)],
        "expected", ref[klass(got) != klass(ref)])
    fin = np.isfinite(ref)
    assert np.all(np.isfinite(scale[fin])), what
    err = np.max(np.abs(got[fin] - ref[fin]) / np.maximum(scale[fin], 1e-300))
    assert err <= TIGHT, (what, err)


def nonfinite_references(M, IRP, JA, AS, Xc):
    """-> (CSR reference, padded-HLL reference, row scale), a list over the
    columns of X each: the strict-IEEE oracle on the CSR arrays, and on the
    column-major HLL form with its pads rewritten (explicit zeros at the row's
    previous valid column, or at column 0)"""
    off, maxnz, _, HJA, HAS = O.csr_to_hll(IRP, JA, AS, True)
    HJA = O.hll_fix_pads(M, True, off, maxnz, HJA)
    csr, hll, scale = [], [], []
    for j in range(MAXK):
        xj = np.ascontiguousarray(Xc[:, j])
        csr.append(O.csr_spmv(IRP, JA, AS, xj))
        hll.append(O.hll_spmv(M, True, off, maxnz, HJA, HAS, xj))
        scale.append(O.csr_abs_spmv(IRP, JA, AS, xj))
    return csr, hll, scale


def test_the_nonfinite_case_holds_what_it_is_meant_to_hold():
    """the premises of the two tests below (no device work)"""
    M, N, IRP, JA, AS, Xc = nonfinite_case()
    lens = np.diff(IRP)
    width = np.array([lens[b:b + 32].max() for b in range(0, M, 32)])
    assert M % 32 != 0 and list(width) == [3, 0, 2]
    holds = lambda r, c: c in JA[IRP[r]:IRP[r + 1]]
    in_wide = np.repeat(width > 0, 32)[:M]
    assert np.any((lens == 0) & in_wide) and np.any((lens == 0) & ~in_wide)
    assert np.any((lens > 0) & (lens < np.repeat(width, 32)[:M]))
    assert any(lens[r] == 1 and AS[IRP[r]] == 0.0 for r in range(M))
    assert any(holds(r, 0) for r in range(M))
    assert any(lens[r] and not holds(r, 0) for r in range(M))
    # column 3 is the last valid column of a row shorter than its block
    assert any(0 < lens[r] < width[r // 32] and JA[IRP[r + 1] - 1] == 3
               for r in range(M))
    assert any(holds(r, 5) and holds(r, 6) for r in range(M))
    csr, hll, _ = nonfinite_references(M, IRP, JA, AS, Xc)
    for j in range(MAXK):
        if j in NF_POISON:
            # a non-finite X[c, j] reaches exactly the rows that hold column c
            hit = np.array([any(holds(r, c) for c in NF_POISON[j])
                            for r in range(M)])
            assert np.array_equal(~np.isfinite(csr[j]), hit), j
            # ... and, through the pads, more rows of the padded form
            assert np.any(klass(hll[j]) != klass(csr[j])), j
        else:
            assert np.all(np.isfinite(csr[j])) and np.all(np.isfinite(hll[j]))
            assert np.array_equal(bits(csr[j]), bits(hll[j])), j
    # x[0] = inf: an empty row of a block of non-zero width turns NaN (pads on
    # column 0), one of the empty block does not
    assert np.isnan(hll[1][1]) and hll[1][40] == 0.0 and csr[1][1] == 0.0


NF_KS = (2, 5, 8)


def check_multi_nonfinite(bench, m, ref, scale, what, empty=None):
    M = bench.M
    for k in NF_KS:
        Yf = bench.multi(m, k)
        only_k_columns_written(Yf, M, k, (what, k))
        for j in range(k):
            check_class_and_bound(Yf[:M, j], ref[j], scale[j], (what, k, j))
        if empty is not None:  # +0.0, every column
            assert np.all(bits(Yf[:M, :k][empty]) == 0), (what, k)
        # a launch of k vectors next to poisoned ones: the finite columns
        # stay finite in every row
        finite = [j for j in range(k) if j not in NF_POISON]
        assert np.all(np.isfinite(Yf[:M][:, finite])), (what, k)


def test_csr_confines_a_nonfinite_x_to_the_rows_that_hold_its_column():
    M, N, IRP, JA, AS, Xc = nonfinite_case()
    csr, _, scale = nonfinite_references(M, IRP, JA, AS, Xc)
    empty = np.diff(IRP) == 0
    A = S.csr_from_arrays("nonfinite", M, N, IRP, JA, AS)
    bench = Bench(M, N, Xc)
    for values in ("f64", "f32"):
        d = S.CsrDevice.upload(A, values=values)
        check_multi_nonfinite(bench, d, csr, scale, (values, "csr multi"),
                              empty)
        for g in (2, 32):
            Yf = bench.multi(d, MAXK, group=g)
            for j in range(MAXK):
                check_class_and_bound(Yf[:M, j], csr[j], scale[j],
                                      (values, "csr multi group", g, j))
        for kid in range(S.NUM_CSR_KERNELS):
            for j in range(MAXK):
                y = bench.single(d, kid, j)
                check_class_and_bound(y, csr[j], scale[j],
                                      (values, "csr kernel", kid, j))
                assert np.all(bits(y[empty]) == 0), (values, kid, j)
        if values == "f64":  # the blocked copy (not available with f32 values)
            for sched in ("steps", "chain", "sweep"):
                d.build_panels(0, sched)
                for j in range(MAXK):
                    check_class_and_bound(
                        bench.single(d, S.CSR_KERNEL_PANELS, j), csr[j],
                        scale[j], ("csr blocked", sched, j))
        d.release()
    bench.free()
    S.csr_free(A)


def test_hll_pads_carry_a_nonfinite_x_and_the_blocked_copy_drops_them():
    """A direct launch on a column-major HLL handle multiplies the pads
    (explicit zeros on the row's previous valid column, or on column 0): it
    follows the oracle on the PADDED matrix, which differs from the CSR one
    on this input.  The handle's blocked copy drops the pads and follows the
    CSR reference."""
    M, N, IRP, JA, AS, Xc = nonfinite_case()
    csr, hll, scale = nonfinite_references(M, IRP, JA, AS, Xc)
    assert any(np.any(klass(hll[j]) != klass(csr[j])) for j in NF_POISON)
    A = S.csr_from_arrays("nonfinite", M, N, IRP, JA, AS)
    bench = Bench(M, N, Xc)
    for values in ("f64", "f32"):
        d = S.CsrDevice.upload(A, values=values)
        made = {"from_csr": d.to_hll(True)}
        Hh = S.csr_to_hll(A, True)  # host form in: pads rewritten at upload
        made["uploaded"] = S.HllDevice.upload(Hh, True, values=values)
        for how, h in made.items():
            check_multi_nonfinite(bench, h, hll, scale, (values, how, "multi"))
            for kid in (1, 2):
                assert S.HLL_KERNEL_COL_MAJOR[kid]
                for j in range(MAXK):
                    check_class_and_bound(bench.single(h, kid, j), hll[j],
                                          scale[j], (values, how, kid, j))
        if values == "f64":
            h = made["from_csr"]
            for sched in ("steps", "chain", "sweep"):
                h.build_panels(0, sched)
                for j in range(MAXK):
                    check_class_and_bound(
                        bench.single(h, S.HLL_KERNEL_PANELS, j), csr[j],
                        scale[j], ("hll blocked", sched, j))
        for h in made.values():
            h.release()
        S.hll_free(Hh)
        d.release()
    bench.free()
    S.csr_free(A)
