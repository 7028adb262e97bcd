"""MINRES on the device (spmv_*_minres, spmv_engine.h) on the GPU: CSR and
column-major HLL handles, f64 and f32 values, 1-8 interleaved systems, with
and without a diagonal preconditioner, and the device square root behind it
(spmv_debug_sqrt).

The expected values come from the numpy restatement of the solver
(tests/_minres.py), with the product of an iteration taken from the SAME
handle's launch_multi and the first and the closing residual from its
launch_axpby, all with the same opts.  numpy rounds every operation once and
np.sqrt is correctly rounded, which is the contract, so the uint64 views of X
are compared, and iterations, status and the bits of pp / bn2 / rr / bb.  No
tolerance appears anywhere except the sanity line of the use cases: the true
residual of the device's X, computed on the host, is at most 10 tol (the
bound tests/test_minres.py holds the restatement to on the same inputs).

Inputs: tests/_cg.py common_inputs (column 1 all zero, column 2 scaled by
1e-3, X0 zero except column 3).  Every test runs under a time limit of its own
(LIMIT_S): a test that exceeds it ends the whole process, so nothing else is
started on the device.
"""
import ctypes as C
import errno
import faulthandler

import numpy as np
import pytest

import _cg as G
import _minres as MR
import spmv_scpa_amd as S
from test_gpu_cg import NWG, T, TOL, fill, neighbours_kept, put, upload
from test_gpu_f32_values import round32
from test_gpu_multi_vector import FILL, PAST, bits
from test_gpu_pcg import PcgBench

pytestmark = pytest.mark.gpu

LIMIT_S = 240
FIELDS = ("pp", "bn2", "rr", "bb")


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


class MrBench(PcgBench):
    """PcgBench (B, X, P / Q of the restatement, a minv buffer) solving
    through minres()"""

    def want(self, m, B, X0, minv=None, tol=TOL, maxit=200, **opts):
        product, residual0 = self.callables(m, B, X0, **opts)
        M, k = B.shape

        def residual(X):
            put(self.P.ptr, X)
            put(self.Q.ptr, B)
            m.launch_axpby(-1.0, 1.0, self.P.ptr, self.Q.ptr, k, **opts)
            S.stream_sync()
            return self.Q.to_numpy(np.float64, M * k).reshape(M, k)
        return MR.restate(product, residual0, B, X0, minv, tol, maxit,
                          residual=residual)

    def solve(self, m, B, X0, ldb=0, ldx=0, shift=0, pre=False, **kw):
        """-> (records, whole X buffer as (M + PAST, ldx), whole B buffer):
        padding columns of B are NaN, those of X and the rows beyond M of
        both hold the 0xFF fill.  pre: with the minv buffer as it stands.
        Asserts that neither B nor minv was written"""
        M, k = B.shape
        lb, lx = ldb or k, ldx or k
        Bh = np.full((M + PAST, lb), np.nan)
        bits(Bh)[M:] = FILL
        Bh[:M, :k] = B
        Xh = np.empty((M + PAST, lx))
        bits(Xh)[:] = FILL
        Xh[:M, :k] = X0
        fill(self.B)
        fill(self.X)
        put(self.B.ptr, Bh)
        put(self.X.ptr + shift, Xh)
        before = self.minv.to_numpy(np.uint64, M + PAST)
        rec = m.minres(self.B.ptr, self.X.ptr + shift, k,
                       d_minv=self.minv.ptr if pre else None, ldb=ldb,
                       ldx=ldx, **kw)
        S.stream_sync()
        Xf = self.X.to_numpy(np.float64, (M + PAST) * lx + shift // 8)
        Bf = self.B.to_numpy(np.float64, (M + PAST) * lb)
        assert np.array_equal(bits(Bf), bits(Bh.ravel())), "B was written"
        assert np.array_equal(self.minv.to_numpy(np.uint64, M + PAST),
                              before), "minv was written"
        return rec, Xf[shift // 8:].reshape(M + PAST, lx), Bh


def same_solve(rec, X, want, tag):
    """a device solve against a restatement (or two device solves): bits"""
    k = len(rec)
    print(tag, "status", [r.status for r in rec], "iterations",
          [r.iterations for r in rec])
    assert [r.status for r in rec] == list(want.status), tag
    assert [r.iterations for r in rec] == list(want.iterations), tag
    for name in FIELDS:
        got = np.array([getattr(r, name) for r in rec])
        assert np.array_equal(bits(got), bits(getattr(want, name))), \
            (tag, name, got, getattr(want, name))
    same = bits(X[:, :k]) == bits(want.X)
    assert np.all(same), (tag, "elements of X that differ",
                          int(np.sum(~same)), np.argwhere(~same)[:4].tolist())


def as_solve(rec, X):
    k = len(rec)
    return MR.Solve(X[:, :k].copy(), [r.status for r in rec],
                    [r.iterations for r in rec],
                    *(np.array([getattr(r, f) for r in rec]) for f in FIELDS))


def column(base, j):
    return MR.Solve(base.X[:, j:j + 1], base.status[j:j + 1],
                    base.iterations[j:j + 1],
                    *(getattr(base, f)[j:j + 1] for f in FIELDS))


def positive_minv(M, seed=9):
    """any positive diagonal is a preconditioner: uniform(0.5, 2)"""
    return np.random.default_rng(seed).uniform(0.5, 2.0, M)


def release(hs):
    for m in hs.values():
        m.release()


# -------------------------------------------------------------------- 1. bits
#: (M, k): the tile of 256 rows and the wrap of the 1024 * 256 dot slots
SIZES = [(1, 1), (2, 3), (255, 4), (256, 8), (257, 3), (1000, 4),
         (262143, 8), (262145, 3)]


@pytest.mark.parametrize("values", ["f64", "f32"])
@pytest.mark.parametrize("M,k", SIZES)
def test_a_solve_has_the_bits_of_the_restatement(M, k, values):
    assert NWG * T == 262144
    mat = MR.shifted_lap1d(M, 0.9)
    B, X0 = G.common_inputs(M, k)
    maxit = 200 if M < 255 else 40 if M < 262143 else 12
    bench = MrBench(M)
    minv = bench.set_minv(positive_minv(M))
    hs = upload(mat, values)
    for fmt, m in hs.items():
        for pre in (False, True):
            tag = (M, k, values, fmt, pre)
            want = bench.want(m, B, X0, minv if pre else None, maxit=maxit)
            rec, Xf, _ = bench.solve(m, B, X0, pre=pre, tol=TOL, maxit=maxit)
            same_solve(rec, Xf[:M], want, tag)
            neighbours_kept(Xf, M, k, tag)
            if M < 255:   # a 1 x 1 or 2 x 2 system: solved in M steps
                assert all(r.status == 0 for r in rec), tag
                assert all(r.iterations <= M for r in rec), tag
            else:
                assert rec[0].status == 1 and rec[0].iterations == maxit, tag
            if k > 1:     # the zero column: converged at once, X untouched
                assert rec[1].status == 0 and rec[1].iterations == 0, tag
                assert rec[1].bb == 0.0 and rec[1].pp == 0.0, tag
                assert np.array_equal(bits(Xf[:M, 1]), bits(X0[:, 1])), tag
    release(hs)
    bench.free()


# -------------------------------------------------------- 2. iteration counts
@pytest.mark.parametrize("maxit", [0, 1, 2, 3, 4, 5])
def test_every_iteration_count_through_two_rotations_of_the_buffers(maxit):
    mat = MR.symscale(MR.shifted_lap2d(15, 17, 1.3), 5)
    M = mat[0]
    B, X0 = G.common_inputs(M)
    bench = MrBench(M)
    hs = upload(mat, "f64")
    for fmt, m in hs.items():
        minv = bench.jacobi(m)
        assert np.all(minv > 0)
        for pre in (False, True):
            tag = (maxit, fmt, pre)
            want = bench.want(m, B, X0, minv if pre else None, maxit=maxit)
            rec, Xf, _ = bench.solve(m, B, X0, pre=pre, tol=TOL, maxit=maxit)
            same_solve(rec, Xf[:M], want, tag)
            neighbours_kept(Xf, M, 4, tag)
            assert [r.status for r in rec] == [1, 0, 1, 1], tag
            assert [r.iterations for r in rec] == [maxit, 0, maxit, maxit], tag
            if maxit == 0:
                assert np.array_equal(bits(Xf[:M, :4]), bits(X0)), tag
    release(hs)
    bench.free()


# ------------------------------------------------------------ 3. independence
@pytest.mark.parametrize("pre", [False, True])
def test_the_result_depends_on_the_system_alone(pre):
    mat = MR.saddle(200, 60, 7)     # M = 260: two workgroups
    M = mat[0]
    B, X0 = G.common_inputs(M)
    bench = MrBench(M)
    bench.set_minv(positive_minv(M))
    hs = upload(mat, "f64")
    work = S.DevBuffer(S.minres_work_bytes(M, 8))
    for fmt, m in hs.items():
        # a loose tol: the columns stop at different iterations
        kw0 = dict(pre=pre, tol=1e-4, maxit=400)
        rec, Xf, _ = bench.solve(m, B, X0, **kw0)
        base = as_solve(rec, Xf[:M])
        assert base.status == [0, 0, 0, 0]
        assert len(set(base.iterations)) >= 3, base.iterations
        for kw in (dict(check_every=1), dict(check_every=3),
                   dict(check_every=0), dict(work=work),
                   dict(waves_per_block=1), dict(waves_per_block=4),
                   dict(waves_per_block=16)):
            rec, Xf, _ = bench.solve(m, B, X0, **kw0, **kw)
            same_solve(rec, Xf[:M], base, (pre, fmt, kw))
        # column j of the k = 4 solve is the k = 1 solve of that column
        for j in range(4):
            rec, Xf, _ = bench.solve(m, B[:, j:j + 1], X0[:, j:j + 1], **kw0)
            same_solve(rec, Xf[:M], column(base, j), (pre, fmt, "column", j))
            neighbours_kept(Xf, M, 1, (pre, fmt, "column", j))
        # k = 8, columns 4-7 copies of columns 0-3: the k = 4 bits twice
        B8, X8 = np.hstack([B, B]), np.hstack([X0, X0])
        for k in (8, 3):
            rec, Xf, _ = bench.solve(m, B8[:, :k], X8[:, :k], **kw0)
            neighbours_kept(Xf, M, k, (pre, fmt, "k", k))
            for j in range(k):
                same_solve(rec[j:j + 1], Xf[:M, j:j + 1], column(base, j % 4),
                           (pre, fmt, "k", k, "column", j))
    work.free()
    release(hs)
    bench.free()


# ----------------------------------------------------------------- 4. strides
class _Exactly:
    """`work` of exactly n bytes at the head of a larger allocation"""

    def __init__(self, buf, n):
        self.ptr, self.nbytes = buf.ptr, n


@pytest.mark.parametrize("pre", [False, True])
def test_strides_an_unaligned_X_and_the_neighbours(pre):
    mat = MR.saddle(200, 60, 7)
    M = mat[0]
    k = 4
    B, X0 = G.common_inputs(M)
    bench = MrBench(M)
    minv = bench.set_minv(MR.abs_inverse_diag(mat))
    hs = upload(mat, "f64")
    need = S.minres_work_bytes(M, k)
    guard = 4096
    work = S.DevBuffer(need + guard)
    for fmt, m in hs.items():
        tag = (pre, fmt)
        want = bench.want(m, B, X0, minv if pre else None, maxit=400)
        S._check(S._lib.spmv_dev_memset(work.ptr, 0xA5, work.nbytes, None),
                 "spmv_dev_memset")
        # ldx = k + 1: a column of X that is not the solver's; ldb = k + 3:
        # NaN padding in B; X 8 bytes off 16; rows beyond M of both; solve()
        # checks that B and minv (and the fill behind minv) keep their bits
        rec, Xf, _ = bench.solve(m, B, X0, ldb=k + 3, ldx=k + 1, shift=8,
                                 pre=pre, tol=TOL, maxit=400,
                                 work=_Exactly(work, need))
        same_solve(rec, Xf[:M], want, tag)
        assert [r.status for r in rec] == [0, 0, 0, 0], tag
        neighbours_kept(Xf, M, k, tag)
        tail = work.to_numpy(np.uint8, need + guard)[need:]
        assert np.all(tail == 0xA5), (tag, "bytes behind the work buffer")
    work.free()
    release(hs)
    bench.free()


# ------------------------------------------- 5. columns that stop on their own
def test_four_columns_that_stop_at_different_iterations():
    # diag(3, -2, 0.5, 3, ...) on the first 300 rows, a shifted 1-D stencil on
    # the other 300: a right-hand side that lives on the first block sees three
    # eigenvalues
    n = 300
    Md, Id, Jd, Ad = MR.diagm(np.resize([3.0, -2.0, 0.5], n))
    Ml, Il, Jl, Al = MR.shifted_lap1d(n, 0.9)
    M = 2 * n
    mat = (M, np.concatenate((Id, Id[-1] + Il[1:])).astype(np.int32),
           np.concatenate((Jd, Jl + n)).astype(np.int32),
           np.concatenate((Ad, Al)))
    rng = np.random.default_rng(6)
    B = rng.uniform(-1, 1, (M, 4))
    B[n:, 0] = 0.0          # three eigenvalues: converges within three steps
    B[:, 1] = 0.0           # converged at once
    B[:, 2] = np.nan        # status 2 at once
    X0 = np.zeros((M, 4))
    X0[:, 2] = 0.5
    bench = MrBench(M)
    fill(bench.minv)
    hs = upload(mat, "f64")
    for fmt, m in hs.items():
        for ce in (1, 0):
            tag = (fmt, ce)
            want = bench.want(m, B, X0, maxit=25)
            rec, Xf, _ = bench.solve(m, B, X0, tol=TOL, maxit=25,
                                     check_every=ce)
            same_solve(rec, Xf[:M], want, tag)
            neighbours_kept(Xf, M, 4, tag)
            assert [r.status for r in rec] == [0, 0, 2, 1], tag
            assert 1 <= rec[0].iterations <= 3, tag
            assert [r.iterations for r in rec[1:]] == [0, 0, 25], tag
            assert np.array_equal(bits(Xf[:M, 1:3]), bits(X0[:, 1:3])), tag
            both = as_solve(rec, Xf[:M])
            for j in range(4):
                rec1, X1, _ = bench.solve(m, B[:, j:j + 1], X0[:, j:j + 1],
                                          tol=TOL, maxit=25, check_every=ce)
                same_solve(rec1, X1[:M], column(both, j), tag + ("column", j))
    release(hs)
    bench.free()


# ---------------------------------------------------------------- 6. statuses
def test_a_breakdown_is_a_status_not_a_fault():
    good = MR.shifted_lap2d(15, 17, 1.3)
    Mg = good[0]
    Bg, Xg = G.common_inputs(Mg)
    gbench = MrBench(Mg)
    fill(gbench.minv)
    ghs = upload(good, "f64")
    clean = {}
    for fmt, m in ghs.items():
        rec, Xf, _ = gbench.solve(m, Bg, Xg, tol=1e-4, maxit=400)
        clean[fmt] = as_solve(rec, Xf[:Mg])
        assert clean[fmt].status == [0, 0, 0, 0]

    def still_solves(tag):
        for fmt, m in ghs.items():
            rec, Xf, _ = gbench.solve(m, Bg, Xg, tol=1e-4, maxit=400)
            same_solve(rec, Xf[:Mg], clean[fmt], (tag, "clean solve", fmt))

    # a preconditioner that is not positive, or not finite
    for tag, d, status in (
            ("negative minv", np.full(Mg, -1.0), [2, 0, 2, 2]),
            ("inf in minv", np.where(np.arange(Mg) == 9, np.inf, 1.0),
             [2, 2, 2, 2])):      # 0 * inf: the zero column's bn2 is NaN
        for fmt, m in ghs.items():
            minv = gbench.set_minv(d)
            want = gbench.want(m, Bg, Xg, minv)
            assert list(want.status) == status, (tag, fmt)
            for ce in (0, 1):
                rec, Xf, _ = gbench.solve(m, Bg, Xg, pre=True, tol=TOL,
                                          maxit=50, check_every=ce)
                same_solve(rec, Xf[:Mg], want, (tag, fmt, ce))
                assert [r.iterations for r in rec] == [0, 0, 0, 0], (tag, fmt)
                assert np.array_equal(bits(Xf[:Mg, :4]), bits(Xg)), (tag, fmt)
                neighbours_kept(Xf, Mg, 4, (tag, fmt, ce))
        still_solves(tag)

    # a matrix of stored zeros, b != 0: Q = 0, alfa = 0, beta = 0, gamma = 0
    M = 70
    bench = MrBench(M)
    fill(bench.minv)
    X0 = np.zeros((M, 2))
    Br = np.random.default_rng(2).uniform(-1, 1, (M, 2))
    hs = upload(MR.diagm(np.zeros(M)), "f64")
    for fmt, m in hs.items():
        want = bench.want(m, Br, X0)
        assert list(want.status) == [2, 2] and list(want.iterations) == [0, 0]
        for ce in (0, 1):
            rec, Xf, _ = bench.solve(m, Br, X0, tol=TOL, maxit=50,
                                     check_every=ce)
            same_solve(rec, Xf[:M], want, ("zeros", fmt, ce))
            assert np.array_equal(bits(Xf[:M]), bits(X0)), fmt
            neighbours_kept(Xf, M, 2, ("zeros", fmt, ce))
    release(hs)
    bench.free()
    still_solves("stored zeros")

    # one inf in column 0 of B: that column stops, the others never notice
    Bi = Bg.copy()
    Bi[7, 0] = np.inf
    for fmt, m in ghs.items():
        for ce in (1, 0):
            rec, Xf, _ = gbench.solve(m, Bi, Xg, tol=1e-4, maxit=400,
                                      check_every=ce)
            assert rec[0].status == 2 and rec[0].iterations == 0, (fmt, rec)
            assert np.array_equal(bits(Xf[:Mg, 0]), bits(Xg[:, 0])), fmt
            for j in (1, 2, 3):
                same_solve(rec[j:j + 1], Xf[:Mg, j:j + 1],
                           column(clean[fmt], j), ("inf", fmt, ce, j))
        same_solve(rec, Xf[:Mg], gbench.want(m, Bi, Xg, tol=1e-4, maxit=400),
                   ("inf", fmt))
    still_solves("inf in B")
    release(ghs)
    gbench.free()


# --------------------------------------------------------------- 7. use cases
def _true_residual(mat, stored, B, X):
    M, IRP, JA, _ = mat
    A = MR.dense((M, IRP, JA, stored))
    r = np.linalg.norm(B - A @ X, axis=0)
    b = np.linalg.norm(B, axis=0)
    return np.where(b > 0, r / np.where(b > 0, b, 1.0), r)


def _rr_bb_are_true(bench, m, B, Xf, rec, tag):
    """rr and bb: _cg.dot of the device's B - A X and of B"""
    M, k = B.shape
    put(bench.P.ptr, Xf[:M, :k])
    put(bench.Q.ptr, B)
    m.launch_axpby(-1.0, 1.0, bench.P.ptr, bench.Q.ptr, k)
    S.stream_sync()
    R = bench.Q.to_numpy(np.float64, M * k).reshape(M, k)
    assert np.array_equal(bits(np.array([r.rr for r in rec])),
                          bits(G.dot(R, R))), (tag, "rr")
    assert np.array_equal(bits(np.array([r.bb for r in rec])),
                          bits(G.dot(B, B))), (tag, "bb")


@pytest.mark.parametrize("values", ["f64", "f32"])
def test_a_saddle_point_system_with_the_absolute_diagonal(values):
    mat = MR.saddle(200, 60, 7)
    M, IRP, JA, AS = mat
    stored = round32(AS) if values == "f32" else AS
    B, X0 = G.common_inputs(M)
    bench = MrBench(M)
    hs = upload(mat, values)
    for fmt, m in hs.items():
        tag = (values, fmt)
        # the diagonal from the device; the last 60 rows store none
        fill(bench.minv)
        m.diag(bench.minv.ptr)
        S.stream_sync()
        d = bench.minv.to_numpy(np.float64, M)
        assert np.all(d[:200] > 0) and np.all(d[200:] == 0.0), tag
        minv = bench.set_minv(np.where(d == 0, 1.0,
                                       1.0 / np.where(d == 0, 1.0, np.abs(d))))
        for pre in (False, True):
            want = bench.want(m, B, X0, minv if pre else None, maxit=400)
            rec, Xf, _ = bench.solve(m, B, X0, pre=pre, tol=TOL, maxit=400)
            same_solve(rec, Xf[:M], want, tag + (pre,))
            assert [r.status for r in rec] == [0, 0, 0, 0], tag
            res = _true_residual(mat, stored, B, Xf[:M, :4])
            print(tag, pre, "true residual", res)
            assert np.all(res <= 10 * TOL), (tag, res)
            _rr_bb_are_true(bench, m, B, Xf, rec, tag + (pre,))
        # CG stops at its first p.Ap <= 0
        fill(bench.X)
        put(bench.X.ptr, np.vstack([X0, np.zeros((PAST, 4))]))
        put(bench.B.ptr, np.vstack([B, np.zeros((PAST, 4))]))
        crec = m.cg(bench.B.ptr, bench.X.ptr, 4, tol=TOL, maxit=400)
        assert [r.status for r in crec] == [2, 0, 2, 2], tag
    release(hs)
    bench.free()


def test_the_arrow_and_a_shifted_stencil_where_cg_breaks_down():
    for name, mat in (("sym_arrow(2051,3)", MR.sym_arrow(2051, 3)),
                      ("shifted_lap2d(37,29,1.3)",
                       MR.shifted_lap2d(37, 29, 1.3))):
        M, IRP, JA, AS = mat
        if name.startswith("sym_arrow"):
            assert IRP[1] == M > 2048   # the CSR long-row kernel, a wide block
        B, X0 = G.common_inputs(M)
        bench = MrBench(M)
        fill(bench.minv)
        hs = upload(mat, "f64")
        for fmt, m in hs.items():
            tag = (name, fmt)
            want = bench.want(m, B, X0, maxit=2000)
            rec, Xf, _ = bench.solve(m, B, X0, tol=TOL, maxit=2000)
            same_solve(rec, Xf[:M], want, tag)
            neighbours_kept(Xf, M, 4, tag)
            assert [r.status for r in rec] == [0, 0, 0, 0], tag
            res = _true_residual(mat, AS, B, Xf[:M, :4])
            print(tag, "iterations", [r.iterations for r in rec],
                  "true residual", res)
            assert np.all(res <= 10 * TOL), (tag, res)
            _rr_bb_are_true(bench, m, B, Xf, rec, tag)
            fill(bench.X)
            put(bench.X.ptr, np.vstack([X0, np.zeros((PAST, 4))]))
            put(bench.B.ptr, np.vstack([B, np.zeros((PAST, 4))]))
            crec = m.cg(bench.B.ptr, bench.X.ptr, 4, tol=TOL, maxit=2000)
            assert [r.status for r in crec] == [2, 0, 2, 2], tag
        release(hs)
        bench.free()


# -------------------------------------------------------------------- 8. sqrt
def sqrt_inputs():
    rng = np.random.default_rng(11)
    # exact squares of 26-bit integers scaled by even powers of two, and their
    # neighbours on both sides
    r = rng.integers(1, 1 << 26, 20000).astype(np.float64)
    sq = (r * r) * 4.0 ** rng.integers(-200, 200, r.size)
    assert np.array_equal(np.sqrt(sq) ** 2, sq)
    near = np.concatenate((sq, np.nextafter(sq, 0.0), np.nextafter(sq, np.inf)))
    # any bit pattern of a positive finite double, subnormals, the largest
    anyd = rng.integers(1, 0x7FF0000000000000, 30000).astype(np.uint64)
    sub = rng.integers(1, 1 << 52, 5000).astype(np.uint64)
    top = (np.uint64(0x7FEFFFFFFFFFFFFF)
           - np.arange(2000).astype(np.uint64))
    tiny = np.arange(1, 2001).astype(np.uint64)
    uni = rng.uniform(0.0, 4.0, 10000)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -1.0, -1e-310,
                        -1e300, 1.0, 2.0, 4.0, 0.25,
                        np.finfo(np.float64).tiny, np.finfo(np.float64).max])
    return np.concatenate((near, anyd.view(np.float64), sub.view(np.float64),
                           top.view(np.float64), tiny.view(np.float64), uni,
                           special))


def test_the_device_square_root_is_numpys():
    a = sqrt_inputs()
    assert 100_000 <= a.size <= 120_000
    d_in = S.DevBuffer.from_numpy(a)
    d_out = S.DevBuffer(a.nbytes)
    fill(d_out)
    S._check(S._lib.spmv_debug_sqrt(d_in.ptr, d_out.ptr, a.size, None),
             "spmv_debug_sqrt")
    S.stream_sync()
    got = d_out.to_numpy(np.float64, a.size)
    with np.errstate(invalid="ignore"):
        want = np.sqrt(a)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert nan.sum() == 5   # NaN, -inf and the three negative numbers
    bad = (bits(got) != bits(want)) & ~nan
    print("square roots that differ:", int(bad.sum()), "of", a.size)
    assert not bad.any(), (int(bad.sum()), a[bad][:4], got[bad][:4],
                           want[bad][:4])
    assert np.signbit(got[a.size - 14 + 1]) and got[a.size - 14 + 1] == 0.0
    d_in.free()
    d_out.free()


# ---------------------------------------------------------------- 9. refusals
def _rc(m, k, B, ldb, X, ldx, minv, tol=TOL, maxit=10, check_every=0,
        work=None, work_bytes=0, info=True, opts=None, stream=None):
    rec = (S.MinresInfo * 8)()
    return m._fn("minres")(m.h, opts, k, B, ldb, X, ldx, minv, tol, maxit,
                           check_every, work, work_bytes,
                           rec if info else None, stream), rec


def test_refusals_on_live_handles():
    mat = MR.saddle(200, 60, 7)
    M = mat[0]
    k = 4
    B, X0 = G.common_inputs(M)
    bench = MrBench(M)
    live = S._lib.spmv_live_handles()
    hs = upload(mat, "f64")
    d, cm = hs["csr"], hs["hll"]
    rm = d.to_hll(False)
    compact = cm.to_index16()
    # 260 x 261: the same rows, one more (empty) column
    A1 = S.csr_from_arrays("wide", M, M + 1, mat[1], mat[2], mat[3])
    d1 = S.CsrDevice.upload(A1)
    h1 = d1.to_hll(True)
    A0 = S.csr_from_arrays("norows", 0, 0, np.zeros(1, np.int32),
                           np.zeros(0, np.int32), np.zeros(0))
    d0 = S.CsrDevice.upload(A0)
    h0 = d0.to_hll(True)
    made = S._lib.spmv_live_handles()
    assert made == live + 8
    bench.set_minv(MR.abs_inverse_diag(mat))
    rec, Xf, _ = bench.solve(d, B, X0, pre=True, tol=TOL, maxit=400)
    assert [r.status for r in rec] == [0, 0, 0, 0]   # the buffers are filled
    Bp, Xp, Dp = bench.B.ptr, bench.X.ptr, bench.minv.ptr
    einval = -errno.EINVAL
    need = S.minres_work_bytes(M, k)
    work = S.DevBuffer(need)
    for m in (d, cm):
        for minv in (Dp, None):  # with and without: the same checks
            put(Xp, np.vstack([X0, np.zeros((PAST, k))]))
            assert _rc(m, k, Bp, 0, Xp, 0, minv)[0] == 0  # opts may be NULL
            for bad in (0, 9):
                assert _rc(m, bad, Bp, 0, Xp, 0, minv)[0] == einval
            assert _rc(m, k, Bp, 3, Xp, 0, minv)[0] == einval
            assert _rc(m, k, Bp, 0, Xp, 3, minv)[0] == einval
            assert _rc(m, k, None, 0, Xp, 0, minv)[0] == einval
            assert _rc(m, k, Bp, 0, None, 0, minv)[0] == einval
            assert _rc(m, k, Bp, 0, Xp, 0, minv, info=False)[0] == einval
            for tol in (-1e-8, float("nan")):
                assert _rc(m, k, Bp, 0, Xp, 0, minv, tol=tol)[0] == einval
            assert _rc(m, k, Bp, 0, Xp, 0, minv, maxit=-1)[0] == einval
            assert _rc(m, k, Bp, 0, Xp, 0, minv, check_every=-1)[0] == einval
            for bad in (dict(variant=1), dict(waves_per_block=17)):
                o = S._opts(**bad)
                assert _rc(m, k, Bp, 0, Xp, 0, minv,
                           opts=C.byref(o))[0] == einval, bad
            # a work buffer one byte short, or not 8-byte aligned
            assert _rc(m, k, Bp, 0, Xp, 0, minv, work=work.ptr,
                       work_bytes=need - 1)[0] == einval
            assert _rc(m, k, Bp, 0, Xp, 0, minv, work=work.ptr + 4,
                       work_bytes=need)[0] == einval
            assert _rc(m, k, Bp, 0, Xp, 0, minv, work=work.ptr,
                       work_bytes=need)[0] == 0
        assert S._lib.spmv_live_handles() == made
    assert _rc(compact, k, Bp, 0, Xp, 0, Dp)[0] == -errno.ENOTSUP
    assert _rc(rm, k, Bp, 0, Xp, 0, Dp)[0] == einval
    for m in (d1, h1):  # M != N
        assert _rc(m, k, Bp, 0, Xp, 0, Dp)[0] == einval
    # no rows: 0, every record zero
    for m in (d0, h0):
        rc, rec = _rc(m, k, Bp, 0, Xp, 0, Dp)
        assert rc == 0
        assert [(r.status, r.iterations, r.pp, r.bn2, r.rr, r.bb)
                for r in rec[:k]] == [(0, 0, 0.0, 0.0, 0.0, 0.0)] * k
    S.stream_sync()
    assert S._lib.spmv_live_handles() == made

    # a capturing stream: -EBUSY, nothing enqueued, the capture ends cleanly
    side = S.Stream()
    for m in (d, cm):
        put(Xp, np.vstack([X0, np.zeros((PAST, k))]))
        S._check(S._lib.spmv_graph_begin_capture(side.ptr), "begin_capture")
        rc, _ = _rc(m, k, Bp, 0, Xp, 0, Dp, stream=side.ptr)
        rc_own, _ = _rc(m, k, Bp, 0, Xp, 0, None, work=work.ptr,
                        work_bytes=need, stream=side.ptr)
        g = C.c_void_p()
        end = S._lib.spmv_graph_end_capture(side.ptr, C.byref(g))
        if end == 0:
            S._check(S._lib.spmv_graph_destroy(g), "spmv_graph_destroy")
        assert rc == -errno.EBUSY and rc_own == -errno.EBUSY
        assert end == 0, "the capture was invalidated"
        got = bench.X.to_numpy(np.float64, M * k).reshape(M, k)
        assert np.array_equal(bits(got), bits(X0)), "something was enqueued"
        # ... and the stream solves afterwards
        rc, rec = _rc(m, k, Bp, 0, Xp, 0, Dp, maxit=400, stream=side.ptr)
        assert rc == 0 and [r.status for r in rec[:k]] == [0, 0, 0, 0]
    side.sync()

    # only the blocked copy left: no source arrays to read
    for m in (d, cm):
        m.build_panels()
        m.release_source()
        assert _rc(m, k, Bp, 0, Xp, 0, Dp)[0] == -errno.ENODATA
        with pytest.raises(OSError) as ei:
            m.minres(Bp, Xp, k, d_minv=Dp)
        assert ei.value.errno == errno.ENODATA
    S.stream_sync()
    assert S._lib.spmv_live_handles() == made
    for m in (d, cm, rm, compact, d1, h1, d0, h0):
        m.release()
    assert S._lib.spmv_csr_minres(C.c_void_p(1 << 20), None, k, Bp, 0, Xp, 0,
                                  Dp, TOL, 10, 0, None, 0,
                                  (S.MinresInfo * 8)(), None) == -errno.EBADF
    assert S._lib.spmv_live_handles() == live
    work.free()
    bench.free()
    S.csr_free(A0)
    S.csr_free(A1)


# ------------------------------------------------------------------ 10. leaks
def test_solves_leave_no_handle_and_no_device_memory_behind():
    M, k = 262145, 8
    mat = MR.shifted_lap1d(M, 0.9)
    B, X0 = G.common_inputs(M, k)
    bench = MrBench(M)
    bench.set_minv(positive_minv(M))
    hs = upload(mat, "f64")
    for m in hs.values():   # the one-off allocations of a first use
        bench.solve(m, B, X0, pre=True, tol=TOL, maxit=2)
    S.device_sync()
    live, free0 = S._lib.spmv_live_handles(), S.dev_mem_info()[0]
    for m in hs.values():
        for pre in (False, True, False):
            rec, _, _ = bench.solve(m, B, X0, pre=pre, tol=TOL, maxit=2)
            assert rec[0].status == 1 and rec[0].iterations == 2
    S.device_sync()
    assert S._lib.spmv_live_handles() == live
    # six library-owned work buffers of 101 MB each would be 604 MB; the
    # runtime's allocator keeps some freed blocks for itself (tests/
    # test_gpu_mgpu.py holds its reload test to 256 MiB for that reason)
    assert S.minres_work_bytes(M, k) * 6 > 2 * (256 << 20)
    assert S.dev_mem_info()[0] > free0 - (256 << 20)
    release(hs)
    bench.free()
    assert S._lib.spmv_live_handles() == live - 2
