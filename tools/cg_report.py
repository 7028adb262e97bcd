#!/usr/bin/env python3
"""Measure the device-resident conjugate-gradient solver (cg(), spmv_*_cg)
and write profiles/cg.md: milliseconds per iteration for k = 1, 4, 8 systems
beside launch_multi alone on the same handle in the same process and beside
the byte model, and the host wall time of a solve for check_every = 1 and 8.

Matrices (built on the host, they have to keep every column running):
  banded   row i holds K = 32 entries at columns s..s+31, s = clamp(i - 16)
           (the pattern of SYNTH_BANDED): 30.05 on the diagonal, -1 within 15
           columns of it, and the one stored entry beyond (column i - 16, or
           what the clamp puts there) an explicit 0.0 -- symmetric, SPD by
           diagonal dominance, 32 stored entries per row.
  stencil  5-point 2-D Laplacian + 0.01 on an n x n grid, n = sqrt(rows): SPD,
           far from converged after the timed iterations.
tol = 0, so no column converges; every solve is checked to end with status 1
(maxit) and `maxit` iterations in every column.

Method.  launch_multi: ROUNDS rounds of 3 warm-ups and 10 launches between
two events, the median round and (min..max).  An iteration: the host clock
around the blocking solve (it ends in a stream synchronise) at maxit = SHORT
and at maxit = LONG with a supplied work buffer, ROUNDS times each in turns;
ms per iteration = (median LONG - median SHORT) / (LONG - SHORT), which takes
the set-up (residual, two dots) and the last copy-back out.  Byte model of an
iteration: multi_bytes(k) + 11 * 8 k M -- the vector passes of the three
kernels: dot 2 reads; update 4 reads + 2 writes; direction 2 reads + 1 write.
`model ms` prices those bytes at the rate launch_multi reached on the same
handle (multi_bytes(k) / its time).

    python tools/cg_report.py [--rows 10000000] [--out FILE]

--pcg writes profiles/pcg.md instead: the preconditioned solver (pcg(),
spmv_*_pcg) with the Jacobi preconditioner of diag(invert=True) beside cg() on
the same handle in the same process -- ms per iteration of both by the method
above, the rounds of the two taken in turns, their ratio beside the byte
model's (multi_bytes(k) + 11 * 8 k M + 16 M) / (multi_bytes(k) + 11 * 8 k M)
(minv is read by the update and by the direction kernel) -- on the two
matrices above and on the stencil scaled row and column i by
2 ** uniform(0, 6) (seed 7, shift 0.5); and on that last matrix the iterations
and the host wall time of both solvers to tol = 1e-8.

    python tools/cg_report.py --pcg [--rows 10000000] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import spmv_scpa_amd as S  # noqa: E402

PROFILES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                        "profiles")
KS = (1, 4, 8)
ROUNDS = 5
SHORT, LONG = 8, 48
VECTOR_PASSES = 11

HEADER = """# Conjugate gradients on the device: one iteration against its parts

Written by `tools/cg_report.py%s` on one MI355X; what the numbers say is in
DESIGN.md section 16. f64 values. `multi ms` is `launch_multi` alone on the same
handle in the same process (median of %d rounds of 10 launches between two
events, min..max in brackets). `iter ms` is one iteration of `cg()`: the host
clock around the blocking solve at maxit = %d and maxit = %d with a supplied work
buffer, %d rounds each in turns, (median long - median short) / %d; the bracket
is the same figure from the fastest and the slowest pair of rounds.
`bytes` is the byte model of an iteration over `multi_bytes(k)`:
(multi_bytes(k) + %d * 8 k M) / multi_bytes(k); `model ms` prices the model at
the rate `launch_multi` reached (`multi ms` x `bytes`). `solve ms` is the host
wall time of a whole solve of %d iterations with `check_every` = 1 and 8
(median of %d). tol = 0: every column runs all iterations (checked).

"""


def banded(M, K=32):
    """-> (IRP, JA, AS): the SYNTH_BANDED pattern, symmetric values"""
    rows = np.arange(M, dtype=np.int32)
    start = np.clip(rows - K // 2, 0, M - K)
    JA = start[:, None] + np.arange(K, dtype=np.int32)[None, :]
    dist = np.abs(JA - rows[:, None])
    AS = np.where(dist == 0, K - 2 + 0.05, np.where(dist < K // 2, -1.0, 0.0))
    IRP = (np.arange(M + 1, dtype=np.int64) * K).astype(np.int32)
    return IRP, np.ascontiguousarray(JA).ravel(), AS.ravel()


def stencil2d(n, shift=0.01):
    """-> (IRP, JA, AS) of the 5-point Laplacian + shift on an n x n grid"""
    M = n * n
    i = np.arange(M, dtype=np.int64)
    ix, iy = i % n, i // n
    cand = np.stack([i - n, i - 1, i, i + 1, i + n], axis=1)
    ok = np.stack([iy > 0, ix > 0, np.ones(M, bool), ix < n - 1, iy < n - 1],
                  axis=1)
    vals = np.broadcast_to(np.array([-1.0, -1.0, 4.0 + shift, -1.0, -1.0]),
                           (M, 5))
    IRP = np.zeros(M + 1, np.int32)
    IRP[1:] = np.cumsum(ok.sum(axis=1))
    return IRP, cand[ok].astype(np.int32), np.ascontiguousarray(vals[ok])


PCG_HEADER = """# Jacobi-preconditioned CG beside plain CG on the same handle

Written by `tools/cg_report.py --pcg%s` on one MI355X; what the numbers say is
in DESIGN.md section 17. f64 values, minv = `diag(invert=True)`. `cg ms` and
`pcg ms` are one iteration of `cg()` and of `pcg()`: the host clock around the
blocking solve at maxit = %d and maxit = %d with a supplied work buffer and
tol = 0 (every column runs all iterations, checked), %d rounds of each solver
in turns, (median long - median short) / %d; the bracket is the same figure
from the fastest and the slowest pair of rounds. `pcg / cg` is the ratio of the
two medians, its bracket (pcg low / cg high .. pcg high / cg low). `model` is
the byte model's ratio, (multi_bytes(k) + %d * 8 k M + 16 M) /
(multi_bytes(k) + %d * 8 k M).

"""

TOL_HEADER = """
## To tol = 1e-8 on the scaled stencil

The matrix of the last rows above, B = the synthetic vector the other rows
use, X0 = 0, check_every = 8, maxit = %d. `iterations` and `status` per column;
`ms` is the host wall time of the whole solve (median of %d, min..max).

"""


def scaled_stencil2d(n, shift=0.5, span=6, seed=7):
    """stencil2d(n, shift) with entry (r, c) multiplied by s_r * s_c,
    s = 2 ** uniform(0, span)"""
    IRP, JA, AS = stencil2d(n, shift)
    s = 2.0 ** np.random.default_rng(seed).uniform(0, span, n * n)
    rows = np.repeat(np.arange(n * n), np.diff(IRP))
    return IRP, JA, np.ascontiguousarray(AS * (s[rows] * s[JA]))


def event_ms(launch, warmup=3, iters=10):
    for _ in range(warmup):
        launch()
    e0, e1 = S.Event(), S.Event()
    e0.record()
    for _ in range(iters):
        launch()
    e1.record()
    return e0.elapsed_ms(e1) / iters


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--pcg", action="store_true",
                    help="pcg() beside cg(): writes profiles/pcg.md")
    a = ap.parse_args()
    if a.pcg:
        return main_pcg(a)
    n = int(round(a.rows ** 0.5))
    workloads = (("banded %gM x 32" % (a.rows / 1e6), a.rows,
                  lambda: banded(a.rows)),
                 ("2-D stencil %d x %d" % (n, n), n * n, lambda: stencil2d(n)))
    lines = ["| matrix | handle | k | multi ms | iter ms | / multi | bytes | "
             "model ms | iter / model | solve ms, check_every 1 | 8 |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for name, M, build in workloads:
        IRP, JA, AS = build()
        A = S.csr_from_arrays("cg_report", M, M, IRP, JA, AS)
        del IRP, JA, AS
        d = S.CsrDevice.upload(A)
        S.csr_free(A)
        hs = (("csr", d), ("hll", d.to_hll(True)))
        B, X = S.DevBuffer(M * 8 * 8), S.DevBuffer(M * 8 * 8)
        work = S.DevBuffer(S.cg_work_bytes(M, 8))
        S.dev_fill_synth(B.ptr, M * 8, 7)

        def solve(m, k, maxit, check_every=0):
            S._check(S._lib.spmv_dev_memset(X.ptr, 0, M * k * 8, None),
                     "spmv_dev_memset")
            S.stream_sync()
            t0 = time.perf_counter()
            rec = m.cg(B.ptr, X.ptr, k, tol=0.0, maxit=maxit,
                       check_every=check_every, work=work)
            ms = (time.perf_counter() - t0) * 1e3
            bad = [r for r in rec if (r.status, r.iterations) != (1, maxit)]
            if bad:
                raise SystemExit("%s k=%d: a column stopped early: %r"
                                 % (name, k, bad))
            return ms

        for label, m in hs:
            for k in KS:
                solve(m, k, SHORT)  # warm-up of every kernel of this k
                tm = sorted(event_ms(
                    lambda: m.launch_multi(B.ptr, X.ptr, k))
                    for _ in range(ROUNDS))
                ts, tl = [], []
                for _ in range(ROUNDS):
                    ts.append(solve(m, k, SHORT))
                    tl.append(solve(m, k, LONG))
                ts.sort()
                tl.sort()
                span = LONG - SHORT
                it = (tl[ROUNDS // 2] - ts[ROUNDS // 2]) / span
                it_lo, it_hi = (tl[0] - ts[0]) / span, (tl[-1] - ts[-1]) / span
                wall = [sorted(solve(m, k, LONG, ce) for _ in range(ROUNDS))
                        [ROUNDS // 2] for ce in (1, 8)]
                multi = tm[ROUNDS // 2]
                ratio = ((m.multi_bytes(k) + VECTOR_PASSES * 8 * k * M)
                         / m.multi_bytes(k))
                lines.append(
                    "| %s | %s | %d | %.3f (%.3f..%.3f) | %.3f (%.3f..%.3f) | "
                    "%.2f | %.2f | %.3f | %.2f | %.1f | %.1f |"
                    % (name, label, k, multi, tm[0], tm[-1], it, it_lo, it_hi,
                       it / multi, ratio, multi * ratio,
                       it / (multi * ratio), wall[0], wall[1]))
                print(lines[-1], flush=True)
        for _, m in hs:
            m.release()
        for b in (B, X, work):
            b.free()
    argv = " --rows %d" % a.rows if a.rows != 10_000_000 else ""
    out = a.out or os.path.join(PROFILES, "cg.md")
    with open(out, "w") as f:
        f.write(HEADER % (argv, ROUNDS, SHORT, LONG, ROUNDS, LONG - SHORT,
                          VECTOR_PASSES, LONG, ROUNDS)
                + "\n".join(lines) + "\n")
    print("wrote", out)


def main_pcg(a):
    n = int(round(a.rows ** 0.5))
    scaled = "scaled stencil %d x %d" % (n, n)
    workloads = (("banded %gM x 32" % (a.rows / 1e6), a.rows,
                  lambda: banded(a.rows)),
                 ("2-D stencil %d x %d" % (n, n), n * n, lambda: stencil2d(n)),
                 (scaled, n * n, lambda: scaled_stencil2d(n)))
    lines = ["| matrix | handle | k | cg ms | pcg ms | pcg / cg | model |",
             "|---|---|---|---|---|---|---|"]
    to_tol = ["| handle | k | solver | iterations | status | ms |",
              "|---|---|---|---|---|---|"]
    MAXIT = 5000
    for name, M, build in workloads:
        IRP, JA, AS = build()
        A = S.csr_from_arrays("pcg_report", M, M, IRP, JA, AS)
        del IRP, JA, AS
        d = S.CsrDevice.upload(A)
        S.csr_free(A)
        hs = (("csr", d), ("hll", d.to_hll(True)))
        B, X = S.DevBuffer(M * 8 * 8), S.DevBuffer(M * 8 * 8)
        minv = S.DevBuffer(M * 8)
        work = S.DevBuffer(S.pcg_work_bytes(M, 8))
        S.dev_fill_synth(B.ptr, M * 8, 7)

        def solve(m, pre, k, maxit, tol=0.0):
            S._check(S._lib.spmv_dev_memset(X.ptr, 0, M * k * 8, None),
                     "spmv_dev_memset")
            S.stream_sync()
            t0 = time.perf_counter()
            if pre:
                rec = m.pcg(B.ptr, X.ptr, minv.ptr, k, tol=tol, maxit=maxit,
                            work=work)
            else:
                rec = m.cg(B.ptr, X.ptr, k, tol=tol, maxit=maxit, work=work)
            ms = (time.perf_counter() - t0) * 1e3
            if tol == 0.0:
                bad = [r for r in rec if (r.status, r.iterations) != (1, maxit)]
                if bad:
                    raise SystemExit("%s k=%d pcg=%d: a column stopped early: "
                                     "%r" % (name, k, pre, bad))
            return ms, rec

        for label, m in hs:
            m.diag(minv.ptr, invert=True)
            S.stream_sync()
            for k in KS:
                t = {(pre, n_it): [] for pre in (0, 1) for n_it in (SHORT, LONG)}
                for pre in (0, 1):
                    solve(m, pre, k, SHORT)  # warm-up of every kernel
                for _ in range(ROUNDS):
                    for pre in (0, 1):
                        for n_it in (SHORT, LONG):
                            t[pre, n_it].append(solve(m, pre, k, n_it)[0])
                span = LONG - SHORT
                it = {}
                for pre in (0, 1):
                    ts, tl = sorted(t[pre, SHORT]), sorted(t[pre, LONG])
                    it[pre] = ((tl[ROUNDS // 2] - ts[ROUNDS // 2]) / span,
                               (tl[0] - ts[0]) / span, (tl[-1] - ts[-1]) / span)
                vec = m.multi_bytes(k) + VECTOR_PASSES * 8 * k * M
                lo, hi = sorted((it[1][1] / it[0][2], it[1][2] / it[0][1]))
                lines.append(
                    "| %s | %s | %d | %.3f (%.3f..%.3f) | %.3f (%.3f..%.3f) | "
                    "%.3f (%.3f..%.3f) | %.3f |"
                    % ((name, label, k) + it[0] + it[1]
                       + (it[1][0] / it[0][0], lo, hi, (vec + 16 * M) / vec)))
                print(lines[-1], flush=True)
            if name != scaled:
                continue
            for k in (1, 4):
                for pre in (0, 1):
                    runs = sorted((solve(m, pre, k, MAXIT, 1e-8)
                                   for _ in range(3)), key=lambda r: r[0])
                    rec = runs[1][1]
                    to_tol.append(
                        "| %s | %d | %s | %s | %s | %.1f (%.1f..%.1f) |"
                        % (label, k, "pcg" if pre else "cg",
                           " ".join(str(r.iterations) for r in rec),
                           " ".join(str(r.status) for r in rec),
                           runs[1][0], runs[0][0], runs[2][0]))
                    print(to_tol[-1], flush=True)
        for _, m in hs:
            m.release()
        for b in (B, X, minv, work):
            b.free()
    argv = " --rows %d" % a.rows if a.rows != 10_000_000 else ""
    out = a.out or os.path.join(PROFILES, "pcg.md")
    with open(out, "w") as f:
        f.write(PCG_HEADER % (argv, SHORT, LONG, ROUNDS, LONG - SHORT,
                              VECTOR_PASSES, VECTOR_PASSES)
                + "\n".join(lines) + "\n" + TOL_HEADER % (MAXIT, 3)
                + "\n".join(to_tol) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
