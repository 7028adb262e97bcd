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
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import spmv_scpa_amd as S  # noqa: E402

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
    ap.add_argument("--out", default=os.path.join(
        os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "cg.md"))
    a = ap.parse_args()
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
    with open(a.out, "w") as f:
        f.write(HEADER % (argv, ROUNDS, SHORT, LONG, ROUNDS, LONG - SHORT,
                          VECTOR_PASSES, LONG, ROUNDS)
                + "\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
