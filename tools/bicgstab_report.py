#!/usr/bin/env python3
"""Measure the device-resident BiCGStab solver (bicgstab(), spmv_*_bicgstab)
and write profiles/bicgstab.md: milliseconds per iteration for k = 1, 4, 8
systems, without and with a diagonal preconditioner, beside TWO launch_multi
launches on the same handle in the same process (an iteration's two products:
the yardstick), beside the byte model, and the rate of the vector work.

Matrices (built on the host, nonsymmetric, they keep every column running):
  banded   row i holds K = 32 entries at columns s..s+31, s = clamp(i - 16)
           (the pattern of SYNTH_BANDED): 30.05 on the diagonal, -0.75 within
           15 columns above it, -1.25 within 15 columns below it, and the one
           stored entry beyond an explicit 0.0 -- 32 stored entries per row.
  stencil  5-point convection-diffusion on an n x n grid, n = sqrt(rows):
           diagonal 4.01, east -0.5, west -1.5, north and south -1 (tests/
           _bicgstab.py convdiff(n, n, 0.01, 0.5)).
tol = 0, so no column converges; every solve is checked to end with status 1
(maxit) and `maxit` iterations in every column.

Method.  launch_multi: ROUNDS rounds of 3 warm-ups and 10 launches between
two events, the median round and (min..max).  An iteration: the host clock
around the blocking solve (it ends in a stream synchronise) at maxit = SHORT
and at maxit = LONG with a supplied work buffer, ROUNDS times each in turns;
ms per iteration = (median LONG - median SHORT) / (LONG - SHORT), which takes
the set-up and the last copy-back out.  Byte model of an iteration:
2 multi_bytes(k) + 20 * 8 k M (+ 3 * 8 M with minv) -- the vector passes as
built: dot 2 reads; S 2 reads + 2 writes; ts/tt 2 reads; update 5 reads + 2
writes; direction 3 reads + 2 writes; minv is read by S, update and direction.
`vector TB/s` is the bytes of those passes over (iter ms - 2 multi ms): the
four finalising launches and every launch gap are charged to the vector work.

    python tools/bicgstab_report.py [--rows 10000000] [--out FILE]
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
VECTOR_PASSES = 20
MINV_READS = 3

HEADER = """# BiCGStab on the device: one iteration against its two products

Written by `tools/bicgstab_report.py%s` on one MI355X; what the numbers say is
in DESIGN.md section 18. f64 values. `2 multi ms` is twice `launch_multi` alone
on the same handle in the same process (median of %d rounds of 10 launches
between two events, min..max in brackets). `iter ms` is one iteration of
`bicgstab()`: the host clock around the blocking solve at maxit = %d and
maxit = %d with a supplied work buffer, %d rounds each in turns,
(median long - median short) / %d; the bracket is the same figure from the
fastest and the slowest pair of rounds. `minv`: none, or `diag(invert=True)`.
`bytes` is the byte model of an iteration over `2 multi_bytes(k)`:
(2 multi_bytes(k) + %d * 8 k M + minv * %d * 8 M) / (2 multi_bytes(k));
`model ms` prices the model at the rate `launch_multi` reached
(`2 multi ms` x `bytes`). `vector TB/s` is the vector passes' bytes over
(iter ms - 2 multi ms): finalising launches and launch gaps are charged to it.
tol = 0: every column runs all iterations (checked).

"""


def banded(M, K=32):
    """-> (IRP, JA, AS): the SYNTH_BANDED pattern, nonsymmetric values"""
    rows = np.arange(M, dtype=np.int32)
    start = np.clip(rows - K // 2, 0, M - K)
    JA = start[:, None] + np.arange(K, dtype=np.int32)[None, :]
    off = JA - rows[:, None]
    AS = np.where(off == 0, K - 2 + 0.05,
                  np.where(np.abs(off) >= K // 2, 0.0,
                           np.where(off > 0, -0.75, -1.25)))
    IRP = (np.arange(M + 1, dtype=np.int64) * K).astype(np.int32)
    return IRP, np.ascontiguousarray(JA).ravel(), AS.ravel()


def convdiff2d(n, shift=0.01, c=0.5):
    """-> (IRP, JA, AS) of the 5-point convection-diffusion stencil on an
    n x n grid: south, west, diagonal, east, north"""
    M = n * n
    i = np.arange(M, dtype=np.int64)
    ix, iy = i % n, i // n
    cand = np.stack([i - n, i - 1, i, i + 1, i + n], axis=1)
    ok = np.stack([iy > 0, ix > 0, np.ones(M, bool), ix < n - 1, iy < n - 1],
                  axis=1)
    vals = np.broadcast_to(
        np.array([-1.0, -1.0 - c, 4.0 + shift, -1.0 + c, -1.0]), (M, 5))
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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = int(round(a.rows ** 0.5))
    workloads = (("banded %gM x 32" % (a.rows / 1e6), a.rows,
                  lambda: banded(a.rows)),
                 ("convdiff %d x %d" % (n, n), n * n, lambda: convdiff2d(n)))
    lines = ["| matrix | handle | k | minv | 2 multi ms | iter ms | / 2 multi | "
             "bytes | model ms | iter / model | vector TB/s |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for name, M, build in workloads:
        IRP, JA, AS = build()
        A = S.csr_from_arrays("bicgstab_report", M, M, IRP, JA, AS)
        del IRP, JA, AS
        d = S.CsrDevice.upload(A)
        S.csr_free(A)
        hs = (("csr", d), ("hll", d.to_hll(True)))
        B, X = S.DevBuffer(M * 8 * 8), S.DevBuffer(M * 8 * 8)
        minv = S.DevBuffer(M * 8)
        work = S.DevBuffer(S.bicgstab_work_bytes(M, 8))
        S.dev_fill_synth(B.ptr, M * 8, 7)

        def solve(m, pre, k, maxit):
            S._check(S._lib.spmv_dev_memset(X.ptr, 0, M * k * 8, None),
                     "spmv_dev_memset")
            S.stream_sync()
            t0 = time.perf_counter()
            rec = m.bicgstab(B.ptr, X.ptr, k,
                             d_minv=minv.ptr if pre else None, tol=0.0,
                             maxit=maxit, work=work)
            ms = (time.perf_counter() - t0) * 1e3
            bad = [r for r in rec if (r.status, r.iterations) != (1, maxit)]
            if bad:
                raise SystemExit("%s k=%d minv=%d: a column stopped early: %r"
                                 % (name, k, pre, bad))
            return ms

        for label, m in hs:
            m.diag(minv.ptr, invert=True)
            S.stream_sync()
            for k in KS:
                for pre in (0, 1):
                    solve(m, pre, k, SHORT)  # warm-up of every kernel
                tm = sorted(2 * event_ms(
                    lambda: m.launch_multi(B.ptr, X.ptr, k))
                    for _ in range(ROUNDS))
                multi2 = tm[ROUNDS // 2]
                t = {(pre, n_it): [] for pre in (0, 1)
                     for n_it in (SHORT, LONG)}
                for _ in range(ROUNDS):
                    for pre in (0, 1):
                        for n_it in (SHORT, LONG):
                            t[pre, n_it].append(solve(m, pre, k, n_it))
                span = LONG - SHORT
                for pre in (0, 1):
                    ts, tl = sorted(t[pre, SHORT]), sorted(t[pre, LONG])
                    it = (tl[ROUNDS // 2] - ts[ROUNDS // 2]) / span
                    it_lo = (tl[0] - ts[0]) / span
                    it_hi = (tl[-1] - ts[-1]) / span
                    vec = VECTOR_PASSES * 8 * k * M + pre * MINV_READS * 8 * M
                    ratio = (2 * m.multi_bytes(k) + vec) / (2 * m.multi_bytes(k))
                    rate = vec / ((it - multi2) * 1e-3) / 1e12
                    lines.append(
                        "| %s | %s | %d | %s | %.3f (%.3f..%.3f) | "
                        "%.3f (%.3f..%.3f) | %.2f | %.2f | %.3f | %.2f | %.2f |"
                        % (name, label, k, "jacobi" if pre else "none", multi2,
                           tm[0], tm[-1], it, it_lo, it_hi, it / multi2, ratio,
                           multi2 * ratio, it / (multi2 * ratio), rate))
                    print(lines[-1], flush=True)
        for _, m in hs:
            m.release()
        for b in (B, X, minv, work):
            b.free()
    argv = " --rows %d" % a.rows if a.rows != 10_000_000 else ""
    out = a.out or os.path.join(PROFILES, "bicgstab.md")
    with open(out, "w") as f:
        f.write(HEADER % (argv, ROUNDS, SHORT, LONG, ROUNDS, LONG - SHORT,
                          VECTOR_PASSES, MINV_READS)
                + "\n".join(lines) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
