#!/usr/bin/env python3
"""Measure the device-resident CGLS solver (cgls(), spmv_*_cgls) and write
profiles/cgls.md: milliseconds per iteration for k = 1, 4, 8 problems, with
damp = 0 and damp = 0.5, for the CSR pair (A, AT) and the column-major HLL pair,
beside ONE launch_multi on A plus ONE on AT in the same process (an iteration's
two products: the yardstick), beside the byte model, and the rate of the
vector work.

Matrices (built on the host; AT = A.transpose() on the device):
  banded   square, row i holds K = 32 entries at columns s..s+31,
           s = clamp(i - 16) (the pattern of SYNTH_BANDED) with the
           nonsymmetric values of tools/bicgstab_report.py.
  tall     rows x rows/4: four such banded blocks of rows/4 rows stacked,
           block b scaled by 1 + b/4 -- 32 entries per row of A, 128 per row
           of AT.  M and N differ, so the M-long and the N-long passes are
           priced apart.
tol = 0, so no column converges; every solve is checked to end with status 1
(maxit) and `maxit` iterations in every column.

Method.  The products: ROUNDS rounds of 3 warm-ups and 10 launches of each
between two events, the median round and (min..max) of the sum.  An iteration:
the host clock around the blocking solve (it ends in a stream synchronise) at
maxit = SHORT and at maxit = LONG with a supplied work buffer, ROUNDS times
each in turns; ms per iteration = (median LONG - median SHORT) / (LONG -
SHORT), which takes the set-up and the last copy-back out.  Byte model of an
iteration: multi_bytes(A, k) + multi_bytes(AT, k) + 8 k (4 M + 7 N), with
damping 8 k (4 M + 9 N) -- the vector passes as built: Q.Q 1 read (M); update
2 reads + 1 write (N) and 2 reads + 1 write (M); S.S 1 read (N), with damping
S - d2 X in the same pass, 2 reads + 1 write (N); direction 2 reads + 1 write
(N).  `vector TB/s` is the bytes of those passes over (iter ms - products ms):
the two finalising launches and every launch gap are charged to the vector
work.

    python tools/cgls_report.py [--rows 10000000] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import spmv_scpa_amd as S  # noqa: E402
from bicgstab_report import banded, event_ms  # noqa: E402

PROFILES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                        "profiles")
KS = (1, 4, 8)
DAMPS = (0.0, 0.5)
ROUNDS = 5
SHORT, LONG = 8, 48

HEADER = """# CGLS on the device: one iteration against its two products

Written by `tools/cgls_report.py%s` on one MI355X; what the numbers say is in
DESIGN.md section 20. f64 values; `AT` is `A.transpose()`, the HLL pair is made
from the CSR pair. `products ms` is one `launch_multi` on `A` plus one on `AT`
in the same process (median of %d rounds of 10 launches each between two
events, min..max in brackets). `iter ms` is one iteration of `cgls()`: the
host clock around the blocking solve at maxit = %d and maxit = %d with a
supplied work buffer, %d rounds each in turns, (median long - median short) /
%d; the bracket is the same figure from the fastest and the slowest pair of
rounds. `bytes` is the byte model of an iteration over the products' bytes:
(multi_bytes(A, k) + multi_bytes(AT, k) + 8 k (4 M + 7 N)) / (multi_bytes(A, k)
+ multi_bytes(AT, k)), 9 N with damping; `model ms` prices the model at the
rate the products reached (`products ms` x `bytes`). `vector TB/s` is the
vector passes' bytes over (iter ms - products ms): finalising launches and
launch gaps are charged to it. tol = 0: every column runs all iterations
(checked).

"""


def tall(rows, blocks=4):
    """-> (M, N, IRP, JA, AS): `blocks` banded blocks of rows / blocks rows
    stacked, block b scaled by 1 + b / blocks"""
    n = rows // blocks
    IRP1, JA1, AS1 = banded(n)
    K = int(IRP1[1])
    M = n * blocks
    IRP = (np.arange(M + 1, dtype=np.int64) * K).astype(np.int32)
    JA = np.tile(JA1, blocks)
    AS = np.concatenate([AS1 * (1.0 + b / blocks) for b in range(blocks)])
    return M, n, IRP, JA, AS


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    workloads = (("banded %gM x 32" % (a.rows / 1e6),
                  lambda: (a.rows, a.rows) + banded(a.rows)),
                 ("tall %gM x %gM" % (a.rows / 1e6, a.rows / 4e6),
                  lambda: tall(a.rows)))
    lines = ["| matrix | pair | k | damp | products ms | iter ms | / products | "
             "bytes | model ms | iter / model | vector TB/s |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for name, build in workloads:
        M, N, IRP, JA, AS = build()
        A = S.csr_from_arrays("cgls_report", M, N, IRP, JA, AS)
        del IRP, JA, AS
        d = S.CsrDevice.upload(A)
        S.csr_free(A)
        dt = d.transpose()
        print(name, "uploaded and transposed", flush=True)
        pairs = (("csr", d, dt), ("hll", d.to_hll(True), dt.to_hll(True)))
        L = max(M, N)
        B, X = S.DevBuffer(L * 8 * 8), S.DevBuffer(L * 8 * 8)
        work = S.DevBuffer(S.cgls_work_bytes(M, N, 8))
        S.dev_fill_synth(B.ptr, L * 8, 7)

        def solve(m, mt, damp, k, maxit):
            S._check(S._lib.spmv_dev_memset(X.ptr, 0, N * k * 8, None),
                     "spmv_dev_memset")
            S.stream_sync()
            t0 = time.perf_counter()
            rec = m.cgls(mt, B.ptr, X.ptr, k, damp=damp, tol=0.0, maxit=maxit,
                         work=work)
            ms = (time.perf_counter() - t0) * 1e3
            bad = [r for r in rec if (r.status, r.iterations) != (1, maxit)]
            if bad:
                raise SystemExit("%s k=%d damp=%g: a column stopped early: %r"
                                 % (name, k, damp, bad))
            return ms

        for label, m, mt in pairs:
            for k in KS:
                for damp in DAMPS:
                    solve(m, mt, damp, k, SHORT)  # warm-up of every kernel
                # B stands in for the N-long input too: only the time counts
                tm = sorted(
                    event_ms(lambda: m.launch_multi(B.ptr, X.ptr, k)) +
                    event_ms(lambda: mt.launch_multi(B.ptr, X.ptr, k))
                    for _ in range(ROUNDS))
                prod = tm[ROUNDS // 2]
                t = {(damp, n_it): [] for damp in DAMPS
                     for n_it in (SHORT, LONG)}
                for _ in range(ROUNDS):
                    for damp in DAMPS:
                        for n_it in (SHORT, LONG):
                            t[damp, n_it].append(solve(m, mt, damp, k, n_it))
                span = LONG - SHORT
                pb = m.multi_bytes(k) + mt.multi_bytes(k)
                for damp in DAMPS:
                    ts, tl = sorted(t[damp, SHORT]), sorted(t[damp, LONG])
                    it = (tl[ROUNDS // 2] - ts[ROUNDS // 2]) / span
                    it_lo = (tl[0] - ts[0]) / span
                    it_hi = (tl[-1] - ts[-1]) / span
                    vec = 8 * k * (4 * M + (9 if damp else 7) * N)
                    ratio = (pb + vec) / pb
                    rate = vec / ((it - prod) * 1e-3) / 1e12
                    lines.append(
                        "| %s | %s | %d | %g | %.3f (%.3f..%.3f) | "
                        "%.3f (%.3f..%.3f) | %.2f | %.2f | %.3f | %.2f | %.2f |"
                        % (name, label, k, damp, prod, tm[0], tm[-1], it,
                           it_lo, it_hi, it / prod, ratio, prod * ratio,
                           it / (prod * ratio), rate))
                    print(lines[-1], flush=True)
        for _, m, mt in pairs:
            m.release()
            mt.release()
        for b in (B, X, work):
            b.free()
    argv = " --rows %d" % a.rows if a.rows != 10_000_000 else ""
    out = a.out or os.path.join(PROFILES, "cgls.md")
    with open(out, "w") as f:
        f.write(HEADER % (argv, ROUNDS, SHORT, LONG, ROUNDS, LONG - SHORT)
                + "\n".join(lines) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
