#!/usr/bin/env python3
"""Measure the device-resident MINRES solver (minres(), spmv_*_minres) and
write profiles/minres.md: milliseconds per iteration for k = 1, 4, 8 systems,
without and with minv = diag(invert=True), on CSR and column-major HLL
handles, beside ONE launch_multi on the same handle in the same process (an
iteration's one product: the yardstick), beside the byte model and the rate of
the vector work -- and beside one iteration of bicgstab() on the same handle,
the solver a symmetric indefinite system had to use before.

Matrices (built on the host): the symmetric-valued `banded` and the 2-D
stencil of tools/cg_report.py.  Both are positive definite: what is timed is
the iteration, which does not look at the signs.  tol = 0, so no column
converges; every solve is checked to end with status 1 (maxit) and `maxit`
iterations in every column.

Method (that of tools/cgls_report.py).  launch_multi: ROUNDS rounds of 3
warm-ups and 10 launches between two events, the median round and (min..max).
An iteration: the host clock around the blocking solve (it ends in a stream
synchronise) at maxit = SHORT and at maxit = LONG with a supplied work buffer,
ROUNDS times each in turns, the two solvers in turns; ms per iteration =
(median LONG - median SHORT) / (LONG - SHORT), which takes the set-up and the
closing residual out.  Byte model of an iteration: multi_bytes(k) +
15 * 8 k M (+ 2 * 8 M with minv) -- the vector passes as launched: V 1 read +
1 write; orth 3 reads + 1 write; res 2 reads + 1 write; step 4 reads +
2 writes; minv is read by V and by res.  `vector TB/s` is the bytes of those
passes over (iter ms - multi ms): the two finalising launches and every launch
gap are charged to the vector work.

Then one solve to tol = 1e-8 on the shifted 2-D stencil (diagonal 4 - sigma:
symmetric indefinite), minres() and bicgstab(): iterations, status and wall
time as measured.

    python tools/minres_report.py [--rows 10000000] [--grid 256] [--out FILE]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import spmv_scpa_amd as S  # noqa: E402
from cg_report import banded, event_ms, stencil2d  # noqa: E402

PROFILES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                        "profiles")
KS = (1, 4, 8)
ROUNDS = 5
SHORT, LONG = 8, 48
VECTOR_PASSES = 15
MINV_READS = 2
BI_PASSES = 20
SIGMA = 1.3
TOL_MAXIT = 40000

HEADER = """# MINRES on the device: one iteration against its product, and BiCGStab

Written by `tools/minres_report.py%s` on one MI355X; what the numbers say is in
DESIGN.md section 21. f64 values. `multi ms` is `launch_multi` alone on the same
handle in the same process (median of %d rounds of 10 launches between two
events, min..max in brackets). `iter ms` is one iteration of `minres()`: the
host clock around the blocking solve at maxit = %d and maxit = %d with a
supplied work buffer, %d rounds each in turns, (median long - median short) /
%d; the bracket is the same figure from the fastest and the slowest pair of
rounds. `minv`: none, or `diag(invert=True)`. `bytes` is the byte model of an
iteration over `multi_bytes(k)`: (multi_bytes(k) + %d * 8 k M + minv * %d * 8 M)
/ multi_bytes(k); `model ms` prices the model at the rate `launch_multi`
reached (`multi ms` x `bytes`). `vector TB/s` is the vector passes' bytes over
(iter ms - multi ms): finalising launches and launch gaps are charged to it.
`bicgstab ms` is one iteration of `bicgstab()` on the same handle by the same
method, its rounds taken in turns with those of `minres()` (two products and
%d vector passes); `/ bicgstab` is the ratio of the two medians. tol = 0: every
column runs all iterations (checked).

"""

TOL_HEADER = """
## To tol = 1e-8 on a shifted stencil

The 5-point stencil with diagonal 4 - %g on a %d x %d grid: symmetric
indefinite. B = the synthetic vector the rows above use, X0 = 0, no minv,
check_every = 8, maxit = %d. `iterations` and `status` per column (0 converged,
1 maxit, 2 breakdown); `true residual` is sqrt(rr / bb) per column, from the
closing residual for `minres()` and from the recurrence's for `bicgstab()`;
`ms` is the host wall time of the whole solve (median of %d, min..max).

"""


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = int(round(a.rows ** 0.5))
    workloads = (("banded %gM x 32" % (a.rows / 1e6), a.rows,
                  lambda: banded(a.rows)),
                 ("2-D stencil %d x %d" % (n, n), n * n, lambda: stencil2d(n)))
    lines = ["| matrix | handle | k | minv | multi ms | iter ms | / multi | "
             "bytes | model ms | iter / model | vector TB/s | bicgstab ms | "
             "/ bicgstab |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for name, M, build in workloads:
        IRP, JA, AS = build()
        A = S.csr_from_arrays("minres_report", M, M, IRP, JA, AS)
        del IRP, JA, AS
        d = S.CsrDevice.upload(A)
        S.csr_free(A)
        hs = (("csr", d), ("hll", d.to_hll(True)))
        B, X = S.DevBuffer(M * 8 * 8), S.DevBuffer(M * 8 * 8)
        minv = S.DevBuffer(M * 8)
        work = S.DevBuffer(max(S.minres_work_bytes(M, 8),
                               S.bicgstab_work_bytes(M, 8)))
        S.dev_fill_synth(B.ptr, M * 8, 7)
        print(name, "uploaded", flush=True)

        def solve(m, solver, pre, k, maxit):
            S._check(S._lib.spmv_dev_memset(X.ptr, 0, M * k * 8, None),
                     "spmv_dev_memset")
            S.stream_sync()
            fn = m.minres if solver == "minres" else m.bicgstab
            t0 = time.perf_counter()
            rec = fn(B.ptr, X.ptr, k, d_minv=minv.ptr if pre else None,
                     tol=0.0, maxit=maxit, work=work)
            ms = (time.perf_counter() - t0) * 1e3
            bad = [r for r in rec if (r.status, r.iterations) != (1, maxit)]
            if bad:
                raise SystemExit("%s %s k=%d minv=%d: a column stopped early: "
                                 "%r" % (name, solver, k, pre, bad))
            return ms

        for label, m in hs:
            m.diag(minv.ptr, invert=True)
            S.stream_sync()
            for k in KS:
                cells = [(s, pre) for s in ("minres", "bicgstab")
                         for pre in (0, 1)]
                for s, pre in cells:
                    solve(m, s, pre, k, SHORT)  # warm-up of every kernel
                tm = sorted(event_ms(
                    lambda: m.launch_multi(B.ptr, X.ptr, k))
                    for _ in range(ROUNDS))
                multi = tm[ROUNDS // 2]
                t = {c + (n_it,): [] for c in cells for n_it in (SHORT, LONG)}
                for _ in range(ROUNDS):
                    for s, pre in cells:
                        for n_it in (SHORT, LONG):
                            t[s, pre, n_it].append(solve(m, s, pre, k, n_it))
                span = LONG - SHORT
                it = {}
                for c in cells:
                    ts, tl = sorted(t[c + (SHORT,)]), sorted(t[c + (LONG,)])
                    it[c] = ((tl[ROUNDS // 2] - ts[ROUNDS // 2]) / span,
                             (tl[0] - ts[0]) / span, (tl[-1] - ts[-1]) / span)
                mb = m.multi_bytes(k)
                for pre in (0, 1):
                    mr, bi = it["minres", pre], it["bicgstab", pre]
                    vec = VECTOR_PASSES * 8 * k * M + pre * MINV_READS * 8 * M
                    ratio = (mb + vec) / mb
                    rate = vec / ((mr[0] - multi) * 1e-3) / 1e12
                    lines.append(
                        "| %s | %s | %d | %s | %.3f (%.3f..%.3f) | "
                        "%.3f (%.3f..%.3f) | %.2f | %.2f | %.3f | %.2f | %.2f | "
                        "%.3f (%.3f..%.3f) | %.2f |"
                        % (name, label, k, "jacobi" if pre else "none", multi,
                           tm[0], tm[-1], mr[0], mr[1], mr[2], mr[0] / multi,
                           ratio, multi * ratio, mr[0] / (multi * ratio), rate,
                           bi[0], bi[1], bi[2], mr[0] / bi[0]))
                    print(lines[-1], flush=True)
        for _, m in hs:
            m.release()
        for b in (B, X, minv, work):
            b.free()

    # one solve to tol = 1e-8 where CG cannot go
    g = a.grid
    M = g * g
    IRP, JA, AS = stencil2d(g, -SIGMA)
    A = S.csr_from_arrays("minres_report_shifted", M, M, IRP, JA, AS)
    d = S.CsrDevice.upload(A)
    S.csr_free(A)
    hs = (("csr", d), ("hll", d.to_hll(True)))
    B, X = S.DevBuffer(M * 8 * 8), S.DevBuffer(M * 8 * 8)
    S.dev_fill_synth(B.ptr, M * 8, 7)
    to_tol = ["| handle | k | solver | iterations | status | true residual | "
              "ms |", "|---|---|---|---|---|---|---|"]
    RUNS = 3
    for label, m in hs:
        for k in (1, 4):
            for solver in ("minres", "bicgstab"):
                fn = m.minres if solver == "minres" else m.bicgstab
                runs = []
                for _ in range(RUNS):
                    S._check(S._lib.spmv_dev_memset(X.ptr, 0, M * k * 8, None),
                             "spmv_dev_memset")
                    S.stream_sync()
                    t0 = time.perf_counter()
                    rec = fn(B.ptr, X.ptr, k, tol=1e-8, maxit=TOL_MAXIT)
                    runs.append(((time.perf_counter() - t0) * 1e3, rec))
                runs.sort(key=lambda r: r[0])
                rec = runs[RUNS // 2][1]
                to_tol.append(
                    "| %s | %d | %s | %s | %s | %s | %.1f (%.1f..%.1f) |"
                    % (label, k, solver,
                       " ".join(str(r.iterations) for r in rec),
                       " ".join(str(r.status) for r in rec),
                       " ".join("%.2e" % ((r.rr / r.bb) ** 0.5
                                          if r.bb > 0 and r.rr >= 0
                                          else float("nan")) for r in rec),
                       runs[RUNS // 2][0], runs[0][0], runs[-1][0]))
                print(to_tol[-1], flush=True)
    for _, m in hs:
        m.release()
    for b in (B, X):
        b.free()

    argv = (" --rows %d" % a.rows if a.rows != 10_000_000 else "") + \
        (" --grid %d" % a.grid if a.grid != 256 else "")
    out = a.out or os.path.join(PROFILES, "minres.md")
    with open(out, "w") as f:
        f.write(HEADER % (argv, ROUNDS, SHORT, LONG, ROUNDS, LONG - SHORT,
                          VECTOR_PASSES, MINV_READS, BI_PASSES)
                + "\n".join(lines) + "\n"
                + TOL_HEADER % (SIGMA, g, g, TOL_MAXIT, RUNS)
                + "\n".join(to_tol) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
