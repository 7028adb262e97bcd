#!/usr/bin/env python3
"""Time sweep plans (spmv_csr_trsv_analyse_sweeps) and print the table rows of
profiles/trsv_sweeps.md.  One process per call, one matrix per process.

    --what sweep   one Jacobi sweep against its bytes: the lower triangle of
                   the matrix as a sweep plan, k = 1 / 4 / 8.  T(s) is the
                   median over --reps solves of a plan of s sweeps between two
                   events; one sweep = (T(13) - T(5)) / 8, the first sweep =
                   T(1).  The yardstick is launch_multi on a CSR handle that
                   holds the same strict triangle, timed the same way.
    --what solve   end to end: Jacobi, exact plans in natural and in
                   multicolour order, sweep plans of 2..5 sweeps in natural
                   order.  stencil5 / stencil27: pcg / pcg_trsv with IC(0);
                   convdiff: bicgstab / bicgstab_trsv with ILU(0).  setup =
                   the two analyses (blocking calls, host clock); ms per
                   iteration = (T(3 n) - T(n)) / (2 n) from solves of exactly
                   m iterations (tol = 0); solve = to tol 1e-8 from X = 0.
    --what exact   the exact plan's solve at k = 1 / 4 / 8 in natural and in
                   multicolour order.  --package DIR imports spmv_scpa_amd
                   (binding and library) from DIR, another checkout built
                   there: run the two alternately to compare two commits.

Matrices: stencil5 (5-point, n^2 points, diagonal 4.01), stencil27 (27-point,
m^3 points, diagonal 26.5) as tools/colour_report.py builds them; convdiff
(5-point convection-diffusion, n^2 points) as tools/ilu0_report.py builds it.
Nothing is asserted about speed.

    python tools/trsv_sweeps_report.py --what solve --matrix stencil5
                                       [--n 3162] [--m 215] [--reps 3]
"""
import argparse
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from colour_report import host_ms, stencil, upload  # noqa: E402

SWEEPS = (2, 3, 4, 5)


def make(a):
    if a.matrix == "stencil5":
        return "5-point, %d^2" % a.n, stencil((a.n, a.n), 4.01)
    if a.matrix == "stencil27":
        return "27-point, %d^3" % a.m, stencil((a.m,) * 3, 26.5)
    import ilu0_report as IR
    args = types.SimpleNamespace(n=a.n, m=a.m)
    return ("convdiff, %d^2" % a.n,
            IR.matrix(IR.grid("convdiff", args), 0.01, 0.5))


def strict_lower(mat):
    M, IRP, JA, AS = mat
    keep = JA < np.repeat(np.arange(M, dtype=np.int32), np.diff(IRP))
    rows = np.repeat(np.arange(M), np.diff(IRP))[keep]
    out = np.zeros(M + 1, np.int32)
    out[1:] = np.cumsum(np.bincount(rows, minlength=M))
    return M, out, JA[keep], AS[keep]


def med(v):
    return float(np.median(v))


def span(v):
    return "%.3f (%.3f .. %.3f)" % (med(v), min(v), max(v))


class Timer:
    def __init__(self, S):
        self.S, self.st = S, S.Stream()

    def ms(self, fn, reps, warm=2):
        out = []
        for i in range(warm + reps):
            a, b = self.S.Event(), self.S.Event()
            a.record(self.st.ptr)
            fn()
            b.record(self.st.ptr)
            self.S.stream_sync(self.st.ptr)
            if i >= warm:
                out.append(a.elapsed_ms(b))
        return out


# ----------------------------------------------------------------- sweep
def what_sweep(S, a):
    label, mat = make(a)
    low = strict_lower(mat)
    M, entries = mat[0], len(low[2])
    d, dL = upload(S, mat), upload(S, low)
    del mat, low
    tm = Timer(S)
    d_B, d_X = S.DevBuffer(M * 8 * 8), S.DevBuffer(M * 8 * 8)
    S.dev_fill_synth(d_B.ptr, M * 8, 7)
    S.stream_sync()
    plans = {s: d.trsv_analyse("lower", sweeps=s) for s in (1, 5, 13)}
    vb = d.value_bytes
    print("| matrix | rows | strict entries | k | one sweep ms | model bytes "
          "| model GB/s | first sweep ms | launch_multi ms (same triangle) | "
          "sweep / launch_multi |\n|---|---|---|---|---|---|---|---|---|---|")
    for k in (1, 4, 8):
        t = {s: tm.ms(lambda: p.solve(d_B.ptr, d_X.ptr, k, stream=tm.st.ptr),
                      a.reps) for s, p in plans.items()}
        one = (med(t[13]) - med(t[5])) / 8
        lm = tm.ms(lambda: dL.launch_multi(d_B.ptr, d_X.ptr, k,
                                           stream=tm.st.ptr), a.reps)
        model = entries * (4 + vb) + 4 * (M + 1) + 8 * M + 3 * 8 * k * M
        print("T(1) %s T(5) %s T(13) %s launch_multi %s"
              % (span(t[1]), span(t[5]), span(t[13]), span(lm)),
              file=sys.stderr, flush=True)
        print("| %s | %d | %d | %d | %.3f | %d | %.0f | %.3f | %.3f | %.2f |"
              % (label, M, entries, k, one, model, model / one / 1e6,
                 med(t[1]), med(lm), one / med(lm)), flush=True)


# ----------------------------------------------------------------- solve
def what_solve(S, a):
    label, mat = make(a)
    M = mat[0]
    sym = a.matrix != "convdiff"
    d = upload(S, mat)
    del mat
    tm = Timer(S)
    st = tm.st
    d_B, d_PB, d_X = (S.DevBuffer(M * 8) for _ in range(3))
    S.dev_fill_synth(d_B.ptr, M, 7)
    S.stream_sync()

    def factor(h):
        """-> (lower handle, upper handle, unit of the lower plan, owned)"""
        if sym:
            L = h.ic0()[0]
            LT = L.transpose()
            return L, LT, False, (L, LT)
        LU = h.ilu0()[0]
        return LU, LU, True, (LU,)

    def plans(h, **kw):
        """the two plans of h's factor and the ms of the two analyses alone"""
        lo_h, up_h, unit, own = factor(h)
        made = []
        setup = host_ms(lambda: made.append(
            (lo_h.trsv_analyse("lower", unit=unit, **kw),
             up_h.trsv_analyse("upper", **kw))), 1 + a.reps)[1:]
        for lo, up in made[:-1]:
            lo.release()
            up.release()
        for f in own:
            f.release()
        return made[-1] + (setup,)

    def solve_ms(run, maxit, tol):
        S._check(S._lib.spmv_dev_memset(d_X.ptr, 0, M * 8, st.ptr), "memset")
        e0, e1 = S.Event(), S.Event()
        e0.record(st.ptr)
        rec = run(maxit, tol)[0]
        e1.record(st.ptr)
        S.stream_sync(st.ptr)
        return e0.elapsed_ms(e1), rec

    base = []

    def measure(name, launches, setup, run, n_iter):
        solve_ms(run, 2, 0.0)  # warm-up: code objects, the allocator
        t = {m: med([solve_ms(run, m, 0.0)[0] for _ in range(a.reps)])
             for m in (n_iter, 3 * n_iter)}
        per_it = (t[3 * n_iter] - t[n_iter]) / (2 * n_iter)
        full = [solve_ms(run, 100000, 1e-8) for _ in range(a.reps)]
        ms, rec = [f[0] for f in full], full[-1][1]
        base.append(med(ms))
        print(name, t, ms, rec, file=sys.stderr, flush=True)
        print("| %s | %s | %s | %s | %.3f | %d%s | %.1f (%.1f .. %.1f) | %.2f |"
              % (label, name, launches,
                 "%.1f" % med(setup) if setup else "", per_it, rec.iterations,
                 "" if rec.status == 0 else " (status %d)" % rec.status,
                 med(ms), min(ms), max(ms), med(ms) / base[0]), flush=True)

    def plain(h, B):
        d_minv = S.DevBuffer(M * 8)
        h.diag(d_minv.ptr, invert=True)
        S.stream_sync()
        if sym:
            return d_minv, lambda maxit, tol: h.pcg(
                B.ptr, d_X.ptr, d_minv.ptr, 1, tol=tol, maxit=maxit,
                check_every=64, stream=st.ptr)
        return d_minv, lambda maxit, tol: h.bicgstab(
            B.ptr, d_X.ptr, d_minv=d_minv.ptr, k=1, tol=tol, maxit=maxit,
            check_every=64, stream=st.ptr)

    def with_plans(h, B, lo, up):
        fn = h.pcg_trsv if sym else h.bicgstab_trsv
        return lambda maxit, tol: fn(B.ptr, d_X.ptr, lo, up, k=1, tol=tol,
                                     maxit=maxit, check_every=64,
                                     stream=st.ptr)

    print("| matrix | preconditioner | launches per apply | two analyses ms | "
          "ms per iteration | iterations to 1e-8 | solve ms (min .. max) | "
          "solve / Jacobi |\n|---|---|---|---|---|---|---|---|")
    kind = "IC(0)" if sym else "ILU(0)"
    d_minv, run = plain(d, d_B)
    measure("Jacobi", 0, None, run, 8)
    d_minv.free()
    for s in SWEEPS:
        lo, up, setup = plans(d, sweeps=s, kmax=1)
        measure("%s, %d sweeps, natural" % (kind, s),
                lo.info["launches"] + up.info["launches"], setup,
                with_plans(d, d_B, lo, up), 8)
        lo.release()
        up.release()
    if not a.skip_exact:
        lo, up, setup = plans(d)
        measure("%s, exact, natural" % kind,
                lo.info["launches"] + up.info["launches"], setup,
                with_plans(d, d_B, lo, up), 2)
        lo.release()
        up.release()
    col = d.colour()
    dP = d.permute(col, col)
    S.permute_vectors(col, d_B, d_PB, M)
    S.stream_sync()
    lo, up, setup = plans(dP)
    measure("%s, exact, multicolour (%d colours)" % (kind, col.colours),
            lo.info["launches"] + up.info["launches"], setup,
            with_plans(dP, d_PB, lo, up), 8)


# ----------------------------------------------------------------- exact
def what_exact(S, a):
    label, mat = make(a)
    M = mat[0]
    d = upload(S, mat)
    del mat
    tm = Timer(S)
    d_B, d_X = S.DevBuffer(M * 8 * 8), S.DevBuffer(M * 8 * 8)
    S.dev_fill_synth(d_B.ptr, M * 8, 7)
    S.stream_sync()
    col = d.colour()
    dP = d.permute(col, col)
    lib = a.package or "this build"
    for order, h in (("natural", d), ("multicolour", dP)):
        plan = h.trsv_analyse("lower")
        for k in (1, 4, 8):
            t = tm.ms(lambda: plan.solve(d_B.ptr, d_X.ptr, k,
                                         stream=tm.st.ptr), a.reps)
            print("| %s | %s | %d | %d | %s | %s |"
                  % (label, order, plan.info["launches"], k, span(t), lib),
                  flush=True)
        plan.release()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--what", choices=("sweep", "solve", "exact"),
                    required=True)
    ap.add_argument("--matrix", choices=("stencil5", "stencil27", "convdiff"),
                    default="stencil5")
    ap.add_argument("--n", type=int, default=3162)
    ap.add_argument("--m", type=int, default=215)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-exact", action="store_true",
                    help="solve: leave out the exact plans in natural order "
                         "(thousands of launches per apply)")
    ap.add_argument("--package", default="",
                    help="exact: the directory to import spmv_scpa_amd from")
    a = ap.parse_args()
    if a.package:
        sys.path.insert(0, os.path.abspath(a.package))
    import spmv_scpa_amd as S
    if S.device_count() == 0:
        raise SystemExit("no GPU: nothing can be timed here")
    t0 = time.perf_counter()
    {"sweep": what_sweep, "solve": what_solve, "exact": what_exact}[a.what](
        S, a)
    print("%.0f s" % (time.perf_counter() - t0), file=sys.stderr)


if __name__ == "__main__":
    main()
