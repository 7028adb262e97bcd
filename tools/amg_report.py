#!/usr/bin/env python
"""Measure smoothed-aggregation AMG on one GPU: the setup by phase, one V
cycle, pcg_amg against Jacobi pcg in the same process (profiles/amg.md).

For each matrix and k = 1 / 4 / 8 right-hand sides (device-filled, X0 = 0):
  setup        host-clock ms of CsrDevice.amg() (median), its phases
               (spmv_amg_last_phases), levels, rows, operator complexity
  apply        event ms of one H.apply(k) and of one launch_multi(k) of the
               fine matrix
  per iter     (T(3 n) - T(n)) / 2 n of solves stopped by maxit
  solve        event ms of the whole solve to tol = 1e-8, iterations
  payback      setup / (Jacobi solve - AMG solve): the solves after which the
               hierarchy has paid for itself (inf: never)

--what sweep: ONE sweep on level 0, fused against composed.  Two hierarchies
of one level (max_levels = 1) with coarse_sweeps 1 and 9: their cycles differ
by exactly eight sweeps, so a sweep is (T(9) - T(1)) / 8 -- once with the fused
kernel (amg_set_fused(2)) and once with the composition (amg_set_fused(0):
launch_axpby(-1, 1) into r and the vector kernel); beside them one
launch_axpby(-1, 1) and one launch_multi of the same handle.  Event ms, two
warm-ups and 2 * reps + 1 launches, medians.

Usage (repository root, one MI355X):
    python tools/amg_report.py [--what solve|sweep] [--only stencil5,stencil27]
                               [--n5 3162] [--n27 215] [--reps 3] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from colour_report import host_ms, stencil, upload  # noqa: E402


def med(v):
    return float(np.median(v))


def event_ms(S, st, fn, reps, warm=1):
    out = []
    for i in range(warm + reps):
        a, b = S.Event(), S.Event()
        a.record(st.ptr)
        fn()
        b.record(st.ptr)
        S.stream_sync(st.ptr)
        if i >= warm:
            out.append(a.elapsed_ms(b))
    return out


def one(S, label, mat, reps, out):
    M, NZ = mat[0], len(mat[2])
    d = upload(S, mat)
    del mat
    st = S.Stream()
    made = []
    setup = host_ms(lambda: made.append(d.amg()), 1 + reps)[1:]
    for H in made[:-1]:
        H.release()
    H = made[-1]
    info, ph = H.info, S.amg_last_phases()
    out("\n### %s (%d rows, %d entries)\n" % (label, M, NZ))
    out("setup %.1f ms (%.1f .. %.1f); phases of the last one: %s\n"
        % (med(setup), min(setup), max(setup),
           ", ".join("%s %.1f" % kv for kv in ph.items())))
    out("levels %d, rows %s, entries %s, rounds %s, operator complexity %.3f, "
        "launches per apply %d, scratch %.0f MB\n"
        % (info["levels"], info["rows"], info["entries"], info["rounds"],
           info["complexity"], info["launches"], info["scratch_bytes"] / 1e6))
    minv = S.DevBuffer(M * 8)
    d.diag(minv.ptr, invert=True)
    S.stream_sync()
    d_B, d_X, d_Z = (S.DevBuffer(M * 8 * 8) for _ in range(3))
    work = S.DevBuffer(S.pcg_trsv_work_bytes(M, 8))
    out("| k | apply ms | launch_multi ms | apply / launch_multi | pcg_amg "
        "ms/iter | pcg ms/iter | pcg_amg iterations | pcg iterations | pcg_amg "
        "solve ms | pcg solve ms | pcg / pcg_amg | solves to pay the setup "
        "|\n|---|---|---|---|---|---|---|---|---|---|---|---|")
    for k in (1, 4, 8):
        S.dev_fill_synth(d_B.ptr, M * k, 7)
        S.stream_sync()
        ap = event_ms(S, st, lambda: H.apply(d_B.ptr, d_Z.ptr, k,
                                             stream=st.ptr), reps)
        lm = event_ms(S, st, lambda: d.launch_multi(d_B.ptr, d_Z.ptr, k,
                                                    stream=st.ptr), reps)

        def run(which, maxit, tol):
            S._check(S._lib.spmv_dev_memset(d_X.ptr, 0, M * k * 8, st.ptr),
                     "memset")
            kw = dict(k=k, tol=tol, maxit=maxit, work=work, stream=st.ptr)
            e0, e1 = S.Event(), S.Event()
            e0.record(st.ptr)
            rec = (d.pcg_amg(d_B.ptr, d_X.ptr, H, **kw) if which == "amg"
                   else d.pcg(d_B.ptr, d_X.ptr, minv.ptr, **kw))
            e1.record(st.ptr)
            S.stream_sync(st.ptr)
            return e0.elapsed_ms(e1), rec

        row = {}
        for which, n in (("amg", 5), ("jacobi", 40)):
            run(which, 2, 0.0)
            t = {m: med([run(which, m, 0.0)[0] for _ in range(reps)])
                 for m in (n, 3 * n)}
            full = [run(which, 100000, 1e-8) for _ in range(reps)]
            rec = full[-1][1]
            row[which] = ((t[3 * n] - t[n]) / (2 * n),
                          max(r.iterations for r in rec),
                          med([f[0] for f in full]),
                          sorted(set(r.status for r in rec)))
            print(label, k, which, t, [f[0] for f in full],
                  [(r.status, r.iterations) for r in rec], file=sys.stderr,
                  flush=True)
        a, j = row["amg"], row["jacobi"]
        gain = j[2] - a[2]
        out("| %d | %.3f | %.3f | %.1f | %.3f | %.3f | %d%s | %d%s | %.1f | "
            "%.1f | %.2f | %s |"
            % (k, med(ap), med(lm), med(ap) / med(lm), a[0], j[0], a[1],
               "" if a[3] == [0] else " (status %s)" % a[3], j[1],
               "" if j[3] == [0] else " (status %s)" % j[3], a[2], j[2],
               j[2] / a[2],
               "%.1f" % (med(setup) / gain) if gain > 0 else "never"))
    H.release()
    for b in (minv, d_B, d_X, d_Z, work):
        b.free()
    d.release()


def sweep(S, label, mat, reps, out):
    M = mat[0]
    d = upload(S, mat)
    del mat
    st = S.Stream()
    H1 = d.amg(max_levels=1, coarse_sweeps=1)
    H9 = d.amg(max_levels=1, coarse_sweeps=9)
    B, Z = S.DevBuffer(M * 64), S.DevBuffer(M * 64)
    S.dev_fill_synth(B.ptr, M * 8, 7)
    S.stream_sync()
    n = 2 * reps + 1
    for k in (1, 4, 8):
        one_ms = {}
        for fused in (True, False):
            S.amg_set_fused(2 if fused else 0)
            t1, t9 = (med(event_ms(S, st, lambda: H.apply(
                B.ptr, Z.ptr, k, stream=st.ptr), n, 2)) for H in (H1, H9))
            one_ms[fused] = (t9 - t1) / 8
            print(label, k, "fused" if fused else "composed", t1, t9,
                  file=sys.stderr, flush=True)
        S.amg_set_fused(1)
        ax = med(event_ms(S, st, lambda: d.launch_axpby(
            -1.0, 1.0, B.ptr, Z.ptr, k, stream=st.ptr), n, 2))
        lm = med(event_ms(S, st, lambda: d.launch_multi(
            B.ptr, Z.ptr, k, stream=st.ptr), n, 2))
        out("| %s | %d | %.3f | %.3f | %.2f | %.3f | %.3f | %.2f |"
            % (label, k, one_ms[True], one_ms[False],
               one_ms[False] / one_ms[True], ax, lm, one_ms[True] / lm))
    for h in (H1, H9, d):
        h.release()
    B.free()
    Z.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="solve", choices=("solve", "sweep"))
    ap.add_argument("--only", default="stencil5,stencil27")
    ap.add_argument("--n5", type=int, default=3162)
    ap.add_argument("--n27", type=int, default=215)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import spmv_scpa_amd as S
    sink = open(a.out, "w") if a.out else None

    def out(line):
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
    run = one if a.what == "solve" else sweep
    if a.what == "sweep":
        out("| matrix | k | fused sweep ms | composed sweep ms | composed / "
            "fused | `launch_axpby` ms | `launch_multi` ms | fused / "
            "`launch_multi` |\n|---|---|---|---|---|---|---|---|")
    for which in a.only.split(","):
        if which == "stencil5":
            run(S, "5-point, %d^2, diagonal 4.01" % a.n5,
                stencil((a.n5, a.n5), 4.01), a.reps, out)
        elif which == "stencil27":
            run(S, "27-point, %d^3, diagonal 26.5" % a.n27,
                stencil((a.n27,) * 3, 26.5), a.reps, out)
        else:
            raise SystemExit("--only: stencil5, stencil27")


if __name__ == "__main__":
    main()
