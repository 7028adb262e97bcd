#!/usr/bin/env python3
"""Time the device colouring (spmv_csr_colour), the permutation of the handle
(spmv_csr_permute) and CG preconditioned by the plans of the PERMUTED matrix
(spmv_csr_pcg_trsv) against Jacobi pcg on the UNPERMUTED one, and write the
tables of profiles/colour.md.

Method: one process per matrix (this script starts itself once per matrix,
each under its own time limit, and stops at the first that fails).  The
matrix -- the 5-point stencil on n^2 points (diagonal 4.01) or the 27-point
stencil on n^3 (diagonal 26.5), natural order, both triangles, rows ascending
-- is built on the host and uploaded as an ordinary CSR handle.  At a reduced
size the colouring is first compared with tests/_colour.py.  Then, at full
size:
  colour, permute, ic0, analyses   `--reps` blocking calls between two host
            clock readings, after one warm-up call; median
  vectors   permute_vectors of one vector, into the new numbering and back,
            between two events; median
  iteration (T(3 n) - T(n)) / (2 n) with T(m) the median over `--reps` solves
            of m iterations (tol = 0) between two events on one stream
  solve     to tol = 1e-8 from X = 0, `--reps` times between two events;
            median, spread and the iteration count.  The solves of the
            permuted matrix take the permuted right-hand side
Nothing is asserted about speed.

    python tools/colour_report.py [--only stencil5,stencil27] [--n5 3162]
                                  [--n27 215] [--reps 3] [--limit 900]
                                  [--out FILE]
"""
import argparse
import itertools
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SETUP = ("| matrix | rows | entries | colours | rounds | widest / narrowest "
         "| colour ms | ms per round | permute ms | ic0 ms | two analyses ms "
         "| vectors there / back ms |\n"
         "|---|---|---|---|---|---|---|---|---|---|---|---|")
SOLVE = ("| matrix | handle | preconditioner | levels | launches per apply | "
         "ms per iteration | iterations to 1e-8 | solve ms (min .. max) | "
         "solve / Jacobi |\n"
         "|---|---|---|---|---|---|---|---|---|")


def stencil(dims, diag):
    """CSR of the full stencil (every offset in {-1, 0, 1}^d) on a grid of
    `dims` points in lexicographic order, rows ascending; 2-D: the 5-point
    stencil (the offsets with one non-zero component)"""
    M = int(np.prod(dims))
    idx = np.arange(M, dtype=np.int64)
    coord = np.unravel_index(idx, dims)
    offsets = [o for o in itertools.product((-1, 0, 1), repeat=len(dims))
               if len(dims) == 3 or sum(map(abs, o)) <= 1]
    cols = np.full((M, len(offsets)), -1, np.int32)
    for j, off in enumerate(offsets):  # lexicographic: ascending columns
        ok = np.ones(M, bool)
        lin = 0
        for c, o, n in zip(coord, off, dims):
            ok &= (c + o >= 0) & (c + o < n)
            lin = lin * n + o
        cols[ok, j] = (idx[ok] + lin).astype(np.int32)
    keep = cols >= 0
    IRP = np.zeros(M + 1, np.int32)
    IRP[1:] = np.cumsum(keep.sum(axis=1))
    JA = cols[keep]
    AS = np.where(JA == np.repeat(idx, np.diff(IRP)).astype(np.int32), diag,
                  -1.0)
    return M, IRP, JA, AS


def make(which, n):
    if which == "stencil5":
        return "5-point, %d^2" % n, stencil((n, n), 4.01)
    return "27-point, %d^3" % n, stencil((n, n, n), 26.5)


def upload(S, mat):
    M, IRP, JA, AS = mat
    A = S.csr_from_arrays("colour", M, M, IRP, JA, AS)
    d = S.CsrDevice.upload(A)
    S.csr_free(A)
    return d


def host_ms(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def one(which, n, reps, n_iter):
    import _colour as CO
    import spmv_scpa_amd as S
    # 1. the integers, at a reduced size
    small = make(which, 40 if which == "stencil5" else 9)[1]
    d = upload(S, small)
    col = d.colour()
    want = CO.reference_colour(small[0], small[1], small[2], 0)
    if not (np.array_equal(col.colour.to_numpy(np.int32, small[0]), want[0])
            and np.array_equal(col.perm.to_numpy(np.int32, small[0]), want[2])
            and col.rounds == want[1].max()):
        raise SystemExit("%s: the colouring differs from the reference" % which)
    col.release()
    d.release()
    print("%s: the reduced size matches the reference" % which,
          file=sys.stderr, flush=True)
    # 2. full size
    label, mat = make(which, n)
    M, NZ = mat[0], len(mat[2])
    d = upload(S, mat)
    del mat
    st = S.Stream()
    d_B, d_PB, d_X = (S.DevBuffer(M * 8) for _ in range(3))
    S.dev_fill_synth(d_B.ptr, M, 7)
    S.stream_sync()

    def med(v):
        return float(np.median(v))

    d.colour().release()  # warm-up
    made = []
    t_colour = host_ms(lambda: made.append(d.colour()), reps)
    for c in made[:-1]:
        c.release()
    col = made[-1]
    d.permute(col, col).release()  # warm-up
    made = []
    t_permute = host_ms(lambda: made.append(d.permute(col, col)), reps)
    for b in made[:-1]:
        b.release()
    dP = made[-1]
    dP.ic0()[0].release()  # warm-up
    made = []
    t_ic0 = host_ms(lambda: made.append(dP.ic0()), reps)
    for L, _ in made[:-1]:
        L.release()
    L, ic = made[-1]
    LT = L.transpose()
    made = []
    t_plans = host_ms(lambda: made.append((L.trsv_analyse("lower"),
                                           LT.trsv_analyse("upper"))), reps)
    for lo, up in made[:-1]:
        lo.release()
        up.release()
    lo, up = made[-1]
    L.release()
    LT.release()
    sg = dP.sgs()

    def event_ms(fn):
        a, b = S.Event(), S.Event()
        a.record(st.ptr)
        fn()
        b.record(st.ptr)
        S.stream_sync(st.ptr)
        return a.elapsed_ms(b)

    def there():
        S.permute_vectors(col, d_B, d_PB, M, stream=st.ptr)

    def back():
        S.permute_vectors(col, d_PB, d_X, M, inverse=True, stream=st.ptr)

    there()
    back()
    t_there = [event_ms(there) for _ in range(reps)]
    t_back = [event_ms(back) for _ in range(reps)]
    print("%s: colour %s | permute %s | ic0 %s | plans %s | vectors %s %s | %d "
          "bad pivots" % (which, t_colour, t_permute, t_ic0, t_plans, t_there,
                          t_back, ic.bad_pivots), file=sys.stderr, flush=True)
    print("SETUP " + json.dumps(
        "| %s | %d | %d | %d | %d | %d / %d | %.1f | %.3f | %.1f | %.1f | %.1f "
        "| %.3f / %.3f |" % (label, M, NZ, col.colours, col.rounds, col.widest,
                             col.narrowest, med(t_colour),
                             med(t_colour) / col.rounds, med(t_permute),
                             med(t_ic0), med(t_plans), med(t_there),
                             med(t_back))), flush=True)

    def solve_ms(run, maxit, tol):
        """one solve from X = 0 between two events -> (ms, record)"""
        S._check(S._lib.spmv_dev_memset(d_X.ptr, 0, M * 8, st.ptr), "memset")
        a, b = S.Event(), S.Event()
        a.record(st.ptr)
        rec = run(maxit, tol)[0]
        b.record(st.ptr)
        S.stream_sync(st.ptr)
        return a.elapsed_ms(b), rec

    def measure(handle, name, levels, launches, run):
        solve_ms(run, 2, 0.0)  # warm-up: code objects, the allocator
        t = {m: med([solve_ms(run, m, 0.0)[0] for _ in range(reps)])
             for m in (n_iter, 3 * n_iter)}
        per_it = (t[3 * n_iter] - t[n_iter]) / (2 * n_iter)
        full = [solve_ms(run, 100000, 1e-8) for _ in range(reps)]
        ms = [f[0] for f in full]
        rec = full[-1][1]
        print("%s %s: T(%d) %.2f T(%d) %.2f | solve %s | %r"
              % (which, name, n_iter, t[n_iter], 3 * n_iter, t[3 * n_iter],
                 " ".join("%.1f" % m for m in ms), rec),
              file=sys.stderr, flush=True)
        return dict(handle=handle, name=name, levels=levels, launches=launches,
                    per_it=per_it, iters=rec.iterations, status=rec.status,
                    ms=med(ms), lo=min(ms), hi=max(ms))

    rows = []
    d_minv = S.DevBuffer(M * 8)
    d.diag(d_minv.ptr, invert=True)
    S.stream_sync()
    rows.append(measure(
        "natural", "Jacobi (pcg)", "", 0,
        lambda maxit, tol: d.pcg(d_B.ptr, d_X.ptr, d_minv.ptr, 1, tol=tol,
                                 maxit=maxit, check_every=64, stream=st.ptr)))
    d_minv.free()
    li, ui = sg.lower.info, sg.upper.info
    rows.append(measure(
        "coloured", "SGS (pcg_trsv)",
        "%d + %d" % (li["levels"], ui["levels"]),
        li["launches"] + ui["launches"],
        lambda maxit, tol: dP.pcg_trsv(d_PB.ptr, d_X.ptr, *sg.args, k=1,
                                       tol=tol, maxit=maxit, check_every=64,
                                       stream=st.ptr)))
    sg.release()
    rows.append(measure(
        "coloured", "IC(0) (pcg_trsv)",
        "%d + %d" % (lo.info["levels"], up.info["levels"]),
        lo.info["launches"] + up.info["launches"],
        lambda maxit, tol: dP.pcg_trsv(d_PB.ptr, d_X.ptr, lo, up, k=1, tol=tol,
                                       maxit=maxit, check_every=64,
                                       stream=st.ptr)))
    for h in (lo, up, dP, col, d):
        h.release()
    base = rows[0]["ms"]
    for r in rows:
        print("SOLVE " + json.dumps(
            "| %s | %s | %s | %s | %d | %.3f | %d%s | %.1f (%.1f .. %.1f) | "
            "%.2f |" % (label, r["handle"], r["name"], r["levels"],
                        r["launches"], r["per_it"], r["iters"],
                        "" if r["status"] == 0 else " (status %d)"
                        % r["status"], r["ms"], r["lo"], r["hi"],
                        r["ms"] / base)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--only", default="stencil5,stencil27")
    ap.add_argument("--n5", type=int, default=3162)
    ap.add_argument("--n27", type=int, default=215)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=8,
                    help="n of the per-iteration time: solves of n and 3 n")
    ap.add_argument("--limit", type=int, default=900,
                    help="seconds one matrix may take")
    ap.add_argument("--one", default="", help=argparse.SUPPRESS)
    ap.add_argument("--n", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.one:
        return one(a.one, a.n, a.reps, a.iters)
    setup, solve = [SETUP], [SOLVE]
    for which in a.only.split(","):
        n = a.n5 if which == "stencil5" else a.n27
        try:
            r = subprocess.run(
                [sys.executable, os.path.abspath(__file__), "--one", which,
                 "--n", str(n), "--reps", str(a.reps), "--iters",
                 str(a.iters)], stdout=subprocess.PIPE, text=True,
                timeout=a.limit)
        except subprocess.TimeoutExpired:
            raise SystemExit("%s: not done after %d s" % (which, a.limit))
        got = [ln for ln in r.stdout.splitlines()
               if ln.startswith(("SETUP ", "SOLVE "))]
        if r.returncode or len(got) != 4:
            raise SystemExit("%s: exit status %d\n%s" % (which, r.returncode,
                                                         r.stdout))
        setup += [json.loads(g[6:]) for g in got if g.startswith("SETUP ")]
        solve += [json.loads(g[6:]) for g in got if g.startswith("SOLVE ")]
        print("\n".join([setup[-1]] + solve[-3:]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(setup) + "\n\n" + "\n".join(solve) + "\n")
        print("wrote", a.out)


if __name__ == "__main__":
    main()
