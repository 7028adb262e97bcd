#!/usr/bin/env python3
"""Time the IC(0) factorisation (spmv_csr_ic0) and CG preconditioned by
triangular plans (spmv_csr_pcg_trsv) against Jacobi pcg on the 5-point stencil
in natural and in red-black order, and write the table of profiles/ic0.md.

Method: one process per ordering (this script starts itself once per
ordering).  The matrix (diagonal 4 + shift, off-diagonals -1, rows ascending)
is built on the host and uploaded as an ordinary CSR handle.  At a reduced size
the factor is first compared bit for bit with tests/_ic0.py.  Then, at full
size, for Jacobi (pcg), symmetric Gauss-Seidel and IC(0) (pcg_trsv):
  setup     the factorisation / the two analyses, `--reps` times between two
            host clock readings (the calls block); median
  iteration (T(3 n) - T(n)) / (2 n) with T(m) the median over `--reps` solves
            of m iterations (tol = 0) between two events on one stream
  solve     to tol = 1e-8 from X = 0, `--reps` times between two events;
            median, spread and the iteration count
Nothing is asserted about speed.

    python tools/ic0_report.py [--only natural,redblack] [--n 3162]
                               [--shift 0.01] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

COLUMNS = ("| order | rows | preconditioner | levels | launches per apply | "
           "setup ms | ms per iteration | iterations to 1e-8 | solve ms "
           "(min .. max) | solve / Jacobi |\n"
           "|---|---|---|---|---|---|---|---|---|---|")


def stencil(n, shift, redblack):
    """CSR of the 5-point stencil on an n x n grid, rows ascending; redblack:
    the points with x + y even are numbered first"""
    M = n * n
    idx = np.arange(M, dtype=np.int64)
    y, x = np.divmod(idx, n)
    if redblack:
        old_of_new = np.argsort((x + y) % 2, kind="stable")
        new_of_old = np.empty(M, np.int64)
        new_of_old[old_of_new] = idx
    else:
        new_of_old = idx
    big = np.int64(M)  # sorts behind every column
    cols = np.full((M, 5), big, np.int64)
    cols[:, 0] = new_of_old
    for j, (ok, nb) in enumerate(((y > 0, idx - n), (x > 0, idx - 1),
                                  (x < n - 1, idx + 1), (y < n - 1, idx + n))):
        cols[ok, j + 1] = new_of_old[nb[ok]]
    cols = cols[np.argsort(new_of_old)] if redblack else cols
    cols.sort(axis=1)
    keep = cols < big
    IRP = np.zeros(M + 1, np.int32)
    IRP[1:] = np.cumsum(keep.sum(axis=1))
    JA = cols[keep].astype(np.int32)
    AS = np.where(JA == np.repeat(idx, np.diff(IRP)), 4.0 + shift, -1.0)
    return M, IRP, JA, AS


def upload(S, mat):
    M, IRP, JA, AS = mat
    A = S.csr_from_arrays("ic0", M, M, IRP, JA, AS)
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


def one(order, n, shift, reps, n_iter):
    import _ic0 as IC
    import spmv_scpa_amd as S
    redblack = order == "redblack"
    # 1. the bits, at a reduced size
    small = stencil(40, shift, redblack)
    d = upload(S, small)
    Ld, info = d.ic0()
    p = Ld.download()
    got = S.csr_arrays(p)[2].copy()
    S.csr_free(p)
    want = IC.reference_ic0(*small)
    if not np.array_equal(got.view(np.uint64), want.AS.view(np.uint64)):
        raise SystemExit("%s: the factor differs from the reference" % order)
    Ld.release()
    d.release()
    print("%s: the reduced size matches the reference" % order,
          file=sys.stderr, flush=True)
    # 2. full size
    mat = stencil(n, shift, redblack)
    M = mat[0]
    d = upload(S, mat)
    del mat
    st = S.Stream()
    d_B, d_X = S.DevBuffer(M * 8), S.DevBuffer(M * 8)
    S.dev_fill_synth(d_B.ptr, M, 7)
    S.stream_sync()

    def solve_ms(run, maxit, tol):
        """one solve from X = 0 between two events -> (ms, record)"""
        S._check(S._lib.spmv_dev_memset(d_X.ptr, 0, M * 8, st.ptr), "memset")
        a, b = S.Event(), S.Event()
        a.record(st.ptr)
        rec = run(maxit, tol)[0]
        b.record(st.ptr)
        S.stream_sync(st.ptr)
        return a.elapsed_ms(b), rec

    def measure(name, setup, levels, launches, run):
        solve_ms(run, 2, 0.0)  # warm-up: code objects, the allocator
        t = {m: float(np.median([solve_ms(run, m, 0.0)[0]
                                 for _ in range(reps)]))
             for m in (n_iter, 3 * n_iter)}
        per_it = (t[3 * n_iter] - t[n_iter]) / (2 * n_iter)
        full = [solve_ms(run, 100000, 1e-8) for _ in range(reps)]
        ms = [f[0] for f in full]
        rec = full[-1][1]
        print("%s %s: setup %s | T(%d) %.2f T(%d) %.2f | solve %s | %r"
              % (order, name, " ".join("%.1f" % m for m in setup), n_iter,
                 t[n_iter], 3 * n_iter, t[3 * n_iter],
                 " ".join("%.1f" % m for m in ms), rec),
              file=sys.stderr, flush=True)
        return dict(name=name, levels=levels, launches=launches,
                    setup=float(np.median(setup)) if setup else 0.0,
                    per_it=per_it, iters=rec.iterations, status=rec.status,
                    ms=float(np.median(ms)), lo=min(ms), hi=max(ms))

    rows = []
    # Jacobi
    d_minv = S.DevBuffer(M * 8)
    setup = host_ms(lambda: (d.diag(d_minv.ptr, invert=True),
                             S.stream_sync()), reps)
    rows.append(measure(
        "Jacobi (pcg)", setup, "", 0,
        lambda maxit, tol: d.pcg(d_B.ptr, d_X.ptr, d_minv.ptr, 1, tol=tol,
                                 maxit=maxit, check_every=64,
                                 stream=st.ptr)))
    d_minv.free()
    # symmetric Gauss-Seidel
    d.sgs().release()  # warm-up
    made = []
    setup = host_ms(lambda: made.append(d.sgs()), reps)
    for sg in made[:-1]:
        sg.release()
    sg = made[-1]
    li, ui = sg.lower.info, sg.upper.info
    rows.append(measure(
        "SGS (pcg_trsv)", setup, "%d + %d" % (li["levels"], ui["levels"]),
        li["launches"] + ui["launches"],
        lambda maxit, tol: d.pcg_trsv(d_B.ptr, d_X.ptr, *sg.args, k=1,
                                      tol=tol, maxit=maxit, check_every=64,
                                      stream=st.ptr)))
    sg.release()
    # IC(0): the factorisation alone, then with the transpose and the plans
    d.ic0()[0].release()  # warm-up
    fact = host_ms(lambda: d.ic0()[0].release(), reps)
    made = []

    def build():
        L, info = d.ic0()
        LT = L.transpose()
        made.append((L.trsv_analyse("lower"), LT.trsv_analyse("upper"), info))
        L.release()
        LT.release()
    setup = host_ms(build, reps)
    for lo, up, _ in made[:-1]:
        lo.release()
        up.release()
    lo, up, info = made[-1]
    r = measure(
        "IC(0) (pcg_trsv)", setup,
        "%d + %d" % (lo.info["levels"], up.info["levels"]),
        lo.info["launches"] + up.info["launches"],
        lambda maxit, tol: d.pcg_trsv(d_B.ptr, d_X.ptr, lo, up, k=1, tol=tol,
                                      maxit=maxit, check_every=64,
                                      stream=st.ptr))
    r["fact"] = float(np.median(fact))
    r["fact_launches"] = info.launches
    r["bad"] = info.bad_pivots
    rows.append(r)
    lo.release()
    up.release()
    d.release()
    base = rows[0]["ms"]
    for r in rows:
        setup = "%.1f" % r["setup"]
        if "fact" in r:
            setup += " (factorisation alone %.1f, %d launches)" % (
                r["fact"], r["fact_launches"])
        print("LINE " + json.dumps(
            "| %s | %d | %s | %s | %d | %s | %.3f | %d%s | %.1f (%.1f .. %.1f) "
            "| %.2f |" % (order, M, r["name"], r["levels"], r["launches"],
                          setup, r["per_it"], r["iters"],
                          "" if r["status"] == 0 else " (status %d)"
                          % r["status"], r["ms"], r["lo"], r["hi"],
                          r["ms"] / base)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--only", default="natural,redblack")
    ap.add_argument("--n", type=int, default=3162)
    ap.add_argument("--shift", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=8,
                    help="n of the per-iteration time: solves of n and 3 n")
    ap.add_argument("--one", default="", help=argparse.SUPPRESS)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.one:
        return one(a.one, a.n, a.shift, a.reps, a.iters)
    lines = [COLUMNS]
    for order in a.only.split(","):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one",
                            order, "--n", str(a.n), "--shift", str(a.shift),
                            "--reps", str(a.reps), "--iters", str(a.iters)],
                           stdout=subprocess.PIPE, text=True)
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("LINE ")]
        if r.returncode or not got:
            raise SystemExit("%s: exit status %d\n%s" % (order, r.returncode,
                                                         r.stdout))
        lines += [json.loads(g[5:]) for g in got]
        print("\n".join(lines[-3:]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        print("wrote", a.out)


if __name__ == "__main__":
    main()
