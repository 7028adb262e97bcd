#!/usr/bin/env python3
"""Time the ILU(0) factorisation (spmv_csr_ilu0) beside IC(0) on the symmetric
counterpart, and BiCGStab preconditioned by its two plans
(spmv_csr_bicgstab_trsv) against bicgstab with Jacobi and without a
preconditioner, in natural order and after colour() + permute(), and write the
tables of profiles/ilu0.md.

Matrices (built on the host, rows ascending, in natural order):
  convdiff   5-point convection-diffusion on an n x n grid: diagonal
             4 + shift, the neighbours -1 - c below and -1 + c above the
             diagonal
  stencil27  the 27-point stencil on an m x m x m grid: diagonal 26 + shift,
             the 26 neighbours -1 - c below and -1 + c above the diagonal
The symmetric counterpart (c = 0) has the same pattern, so spmv_csr_ic0 walks
the same schedule: it is the yardstick of the factorisation.

Method: one process per (matrix, ordering); this script starts itself.  At a
reduced size the factor is first compared bit for bit with tests/_ilu0.py.
Then, at full size:
  factorisation  `--reps` blocking calls between two host clock readings;
                 median (min .. max); the same for ic0
  setup          the factorisation and the two analyses together, likewise
                 (Jacobi: diag(invert); multicolour adds colour + permute,
                 listed on its own)
  solve          to tol = 1e-8 from X = 0 (at most --maxit iterations), B the
                 synthetic vector in the ordering of the handle, `--reps` times
                 between two events on one stream; median (min .. max), the
                 iteration count, and ms per iteration = solve / iterations
Nothing is asserted about speed.  --factor-only stops after the factorisation
(to compare two builds of the kernel through SPMV_LIB).

    python tools/ilu0_report.py [--only convdiff:natural,...] [--n 3162]
        [--m 215] [--shift 0.01] [--c 0.5] [--reps 3] [--limit 900]
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

CASES = ("convdiff:natural", "convdiff:multicolour", "stencil27:natural",
         "stencil27:multicolour")
FACTOR = ("| matrix | order | rows | levels | launches | ilu0 ms (min .. max) "
          "| ic0 ms, symmetric counterpart (min .. max) | ilu0 / ic0 |\n"
          "|---|---|---|---|---|---|---|---|")
SOLVE = ("| matrix | order | preconditioner | launches per apply | setup ms | "
         "iterations to 1e-8 | ms per iteration | solve ms (min .. max) | "
         "solve / Jacobi |\n|---|---|---|---|---|---|---|---|---|")


def pattern(dims, full):
    """(M, IRP, JA, side, neighbours) of the stencil on a grid of `dims`
    points in natural order, rows ascending.  full: every neighbour with
    offsets in {-1, 0, 1}; else only those along one axis.  side[e] is -1, 0 or
    1 for an entry below, on or above the diagonal: the values are made from
    it, so one pattern serves the matrix and its symmetric counterpart"""
    nd = len(dims)
    M = int(np.prod(dims))
    strides = [int(np.prod(dims[a + 1:])) for a in range(nd)]
    offs = [o for o in itertools.product((-1, 0, 1), repeat=nd)
            if full or sum(map(abs, o)) <= 1]
    offs.sort(key=lambda o: sum(x * s for x, s in zip(o, strides)))
    idx = np.arange(M, dtype=np.int32)
    coords = np.unravel_index(idx, dims)
    cols = np.full((M, len(offs)), -1, np.int32)
    for j, o in enumerate(offs):
        lin = sum(x * s for x, s in zip(o, strides))
        ok = np.ones(M, bool)
        for a in range(nd):
            if o[a] < 0:
                ok &= coords[a] > 0
            elif o[a] > 0:
                ok &= coords[a] < dims[a] - 1
        cols[:, j] = np.where(ok, idx + np.int32(lin), np.int32(-1))
    keep = cols >= 0
    IRP = np.zeros(M + 1, np.int32)
    IRP[1:] = np.cumsum(keep.sum(axis=1))
    lins = np.array([sum(x * s for x, s in zip(o, strides)) for o in offs])
    side = np.broadcast_to(np.sign(lins).astype(np.int8), cols.shape)[keep]
    return M, IRP, cols[keep], side, len(offs) - 1


def values(side, neighbours, shift, c):
    """diagonal neighbours + shift; a neighbour below the diagonal is -1 - c,
    one above it -1 + c"""
    return np.array([-1.0 - c, neighbours + shift, -1.0 + c])[side + 1]


def grid(name, a, small=False):
    if name == "convdiff":
        n = 40 if small else a.n
        return pattern((n, n), False)
    m = 12 if small else a.m
    return pattern((m, m, m), True)


def matrix(pat, shift, c):
    M, IRP, JA, side, neighbours = pat
    return M, IRP, JA, values(side, neighbours, shift, c)


def upload(S, mat):
    M, IRP, JA, AS = mat
    A = S.csr_from_arrays("ilu0", M, M, IRP, JA, AS)
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


def span(ms):
    return "%.1f (%.1f .. %.1f)" % (float(np.median(ms)), min(ms), max(ms))


def emit(kind, text):
    print(kind + " " + json.dumps(text), flush=True)


def one(case, a):
    import _ilu0 as IL
    import spmv_scpa_amd as S
    name, order = case.split(":")
    # 1. the bits, at a reduced size
    small = matrix(grid(name, a, small=True), a.shift, a.c)
    d = upload(S, small)
    LU, info = d.ilu0()
    p = LU.download()
    got = S.csr_arrays(p)[2].copy()
    S.csr_free(p)
    if not np.array_equal(got.view(np.uint64),
                          IL.reference_ilu0(*small).AS.view(np.uint64)):
        raise SystemExit("%s: the factor differs from the reference" % case)
    LU.release()
    d.release()
    print("%s: the reduced size matches the reference" % case,
          file=sys.stderr, flush=True)
    # 2. full size: the matrix and its symmetric counterpart, in the ordering
    pat = grid(name, a)
    dA = upload(S, matrix(pat, a.shift, a.c))
    dS = upload(S, matrix(pat, a.shift, 0.0))
    del pat
    M = dA.M
    d_B, d_X = S.DevBuffer(M * 8), S.DevBuffer(M * 8)
    S.dev_fill_synth(d_B.ptr, M, 7)
    S.stream_sync()
    order_ms = []
    if order == "multicolour":
        t0 = time.perf_counter()
        col = dA.colour()
        dP = dA.permute(col, col)
        order_ms.append((time.perf_counter() - t0) * 1e3)
        dQ = dS.permute(col, col)   # the same pattern: the same ordering
        S.permute_vectors(col, d_B, d_X, M)
        S.stream_sync()
        d_B, d_X = d_X, d_B
        for h in (dA, dS, col):
            h.release()
        dA, dS = dP, dQ
    dS.ic0()[0].release()   # warm-up
    ic = host_ms(lambda: dS.ic0()[0].release(), a.reps)
    dS.release()
    info = dA.ilu0()[1]
    il = host_ms(lambda: dA.ilu0()[0].release(), a.reps)
    emit("FACTOR", "| %s | %s | %d | %d | %d | %s | %s | %.2f |" % (
        name, order, M, info.levels, info.launches, span(il), span(ic),
        np.median(il) / np.median(ic)))
    if info.bad_pivots:
        raise SystemExit("%s: %d bad pivots" % (case, info.bad_pivots))
    if a.factor_only:
        return
    st = S.Stream()

    def solve_ms(run):
        S._check(S._lib.spmv_dev_memset(d_X.ptr, 0, M * 8, st.ptr), "memset")
        e0, e1 = S.Event(), S.Event()
        e0.record(st.ptr)
        rec = run()[0]
        e1.record(st.ptr)
        S.stream_sync(st.ptr)
        return e0.elapsed_ms(e1), rec

    def measure(label, launches, setup, run):
        solve_ms(run)   # warm-up: code objects, the allocator
        got = [solve_ms(run) for _ in range(a.reps)]
        ms, rec = [g[0] for g in got], got[-1][1]
        print(case, label, span(ms), rec, file=sys.stderr, flush=True)
        return dict(label=label, launches=launches, setup=setup, ms=ms,
                    rec=rec)

    kw = dict(k=1, tol=1e-8, maxit=a.maxit, check_every=64, stream=st.ptr)
    rows = []
    d_minv = S.DevBuffer(M * 8)
    setup = host_ms(lambda: (dA.diag(d_minv.ptr, invert=True),
                             S.stream_sync()), a.reps)
    rows.append(measure("Jacobi (bicgstab)", 0, setup,
                        lambda: dA.bicgstab(d_B.ptr, d_X.ptr, d_minv=d_minv.ptr,
                                            **kw)))
    rows.append(measure("none (bicgstab)", 0, [0.0],
                        lambda: dA.bicgstab(d_B.ptr, d_X.ptr, **kw)))
    made = []

    def build():
        LU = dA.ilu0()[0]
        made.append((LU.trsv_analyse("lower", unit=True),
                     LU.trsv_analyse("upper")))
        LU.release()
    setup = host_ms(build, a.reps)
    for lo, up in made[:-1]:
        lo.release()
        up.release()
    lo, up = made[-1]
    rows.append(measure(
        "ILU(0) (bicgstab_trsv)", lo.info["launches"] + up.info["launches"],
        setup, lambda: dA.bicgstab_trsv(d_B.ptr, d_X.ptr, lo, up, **kw)))
    base = float(np.median(rows[0]["ms"]))
    for r in rows:
        rec = r["rec"]
        emit("SOLVE", "| %s | %s | %s | %d | %s%s | %d%s | %.3f | %s | %.2f |" % (
            name, order, r["label"], r["launches"],
            "%.1f" % float(np.median(r["setup"])),
            " (+ %.1f colour and permute)" % order_ms[0] if order_ms else "",
            rec.iterations,
            "" if rec.status == 0 else " (status %d)" % rec.status,
            float(np.median(r["ms"])) / max(rec.iterations, 1), span(r["ms"]),
            float(np.median(r["ms"])) / base))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--only", default=",".join(CASES))
    ap.add_argument("--n", type=int, default=3162)
    ap.add_argument("--m", type=int, default=215)
    ap.add_argument("--shift", type=float, default=0.01)
    ap.add_argument("--c", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--maxit", type=int, default=5000)
    ap.add_argument("--factor-only", action="store_true")
    ap.add_argument("--limit", type=int, default=900,
                    help="seconds one (matrix, ordering) process may take")
    ap.add_argument("--one", default="", help=argparse.SUPPRESS)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.one:
        return one(a.one, a)
    tables = {"FACTOR": [FACTOR], "SOLVE": [SOLVE]}
    for case in a.only.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", case]
        for f in ("n", "m", "shift", "c", "reps", "maxit"):
            cmd += ["--" + f, str(getattr(a, f))]
        if a.factor_only:
            cmd.append("--factor-only")
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True,
                               timeout=a.limit)
        except subprocess.TimeoutExpired:
            raise SystemExit("%s: not done after %d s" % (case, a.limit))
        got = [ln.split(" ", 1) for ln in r.stdout.splitlines()
               if ln.startswith(("FACTOR ", "SOLVE "))]
        if r.returncode or not got:
            raise SystemExit("%s: exit status %d\n%s" % (case, r.returncode,
                                                         r.stdout))
        for kind, text in got:
            tables[kind].append(json.loads(text))
            print(tables[kind][-1], flush=True)
        if a.out:   # after every case: a run cut short keeps what it has
            with open(a.out, "w") as f:
                f.write("\n".join(tables["FACTOR"]) + "\n\n")
                if len(tables["SOLVE"]) > 1:
                    f.write("\n".join(tables["SOLVE"]) + "\n")
    if a.out:
        print("wrote", a.out)


if __name__ == "__main__":
    main()
