#!/usr/bin/env python3
"""Measure restarted GMRES on the device (gmres(), spmv_*_gmres) and write
profiles/gmres.md:

  1. milliseconds per Arnoldi step at positions p = 0, 7, 15, 29 of a cycle of
     restart = 30 for k = 1, 4, 8 systems on the banded 10M x 32 matrix (HLL),
     beside launch_multi alone on the same handle in the same process and
     beside the byte model of the orthogonalisation;
  2. an iteration of bicgstab() on the same handle, with this tree and --
     given --parent-tree DIR, a checkout of the parent commit with its library
     built -- with the parent's, in a child process each;
  3. iterations and host wall time of gmres(30) against bicgstab() to
     tol = 1e-8 on matrices where BiCGStab does badly;
  4. registers, LDS and scratch of every kernel of gmres_kernels.hip from
     hipcc -Rpass-analysis=kernel-resource-usage (--resources: this section
     alone, rewritten in an existing report; it needs hipcc and no GPU).

Method.  tol = 0 so no column stops.  T(n) = host clock around the blocking
solve (it ends in a stream synchronise) at maxit = n with a supplied work
buffer and check_every = 64 (one batch), ROUNDS times for every n in turns;
the step at position p costs median T(p + 1) - median T(p).  The last update
of X in T(p + 1) reads one basis vector more than in T(p): 8 k M bytes of the
figure.  launch_multi: ROUNDS rounds of 3 warm-ups and 10 launches between two
events.

Byte model of the step at position p, in vectors of 8 k M bytes: each of the
two Gram-Schmidt passes must read the p + 1 basis vectors twice (the sums,
then the update, which needs the sums) and W twice, and write W once; the
scaling reads W and writes V_{p+1}: 4 (p + 1) + 8 vectors.  `moved` adds what
the chunked multi-dot reads again: W once more per launch after the first of a
pass, ceil((p + 1) / chunk) launches with chunk = min(16, 32 // k).  Both are
priced at the rate the vector kernels of cg() reached on this matrix in
profiles/cg.md, (11 * 8 k M) / (iter ms - multi ms): 3.4 / 5.1 / 5.5 TB/s at
k = 1 / 4 / 8.

    python tools/gmres_report.py [--rows 10000000] [--parent-tree DIR] [--out FILE]
    python tools/gmres_report.py --resources [--out FILE]
"""
import argparse
import collections
import json
import re
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# SPMV_TREE: the package of another checkout (the child of --parent-tree)
sys.path.insert(0, os.environ.get("SPMV_TREE") or os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import spmv_scpa_amd as S  # noqa: E402
from cg_report import banded, event_ms  # noqa: E402

PROFILES = os.path.join(HERE, "..", "profiles")
KS = (1, 4, 8)
POSITIONS = (0, 7, 15, 29)
RESTART = 30
ROUNDS = 5
SHORT, LONG = 8, 48
#: TB/s of the vector kernels of cg() on banded 10M x 32, HLL (profiles/cg.md)
CG_RATE = {1: 3.4e12, 4: 5.1e12, 8: 5.5e12}


def median(v):
    return sorted(v)[len(v) // 2]


def upload(M, arrays, hll=True):
    A = S.csr_from_arrays("gmres_report", M, M, *arrays)
    d = S.CsrDevice.upload(A)
    S.csr_free(A)
    if not hll:
        return d
    h = d.to_hll(True)
    d.release()
    return h


def bicgstab_iter_ms(rows):
    """-> {k: (median, low, high)} ms per iteration of bicgstab(), HLL"""
    M = rows
    m = upload(M, banded(M))
    B, X = S.DevBuffer(M * 8 * 8), S.DevBuffer(M * 8 * 8)
    work = S.DevBuffer(S.bicgstab_work_bytes(M, 8))
    S.dev_fill_synth(B.ptr, M * 8, 7)
    out = {}

    def solve(k, maxit):
        S._check(S._lib.spmv_dev_memset(X.ptr, 0, M * k * 8, None), "memset")
        S.stream_sync()
        t0 = time.perf_counter()
        rec = m.bicgstab(B.ptr, X.ptr, k, tol=0.0, maxit=maxit, work=work)
        ms = (time.perf_counter() - t0) * 1e3
        if any((r.status, r.iterations) != (1, maxit) for r in rec):
            raise SystemExit("bicgstab k=%d: a column stopped early" % k)
        return ms

    for k in KS:
        solve(k, SHORT)
        ts, tl = [], []
        for _ in range(ROUNDS):
            ts.append(solve(k, SHORT))
            tl.append(solve(k, LONG))
        ts.sort()
        tl.sort()
        span = LONG - SHORT
        out[k] = ((tl[ROUNDS // 2] - ts[ROUNDS // 2]) / span,
                  (tl[0] - ts[0]) / span, (tl[-1] - ts[-1]) / span)
    return out


def child_bicgstab(rows, tree):
    env = dict(os.environ)
    if tree:
        env["SPMV_TREE"] = os.path.abspath(tree)
    r = subprocess.run([sys.executable, os.path.abspath(__file__),
                        "--bicgstab-only", "--rows", str(rows)], env=env,
                       capture_output=True, text=True)
    if r.returncode:
        raise SystemExit("bicgstab child (%s): %s" % (tree, r.stderr[-2000:]))
    out = r.stdout
    return {int(k): v for k, v in json.loads(out.splitlines()[-1]).items()}


def steps(rows):
    M = rows
    m = upload(M, banded(M))
    B, X = S.DevBuffer(M * 8 * 8), S.DevBuffer(M * 8 * 8)
    work = S.DevBuffer(S.gmres_work_bytes(M, 8, RESTART))
    S.dev_fill_synth(B.ptr, M * 8, 7)
    lines = ["| k | multi ms | p | step ms | / multi | model vectors | "
             "model ms | moved vectors | moved ms | step - multi, / model |",
             "|---|---|---|---|---|---|---|---|---|---|"]

    def solve(k, maxit):
        S._check(S._lib.spmv_dev_memset(X.ptr, 0, M * k * 8, None), "memset")
        S.stream_sync()
        t0 = time.perf_counter()
        rec = m.gmres(B.ptr, X.ptr, k, RESTART, tol=0.0, maxit=maxit,
                      check_every=64, work=work)
        ms = (time.perf_counter() - t0) * 1e3
        if any((r.status, r.iterations) != (1, maxit) for r in rec):
            raise SystemExit("gmres k=%d: a column stopped early: %r"
                             % (k, rec))
        return ms

    for k in KS:
        solve(k, RESTART)  # warm-up of every kernel of this k
        multi = median([event_ms(lambda: m.launch_multi(B.ptr, X.ptr, k))
                        for _ in range(ROUNDS)])
        ns = sorted({p for p in POSITIONS} | {p + 1 for p in POSITIONS})
        t = {n: [] for n in ns}
        for _ in range(ROUNDS):
            for n in ns:
                t[n].append(solve(k, n))
        chunk = min(16, 32 // k)
        for p in POSITIONS:
            step = median(t[p + 1]) - median(t[p])
            vec = 8.0 * k * M
            model = 4 * (p + 1) + 8
            moved = model + 2 * (-(-(p + 1) // chunk) - 1)
            model_ms = model * vec / CG_RATE[k] * 1e3
            moved_ms = moved * vec / CG_RATE[k] * 1e3
            lines.append("| %d | %.3f | %d | %.3f | %.2f | %d | %.3f | %d | "
                         "%.3f | %.2f |"
                         % (k, multi, p, step, step / multi, model, model_ms,
                            moved, moved_ms, (step - multi) / model_ms))
            print(lines[-1], flush=True)
    for b in (B, X, work):
        b.free()
    m.release()
    return lines


def hard_matrices():
    import _bicgstab as BI
    n = 256
    M, IRP, JA, AS = BI.convdiff(n, n, -1.3, 0.0)
    yield "256 x 256 stencil, diagonal 4 - 1.3 (profiles/minres.md)", M, \
        (IRP, JA, AS)
    for c in (0.9, 3.0):
        M, IRP, JA, AS = BI.convdiff(512, 512, 0.0, c)
        yield ("convdiff(512, 512, 0, %g): east -1 + %g, west -1 - %g"
               % (c, c, c)), M, (IRP, JA, AS)


def comparison(maxit=40000):
    lines = ["| matrix | solver | status | steps | products | true residual | "
             "ms |", "|---|---|---|---|---|---|---|"]
    for name, M, arrays in hard_matrices():
        m = upload(M, arrays)
        B, X = S.DevBuffer(M * 8), S.DevBuffer(M * 8)
        S.dev_fill_synth(B.ptr, M, 7)
        for solver in ("bicgstab", "gmres(30)"):
            runs = []
            for _ in range(3):
                if runs and runs[0][0] > 3000.0:  # long enough to stand alone
                    runs = runs * 3
                    break
                S._check(S._lib.spmv_dev_memset(X.ptr, 0, M * 8, None),
                         "memset")
                S.stream_sync()
                t0 = time.perf_counter()
                if solver == "bicgstab":
                    r = m.bicgstab(B.ptr, X.ptr, 1, tol=1e-8, maxit=maxit)[0]
                else:
                    r = m.gmres(B.ptr, X.ptr, 1, RESTART, tol=1e-8,
                                maxit=maxit)[0]
                runs.append(((time.perf_counter() - t0) * 1e3, r))
            runs.sort(key=lambda x: x[0])
            ms, r = runs[1]
            if solver == "bicgstab":
                # its rr is the recurrence's: take the true one
                b = B.to_numpy(np.float64, M)
                Y = S.DevBuffer.from_numpy(b)
                m.launch_axpby(-1.0, 1.0, X.ptr, Y.ptr, 1)
                S.stream_sync()
                res = np.linalg.norm(Y.to_numpy(np.float64, M)) / \
                    np.linalg.norm(b)
                Y.free()
                products = 2 * r.iterations
            else:
                res = (r.rr / r.bb) ** 0.5
                products = r.iterations + r.restarts + 2
            lines.append("| %s | %s | %d | %d | %d | %.2e | %.1f (%.1f..%.1f) |"
                         % (name, solver, r.status, r.iterations, products,
                            res, ms, runs[0][0], runs[2][0]))
            print(lines[-1], flush=True)
        B.free()
        X.free()
        m.release()
    return lines


HEADER = """# Restarted GMRES on the device: a step against its parts

Written by `tools/gmres_report.py%s`
on one MI355X, in one session; what the numbers say is in DESIGN.md section
26. f64 values, column-major HLL, banded 10M x 32 (the matrix of
profiles/cg.md), restart = %d, tol = 0 (every column runs every step, checked).

## Step time by position in the cycle

`multi ms`: `launch_multi` alone on the same handle in the same process (median
of %d rounds of 10 launches between two events). `step ms`: the step at
position `p`, median T(p + 1) - median T(p), T(n) the host clock around the
blocking solve at maxit = n with a supplied work buffer and check_every = 64,
%d rounds of every n in turns; it includes 8 k M bytes of the final update (one
basis vector more), and at p = 29, the last of the cycle, the start of the next
one (launch_axpby, a dot, the scaling). `model vectors`: what the
orthogonalisation must move, in vectors of 8 k M bytes: 4 (p + 1) + 8. `moved
vectors`: with W read again by every launch of the chunked multi-dot after the
first. Both priced at the rate of the vector kernels of `cg()` on this matrix
(profiles/cg.md: 3.4 / 5.1 / 5.5 TB/s at k = 1 / 4 / 8). Last column:
(step - multi) / model ms.

"""

BI_HEADER = """
## An iteration of bicgstab(), this library and the parent commit's

The same matrix and handle type; ms per iteration by the method of
profiles/cg.md (maxit = %d and %d, %d rounds in turns, (median long - median
short) / %d; fastest..slowest pair in brackets), each library in a process of
its own, one after the other.

| k | this commit | parent commit |
|---|---|---|
"""

CMP_HEADER = """
## gmres(30) against bicgstab() to tol = 1e-8

One system, B the synthetic vector of the other tables, X0 = 0, maxit = 40000
(steps for gmres, iterations of two products each for bicgstab), the library's
own work buffer, check_every = 8. `products`: launches of the matrix kernel
(gmres: one per step and one per cycle start and for the true residual).
`true residual`: ||b - A x|| / ||b|| from `launch_axpby`. `ms`: host wall time,
median of 3 (min..max); a run of more than 3 s is not repeated.

"""


RES_TITLE = "## Registers, LDS and scratch of the new kernels"
RES_HEADER = RES_TITLE + """

`hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage` on
gmres_kernels.hip, the templates over k = 1..8 (and the preconditioner mode or
flag) folded into one row each with the range over their instances.  No kernel
uses scratch.

| kernel | instances | VGPRs | SGPRs | LDS bytes | occupancy | scratch bytes |
|---|---|---|---|---|---|---|
"""


def resources():
    """-> the section above, from a compile of gmres_kernels.hip"""
    csrc = os.path.join(HERE, "..", "spmv_scpa_amd", "csrc")
    hipcc = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc")
    r = subprocess.run(
        [hipcc, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17",
         "-I", os.path.join(HERE, "..", "include"),
         "-Rpass-analysis=kernel-resource-usage", "-c",
         os.path.join(csrc, "gmres_kernels.hip"), "-o", os.devnull],
        capture_output=True, text=True, check=True)
    keys = (("VGPRs", r"\bVGPRs: (\d+)"), ("SGPRs", r"TotalSGPRs: (\d+)"),
            ("LDS", r"LDS Size \[bytes/block\]: (\d+)"),
            ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"),
            ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"))
    per = collections.OrderedDict()
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            mangled = m.group(1)
            m = re.match(r"_Z(\d+)", mangled)  # the length of the plain name
            name = (mangled[m.end():m.end() + int(m.group(1))] if m
                    else mangled)
            per.setdefault(name, collections.defaultdict(list))
            per[name]["n"].append(1)
            continue
        for key, pat in keys:
            m = re.search(pat, line)
            if m and name:
                per[name][key].append(int(m.group(1)))
    if not per:
        raise SystemExit("no resource remarks in the compiler's output")

    def span(v):
        return "%d" % v[0] if min(v) == max(v) else "%d..%d" % (min(v), max(v))
    rows = ["| %s | %d | %s | %s | %s | %s | %s |"
            % (name, len(d["n"]), span(d["VGPRs"]), span(d["SGPRs"]),
               span(d["LDS"]), span(d["occupancy"]), span(d["scratch"]))
            for name, d in per.items()]
    if any(max(d["scratch"]) for d in per.values()):
        raise SystemExit("a kernel uses scratch:\n" + "\n".join(rows))
    return RES_HEADER + "\n".join(rows) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--bicgstab-only", action="store_true")
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = a.out or os.path.join(PROFILES, "gmres.md")
    if a.resources:
        text = open(out).read().split(RES_TITLE)[0].rstrip("\n")
        res = resources()
        with open(out, "w") as f:
            f.write(text + "\n\n" + res)
        print("wrote", out)
        return
    if a.bicgstab_only:
        print(os.path.dirname(S.__file__), file=sys.stderr)
        print(json.dumps(bicgstab_iter_ms(a.rows)))
        return
    here = child_bicgstab(a.rows, None)
    parent = (child_bicgstab(a.rows, a.parent_tree) if a.parent_tree
              else None)
    step_lines = steps(a.rows)
    cmp_lines = comparison()
    fmt = "%.3f (%.3f..%.3f)"
    bi = "".join("| %d | %s | %s |\n"
                 % (k, fmt % tuple(here[k]),
                    fmt % tuple(parent[k]) if parent else "not measured")
                 for k in KS)
    argv = " --rows %d" % a.rows if a.rows != 10_000_000 else ""
    argv += " --parent-tree DIR" if a.parent_tree else ""
    try:
        res = "\n" + resources()
    except (OSError, subprocess.CalledProcessError) as e:
        res = ""
        print("no resource section (--resources writes it later):", e)
    with open(out, "w") as f:
        f.write(HEADER % (argv, RESTART, ROUNDS, ROUNDS)
                + "\n".join(step_lines) + "\n"
                + BI_HEADER % (SHORT, LONG, ROUNDS, LONG - SHORT) + bi
                + CMP_HEADER + "\n".join(cmp_lines) + "\n" + res)
    print("wrote", out)


if __name__ == "__main__":
    main()
