#!/usr/bin/env python3
"""Time the level-scheduled triangular solve (spmv_csr_trsv_analyse,
spmv_trsv_solve) on the lower triangles of two stencils and write the table of
profiles/trsv.md.

Method: one process per matrix (this script starts itself once per matrix).
The lower triangle, diagonal included, is built on the host and uploaded as an
ordinary CSR handle; the plan is analysed from that handle.  The result of one
solve is first compared bit for bit with tests/_trsv.py at a reduced size.
Then, at full size: the analysis three times between two host clock readings
(it blocks); the solve at k = 1, 4, 8, `--reps` times each between two events
on one stream, median and spread; and the floor, launch_multi of the SAME
handle at the same k -- the same bytes with no dependencies -- timed the same
way.  Nothing is asserted about speed.

    python tools/trsv_report.py [--only stencil5,stencil27] [--n5 3162]
                                [--n27 215] [--reps 7] [--out FILE]

SPMV_LIB selects the library, so builds with other -DTRSV_GROUP /
-DTRSV_SMALL_ROWS can be compared; --label names the build in the table.
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

COLUMNS = ("| build | matrix | rows | strict entries | levels | widest | "
           "launches (chain + wide) | analysis ms | k | solve ms (min .. max) "
           "| launch_multi ms | solve / multi | us per launch |\n"
           "|---|---|---|---|---|---|---|---|---|---|---|---|---|")


def stencil_lower(dims, offsets, diag):
    """CSR of the lower triangle of a stencil on a grid of `dims` points in
    lexicographic order: the offsets (last index fastest) that lead to a
    smaller row, then the diagonal"""
    M = int(np.prod(dims))
    idx = np.arange(M, dtype=np.int64)
    coord = np.unravel_index(idx, dims)
    cols = np.full((M, len(offsets) + 1), -1, np.int32)
    for j, off in enumerate(offsets):
        ok = np.ones(M, bool)
        lin = 0
        for c, o, n in zip(coord, off, dims):
            ok &= (c + o >= 0) & (c + o < n)
            lin = lin * n + o
        cols[ok, j] = (idx[ok] + lin).astype(np.int32)
    cols[:, -1] = idx
    keep = cols >= 0
    IRP = np.zeros(M + 1, np.int32)
    IRP[1:] = np.cumsum(keep.sum(axis=1))
    JA = cols[keep]
    AS = np.where(JA == np.repeat(idx, np.diff(IRP)), diag, -1.0)
    return M, IRP, JA, AS


def make(which, n):
    if which == "stencil5":
        return ("5-point, %d^2 grid" % n,
                stencil_lower((n, n), [(-1, 0), (0, -1)], 4.5))
    offs = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1)
            for c in (-1, 0, 1) if (a, b, c) < (0, 0, 0)]
    return "27-point, %d^3 grid" % n, stencil_lower((n, n, n), offs, 26.5)


def timed(S, fn, reps, stream):
    fn()
    S.stream_sync(stream.ptr)
    ms = []
    for _ in range(reps):
        a, b = S.Event(), S.Event()
        a.record(stream.ptr)
        fn()
        b.record(stream.ptr)
        ms.append(a.elapsed_ms(b))
    return ms


def one(which, n, reps, label):
    import _trsv as TV
    import spmv_scpa_amd as S
    shape = S.trsv_shape()
    # 1. the bits, at a reduced size
    name, (M, IRP, JA, AS) = make(which, 40 if which == "stencil5" else 12)
    A = S.csr_from_arrays("t", M, M, IRP, JA, AS)
    d = S.CsrDevice.upload(A)
    S.csr_free(A)
    plan = d.trsv_analyse("lower")
    B = np.random.default_rng(1).uniform(-1, 1, (M, 4))
    d_B, d_X = S.DevBuffer.from_numpy(B), S.DevBuffer(M * 32)
    plan.solve(d_B.ptr, d_X.ptr, 4)
    S.stream_sync()
    want = TV.reference_solve(TV.reference_plan(IRP, JA, AS, "lower"), B, None,
                              shape["group"])
    got = d_X.to_numpy(np.float64, M * 4).reshape(M, 4)
    if not np.array_equal(got.view(np.uint64), want.view(np.uint64)):
        raise SystemExit("%s: the solve differs from the reference" % name)
    for h in (d_B, d_X):
        h.free()
    plan.release()
    d.release()
    print("%s: the reduced size matches the reference" % name, file=sys.stderr,
          flush=True)
    # 2. full size
    name, (M, IRP, JA, AS) = make(which, n)
    A = S.csr_from_arrays("t", M, M, IRP, JA, AS)
    d = S.CsrDevice.upload(A)
    S.csr_free(A)
    del IRP, JA, AS
    d.trsv_analyse("lower").release()  # warm-up: code objects, the allocator
    an = []
    for _ in range(3):
        t0 = time.perf_counter()
        plan = d.trsv_analyse("lower")
        an.append((time.perf_counter() - t0) * 1e3)
        if len(an) < 3:
            plan.release()
    info = plan.info
    p = plan.download()
    segs = TV.segments(p["level_ptr"], shape["small_rows"])
    chains = sum(1 for s in segs if s[0] == TV.CHAIN)
    del p
    print("%s: analysis ms %s, %r" % (name, " ".join("%.1f" % m for m in an),
                                      info), file=sys.stderr, flush=True)
    st = S.Stream()
    lines = []
    for k in (1, 4, 8):
        d_B, d_X = S.DevBuffer(M * 8 * k), S.DevBuffer(M * 8 * k)
        S.dev_fill_synth(d_B.ptr, M * k, 7)
        S._lib.spmv_dev_memset(d_X.ptr, 0, M * 8 * k, None)
        S.stream_sync()
        solve = timed(S, lambda: plan.solve(d_B.ptr, d_X.ptr, k,
                                            stream=st.ptr), reps, st)
        multi = timed(S, lambda: d.launch_multi(d_B.ptr, d_X.ptr, k,
                                                stream=st.ptr), reps, st)
        sm, mm = float(np.median(solve)), float(np.median(multi))
        print("%s k=%d: solve %s | multi %s" % (
            name, k, " ".join("%.3f" % m for m in solve),
            " ".join("%.3f" % m for m in multi)), file=sys.stderr, flush=True)
        lines.append(
            "| %s | %s | %d | %d | %d | %d | %d (%d + %d) | %.1f | %d "
            "| %.3f (%.3f .. %.3f) | %.3f | %.1f | %.2f |"
            % (label, name, M, info["entries"], info["levels"],
               info["widest_level"], info["launches"], chains,
               info["launches"] - chains, float(np.median(an)), k, sm,
               min(solve), max(solve), mm, sm / mm,
               1e3 * sm / max(info["launches"], 1)))
        d_B.free()
        d_X.free()
    plan.release()
    d.release()
    for ln in lines:
        print("LINE " + json.dumps(ln), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--only", default="stencil5,stencil27")
    ap.add_argument("--n5", type=int, default=3162)
    ap.add_argument("--n27", type=int, default=215)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--label", default="")
    ap.add_argument("--one", default="", help=argparse.SUPPRESS)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.one:
        import spmv_scpa_amd as S
        sh = S.trsv_shape()
        label = a.label or "G = %d, small_rows = %d" % (sh["group"],
                                                        sh["small_rows"])
        return one(a.one, a.n5 if a.one == "stencil5" else a.n27, a.reps,
                   label)
    lines = [COLUMNS]
    for which in a.only.split(","):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one",
                            which, "--n5", str(a.n5), "--n27", str(a.n27),
                            "--reps", str(a.reps), "--label", a.label],
                           stdout=subprocess.PIPE, text=True)
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("LINE ")]
        if r.returncode or not got:
            raise SystemExit("%s: exit status %d\n%s" % (which, r.returncode,
                                                         r.stdout))
        lines += [json.loads(g[5:]) for g in got]
        print("\n".join(lines[-3:]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        print("wrote", a.out)


if __name__ == "__main__":
    main()
