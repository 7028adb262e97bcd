#!/usr/bin/env python3
"""Time the sparse product of CSR handles (spmv_csr_spgemm, CsrDevice.matmul)
and the Galerkin product made of it, and write the table of
profiles/spgemm.md.

Cases (built on the host, rows ascending):
  stencil5:AA     A A of the five-point stencil on an n x n grid
  stencil5:AP     A P, P the 2 x 2 aggregates of that grid
  stencil5:PTAP   P^T (A P), the second product of the Galerkin pair
  stencil27:AP    A P, the 27-point stencil on m x m x m, 2 x 2 x 2 aggregates
  stencil27:PTAP  P^T (A P) there
  banded:AAT      A A^T of the synthetic banded matrix, 1M rows x 16 a row

Method: one process per case; this script starts itself.  At a reduced size
the product is first compared bit for bit with tests/_spgemm.py.  Then, at
full size, `--reps` blocking calls between two host clock readings after one
warm-up; median (min .. max).  The phases are the library's own host-clock
split of the call (S.spgemm_last_phases(): checks and bounds; class lists and
symbolic pass; scan, allocation and numeric pass; the part of the last two
spent in the fallback's launches), medians over the same calls.

The yardsticks are things the library had before the product existed:
  transpose   transpose() of the resulting C, timed the same way: the same
              output bytes through the existing conversion
  model       read A, the gathered rows of B twice (once per pass), write C:
              4 (M + 1) + 12 NZ_A + 2 * 12 products + 4 (M + 1) + 12 NZ_C
              bytes at the 8 TB/s that profiles/transpose.md prices its
              model with
Nothing is asserted about speed.  rocsparse is not timed by this tool.

    python tools/spgemm_report.py [--only stencil5:AA,...] [--n 3162]
        [--m 215] [--rows 1000000] [--reps 5] [--limit 600] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ilu0_report import host_ms, pattern, span  # noqa: E402

CASES = ("stencil5:AA", "stencil5:AP", "stencil5:PTAP", "stencil27:AP",
         "stencil27:PTAP", "banded:AAT")
HEAD = ("| case | M x K x N | products | nz of C | rows in class 0 / 1 / 2 / "
        "fallback | matmul ms (min .. max) | bound | symbolic | numeric | "
        "of which fallback | transpose(C) ms | matmul / transpose | model ms "
        "| matmul / model |\n" + "|---" * 14 + "|")
STREAM_BYTES_PER_MS = 8e9  # 8 TB/s: the rate of profiles/transpose.md's model


def stencil(dims):
    """(M, M, IRP, JA, AS): diagonal = neighbours, off-diagonals -1"""
    M, IRP, JA, side, neighbours = pattern(dims, len(dims) == 3)
    return M, M, IRP, JA, np.where(side == 0, float(neighbours), -1.0)


def aggregates(dims):
    """P: one 1.0 per row at the row's aggregate of 2 points a direction"""
    M = int(np.prod(dims))
    coords = np.unravel_index(np.arange(M), dims)
    coarse = [(d + 1) // 2 for d in dims]
    agg = np.ravel_multi_index([c // 2 for c in coords], coarse)
    return (M, int(np.prod(coarse)), np.arange(M + 1, dtype=np.int32),
            agg.astype(np.int32), np.ones(M))


def upload(S, mat):
    M, N, IRP, JA, AS = mat
    A = S.csr_from_arrays("spgemm", M, N, IRP, JA, AS)
    d = S.CsrDevice.upload(A)
    S.csr_free(A)
    return d


def arrays(S, d):
    p = d.download()
    out = tuple(a.copy() for a in S.csr_arrays(p))
    S.csr_free(p)
    return out


def operands(S, case, a, small):
    """-> (dA, dB, host pair or None) of the product the case times"""
    name, what = case.split(":")
    if name == "banded":
        rows = 2000 if small else a.rows
        dA = S.CsrDevice.generate(S.SYNTH_BANDED, rows, rows, 16, 0)
        dB = dA.transpose()
        host = None
        if small:
            I, J, V = arrays(S, dA)
            TI, TJ, TV = arrays(S, dB)
            host = ((rows, rows, I, J, V), (rows, rows, TI, TJ, TV))
        return dA, dB, host
    if name == "stencil5":
        dims = (40, 40) if small else (a.n, a.n)
    else:
        dims = (12, 12, 12) if small else (a.m, a.m, a.m)
    A, P = stencil(dims), aggregates(dims)
    dA = upload(S, A)
    if what == "AA":
        return dA, dA, (A, A)
    dP = upload(S, P)
    if what == "AP":
        return dA, dP, (A, P)
    dAP = dA.matmul(dP)
    dPT = dP.transpose()
    host = None
    if small:
        import _spgemm as SG
        host = (SG.transpose(P), (A[0], P[1]) + SG.reference(A, P))
    return dPT, dAP, host


def one(case, a):
    import _spgemm as SG
    import spmv_scpa_amd as S
    # 1. the bits, at a reduced size
    dA, dB, host = operands(S, case, a, True)
    dC = dA.matmul(dB)
    got, want = arrays(S, dC), SG.reference(*host)
    if not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            and np.array_equal(got[2].view(np.uint64),
                               want[2].view(np.uint64))):
        raise SystemExit("%s: the product differs from the reference" % case)
    print("%s: the reduced size matches the reference" % case,
          file=sys.stderr, flush=True)
    del dC, dA, dB
    # 2. full size
    dA, dB, _ = operands(S, case, a, False)
    dC = dA.matmul(dB)  # warm-up: code objects, the allocator
    info = dC.spgemm_info
    phases = []

    def product():
        dA.matmul(dB).release()
        phases.append(S.spgemm_last_phases())

    ms = host_ms(product, a.reps)
    dC.transpose().release()
    tr = host_ms(lambda: dC.transpose().release(), a.reps)
    med = {k: float(np.median([p[k] for p in phases])) for k in phases[0]}
    model = (4 * (dA.M + 1) + 12 * dA.NZ + 2 * 12 * info.products
             + 4 * (dA.M + 1) + 12 * info.nz) / STREAM_BYTES_PER_MS
    m, t = float(np.median(ms)), float(np.median(tr))
    print("ROW " + json.dumps(
        "| %s | %d x %d x %d | %d | %d | %s | %s | %.2f | %.2f | %.2f | %.2f "
        "| %s | %.2f | %.3f | %.1f |" % (
            case, dA.M, dA.N, dB.N, info.products, info.nz,
            " / ".join(str(n) for n in info.rows_in_bin), span(ms),
            med["bound"], med["symbolic"], med["numeric"], med["fallback"],
            span(tr), m / t, model, m / model)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--only", default=",".join(CASES))
    ap.add_argument("--n", type=int, default=3162)
    ap.add_argument("--m", type=int, default=215)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=600,
                    help="seconds one case's process may take")
    ap.add_argument("--one", default="", help=argparse.SUPPRESS)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.one:
        return one(a.one, a)
    table = [HEAD]
    for case in a.only.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", case]
        for f in ("n", "m", "rows", "reps"):
            cmd += ["--" + f, str(getattr(a, f))]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True,
                               timeout=a.limit)
        except subprocess.TimeoutExpired:
            raise SystemExit("%s: not done after %d s" % (case, a.limit))
        got = [ln.split(" ", 1)[1] for ln in r.stdout.splitlines()
               if ln.startswith("ROW ")]
        if r.returncode or not got:
            raise SystemExit("%s: exit status %d\n%s" % (case, r.returncode,
                                                         r.stdout))
        table.append(json.loads(got[0]))
        print(table[-1], flush=True)
        if a.out:  # after every case: a run cut short keeps what it has
            with open(a.out, "w") as f:
                f.write("\n".join(table) + "\n")
    if a.out:
        print("wrote", a.out)


if __name__ == "__main__":
    main()
