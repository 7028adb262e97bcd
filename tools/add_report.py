#!/usr/bin/env python3
"""Time the sparse sum of CSR handles (spmv_csr_add, CsrDevice.add) and its
companions, and write the table of profiles/add.md.

Cases (rows ascending):
  convdiff5:A+AT   A + A^T of the five-point convection-diffusion stencil on
                   an n x n grid (the symmetric part, every column matched)
  stencil5:A-sI    A - 1.3 I of the five-point stencil on n x n, I from
                   from_diag (one match a row)
  stencil27:A+A    the 27-point stencil on m x m x m plus itself (one handle)
  banded:half      the synthetic band, `rows` x 32, plus the same band
                   shifted by 16 columns: half of every row matched

Method: ONE process.  At a reduced size every sum is first compared byte for
byte with tests/_add.py, in the three modes of add_set_class.  Then, at full
size, `--reps` blocking calls between two host clock readings after one
warm-up; median (min .. max).  The phases are the library's own host-clock
split of the call (S.add_last_phases(): checks; count pass and scan;
allocation, fill pass and the finishing of the handle), medians over the same
calls.  The split per class is the same sum timed with add_set_class(1) (lane
groups only) and (2) (a workgroup a row; skipped above --wg-rows rows, where
it is a launch of millions of workgroups).  scale() and from_diag() are timed
the same way on the case's matrix.

The yardsticks:
  transpose   transpose() of the resulting C, timed the same way: the same
              output bytes through the existing conversion
  model       read the two patterns twice (both passes) and the values once,
              write C: 4 (nzA + nzB) + 12 (nzA + nzB) + 12 nzC bytes plus the
              row pointers 4 (M + 1) * 5 (A's and B's in both passes, C's
              once), at the stream rate THIS process measures: launch_axpby
              of the identity handle (from_diag) on a vector of 2^24 doubles,
              40 bytes a row, timed with events
Nothing is asserted about speed.  rocsparse is not timed by this tool.

    python tools/add_report.py [--only convdiff5:A+AT,...] [--n 3162]
        [--m 215] [--rows 10000000] [--reps 5] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ilu0_report import host_ms, pattern, span  # noqa: E402

CASES = ("convdiff5:A+AT", "stencil5:A-sI", "stencil27:A+A", "banded:half")
HEAD = ("| case | M x N | nzA + nzB | nz of C | matched | width | add ms "
        "(min .. max) | checks | count + scan | alloc + fill + finish | "
        "groups only ms | workgroups only ms | transpose(C) ms | add / "
        "transpose | model ms | add / model | scale(l, r) ms | from_diag ms "
        "|\n" + "|---" * 18 + "|")


def stencil(dims, c=0.0):
    """(M, M, IRP, JA, AS): diagonal = neighbours, off-diagonals -1 -+ c"""
    M, IRP, JA, side, neighbours = pattern(dims, len(dims) == 3)
    return M, M, IRP, JA, np.where(side == 0, float(neighbours),
                                   -1.0 + c * side)


def upload(S, mat):
    M, N, IRP, JA, AS = mat
    A = S.csr_from_arrays("add", M, N, IRP, JA, AS)
    d = S.CsrDevice.upload(A)
    S.csr_free(A)
    return d


def arrays(S, d):
    p = d.download()
    out = tuple(a.copy() for a in S.csr_arrays(p))
    S.csr_free(p)
    return out


def operands(S, case, a, small):
    """-> (alpha, dA, beta, dB) of the sum the case times"""
    name = case.split(":")[0]
    if name == "banded":
        rows = 3000 if small else a.rows
        return (1.0, S.CsrDevice.generate(S.SYNTH_BANDED, rows, rows + 64, 32,
                                          0),
                1.0, S.CsrDevice.generate(S.SYNTH_BANDED, rows, rows + 64, 32,
                                          0, row0=16))
    if name == "stencil27":
        dA = upload(S, stencil((12,) * 3 if small else (a.m,) * 3))
        return 1.0, dA, 1.0, dA
    n = 40 if small else a.n
    if name == "convdiff5":
        dA = upload(S, stencil((n, n), 0.5))
        return 1.0, dA, 1.0, dA.transpose()
    dA = upload(S, stencil((n, n)))
    return 1.0, dA, -1.3, S.CsrDevice.from_diag(dA.M)


def stream_bytes_per_ms(S, n=1 << 24, reps=20):
    """launch_axpby of the identity on a vector: 40 n bytes a launch"""
    dI = S.CsrDevice.from_diag(n)
    d_x, d_y = S.DevBuffer(n * 8), S.DevBuffer(n * 8)
    S._lib.spmv_dev_memset(d_x.ptr, 0, n * 8, None)
    S._lib.spmv_dev_memset(d_y.ptr, 0, n * 8, None)
    ms = []
    for i in range(reps + 2):
        e0, e1 = S.Event(), S.Event()
        e0.record()
        dI.launch_axpby(1.5, 0.5, d_x.ptr, d_y.ptr)
        e1.record()
        S.stream_sync()
        if i >= 2:
            ms.append(e0.elapsed_ms(e1))
    for b in (d_x, d_y):
        b.free()
    dI.release()
    return 40.0 * n / float(np.median(ms))


def check_small(S, case, a):
    import _add as AD
    alpha, dA, beta, dB = operands(S, case, a, True)
    A = (dA.M, dA.N) + arrays(S, dA)
    B = (dB.M, dB.N) + arrays(S, dB)
    want = AD.reference(alpha, A, beta, B)
    for mode in (0, 1, 2):
        S.add_set_class(mode)
        got = arrays(S, dA.add(dB, alpha, beta))
        if not (np.array_equal(got[0], want[0])
                and np.array_equal(got[1], want[1])
                and np.array_equal(got[2].view(np.uint64),
                                   want[2].view(np.uint64))):
            raise SystemExit("%s, mode %d: the sum differs from the "
                             "reference" % (case, mode))
    S.add_set_class(0)
    print("%s: the reduced size matches the reference in every mode" % case,
          file=sys.stderr, flush=True)


def one(S, case, a, rate):
    check_small(S, case, a)
    alpha, dA, beta, dB = operands(S, case, a, False)
    dC = dA.add(dB, alpha, beta)  # warm-up: code objects, the allocator
    info = dC.add_info
    phases = []

    def add():
        dA.add(dB, alpha, beta).release()
        phases.append(S.add_last_phases())

    ms = host_ms(add, a.reps)
    med = {k: float(np.median([p[k] for p in phases])) for k in phases[0]}
    by_class = []
    for mode in (1, 2):
        if mode == 2 and dA.M > a.wg_rows:
            by_class.append("-")
            continue
        S.add_set_class(mode)
        dA.add(dB, alpha, beta).release()
        by_class.append(span(host_ms(
            lambda: dA.add(dB, alpha, beta).release(), a.reps)))
    S.add_set_class(0)
    dC.transpose().release()
    tr = host_ms(lambda: dC.transpose().release(), a.reps)
    dC.release()
    d_l, d_r = S.DevBuffer(dA.M * 8), S.DevBuffer(dA.N * 8)
    S._lib.spmv_dev_memset(d_l.ptr, 0, dA.M * 8, None)
    S._lib.spmv_dev_memset(d_r.ptr, 0, dA.N * 8, None)
    dA.scale(d_l.ptr, d_r.ptr).release()
    sc = host_ms(lambda: dA.scale(d_l.ptr, d_r.ptr).release(), a.reps)
    S.CsrDevice.from_diag(dA.M, d_l.ptr).release()
    fd = host_ms(lambda: S.CsrDevice.from_diag(dA.M, d_l.ptr).release(),
                 a.reps)
    for b in (d_l, d_r):
        b.free()
    both = dA.NZ + dB.NZ
    model = (16 * both + 12 * info.nz + 20 * (dA.M + 1)) / rate
    m, t = float(np.median(ms)), float(np.median(tr))
    width = [w for w in S.add_shape()["widths"]
             if w * dA.M >= both or w == 32][0]
    return ("| %s | %d x %d | %d | %d | %d | %d | %s | %.2f | %.2f | %.2f | "
            "%s | %s | %s | %.2f | %.3f | %.1f | %s | %s |" % (
                case, dA.M, dA.N, both, info.nz, info.matched, width,
                span(ms), med["checks"], med["count"], med["fill"],
                by_class[0], by_class[1], span(tr), m / t, model, m / model,
                span(sc), span(fd)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--only", default=",".join(CASES))
    ap.add_argument("--n", type=int, default=3162)
    ap.add_argument("--m", type=int, default=215)
    ap.add_argument("--rows", type=int, default=10000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--wg-rows", type=int, default=20000000,
                    help="most rows the workgroups-only mode is timed on")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import spmv_scpa_amd as S
    rate = stream_bytes_per_ms(S)
    head = "stream rate (launch_axpby of the identity, 2^24 rows): " \
        "%.2f TB/s\n" % (rate / 1e9)
    print(head, flush=True)
    table = [head, HEAD]
    for case in a.only.split(","):
        table.append(one(S, case, a, rate))
        print(table[-1], flush=True)
        if a.out:  # after every case: a run cut short keeps what it has
            with open(a.out, "w") as f:
                f.write("\n".join(table) + "\n")
    if a.out:
        print("wrote", a.out)


if __name__ == "__main__":
    main()
