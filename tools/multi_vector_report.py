#!/usr/bin/env python3
"""Measure launch_multi (Y = A X, k interleaved vectors) against k launches of
the single-vector kernel of the same summation order (CSR kernel 2, HLL kernel
1) on the same handle, and write the table of profiles/multi_vector.md.

Method (as profiles/f32_values.md): one process, the handles generated on the
device, every (handle, k) timed in two alternating rounds -- single, multi,
single, multi -- of 3 warm-ups and 20 launches, each launch between its own
event pair, median per round; a figure is the mean of its two round medians.
Fractions of the 8 TB/s roofline are priced on multi_bytes(k).

    python tools/multi_vector_report.py [--rows 10000000] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import spmv_scpa_amd as S  # noqa: E402

PEAK = 8.0e12
KS = (1, 2, 4, 8)
SINGLE = {"csr": 2, "hll": 1}


HEADER = """# Y = A X for k interleaved vectors against k single-vector launches

Written by `tools/multi_vector_report.py` on one MI355X; what the numbers say is
in DESIGN.md section 13. Every handle is generated on the device (`to_f32()`,
`to_hll(True)` for the others). `single` is the kernel whose summation order
`launch_multi` repeats (CSR kernel 2 `subwave_row`, HLL kernel 1
`threads_col_major`) on the same handle with one contiguous vector. A (handle, k)
pair is timed single, multi, single, multi: two alternating rounds of 3 warm-ups
and 20 launches, every launch between its own event pair, median per round, mean
of the two rounds. `of 8 TB/s` prices `multi_bytes(k)`; `byte model` is
`multi_bytes(k) / (k * multi_bytes(1))`. No cache flush: the matrices are far
beyond the Infinity Cache.

"""


def time_multi(m, X, Y, k, warmup=3, iters=20):
    for _ in range(warmup):
        m.launch_multi(X.ptr, Y.ptr, k)
    ms = []
    e0, e1 = S.Event(), S.Event()
    for _ in range(iters):
        e0.record()
        m.launch_multi(X.ptr, Y.ptr, k)
        e1.record()
        ms.append(e0.elapsed_ms(e1))
    return float(np.median(ms))


def time_single(m, kernel, x, y):
    return float(np.median(m.time(kernel, x.ptr, y.ptr, 3, 20)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--out", default=os.path.join(
        os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
        "multi_vector.md"))
    a = ap.parse_args()
    M = N = a.rows
    tag = "%gM x 32" % (M / 1e6)
    workloads = (("banded " + tag, S.SYNTH_BANDED, 0, False),
                 ("random %s, W = 2^11" % tag, S.SYNTH_RANDOM, 1 << 11, False),
                 ("random %s, columns anywhere" % tag, S.SYNTH_RANDOM, 2 * N,
                  True))
    x, y = S.DevBuffer(N * 8), S.DevBuffer(M * 8)
    X, Y = S.DevBuffer(N * 8 * 8), S.DevBuffer(M * 8 * 8)
    S.dev_fill_synth(x.ptr, N, 7)
    S.dev_fill_synth(X.ptr, N * 8, 7)
    lines = ["| workload | handle | k | single ms | multi ms (round 1 / 2) | "
             "ms per vector | of 8 TB/s | multi / (k x single) | byte model |",
             "|---|---|---|---|---|---|---|---|---|"]
    blocked = []
    for name, kind, W, anywhere in workloads:
        d64 = S.CsrDevice.generate(kind, M, N, 32, W, 0, 42)
        d32 = d64.to_f32()
        hs = (("csr f64", "csr", d64), ("csr f32", "csr", d32),
              ("hll f64", "hll", d64.to_hll(True)),
              ("hll f32", "hll", d32.to_hll(True)))
        for label, fmt, m in hs:
            for k in KS:
                t1, tk = [], []
                for _ in range(2):
                    t1.append(time_single(m, SINGLE[fmt], x, y))
                    tk.append(time_multi(m, X, Y, k))
                s, t = float(np.mean(t1)), float(np.mean(tk))
                lines.append(
                    "| %s | %s | %d | %.4f | %.4f / %.4f | %.4f | %.3f | %.3f "
                    "| %.3f |" % (name, label, k, s, tk[0], tk[1], t / k,
                                  m.multi_bytes(k) / (t * 1e-3) / PEAK,
                                  t / (k * s),
                                  m.multi_bytes(k) / (k * m.multi_bytes(1))))
                print(lines[-1], flush=True)
        if anywhere:  # the headline path: the blocked copy, one vector
            best, _ = d64.autotune(x.ptr, y.ptr, allow_panels=True)
            tb = time_single(d64, best, x, y)
            blocked.append("%s: the selector's pick for one vector is CSR "
                           "kernel %d (%s), %.4f ms per launch; k launches: "
                           "%s ms" % (name, best,
                                      d64.panels_describe() or "direct", tb,
                                      ", ".join("k=%d %.3f" % (k, k * tb)
                                                for k in KS)))
            print(blocked[-1], flush=True)
        for _, _, m in hs:
            m.release()
    with open(a.out, "w") as f:
        f.write(HEADER + "\n".join(lines) + "\n\n" + "\n\n".join(blocked)
                + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
