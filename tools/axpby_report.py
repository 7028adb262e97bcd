#!/usr/bin/env python3
"""Measure launch_axpby (Y = alpha A X + beta Y in place) against launch_multi
(Y = A X) on the same handle in the same process, and write the table of
profiles/axpby.md.

Method (as tools/multi_vector_report.py): the handles are generated on the
device; every (handle, k) is timed in two alternating rounds -- multi, axpby
with beta = 0, axpby with beta = 1 -- of 3 warm-ups and 20 launches between
two events (the scheme of tests/test_gpu_axpby.py); a figure is the mean of
its two rounds.  `bytes` is axpby_bytes(k, 1) / multi_bytes(k): what reading Y
adds to the launch by the byte model.

    python tools/axpby_report.py [--rows 4000000] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import spmv_scpa_amd as S  # noqa: E402

PEAK = 8.0e12
KS = (1, 2, 4, 8)

HEADER = """# Y = alpha A X + beta Y in place against Y = A X

Written by `tools/axpby_report.py` on one MI355X; what the numbers say is in
DESIGN.md section 15. Every handle is generated on the device (`to_f32()`,
`to_hll(True)` for the others). `multi` is `launch_multi` on the same handle with
the same `k`: the kernels of `launch_axpby` without the epilogue. A (handle, k)
pair is timed multi, axpby (beta = 0), axpby (beta = 1), twice over: two
alternating rounds of 3 warm-ups and 20 launches between two events, both rounds
shown for the yardstick, the mean of the two for the others. `bytes` is
`axpby_bytes(k, 1) / multi_bytes(k)`; `of 8 TB/s` prices `axpby_bytes(k, 1)` on
the beta = 1 launch. No cache flush: the matrices are far beyond the Infinity
Cache.

"""


def ms_per_launch(launch, warmup=3, iters=20):
    for _ in range(warmup):
        launch()
    e0, e1 = S.Event(), S.Event()
    e0.record()
    for _ in range(iters):
        launch()
    e1.record()
    return e0.elapsed_ms(e1) / iters


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--out", default=os.path.join(
        os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
        "axpby.md"))
    a = ap.parse_args()
    M = N = a.rows
    tag = "%gM x 32" % (M / 1e6)
    workloads = (("banded " + tag, S.SYNTH_BANDED, 0),
                 ("random %s, W = 2^11" % tag, S.SYNTH_RANDOM, 1 << 11))
    X, Y = S.DevBuffer(N * 8 * 8), S.DevBuffer(M * 8 * 8)
    S.dev_fill_synth(X.ptr, N * 8, 7)
    S.dev_fill_synth(Y.ptr, M * 8, 9)
    lines = ["| workload | handle | k | multi ms (round 1 / 2) | beta = 0 ms | "
             "/ multi | beta = 1 ms | / multi | bytes | of 8 TB/s |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for name, kind, W in workloads:
        d64 = S.CsrDevice.generate(kind, M, N, 32, W, 0, 42)
        d32 = d64.to_f32()
        hs = (("csr f64", d64), ("csr f32", d32),
              ("hll f64", d64.to_hll(True)), ("hll f32", d32.to_hll(True)))
        for label, m in hs:
            for k in KS:
                tm, t0, t1 = [], [], []
                for _ in range(2):
                    tm.append(ms_per_launch(
                        lambda: m.launch_multi(X.ptr, Y.ptr, k)))
                    t0.append(ms_per_launch(
                        lambda: m.launch_axpby(-1.0, 0.0, X.ptr, Y.ptr, k)))
                    t1.append(ms_per_launch(
                        lambda: m.launch_axpby(-1.0, 1.0, X.ptr, Y.ptr, k)))
                s, b0, b1 = (float(np.mean(t)) for t in (tm, t0, t1))
                lines.append(
                    "| %s | %s | %d | %.4f / %.4f | %.4f | %.3f | %.4f | %.3f "
                    "| %.3f | %.3f |"
                    % (name, label, k, tm[0], tm[1], b0, b0 / s, b1, b1 / s,
                       m.axpby_bytes(k, 1.0) / m.multi_bytes(k),
                       m.axpby_bytes(k, 1.0) / (b1 * 1e-3) / PEAK))
                print(lines[-1], flush=True)
        for _, m in hs:
            m.release()
    with open(a.out, "w") as f:
        f.write(HEADER + "\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
