#!/usr/bin/env python3
"""Measure compact HLL handles (16-bit column offsets, spmv_hll_to_index16)
against the 4-byte handle of the same matrix, and write the table of
profiles/index16.md.

Method (as profiles/f32_values.md): one process, the matrices generated on the
device; for every (matrix, value type, kernel id) the two handles are timed in
turns -- 4-byte, compact, 4-byte, compact -- two rounds of time(warmup=3,
iters=20) each, every launch between its own event pair; a figure is the
median over a handle's 40 launches.  Fractions of the 8 TB/s roofline are
priced on kernel_bytes().  Before anything is timed, y of the compact handle
is compared bit for bit with y of launch(1) on the 4-byte handle, at the timed
size.  Nothing is asserted about speed.

    python tools/index16_ratio.py [--rows 10000000] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import spmv_scpa_amd as S  # noqa: E402

PEAK = 8.0e12

HEADER = """# 16-bit column offsets against 4-byte columns, column-major HLL

Written by `tools/index16_ratio.py` on one MI355X; what the numbers say is in
DESIGN.md section 14. Every matrix is generated on the device (`to_f32()`,
`to_hll(True)`, `to_index16()`). The 4-byte handle of the same matrix in the
same process is the yardstick: the two handles are timed in turns (4-byte,
compact, 4-byte, compact; `time(warmup=3, iters=20)` each, every launch between
its own event pair), median over a handle's 40 launches. `of 8 TB/s` prices
`kernel_bytes()`; `bytes` is the ratio of the two handles' `kernel_bytes()`.
Both handles run in their default workgroup order (grouped, at this size) with
the default `waves_per_block`. No cache flush: the matrices are far beyond the
Infinity Cache. `y` of every compact launch configuration had the bits of
`launch(1)` on the 4-byte handle before it was timed.

"""


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--out", default=os.path.join(
        os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
        "index16.md"))
    a = ap.parse_args()
    M = N = a.rows
    tag = "%gM x 32" % (M / 1e6)
    workloads = (("banded " + tag, S.SYNTH_BANDED, 0),
                 ("random %s, W = 2^11" % tag, S.SYNTH_RANDOM, 1 << 11))
    x, y = S.DevBuffer(N * 8), S.DevBuffer(M * 8)
    S.dev_fill_synth(x.ptr, N, 7)
    lines = ["| workload | values | kernel | 4-byte ms | of 8 TB/s | compact ms "
             "| of 8 TB/s | ratio | bytes |",
             "|---|---|---|---|---|---|---|---|---|"]
    for name, kind, W in workloads:
        d64 = S.CsrDevice.generate(kind, M, N, 32, W, 0, 42)
        d32 = d64.to_f32()
        for vname, d in (("f64", d64), ("f32", d32)):
            h4 = d.to_hll(True)
            h2 = h4.to_index16()
            h4.launch(1, x.ptr, y.ptr)
            S.stream_sync()
            y_ref = y.to_numpy(np.float64, M)
            for k in (1, 2):
                h2.launch(k, x.ptr, y.ptr)
                S.stream_sync()
                if not np.array_equal(bits(y.to_numpy(np.float64, M)),
                                      bits(y_ref)):
                    raise SystemExit("%s %s kernel %d: y differs from the "
                                     "4-byte handle's" % (name, vname, k))
            for k in (1, 2):
                ms = {4: [], 2: []}
                for _ in range(2):
                    for h in (h4, h2):
                        ms[h.index_bytes] += list(h.time(k, x.ptr, y.ptr, 3, 20))
                t4, t2 = float(np.median(ms[4])), float(np.median(ms[2]))
                b4, b2 = h4.kernel_bytes(k), h2.kernel_bytes(k)
                lines.append("| %s | %s | %d | %.4f | %.3f | %.4f | %.3f | %.3f "
                             "| %.3f |" % (name, vname, k, t4,
                                           b4 / (t4 * 1e-3) / PEAK, t2,
                                           b2 / (t2 * 1e-3) / PEAK, t2 / t4,
                                           b2 / b4))
                print(lines[-1], flush=True)
            h2.release()
            h4.release()
        d32.release()
        d64.release()
    with open(a.out, "w") as f:
        f.write(HEADER + "\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
