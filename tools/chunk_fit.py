#!/usr/bin/env python3
"""The sweep kernel's launch shapes on one sweep copy, timed beside each other
(panel_launch.h "Chunk fit"): the built-in 512 lanes x 2 groups (chunks of
4096 slots) against 576 x 2 and 384 x 3 (4608 slots), with ordered additions
and in arrival order.  Every shape is asked for through variant bits 16-17 on
the SAME copy, the shapes alternate over `--rounds` rounds of 20 timed
launches, and a sample of rows is checked against the generator's row sums.

    python tools/chunk_fit.py [--rows 10000000] [--rounds 3] \
        > profiles/sweep_chunk_fit.shapes.md
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import spmv_scpa_amd as S  # noqa: E402

SHAPES = (("512 x 2", 3 << 16), ("576 x 2", 1 << 16), ("384 x 3", 2 << 16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--cols", type=int, default=0)
    ap.add_argument("--nnz-row", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    M, N, K = a.rows, a.cols or a.rows, a.nnz_row
    W = 2 * N
    d_x, d_y = S.DevBuffer(N * 8), S.DevBuffer(M * 8)
    S.dev_fill_synth(d_x.ptr, N, 7)
    dA = S.CsrDevice.generate(S.SYNTH_RANDOM, M, N, K, W, 0, 42)
    dH = dA.to_hll(True)
    dA.release()
    try:
        import _oracle as O
        rows = np.random.default_rng(1).integers(0, M, 64)
        want = [O.synth_row_dot(S.SYNTH_RANDOM, M, N, K, W, 0, 42, 7, int(r))
                for r in rows]
    except (ImportError, OSError):
        rows, want = [], []
    print("| additions | shape | median ms per round | median | vs 512 x 2 | "
          "rows checked |")
    print("|---|---|---|---|---|---|")
    for det in (True, False):
        dH.build_panels(0, "sweep", deterministic=det)
        steps = dH.panels_fit_steps()
        ms = {name: [] for name, _ in SHAPES}
        bad = {name: 0 for name, _ in SHAPES}
        for name, v in SHAPES:
            dH.launch(S.HLL_KERNEL_PANELS, d_x.ptr, d_y.ptr, variant=v)
            S.stream_sync()
            y = d_y.to_numpy(np.float64, M)
            bad[name] = sum(abs(y[r] - w) > 1e-12 * sc
                            for r, (w, sc) in zip(rows, want))
        for _ in range(a.rounds):
            for name, v in SHAPES:
                ms[name].append(float(np.median(dH.time(
                    S.HLL_KERNEL_PANELS, d_x.ptr, d_y.ptr, 3, 20, variant=v))))
        base = float(np.median(ms[SHAPES[0][0]]))
        for name, _ in SHAPES:
            m = float(np.median(ms[name]))
            print("| %s | %s | %s | %.4f | %+.1f %% | %d of %d wrong |" % (
                "ordered" if det else "arrival order", name,
                " ".join("%.4f" % t for t in ms[name]), m,
                100.0 * (m / base - 1.0), bad[name], len(rows)))
        print("| | %s; steps %d (4096-slot chunks) / %d (4608); default plan "
              "%s | | | | |" % (dH.panels_describe(), steps[0], steps[1],
                                "%d x %d" % dH.panels_plan()[:2]))
        sys.stdout.flush()
    dH.release()


if __name__ == "__main__":
    main()
