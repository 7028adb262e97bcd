#!/usr/bin/env python3
"""Time the device-side transposition of CSR handles (spmv_csr_transpose)
against the route a user had before it -- download(), a stable sort on the
host, upload() -- and write the table of profiles/transpose.md.

Method: one process per matrix (this script starts itself once per matrix, so
no process holds two of them).  In each, the result is first compared byte
for byte with tests/_transpose.py `reference` at a reduced size; then, at full
size, the conversion is run five times, each between two host clock readings
(the call blocks, and it includes the hipMalloc / hipFree of its scratch and
the O(rows) host work of every new handle) -- median and spread of the five;
then the host route is timed once, in the same process; then autotune picks a
kernel for y = A x and for y = A^T x.  The byte model prices what the plan
must move at 8 TB/s: per pass the keys read twice (histogram, scatter; 4 bytes
in pass 0, the pairs' 8 after) and the pairs written once, the column count's
read of JA, and the gather (positions, values, JA and values of T); counters
and IRP are left out.  Nothing is asserted about speed.

    python tools/transpose_time.py [--rows 10000000] [--out FILE]
                                   [--only banded,random,kkt] [--kkt-n 160]
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

PEAK = 8.0e12

HEADER = """# Device-side transposition of CSR handles

Written by `tools/transpose_time.py` on one MI355X, one process per matrix;
what the numbers say is in DESIGN.md section 19. `device ms` is the median of
five `transpose()` calls, each between two host clock readings (the call
blocks; it includes the allocation of its scratch and the host work every new
handle needs), `min .. max` their spread. `host route s` is `download()`,
`tests/_transpose.py reference`, `upload()` in the same process, once.
`model ms` prices the plan's bytes at 8 TB/s (per pass: keys read twice, pairs
written once; the column count; the gather), `reached` is model / device.
`A` and `A^T` are `autotune`'s pick and median ms for one product on the
source and on its transpose. Before anything was timed, the device result was
compared byte for byte with the reference at a reduced size.

"""

COLUMNS = ("| matrix | rows x cols | entries | passes | tile | scratch MB "
           "| device ms | min .. max | model ms | reached | host route s "
           "| A: kernel, ms | A^T: kernel, ms |\n"
           "|---|---|---|---|---|---|---|---|---|---|---|---|---|")


def model_bytes(plan, NZ, value_bytes):
    b = 4 * NZ  # the column count reads JA
    for p in range(plan["passes"]):
        key = 4 if p == 0 else 8
        b += 2 * key * NZ + 8 * NZ
    b += 4 * NZ + 2 * value_bytes * NZ + 4 * NZ  # the gather
    return b


def same(S, TR, d, T):
    def arrays(h):
        p = h.download()
        out = tuple(a.copy() for a in S.csr_arrays(p))
        S.csr_free(p)
        return out
    IRP, JA, AS = arrays(d)
    want = TR.reference(IRP, JA, AS, d.N)
    got = arrays(T)
    return (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            and np.array_equal(got[2].view(np.uint64),
                               want[2].view(np.uint64)))


def make(S, which, rows, kkt_n):
    if which == "banded":
        return ("banded %gM x 32" % (rows / 1e6),
                S.CsrDevice.generate(S.SYNTH_BANDED, rows, rows, 32, 0, 0, 42))
    if which == "random":
        return ("random %gM x 32, columns anywhere" % (rows / 1e6),
                S.CsrDevice.generate(S.SYNTH_RANDOM, rows, rows, 32, 1 << 30,
                                     0, 42))
    from benchlib.common import config4_file
    path, info = config4_file("", kkt_n)
    A = S.io_load_csr_cached(path)
    d = S.CsrDevice.upload(A)
    S.csr_free(A)
    return "KKT, %d^3 grid (config 4)" % kkt_n, d


def one(which, rows, kkt_n):
    import _transpose as TR
    import spmv_scpa_amd as S
    # 1. the bytes, at a reduced size
    name, small = make(S, which, min(rows, 200_000), min(kkt_n, 20))
    T = small.transpose()
    if not same(S, TR, small, T):
        raise SystemExit("%s: the result differs from the reference" % name)
    T.release()
    small.release()
    print("%s: the reduced size matches the reference" % name,
          file=sys.stderr, flush=True)
    # 2. the time, at full size
    name, d = make(S, which, rows, kkt_n)
    plan = S.transpose_plan(d.N, d.NZ)
    d.transpose().release()  # warm-up: code objects, the allocator
    ms = []
    for _ in range(5):
        t0 = time.perf_counter()
        T = d.transpose()
        ms.append((time.perf_counter() - t0) * 1e3)
        T.release()
    print("%s: device ms %s" % (name, " ".join("%.2f" % m for m in ms)),
          file=sys.stderr, flush=True)
    # 3. the route without it
    t0 = time.perf_counter()
    p = d.download()
    IRP, JA, AS = S.csr_arrays(p)
    tI, tJ, tA = TR.reference(IRP, JA, AS, d.N)
    S.csr_free(p)
    H = S.csr_from_arrays("t", d.N, d.M, tI, tJ, tA)
    hT = S.CsrDevice.upload(H)
    host_s = time.perf_counter() - t0
    print("%s: host route %.1f s" % (name, host_s), file=sys.stderr,
          flush=True)
    S.csr_free(H)
    hT.release()
    del tI, tJ, tA
    # 4. one product on A and on A^T
    T = d.transpose()
    picks = []
    for h in (d, T):
        x, y = S.DevBuffer(h.N * 8), S.DevBuffer(h.M * 8)
        S.dev_fill_synth(x.ptr, h.N, 7)
        k, t = h.autotune(x.ptr, y.ptr)
        picks.append("%s, %.3f" % (S.CSR_KERNEL_LABELS[k], t))
        x.free()
        y.free()
    med = float(np.median(ms))
    model = model_bytes(plan, d.NZ, d.value_bytes) / PEAK * 1e3
    line = ("| %s | %d x %d | %d | %d | %d | %.0f | %.2f | %.2f .. %.2f | %.2f "
            "| %.3f | %.1f | %s | %s |"
            % (name, d.M, d.N, d.NZ, plan["passes"], plan["tile"],
               plan["scratch_bytes"] / 1e6, med, min(ms), max(ms), model,
               model / med, host_s, picks[0], picks[1]))
    T.release()
    d.release()
    print("LINE " + json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--kkt-n", type=int, default=160)
    ap.add_argument("--only", default="banded,random,kkt")
    ap.add_argument("--one", default="", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles",
                                                  "transpose.md"))
    a = ap.parse_args()
    if a.one:
        return one(a.one, a.rows, a.kkt_n)
    lines = [COLUMNS]
    for which in a.only.split(","):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one",
                            which, "--rows", str(a.rows), "--kkt-n",
                            str(a.kkt_n)], stdout=subprocess.PIPE, text=True)
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("LINE ")]
        if r.returncode or not got:
            raise SystemExit("%s: exit status %d\n%s" % (which, r.returncode,
                                                         r.stdout))
        lines.append(json.loads(got[-1][5:]))
        print(lines[-1], flush=True)
    with open(a.out, "w") as f:
        f.write(HEADER + "\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
