"""What tests/test_index16.py and tests/test_gpu_index16.py share: the cases of
the compact-handle tests (spmv_hll_to_index16) and a numpy packer that states
the stored form -- one base column per hack block, a 16-bit offset per slot --
independently of the library."""
import glob
import os

import numpy as np

import _oracle as O
import spmv_scpa_amd as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HLL_WIDE = 512  # hack blocks wider than this are refused (-ENOTSUP)


def _loads(path):
    try:
        S.csr_free(S.io_load_csr(path))
        return True
    except OSError:
        return False


#: every .mtx of tests/golden that the loader accepts
MTX = sorted(os.path.basename(p)[:-4]
             for p in glob.glob(os.path.join(GOLDEN, "*.mtx")) if _loads(p))

#: tag, kind, M (= N), K, W -- the project's small cases
SYNTH = [
    ("banded", S.SYNTH_BANDED, 50_000, 16, 0),
    ("random_narrow", S.SYNTH_RANDOM, 40_000, 32, 512),
    # ragged last block (20 011 = 625 * 32 + 11) and an odd block count (626)
    ("ragged", S.SYNTH_RAGGED, 20_011, 32, 4096),
    ("stencil27", S.SYNTH_STENCIL, 40_000, 27, 0),
]
CASES = ["synth:" + t[0] for t in SYNTH] + ["mtx:" + n for n in MTX]


def case_arrays(case):
    """-> (M, N, IRP, JA, AS, x)"""
    if case.startswith("mtx:"):
        A = S.io_load_csr(os.path.join(GOLDEN, case[4:] + ".mtx"))
        IRP, JA, AS = (a.copy() for a in S.csr_arrays(A))
        M, N = A.contents.M, A.contents.N
        S.csr_free(A)
        return M, N, IRP, JA, AS, S.vec_random(N)
    tag, kind, M, K, W = next(t for t in SYNTH if t[0] == case[6:])
    IRP, JA, AS = O.synth_csr(kind, M, M, K, W, 42)
    return M, M, IRP, JA, AS, O.synth_x(7, 0, M)


def pack16(IRP, JA, AS):
    """The stored form of a compact handle, from the oracle's padded HLL.

    -> dict(off, pad, ja, base, off16, span, width): `pad` marks the slots
    that are padding (JA == -1 before the rewrite), `ja` the columns after the
    pad rewrite, base[b] the smallest column among the non-pad slots of block
    b (0 when it has none), off16 = ja - base with 0 where that lies outside
    0..65535 (only pads can), span[b] = largest - smallest valid column,
    width[b] the block's columns."""
    M = len(IRP) - 1
    off, maxnz, _, HJA, _ = O.csr_to_hll(IRP, JA, AS, True)
    pad = HJA < 0
    ja = O.hll_fix_pads(M, True, off, maxnz, HJA) if len(HJA) else HJA
    nb = len(off) - 1
    base = np.zeros(nb, np.int32)
    span = np.zeros(nb, np.int64)
    off16 = np.zeros(len(HJA), np.uint16)
    for b in range(nb):
        sl = slice(int(off[b]), int(off[b + 1]))
        valid = ja[sl][~pad[sl]]
        if len(valid):
            base[b] = valid.min()
            span[b] = int(valid.max()) - int(valid.min())
        d = ja[sl].astype(np.int64) - int(base[b])
        d[(d < 0) | (d > 65535)] = 0
        off16[sl] = d
    return dict(off=off, pad=pad, ja=ja, base=base, off16=off16, span=span,
                width=np.asarray(maxnz, np.int64))


def fits(p):
    """the errno a conversion must answer, 0 when it converts"""
    import errno
    if len(p["width"]) and p["width"].max() > HLL_WIDE:
        return errno.ENOTSUP
    if len(p["span"]) and p["span"].max() > 65535:
        return errno.ERANGE
    return 0
