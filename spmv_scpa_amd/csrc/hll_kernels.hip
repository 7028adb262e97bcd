/*
 * hll_kernels.hip -- fp64 HLL (hacked ELLPACK, hack = 32) SpMV kernels for
 * gfx950 (wave64).  Templates over the handle's STORED value type V (double,
 * or float: 8 B per slot instead of 12); x, y, products and sums are fp64.
 *
 * Four kernels fill the four slots of the reference's driver table
 * (reference cuda_hll.cu:19-152, main.c:310-315); the designs are new.
 * Device layout: one JA slab and one AS slab; hack block b occupies slots
 * [off[b], off[b+1]) with rows_b = min(32, M - 32 b) rows and width
 * w_b = (off[b+1] - off[b]) / rows_b; pads already point at a valid column
 * and carry the value 0.0 (hip_hll.h).
 *
 *   0 threads_row_major  lane per row; slot(i,j) = i*w + j.
 *   1 threads_col_major  lane per row; a 64-lane wavefront owns TWO hack
 *                        blocks (lanes 0-31 / 32-63).  Each block's slab is
 *                        contiguous, so the wavefront copies it to LDS in
 *                        chunks of 8 columns with 16 B/lane loads (1 KiB per
 *                        instruction, fully coalesced), then every lane
 *                        walks its row out of LDS (conflict-free: lane i
 *                        reads word j*32+i) and gathers x.
 *   2 wave_block         same mapping, direct global loads, no LDS.
 *   3 subwave_row        16 lanes per row over row-major blocks,
 *                        __shfl_down(width 16) reduction.
 *
 * Kernels 1 and 2 are templates over the handle's INDEX type as well (cols32 /
 * cols16 below): 4-byte columns, or on a "compact" handle one base column per
 * hack block and a 16-bit offset per slot (spmv_hll_to_index16, DESIGN.md
 * section 14),
 *
 *     column of slot t of block b = base16[b] + off16[t]
 *
 * 10 bytes per slot instead of 12 (fp64 values), 6 instead of 8 (fp32).  Slot
 * order, off[], values and the order of the sums are the same for both, and
 * so are the bits of y: acc = 0.0, one fused multiply-add per column in column
 * order, pads included.
 *
 * No MFMA (no dense contraction).  JA/AS stream once -> non-temporal loads;
 * x gathers are ordinary cached loads.
 */
#include <algorithm>
#include "hip_common.h"

typedef int v4i __attribute__((ext_vector_type(4)));
typedef double v2d __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef unsigned short u16;

/* ------------------------------------------------------------------ */
/* index types of the col-major kernels: where the column of a slot is  */
/* ------------------------------------------------------------------ */
struct cols32 { /* 4-byte columns: the handle's ja */
    typedef int slot_t;
    typedef const int *__restrict__ arg; /* a plain pointer kernel argument */
    static constexpr bool compact = false;
    static constexpr bool wide_blocks = true; /* k_hll_wide may own blocks */
    static arg of(const spmv_hll_dev *H) { return H->ja; }
    static __device__ __forceinline__ const int *slots(const int *a) { return a; }
    static __device__ __forceinline__ int base(const int *, int) { return 0; }
};
struct cols16 { /* compact handle: base16[b] + off16[t] */
    typedef u16 slot_t;
    struct arg {
        const int *base16;
        const u16 *off16;
    };
    static constexpr bool compact = true; /* ids 1 / 2 only, no experiment arms */
    static constexpr bool wide_blocks = false; /* the conversion refused them */
    static arg of(const spmv_hll_dev *H) { return arg{H->base16, H->off16}; }
    static __device__ __forceinline__ const u16 *slots(arg a) { return a.off16; }
    static __device__ __forceinline__ int base(arg a, int b) { return a.base16[b]; }
};

/* ------------------------------------------------------------------ */
/* pad rewrite on the device (reference cuda_hll.cu:173-195 does it on  */
/* the host, block by block): pad -> previous valid column, or 0.        */
/* ------------------------------------------------------------------ */
/* also records which slots were pads (bit t of padmask, zeroed by the    */
/* caller): the blocked copy drops exactly those, never an explicit zero */
__global__ void k_hll_fix_pads(int M, int col_major,
                               const int64_t *__restrict__ off,
                               int *__restrict__ ja,
                               unsigned *__restrict__ padmask) {
    int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= M)
        return;
    int b = row / HACK, i = row % HACK;
    int rows = min(HACK, M - b * HACK);
    int64_t o = off[b];
    int w = (int)((off[b + 1] - o) / rows);
    int last = 0;
    for (int j = 0; j < w; ++j) {
        int64_t t = o + (col_major ? (int64_t)j * rows + i : (int64_t)i * w + j);
        int c = ja[t];
        if (c < 0) {
            ja[t] = last;
            atomicOr(padmask + (t >> 5), 1u << (t & 31));
        } else {
            last = c;
        }
    }
}

int hll_fix_pads_dev(spmv_hll_dev *H, hipStream_t s) {
    if (H->M == 0)
        return 0;
    HIP_RET(hipMemsetAsync(H->padmask, 0,
                           (((size_t)H->slots + 31) / 32 + 1) * sizeof(unsigned),
                           s));
    hipLaunchKernelGGL(k_hll_fix_pads, dim3((H->M + 255) / 256), dim3(256), 0,
                       s, H->M, H->col_major, H->off, H->ja, H->padmask);
    return hip_errno(hipGetLastError());
}

/* ------------------------------------------------------------------ */
/* conversion: 4-byte columns -> base + 16-bit offsets                   */
/* ------------------------------------------------------------------ */
/* One wavefront per hack block (at most 32 x HLL_WIDE slots: the caller has
 * refused wide blocks).  Pass 1: min / max over the slots that were entries
 * before the pad rewrite (bit t of padmask clear).  Pass 2: the offsets.  A
 * pad that points outside [base, base + 65535] -- the column-0 pad of an
 * empty row in a block whose columns start further right -- gets offset 0:
 * its value is 0.0 and its product a zero wherever it points. */
__global__ void __launch_bounds__(WAVE)
    k_hll16_convert(int nb, const int64_t *__restrict__ off,
                    const int *__restrict__ ja,
                    const unsigned *__restrict__ padmask,
                    int *__restrict__ base, u16 *__restrict__ off16,
                    unsigned *overflow) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= nb)
        return;
    const int64_t o = off[b];
    const int n = (int)(off[b + 1] - o);
    int lo = 0x7fffffff, hi = -1;
    for (int t = lane; t < n; t += WAVE) {
        const int64_t g = o + t;
        const int c = ja[g];
        if (!((padmask[g >> 5] >> (g & 31)) & 1u)) {
            lo = min(lo, c);
            hi = max(hi, c);
        }
    }
#pragma unroll
    for (int d = WAVE / 2; d > 0; d >>= 1) {
        lo = min(lo, __shfl_xor(lo, d, WAVE));
        hi = max(hi, __shfl_xor(hi, d, WAVE));
    }
    const int bs = hi < 0 ? 0 : lo; /* no entry at all (width 0): base 0 */
    if (lane == 0)
        base[b] = bs;
    if (hi >= 0 && hi - lo > 65535) {
        if (lane == 0)
            atomicOr(overflow, 1u);
        return;
    }
    for (int t = lane; t < n; t += WAVE) {
        const int d = ja[o + t] - bs;
        off16[o + t] = (u16)(d < 0 || d > 65535 ? 0 : d);
    }
}

int hll16_convert_dev(const spmv_hll_dev *src, spmv_hll_dev *dst,
                      unsigned *d_overflow, hipStream_t s) {
    if (!src || !dst || !d_overflow || dst->nb != src->nb ||
        dst->slots != src->slots)
        return -EINVAL;
    if (src->nb == 0)
        return 0;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_hll16_convert, dim3(src->nb), dim3(WAVE), 0, s, src->nb,
                       src->off, src->ja, src->padmask, dst->base16, dst->off16,
                       d_overflow);
    return hip_errno(hipGetLastError());
}

/* ------------------------------------------------------------------ */
/* 0: lane per row, row-major                                           */
/* ------------------------------------------------------------------ */
/* `wide` > 0 (kernels 0-3): the matrix has hack blocks of more than `wide`
 * columns; they are left to k_hll_wide, launched right after on the same
 * stream */
template <typename V>
__global__ void k_hll_row_major(int M, int b0, int b1, int wide,
                                const int64_t *__restrict__ off,
                                const int *__restrict__ ja,
                                const V *__restrict__ as,
                                const double *__restrict__ x,
                                double *__restrict__ y) {
    long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    int b = b0 + (int)(t / HACK), i = (int)(t % HACK);
    if (b >= b1)
        return;
    int rows = min(HACK, M - b * HACK);
    if (i >= rows)
        return;
    int64_t o = off[b];
    int w = hack_block_width(off, b, rows);
    if (wide > 0 && w > wide)
        return;
    const int *rj = ja + o + (int64_t)i * w;
    const V *ra = as + o + (int64_t)i * w;
    /* the row's slots in order, four loads in flight (hip_common.h) */
    y[(int64_t)b * HACK + i] = strided_dot<1, 4>(rj, ra, x, 0, w, 0);
}

/* ------------------------------------------------------------------ */
/* 2: wavefront per pair of hack blocks, col-major, direct loads        */
/*    Software pipelined: while the x gathers of columns [j, j+U) are    */
/*    in flight the JA/AS loads of [j+U, j+2U) are already issued, so    */
/*    the stream never waits behind a gather round trip.                 */
/*    On 16-bit offsets the index is one 2-byte load per lane and column */
/*    (64 contiguous bytes per block and column).                        */
/* ------------------------------------------------------------------ */
/*
 * Workgroup -> hack blocks.  REMAP: workgroups are dealt round-robin over the
 * 8 XCDs; XCD k runs the CONTIGUOUS block range [xr.first[k], xr.first[k+1])
 * so that neighbouring row tiles (which share their x window) meet in one L2
 * (+18 % on a band of 2048 columns), and the ranges hold about equal numbers
 * of SLOTS, not of blocks: a matrix whose rows are wider in one half
 * otherwise leaves XCDs idle (the finding of round 2 on the blocked path,
 * DESIGN.md section 4).  The launch has 8 x (longest range) workgroups; the
 * surplus ones of shorter ranges exit.
 */
template <typename V, int U, int ORDER, int ABL = 0, /* ABL 1: all gathers read x[0] */
          typename IX = cols32>
__global__ void k_hll_col_direct(int M, int b0, int b1, int wide, xcd_ranges xr,
                                 const int64_t *__restrict__ off,
                                 typename IX::arg ix,
                                 const V *__restrict__ as,
                                 const double *__restrict__ x,
                                 double *__restrict__ y) {
    static_assert(ABL == 0 || !IX::compact, "the ABL arm is 4-byte only");
    int b, i;
    if (ORDER == 1) {
        const int xx = blockIdx.x % NUM_XCD, kk = blockIdx.x / NUM_XCD;
        const long long t = (long long)kk * blockDim.x + threadIdx.x;
        b = xr.first[xx] + (int)(t / HACK);
        i = (int)(t % HACK);
        if (b >= xr.first[xx + 1])
            return;
    } else if (ORDER == 2) { /* groups of XCD_GROUP workgroups per XCD */
        const long long w = xcd_grouped<unsigned, int, long long>(blockIdx.x);
        const long long t = w * blockDim.x + threadIdx.x;
        b = b0 + (int)(t / HACK);
        i = (int)(t % HACK);
    } else {
        const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
        b = b0 + (int)(t / HACK);
        i = (int)(t % HACK);
    }
    if (b >= b1)
        return;
    int rows = min(HACK, M - b * HACK);
    if (i >= rows)
        return;
    const int64_t o = off[b];
    const int w = hack_block_width(off, b, rows);
    if (IX::wide_blocks && wide > 0 && w > wide)
        return;
    const int bs = IX::base(ix, b);
    const typename IX::slot_t *cj = IX::slots(ix) + o + i;
    const V *ca = as + o + i;
    double acc = 0.0;
    int cJ[U];
    V cA[U];
    const int nfull = w / U;
    if (nfull > 0) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            cJ[u] = ld_stream(cj + u * rows);
            cA[u] = ld_stream(ca + u * rows);
        }
    }
    for (int c = 0; c < nfull; ++c) {
        double xv[U];
        V av[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            xv[u] = (ABL & 1) ? x[cJ[u] & 1] : x[bs + cJ[u]];
            av[u] = cA[u];
        }
        if (c + 1 < nfull) {
            const typename IX::slot_t *nj = cj + (size_t)(c + 1) * U * rows;
            const V *na = ca + (size_t)(c + 1) * U * rows;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                cJ[u] = ld_stream(nj + u * rows);
                cA[u] = ld_stream(na + u * rows);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            acc += widen(av[u]) * xv[u];
    }
    for (int j = nfull * U; j < w; ++j)
        acc += widen(ld_stream(ca + (size_t)j * rows)) *
               x[bs + (int)ld_stream(cj + (size_t)j * rows)];
    __builtin_nontemporal_store(acc, y + (int64_t)b * HACK + i);
}

/* ------------------------------------------------------------------ */
/* 1: lane per row, col-major, hack blocks staged through LDS           */
/*    (full 32-row blocks only; the launcher sends a ragged tail block  */
/*    to k_hll_col_direct)                                              */
/* ------------------------------------------------------------------ */
#define CH 8                     /* columns per staged chunk */
#define CH_SLOTS (CH * HACK)     /* 256 slots: 1 KiB of JA, 2 KiB of AS */

/* a chunk in registers, values and indices apart.  Values: every lane loads
 * 16 B pieces of both blocks. */
template <typename V> struct val_chunk;
template <> struct val_chunk<double> {
    v2d aA0, aA1, aB0, aB1;
};
/* fp32 values: a chunk's 256 values are 1 KiB -- one 16 B/lane load per block */
template <> struct val_chunk<float> {
    v4f aA, aB;
};
/* 4-byte columns: 1 KiB per block, a lane's four indices of either block.
 * 16-bit offsets: 512 B per block, so ONE 16 B/lane load fetches both blocks'
 * -- j is the 8 offsets at slots s0 + 8 (lane & 31) of the lane's OWN block
 * (lanes 0-31 block A, 32-63 block B) */
template <typename IX> struct idx_chunk;
template <> struct idx_chunk<cols32> {
    v4i jA, jB;
};
template <> struct idx_chunk<cols16> {
    v4i j;
};

/* coalesced 16 B/lane loads of slots [s0, s0+256) of the wavefront's two
 * blocks, predicated past the end of each block (a block's slot count is a
 * multiple of 32, so every 16-byte piece is wholly inside or wholly outside) */
__device__ __forceinline__ void chunk_load(val_chunk<double> &c, int s0, int lane,
                                           const double *gaA, const double *gaB,
                                           int nA, int nB) {
    const int sa = s0 + 2 * lane; /* 2 doubles, twice */
    const v2d zd = {0, 0};
    c.aA0 = sa < nA ? ld_stream((const v2d *)(gaA + sa)) : zd;
    c.aA1 = sa + 128 < nA ? ld_stream((const v2d *)(gaA + sa + 128)) : zd;
    c.aB0 = sa < nB ? ld_stream((const v2d *)(gaB + sa)) : zd;
    c.aB1 = sa + 128 < nB ? ld_stream((const v2d *)(gaB + sa + 128)) : zd;
}
__device__ __forceinline__ void chunk_load(val_chunk<float> &c, int s0, int lane,
                                           const float *gaA, const float *gaB,
                                           int nA, int nB) {
    const int sa = s0 + 4 * lane; /* 4 floats */
    const v4f zf = {0, 0, 0, 0};
    c.aA = sa < nA ? ld_stream((const v4f *)(gaA + sa)) : zf;
    c.aB = sa < nB ? ld_stream((const v4f *)(gaB + sa)) : zf;
}
__device__ __forceinline__ void chunk_load(idx_chunk<cols32> &c, int s0, int lane,
                                           const int *gjA, const int *gjB, int nA,
                                           int nB) {
    const int sj = s0 + 4 * lane; /* 4 ints */
    const v4i zi = {0, 0, 0, 0};
    c.jA = sj < nA ? ld_stream((const v4i *)(gjA + sj)) : zi;
    c.jB = sj < nB ? ld_stream((const v4i *)(gjB + sj)) : zi;
}
__device__ __forceinline__ void chunk_load(idx_chunk<cols16> &c, int s0, int lane,
                                           const u16 *gjA, const u16 *gjB, int nA,
                                           int nB) {
    const int sj = s0 + 8 * (lane & 31); /* 8 offsets */
    const v4i zi = {0, 0, 0, 0};
    const u16 *gj = lane < HACK ? gjA : gjB;
    c.j = sj < (lane < HACK ? nA : nB) ? ld_stream((const v4i *)(gj + sj)) : zi;
}

/* a chunk into the wavefront's LDS slices (two blocks x CH_SLOTS each) */
__device__ __forceinline__ void chunk_store(const val_chunk<double> &c,
                                            double *s_as, int lane) {
    *(v2d *)(s_as + 2 * lane) = c.aA0;
    *(v2d *)(s_as + 128 + 2 * lane) = c.aA1;
    *(v2d *)(s_as + CH_SLOTS + 2 * lane) = c.aB0;
    *(v2d *)(s_as + CH_SLOTS + 128 + 2 * lane) = c.aB1;
}
__device__ __forceinline__ void chunk_store(const val_chunk<float> &c,
                                            float *s_as, int lane) {
    *(v4f *)(s_as + 4 * lane) = c.aA;
    *(v4f *)(s_as + CH_SLOTS + 4 * lane) = c.aB;
}
__device__ __forceinline__ void chunk_store(const idx_chunk<cols32> &c, int *s_ja,
                                            int lane) {
    *(v4i *)(s_ja + 4 * lane) = c.jA;
    *(v4i *)(s_ja + CH_SLOTS + 4 * lane) = c.jB;
}
/* lane l's 16 bytes land at byte 16 l of the wavefront's 1 KiB: block A's 256
 * offsets, then block B's */
__device__ __forceinline__ void chunk_store(const idx_chunk<cols16> &c, u16 *s_ja,
                                            int lane) {
    *(v4i *)(s_ja + 8 * lane) = c.j;
}

template <int ORDER, typename V, typename IX>
__global__ void k_hll_col_lds(int b0, int b1, int wide, xcd_ranges xr,
                              const int64_t *__restrict__ off,
                              typename IX::arg ix,
                              const V *__restrict__ as,
                              const double *__restrict__ x,
                              double *__restrict__ y) {
    /* per wavefront: two blocks x (256 values + 256 indices) = 6 KiB (fp64
     * values) or 4 KiB (fp32) with 4-byte columns, 5 / 3 KiB with 16-bit
     * offsets: values of all wavefronts first, then indices (every carve is a
     * multiple of 16 bytes) */
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = threadIdx.x / WAVE;
    const int waves = blockDim.x / WAVE;
    V *s_as = (V *)lds_raw + (size_t)wave * 2 * CH_SLOTS;
    typedef typename IX::slot_t slot_t;
    slot_t *s_ja = (slot_t *)((V *)lds_raw + (size_t)waves * 2 * CH_SLOTS) +
                   (size_t)wave * 2 * CH_SLOTS;

    int bA; /* wave-uniform */
    if (ORDER == 1) {
        const int xx = blockIdx.x % NUM_XCD, kk = blockIdx.x / NUM_XCD;
        bA = xr.first[xx] + 2 * (kk * waves + wave);
        if (xr.first[xx + 1] < b1)
            b1 = xr.first[xx + 1]; /* the pair stays inside the XCD's range */
    } else if (ORDER == 2) { /* groups of XCD_GROUP workgroups per XCD */
        const int w = xcd_grouped<unsigned, int>(blockIdx.x);
        bA = b0 + 2 * (w * waves + wave);
    } else {
        bA = b0 + 2 * ((int)blockIdx.x * waves + wave);
    }
    if (bA >= b1)
        return;
    const bool hasB = bA + 1 < b1;
    const int64_t oA = off[bA], oB = off[bA + 1];
    /* slots of block A = 32 * wA; 64-bit until the wide blocks are out (a
     * hub block of 2^26 columns and more does not fit an int) */
    const int64_t nA64 = oB - oA, nB64 = hasB ? off[bA + 2] - oB : 0;
    /* a wide block of the pair is k_hll_wide's: nothing read, nothing stored */
    const bool skipA = IX::wide_blocks && wide > 0 && (nA64 >> 5) > wide;
    const bool skipB = IX::wide_blocks && wide > 0 && (nB64 >> 5) > wide;
    const int nA = skipA ? 0 : (int)nA64;
    const int nB = skipB ? 0 : (int)nB64;
    const int half = lane >> 5, i = lane & 31;
    const int w = (half ? nB : nA) >> 5;
    const int nmax = nA > nB ? nA : nB;
    const int bs = half ? (hasB ? IX::base(ix, bA + 1) : 0) : IX::base(ix, bA);

    const slot_t *gjA = IX::slots(ix) + oA, *gjB = IX::slots(ix) + oB;
    const V *gaA = as + oA, *gaB = as + oB;
    const slot_t *lj = s_ja + half * CH_SLOTS + i;
    const V *la = s_as + half * CH_SLOTS + i;
    double acc = 0.0;

    /* register-staged pipeline: chunk c+1 is in flight from HBM while chunk
     * c is consumed out of LDS */
    idx_chunk<IX> curj;
    val_chunk<V> cura;
    chunk_load(curj, 0, lane, gjA, gjB, nA, nB);
    chunk_load(cura, 0, lane, gaA, gaB, nA, nB);
    for (int s0 = 0; s0 < nmax; s0 += CH_SLOTS) {
        chunk_store(curj, s_ja, lane);
        chunk_store(cura, s_as, lane);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        /* this lane's 8 columns out of LDS, their x gathers issued first */
        const int c0 = s0 >> 5;
        int cc[CH];
        V av[CH];
        double xv[CH];
#pragma unroll
        for (int jj = 0; jj < CH; ++jj) {
            cc[jj] = bs + (int)lj[jj * HACK];
            av[jj] = la[jj * HACK];
        }
#pragma unroll
        for (int jj = 0; jj < CH; ++jj)
            xv[jj] = (c0 + jj < w) ? x[cc[jj]] : 0.0;
        if (s0 + CH_SLOTS < nmax) {
            chunk_load(curj, s0 + CH_SLOTS, lane, gjA, gjB, nA, nB);
            chunk_load(cura, s0 + CH_SLOTS, lane, gaA, gaB, nA, nB);
        }
#pragma unroll
        for (int jj = 0; jj < CH; ++jj)
            if (c0 + jj < w)
                acc += (double)av[jj] * xv[jj];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    if (half == 0 ? !skipA : (hasB && !skipB))
        __builtin_nontemporal_store(acc, y + (int64_t)(bA + half) * HACK + i);
}

/* ------------------------------------------------------------------ */
/* 3: 16 lanes per row, row-major                                       */
/* ------------------------------------------------------------------ */
template <typename V>
__global__ void k_hll_subwave_row(int M, int b0, int b1, int wide,
                                  const int64_t *__restrict__ off,
                                  const int *__restrict__ ja,
                                  const V *__restrict__ as,
                                  const double *__restrict__ x,
                                  double *__restrict__ y) {
    const int sub = threadIdx.x & 15;
    /* grid-stride over the rows: 16 work-items per row are more than one
     * launch holds (2^32) beyond 2^28 rows.  The trip count is the same for
     * every lane of a wavefront (`first` is the wavefront's first row); rows
     * past the end are masked */
    const long long total = (long long)(b1 - b0) * HACK;
    const long long step = ((long long)gridDim.x * blockDim.x) >> 4;
    const long long lane_g = (threadIdx.x & (WAVE - 1)) >> 4;
    for (long long first =
             (((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 4) - lane_g;
         first < total; first += step) {
        const long long g = first + lane_g;
        const int b = b0 + (int)(g / HACK), i = (int)(g % HACK);
        double acc = 0.0;
        bool live = false;
        if (g < total) {
            int rows = min(HACK, M - b * HACK);
            if (i < rows) {
                int64_t o = off[b];
                int w = hack_block_width(off, b, rows);
                live = !(wide > 0 && w > wide);
                const int *rj = ja + o + (int64_t)i * w;
                const V *ra = as + o + (int64_t)i * w;
                if (live)
                    acc = strided_dot<16, 4>(rj, ra, x, 0, w, sub);
            }
        }
#pragma unroll
        for (int d = 8; d > 0; d >>= 1)
            acc += __shfl_down(acc, d, 16);
        if (live && sub == 0)
            y[(int64_t)b * HACK + i] = acc;
    }
}

/* ------------------------------------------------------------------ */
/* wide hack blocks (> HLL_WIDE columns): workgroup g sums one segment of  */
/* columns (seg.y wide) of block b for all its rows, either layout; the    */
/* block's last segment to arrive adds the partial row sums in a fixed      */
/* order (deterministic), writes y and re-arms the counter.                */
/* ------------------------------------------------------------------ */
template <typename V>
__global__ void __launch_bounds__(256)
    k_hll_wide(int M, int b0, int b1, int col_major,
               const int4 *__restrict__ seg, const int64_t *__restrict__ off,
               const int *__restrict__ ja, const V *__restrict__ as,
               const double *__restrict__ x, double *__restrict__ y,
               double *part, unsigned long long *cnt, unsigned epoch) {
    __shared__ double red[8][HACK];
    __shared__ int s_seen;
    const int g = blockIdx.x, tid = threadIdx.x;
    const int4 sg = seg[g];
    const int b = sg.x, segw = sg.y, kseg = sg.z, nseg = sg.w;
    if (b < b0 || b >= b1)
        return; /* another launch of a chunked exchange owns this block */
    const int rows = min(HACK, M - b * HACK);
    const int64_t o = off[b];
    const int w = hack_block_width(off, b, rows);
    const int j0 = min(kseg * segw, w), j1 = min(j0 + segw, w);
    /* col-major: a wavefront reads two columns x 32 rows, each 256 B
     * contiguous; row-major: eight neighbouring columns of a row per 8 lanes */
    const int i = col_major ? (tid & 31) : (tid >> 3);
    const int cl = col_major ? (tid >> 5) : (tid & 7);
    double acc = 0.0;
    if (i < rows) {
        /* slot of column j of row i; the lane's columns are j0 + cl, + 8, ...
         * Eight of them in flight at a time, added in column order (one
         * accumulator): one at a time is two dependent memory round trips
         * per slot, 32 times over -- the launch was latency, not bandwidth */
        const int64_t base = o + (col_major ? i : (int64_t)i * w);
        const int64_t step = col_major ? rows : 1;
        int j = j0 + cl;
        constexpr int U = 8;
        for (; j + 8 * (U - 1) < j1; j += 8 * U) {
            int c[U];
            V v[U];
            double xv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t t = base + (int64_t)(j + 8 * u) * step;
                c[u] = ld_stream(ja + t);
                v[u] = ld_stream(as + t);
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                xv[u] = x[c[u]];
#pragma unroll
            for (int u = 0; u < U; ++u)
                acc += widen(v[u]) * xv[u];
        }
        for (; j < j1; j += 8) {
            const int64_t t = base + (int64_t)j * step;
            acc += widen(ld_stream(as + t)) * x[ld_stream(ja + t)];
        }
    }
    red[cl][i] = acc;
    __syncthreads();
    if (tid < HACK) {
        double t = 0.0;
#pragma unroll
        for (int c = 0; c < 8; ++c)
            t += red[c][tid];
        __hip_atomic_store(part + (size_t)g * HACK + tid, t, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    const int g0 = g - kseg;
    if (tid == 0) /* epoch_arrive (hip_common.h): 1 .. nseg */
        s_seen = (int)epoch_arrive(cnt + g0, epoch);
    __syncthreads();
    if (s_seen != nseg)
        return;
    /* the block's last segment: 8 lanes per row add every 8th segment's
     * partial, then the eight are added in lane order -- a fixed order */
    {
        const int r = tid & 31, c = tid >> 5;
        const double sum = ordered_partial_sum<8>(part + (size_t)g0 * HACK + r,
                                                  nseg, c, 8, HACK);
        __syncthreads(); /* red[] of the column lanes is no longer needed */
        red[c][r] = sum;
    }
    __syncthreads();
    if (tid < rows) {
        double sum = 0.0;
#pragma unroll
        for (int c = 0; c < 8; ++c)
            sum += red[c][tid];
        y[(int64_t)b * HACK + tid] = sum;
    }
    if (tid == 0)
        epoch_rearm(cnt + g0, epoch);
}

/* ------------------------------------------------------------------ */
template <typename V, typename IX>
static int hll_launch_t(const spmv_hll_dev *H, int kernel, int waves,
                        int variant, const double *x, double *y, int b0,
                        int b1, hipStream_t s) {
    (void)hipGetLastError(); /* an earlier caller's unread error is not ours */
    if (!H || !x || !y || b0 < 0 || b1 > H->nb || b0 > b1)
        return -EINVAL;
    if ((kernel == 0 || kernel == 3) == (H->col_major != 0))
        return -EINVAL; /* layout of the handle does not fit the kernel */
    if (IX::compact && kernel != 1 && kernel != 2)
        return -EINVAL; /* a compact handle is col-major: ids 1 and 2 only */
    /* product build: only the documented bits (spmv_engine.h: 0, 1, 2 the
     * workgroup orders; 29 belongs to the timed loops).  The ablation arms
     * (bits 4-6: pipeline depths, an arm whose result is wrong by design) are
     * compiled only with -DSPMV_ABLATIONS (make abl), and for 4-byte columns
     * only: a compact handle refuses them in either build flavour */
#ifdef SPMV_ABLATIONS
    constexpr bool arms = !IX::compact;
#else
    constexpr bool arms = false;
#endif
    if (!arms && (variant & ~(1 | 2 | 4 | SPMV_VARIANT_TIMING_BITS)))
        return -EINVAL;
    if (b0 == b1)
        return 0;
    /* workgroup order: variant bit 0 hardware, bit 1 XCD ranges, bit 2
     * grouped; none: the handle's (0 hardware / 1 ranges / 2 grouped) */
    const int order = (variant & 1) ? 0 : (variant & 2) ? 1 : (variant & 4) ? 2
                                                        : H->order;
    const int threads = waves * WAVE;
    const long long lanes = (long long)(b1 - b0) * HACK;
    const int wide = IX::wide_blocks && H->n_wide_seg > 0 ? HLL_WIDE : 0;
    const V *as = values_of<V>(H);
    const typename IX::arg ix = IX::of(H);
    /* XCD ranges of this launch: the handle's slot-balanced table for the
     * whole matrix, an even split for a block sub-range (multi-GPU chunks) */
    xcd_ranges xr = H->xcd_blk;
    if (b0 != 0 || b1 != H->nb)
        for (int k = 0; k <= NUM_XCD; ++k) {
            long long c = b0 + ((long long)(b1 - b0) * k / NUM_XCD + 1) / 2 * 2;
            xr.first[k] = k == NUM_XCD || c > b1 ? b1 : (int)c;
        }
    int xmax = 0; /* longest range, in blocks */
    for (int k = 0; k < NUM_XCD; ++k)
        xmax = xr.first[k + 1] - xr.first[k] > xmax
                   ? xr.first[k + 1] - xr.first[k] : xmax;
    switch (kernel) {
    case 0:
        hipLaunchKernelGGL(k_hll_row_major<V>,
                           dim3((unsigned)((lanes + threads - 1) / threads)),
                           dim3(threads), 0, s, H->M, b0, b1, wide, H->off,
                           H->ja, as, x, y);
        break;
    case 1: {
        /* full blocks through LDS; a ragged last block goes direct */
        int full_end = b1;
        if (b1 == H->nb && (H->M % HACK) != 0)
            full_end = b1 - 1;
        if (full_end > b0) {
            int pairs = (full_end - b0 + 1) / 2;
            size_t lds = (size_t)waves * 2 * CH_SLOTS *
                         (sizeof(V) + sizeof(typename IX::slot_t));
            const int nwg = (pairs + waves - 1) / waves;
            if (order == 1)
                hipLaunchKernelGGL((k_hll_col_lds<1, V, IX>),
                                   dim3(NUM_XCD * (((xmax + 1) / 2 + waves - 1) /
                                                   waves)),
                                   dim3(threads), lds, s, b0, full_end, wide, xr,
                                   H->off, ix, as, x, y);
            else if (order == 2)
                hipLaunchKernelGGL((k_hll_col_lds<2, V, IX>),
                                   dim3(grouped_grid(nwg)), dim3(threads), lds,
                                   s, b0, full_end, wide, xr, H->off, ix, as,
                                   x, y);
            else
                hipLaunchKernelGGL((k_hll_col_lds<0, V, IX>), dim3(nwg), dim3(threads),
                                   lds, s, b0, full_end, wide, xr, H->off, ix,
                                   as, x, y);
        }
        if (full_end < b1)
            hipLaunchKernelGGL((k_hll_col_direct<V, 8, 0, 0, IX>), dim3(1),
                               dim3(WAVE), 0, s, H->M, full_end, b1, wide, xr,
                               H->off, ix, as, x, y);
        break;
    }
    case 2: {
        /* REMAP grid: 8 x (workgroups of the longest XCD range) */
        const unsigned xgrid =
            NUM_XCD * (unsigned)(((long long)xmax * HACK + threads - 1) / threads);
        if constexpr (arms) { /* experiment arms: `make abl` builds them */
            if (variant & 32) { /* tuning: 4 columns per pipeline stage */
                hipLaunchKernelGGL((k_hll_col_direct<V, 4, 1>), dim3(xgrid),
                                   dim3(threads), 0, s, H->M, b0, b1, wide, xr,
                                   H->off, ix, as, x, y);
                break;
            }
            if (variant & 64) { /* tuning: 16 columns per pipeline stage */
                hipLaunchKernelGGL((k_hll_col_direct<V, 16, 1>), dim3(xgrid),
                                   dim3(threads), 0, s, H->M, b0, b1, wide, xr,
                                   H->off, ix, as, x, y);
                break;
            }
            if (variant & 16) { /* ABL 1: every gather reads x[0..1]: WRONG y */
                hipLaunchKernelGGL((k_hll_col_direct<V, 8, 1, 1>), dim3(xgrid),
                                   dim3(threads), 0, s, H->M, b0, b1, wide, xr,
                                   H->off, ix, as, x, y);
                break;
            }
        }
        const unsigned hwgrid = (unsigned)((lanes + threads - 1) / threads);
        if (order == 1)
            hipLaunchKernelGGL((k_hll_col_direct<V, 8, 1, 0, IX>), dim3(xgrid),
                               dim3(threads), 0, s, H->M, b0, b1, wide, xr, H->off,
                               ix, as, x, y);
        else if (order == 2)
            hipLaunchKernelGGL((k_hll_col_direct<V, 8, 2, 0, IX>),
                               dim3(grouped_grid(hwgrid)), dim3(threads), 0, s,
                               H->M, b0, b1, wide, xr, H->off, ix, as, x, y);
        else
            hipLaunchKernelGGL((k_hll_col_direct<V, 8, 0, 0, IX>), dim3(hwgrid),
                               dim3(threads), 0, s, H->M, b0, b1, wide, xr, H->off,
                               ix, as, x, y);
        break;
    }
    case 3:
        hipLaunchKernelGGL(
            k_hll_subwave_row<V>,
            dim3((unsigned)std::min<long long>((lanes * 16 + threads - 1) / threads,
                                               0xFFFFFFFFll / threads)),
            dim3(threads), 0, s, H->M, b0, b1, wide, H->off, H->ja, as, x,
            y);
        break;
    default:
        return -EINVAL;
    }
    if (wide > 0)
        hipLaunchKernelGGL(k_hll_wide<V>, dim3(H->n_wide_seg), dim3(256), 0, s,
                           H->M, b0, b1, H->col_major, H->wide_seg, H->off,
                           H->ja, as, x, y, H->wide_part, H->wide_cnt,
                           next_launch_epoch(&H->launch_epoch));
    return hip_errno(hipGetLastError());
}

/* dispatch on the handle's index and value types (hip_common.h: index_bytes,
 * value_bytes); `waves` is 1..16 (kernel 1: at most 8, engine.hip
 * launch_direct) */
int hll_launch_kernel(const spmv_hll_dev *H, int kernel, int waves,
                      int variant, const double *x, double *y, int b0, int b1,
                      hipStream_t s) {
    const bool f32 = H && H->value_bytes == 4;
    if (H && H->index_bytes == 2) {
        if (!H->off16 || !H->base16)
            return -EINVAL;
        return f32 ? hll_launch_t<float, cols16>(H, kernel, waves, variant, x, y,
                                                 b0, b1, s)
                   : hll_launch_t<double, cols16>(H, kernel, waves, variant, x,
                                                  y, b0, b1, s);
    }
    return f32 ? hll_launch_t<float, cols32>(H, kernel, waves, variant, x, y, b0,
                                             b1, s)
               : hll_launch_t<double, cols32>(H, kernel, waves, variant, x, y,
                                              b0, b1, s);
}
