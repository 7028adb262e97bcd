/*
 * hll16_kernels.hip -- col-major HLL SpMV on "compact" handles for gfx950
 * (wave64): the column of a slot is stored as a 16-bit offset from one base
 * column per hack block (spmv_hll_to_index16).
 *
 *     column of slot t of block b = base[b] + off16[t]
 *
 * 10 bytes per slot instead of 12 (fp64 values), 6 instead of 8 (fp32).  The
 * slot order and off[] are the source handle's; values, x, y, products and
 * sums are what hll_kernels.hip makes of them, and so are the bits of y:
 * acc = 0.0, one fused multiply-add per column in column order, pads included.
 *
 *   convert   wavefront per hack block: min / max column over the non-pad
 *             slots (padmask of the source), base = min, offsets written;
 *             max - min > 65535 raises the overflow flag instead.
 *   1         k_hll16_col_lds: the structure of k_hll_col_lds.  A wavefront
 *             owns two full blocks and stages chunks of 8 columns through
 *             LDS.  A chunk's offsets are 512 B per block: ONE 16 B/lane load
 *             fetches both blocks' (lanes 0-31 block A, lanes 32-63 block B).
 *   2         k_hll16_col_direct: the pipeline of k_hll_col_direct, the
 *             offset read with a 2-byte load per lane and column (64
 *             contiguous bytes per block and column).  Also the ragged last
 *             block of kernel 1.
 *
 * A compact handle has no wide hack blocks (the conversion refuses them), so
 * there is no side launch and no `wide` argument.
 */
#include "hip_common.h"

typedef int v4i __attribute__((ext_vector_type(4)));
typedef double v2d __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef unsigned short u16;

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
/* 2: lane per row, direct loads (k_hll_col_direct on 16-bit offsets)    */
/* ------------------------------------------------------------------ */
template <typename V, int U, int ORDER>
__global__ void k_hll16_col_direct(int M, int b0, int b1, xcd_ranges xr,
                                   const int64_t *__restrict__ off,
                                   const int *__restrict__ base,
                                   const u16 *__restrict__ off16,
                                   const V *__restrict__ as,
                                   const double *__restrict__ x,
                                   double *__restrict__ y) {
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
    const int bs = base[b];
    const u16 *cj = off16 + o + i;
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
            xv[u] = x[bs + cJ[u]];
            av[u] = cA[u];
        }
        if (c + 1 < nfull) {
            const u16 *nj = cj + (size_t)(c + 1) * U * rows;
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
/* 1: lane per row, hack blocks staged through LDS (full blocks only)    */
/* ------------------------------------------------------------------ */
#define CH16 8                    /* columns per staged chunk */
#define CH16_SLOTS (CH16 * HACK)  /* 256 slots: 512 B of offsets per block */

/* a chunk in registers.  j: the 8 offsets at slots s0 + 8 (lane & 31) of the
 * lane's OWN block (lanes 0-31 block A, 32-63 block B): 512 contiguous bytes
 * per block, one 16 B/lane instruction for the pair.  Values as in
 * hll_kernels.hip: every lane loads for both blocks. */
template <typename V> struct hll16_chunk;
template <> struct hll16_chunk<double> {
    v4i j;
    v2d aA0, aA1, aB0, aB1;
};
template <> struct hll16_chunk<float> {
    v4i j;
    v4f aA, aB;
};

/* slots [s0, s0+256) of the wavefront's two blocks, predicated past the end
 * of each block (a block's slot count is a multiple of 32, so every 16-byte
 * piece is wholly inside or wholly outside).  gj: the lane's own block's
 * offsets, n: its slot count */
__device__ __forceinline__ void hll16_chunk_load(hll16_chunk<double> &c, int s0,
                                                 int lane, const u16 *gj, int n,
                                                 const double *gaA,
                                                 const double *gaB, int nA,
                                                 int nB) {
    const int sj = s0 + 8 * (lane & 31); /* 8 offsets */
    const int sa = s0 + 2 * lane;        /* 2 doubles, twice */
    const v4i zi = {0, 0, 0, 0};
    const v2d zd = {0, 0};
    c.j = sj < n ? ld_stream((const v4i *)(gj + sj)) : zi;
    c.aA0 = sa < nA ? ld_stream((const v2d *)(gaA + sa)) : zd;
    c.aA1 = sa + 128 < nA ? ld_stream((const v2d *)(gaA + sa + 128)) : zd;
    c.aB0 = sa < nB ? ld_stream((const v2d *)(gaB + sa)) : zd;
    c.aB1 = sa + 128 < nB ? ld_stream((const v2d *)(gaB + sa + 128)) : zd;
}

__device__ __forceinline__ void hll16_chunk_load(hll16_chunk<float> &c, int s0,
                                                 int lane, const u16 *gj, int n,
                                                 const float *gaA,
                                                 const float *gaB, int nA,
                                                 int nB) {
    const int sj = s0 + 8 * (lane & 31); /* 8 offsets */
    const int sa = s0 + 4 * lane;        /* 4 floats */
    const v4i zi = {0, 0, 0, 0};
    const v4f zf = {0, 0, 0, 0};
    c.j = sj < n ? ld_stream((const v4i *)(gj + sj)) : zi;
    c.aA = sa < nA ? ld_stream((const v4f *)(gaA + sa)) : zf;
    c.aB = sa < nB ? ld_stream((const v4f *)(gaB + sa)) : zf;
}

/* a chunk's values into the wavefront's LDS slice (two blocks x CH16_SLOTS) */
__device__ __forceinline__ void hll16_chunk_store(const hll16_chunk<double> &c,
                                                  double *s_as, int lane) {
    *(v2d *)(s_as + 2 * lane) = c.aA0;
    *(v2d *)(s_as + 128 + 2 * lane) = c.aA1;
    *(v2d *)(s_as + CH16_SLOTS + 2 * lane) = c.aB0;
    *(v2d *)(s_as + CH16_SLOTS + 128 + 2 * lane) = c.aB1;
}
__device__ __forceinline__ void hll16_chunk_store(const hll16_chunk<float> &c,
                                                  float *s_as, int lane) {
    *(v4f *)(s_as + 4 * lane) = c.aA;
    *(v4f *)(s_as + CH16_SLOTS + 4 * lane) = c.aB;
}

template <int ORDER, typename V>
__global__ void k_hll16_col_lds(int b0, int b1, xcd_ranges xr,
                                const int64_t *__restrict__ off,
                                const int *__restrict__ base,
                                const u16 *__restrict__ off16,
                                const V *__restrict__ as,
                                const double *__restrict__ x,
                                double *__restrict__ y) {
    /* per wavefront: two blocks x 256 x (value + 2-byte offset) = 5 KiB (fp64
     * values) or 3 KiB (fp32), against 6 / 4 KiB with 4-byte columns: values
     * of all wavefronts first, then the offsets (1 KiB per wavefront: every
     * carve is a multiple of 16 bytes) */
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = threadIdx.x / WAVE;
    const int waves = blockDim.x / WAVE;
    V *s_as = (V *)lds_raw + (size_t)wave * 2 * CH16_SLOTS;
    u16 *s_ja = (u16 *)((V *)lds_raw + (size_t)waves * 2 * CH16_SLOTS) +
                (size_t)wave * 2 * CH16_SLOTS;

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
    /* at most 32 x HLL_WIDE slots per block: no wide blocks here */
    const int nA = (int)(oB - oA), nB = hasB ? (int)(off[bA + 2] - oB) : 0;
    const int half = lane >> 5, i = lane & 31;
    const int n = half ? nB : nA;
    const int w = n >> 5;
    const int nmax = nA > nB ? nA : nB;
    const int bs = half ? (hasB ? base[bA + 1] : 0) : base[bA];

    const u16 *gj = off16 + (half ? oB : oA);
    const V *gaA = as + oA, *gaB = as + oB;
    const u16 *lj = s_ja + half * CH16_SLOTS + i;
    const V *la = s_as + half * CH16_SLOTS + i;
    double acc = 0.0;

    /* register-staged pipeline: chunk c+1 is in flight from HBM while chunk
     * c is consumed out of LDS */
    hll16_chunk<V> cur;
    hll16_chunk_load(cur, 0, lane, gj, n, gaA, gaB, nA, nB);
    for (int s0 = 0; s0 < nmax; s0 += CH16_SLOTS) {
        /* lane l's 16 bytes land at byte 16 l of the wavefront's 1 KiB:
         * block A's 256 offsets, then block B's */
        *(v4i *)(s_ja + 8 * lane) = cur.j;
        hll16_chunk_store(cur, s_as, lane);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        /* this lane's 8 columns out of LDS, their x gathers issued first */
        const int c0 = s0 >> 5;
        int cc[CH16];
        V av[CH16];
        double xv[CH16];
#pragma unroll
        for (int jj = 0; jj < CH16; ++jj) {
            cc[jj] = bs + (int)lj[jj * HACK];
            av[jj] = la[jj * HACK];
        }
#pragma unroll
        for (int jj = 0; jj < CH16; ++jj)
            xv[jj] = (c0 + jj < w) ? x[cc[jj]] : 0.0;
        if (s0 + CH16_SLOTS < nmax)
            hll16_chunk_load(cur, s0 + CH16_SLOTS, lane, gj, n, gaA, gaB, nA,
                             nB);
#pragma unroll
        for (int jj = 0; jj < CH16; ++jj)
            if (c0 + jj < w)
                acc += (double)av[jj] * xv[jj];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    if (half == 0 || hasB)
        __builtin_nontemporal_store(acc, y + (int64_t)(bA + half) * HACK + i);
}

/* ------------------------------------------------------------------ */
template <typename V>
static int hll16_launch_t(const spmv_hll_dev *H, int kernel, int waves,
                          int variant, const double *x, double *y, int b0,
                          int b1, hipStream_t s) {
    (void)hipGetLastError(); /* an earlier caller's unread error is not ours */
    if (!H || !x || !y || b0 < 0 || b1 > H->nb || b0 > b1)
        return -EINVAL;
    if (kernel != 1 && kernel != 2)
        return -EINVAL; /* a compact handle is col-major: ids 1 and 2 only */
    /* the workgroup orders (bits 0, 1, 2) and the timed loops' bit; compact
     * handles have no experiment arms, in either build flavour */
    if (variant & ~(1 | 2 | 4 | SPMV_VARIANT_TIMING_BITS))
        return -EINVAL;
    if (b0 == b1)
        return 0;
    const int order = (variant & 1) ? 0 : (variant & 2) ? 1 : (variant & 4) ? 2
                                                        : H->order;
    const int threads = waves * WAVE;
    const long long lanes = (long long)(b1 - b0) * HACK;
    const V *as = values_of<V>(H);
    /* XCD ranges of this launch: as hll_launch_t */
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
    if (kernel == 1) {
        /* full blocks through LDS; a ragged last block goes direct */
        int full_end = b1;
        if (b1 == H->nb && (H->M % HACK) != 0)
            full_end = b1 - 1;
        if (full_end > b0) {
            const int pairs = (full_end - b0 + 1) / 2;
            const size_t lds =
                (size_t)waves * 2 * CH16_SLOTS * (sizeof(V) + sizeof(u16));
            const int nwg = (pairs + waves - 1) / waves;
            if (order == 1)
                hipLaunchKernelGGL((k_hll16_col_lds<1, V>),
                                   dim3(NUM_XCD * (((xmax + 1) / 2 + waves - 1) /
                                                   waves)),
                                   dim3(threads), lds, s, b0, full_end, xr,
                                   H->off, H->base16, H->off16, as, x, y);
            else if (order == 2)
                hipLaunchKernelGGL((k_hll16_col_lds<2, V>),
                                   dim3(grouped_grid(nwg)), dim3(threads), lds,
                                   s, b0, full_end, xr, H->off, H->base16,
                                   H->off16, as, x, y);
            else
                hipLaunchKernelGGL((k_hll16_col_lds<0, V>), dim3(nwg),
                                   dim3(threads), lds, s, b0, full_end, xr,
                                   H->off, H->base16, H->off16, as, x, y);
        }
        if (full_end < b1)
            hipLaunchKernelGGL((k_hll16_col_direct<V, 8, 0>), dim3(1),
                               dim3(WAVE), 0, s, H->M, full_end, b1, xr, H->off,
                               H->base16, H->off16, as, x, y);
    } else {
        /* REMAP grid: 8 x (workgroups of the longest XCD range) */
        const unsigned xgrid =
            NUM_XCD * (unsigned)(((long long)xmax * HACK + threads - 1) / threads);
        const unsigned hwgrid = (unsigned)((lanes + threads - 1) / threads);
        if (order == 1)
            hipLaunchKernelGGL((k_hll16_col_direct<V, 8, 1>), dim3(xgrid),
                               dim3(threads), 0, s, H->M, b0, b1, xr, H->off,
                               H->base16, H->off16, as, x, y);
        else if (order == 2)
            hipLaunchKernelGGL((k_hll16_col_direct<V, 8, 2>),
                               dim3(grouped_grid(hwgrid)), dim3(threads), 0, s,
                               H->M, b0, b1, xr, H->off, H->base16, H->off16, as,
                               x, y);
        else
            hipLaunchKernelGGL((k_hll16_col_direct<V, 8, 0>), dim3(hwgrid),
                               dim3(threads), 0, s, H->M, b0, b1, xr, H->off,
                               H->base16, H->off16, as, x, y);
    }
    return hip_errno(hipGetLastError());
}

/* dispatch on the handle's value type; `waves` is 1..16 (kernel 1: at most 8,
 * engine.hip launch_direct) */
int hll16_launch_kernel(const spmv_hll_dev *H, int kernel, int waves,
                        int variant, const double *x, double *y, int b0, int b1,
                        hipStream_t s) {
    if (!H || H->index_bytes != 2 || !H->off16 || !H->base16)
        return -EINVAL;
    if (H->value_bytes == 4)
        return hll16_launch_t<float>(H, kernel, waves, variant, x, y, b0, b1, s);
    return hll16_launch_t<double>(H, kernel, waves, variant, x, y, b0, b1, s);
}
