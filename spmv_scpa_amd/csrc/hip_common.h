/*
 * hip_common.h -- internals shared by the HIP translation units
 * (engine.hip, csr_kernels.hip, hll_kernels.hip, multi_kernels.hip,
 * cg_kernels.hip, bicgstab_kernels.hip, cgls_kernels.hip, minres_kernels.hip,
 * diag_kernels.hip, transpose_kernels.hip, trsv_kernels.hip, ic0_kernels.hip,
 * ilu0_kernels.hip, spgemm_kernels.hip, add_kernels.hip, amg_kernels.hip,
 * csr_build.hip, panels.hip, mgpu.hip, and
 * mat_ref.h on behalf of the first and the last).
 * Not installed.
 */
#ifndef SPMV_HIP_COMMON_H
#define SPMV_HIP_COMMON_H

#include <errno.h>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "solver_work.h"
#include "spmv_engine.h"

#define WAVE 64 /* gfx950 wavefront */
/* MI355X: 8 accelerator dies, workgroups are dealt to them round-robin.  The
 * library is built for gfx950 only (Makefile) and refuses other devices
 * (spmv_set_device / panels_build check the arch name), so this is a
 * build-time constant rather than a queried property -- HIP exposes no XCD
 * count. */
#define NUM_XCD 8
/* grouped workgroup order: runs of this many consecutive workgroups per XCD,
 * the runs dealt to the XCDs round-robin (xcd_grouped below; panels.hip
 * carries its own, run-time group size) */
#define XCD_GROUP 32
#define HACK HACK_SIZE /* rows of a hack block (hll.h) */

/* grid of a launch in grouped order: n workgroups padded to whole rounds of
 * NUM_XCD runs (the kernels mask the surplus workgroups) */
static inline unsigned grouped_grid(unsigned n) {
    return (n + NUM_XCD * XCD_GROUP - 1) / (NUM_XCD * XCD_GROUP) * NUM_XCD *
           XCD_GROUP;
}

/* HIP status -> negative errno (the host API's error convention) */
static inline int hip_errno(hipError_t e) {
    switch (e) {
    case hipSuccess:
        return 0;
    case hipErrorNoDevice:
    case hipErrorInvalidDevice:
    case hipErrorInsufficientDriver:
    case hipErrorNotInitialized:
        return -ENODEV;
    case hipErrorOutOfMemory:
        return -ENOMEM;
    case hipErrorInvalidValue:
    case hipErrorInvalidConfiguration:
        return -EINVAL;
    default:
        return -EIO;
    }
}

#define HIP_TRY(call)                                                         \
    do {                                                                      \
        hipError_t e_ = (call);                                               \
        if (e_ != hipSuccess) {                                               \
            rc = hip_errno(e_);                                               \
            goto fail;                                                        \
        }                                                                     \
    } while (0)

#define HIP_RET(call)                                                         \
    do {                                                                      \
        hipError_t e_ = (call);                                               \
        if (e_ != hipSuccess)                                                 \
            return hip_errno(e_);                                             \
    } while (0)

/* variant bits the launchers ignore (they belong to the timed loops) */
#define SPMV_VARIANT_TIMING_BITS (1 << 29)

/* nnz budget of one workgroup of the CSR stream kernel */
#define STREAM_NNZ 2048
#define STREAM_THREADS 256
/* rows a range may hold: matrices with 2-5 entries per row (web / road /
 * co-purchase graphs) fill the entry budget only with several rows per lane */
#define STREAM_ROWS 1024
/* ranges whose longest row is at most this use the transposed form */
#define STREAM_ROW_T 48
/* hack blocks wider than HLL_WIDE columns go to k_hll_wide in segments of
 * HLL_WSEG columns (hll_kernels.hip) */
#define HLL_WIDE 512
#ifndef HLL_WSEG
#define HLL_WSEG 256      /* narrowest segment */
#endif
#ifndef HLL_WSEG_MAX
#define HLL_WSEG_MAX 512  /* most segments per block: a hub block of 5 x 10^5
                             columns is then cut into ~1000-column segments
                             (the block's last segment adds up one partial
                             sum per segment and row) */
#endif
/* a row beyond STREAM_LONG_ROW entries is cut into segments of
 * STREAM_SEG entries, one workgroup each (one lane team walking a row of
 * 10^5 entries is the whole launch otherwise: dc1-class matrices) */
#define STREAM_LONG_ROW 8192
#ifndef STREAM_SEG
#define STREAM_SEG 2048
#endif

struct spmv_panels; /* panels.hip */

/* contiguous ranges of a launch's work items, one per XCD, holding about
 * equal numbers of ENTRIES: workgroup b (dealt round-robin to the XCDs) runs
 * item first[b % NUM_XCD] + b / NUM_XCD, or nothing when that lies beyond
 * its XCD's range; the launch has NUM_XCD * (longest range) workgroups.
 * Neighbouring items share their window of x, so they meet in one L2 --
 * and no XCD idles when the rows are denser in one part of the matrix. */
struct xcd_ranges {
    int first[NUM_XCD + 1];
};

struct spmv_csr_dev {
    int M, N;
    int64_t NZ;
    int device;
    int *irp;   /* [M+1] */
    int *ja;    /* [NZ]  */
    double *as; /* [NZ]  (value_bytes 8; NULL in an f32 handle) */
    float *as32; /* [NZ] (value_bytes 4: the values rounded to fp32; every
                    product and sum stays fp64; NULL in an f64 handle) */
    int value_bytes; /* 8 or 4: which of the two arrays the handle owns */
    /* stream kernel: workgroup k owns rows [rowblk[2k], rowblk[2k+2]),
     * entries [rowblk[2k+1], rowblk[2k+3]) */
    int *rowblk;
    int n_rowblk;
    unsigned char *rowblk_mode; /* per range: 0 transposed, 1 cooperative,
                                   2 segment of a long row */
    double *seg_partial; /* [n_rowblk] partial sum of a segment's range */
    unsigned long long *seg_count; /* [n_rowblk] (launch epoch << 32 |
                            arrivals), at a long row's first range
                            (epoch_arrive below); both NULL when no row is
                            that long */
    unsigned launch_epoch; /* number of the last launch that counted arrivals */
    int *long_rb;        /* [n_long_rb] indices of the ranges that hold (a
                            segment of) ONE row of more than STREAM_NNZ
                            entries: kernels 0-3 leave such rows to a second
                            launch over exactly these ranges */
    int n_long_rb;
    int max_row_len;
    int uniform_len; /* > 0: EVERY row holds exactly this many entries (banded
                        and fixed-degree matrices: IRP[r] = r * uniform_len),
                        so the sub-wave kernel need not wait for IRP before it
                        can fetch JA / AS; 0: row lengths vary */
    int order; /* sub-wave kernel, workgroup order: 0 hardware, 1 XCD-contiguous
                  equal ranges, 2 grouped runs of 32 workgroups per XCD
                  (spmv_csr_autotune measures all three) */
    int stream_grouped; /* stream kernel: ranges in grouped runs instead of
                           hardware order (spmv_csr_autotune measures both) */
    spmv_panels *panels; /* optional column-panel copy (kernel 5) */
    double tune_ms[8];   /* last spmv_csr_autotune: best median per kernel id
                            (0: not timed) */
    char *tune_log;      /* ... and what it did, one line per phase (malloc) */
};

struct spmv_hll_dev {
    int M, N;
    int64_t NZ;
    int device;
    int nb;        /* hack blocks */
    int col_major; /* layout inside a block */
    int64_t slots; /* S */
    int max_width; /* largest max_NZ */
    int *ja;       /* [S] pads already rewritten */
    double *as;    /* [S] (value_bytes 8; NULL in an f32 handle) */
    float *as32;   /* [S] (value_bytes 4; NULL in an f64 handle) */
    int value_bytes; /* 8 or 4 */
    int64_t *off;  /* [nb+1] slot offset of each block */
    int order; /* kernels 1 / 2, which blocks a workgroup runs: 0 = hardware
                  order (eight XCDs advancing through ONE region of the
                  slabs: 3-8 % faster on banded matrices than eight contiguous
                  regions), 1 = the XCD ranges below, 2 = grouped (runs of 32
                  workgroups per XCD, runs round-robin: region locality AND
                  neighbours in one L2 -- banded 10M x 32: 85 % of 8 TB/s);
                  spmv_hll_autotune measures all three */
    xcd_ranges xcd_blk; /* hack-block ranges per XCD holding ~1/8 of the SLOTS
                           each (even boundaries: a wavefront owns a pair) */
    unsigned *padmask; /* [(S+31)/32] bit t set: slot t was a pad (JA == -1)
                          before the rewrite; read only when the blocked copy
                          is built */
    spmv_panels *panels; /* optional column-panel copy (kernel 4) */
    /* WIDE hack blocks (a block is as wide as its longest row: one hub row
     * of 10^5 entries makes 32 lanes walk 10^5 columns, 10-60 ms; even 4096
     * columns are a 0.2-0.5 ms walk of dependent steps).  Blocks
     * wider than HLL_WIDE columns are skipped by kernels 0-3 and summed by a
     * second launch, one workgroup per segment of HLL_WSEG columns
     * (k_hll_wide; deterministic last-arriver reduction per block) */
    int4 *wide_seg;    /* [n_wide_seg] (block, segment width, segment, segments) */
    int n_wide_seg;
    double *wide_part; /* [n_wide_seg * 32] partial row sums */
    unsigned long long *wide_cnt; /* [n_wide_seg] (launch epoch << 32 |
                          arrivals), at a block's first segment */
    unsigned launch_epoch;
    double tune_ms[8];   /* last spmv_hll_autotune: best median per kernel id */
    char *tune_log;
    /* index type (spmv_hll_to_index16): 4 = `ja` above; 2 = a "compact"
     * col-major handle that owns NO ja and NO padmask but one base column per
     * hack block and a 16-bit offset per slot, column of slot t of block b =
     * base16[b] + off16[t] (hll_kernels.hip: cols16) */
    int index_bytes;
    int *base16;            /* [nb] smallest valid column of the block */
    unsigned short *off16;  /* [S] in the slot order of the source's ja */
};

/* The next launch number of a handle, never 0 (a zeroed counter belongs to
 * no launch).  The handle is `const` to the launch path but this one field
 * moves; launches of ONE handle are stream-ordered by contract, the atomic
 * only keeps two host threads that break it from tearing the number. */
static inline unsigned next_launch_epoch(const unsigned *field) {
    unsigned *f = const_cast<unsigned *>(field);
    unsigned e = __atomic_add_fetch(f, 1u, __ATOMIC_RELAXED);
    if (e == 0)
        e = __atomic_add_fetch(f, 1u, __ATOMIC_RELAXED);
    return e;
}

/* the handle's value array (CSR or HLL) as the type V the kernels are
 * instantiated for: `as` of an f64 handle, `as32` of an f32 handle */
template <typename V, typename H> static inline const V *values_of(const H *h) {
    if constexpr (std::is_same<V, float>::value)
        return h->as32;
    else
        return h->as;
}

#if defined(__HIPCC__)
/* JA / AS are read once: non-temporal, so they do not evict x from the L2 /
 * Infinity Cache */
template <typename T> __device__ __forceinline__ T ld_stream(const T *p) {
    return __builtin_nontemporal_load(p);
}

/*
 * Segmented reduction inside a wavefront: sum over groups of G consecutive
 * lanes, result in the first lane of each group (what a __shfl_down(width G)
 * tree gives).  Offsets 8,4,2,1 stay inside a 16-lane DPP row and run on the
 * VALU as row_shl moves (no LDS-crossbar ds_bpermute); only the 16- and
 * 32-lane steps use __shfl_down.  The single- and the multi-vector sub-wave
 * kernels share this tree: the order contract of multi_kernels.hip.
 */
template <int CTRL> __device__ __forceinline__ double dpp_f64(double v) {
    const long long b = __builtin_bit_cast(long long, v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, 0xf, 0xf, true);
    const int hi =
        __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xf, 0xf, true);
    return __builtin_bit_cast(
        double, ((long long)hi << 32) | (unsigned long long)(unsigned)lo);
}

template <int G> __device__ __forceinline__ double group_sum(double v) {
    if (G >= 64)
        v += __shfl_down(v, 32, 64);
    if (G >= 32)
        v += __shfl_down(v, 16, G >= 64 ? 64 : 32);
    if (G >= 16)
        v += dpp_f64<0x108>(v); /* row_shl:8 */
    if (G >= 8)
        v += dpp_f64<0x104>(v); /* row_shl:4 */
    if (G >= 4)
        v += dpp_f64<0x102>(v); /* row_shl:2 */
    if (G >= 2)
        v += dpp_f64<0x101>(v); /* row_shl:1 */
    return v;
}

/* Workgroup orders (workgroups are dealt to the XCDs round-robin).
 * XCD-contiguous: a contiguous range of the grid per XCD (bijective for any
 * nblk): row tiles that share an x window then meet in the same L2 */
__device__ __forceinline__ int xcd_remap(int bid, int nblk) {
    const int nx = NUM_XCD;
    int q = nblk / nx, r = nblk % nx;
    int x = bid % nx, k = bid / nx;
    return x * q + (x < r ? x : r) + k;
}

/* Grouped: workgroup bid, the kk-th of XCD xx, runs item
 * ((kk / XCD_GROUP) * NUM_XCD + xx) * XCD_GROUP + kk % XCD_GROUP of a grid of
 * grouped_grid() workgroups.  The kernels differ in the arithmetic they need,
 * and their code is to stay what it is: B is the type bid is split in (name it
 * where blockIdx.x is passed: deduction chooses unsigned), K the type kk and
 * xx are held in, I the type the item is formed in (the run number is widened
 * BEFORE the products) */
template <typename B, typename K = B, typename I = K>
__device__ __forceinline__ I xcd_grouped(B bid) {
    const K xx = bid % NUM_XCD, kk = bid / NUM_XCD;
    return ((I)(kk / XCD_GROUP) * NUM_XCD + xx) * XCD_GROUP + kk % XCD_GROUP;
}

/*
 * Arrival at a last-arriver counter.  The counter holds (launch epoch << 32 |
 * arrivals of that launch).  Fast path: ONE fetch-and-add that finds the
 * launch's own epoch -- what every arrival of an ordinary launch takes (the
 * last arriver of the launch before left (epoch + 1, 0), and a handle's
 * launches are numbered consecutively).  An arrival that finds ANOTHER epoch
 * -- a launch that never completed left its count behind (a fault, a process
 * killed between the main kernel and its side launch: that used to make every
 * later launch of the handle reduce too early, a wrong y[row] with no error,
 * ADVICE r04), or the launch is a REPLAY of a captured hipGraph, whose kernel
 * arguments are frozen -- resets the word to (epoch, 1) with a compare-and-
 * swap, or, when another arrival has done so meanwhile, adds itself to it:
 * every arrival is counted exactly once on the launch's own word (the add it
 * spent on the foreign word counted nothing).  A compare-and-swap loop for
 * EVERY arrival was measured first: 128 segments of a hub row meeting on one
 * word went from 7 to 90 us (hub 1M: 0.030 -> 0.116 ms).  Returns this
 * arrival's number, 1 .. n; the caller that gets n is the last and calls
 * epoch_rearm().  Agent scope: the arrivals come from different XCDs.
 */
__device__ __forceinline__ unsigned epoch_arrive(unsigned long long *cnt,
                                                 unsigned epoch) {
    unsigned long long old = __hip_atomic_fetch_add(
        cnt, 1ull, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if ((unsigned)(old >> 32) == epoch)
        return (unsigned)old + 1u;
    old = __hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (;;) {
        if ((unsigned)(old >> 32) == epoch) /* reset by another arrival */
            return (unsigned)__hip_atomic_fetch_add(cnt, 1ull, __ATOMIC_ACQ_REL,
                                                    __HIP_MEMORY_SCOPE_AGENT) +
                   1u;
        const unsigned long long first = ((unsigned long long)epoch << 32) | 1ull;
        if (__hip_atomic_compare_exchange_strong(cnt, &old, first,
                                                 __ATOMIC_ACQ_REL,
                                                 __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
            return 1u;
    }
}

/* the last arriver leaves (epoch + 1, 0 arrivals): the word the handle's next
 * launch expects (see epoch_arrive) */
__device__ __forceinline__ void epoch_rearm(unsigned long long *cnt,
                                            unsigned epoch) {
    __hip_atomic_store(cnt, (unsigned long long)(epoch + 1u) << 32,
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

/* part[first * stride], part[(first + step) * stride], ... (indices below n)
 * added up in THAT order, U loads in flight at a time.  The partial sums were
 * written by other workgroups, on other XCDs: agent-scope atomic loads, each a
 * round trip to the L2 / fabric -- one at a time, the 64 loads per lane of a
 * 512-segment hack block were most of k_hll_wide's launch. */
template <int U>
__device__ __forceinline__ double ordered_partial_sum(const double *part, int n,
                                                      int first, int step,
                                                      size_t stride) {
    double s = 0.0;
    for (int j = first; j < n; j += step * U) {
        double v[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
            v[u] = j + u * step < n
                       ? __hip_atomic_load(part + (size_t)(j + u * step) * stride,
                                           __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT)
                       : 0.0;
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (j + u * step < n)
                s += v[u];
    }
    return s;
}

/* Sum part[0 .. n) in a FIXED order with one wavefront (all 64 lanes call):
 * lane l adds part[l], part[l + 64], ... in index order, then a shuffle tree.
 * Total in lane 0.  (One lane adding 10^2..10^3 partials one dependent load
 * at a time was a third of the hub matrices' launch.) */
__device__ __forceinline__ double wave_ordered_sum(const double *part, int n,
                                                   int lane) {
    double s = ordered_partial_sum<4>(part, n, lane, WAVE, 1);
#pragma unroll
    for (int d = WAVE / 2; d > 0; d >>= 1)
        s += __shfl_down(s, d, WAVE);
    return s;
}

/* lanes of this wavefront below the caller whose bit is set in mask */
__device__ __forceinline__ unsigned lanes_below(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi(
        (unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

/* the wavefront's sum / maximum of v in lane 0 (all 64 lanes call) */
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int d = WAVE / 2; d > 0; d >>= 1)
        v += __shfl_down(v, d, WAVE);
    return v;
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
#pragma unroll
    for (int d = WAVE / 2; d > 0; d >>= 1) {
        const unsigned long long o = __shfl_down(v, d, WAVE);
        v = o > v ? o : v;
    }
    return v;
}

/* Columns of hack block b (`rows` = its row count).  The slot count is 64-bit:
 * a hub block of 2^27 columns holds 2^32 slots, and `(unsigned)(off[b + 1] -
 * off[b])` -- a 32-bit division is cheaper -- silently halved such a block */
__device__ __forceinline__ int hack_block_width(const int64_t *__restrict__ off,
                                                int b, int rows) {
    const uint64_t n = (uint64_t)(off[b + 1] - off[b]);
    return rows == HACK_SIZE ? (int)(n >> 5) : (int)(n / (unsigned)rows);
}

/*
 * A stored matrix value as the fp64 factor of its product.  The fp32 form is
 * ONE v_cvt_f64_f32 that stays where it is written, at the product.  Written
 * as `(double)v` the compiler folds the conversion into the predicated load
 * that produced v (the phi of "loaded value" and "0 for a lane without an
 * entry") and then has to wait for that load before it may issue the next
 * one: the P independent passes of the sub-wave kernel ran one memory latency
 * after the other (banded 10M x 32: 0.839 ms against 0.784 for fp64 values
 * that are half as many bytes again).  Denormal inputs are kept (the kernels
 * run with fp32 denormals on).
 */
__device__ __forceinline__ double widen(double v) { return v; }
__device__ __forceinline__ double widen(float v) {
    double d;
    asm("v_cvt_f64_f32_e32 %0, %1" : "=v"(d) : "v"(v));
    return d;
}

/* Thread `tid` of NT sums as[k] * x[ja[k]] over k = beg + tid, + NT, ... < end
 * in THAT order (one accumulator: the bits do not depend on U), with the loads
 * of U entries in flight at a time.  The plain loop is two dependent memory
 * round trips per entry -- 4 us per 8 entries on a busy chip -- and a long
 * row's segment is 4-32 entries per thread: the side launches of the long
 * rows were latency, not bandwidth.  Entries stream past (non-temporal).
 * V = double or float, the handle's stored value type: a float is widened in
 * the lane and the product is fp64 either way. */
template <int NT, int U, typename V>
__device__ __forceinline__ double strided_dot(const int *__restrict__ ja,
                                              const V *__restrict__ as,
                                              const double *__restrict__ x,
                                              int beg, int end, int tid) {
    double acc = 0.0;
    /* indices relative to `beg`: `end` may sit next to INT32_MAX (the entry
     * count's limit), beg + k + U * NT must not be formed in 32 bits */
    ja += beg;
    as += beg;
    end -= beg;
    int k = tid;
    for (; k + (U - 1) * NT < end; k += U * NT) {
        int c[U];
        V v[U];
        double xv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            c[u] = __builtin_nontemporal_load(ja + k + u * NT);
            v[u] = __builtin_nontemporal_load(as + k + u * NT);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            xv[u] = x[c[u]];
#pragma unroll
        for (int u = 0; u < U; ++u)
            acc += widen(v[u]) * xv[u];
    }
    if (k < end) { /* fewer than U left: one predicated batch */
        int c[U];
        V v[U];
        double xv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool on = k + u * NT < end;
            c[u] = on ? __builtin_nontemporal_load(ja + k + u * NT) : -1;
            v[u] = on ? __builtin_nontemporal_load(as + k + u * NT) : V(0);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            xv[u] = c[u] >= 0 ? x[c[u]] : 0.0;
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (c[u] >= 0)
                acc += widen(v[u]) * xv[u];
    }
    return acc;
}
#endif

/* clamp the launch knob: waves per workgroup */
static inline int pick_waves(const spmv_launch_opts *o, int dflt) {
    int w = (o && o->waves_per_block > 0) ? o->waves_per_block : dflt;
    if (w < 1)
        w = 1;
    if (w > 16)
        w = 16;
    return w;
}

/* lanes per row of the CSR sub-wave kernels (single- and multi-vector): the
 * caller's power of two in 2..32, else by the mean row length */
static inline int pick_group(const spmv_csr_dev *A, int group) {
    if (group >= 2 && group <= 32 && (group & (group - 1)) == 0)
        return group;
    double mean = A->M > 0 ? (double)A->NZ / A->M : 1.0;
    int g = 2;
    while (g < 32 && g < mean)
        g <<= 1;
    return g;
}

/* Y = A X for k = 1..8 interleaved vectors (multi_kernels.hip); the caller
 * has checked the arguments, `waves` is 1..16 */
int csr_launch_multi(const spmv_csr_dev *A, int waves, int group, int k,
                     const double *X, int64_t ldx, double *Y, int64_t ldy,
                     hipStream_t s);
int hll_launch_multi(const spmv_hll_dev *H, int waves, int k, const double *X,
                     int64_t ldx, double *Y, int64_t ldy, hipStream_t s);
/* ... and Y = alpha A X + beta Y in place, by the same kernels with an
 * epilogue at the store (spmv_*_launch_axpby) */
int csr_launch_axpby(const spmv_csr_dev *A, int waves, int group, int k,
                     double alpha, double beta, const double *X, int64_t ldx,
                     double *Y, int64_t ldy, hipStream_t s);
int hll_launch_axpby(const spmv_hll_dev *H, int waves, int k, double alpha,
                     double beta, const double *X, int64_t ldx, double *Y,
                     int64_t ldy, hipStream_t s);

/*
 * Conjugate gradients (cg_kernels.hip; spmv_*_cg).  The shape of the dot
 * product -- CG_NWG workgroups of CG_T threads, element i in slot
 * i mod (CG_NWG * CG_T) -- is part of the result contract
 * (spmv_cg_dot_shape): the order of a dot depends on M and on nothing else.
 * CG_NWG, the sizes of the state blocks and of a set of partial sums, and the
 * work buffer of every solver are in solver_work.h (free of HIP).
 */
#define CG_T 256
/* spmv_cg_info.status, and the one value only the device sees */
#define CG_CONVERGED 0
#define CG_MAXIT 1
#define CG_BREAKDOWN 2
#define CG_RUNNING 3
/* the matrix as the solver sees it: the handle's launch_multi and
 * launch_axpby with the caller's opts (engine.hip fills it in) */
struct cg_matrix {
    const void *handle;
    const spmv_launch_opts *opts;
    int M;
    int (*multi)(const void *handle, const spmv_launch_opts *opts, int k,
                 const double *X, int64_t ldx, double *Y, int64_t ldy,
                 hipStream_t s);
    int (*axpby)(const void *handle, const spmv_launch_opts *opts, int k,
                 double alpha, double beta, const double *X, int64_t ldx,
                 double *Y, int64_t ldy, hipStream_t s);
};
/* the preconditioner of spmv_*_pcg_trsv: Z = z(R) is trsv_solve_dev(first,
 * R -> Z, no scale), then, with a second plan, trsv_solve_dev(second, Z -> Z in
 * place, scale), all k columns, `waves` lanes as the caller's opts say */
struct spmv_trsv_plan;
struct cg_plans {
    const spmv_trsv_plan *first, *second; /* second may be NULL */
    const double *scale;                  /* M doubles or NULL */
    int waves;
    /* the other preconditioner with a stored Z (spmv_*_pcg_amg): apply !=
     * NULL makes Z = apply(ctx, waves, k, R) where the plans' solves are, R
     * and Z with ld = k; first, second and scale are then unused */
    int (*apply)(const void *ctx, int waves, int k, const double *R, double *Z,
                 hipStream_t s);
    const void *ctx;
};
/* minv == NULL: plain (spmv_*_cg); else preconditioned with z = minv .* r,
 * minv[M] (spmv_*_pcg, pre == 1): the same loop, one more set of partial sums
 * in the work buffer.  plans != NULL (minv NULL, pre == 2; spmv_*_pcg_trsv):
 * the preconditioned loop with a STORED Z = z(R), one more vector behind Q */
int64_t cg_work_bytes(int M, int k, int pre);
int cg_solve(const cg_matrix *A, int k, const double *B, int64_t ldb, double *X,
             int64_t ldx, const double *minv, const cg_plans *plans, double tol,
             int maxit, int check_every, void *d_work, size_t work_bytes,
             spmv_cg_info *info, hipStream_t s);
/* the kernels every solver launches (k_cg_copy, k_cg_dot; k = 1..8): dst = src
 * over M rows of k interleaved columns, and the partial sums of U . V in the
 * dot order -> part[workgroup * k + column] */
void cg_launch_copy(int k, int M, const double *src, int64_t lds, double *dst,
                    int64_t ldd, hipStream_t s);
void cg_launch_dot(int k, int M, const double *U, int64_t ldu, const double *V,
                   int64_t ldv, double *part, hipStream_t s);

/*
 * BiCGStab for nonsymmetric A (bicgstab_kernels.hip; spmv_*_bicgstab): the
 * matrix, the dot, the state block and the records of cg; minv == NULL is no
 * preconditioner, else Z = minv .* P is what the matrix multiplies.  plans !=
 * NULL (minv NULL; spmv_*_bicgstab_trsv): Z = z(P) and z(S) are made by the
 * plans and STORED, one more vector in the work buffer (trsv: 1).
 */
int64_t bicgstab_work_bytes(int M, int k, int trsv);
int bicgstab_solve(const cg_matrix *A, int k, const double *B, int64_t ldb,
                   double *X, int64_t ldx, const double *minv,
                   const cg_plans *plans, double tol, int maxit,
                   int check_every, void *d_work, size_t work_bytes,
                   spmv_cg_info *info, hipStream_t s);

/*
 * CGLS for rectangular least squares (cgls_kernels.hip; spmv_*_cgls): A is
 * M x N (A->M rows), AT its N x M transpose (AT->M = N rows); the dot, the
 * state block and the host loop of cg, with vectors of both lengths.
 */
int64_t cgls_work_bytes(int M, int N, int k);
int cgls_solve(const cg_matrix *A, const cg_matrix *AT, int k, const double *B,
               int64_t ldb, double *X, int64_t ldx, double damp, double tol,
               int maxit, int check_every, void *d_work, size_t work_bytes,
               spmv_cgls_info *info, hipStream_t s);

/*
 * MINRES for symmetric, possibly indefinite A (minres_kernels.hip;
 * spmv_*_minres): the matrix, the dot and the host loop of cg, a state block
 * of its own; minv == NULL is no preconditioner, else a positive diagonal.
 * minres_debug_sqrt: out[i] = the solver's square root of in[i] (test hook).
 */
int64_t minres_work_bytes(int M, int k);
int minres_solve(const cg_matrix *A, int k, const double *B, int64_t ldb,
                 double *X, int64_t ldx, const double *minv, double tol,
                 int maxit, int check_every, void *d_work, size_t work_bytes,
                 spmv_minres_info *info, hipStream_t s);
int minres_debug_sqrt(const double *d_in, double *d_out, int64_t n,
                      hipStream_t s);

/*
 * Restarted GMRES(m) for nonsymmetric A (gmres_kernels.hip; spmv_*_gmres): the
 * matrix, the dot and the host loop of cg, the preconditioner modes of
 * bicgstab (minv, or plans with minv NULL: spmv_*_gmres_trsv), a state of its
 * own (gmres_work, solver_work.h; the dense arithmetic is gmres_small.h).
 */
int64_t gmres_work_bytes(int M, int k, int restart);
int gmres_solve(const cg_matrix *A, int k, const double *B, int64_t ldb,
                double *X, int64_t ldx, const double *minv,
                const cg_plans *plans, int restart, double tol, int maxit,
                int check_every, void *d_work, size_t work_bytes,
                spmv_gmres_info *info, hipStream_t s);

/* out[r] = the sum of row r's stored entries in column r, or 1 / that sum,
 * r < min(M, N) (diag_kernels.hip; spmv_*_diag); the caller has checked the
 * handle */
int csr_diag(const spmv_csr_dev *A, double *out, int invert, hipStream_t s);
int hll_diag(const spmv_hll_dev *H, double *out, int invert, hipStream_t s);

/* A new handle of the live table with irp, ja and values of value_bytes
 * allocated and nothing in them (engine.hip).  Every device operation that
 * makes a handle takes its result from here; on an error *out is untouched */
int csr_alloc_dev(int M, int N, int64_t NZ, int value_bytes,
                  spmv_csr_dev **out);

/* T = A^T (transpose_kernels.hip; spmv_csr_transpose): T comes from
 * csr_alloc_dev(N, M, NZ, value type of A) and gets its irp, ja and values;
 * blocks; -EDOM when a column of A lies outside [0, N).  csr_equal_dev: two
 * handles of one shape, entry count and value type compared element by
 * element (spmv_csr_symmetry) */
int csr_transpose_dev(const spmv_csr_dev *A, spmv_csr_dev *T, hipStream_t s);
int csr_equal_dev(const spmv_csr_dev *X, const spmv_csr_dev *Y, int *pattern,
                  int *values, hipStream_t s);

/*
 * Level-scheduled triangular solve (trsv_kernels.hip; spmv_csr_trsv_analyse,
 * spmv_trsv_solve).  The plan owns device copies of everything the solve
 * reads and a host copy of level_ptr with the launch list made from it
 * (trsv_plan.h): the sequence of launches is a function of the plan alone.
 */
struct trsv_segment;
struct spmv_trsv_plan {
    int M, uplo, unit, levels, value_bytes, device;
    int widest_level;
    int64_t entries;   /* strict entries */
    int64_t zero_diag; /* rows whose diagonal sum is 0.0 */
    int64_t bytes;     /* device memory the plan owns */
    int *level;        /* [M] by row */
    int *order;        /* [M] rows by (level, row) */
    int *level_ptr;    /* [levels + 1] */
    int *rowptr;       /* [M + 1] by position in `order` */
    int *ja;           /* [entries] */
    void *as;          /* [entries] of value_bytes each, A's bits */
    double *diag;      /* [M] by row */
    int *h_level_ptr;  /* host copy (malloc) */
    trsv_segment *segs; /* host, the launches of one solve (malloc) */
    int n_segs;
    /* a sweep plan (spmv_csr_trsv_analyse_sweeps): sweeps > 0, one level, order
     * the identity, no segs; a solve is `sweeps` launches (trsv_sweep_route) */
    int sweeps, kmax;
    double *sweep_buf[2]; /* trsv_sweep_scratch(sweeps) of kmax * M doubles */
};
/* fills *P (zeroed by the caller) from A's chosen triangle; blocks; on an error
 * the caller runs trsv_free_dev.  -E2BIG: more than max_levels levels.
 * sweeps > 0: a sweep plan for at most kmax right-hand sides, max_levels unread */
int trsv_analyse_dev(const spmv_csr_dev *A, int uplo, int unit, int max_levels,
                     int sweeps, int kmax, spmv_trsv_plan *P, hipStream_t s);
void trsv_free_dev(spmv_trsv_plan *P); /* the arrays, not P itself */
/* the arguments were checked by the caller (k <= kmax of a sweep plan too);
 * waves 0 = each kernel's default */
int trsv_solve_dev(const spmv_trsv_plan *P, int waves, int k, const double *B,
                   int64_t ldb, double *X, int64_t ldx, const double *scale,
                   hipStream_t s);

/*
 * Zero-fill incomplete Cholesky (ic0_kernels.hip; spmv_csr_ic0).  The caller
 * has checked the handle (square, f64, with its source).  *out comes from
 * csr_alloc_dev once the pattern passed its check and the schedule is known,
 * and holds irp, ja and the factor; the caller finishes it (engine.hip,
 * publish_csr_handle).  waves 0 = each kernel's default.  Blocks; on an error
 * *out is untouched and everything is freed.
 */
int ic0_factor_dev(const spmv_csr_dev *A, double shift, int max_levels,
                   int waves, spmv_csr_dev **out, spmv_ic0_info *info,
                   hipStream_t s);
/*
 * Zero-fill incomplete LU (ilu0_kernels.hip; spmv_csr_ilu0): the same
 * arrangement.  *out holds A's irp and ja and the factor, L strictly below the
 * diagonal (its unit diagonal implied), U on and above it.
 */
int ilu0_factor_dev(const spmv_csr_dev *A, double shift, int max_levels,
                    int waves, spmv_csr_dev **out, spmv_ilu0_info *info,
                    hipStream_t s);

/*
 * Colouring and permutation (colour_kernels.hip; spmv_csr_colour,
 * spmv_csr_permute, spmv_permute_vectors).  The caller has checked the handle
 * (with its source; square for the colouring) and the arguments.  Both block,
 * free their scratch on every path and leave the caller's arrays / *out
 * untouched on an error.  csr_permute_dev takes *out from csr_alloc_dev once p
 * and q passed their checks; the caller finishes it.
 */
int csr_colour_dev(const spmv_csr_dev *A, uint32_t seed, int max_rounds,
                   int *d_colour, int *d_new_of_old, spmv_colour_info *info,
                   hipStream_t s);
int csr_permute_dev(const spmv_csr_dev *A, const int *p, const int *q,
                    spmv_csr_dev **out, hipStream_t s);
/*
 * C = A B (spgemm_kernels.hip; spmv_csr_spgemm).  The caller has checked the
 * handles (live, with their sources, A->N == B->M).  *out comes from
 * csr_alloc_dev once the entries of C are known and holds irp, ja and the
 * values; the caller finishes it.  Blocks; on an error *out and *info are
 * untouched and everything is freed.
 */
int csr_spgemm_dev(const spmv_csr_dev *A, const spmv_csr_dev *B,
                   spmv_csr_dev **out, spmv_spgemm_info *info, hipStream_t s);
/* host-clock ms of the last successful product of this process: checks and
 * bounds, lists and symbolic pass, scan + allocation + numeric pass, and the
 * part of the last two spent in the fallback's launches */
void csr_spgemm_last_phases(double ms[4]);
/*
 * C = alpha A + beta B (add_kernels.hip; spmv_csr_add).  The caller has
 * checked the handles (live, with their sources, one shape) and the scalars.
 * mode: spmv_add_set_class.  *out comes from csr_alloc_dev once the entries of
 * C are known and holds irp, ja and the values; the caller finishes it and
 * reports the time of that with csr_add_finish_ms.  Blocks; on an error *out
 * and *info are untouched and everything is freed.
 */
int csr_add_dev(double alpha, const spmv_csr_dev *A, double beta,
                const spmv_csr_dev *B, int mode, spmv_csr_dev **out,
                spmv_add_info *info, hipStream_t s);
void csr_add_last_phases(double ms[3]);
void csr_add_finish_ms(double ms);
/* the companions: D (M x M, M entries, f64, allocated) gets the arrays of
 * diag(d) (d NULL: the identity); S (A's shape and entry count, f64,
 * allocated) gets A's irp and ja and the scaled values, -EDOM when d_right is
 * given and a column lies outside [0, N).  Both block */
int csr_from_diag_dev(const double *d_diag, spmv_csr_dev *D, hipStream_t s);
int csr_scale_dev(const spmv_csr_dev *A, const double *d_left,
                  const double *d_right, spmv_csr_dev *S, hipStream_t s);
int permute_vectors_dev(const int *p, int M, int k, int inverse,
                        const double *in, int64_t ldin, double *out,
                        int64_t ldout, hipStream_t s);

/*
 * Smoothed-aggregation AMG (amg_kernels.hip; spmv_csr_aggregate,
 * spmv_csr_amg_setup, spmv_amg_apply).  The caller has checked the handles
 * (square, f64, with their sources).  amg_check_dev: 0, -EDOM (a column
 * outside) or -EINVAL (a row not strictly ascending, or without its diagonal);
 * d_diag (M doubles or NULL) receives the diagonal.  amg_aggregate_dev makes
 * that check itself, blocks, frees its scratch on every path and leaves d_agg
 * and *info untouched on an error.  amg_rho_dev: d_w receives the diagonal and
 * *rho the Gershgorin bound of D^-1 A (one read-back); amg_w_dev then turns
 * d_w into w = omega / d in place.  amg_tentative_dev fills the arrays of an
 * M x n handle with M entries; amg_smooth_p_dev turns the values of A T into
 * those of P in place.  amg_first_dev / amg_update_dev: the two vector
 * kernels of a sweep (r has ld = k), asynchronous.
 */
int amg_check_dev(const spmv_csr_dev *A, double *d_diag, hipStream_t s);
int amg_aggregate_dev(const spmv_csr_dev *A, double theta2, uint32_t seed,
                      int max_rounds, int *d_agg, spmv_aggregate_info *info,
                      hipStream_t s);
int amg_rho_dev(const spmv_csr_dev *A, double *d_w, double *rho, hipStream_t s);
int amg_w_dev(int M, double omega, double *d_w, hipStream_t s);
int amg_tentative_dev(int M, const int *d_agg, spmv_csr_dev *T, hipStream_t s);
int amg_smooth_p_dev(spmv_csr_dev *AT, const int *d_agg, const double *d_w,
                     hipStream_t s);
void amg_first_dev(int M, int k, const double *w, const double *b, int64_t ldb,
                   double *x, int64_t ldx, double *r, hipStream_t s);
/* the fused sweep (k_amg_sweep): W NULL is its residual mode.  Only for a
 * handle without long rows (amg_sweep_fusable); OUT apart from X */
bool amg_sweep_fusable(const spmv_csr_dev *A);
void amg_sweep_dev(const spmv_csr_dev *A, int waves, int k, const double *X,
                   int64_t ldx, const double *B, int64_t ldb, const double *W,
                   double *OUT, int64_t ldo, hipStream_t s);
void amg_update_dev(int M, int k, int refill, const double *w, const double *b,
                    int64_t ldb, double *x, int64_t ldx, double *r,
                    hipStream_t s);

/* kernel launchers (csr_kernels.hip / hll_kernels.hip) */
int csr_launch_kernel(const spmv_csr_dev *A, int kernel, int waves, int group,
                      int variant, const double *x, double *y, int r0, int r1,
                      hipStream_t s);
int hll_launch_kernel(const spmv_hll_dev *H, int kernel, int waves,
                      int variant, const double *x, double *y, int b0, int b1,
                      hipStream_t s);
int hll_fix_pads_dev(spmv_hll_dev *H, hipStream_t s);
/* compact handles (hll_launch_kernel takes them: kernel ids 1 / 2 only), the
 * conversion: dst->base16 / dst->off16 from src->ja / src->padmask,
 * *d_overflow |= 1 when the valid columns of a block span more than 65 536 */
int hll16_convert_dev(const spmv_hll_dev *src, spmv_hll_dev *dst,
                      unsigned *d_overflow, hipStream_t s);

/* column-panel path (panels.hip) */
int panels_from_csr(const spmv_csr_dev *A, int panel_cols, int sched,
                    int tile_rows, spmv_panels **out);
int panels_from_hll(const spmv_hll_dev *H, int panel_cols, int sched,
                    int tile_rows, spmv_panels **out);
int panels_from_csr_opts(const spmv_csr_dev *A, const spmv_panel_opts *o,
                         spmv_panels **out);
int panels_from_hll_opts(const spmv_hll_dev *H, const spmv_panel_opts *o,
                         spmv_panels **out);
void panels_get_opts(const spmv_panels *P, spmv_panel_opts *o);
int panels_is_sweep(const spmv_panels *P);
int panels_tile_rows(const spmv_panels *P);
int panels_is_chain(const spmv_panels *P);
void panels_set_chain(spmv_panels *P, int chain);
void panels_set_waves(spmv_panels *P, int waves);
int panels_debug_stale_arrivals(spmv_panels *P);
void panels_set_order(spmv_panels *P, int order);
int panels_waves(const spmv_panels *P);
void panels_fit_steps(const spmv_panels *P, int64_t *builtin, int64_t *fit);
void panels_set_fit_steps(spmv_panels *P, int64_t builtin, int64_t fit);
int panels_plan_kernel(const spmv_panels *P, int waves, int variant,
                       int *threads, int *groups, int *ordered);
int panels_launch(const spmv_panels *P, int M, int waves, int variant,
                  const double *x, double *y, hipStream_t s);
void panels_free(spmv_panels *p);
int64_t panels_nnz(const spmv_panels *P);
int panels_count(const spmv_panels *P);
int panels_steps(const spmv_panels *P);
int panels_tiles(const spmv_panels *P);
int panels_balanced_tile_rows(int M, int max_rows);
int panels_describe(const spmv_panels *P, char *buf, size_t len);
const char *panels_last_build_phases(void);
void panels_pool_begin(void); /* block reuse across the builds of one */
void panels_pool_end(void);   /* selector run (panels.hip, build_pool)  */

extern int g_csr_waves; /* process defaults behind set_*_waves_per_block */
extern int g_hll_waves;

#endif /* SPMV_HIP_COMMON_H */
