/*
 * multi_kernels.hip -- Y = A X for 1..8 right-hand sides stored interleaved
 * (X[c * ldx + j], Y[r * ldy + j]; spmv_*_launch_multi, spmv_engine.h), fp64
 * products and sums, gfx950 (wave64).  One kernel family per format, templates
 * over the handle's stored value type V (double / float), the number of
 * vectors K and, for CSR, the lanes per row G.
 *
 * One pass over JA / AS serves all K products, and the K values of a column
 * are one request to one 128-byte line instead of K requests to K lines.
 *
 * ORDER CONTRACT.  Column j of Y carries the bits of a single-vector launch
 * the library already has, on the same handle with x = X[:, j]:
 *   CSR  k_csr_subwave_row (kernel 2) with the same G: lane `sub` of a row's G
 *        lanes starts from the plain product of entry `sub`, adds the entries
 *        sub + G, sub + 2G, ... in order with fused multiply-adds, then
 *        group_sum<G> -- the SAME function in both kernels (hip_common.h), so
 *        the two trees cannot drift apart.  The passes P are independent rows,
 *        so P is free: it falls as K grows (multi_shape) to keep P * K
 *        accumulators in registers.
 *   HLL  k_hll_col_lds / k_hll_col_direct (kernels 1 / 2, column-major): one
 *        lane per row, acc = 0.0, then acc = fma(a, x, acc) over the block's
 *        columns in order, pads included.
 * Rows of more than STREAM_NNZ entries and hack blocks of more than HLL_WIDE
 * columns (what the single-vector kernels leave to their segment kernels) get
 * one workgroup each here: a fixed-order reduction through LDS, no state
 * between workgroups -- reproducible, within the parity bound, but not the
 * bits of the segment kernels.
 */
#include <algorithm>
#include "hip_common.h"

#define MULTI_MAXK 8
#define MULTI_LONG_THREADS 256

/* X[c * ldx + 0 .. K): plain cached loads, the row offset formed in 64 bits.
 * Written as K 8-byte loads of consecutive doubles; the compiler merges pairs
 * into 16-byte loads whatever ldx and the alignment of X are (global loads of
 * gfx950 need no more than 4-byte alignment), so there is no separate path for
 * an odd ldx or an unaligned base */
template <int K>
__device__ __forceinline__ void load_xrow(const double *__restrict__ X,
                                          int64_t ldx, int c, double (&xv)[K]) {
    const double *p = X + (int64_t)c * ldx;
#pragma unroll
    for (int j = 0; j < K; ++j)
        xv[j] = p[j];
}

/* ------------------------------------------------------------------ */
/* CSR: G lanes per row, P rows per lane group, K accumulators per row  */
/* ------------------------------------------------------------------ */
template <int G, int P, int K, typename V>
__global__ void k_csr_multi(int M, int order, const int *__restrict__ irp,
                            const int *__restrict__ ja,
                            const V *__restrict__ as,
                            const double *__restrict__ X, int64_t ldx,
                            double *__restrict__ Y, int64_t ldy) {
    constexpr int RPP = WAVE / G; /* rows per pass */
    const int lane = threadIdx.x & (WAVE - 1);
    const int sub = lane & (G - 1);
    /* order 0: hardware, 1: XCD-contiguous equal ranges, 2: grouped (grid
     * padded to a multiple of NUM_XCD x XCD_GROUP; rows beyond M are masked) */
    const long long bid = order == 1 ? xcd_remap(blockIdx.x, gridDim.x)
                          : order == 2 ? xcd_grouped<long long>(blockIdx.x)
                                       : (long long)blockIdx.x;
    const long long wave_global = (bid * blockDim.x + threadIdx.x) / WAVE;
    const long long rbase = wave_global * (P * RPP) + lane / G;

    int beg[P], end[P];
    bool mine[P]; /* this kernel writes the row (inside M, not a long row) */
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const long long row = rbase + p * RPP;
        const bool live = row < M;
        beg[p] = live ? irp[row] : 0;
        end[p] = live ? irp[row + 1] : 0;
        mine[p] = live;
        if (end[p] - beg[p] > STREAM_NNZ) { /* k_csr_multi_long's row */
            end[p] = beg[p];
            mine[p] = false;
        }
    }
    int c[P];
    V a[P];
    double acc[P][K];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        /* offsets relative to the row's first entry: beg + sub (+ G below)
         * must not be formed in 32 bits next to INT32_MAX */
        const bool has = sub < end[p] - beg[p];
        c[p] = has ? ld_stream(ja + beg[p] + sub) : -1;
        a[p] = has ? ld_stream(as + beg[p] + sub) : V(0);
    }
    /* the gathers of all P passes are issued before the first product waits */
#pragma unroll
    for (int p = 0; p < P; ++p) {
#pragma unroll
        for (int j = 0; j < K; ++j)
            acc[p][j] = 0.0;
        if (c[p] >= 0)
            load_xrow<K>(X, ldx, c[p], acc[p]);
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const double av = widen(a[p]);
#pragma unroll
        for (int j = 0; j < K; ++j) /* the lane's first product: a multiply */
            acc[p][j] = c[p] >= 0 ? av * acc[p][j] : 0.0;
    }
#pragma unroll
    for (int p = 0; p < P; ++p)
        for (int k = sub + G, n = end[p] - beg[p]; k < n; k += G) {
            double xv[K];
            const double av = widen(ld_stream(as + beg[p] + k));
            load_xrow<K>(X, ldx, ld_stream(ja + beg[p] + k), xv);
#pragma unroll
            for (int j = 0; j < K; ++j)
                acc[p][j] += av * xv[j];
        }
#pragma unroll
    for (int p = 0; p < P; ++p) {
#pragma unroll
        for (int j = 0; j < K; ++j)
            acc[p][j] = group_sum<G>(acc[p][j]);
        const long long row = rbase + p * RPP;
        if (sub == 0 && mine[p]) {
            double *yr = Y + row * ldy;
#pragma unroll
            for (int j = 0; j < K; ++j)
                __builtin_nontemporal_store(acc[p][j], yr + j);
        }
    }
}

/*
 * The rows of more than STREAM_NNZ entries: workgroup g takes range
 * long_rb[g] of the stream table and, when that is the FIRST range of its
 * row (a row beyond STREAM_LONG_ROW entries owns several), sums the whole
 * row: thread t adds entries t, t + 256, ... in order (four in flight), a
 * wavefront tree, then the four wavefronts' partial sums in wavefront order.
 */
template <int K, typename V>
__global__ void __launch_bounds__(MULTI_LONG_THREADS)
    k_csr_multi_long(const int *__restrict__ long_rb,
                     const int2 *__restrict__ rowblk,
                     const int *__restrict__ irp, const int *__restrict__ ja,
                     const V *__restrict__ as, const double *__restrict__ X,
                     int64_t ldx, double *__restrict__ Y, int64_t ldy) {
    constexpr int NT = MULTI_LONG_THREADS, U = 4;
    __shared__ double part[NT / WAVE][K];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int rb = long_rb[blockIdx.x];
    const int row = rowblk[rb].x;
    const int beg = irp[row];
    if (rowblk[rb].y != beg)
        return; /* a later segment of the same row: workgroup-uniform */
    const int n = irp[row + 1] - beg;
    ja += beg;
    as += beg;
    double acc[K];
#pragma unroll
    for (int j = 0; j < K; ++j)
        acc[j] = 0.0;
    /* 64-bit: a row may hold close to INT32_MAX entries, k + u * NT more */
    for (int64_t k = tid; k < n; k += U * NT) {
        int c[U];
        V v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool on = k + u * NT < n;
            c[u] = on ? ld_stream(ja + k + u * NT) : -1;
            v[u] = on ? ld_stream(as + k + u * NT) : V(0);
        }
        double xv[U][K];
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (c[u] >= 0)
                load_xrow<K>(X, ldx, c[u], xv[u]);
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (c[u] >= 0) {
                const double av = widen(v[u]);
#pragma unroll
                for (int j = 0; j < K; ++j)
                    acc[j] += av * xv[u][j];
            }
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        acc[j] = group_sum<WAVE>(acc[j]);
        if (lane == 0)
            part[tid / WAVE][j] = acc[j];
    }
    __syncthreads();
    if (tid < K) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < NT / WAVE; ++w)
            t += part[w][tid];
        Y[(int64_t)row * ldy + tid] = t;
    }
}

/* ------------------------------------------------------------------ */
/* HLL, column-major: lane per row, U columns in flight, K accumulators */
/* ------------------------------------------------------------------ */
template <int K, int U, typename V>
__global__ void k_hll_multi(int M, int nb, int order,
                            const int64_t *__restrict__ off,
                            const int *__restrict__ ja,
                            const V *__restrict__ as,
                            const double *__restrict__ X, int64_t ldx,
                            double *__restrict__ Y, int64_t ldy) {
    /* order 2: groups of XCD_GROUP workgroups per XCD; else hardware */
    const long long wg = order == 2 ? xcd_grouped<long long>(blockIdx.x)
                                    : (long long)blockIdx.x;
    const long long t = wg * blockDim.x + threadIdx.x;
    if (t / HACK >= nb)
        return;
    const int b = (int)(t / HACK), i = (int)(t % HACK);
    const int rows = min(HACK, M - b * HACK);
    if (i >= rows)
        return;
    const int64_t o = off[b];
    const int w = hack_block_width(off, b, rows);
    if (w > HLL_WIDE)
        return; /* k_hll_multi_wide's block */
    const int *cj = ja + o + i;
    const V *ca = as + o + i;
    double acc[K];
#pragma unroll
    for (int j = 0; j < K; ++j)
        acc[j] = 0.0;
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
        double xv[U][K];
        V av[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            load_xrow<K>(X, ldx, cJ[u], xv[u]);
            av[u] = cA[u];
        }
        if (c + 1 < nfull) { /* the next columns' stream behind the gathers */
            const int *nj = cj + (size_t)(c + 1) * U * rows;
            const V *na = ca + (size_t)(c + 1) * U * rows;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                cJ[u] = ld_stream(nj + u * rows);
                cA[u] = ld_stream(na + u * rows);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const double a = widen(av[u]);
#pragma unroll
            for (int j = 0; j < K; ++j)
                acc[j] += a * xv[u][j];
        }
    }
    for (int jc = nfull * U; jc < w; ++jc) {
        double xv[K];
        const double a = widen(ld_stream(ca + (size_t)jc * rows));
        load_xrow<K>(X, ldx, ld_stream(cj + (size_t)jc * rows), xv);
#pragma unroll
        for (int j = 0; j < K; ++j)
            acc[j] += a * xv[j];
    }
    double *yr = Y + ((int64_t)b * HACK + i) * ldy;
#pragma unroll
    for (int j = 0; j < K; ++j)
        __builtin_nontemporal_store(acc[j], yr + j);
}

/*
 * The hack blocks of more than HLL_WIDE columns: workgroup g looks at segment
 * g of the handle's segment table and, when that is the FIRST segment of its
 * block, sums the whole block: thread (row i, column lane cl) adds columns
 * cl, cl + 8, ... in order, then the eight column lanes of a row are added in
 * lane order out of LDS.
 */
template <int K, int U, typename V>
__global__ void __launch_bounds__(256)
    k_hll_multi_wide(int M, const int4 *__restrict__ seg,
                     const int64_t *__restrict__ off,
                     const int *__restrict__ ja, const V *__restrict__ as,
                     const double *__restrict__ X, int64_t ldx,
                     double *__restrict__ Y, int64_t ldy) {
    __shared__ double red[8][K][HACK];
    const int tid = threadIdx.x;
    const int4 sg = seg[blockIdx.x];
    if (sg.z != 0)
        return; /* not the block's first segment: workgroup-uniform */
    const int b = sg.x;
    const int rows = min(HACK, M - b * HACK);
    const int64_t o = off[b];
    const int w = hack_block_width(off, b, rows);
    const int i = tid & 31, cl = tid >> 5;
    double acc[K];
#pragma unroll
    for (int j = 0; j < K; ++j)
        acc[j] = 0.0;
    if (i < rows) {
        const int64_t base = o + i;
        /* 64-bit column arithmetic: w may sit next to INT32_MAX */
        for (int64_t jc = cl; jc < w; jc += 8 * U) {
            int c[U];
            V v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t col = jc + 8 * u;
                const bool on = col < w;
                c[u] = on ? ld_stream(ja + base + col * rows) : -1;
                v[u] = on ? ld_stream(as + base + col * rows) : V(0);
            }
            double xv[U][K];
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (c[u] >= 0)
                    load_xrow<K>(X, ldx, c[u], xv[u]);
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (c[u] >= 0) {
                    const double a = widen(v[u]);
#pragma unroll
                    for (int j = 0; j < K; ++j)
                        acc[j] += a * xv[u][j];
                }
        }
    }
#pragma unroll
    for (int j = 0; j < K; ++j)
        red[cl][j][i] = acc[j];
    __syncthreads();
    /* thread (vector j = tid / 32, row i): 32 * K <= 256 threads take part */
    if (cl < K && i < rows) {
        double t = 0.0;
#pragma unroll
        for (int c = 0; c < 8; ++c)
            t += red[c][cl][i];
        Y[((int64_t)b * HACK + i) * ldy + cl] = t;
    }
}

/* ------------------------------------------------------------------ */
/* launchers                                                            */
/* ------------------------------------------------------------------ */

/* passes of the CSR kernel / columns in flight of the HLL kernel per K: both
 * keep the accumulators and the gathered values of a lane in registers (no
 * scratch; the table is in DESIGN.md section 13) */
template <int K> struct multi_shape {
    static constexpr int P = K == 1 ? 8 : K <= 4 ? 4 : 2;
    static constexpr int U = K == 1 ? 8 : K <= 4 ? 4 : 2;
};

template <typename V, int G, int K>
static void csr_multi_gk(const spmv_csr_dev *A, int threads, const double *X,
                         int64_t ldx, double *Y, int64_t ldy, hipStream_t s) {
    constexpr int P = multi_shape<K>::P;
    const V *as = values_of<V>(A);
    const int rows_per_wave = P * (WAVE / G);
    const long long waves = ((long long)A->M + rows_per_wave - 1) / rows_per_wave;
    const long long wpb = threads / WAVE;
    unsigned grid = (unsigned)((waves + wpb - 1) / wpb);
    if (A->order == 2)
        grid = grouped_grid(grid);
    hipLaunchKernelGGL((k_csr_multi<G, P, K, V>), dim3(grid), dim3(threads), 0,
                       s, A->M, A->order, A->irp, A->ja, as, X, ldx, Y, ldy);
    if (A->n_long_rb > 0)
        hipLaunchKernelGGL((k_csr_multi_long<K, V>), dim3(A->n_long_rb),
                           dim3(MULTI_LONG_THREADS), 0, s, A->long_rb,
                           (const int2 *)A->rowblk, A->irp, A->ja, as, X, ldx, Y,
                           ldy);
}

#define MULTI_K_SWITCH(k, CALL)                                               \
    switch (k) {                                                              \
    case 1: CALL(1); break;                                                   \
    case 2: CALL(2); break;                                                   \
    case 3: CALL(3); break;                                                   \
    case 4: CALL(4); break;                                                   \
    case 5: CALL(5); break;                                                   \
    case 6: CALL(6); break;                                                   \
    case 7: CALL(7); break;                                                   \
    default: CALL(8); break;                                                  \
    }

template <typename V, int G>
static void csr_multi_g(const spmv_csr_dev *A, int threads, int k,
                        const double *X, int64_t ldx, double *Y, int64_t ldy,
                        hipStream_t s) {
#define CALL(KK) csr_multi_gk<V, G, KK>(A, threads, X, ldx, Y, ldy, s)
    MULTI_K_SWITCH(k, CALL)
#undef CALL
}

template <typename V>
static int csr_multi_t(const spmv_csr_dev *A, int waves, int group, int k,
                       const double *X, int64_t ldx, double *Y, int64_t ldy,
                       hipStream_t s) {
    (void)hipGetLastError(); /* an earlier caller's unread error is not ours */
    const int threads = waves * WAVE;
    switch (pick_group(A, group)) {
    case 2:
        csr_multi_g<V, 2>(A, threads, k, X, ldx, Y, ldy, s);
        break;
    case 4:
        csr_multi_g<V, 4>(A, threads, k, X, ldx, Y, ldy, s);
        break;
    case 8:
        csr_multi_g<V, 8>(A, threads, k, X, ldx, Y, ldy, s);
        break;
    case 16:
        csr_multi_g<V, 16>(A, threads, k, X, ldx, Y, ldy, s);
        break;
    default:
        csr_multi_g<V, 32>(A, threads, k, X, ldx, Y, ldy, s);
        break;
    }
    return hip_errno(hipGetLastError());
}

/* the arguments were checked by the caller (engine.hip, launch_multi) */
int csr_launch_multi(const spmv_csr_dev *A, int waves, int group, int k,
                     const double *X, int64_t ldx, double *Y, int64_t ldy,
                     hipStream_t s) {
    if (!A || k < 1 || k > MULTI_MAXK || !X || !Y || ldx < k || ldy < k)
        return -EINVAL;
    if (A->M == 0)
        return 0;
    if (A->value_bytes == 4)
        return csr_multi_t<float>(A, waves, group, k, X, ldx, Y, ldy, s);
    return csr_multi_t<double>(A, waves, group, k, X, ldx, Y, ldy, s);
}

template <typename V, int K>
static void hll_multi_k(const spmv_hll_dev *H, int threads, const double *X,
                        int64_t ldx, double *Y, int64_t ldy, hipStream_t s) {
    constexpr int U = multi_shape<K>::U;
    const V *as = values_of<V>(H);
    const long long lanes = (long long)H->nb * HACK;
    unsigned grid = (unsigned)((lanes + threads - 1) / threads);
    /* the handle's order; XCD ranges (1) run in hardware order here */
    const int order = H->order == 2 ? 2 : 0;
    if (order == 2)
        grid = grouped_grid(grid);
    hipLaunchKernelGGL((k_hll_multi<K, U, V>), dim3(grid), dim3(threads), 0, s,
                       H->M, H->nb, order, H->off, H->ja, as, X, ldx, Y,
                       ldy);
    if (H->n_wide_seg > 0)
        hipLaunchKernelGGL((k_hll_multi_wide<K, U, V>), dim3(H->n_wide_seg),
                           dim3(256), 0, s, H->M, H->wide_seg, H->off,
                           H->ja, as, X, ldx, Y, ldy);
}

template <typename V>
static int hll_multi_t(const spmv_hll_dev *H, int waves, int k, const double *X,
                       int64_t ldx, double *Y, int64_t ldy, hipStream_t s) {
    (void)hipGetLastError();
    const int threads = waves * WAVE;
#define CALL(KK) hll_multi_k<V, KK>(H, threads, X, ldx, Y, ldy, s)
    MULTI_K_SWITCH(k, CALL)
#undef CALL
    return hip_errno(hipGetLastError());
}

int hll_launch_multi(const spmv_hll_dev *H, int waves, int k, const double *X,
                     int64_t ldx, double *Y, int64_t ldy, hipStream_t s) {
    if (!H || !H->col_major || k < 1 || k > MULTI_MAXK || !X || !Y || ldx < k ||
        ldy < k)
        return -EINVAL;
    if (H->index_bytes == 2)
        return -ENOTSUP; /* compact handle: no 4-byte columns to read */
    if (H->M == 0)
        return 0;
    if (H->value_bytes == 4)
        return hll_multi_t<float>(H, waves, k, X, ldx, Y, ldy, s);
    return hll_multi_t<double>(H, waves, k, X, ldx, Y, ldy, s);
}
