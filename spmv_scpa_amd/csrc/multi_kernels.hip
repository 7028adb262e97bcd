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
 *
 * AXPBY.  The kernels live in multi_body.h, which this file includes twice:
 * once for Y = A X (k_*_multi) and once for Y = alpha A X + beta Y in place
 * (k_*_axpby: spmv_*_launch_axpby), the same loops with an epilogue at the
 * store.
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

/* The epilogue of the axpby kernels, contraction off: the rest of this file
 * relies on it for its fused multiply-adds, here no product may be fused into
 * the sum.  beta != 0: rn(rn(alpha s) + rn(beta y_old)) -- v_mul_f64,
 * v_mul_f64, v_add_f64; beta == 0: rn(alpha s) -- the first of the two
 * products.  The callers choose by beta != 0, which is uniform: k_hll_axpby
 * with a branch around the K elements of a row, the others with a select. */
__device__ __forceinline__ double axpby_of(double alpha, double s, double beta,
                                           double y_old) {
#pragma clang fp contract(off)
    const double as = alpha * s;
    const double by = beta * y_old;
    return as + by;
}
__device__ __forceinline__ double scaled_of(double alpha, double s) {
#pragma clang fp contract(off)
    return alpha * s;
}

/* k_csr_axpby keeps y_old spread over a row's G lanes (element j in lane
 * j % G, slot j / G): the values as lane 0 of the group needs them, fetched
 * with DPP row_shl moves (lane i reads lane i + j % G < 8, inside its row of
 * 16).  All lanes call. */
template <int G, int K, int YS, int J = 0>
__device__ __forceinline__ void lane_yold(const double (&yo)[YS],
                                          double (&yj)[K]) {
    if constexpr (J < K) {
        if constexpr (J % G == 0)
            yj[J] = yo[J / G];
        else
            yj[J] = dpp_f64<0x100 + J % G>(yo[J / G]);
        lane_yold<G, K, YS, J + 1>(yo, yj);
    }
}

#define MULTI_AXPBY 0
#include "multi_body.h"
#undef MULTI_AXPBY
#define MULTI_AXPBY 1
#include "multi_body.h"
#undef MULTI_AXPBY

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

/* one set of launchers for both families: AX = false launches the k_*_multi
 * kernels (alpha, beta unused), AX = true their k_*_axpby twins */
template <bool AX, typename V, int G, int K>
static void csr_multi_gk(const spmv_csr_dev *A, int threads, const double *X,
                         int64_t ldx, double *Y, int64_t ldy, double alpha,
                         double beta, hipStream_t s) {
    constexpr int P = multi_shape<K>::P;
    const V *as = values_of<V>(A);
    const int rows_per_wave = P * (WAVE / G);
    const long long waves = ((long long)A->M + rows_per_wave - 1) / rows_per_wave;
    const long long wpb = threads / WAVE;
    unsigned grid = (unsigned)((waves + wpb - 1) / wpb);
    if (A->order == 2)
        grid = grouped_grid(grid);
    if constexpr (AX)
        hipLaunchKernelGGL((k_csr_axpby<G, P, K, V>), dim3(grid), dim3(threads),
                           0, s, A->M, A->order, A->irp, A->ja, as, X, ldx, Y,
                           ldy, alpha, beta);
    else
        hipLaunchKernelGGL((k_csr_multi<G, P, K, V>), dim3(grid), dim3(threads),
                           0, s, A->M, A->order, A->irp, A->ja, as, X, ldx, Y,
                           ldy);
    if (A->n_long_rb == 0)
        return;
    if constexpr (AX)
        hipLaunchKernelGGL((k_csr_axpby_long<K, V>), dim3(A->n_long_rb),
                           dim3(MULTI_LONG_THREADS), 0, s, A->long_rb,
                           (const int2 *)A->rowblk, A->irp, A->ja, as, X, ldx, Y,
                           ldy, alpha, beta);
    else
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

template <bool AX, typename V, int G>
static void csr_multi_g(const spmv_csr_dev *A, int threads, int k,
                        const double *X, int64_t ldx, double *Y, int64_t ldy,
                        double alpha, double beta, hipStream_t s) {
#define CALL(KK)                                                              \
    csr_multi_gk<AX, V, G, KK>(A, threads, X, ldx, Y, ldy, alpha, beta, s)
    MULTI_K_SWITCH(k, CALL)
#undef CALL
}

template <bool AX, typename V>
static int csr_multi_t(const spmv_csr_dev *A, int waves, int group, int k,
                       const double *X, int64_t ldx, double *Y, int64_t ldy,
                       double alpha, double beta, hipStream_t s) {
    (void)hipGetLastError(); /* an earlier caller's unread error is not ours */
    const int threads = waves * WAVE;
#define CALL_G(GG)                                                            \
    csr_multi_g<AX, V, GG>(A, threads, k, X, ldx, Y, ldy, alpha, beta, s)
    switch (pick_group(A, group)) {
    case 2:
        CALL_G(2);
        break;
    case 4:
        CALL_G(4);
        break;
    case 8:
        CALL_G(8);
        break;
    case 16:
        CALL_G(16);
        break;
    default:
        CALL_G(32);
        break;
    }
#undef CALL_G
    return hip_errno(hipGetLastError());
}

template <bool AX>
static int csr_multi_any(const spmv_csr_dev *A, int waves, int group, int k,
                         const double *X, int64_t ldx, double *Y, int64_t ldy,
                         double alpha, double beta, hipStream_t s) {
    if (!A || k < 1 || k > MULTI_MAXK || !X || !Y || ldx < k || ldy < k)
        return -EINVAL;
    if (A->M == 0)
        return 0;
    if (A->value_bytes == 4)
        return csr_multi_t<AX, float>(A, waves, group, k, X, ldx, Y, ldy, alpha,
                                      beta, s);
    return csr_multi_t<AX, double>(A, waves, group, k, X, ldx, Y, ldy, alpha,
                                   beta, s);
}

/* the arguments were checked by the caller (engine.hip, launch_multi) */
int csr_launch_multi(const spmv_csr_dev *A, int waves, int group, int k,
                     const double *X, int64_t ldx, double *Y, int64_t ldy,
                     hipStream_t s) {
    return csr_multi_any<false>(A, waves, group, k, X, ldx, Y, ldy, 0.0, 0.0,
                                s);
}

int csr_launch_axpby(const spmv_csr_dev *A, int waves, int group, int k,
                     double alpha, double beta, const double *X, int64_t ldx,
                     double *Y, int64_t ldy, hipStream_t s) {
    return csr_multi_any<true>(A, waves, group, k, X, ldx, Y, ldy, alpha, beta,
                               s);
}

template <bool AX, typename V, int K>
static void hll_multi_k(const spmv_hll_dev *H, int threads, const double *X,
                        int64_t ldx, double *Y, int64_t ldy, double alpha,
                        double beta, hipStream_t s) {
    constexpr int U = multi_shape<K>::U;
    const V *as = values_of<V>(H);
    const long long lanes = (long long)H->nb * HACK;
    unsigned grid = (unsigned)((lanes + threads - 1) / threads);
    /* the handle's order; XCD ranges (1) run in hardware order here */
    const int order = H->order == 2 ? 2 : 0;
    if (order == 2)
        grid = grouped_grid(grid);
    if constexpr (AX)
        hipLaunchKernelGGL((k_hll_axpby<K, U, V>), dim3(grid), dim3(threads), 0,
                           s, H->M, H->nb, order, H->off, H->ja, as, X, ldx, Y,
                           ldy, alpha, beta);
    else
        hipLaunchKernelGGL((k_hll_multi<K, U, V>), dim3(grid), dim3(threads), 0,
                           s, H->M, H->nb, order, H->off, H->ja, as, X, ldx, Y,
                           ldy);
    if (H->n_wide_seg == 0)
        return;
    if constexpr (AX)
        hipLaunchKernelGGL((k_hll_axpby_wide<K, U, V>), dim3(H->n_wide_seg),
                           dim3(256), 0, s, H->M, H->wide_seg, H->off, H->ja,
                           as, X, ldx, Y, ldy, alpha, beta);
    else
        hipLaunchKernelGGL((k_hll_multi_wide<K, U, V>), dim3(H->n_wide_seg),
                           dim3(256), 0, s, H->M, H->wide_seg, H->off, H->ja,
                           as, X, ldx, Y, ldy);
}

template <bool AX, typename V>
static int hll_multi_t(const spmv_hll_dev *H, int waves, int k, const double *X,
                       int64_t ldx, double *Y, int64_t ldy, double alpha,
                       double beta, hipStream_t s) {
    (void)hipGetLastError();
    const int threads = waves * WAVE;
#define CALL(KK)                                                              \
    hll_multi_k<AX, V, KK>(H, threads, X, ldx, Y, ldy, alpha, beta, s)
    MULTI_K_SWITCH(k, CALL)
#undef CALL
    return hip_errno(hipGetLastError());
}

template <bool AX>
static int hll_multi_any(const spmv_hll_dev *H, int waves, int k,
                         const double *X, int64_t ldx, double *Y, int64_t ldy,
                         double alpha, double beta, hipStream_t s) {
    if (!H || !H->col_major || k < 1 || k > MULTI_MAXK || !X || !Y || ldx < k ||
        ldy < k)
        return -EINVAL;
    if (H->index_bytes == 2)
        return -ENOTSUP; /* compact handle: no 4-byte columns to read */
    if (H->M == 0)
        return 0;
    if (H->value_bytes == 4)
        return hll_multi_t<AX, float>(H, waves, k, X, ldx, Y, ldy, alpha, beta,
                                      s);
    return hll_multi_t<AX, double>(H, waves, k, X, ldx, Y, ldy, alpha, beta, s);
}

int hll_launch_multi(const spmv_hll_dev *H, int waves, int k, const double *X,
                     int64_t ldx, double *Y, int64_t ldy, hipStream_t s) {
    return hll_multi_any<false>(H, waves, k, X, ldx, Y, ldy, 0.0, 0.0, s);
}

int hll_launch_axpby(const spmv_hll_dev *H, int waves, int k, double alpha,
                     double beta, const double *X, int64_t ldx, double *Y,
                     int64_t ldy, hipStream_t s) {
    return hll_multi_any<true>(H, waves, k, X, ldx, Y, ldy, alpha, beta, s);
}
