/*
 * diag_kernels.hip -- the diagonal of a device handle (spmv_*_diag,
 * spmv_engine.h): d[r] = the fp64 sum of the stored entries of row r whose
 * column is r, for r < min(M, N), or rn(1.0 / that sum).  CSR and column-major
 * HLL handles with 4-byte columns, both value types, gfx950 (wave64).
 *
 * Run once per matrix, so the kernels are the plain ones: JA is read for every
 * entry, the value only where the column matches.  What they share with the
 * multi-vector kernels (multi_body.h) is the division of the work: a row of
 * more than STREAM_NNZ entries and a hack block of more than HLL_WIDE columns
 * are left to a second launch over the handle's long-row / wide-segment table,
 * one workgroup each, so no lane walks such a row or block alone.
 *
 * ORDER of the sum (it matters only where a row stores its diagonal more than
 * once; a sum starts from 0.0 and pads add their 0.0).  It is a function of
 * the handle -- its arrays and, for CSR, its mean row length -- and of nothing
 * a launch could choose:
 *   CSR row of at most STREAM_NNZ entries: lane l of the row's G lanes
 *     (G = pick_group(A, 0)) adds entries l, l + G, ... in order; group_sum<G>.
 *   CSR longer row: thread t of 256 adds entries t, t + 256, ...; a wavefront
 *     tree; the four wavefront sums in wavefront order.
 *   HLL block of at most HLL_WIDE columns: the row's lane adds in column order.
 *   HLL wider block: column lane c of 8 adds columns c, c + 8, ...; the eight
 *     sums in lane order.
 */
#include "hip_common.h"

#define DIAG_THREADS 256

__device__ __forceinline__ double diag_result(double sum, int invert) {
    return invert ? 1.0 / sum : sum;
}

/* G lanes per row */
template <int G, typename V>
__global__ void __launch_bounds__(DIAG_THREADS)
k_csr_diag(int n, const int *__restrict__ irp, const int *__restrict__ ja,
           const V *__restrict__ as, double *__restrict__ out, int invert) {
    const int sub = threadIdx.x & (G - 1);
    const long long row =
        ((long long)blockIdx.x * DIAG_THREADS + threadIdx.x) / G;
    const bool live = row < n;
    const int beg = live ? irp[row] : 0;
    int len = live ? irp[row + 1] - beg : 0;
    const bool mine = live && len <= STREAM_NNZ; /* else k_csr_diag_long's */
    if (!mine)
        len = 0;
    double acc = 0.0;
    for (int k = sub; k < len; k += G)
        if (ld_stream(ja + beg + k) == row)
            acc += widen(ld_stream(as + beg + k));
    acc = group_sum<G>(acc); /* every lane takes part */
    if (sub == 0 && mine)
        out[row] = diag_result(acc, invert);
}

/* workgroup g takes range long_rb[g] of the stream table and, when that is
 * the FIRST range of its row, the whole row (as k_csr_multi_long) */
template <typename V>
__global__ void __launch_bounds__(DIAG_THREADS)
k_csr_diag_long(int n, const int *__restrict__ long_rb,
                const int2 *__restrict__ rowblk, const int *__restrict__ irp,
                const int *__restrict__ ja, const V *__restrict__ as,
                double *__restrict__ out, int invert) {
    __shared__ double part[DIAG_THREADS / WAVE];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int rb = long_rb[blockIdx.x];
    const int row = rowblk[rb].x;
    const int beg = irp[row];
    if (rowblk[rb].y != beg || row >= n)
        return; /* workgroup-uniform */
    const int len = irp[row + 1] - beg;
    ja += beg;
    as += beg;
    double acc = 0.0;
    /* 64-bit: a row may hold close to INT32_MAX entries */
    for (int64_t k = tid; k < len; k += DIAG_THREADS)
        if (ld_stream(ja + k) == row)
            acc += widen(ld_stream(as + k));
    acc = group_sum<WAVE>(acc);
    if (lane == 0)
        part[tid / WAVE] = acc;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < DIAG_THREADS / WAVE; ++w)
            t += part[w];
        out[row] = diag_result(t, invert);
    }
}

/* column-major HLL: a lane per row */
template <typename V>
__global__ void __launch_bounds__(DIAG_THREADS)
k_hll_diag(int M, int n, int nb, const int64_t *__restrict__ off,
           const int *__restrict__ ja, const V *__restrict__ as,
           double *__restrict__ out, int invert) {
    const long long t = (long long)blockIdx.x * DIAG_THREADS + threadIdx.x;
    if (t / HACK >= nb)
        return;
    const int b = (int)(t / HACK), i = (int)(t % HACK);
    const int rows = min(HACK, M - b * HACK);
    const long long row = (long long)b * HACK + i;
    if (i >= rows || row >= n)
        return;
    const int w = hack_block_width(off, b, rows);
    if (w > HLL_WIDE)
        return; /* k_hll_diag_wide's block */
    const int *cj = ja + off[b] + i;
    const V *ca = as + off[b] + i;
    double acc = 0.0;
    for (int c = 0; c < w; ++c)
        if (ld_stream(cj + (size_t)c * rows) == row)
            acc += widen(ld_stream(ca + (size_t)c * rows));
    out[row] = diag_result(acc, invert);
}

/* workgroup g looks at segment g of the handle's segment table and, when that
 * is the FIRST segment of its block, takes the whole block: thread (row i,
 * column lane cl) walks columns cl, cl + 8, ... (as k_hll_multi_wide) */
template <typename V>
__global__ void __launch_bounds__(DIAG_THREADS)
k_hll_diag_wide(int M, int n, const int4 *__restrict__ seg,
                const int64_t *__restrict__ off, const int *__restrict__ ja,
                const V *__restrict__ as, double *__restrict__ out,
                int invert) {
    __shared__ double red[DIAG_THREADS / HACK][HACK];
    const int tid = threadIdx.x;
    const int4 sg = seg[blockIdx.x];
    if (sg.z != 0)
        return; /* not the block's first segment: workgroup-uniform */
    const int b = sg.x;
    const int rows = min(HACK, M - b * HACK);
    const int w = hack_block_width(off, b, rows);
    const int i = tid & (HACK - 1), cl = tid / HACK;
    const long long row = (long long)b * HACK + i;
    double acc = 0.0;
    if (i < rows) {
        const int64_t base = off[b] + i;
        /* 64-bit column arithmetic: w may sit next to INT32_MAX */
        for (int64_t c = cl; c < w; c += DIAG_THREADS / HACK)
            if (ld_stream(ja + base + c * rows) == row)
                acc += widen(ld_stream(as + base + c * rows));
    }
    red[cl][i] = acc;
    __syncthreads();
    if (cl == 0 && i < rows && row < n) {
        double t = 0.0;
#pragma unroll
        for (int c = 0; c < DIAG_THREADS / HACK; ++c)
            t += red[c][i];
        out[row] = diag_result(t, invert);
    }
}

/* ------------------------------------------------------------------ */
/* launchers: the arguments were checked by the caller (engine.hip)     */
/* ------------------------------------------------------------------ */

template <typename V, int G>
static void csr_diag_g(const spmv_csr_dev *A, int n, double *out, int invert,
                       hipStream_t s) {
    const V *as = values_of<V>(A);
    const long long lanes = (long long)n * G;
    hipLaunchKernelGGL((k_csr_diag<G, V>),
                       dim3((unsigned)((lanes + DIAG_THREADS - 1) / DIAG_THREADS)),
                       dim3(DIAG_THREADS), 0, s, n, A->irp, A->ja, as, out,
                       invert);
    if (A->n_long_rb > 0)
        hipLaunchKernelGGL((k_csr_diag_long<V>), dim3(A->n_long_rb),
                           dim3(DIAG_THREADS), 0, s, n, A->long_rb,
                           (const int2 *)A->rowblk, A->irp, A->ja, as, out,
                           invert);
}

template <typename V>
static int csr_diag_t(const spmv_csr_dev *A, int n, double *out, int invert,
                      hipStream_t s) {
    (void)hipGetLastError(); /* an earlier caller's unread error is not ours */
    switch (pick_group(A, 0)) {
    case 2:
        csr_diag_g<V, 2>(A, n, out, invert, s);
        break;
    case 4:
        csr_diag_g<V, 4>(A, n, out, invert, s);
        break;
    case 8:
        csr_diag_g<V, 8>(A, n, out, invert, s);
        break;
    case 16:
        csr_diag_g<V, 16>(A, n, out, invert, s);
        break;
    default:
        csr_diag_g<V, 32>(A, n, out, invert, s);
        break;
    }
    return hip_errno(hipGetLastError());
}

int csr_diag(const spmv_csr_dev *A, double *out, int invert, hipStream_t s) {
    if (!A || !out)
        return -EINVAL;
    const int n = A->M < A->N ? A->M : A->N;
    if (n == 0)
        return 0;
    if (A->value_bytes == 4)
        return csr_diag_t<float>(A, n, out, invert, s);
    return csr_diag_t<double>(A, n, out, invert, s);
}

template <typename V>
static int hll_diag_t(const spmv_hll_dev *H, int n, double *out, int invert,
                      hipStream_t s) {
    (void)hipGetLastError();
    const V *as = values_of<V>(H);
    const long long lanes = (long long)H->nb * HACK;
    hipLaunchKernelGGL((k_hll_diag<V>),
                       dim3((unsigned)((lanes + DIAG_THREADS - 1) / DIAG_THREADS)),
                       dim3(DIAG_THREADS), 0, s, H->M, n, H->nb, H->off, H->ja,
                       as, out, invert);
    if (H->n_wide_seg > 0)
        hipLaunchKernelGGL((k_hll_diag_wide<V>), dim3(H->n_wide_seg),
                           dim3(DIAG_THREADS), 0, s, H->M, n, H->wide_seg,
                           H->off, H->ja, as, out, invert);
    return hip_errno(hipGetLastError());
}

int hll_diag(const spmv_hll_dev *H, double *out, int invert, hipStream_t s) {
    if (!H || !H->col_major || !out)
        return -EINVAL;
    if (H->index_bytes == 2)
        return -ENOTSUP; /* compact handle: no 4-byte columns to read */
    const int n = H->M < H->N ? H->M : H->N;
    if (n == 0)
        return 0;
    if (H->value_bytes == 4)
        return hll_diag_t<float>(H, n, out, invert, s);
    return hll_diag_t<double>(H, n, out, invert, s);
}
