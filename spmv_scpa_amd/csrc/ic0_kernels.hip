/*
 * ic0_kernels.hip -- zero-fill incomplete Cholesky A ~ L L^T on the lower
 * triangle of a square f64 CSR handle (spmv_csr_ic0; spmv_engine.h), gfx950
 * (wave64).
 *
 *   k_ic0_check   one lane per row, in stored order: the number of entries
 *                 with column <= row, a flag for a column outside [0, M), a
 *                 flag for a lower triangle that is not strictly ascending or
 *                 stores no diagonal
 *   scan, k_ic0_fill   L's pattern and A's values in it: the lower triangle in
 *                 row order, so the diagonal is the LAST entry of every row
 *   trsv_analyse_dev(A, lower)   the levels of the strict lower pattern are
 *                 the dependency order of a row-wise factorisation: row i reads
 *                 the finished rows j of its strict columns and nothing else.
 *                 Only order, level_ptr and the launch list of that plan are
 *                 used; the plan is freed before the call returns
 *   k_ic0_wide    ONE level of more than small_rows rows over a grid
 *   k_ic0_chain   a maximal run of thinner levels in ONE workgroup with a
 *                 workgroup barrier between levels
 *
 * ic0_row below is the result contract of spmv_csr_ic0: one lane per row, a
 * two-pointer merge of row i with row j for every strict entry (i, j), every
 * operation rounded once (contraction off), an IEEE division, a correctly
 * rounded square root.  The factorisation is IN PLACE: L[t] holds a_ij until
 * the lane replaces it with l_ij, and everything the lane reads of its own row
 * it wrote itself before.  Both kernels call the same ic0_row, so the bits do
 * not depend on which kernel ran a level or on the workgroup size.
 *
 * There is NO waiting between workgroups: a row's dependencies were written by
 * an earlier kernel of the stream (wide) or by this workgroup before the last
 * barrier (chain, as k_trsv_chain).  L is read and written through one plain,
 * non-restrict pointer: vector loads only.  Every device loop is bounded by a
 * row length.
 */
#include <stdlib.h>
#include <string.h>

#include "hip_common.h"
#include "transpose_plan.h"
#include "trsv_plan.h"

#define IC_T 256 /* lanes of a check / fill workgroup */
#define IC_BAD_COLUMN 1u
#define IC_BAD_ORDER 2u

__global__ void __launch_bounds__(IC_T)
k_ic0_check(int M, const int *__restrict__ irp, const int *__restrict__ ja,
            int *__restrict__ cnt, unsigned *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * IC_T + threadIdx.x;
    if (i >= M)
        return;
    int n = 0, prev = -1;
    bool bad_col = false, bad_order = false;
    for (int64_t e = irp[i], end = irp[i + 1]; e < end; ++e) {
        const int c = ja[e];
        if ((unsigned)c >= (unsigned)M) {
            bad_col = true;
        } else if (c <= (int)i) {
            if (c <= prev)
                bad_order = true;
            prev = c;
            ++n;
        }
    }
    cnt[i] = n;
    if (bad_col)
        atomicOr(flag, IC_BAD_COLUMN);
    if (bad_order || prev != (int)i) /* ascending: the diagonal is the last */
        atomicOr(flag, IC_BAD_ORDER);
}

/* lptr: cnt scanned.  Only after k_ic0_check found nothing */
__global__ void __launch_bounds__(IC_T)
k_ic0_fill(int M, const int *__restrict__ irp, const int *__restrict__ ja,
           const double *__restrict__ as, const int *__restrict__ lptr,
           int *__restrict__ lja, double *__restrict__ las) {
    const int64_t i = (int64_t)blockIdx.x * IC_T + threadIdx.x;
    if (i >= M)
        return;
    int64_t at = lptr[i];
    const int64_t stop = lptr[i + 1]; /* never written past: the same count */
    for (int64_t e = irp[i], end = irp[i + 1]; e < end && at < stop; ++e) {
        const int c = ja[e];
        if ((unsigned)c <= (unsigned)i) {
            lja[at] = c;
            las[at] = as[e];
            ++at;
        }
    }
}

/*
 * Row i by one lane.  THE RESULT CONTRACT (spmv_engine.h).  The pattern passed
 * k_ic0_check: the strict columns of row i are ascending, below i, and every
 * row ends with its diagonal, so every index below stays inside L.
 */
__device__ __forceinline__ void
ic0_row(int i, double shift, const int *__restrict__ irp,
        const int *__restrict__ ja, double *L, unsigned long long *bad) {
#pragma clang fp contract(off)
    const int bi = irp[i], di = irp[i + 1] - 1; /* di: the diagonal */
    double ss = 0.0;
    for (int t = bi; t < di; ++t) {
        const int j = ja[t];
        const int bj = irp[j], dj = irp[j + 1] - 1;
        double s = 0.0;
        int a = bi, b = bj;
        while (a < t && b < dj) { /* at most the two row lengths */
            const int ca = ja[a], cb = ja[b];
            if (ca == cb) {
                const double p = L[a] * L[b];
                s = s + p;
            }
            a += ca <= cb;
            b += cb <= ca;
        }
        const double num = L[t] - s;
        const double l = num / L[dj];
        L[t] = l;
        const double q = l * l;
        ss = ss + q;
    }
    const double aii = L[di];
    const double sh = shift * aii;
    const double shifted = aii + sh;
    const double d = shifted - ss;
    L[di] = __builtin_sqrt(d); /* correctly rounded (minres_kernels.hip) */
    if (!(d > 0.0))
        atomicAdd(bad, 1ull); /* a COUNT: any order of arrival */
}

/* one level: positions [first, end) of `order`, one lane each */
__global__ void __launch_bounds__(1024)
k_ic0_wide(int first, int end, double shift, const int *__restrict__ order,
           const int *__restrict__ irp, const int *__restrict__ ja, double *L,
           unsigned long long *bad) {
    const int64_t p = first + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < end)
        ic0_row(order[p], shift, irp, ja, L, bad);
}

/* levels l0 .. l1 by ONE workgroup: the loop bounds are workgroup-uniform, so
 * every lane reaches every barrier */
__global__ void __launch_bounds__(1024)
k_ic0_chain(int l0, int l1, double shift, const int *__restrict__ level_ptr,
            const int *__restrict__ order, const int *__restrict__ irp,
            const int *__restrict__ ja, double *L, unsigned long long *bad) {
    for (int l = l0; l <= l1; ++l) {
        const int end = level_ptr[l + 1];
        for (int64_t p = (int64_t)level_ptr[l] + threadIdx.x; p < end;
             p += blockDim.x)
            ic0_row(order[p], shift, irp, ja, L, bad);
        __syncthreads(); /* the level's rows are visible to the workgroup */
    }
}

static inline dim3 ic_grid(int64_t n, int threads) {
    return dim3((unsigned)transpose_ceil_div(n > 0 ? n : 1, threads));
}

int ic0_factor_dev(const spmv_csr_dev *A, double shift, int max_levels,
                   int waves, ic0_alloc_fn alloc, spmv_csr_dev **out,
                   spmv_ic0_info *info, hipStream_t s) {
    int rc = 0;
    const int M = A->M;
    const int wide_t = waves > 0 ? waves * WAVE : TRSV_WIDE_THREADS;
    const int chain_t = waves > 0 ? waves * WAVE : TRSV_THREADS;
    int *cnt = NULL, *sums = NULL;
    unsigned *d_flag = NULL; /* the flag word, then the count of bad pivots */
    unsigned long long *d_bad = NULL;
    unsigned flag = 0;
    unsigned long long bad = 0;
    int lnz = 0;
    spmv_csr_dev *L = NULL;
    spmv_trsv_plan P;
    memset(&P, 0, sizeof P);
    memset(info, 0, sizeof *info);
    (void)hipGetLastError(); /* an earlier caller's unread error is not ours */
    if (M == 0) { /* a valid empty handle: its row pointer is one zero */
        rc = alloc(0, 0, 0, 8, &L);
        if (rc)
            return rc;
        HIP_TRY(hipMemsetAsync(L->irp, 0, sizeof(int), s));
        HIP_TRY(hipStreamSynchronize(s));
        *out = L;
        return 0;
    }
    HIP_TRY(hipMalloc((void **)&cnt, ((size_t)M + 1) * sizeof(int)));
    HIP_TRY(hipMalloc((void **)&sums,
                      (size_t)transpose_scan_tiles((int64_t)M + 1) * sizeof(int)));
    HIP_TRY(hipMalloc((void **)&d_bad, 2 * sizeof(unsigned long long)));
    d_flag = (unsigned *)(d_bad + 1);
    HIP_TRY(hipMemsetAsync(cnt, 0, ((size_t)M + 1) * sizeof(int), s));
    HIP_TRY(hipMemsetAsync(d_bad, 0, 2 * sizeof(unsigned long long), s));
    if (M > 0)
        hipLaunchKernelGGL(k_ic0_check, ic_grid(M, IC_T), dim3(IC_T), 0, s, M,
                           A->irp, A->ja, cnt, d_flag);
    tr_scan(cnt, (int64_t)M + 1, sums, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&lnz, cnt + M, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&flag, d_flag, sizeof flag, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (flag & IC_BAD_COLUMN) {
        rc = -EDOM;
        goto fail;
    }
    if (flag & IC_BAD_ORDER) {
        rc = -EINVAL;
        goto fail;
    }
    if (lnz < M || lnz > A->NZ) {
        rc = -EIO; /* every row holds its diagonal, and no more than A holds */
        goto fail;
    }
    /* the schedule, before anything is allocated for the result: -E2BIG */
    rc = trsv_analyse_dev(A, 0, 0, max_levels, 0, 0, &P, s);
    if (rc)
        goto fail;
    rc = alloc(M, M, lnz, 8, &L);
    if (rc)
        goto fail;
    HIP_TRY(hipMemcpyAsync(L->irp, cnt, ((size_t)M + 1) * sizeof(int),
                           hipMemcpyDeviceToDevice, s));
    if (M > 0)
        hipLaunchKernelGGL(k_ic0_fill, ic_grid(M, IC_T), dim3(IC_T), 0, s, M,
                           A->irp, A->ja, A->as, cnt, L->ja, L->as);
    for (int i = 0; i < P.n_segs; ++i) {
        const trsv_segment &g = P.segs[i];
        if (g.kind == TRSV_WIDE) {
            const int first = P.h_level_ptr[g.first_level];
            const int end = P.h_level_ptr[g.first_level + 1];
            hipLaunchKernelGGL(k_ic0_wide, ic_grid(end - first, wide_t),
                               dim3(wide_t), 0, s, first, end, shift, P.order,
                               L->irp, L->ja, L->as, d_bad);
        } else {
            hipLaunchKernelGGL(k_ic0_chain, dim3(1), dim3(chain_t), 0, s,
                               g.first_level, g.last_level, shift, P.level_ptr,
                               P.order, L->irp, L->ja, L->as, d_bad);
        }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    info->levels = P.levels;
    info->launches = P.n_segs;
    info->entries = lnz;
    info->bad_pivots = (int64_t)bad;
    *out = L;
    L = NULL;
fail:
    if (rc) /* nothing of ours is left running when the scratch is freed */
        (void)hipStreamSynchronize(s);
    trsv_free_dev(&P);
    (void)hipFree(cnt);
    (void)hipFree(sums);
    (void)hipFree(d_bad);
    if (L)
        spmv_csr_release(L);
    return rc;
}
