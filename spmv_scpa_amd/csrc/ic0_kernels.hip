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
 *   factor_levels_dev   the schedule and its launches (factor_levels.h), one
 *                 lane per row
 *
 * ic0_row below is the result contract of spmv_csr_ic0: one lane per row, a
 * two-pointer merge of row i with row j for every strict entry (i, j), every
 * operation rounded once (contraction off), an IEEE division, a correctly
 * rounded square root.  The factorisation is IN PLACE: L[t] holds a_ij until
 * the lane replaces it with l_ij, and everything the lane reads of its own row
 * it wrote itself before.
 *
 * L is read and written through one plain, non-restrict pointer: vector loads
 * only.  Every device loop is bounded by a row length.
 */
#include <stdlib.h>

#include "factor_levels.h"

#define IC_T 256 /* lanes of a check / fill workgroup */

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
        atomicOr(flag, CSR_BAD_COLUMN);
    if (bad_order || prev != (int)i) /* ascending: the diagonal is the last */
        atomicOr(flag, CSR_BAD_ORDER);
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

/* the row routine as factor_levels.h runs it, one lane per row */
struct ic0_rows {
    double shift;
    unsigned long long *bad;
    const int *irp, *ja; /* of L */
    double *as;
    __device__ void operator()(int i, int) const {
        ic0_row(i, shift, irp, ja, as, bad);
    }
};

int ic0_factor_dev(const spmv_csr_dev *A, double shift, int max_levels,
                   int waves, spmv_csr_dev **out, spmv_ic0_info *info,
                   hipStream_t s) {
    int rc = 0;
    const int M = A->M;
    int *cnt = NULL, *sums = NULL;
    unsigned *d_flag = NULL; /* the count of bad pivots, then the flag word */
    unsigned long long *d_bad = NULL;
    unsigned flag = 0;
    int lnz = 0;
    memset(info, 0, sizeof *info);
    (void)hipGetLastError(); /* an earlier caller's unread error is not ours */
    if (M == 0)
        return factor_empty_dev(out, s);
    HIP_TRY(hipMalloc((void **)&cnt, ((size_t)M + 1) * sizeof(int)));
    HIP_TRY(hipMalloc((void **)&sums,
                      (size_t)transpose_scan_tiles((int64_t)M + 1) * sizeof(int)));
    HIP_TRY(hipMalloc((void **)&d_bad, 2 * sizeof(unsigned long long)));
    d_flag = (unsigned *)(d_bad + 1);
    HIP_TRY(hipMemsetAsync(cnt, 0, ((size_t)M + 1) * sizeof(int), s));
    HIP_TRY(hipMemsetAsync(d_bad, 0, 2 * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_ic0_check, grid_for(M, IC_T), dim3(IC_T), 0, s, M,
                       A->irp, A->ja, cnt, d_flag);
    tr_scan(cnt, (int64_t)M + 1, sums, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&lnz, cnt + M, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&flag, d_flag, sizeof flag, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    rc = csr_flags_errno(flag);
    if (rc)
        goto fail;
    if (lnz < M || lnz > A->NZ) {
        rc = -EIO; /* every row holds its diagonal, and no more than A holds */
        goto fail;
    }
    rc = factor_levels_dev<1>(
        A, max_levels, waves, lnz, ic0_rows{shift, d_bad, NULL, NULL, NULL},
        [&](spmv_csr_dev *L) { /* the lower triangle, A's values in it */
            HIP_RET(hipMemcpyAsync(L->irp, cnt, ((size_t)M + 1) * sizeof(int),
                                   hipMemcpyDeviceToDevice, s));
            hipLaunchKernelGGL(k_ic0_fill, grid_for(M, IC_T), dim3(IC_T), 0, s,
                               M, A->irp, A->ja, A->as, cnt, L->ja, L->as);
            return 0;
        },
        d_bad, out, info, s);
fail:
    if (rc) /* nothing of ours is left running when the scratch is freed */
        (void)hipStreamSynchronize(s);
    (void)hipFree(cnt);
    (void)hipFree(sums);
    (void)hipFree(d_bad);
    return rc;
}
