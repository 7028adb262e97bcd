/*
 * ilu0_kernels.hip -- zero-fill incomplete LU A ~ L U on the pattern of a
 * square f64 CSR handle (spmv_csr_ilu0; spmv_engine.h), gfx950 (wave64).
 *
 *   k_ilu0_check  one lane per row, in stored order: a flag for a column
 *                 outside [0, M), a flag for a row that is not strictly
 *                 ascending or stores no diagonal, and dpos[row] = the position
 *                 of the diagonal, so that the factor kernels never search it
 *   factor_levels_dev   the schedule and its launches (factor_levels.h),
 *                 ILU_G lanes per row
 *
 * ilu0_row below is the result contract of spmv_csr_ilu0.  The factorisation
 * is IN PLACE in a copy of A's values: W[e] holds a_ic until the row's lanes
 * replace it.  ILU_G lanes share a row.  Lane g OWNS the positions e of row i
 * with (e - first) % ILU_G == g: only the owner ever reads or writes W[e], so
 * no value travels between lanes through memory and no ordering between them
 * is needed.  For the strict lower positions t in increasing order the owner
 * forms l = rn(w_t / u_jj), the group takes it by a shuffle, and every lane
 * updates the positions it owns behind t whose column is stored in the tail of
 * row j (a binary search of that tail).  For one t every w_m is touched at
 * most once and t increases, so each entry receives its updates in increasing
 * j: the bits are a function of A and shift alone, whatever ILU_G is.  Every
 * operation is rounded once (contraction off), the division is IEEE.
 *
 * W is read and written through one plain, non-restrict pointer: vector loads
 * and stores only.  Every device loop is bounded by a row length.
 */
#include <stdlib.h>

#include "factor_levels.h"

#define ILU_T 256 /* lanes of a check workgroup */
#define ILU_G 8   /* lanes of a row (EXPERIMENTS.md: one lane per row lost) */

static_assert(ILU_G > 0 && (ILU_G & (ILU_G - 1)) == 0 && WAVE % ILU_G == 0,
              "a group is a power of two of lanes inside one wavefront");

__global__ void __launch_bounds__(ILU_T)
k_ilu0_check(int M, const int *__restrict__ irp, const int *__restrict__ ja,
             int *__restrict__ dpos, unsigned *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * ILU_T + threadIdx.x;
    if (i >= M)
        return;
    const int beg = irp[i], end = irp[i + 1];
    int prev = -1, at = beg; /* at: a position inside A whatever the row holds */
    bool bad_col = false, bad_order = false, found = false;
    for (int e = beg; e < end; ++e) {
        const int c = ja[e];
        if ((unsigned)c >= (unsigned)M) {
            bad_col = true;
        } else {
            if (c <= prev)
                bad_order = true;
            prev = c;
            if (c == (int)i) {
                found = true;
                at = e;
            }
        }
    }
    dpos[i] = at;
    if (bad_col)
        atomicOr(flag, CSR_BAD_COLUMN);
    if (bad_order || !found)
        atomicOr(flag, CSR_BAD_ORDER);
}

/*
 * Row i by the ILU_G lanes of one group, g = the lane's number in it.  THE
 * RESULT CONTRACT (spmv_engine.h).  The pattern passed k_ilu0_check: every row
 * is strictly ascending, inside [0, M), and dpos[r] is the position of row r's
 * diagonal, so the positions before dpos[i] hold columns below i and every
 * index below stays inside W.  All lanes of a group call with the same i: the
 * trip count of the loop over t is the same for them, so they meet at the
 * shuffle.
 */
__device__ __forceinline__ void
ilu0_row(int i, int g, double shift, const int *__restrict__ irp,
         const int *__restrict__ ja, const int *__restrict__ dpos, double *W,
         unsigned long long *bad) {
#pragma clang fp contract(off)
    const int bi = irp[i], ei = irp[i + 1], di = dpos[i];
    const bool owns_diag = ((di - bi) & (ILU_G - 1)) == g;
    if (owns_diag) {
        const double aii = W[di];
        const double sh = shift * aii;
        W[di] = aii + sh;
    }
    for (int t = bi; t < di; ++t) {
        const int j = ja[t];
        const int dj = dpos[j], ej = irp[j + 1];
        const int owner = (t - bi) & (ILU_G - 1);
        double l = 0.0;
        if (g == owner) {
            l = W[t] / W[dj];
            W[t] = l;
        }
        l = __shfl(l, owner, ILU_G);
        /* the first position behind t that this lane owns */
        int e = t + 1 + ((g - (t + 1 - bi)) & (ILU_G - 1));
        for (; e < ei; e += ILU_G) {
            const int m = ja[e];
            int lo = dj + 1, hi = ej; /* the tail of row j: columns > j */
            while (lo < hi) {
                const int mid = lo + ((hi - lo) >> 1);
                if (ja[mid] < m)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            if (lo < ej && ja[lo] == m) {
                const double p = l * W[lo];
                W[e] = W[e] - p;
            }
        }
    }
    if (owns_diag) {
        const double u = W[di];
        if (!(u != 0.0 && __builtin_fabs(u) <= 1.7976931348623157e308))
            atomicAdd(bad, 1ull); /* a COUNT: any order of arrival */
    }
}

/* the row routine as factor_levels.h runs it, ILU_G lanes per row */
struct ilu0_rows {
    double shift;
    const int *dpos;
    unsigned long long *bad;
    const int *irp, *ja; /* of LU */
    double *as;
    __device__ void operator()(int i, int g) const {
        ilu0_row(i, g, shift, irp, ja, dpos, as, bad);
    }
};

int ilu0_factor_dev(const spmv_csr_dev *A, double shift, int max_levels,
                    int waves, spmv_csr_dev **out, spmv_ilu0_info *info,
                    hipStream_t s) {
    int rc = 0;
    const int M = A->M;
    int *dpos = NULL;
    unsigned *d_flag = NULL; /* the count of bad pivots, then the flag word */
    unsigned long long *d_bad = NULL;
    unsigned flag = 0;
    memset(info, 0, sizeof *info);
    (void)hipGetLastError(); /* an earlier caller's unread error is not ours */
    if (M == 0)
        return factor_empty_dev(out, s);
    HIP_TRY(hipMalloc((void **)&dpos, (size_t)M * sizeof(int)));
    HIP_TRY(hipMalloc((void **)&d_bad, 2 * sizeof(unsigned long long)));
    d_flag = (unsigned *)(d_bad + 1);
    HIP_TRY(hipMemsetAsync(d_bad, 0, 2 * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_ilu0_check, grid_for(M, ILU_T), dim3(ILU_T), 0, s, M,
                       A->irp, A->ja, dpos, d_flag);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&flag, d_flag, sizeof flag, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    rc = csr_flags_errno(flag);
    if (rc)
        goto fail;
    rc = factor_levels_dev<ILU_G>(
        A, max_levels, waves, A->NZ,
        ilu0_rows{shift, dpos, d_bad, NULL, NULL, NULL},
        [&](spmv_csr_dev *LU) { /* A's pattern and values */
            HIP_RET(hipMemcpyAsync(LU->irp, A->irp,
                                   ((size_t)M + 1) * sizeof(int),
                                   hipMemcpyDeviceToDevice, s));
            HIP_RET(hipMemcpyAsync(LU->ja, A->ja, (size_t)A->NZ * sizeof(int),
                                   hipMemcpyDeviceToDevice, s));
            HIP_RET(hipMemcpyAsync(LU->as, A->as,
                                   (size_t)A->NZ * sizeof(double),
                                   hipMemcpyDeviceToDevice, s));
            return 0;
        },
        d_bad, out, info, s);
fail:
    if (rc) /* nothing of ours is left running when the scratch is freed */
        (void)hipStreamSynchronize(s);
    (void)hipFree(dpos);
    (void)hipFree(d_bad);
    return rc;
}
