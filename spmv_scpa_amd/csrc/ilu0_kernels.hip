/*
 * ilu0_kernels.hip -- zero-fill incomplete LU A ~ L U on the pattern of a
 * square f64 CSR handle (spmv_csr_ilu0; spmv_engine.h), gfx950 (wave64).
 *
 *   k_ilu0_check  one lane per row, in stored order: a flag for a column
 *                 outside [0, M), a flag for a row that is not strictly
 *                 ascending or stores no diagonal, and dpos[row] = the position
 *                 of the diagonal, so that the factor kernels never search it
 *   trsv_analyse_dev(A, lower)   the levels of the strict lower pattern are
 *                 the dependency order of a row-wise factorisation, as in
 *                 ic0_kernels.hip: row i reads the finished rows j of its
 *                 strict lower columns and nothing else.  Only order, level_ptr
 *                 and the launch list of that plan are used; the plan is freed
 *                 before the call returns
 *   k_ilu0_wide   ONE level of more than small_rows rows over a grid
 *   k_ilu0_chain  a maximal run of thinner levels in ONE workgroup with a
 *                 workgroup barrier between levels
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
 * operation is rounded once (contraction off), the division is IEEE.  Both
 * kernels call the same ilu0_row.
 *
 * There is NO waiting between workgroups: a row's dependencies were written by
 * an earlier kernel of the stream (wide) or by this workgroup before the last
 * barrier (chain, as k_trsv_chain).  W is read and written through one plain,
 * non-restrict pointer: vector loads and stores only.  Every device loop is
 * bounded by a row length.
 */
#include <stdlib.h>
#include <string.h>

#include "hip_common.h"
#include "transpose_plan.h"
#include "trsv_plan.h"

#define ILU_T 256 /* lanes of a check workgroup */
#define ILU_G 8   /* lanes of a row (EXPERIMENTS.md: one lane per row lost) */
#define ILU_BAD_COLUMN 1u
#define ILU_BAD_ORDER 2u

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
        atomicOr(flag, ILU_BAD_COLUMN);
    if (bad_order || !found)
        atomicOr(flag, ILU_BAD_ORDER);
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

/* one level: positions [first, end) of `order`, one group each */
__global__ void __launch_bounds__(1024)
k_ilu0_wide(int first, int end, double shift, const int *__restrict__ order,
            const int *__restrict__ irp, const int *__restrict__ ja,
            const int *__restrict__ dpos, double *W, unsigned long long *bad) {
    const int64_t p =
        first + ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / ILU_G;
    if (p < end)
        ilu0_row(order[p], threadIdx.x & (ILU_G - 1), shift, irp, ja, dpos, W,
                 bad);
}

/* levels l0 .. l1 by ONE workgroup: the loop bounds are workgroup-uniform, so
 * every lane reaches every barrier */
__global__ void __launch_bounds__(1024)
k_ilu0_chain(int l0, int l1, double shift, const int *__restrict__ level_ptr,
             const int *__restrict__ order, const int *__restrict__ irp,
             const int *__restrict__ ja, const int *__restrict__ dpos,
             double *W, unsigned long long *bad) {
    const int groups = blockDim.x / ILU_G;
    for (int l = l0; l <= l1; ++l) {
        const int end = level_ptr[l + 1];
        for (int64_t p = (int64_t)level_ptr[l] + threadIdx.x / ILU_G; p < end;
             p += groups)
            ilu0_row(order[p], threadIdx.x & (ILU_G - 1), shift, irp, ja, dpos,
                     W, bad);
        __syncthreads(); /* the level's rows are visible to the workgroup */
    }
}

static inline dim3 ilu_grid(int64_t n, int threads) {
    return dim3((unsigned)transpose_ceil_div(n > 0 ? n : 1, threads));
}

int ilu0_factor_dev(const spmv_csr_dev *A, double shift, int max_levels,
                    int waves, ic0_alloc_fn alloc, spmv_csr_dev **out,
                    spmv_ilu0_info *info, hipStream_t s) {
    int rc = 0;
    const int M = A->M;
    const int wide_t = waves > 0 ? waves * WAVE : TRSV_WIDE_THREADS;
    const int chain_t = waves > 0 ? waves * WAVE : TRSV_THREADS;
    int *dpos = NULL;
    unsigned *d_flag = NULL; /* the count of bad pivots, then the flag word */
    unsigned long long *d_bad = NULL;
    unsigned flag = 0;
    unsigned long long bad = 0;
    spmv_csr_dev *LU = NULL;
    spmv_trsv_plan P;
    memset(&P, 0, sizeof P);
    memset(info, 0, sizeof *info);
    (void)hipGetLastError(); /* an earlier caller's unread error is not ours */
    if (M == 0) { /* a valid empty handle: its row pointer is one zero */
        rc = alloc(0, 0, 0, 8, &LU);
        if (rc)
            return rc;
        HIP_TRY(hipMemsetAsync(LU->irp, 0, sizeof(int), s));
        HIP_TRY(hipStreamSynchronize(s));
        *out = LU;
        return 0;
    }
    HIP_TRY(hipMalloc((void **)&dpos, (size_t)M * sizeof(int)));
    HIP_TRY(hipMalloc((void **)&d_bad, 2 * sizeof(unsigned long long)));
    d_flag = (unsigned *)(d_bad + 1);
    HIP_TRY(hipMemsetAsync(d_bad, 0, 2 * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_ilu0_check, ilu_grid(M, ILU_T), dim3(ILU_T), 0, s, M,
                       A->irp, A->ja, dpos, d_flag);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&flag, d_flag, sizeof flag, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (flag & ILU_BAD_COLUMN) {
        rc = -EDOM;
        goto fail;
    }
    if (flag & ILU_BAD_ORDER) {
        rc = -EINVAL;
        goto fail;
    }
    /* the schedule, before anything is allocated for the result: -E2BIG */
    rc = trsv_analyse_dev(A, 0, 0, max_levels, 0, 0, &P, s);
    if (rc)
        goto fail;
    rc = alloc(M, M, A->NZ, 8, &LU);
    if (rc)
        goto fail;
    HIP_TRY(hipMemcpyAsync(LU->irp, A->irp, ((size_t)M + 1) * sizeof(int),
                           hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(LU->ja, A->ja, (size_t)A->NZ * sizeof(int),
                           hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(LU->as, A->as, (size_t)A->NZ * sizeof(double),
                           hipMemcpyDeviceToDevice, s));
    for (int i = 0; i < P.n_segs; ++i) {
        const trsv_segment &g = P.segs[i];
        if (g.kind == TRSV_WIDE) {
            const int first = P.h_level_ptr[g.first_level];
            const int end = P.h_level_ptr[g.first_level + 1];
            hipLaunchKernelGGL(k_ilu0_wide,
                               ilu_grid(end - first, wide_t / ILU_G),
                               dim3(wide_t), 0, s, first, end, shift, P.order,
                               LU->irp, LU->ja, dpos, LU->as, d_bad);
        } else {
            hipLaunchKernelGGL(k_ilu0_chain, dim3(1), dim3(chain_t), 0, s,
                               g.first_level, g.last_level, shift, P.level_ptr,
                               P.order, LU->irp, LU->ja, dpos,
                               LU->as, d_bad);
        }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    info->levels = P.levels;
    info->launches = P.n_segs;
    info->entries = A->NZ;
    info->bad_pivots = (int64_t)bad;
    *out = LU;
    LU = NULL;
fail:
    if (rc) /* nothing of ours is left running when the scratch is freed */
        (void)hipStreamSynchronize(s);
    trsv_free_dev(&P);
    (void)hipFree(dpos);
    (void)hipFree(d_bad);
    if (LU)
        spmv_csr_release(LU);
    return rc;
}
