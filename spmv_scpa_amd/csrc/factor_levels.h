/*
 * factor_levels.h -- the level-scheduled driver of the two zero-fill
 * factorisations (ic0_kernels.hip, ilu0_kernels.hip): what runs a row routine
 * over the levels of the strict lower pattern.  Not installed.
 *
 *   trsv_analyse_dev(A, lower)   the levels of the strict lower pattern are
 *                 the dependency order of a row-wise factorisation: row i reads
 *                 the finished rows j of its strict lower columns and nothing
 *                 else.  Only order, level_ptr and the launch list of that plan
 *                 are used; the plan is freed before the call returns
 *   k_factor_wide   ONE level of more than small_rows rows over a grid
 *   k_factor_chain  a maximal run of thinner levels in ONE workgroup with a
 *                 workgroup barrier between levels
 *
 * Both kernels call the same row functor, so the bits do not depend on which
 * kernel ran a level or on the workgroup size.  There is NO waiting between
 * workgroups: a row's dependencies were written by an earlier kernel of the
 * stream (wide) or by this workgroup before the last barrier (chain, as
 * k_trsv_chain).
 *
 * Row: passed by value, carries the factorisation's pointers and shift; the
 * driver points its members irp, ja and as at the factor's arrays;
 * operator()(row, lane of the row's group) is the row routine.  G lanes share
 * a row; with G == 1 the divisions and masks below fold away.
 */
#ifndef SPMV_FACTOR_LEVELS_H
#define SPMV_FACTOR_LEVELS_H

#include <string.h>

#include "csr_build.h"
#include "trsv_plan.h"

/* one level: positions [first, end) of `order`, one group each */
template <int G, typename Row>
__global__ void __launch_bounds__(1024)
k_factor_wide(int first, int end, const int *__restrict__ order, Row row) {
    const int64_t p =
        first + ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    if (p < end)
        row(order[p], threadIdx.x & (G - 1));
}

/* levels l0 .. l1 by ONE workgroup: the loop bounds are workgroup-uniform, so
 * every lane reaches every barrier */
template <int G, typename Row>
__global__ void __launch_bounds__(1024)
k_factor_chain(int l0, int l1, const int *__restrict__ level_ptr,
               const int *__restrict__ order, Row row) {
    const int groups = blockDim.x / G;
    for (int l = l0; l <= l1; ++l) {
        const int end = level_ptr[l + 1];
        for (int64_t p = (int64_t)level_ptr[l] + threadIdx.x / G; p < end;
             p += groups)
            row(order[p], threadIdx.x & (G - 1));
        __syncthreads(); /* the level's rows are visible to the workgroup */
    }
}

/* the factor of a 0 x 0 matrix, a valid empty handle: its row pointer is one
 * zero */
static inline int factor_empty_dev(spmv_csr_dev **out, hipStream_t s) {
    spmv_csr_dev *F = NULL;
    int rc = csr_alloc_dev(0, 0, 0, 8, &F);
    if (rc)
        return rc;
    rc = hip_errno(hipMemsetAsync(F->irp, 0, sizeof(int), s));
    if (!rc)
        rc = hip_errno(hipStreamSynchronize(s));
    if (rc) {
        spmv_csr_release(F);
        return rc;
    }
    *out = F;
    return 0;
}

/*
 * A (M > 0) passed the caller's check.  The schedule is made before anything
 * is allocated for the result (-E2BIG: more than max_levels levels); *out then
 * comes from csr_alloc_dev(M, M, entries, f64), fill(*out) enqueues what puts
 * the pattern and A's values into it, and the rows are factorised level by
 * level.  d_bad: a zeroed device word of the caller's, the count of bad
 * pivots the row routine keeps.  waves 0 = each kernel's default.  Blocks; on
 * an error *out is untouched and everything made here is freed.
 */
template <int G, typename Row, typename Fill, typename Info>
static int factor_levels_dev(const spmv_csr_dev *A, int max_levels, int waves,
                             int64_t entries, Row row, Fill fill,
                             const unsigned long long *d_bad,
                             spmv_csr_dev **out, Info *info, hipStream_t s) {
    int rc = 0;
    const int M = A->M;
    const int wide_t = waves > 0 ? waves * WAVE : TRSV_WIDE_THREADS;
    const int chain_t = waves > 0 ? waves * WAVE : TRSV_THREADS;
    unsigned long long bad = 0;
    spmv_csr_dev *F = NULL;
    spmv_trsv_plan P;
    memset(&P, 0, sizeof P);
    rc = trsv_analyse_dev(A, 0, 0, max_levels, 0, 0, &P, s);
    if (rc)
        goto fail;
    rc = csr_alloc_dev(M, M, entries, 8, &F);
    if (rc)
        goto fail;
    rc = fill(F);
    if (rc)
        goto fail;
    row.irp = F->irp;
    row.ja = F->ja;
    row.as = F->as;
    for (int i = 0; i < P.n_segs; ++i) {
        const trsv_segment &g = P.segs[i];
        if (g.kind == TRSV_WIDE) {
            const int first = P.h_level_ptr[g.first_level];
            const int end = P.h_level_ptr[g.first_level + 1];
            hipLaunchKernelGGL((k_factor_wide<G, Row>),
                               grid_for(end - first, wide_t / G), dim3(wide_t),
                               0, s, first, end, P.order, row);
        } else {
            hipLaunchKernelGGL((k_factor_chain<G, Row>), dim3(1), dim3(chain_t),
                               0, s, g.first_level, g.last_level, P.level_ptr,
                               P.order, row);
        }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    info->levels = P.levels;
    info->launches = P.n_segs;
    info->entries = entries;
    info->bad_pivots = (int64_t)bad;
    *out = F;
    F = NULL;
fail:
    if (rc) /* nothing of ours is left running when the plan is freed */
        (void)hipStreamSynchronize(s);
    trsv_free_dev(&P);
    spmv_csr_release(F); /* NULL: ignored */
    return rc;
}

#endif /* SPMV_FACTOR_LEVELS_H */
