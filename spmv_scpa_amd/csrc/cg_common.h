/*
 * cg_common.h -- what the device-resident solvers share (cg_kernels.hip:
 * spmv_*_cg / spmv_*_pcg; bicgstab_kernels.hip: spmv_*_bicgstab;
 * cgls_kernels.hip: spmv_*_cgls; minres_kernels.hip: spmv_*_minres;
 * gmres_kernels.hip: spmv_*_gmres): the tile of a vector kernel, the two
 * halving trees of the dot order, the finite test, the square root (mr_sqrt),
 * the frozen-column test (cg_running), the launch macros and the plan apply of
 * the _trsv solvers (bi_apply).  One text, included by these files; the two
 * kernels every solver launches (k_cg_copy, k_cg_dot) stay in cg_kernels.hip and are reached through cg_launch_copy /
 * cg_launch_dot (hip_common.h), so they exist once in the library.  The host
 * side the solvers share is included from here too: the work buffer
 * (solver_work.h, through hip_common.h) and the refusals, the own buffer and
 * the bounded loop of a solve (solver_host.h, solver_run).
 *
 * DOT ORDER, a function of M alone (CG_NWG, CG_T are constants of the
 * library, exported to the tests as spmv_cg_dot_shape):
 *   element i belongs to slot i mod (CG_NWG * CG_T); slot s is slot s % CG_T
 *   of workgroup s / CG_T.  A slot starts at 0.0 and adds rn(u_i * v_i) in
 *   increasing i.  The CG_T slots of a workgroup are combined by a halving
 *   tree, s[t] += s[t + h] for h = CG_T / 2 .. 1; the CG_NWG workgroup sums by
 *   the same tree.  Workgroups whose slots hold no element are not launched:
 *   their sum is the 0.0 the tree would have given.
 */
#ifndef SPMV_CG_COMMON_H
#define SPMV_CG_COMMON_H

#include "solver_host.h"

#define CG_FINAL_T 1024 /* threads of a finalising workgroup, >= CG_NWG */

static_assert(CG_FINAL_T >= CG_NWG && (CG_NWG & (CG_NWG - 1)) == 0 &&
                  (CG_T & (CG_T - 1)) == 0,
              "the halving trees need powers of two");

/*
 * LANES.  A workgroup's share of one sweep is a tile of CG_T rows x K columns
 * -- CG_T * K consecutive doubles in R, P, Q (ld = K).  Which lane holds which
 * slot is no part of the dot order, so the tile is read the way memory wants
 * it: in pass n = 0..K-1 thread p takes element f = p + n CG_T of the tile,
 * row t = f / K, column j = f % K -- a wavefront's load is 512 consecutive
 * bytes, whatever K.  (One row per thread was measured first: at K = 8 a load
 * touched 64 lines for 8 bytes each and the three kernels ran at 1.5 TB/s.)
 * (t, j) of a pass is the same in every sweep, so acc[n] is the slot sum of
 * (slot t, column j).  The loads are unconditional, at a row clamped to M - 1,
 * so all K passes are in flight together; sums and stores are predicated.  A
 * frozen column shares its cache lines with the running ones: it may be read,
 * it is never written.
 */
template <int K> struct cg_lanes {
    int t[K], j[K];
    __device__ __forceinline__ cg_lanes() {
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int f = threadIdx.x + n * CG_T;
            t[n] = f / K;
            j[n] = f % K;
        }
    }
};

/* running[n]: the column of pass n is running (State: a solver's state block,
 * with its status[CG_MAXK]) */
template <int K, typename State>
__device__ __forceinline__ void cg_running(const State *st,
                                           const cg_lanes<K> &l,
                                           bool (&running)[K]) {
#pragma unroll
    for (int n = 0; n < K; ++n)
        running[n] = st->status[l.j[n]] == CG_RUNNING;
}

/* The slot sums of a workgroup -> part[blockIdx.x * K + j]: the halving tree
 * of the dot order.  All CG_T threads call. */
template <int K>
__device__ __forceinline__ void slots_to_partial(const cg_lanes<K> &l,
                                                 const double (&acc)[K],
                                                 double *__restrict__ part) {
    __shared__ double s[K][CG_T];
    const int t = threadIdx.x;
#pragma unroll
    for (int n = 0; n < K; ++n)
        s[l.j[n]][l.t[n]] = acc[n];
    __syncthreads();
    for (int h = CG_T / 2; h > 0; h >>= 1) {
        if (t < h) {
#pragma unroll
            for (int j = 0; j < K; ++j)
                s[j][t] += s[j][t + h];
        }
        __syncthreads();
    }
    if (t < K)
        part[(size_t)blockIdx.x * K + t] = s[t][0];
}

/* the sweeps of a workgroup: `base` = first row of its tile */
#define CG_SWEEPS(base, M)                                                    \
    for (int64_t base = (int64_t)blockIdx.x * CG_T; base < (M);               \
         base += (int64_t)CG_NWG * CG_T)

/* ---- helpers of the finalising kernels ---- */

/* column j of the nwg workgroup sums (0.0 for the workgroups that were not
 * launched) by the halving tree over CG_NWG; the total in every thread */
__device__ __forceinline__ double final_sum(const double *__restrict__ part,
                                            int nwg, int k, int j, double *s) {
    const int t = threadIdx.x;
    s[t] = t < nwg ? part[(size_t)t * k + j] : 0.0;
    __syncthreads();
    for (int h = CG_NWG / 2; h > 0; h >>= 1) {
        if (t < h)
            s[t] += s[t + h];
        __syncthreads();
    }
    const double v = s[0];
    __syncthreads(); /* s is reused for the next column */
    return v;
}

__device__ __forceinline__ bool cg_finite(double v) {
    return __builtin_fabs(v) <= 1.7976931348623157e308; /* false for NaN */
}

/* The one square root of the library: correctly rounded (the v_rsq_f64
 * refinement with two residual corrections the compiler expands
 * __builtin_sqrt to; spmv_debug_sqrt checks it against the host's) */
__device__ __forceinline__ double mr_sqrt(double a) {
    return __builtin_sqrt(a);
}

/* ---- launches ---- */

/* workgroups whose slots hold an element */
static inline unsigned cg_grid(int M) {
    const int64_t g = ((int64_t)M + CG_T - 1) / CG_T;
    return (unsigned)(g < CG_NWG ? g : CG_NWG);
}

#define CG_K_SWITCH(k, CALL, ...)                                             \
    switch (k) {                                                              \
    case 1: CALL(1, __VA_ARGS__); break;                                      \
    case 2: CALL(2, __VA_ARGS__); break;                                      \
    case 3: CALL(3, __VA_ARGS__); break;                                      \
    case 4: CALL(4, __VA_ARGS__); break;                                      \
    case 5: CALL(5, __VA_ARGS__); break;                                      \
    case 6: CALL(6, __VA_ARGS__); break;                                      \
    case 7: CALL(7, __VA_ARGS__); break;                                      \
    default: CALL(8, __VA_ARGS__); break;                                     \
    }

/* kernel<k>(M, ...) over the slots of M rows on stream s: every vector kernel */
#define CG_LAUNCH_K(KK, kernel, M, s, ...)                                    \
    hipLaunchKernelGGL((kernel<KK>), dim3(cg_grid(M)), dim3(CG_T), 0, s, M,    \
                       __VA_ARGS__)
#define CG_LAUNCH(kernel, k, M, s, ...)                                       \
    CG_K_SWITCH(k, CG_LAUNCH_K, kernel, M, s, __VA_ARGS__)
/* kernel<k, flag>(M, ...) the same way: the vector kernels with a second, bool
 * template argument (a preconditioner, a damping term, the first iteration) */
#define CG_LAUNCH_FLAG_K(KK, kernel, flag, M, s, ...)                         \
    do {                                                                      \
        if (flag)                                                             \
            hipLaunchKernelGGL((kernel<KK, true>), dim3(cg_grid(M)),          \
                               dim3(CG_T), 0, s, M, __VA_ARGS__);             \
        else                                                                  \
            hipLaunchKernelGGL((kernel<KK, false>), dim3(cg_grid(M)),         \
                               dim3(CG_T), 0, s, M, __VA_ARGS__);             \
    } while (0)
#define CG_LAUNCH_FLAG(kernel, flag, k, M, s, ...)                            \
    CG_K_SWITCH(k, CG_LAUNCH_FLAG_K, kernel, flag, M, s, __VA_ARGS__)
/* kernel(...) in one workgroup on stream s: every finalising kernel */
#define CG_FINAL(kernel, s, ...)                                              \
    hipLaunchKernelGGL(kernel, dim3(1), dim3(CG_FINAL_T), 0, s, __VA_ARGS__)

/* Z = z(U) of spmv_*_bicgstab_trsv and spmv_*_gmres_trsv, all k columns (a
 * frozen column's Z reaches nothing: every consumer is predicated); a refused
 * plan solve is the code that ends the batch */
static inline int bi_apply(const cg_plans &pl, int k, const double *U,
                           double *Z, hipStream_t s) {
    int rc = trsv_solve_dev(pl.first, pl.waves, k, U, k, Z, k, NULL, s);
    if (!rc && pl.second)
        rc = trsv_solve_dev(pl.second, pl.waves, k, Z, k, Z, k, pl.scale, s);
    return rc;
}

#endif /* SPMV_CG_COMMON_H */
