/*
 * solver_work.h -- the work buffer of the device-resident solvers
 * (cg_kernels.hip, bicgstab_kernels.hip, cgls_kernels.hip, minres_kernels.hip,
 * gmres_kernels.hip),
 * described ONCE: the size a caller is told (*_work_bytes) and the pointers a
 * solve cuts the buffer into come from the same description, so a vector added
 * to one cannot be forgotten in the other.
 *
 * Header-only and free of HIP: tests/asan/solver_work_asan.cc runs it under
 * AddressSanitizer + UBSan on the CPU.
 *
 * A buffer is, in this order: the state block (state_bytes), `parts` sets of
 * partial sums of CG_PART_BYTES each, `vectors` vectors of rows[i] rows of k
 * interleaved doubles each.  Every offset is a multiple of 8.
 */
#ifndef SPMV_SOLVER_WORK_H
#define SPMV_SOLVER_WORK_H

#include <errno.h>
#include <stdint.h>

#include "gmres_small.h"

#define CG_MAXK 8 /* right-hand sides of one solve */
/* workgroups of a dot: part of the result contract (hip_common.h, CG_T) */
#define CG_NWG 1024
#define CG_PART_BYTES (CG_NWG * 8 * 8) /* CG_NWG workgroup sums of 8 columns */
#define CG_STATE_BYTES 512  /* cg_state, bi_state, ls_state */
#define MR_STATE_BYTES 2048 /* mr_state */
#define GM_HEAD_BYTES 512   /* gm_state: the part of GMRES' state read back */

#define SOLVER_WORK_MAXV 7

struct solver_work {
    int k;
    int64_t state_bytes;
    int parts;
    int vectors;
    int64_t rows[SOLVER_WORK_MAXV]; /* of vector i */
};

/* byte offset of the i-th set of partial sums, i in 0..parts */
static inline int64_t solver_work_part(const solver_work &w, int i) {
    return w.state_bytes + (int64_t)i * CG_PART_BYTES;
}

/* byte offset of vector i, i in 0..vectors; i == vectors: the end */
static inline int64_t solver_work_vec(const solver_work &w, int i) {
    int64_t at = solver_work_part(w, w.parts);
    for (int v = 0; v < i; ++v)
        at += 8 * w.rows[v] * w.k;
    return at;
}

/* the size of the buffer; -EINVAL for a negative row count or k outside
 * 1..CG_MAXK */
static inline int64_t solver_work_bytes(const solver_work &w) {
    if (w.k < 1 || w.k > CG_MAXK)
        return -EINVAL;
    for (int v = 0; v < w.vectors; ++v)
        if (w.rows[v] < 0)
            return -EINVAL;
    return solver_work_vec(w, w.vectors);
}

/* ---- the buffers of the solvers: what each vector is, in its solve ---- */

/* pre 0: spmv_*_cg, parts (pq, rn), R, P, Q;  1: spmv_*_pcg, a third set (zn,
 * live together with rn);  2: spmv_*_pcg_trsv, and a stored Z behind Q */
static inline solver_work cg_work(int M, int k, int pre) {
    return solver_work{k, CG_STATE_BYTES, pre ? 3 : 2, pre == 2 ? 4 : 3,
                       {M, M, M, M}};
}

/* parts (rv | ts | rn | bb), (tt | rhon | rr);  R, Rh, P, V, T, Z */
static inline solver_work bicgstab_work(int M, int k) {
    return solver_work{k, CG_STATE_BYTES, 2, 6, {M, M, M, M, M, M}};
}

/* spmv_*_bicgstab_trsv: the same parts;  R, Rh, P, V, T, Zp = z(P), Zs = z(S):
 * the plans cannot recompute a z, so both are stored and live at the update */
static inline solver_work bicgstab_trsv_work(int M, int k) {
    return solver_work{k, CG_STATE_BYTES, 2, 7, {M, M, M, M, M, M, M}};
}

/* parts (qq | ss | sn | rr), atb, pp;  R, Q of M rows, S, P of N rows */
static inline solver_work cgls_work(int M, int N, int k) {
    return solver_work{k, CG_STATE_BYTES, 3, 4, {M, M, N, N}};
}

/* parts (bb | alfa | rr), (bn2 | bnew), b1;  two residuals, V, Q, two
 * directions (the pair is zeroed by one memset: neighbours) */
static inline solver_work minres_work(int M, int k) {
    return solver_work{k, MR_STATE_BYTES, 3, 6, {M, M, M, M, M, M}};
}

/* spmv_*_gmres and spmv_*_gmres_trsv, restart in 1..GM_MAXM (the caller's
 * check; anything else gives a buffer solver_work_bytes refuses): the state is
 * gm_state and, behind it, the blocks of gmres_small.h for 8 columns, so it
 * depends on restart alone; one set of partial sums per basis vector (bb, rr
 * and nn pass through sets 0 and 1);  the basis as ONE vector of
 * (restart + 1) M rows -- basis vector i starts at element (size_t)i * M * k --
 * then W and Z */
static inline solver_work gmres_work(int M, int k, int restart) {
    if (restart < 1 || restart > GM_MAXM)
        return solver_work{k, GM_HEAD_BYTES, 0, 1, {-1}};
    return solver_work{
        k,
        GM_HEAD_BYTES + 8 * CG_MAXK * (int64_t)gm_col_doubles(restart),
        restart + 1,
        3,
        {(int64_t)(restart + 1) * M, M, M}};
}

#endif /* SPMV_SOLVER_WORK_H */
