/*
 * cg_kernels.hip -- conjugate gradients for A X = B on the device, plain
 * (spmv_*_cg, spmv_engine.h) and with a diagonal preconditioner (spmv_*_pcg):
 * k = 1..8 independent systems stored interleaved (X[i * ldx + j]), A a CSR or
 * column-major HLL handle, gfx950 (wave64).
 *
 * The product Q = A P and the initial residual are the handle's launch_multi /
 * launch_axpby (two function pointers, cg_matrix); everything else is here:
 * the fixed-order dot, the two fused vector updates and the per-column state.
 * Templates over the number of vectors K, as in multi_kernels.hip.  The host
 * side -- the refusals, the own work buffer, the bounded loop -- is
 * solver_run (solver_host.h), shared with the other solvers; cg_solve gives it
 * the buffer (cg_work, solver_work.h) and its launches.
 *
 * The kernels both solvers launch (k_cg_copy, k_cg_dot) and the one only the
 * preconditioned solver has (k_pcg_first) are in this file.
 * The kernels of an iteration -- update, dir, final_init, final_pq, final_rr /
 * final_rz -- are in cg_body.h, written once and included twice below: the
 * k_cg_* and the k_pcg_* kernel of a pair are one text.  The solver
 * preconditioned by triangular plans (spmv_*_pcg_trsv) has no kernel of its
 * own: pcgt_start / pcgt_iterate below enqueue the plain vector kernels, the
 * plans' solves and the finalising kernels of the preconditioned pass.  The
 * solver preconditioned by an AMG cycle (spmv_*_pcg_amg) is the same text with
 * the cycle (cg_plans.apply, engine.hip) where the plans' solves are.
 *
 * The dot order, the tile of a vector kernel (cg_lanes), the halving trees and
 * the launch macros are in cg_common.h, shared with the other solvers.
 *
 * STATE.  alpha, beta, rr, bb, status and the iteration count of every column
 * live in one cg_state block at the head of the work buffer.  It is written
 * by ONE workgroup: the finalising kernels k_cg_final_*, one thread per column,
 * plain stores.  The vector kernels only read it.  No workgroup ever waits for
 * another; no counters, no atomics: every dependence is a kernel boundary on
 * the stream.
 *
 * A column whose status is not CG_RUNNING is frozen: the vector kernels
 * predicate its stores and its sums away, the finalising kernels leave its
 * state alone.  So X, R, P and rr of a frozen column keep their bits
 * however many iterations are enqueued after it stopped, and whatever the
 * other columns hold.
 */
#include "cg_common.h"

/* per-column state, device memory (CG_STATE_BYTES at the head of the work
 * buffer) */
struct cg_state {
    double rr[CG_MAXK];    /* r.r of the recurrence */
    double bb[CG_MAXK];    /* b.b */
    double alpha[CG_MAXK]; /* of the iteration under way */
    double beta[CG_MAXK];
    int status[CG_MAXK];   /* spmv_cg_info.status, or CG_RUNNING */
    int iters[CG_MAXK];    /* updates of x applied */
    double rz[CG_MAXK];    /* r.z of the preconditioned recurrence (CG_PRE 1
                              only; behind the fields the plain kernels use) */
};
static_assert(sizeof(cg_state) <= CG_STATE_BYTES, "state block");

/* dst[i * ldd + j] = src[i * lds + j], j < K (R = B, P = R) */
template <int K>
__global__ void __launch_bounds__(CG_T)
k_cg_copy(int M, const double *__restrict__ src, int64_t lds,
          double *__restrict__ dst, int64_t ldd) {
    const cg_lanes<K> l;
    CG_SWEEPS(base, M) {
        double v[K];
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n] < M ? base + l.t[n] : M - 1;
            v[n] = src[i * lds + l.j[n]];
        }
#pragma unroll
        for (int n = 0; n < K; ++n)
            if (base + l.t[n] < M)
                dst[(base + l.t[n]) * ldd + l.j[n]] = v[n];
    }
}

/* partial dot: part[w * K + j] = workgroup w's sum of U[:, j] . V[:, j] */
template <int K>
__global__ void __launch_bounds__(CG_T)
k_cg_dot(int M, const double *__restrict__ U, int64_t ldu,
         const double *__restrict__ V, int64_t ldv, double *__restrict__ part) {
#pragma clang fp contract(off)
    const cg_lanes<K> l;
    double acc[K];
#pragma unroll
    for (int n = 0; n < K; ++n)
        acc[n] = 0.0;
    CG_SWEEPS(base, M) {
        double u[K], v[K];
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n] < M ? base + l.t[n] : M - 1;
            u[n] = U[i * ldu + l.j[n]];
            v[n] = V[i * ldv + l.j[n]];
        }
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const double p = u[n] * v[n];
            const double sum = acc[n] + p;
            acc[n] = base + l.t[n] < M ? sum : acc[n];
        }
    }
    slots_to_partial<K>(l, acc, part);
}

/* preconditioned only (z(R) = rn(minv_i * r_i) per row, cg_body.h):
 * dst = z(src) (P = z(R)) and the partials of src . z(src), both interleaved
 * with ld = K; all columns (nothing is frozen before the first classification) */
template <int K>
__global__ void __launch_bounds__(CG_T)
k_pcg_first(int M, const double *__restrict__ minv,
            const double *__restrict__ R, double *__restrict__ P,
            double *__restrict__ part) {
#pragma clang fp contract(off)
    const cg_lanes<K> l;
    double acc[K];
#pragma unroll
    for (int n = 0; n < K; ++n)
        acc[n] = 0.0;
    CG_SWEEPS(base, M) {
        double r[K], d[K];
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n] < M ? base + l.t[n] : M - 1;
            r[n] = R[i * K + l.j[n]];
            d[n] = minv[i];
        }
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n];
            const double z = d[n] * r[n];
            const double rz = r[n] * z;
            const double sum = acc[n] + rz;
            if (i < M) {
                P[i * K + l.j[n]] = z;
                acc[n] = sum;
            }
        }
    }
    slots_to_partial<K>(l, acc, part);
}

/* ------------------------------------------------------------------ */
/* launches, and the kernels of an iteration (cg_body.h)                */
/* ------------------------------------------------------------------ */

/* one solve as its launches see it: the sizes, the caller's vectors and the
 * work buffer cut up (cg_solve() below) */
struct cg_run {
    int k, M, nwg;
    double tol2;
    cg_state *st;
    const double *minv; /* NULL: plain */
    double *X;
    int64_t ldx;
    double *part0, *part1, *part2; /* part2: preconditioned only */
    double *R, *P, *Q;
    hipStream_t s;
    const cg_plans *plans; /* spmv_*_pcg_trsv only, with Z and err */
    double *Z;
    int *err; /* the first refusal of a plan solve */
};

#define CG_PRE 0
#include "cg_body.h"
#undef CG_PRE
#define CG_PRE 1
#include "cg_body.h"
#undef CG_PRE

/*
 * spmv_*_pcg_trsv: the preconditioned recurrence with Z = z(R) STORED and made
 * by the plans (cg_plans, hip_common.h).  No kernel of its own: the plain
 * update and direction kernels (Z where k_cg_dir has R), k_cg_dot for R.Z in
 * the dot order, and the finalising kernels of the preconditioned pass, which
 * read only partial sums and the state.  Z is made for all k columns; a frozen
 * column's Z reaches nothing, since every consumer is predicated or skips it.
 */
static void pcgt_apply(const cg_run &c) {
    const cg_plans &pl = *c.plans;
    /* the one place the two stored-Z preconditioners part: the cycle of a
     * hierarchy (spmv_*_pcg_amg) or the plans' solves */
    int rc = pl.apply ? pl.apply(pl.ctx, pl.waves, c.k, c.R, c.Z, c.s)
                      : trsv_solve_dev(pl.first, pl.waves, c.k, c.R, c.k, c.Z,
                                       c.k, NULL, c.s);
    if (!rc && !pl.apply && pl.second)
        rc = trsv_solve_dev(pl.second, pl.waves, c.k, c.Z, c.k, c.Z, c.k,
                            pl.scale, c.s);
    if (rc && !*c.err)
        *c.err = rc;
    CG_LAUNCH(k_cg_dot, c.k, c.M, c.s, c.R, c.k, c.Z, c.k, c.part2);
}

/* Z = z(R), P = Z, the partials of rz; bb, rr, rz, the first classification */
static void pcgt_start(const cg_run &c) {
    pcgt_apply(c);
    CG_LAUNCH(k_cg_copy, c.k, c.M, c.s, c.Z, c.k, c.P, c.k);
    CG_FINAL(k_pcg_final_init, c.s, c.k, c.nwg, c.part0, c.part1, c.part2,
             c.tol2, c.st);
}

/* one iteration behind the partials of P.Q in part0 */
static void pcgt_iterate(const cg_run &c) {
    CG_FINAL(k_pcg_final_pq, c.s, c.k, c.nwg, c.part0, c.st);
    CG_LAUNCH(k_cg_update, c.k, c.M, c.s, c.st, c.X, c.ldx, c.P, c.R, c.Q,
              c.part1);
    pcgt_apply(c);
    CG_FINAL(k_pcg_final_rz, c.s, c.k, c.nwg, c.part1, c.part2, c.tol2, c.st);
    CG_LAUNCH(k_cg_dir, c.k, c.M, c.s, c.st, c.Z, c.P);
}

/* ------------------------------------------------------------------ */
/* host                                                                 */
/* ------------------------------------------------------------------ */

/* the two kernels every solver launches, for the other translation units
 * (hip_common.h) */
void cg_launch_copy(int k, int M, const double *src, int64_t lds, double *dst,
                    int64_t ldd, hipStream_t s) {
    CG_LAUNCH(k_cg_copy, k, M, s, src, lds, dst, ldd);
}
void cg_launch_dot(int k, int M, const double *U, int64_t ldu, const double *V,
                   int64_t ldv, double *part, hipStream_t s) {
    CG_LAUNCH(k_cg_dot, k, M, s, U, ldu, V, ldv, part);
}

int64_t cg_work_bytes(int M, int k, int pre) {
    return solver_work_bytes(cg_work(M, k, pre));
}

/* The three solvers on the loop of solver_host.h: minv == NULL is the plain
 * one, else the preconditioned one (the CG_PRE 1 pass of cg_body.h, a third
 * set of partial sums); plans != NULL (and minv NULL) is the one
 * preconditioned by triangular plans (pcgt_* above, and a stored Z).  The
 * arguments were checked by the caller (engine.hip, cg / cg_trsv): k in 1..8,
 * ldb, ldx >= k, M == N > 0, tol >= 0, maxit >= 0, check_every > 0, live plans
 * of M rows. */
int cg_solve(const cg_matrix *A, int k, const double *B, int64_t ldb, double *X,
             int64_t ldx, const double *minv, const cg_plans *plans, double tol,
             int maxit, int check_every, void *d_work, size_t work_bytes,
             spmv_cg_info *info, hipStream_t s) {
    const int M = A->M;
    const solver_work w = cg_work(M, k, plans ? 2 : minv != NULL);
    /* the one place the solvers part: which pass of cg_body.h enqueues */
    void (*const start)(const cg_run &) =
        plans ? pcgt_start : minv ? pcg_start : cg_start;
    void (*const iterate)(const cg_run &) =
        plans ? pcgt_iterate : minv ? pcg_iterate : cg_iterate;
    int plan_rc = 0;
    cg_run c = {};
    cg_state h;
    const int rc = solver_run(
        w, maxit, check_every, d_work, work_bytes, &h, s,
        /* R = B - A X; bb, rr; P, the first classification */
        [&](void *work) {
            /* part2 and Z of a solver without them: where the next region
             * starts, and never used */
            c = cg_run{k, M, (int)cg_grid(M), tol * tol, (cg_state *)work,
                       minv, X, ldx, solver_part(work, w, 0),
                       solver_part(work, w, 1), solver_part(work, w, 2),
                       solver_vec(work, w, 0), solver_vec(work, w, 1),
                       solver_vec(work, w, 2), s, plans,
                       solver_vec(work, w, 3), &plan_rc};
            CG_LAUNCH(k_cg_copy, k, M, s, B, ldb, c.R, k);
            const int rc =
                A->axpby(A->handle, A->opts, k, -1.0, 1.0, X, ldx, c.R, k, s);
            if (rc)
                return rc;
            CG_LAUNCH(k_cg_dot, k, M, s, B, ldb, B, ldb, c.part0);
            CG_LAUNCH(k_cg_dot, k, M, s, c.R, k, c.R, k, c.part1);
            start(c);
            return plan_rc;
        },
        [&](int) {
            const int rc = A->multi(A->handle, A->opts, k, c.P, k, c.Q, k, s);
            if (rc)
                return rc;
            CG_LAUNCH(k_cg_dot, k, M, s, c.P, k, c.Q, k, c.part0);
            iterate(c);
            return plan_rc;
        },
        [] { return 0; });
    if (rc)
        return rc;
    for (int j = 0; j < k; ++j) {
        info[j].status = h.status[j];
        info[j].iterations = h.iters[j];
        info[j].rr = h.rr[j];
        info[j].bb = h.bb[j];
    }
    return 0;
}
