/*
 * cgls_kernels.hip -- CGLS for min ||A X - B||^2 + damp^2 ||X||^2 on the
 * device (spmv_*_cgls, spmv_engine.h), A rectangular (M x N) and given with
 * its transpose AT (N x M) as a second handle: k = 1..8 independent problems
 * stored interleaved (X[i * ldx + j]), both handles CSR or both column-major
 * HLL, gfx950 (wave64).  Bjorck's form: A^T A is never formed.
 *
 * TWO LENGTHS.  R, Q and B have M rows; X, P and S have N rows.  Every vector
 * kernel here takes the length of the vectors it touches and is launched over
 * that length; the one kernel that touches both (k_ls_update) runs two loops,
 * each bounded, clamped and predicated by its own length.  The two products of
 * an iteration are A's and AT's launch_multi (cg_matrix, as in
 * cg_kernels.hip), the initial residual A's launch_axpby.  The dot is the dot
 * of spmv_cg_dot_shape over the length of its operands: the tile, the halving
 * trees and the launch macros come from cg_common.h, k_cg_dot and k_cg_copy
 * from cg_kernels.hip through cg_launch_dot / cg_launch_copy.  The refusals,
 * the own work buffer and the bounded host loop are solver_run (solver_host.h);
 * the buffer, with its vectors of both lengths, is cgls_work (solver_work.h).
 *
 * ONE ITERATION, in launch order:
 *   launch_multi(A)     Q = A P
 *   k_cg_dot            partials of qq = Q . Q                       (1 M)
 *   k_ls_final_alpha    breakdown, or alpha = ss / delta, iterations += 1
 *   k_ls_update         X <- X + alpha P (N rows);  R <- R - alpha Q (M rows)
 *                                                              (3 N + 3 M)
 *   launch_multi(AT)    S = AT R
 *   k_cg_dot            partials of sn = S . S                       (1 N)
 *     DAMP: k_ls_damp   S <- S - d2 X and the partials of S . S      (3 N)
 *   k_ls_final_beta     converged, breakdown, or beta, ss
 *   k_ls_dir            P <- S + beta P;  DAMP: partials of P . P    (3 N)
 * In brackets: the vectors of 8 k M or 8 k N bytes a kernel reads and writes:
 * 4 M + 7 N without damping, 4 M + 9 N with.
 *
 * DAMP.  damp == 0 is another instantiation, not a multiplication by zero:
 * DAMP false has no d2 term anywhere (S is never rewritten, P . P is never
 * summed, delta = qq).  DAMP true: delta = rn(qq + rn(d2 * pp)), pp = P . P in
 * the dot order over N, summed where P is written.
 *
 * STATE and FROZEN COLUMNS: as in cg_kernels.hip.  ls_state is written by ONE
 * workgroup (the finalising kernels, thread 0), the vector kernels read it and
 * predicate the stores of a column that is not CG_RUNNING away; no atomics, no
 * counters, every dependence is a kernel boundary on the stream.  S and Q are
 * scratch: the products rewrite all k columns of them.
 */
#include "cg_common.h"

/* per-column state, device memory (CG_STATE_BYTES at the head of the work
 * buffer) */
struct ls_state {
    double ss[CG_MAXK];    /* s.s of the recurrence */
    double atb[CG_MAXK];   /* (A^T b).(A^T b) */
    double rr[CG_MAXK];    /* r.r, once, after the loop */
    double alpha[CG_MAXK]; /* of the iteration under way */
    double beta[CG_MAXK];
    int status[CG_MAXK];   /* spmv_cgls_info.status, or CG_RUNNING */
    int iters[CG_MAXK];    /* updates of x */
};
static_assert(sizeof(ls_state) <= CG_STATE_BYTES, "state block");

/* after S = AT R, N rows: DAMP: S <- S - d2 X;  P = S;  the partials of S . S
 * (DAMP: to part_pp too -- P . P of the first delta is the same sum); all
 * columns (nothing is frozen before the first classification) */
template <int K, bool DAMP>
__global__ void __launch_bounds__(CG_T)
k_ls_first(int N, double d2, const double *__restrict__ X, int64_t ldx,
           const double *__restrict__ S, double *__restrict__ P,
           double *__restrict__ part_ss, double *__restrict__ part_pp) {
#pragma clang fp contract(off)
    const cg_lanes<K> l;
    double acc[K];
#pragma unroll
    for (int n = 0; n < K; ++n)
        acc[n] = 0.0;
    CG_SWEEPS(base, N) {
        double sv[K], x[K];
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n] < N ? base + l.t[n] : N - 1;
            sv[n] = S[i * K + l.j[n]];
            x[n] = 0.0;
            if constexpr (DAMP)
                x[n] = X[i * ldx + l.j[n]];
        }
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n];
            double s = sv[n];
            if constexpr (DAMP) {
                const double dx = d2 * x[n];
                s = sv[n] - dx;
            }
            const double s2 = s * s;
            const double sum = acc[n] + s2;
            if (i < N) {
                P[i * K + l.j[n]] = s;
                acc[n] = sum;
            }
        }
    }
    slots_to_partial<K>(l, acc, part_ss);
    if constexpr (DAMP) {
        __syncthreads(); /* the tree's LDS is reused */
        slots_to_partial<K>(l, acc, part_pp);
    }
}

/* the running columns: X = X + alpha P over N rows, R = R - alpha Q over M
 * rows.  Launched over max(M, N); each loop is bounded by its own length */
template <int K>
__global__ void __launch_bounds__(CG_T)
k_ls_update(int L, int M, int N, const ls_state *__restrict__ st,
            double *__restrict__ X, int64_t ldx, const double *__restrict__ P,
            double *__restrict__ R, const double *__restrict__ Q) {
#pragma clang fp contract(off)
    (void)L; /* the launch macro's length: max(M, N) */
    const cg_lanes<K> l;
    bool running[K];
    cg_running<K>(st, l, running);
    double alpha[K];
#pragma unroll
    for (int n = 0; n < K; ++n)
        alpha[n] = st->alpha[l.j[n]];
    CG_SWEEPS(base, N) {
        double x[K], p[K];
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n] < N ? base + l.t[n] : N - 1;
            x[n] = X[i * ldx + l.j[n]];
            p[n] = P[i * K + l.j[n]];
        }
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n];
            const double ap = alpha[n] * p[n];
            const double xn = x[n] + ap;
            if (i < N && running[n])
                X[i * ldx + l.j[n]] = xn;
        }
    }
    CG_SWEEPS(base, M) {
        double r[K], q[K];
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n] < M ? base + l.t[n] : M - 1;
            r[n] = R[i * K + l.j[n]];
            q[n] = Q[i * K + l.j[n]];
        }
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n];
            const double aq = alpha[n] * q[n];
            const double rn = r[n] - aq;
            if (i < M && running[n])
                R[i * K + l.j[n]] = rn;
        }
    }
}

/* DAMP only, N rows: S <- S - d2 X in S's place and the partials of S . S in
 * the same pass; every column (S is scratch, the finalising kernel does not
 * look at the sums of a frozen column) */
template <int K>
__global__ void __launch_bounds__(CG_T)
k_ls_damp(int N, double d2, const double *__restrict__ X, int64_t ldx,
          double *__restrict__ S, double *__restrict__ part_ss) {
#pragma clang fp contract(off)
    const cg_lanes<K> l;
    double acc[K];
#pragma unroll
    for (int n = 0; n < K; ++n)
        acc[n] = 0.0;
    CG_SWEEPS(base, N) {
        double sv[K], x[K];
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n] < N ? base + l.t[n] : N - 1;
            sv[n] = S[i * K + l.j[n]];
            x[n] = X[i * ldx + l.j[n]];
        }
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n];
            const double dx = d2 * x[n];
            const double s = sv[n] - dx;
            const double s2 = s * s;
            const double sum = acc[n] + s2;
            if (i < N) {
                S[i * K + l.j[n]] = s;
                acc[n] = sum;
            }
        }
    }
    slots_to_partial<K>(l, acc, part_ss);
}

/* direction update of the running columns over N rows: P = S + beta P; DAMP:
 * the partials of P . P for the next delta, of every column as it stands */
template <int K, bool DAMP>
__global__ void __launch_bounds__(CG_T)
k_ls_dir(int N, const ls_state *__restrict__ st, const double *__restrict__ S,
         double *__restrict__ P, double *__restrict__ part_pp) {
#pragma clang fp contract(off)
    const cg_lanes<K> l;
    bool running[K];
    cg_running<K>(st, l, running);
    double beta[K], acc[K];
#pragma unroll
    for (int n = 0; n < K; ++n) {
        beta[n] = st->beta[l.j[n]];
        acc[n] = 0.0;
    }
    CG_SWEEPS(base, N) {
        double sv[K], p[K];
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n] < N ? base + l.t[n] : N - 1;
            sv[n] = S[i * K + l.j[n]];
            p[n] = P[i * K + l.j[n]];
        }
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n];
            const double bp = beta[n] * p[n];
            const double pn = sv[n] + bp;
            if (i < N && running[n])
                P[i * K + l.j[n]] = pn;
            if constexpr (DAMP) {
                const double p2 = pn * pn;
                const double sum = acc[n] + p2;
                if (i < N)
                    acc[n] = sum;
            }
        }
    }
    if constexpr (DAMP)
        slots_to_partial<K>(l, acc, part_pp);
}

/* ---- the finalising kernels: ONE workgroup of CG_FINAL_T threads ---- */

/* ss = S.S, atb = W.W (both over N, nwg workgroup sums): a column starts
 * broken down (a non-finite sum), converged or running */
__global__ void __launch_bounds__(CG_FINAL_T)
k_ls_final_init(int k, int nwg, const double *__restrict__ part_ss,
                const double *__restrict__ part_atb, double tol2,
                ls_state *__restrict__ st) {
#pragma clang fp contract(off)
    __shared__ double s[CG_FINAL_T];
    for (int j = 0; j < CG_MAXK; ++j) {
        double ss = 0.0, atb = 0.0;
        if (j < k) { /* uniform */
            ss = final_sum(part_ss, nwg, k, j, s);
            atb = final_sum(part_atb, nwg, k, j, s);
        }
        if (threadIdx.x == 0) {
            st->ss[j] = ss;
            st->atb[j] = atb;
            st->rr[j] = 0.0;
            st->alpha[j] = 0.0;
            st->beta[j] = 0.0;
            st->iters[j] = 0;
            st->status[j] =
                j >= k ? CG_CONVERGED
                : !(cg_finite(ss) && cg_finite(atb)) ? CG_BREAKDOWN
                : ss <= tol2 * atb ? CG_CONVERGED
                                   : CG_RUNNING;
        }
    }
}

/* qq = Q.Q over M (nwg_m sums); DAMP: pp = P.P over N (nwg_n sums), delta =
 * qq + d2 pp.  A running column breaks down, or gets its alpha = ss / delta and
 * counts the step of x that follows */
template <bool DAMP>
__global__ void __launch_bounds__(CG_FINAL_T)
k_ls_final_alpha(int k, int nwg_m, const double *__restrict__ part_qq,
                 int nwg_n, const double *__restrict__ part_pp, double d2,
                 ls_state *st) {
#pragma clang fp contract(off)
    __shared__ double s[CG_FINAL_T];
    for (int j = 0; j < k; ++j) {
        if (st->status[j] != CG_RUNNING) /* uniform */
            continue;
        double delta = final_sum(part_qq, nwg_m, k, j, s);
        if constexpr (DAMP) {
            const double pp = final_sum(part_pp, nwg_n, k, j, s);
            const double dp = d2 * pp;
            delta = delta + dp;
        }
        if (threadIdx.x == 0) {
            if (!(delta > 0.0 && cg_finite(delta))) {
                st->status[j] = CG_BREAKDOWN;
            } else {
                st->alpha[j] = st->ss[j] / delta;
                st->iters[j] += 1;
            }
        }
    }
}

/* sn = S.S over N after the step: a running column converges, breaks down, or
 * gets its beta = sn / ss and the new ss */
__global__ void __launch_bounds__(CG_FINAL_T)
k_ls_final_beta(int k, int nwg, const double *__restrict__ part_sn,
                double tol2, ls_state *st) {
#pragma clang fp contract(off)
    __shared__ double s[CG_FINAL_T];
    for (int j = 0; j < k; ++j) {
        if (st->status[j] != CG_RUNNING) /* uniform */
            continue;
        const double sn = final_sum(part_sn, nwg, k, j, s);
        if (threadIdx.x == 0) {
            if (sn <= tol2 * st->atb[j]) {
                st->status[j] = CG_CONVERGED;
                st->ss[j] = sn;
            } else if (!cg_finite(sn)) {
                st->status[j] = CG_BREAKDOWN;
            } else {
                st->beta[j] = sn / st->ss[j];
                st->ss[j] = sn;
            }
        }
    }
}

/* rr = R.R over M, once, after the loop: every column */
__global__ void __launch_bounds__(CG_FINAL_T)
k_ls_final_rr(int k, int nwg, const double *__restrict__ part_rr,
              ls_state *st) {
    __shared__ double s[CG_FINAL_T];
    for (int j = 0; j < k; ++j) {
        const double rr = final_sum(part_rr, nwg, k, j, s);
        if (threadIdx.x == 0)
            st->rr[j] = rr;
    }
}

/* ------------------------------------------------------------------ */
/* host                                                                 */
/* ------------------------------------------------------------------ */

int64_t cgls_work_bytes(int M, int N, int k) {
    return solver_work_bytes(cgls_work(M, N, k));
}

/* The arguments were checked by the caller (engine.hip, cgls): k in 1..8,
 * ldb, ldx >= k, A M x N and AT N x M with M, N > 0, damp, tol >= 0,
 * maxit >= 0, check_every > 0. */
int cgls_solve(const cg_matrix *A, const cg_matrix *AT, int k, const double *B,
               int64_t ldb, double *X, int64_t ldx, double damp, double tol,
               int maxit, int check_every, void *d_work, size_t work_bytes,
               spmv_cgls_info *info, hipStream_t s) {
    const int M = A->M, N = AT->M;
    const int L = M > N ? M : N;
    const bool damped = damp != 0.0;
    const solver_work w = cgls_work(M, N, k);
    const int nwg_m = (int)cg_grid(M), nwg_n = (int)cg_grid(N);
    const double tol2 = tol * tol;
    const double d2 = damp * damp;
    ls_state *st = NULL;
    double *part0 = NULL, *part1 = NULL, *part2 = NULL;
    double *R = NULL, *Q = NULL, *S = NULL, *P = NULL;
    ls_state h;
    const int rc = solver_run(
        w, maxit, check_every, d_work, work_bytes, &h, s,
        /* R = B - A X;  W = AT B in S's storage, atb;  S = AT R (- d2 X),
         * P = S, ss;  the first classification */
        [&](void *work) {
            st = (ls_state *)work;
            part0 = solver_part(work, w, 0);
            part1 = solver_part(work, w, 1);
            part2 = solver_part(work, w, 2);
            R = solver_vec(work, w, 0);
            Q = solver_vec(work, w, 1);
            S = solver_vec(work, w, 2);
            P = solver_vec(work, w, 3);
            cg_launch_copy(k, M, B, ldb, R, k, s);
            int rc = A->axpby(A->handle, A->opts, k, -1.0, 1.0, X, ldx, R, k, s);
            if (rc)
                return rc;
            rc = AT->multi(AT->handle, AT->opts, k, B, ldb, S, k, s);
            if (rc)
                return rc;
            cg_launch_dot(k, N, S, k, S, k, part1, s);
            rc = AT->multi(AT->handle, AT->opts, k, R, k, S, k, s);
            if (rc)
                return rc;
            CG_LAUNCH_FLAG(k_ls_first, damped, k, N, s, d2, X, ldx, S, P, part0,
                           part2);
            CG_FINAL(k_ls_final_init, s, k, nwg_n, part0, part1, tol2, st);
            return 0;
        },
        [&](int) {
            int rc = A->multi(A->handle, A->opts, k, P, k, Q, k, s);
            if (rc)
                return rc;
            cg_launch_dot(k, M, Q, k, Q, k, part0, s);
            if (damped) {
                CG_FINAL(k_ls_final_alpha<true>, s, k, nwg_m, part0, nwg_n,
                         part2, d2, st);
            } else {
                CG_FINAL(k_ls_final_alpha<false>, s, k, nwg_m, part0, nwg_n,
                         part2, d2, st);
            }
            CG_LAUNCH(k_ls_update, k, L, s, M, N, st, X, ldx, P, R, Q);
            rc = AT->multi(AT->handle, AT->opts, k, R, k, S, k, s);
            if (rc)
                return rc;
            if (damped) {
                CG_LAUNCH(k_ls_damp, k, N, s, d2, X, ldx, S, part0);
            } else {
                cg_launch_dot(k, N, S, k, S, k, part0, s);
            }
            CG_FINAL(k_ls_final_beta, s, k, nwg_n, part0, tol2, st);
            CG_LAUNCH_FLAG(k_ls_dir, damped, k, N, s, st, S, P, part2);
            return 0;
        },
        /* rr of the true residual, once */
        [&] {
            cg_launch_dot(k, M, R, k, R, k, part0, s);
            CG_FINAL(k_ls_final_rr, s, k, nwg_m, part0, st);
            return hip_errno(hipGetLastError());
        });
    if (rc)
        return rc;
    for (int j = 0; j < k; ++j) {
        info[j].status = h.status[j];
        info[j].iterations = h.iters[j];
        info[j].ss = h.ss[j];
        info[j].atb = h.atb[j];
        info[j].rr = h.rr[j];
    }
    return 0;
}
