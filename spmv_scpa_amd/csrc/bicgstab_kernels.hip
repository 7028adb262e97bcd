/*
 * bicgstab_kernels.hip -- BiCGStab for A X = B on the device (spmv_*_bicgstab,
 * spmv_*_bicgstab_trsv; spmv_engine.h), A square and otherwise arbitrary, with
 * an optional right preconditioner, a diagonal or triangular plans: k = 1..8
 * independent systems stored interleaved (X[i * ldx + j]), A a CSR or column-major HLL handle, gfx950 (wave64).
 *
 * The two products of an iteration and the initial residual are the handle's
 * launch_multi / launch_axpby (cg_matrix, as in cg_kernels.hip); only A x is
 * ever asked for, never a transposed product.  The dot is the dot of
 * spmv_cg_dot_shape: the tile, the halving trees and the launch macros come
 * from cg_common.h, k_cg_dot and k_cg_copy from cg_kernels.hip through
 * cg_launch_dot / cg_launch_copy.  Here: the four vector kernels, the four
 * finalising kernels, the per-column state and the launches of a solve in
 * their order; the refusals, the own work buffer and the bounded host loop are
 * solver_run (solver_host.h), the buffer is bicgstab_work (solver_work.h).
 *
 * ONE ITERATION, in launch order (Z = z(P) stands in its buffer on entry):
 *   launch_multi        V = A Z
 *   k_cg_dot            partials of rv = Rh . V
 *   k_bi_final_alpha    breakdown, or alpha = rho / rv
 *   k_bi_s              R <- S = R - alpha V;  Z <- z(S)            (4 + d)
 *   launch_multi        T = A Z
 *   k_bi_tstt           partials of ts = T . S and tt = T . T       (2)
 *   k_bi_final_omega    breakdown, or omega, iterations += 1
 *   k_bi_update         X <- (X + alpha z(P)) + omega z(S);
 *                       R <- S - omega T; partials of R . R, Rh . R  (7 + d)
 *   k_bi_final_beta     converged, breakdown, or beta, rho, rr
 *   k_bi_dir            P <- R + beta (P - omega V);  Z <- z(P)     (5 + d)
 * In brackets: the vectors of 8 k M bytes a kernel reads and writes, d = the
 * 8 M bytes of minv; with the dot's 2 that is 20 vector passes an iteration.
 * z(.) is recomputed from minv[row] in k_bi_update (z(P), z(S)) instead of
 * being read: 8 M bytes for two streams of 8 k M.  S lives in R's storage, Z
 * and Zs share one buffer: the vector launch_multi reads.
 *
 * PRE.  Every vector kernel is a template over <K, PRE>: BI_NONE has no minv
 * argument to read and z(u) = u; BI_DIAG forms rn(minv_i * u).  rn(1.0 * u)
 * is u, so minv of all 1.0 gives the bits of minv == NULL by arithmetic.
 * BI_STORED is spmv_*_bicgstab_trsv: z(.) is made by triangular plans
 * (bi_apply: trsv_solve_dev once or twice) BEHIND the kernel that made its
 * argument -- behind k_bi_first and k_bi_dir for Zp = z(P), behind k_bi_s for
 * Zs = z(S) -- so those three write no Z at all, and k_bi_update reads Zp and Zs
 * where the other modes multiply: a plan cannot be recomputed, so the two are
 * vectors of their own, both live at the update (bicgstab_trsv_work: 7
 * vectors).  The statements of the other two modes are what they were.
 *
 * STATE and FROZEN COLUMNS: as in cg_kernels.hip.  bi_state is written by ONE
 * workgroup (the finalising kernels, thread 0), the vector kernels read it and
 * predicate the stores and sums of a column that is not CG_RUNNING away; no
 * atomics, no counters, every dependence is a kernel boundary on the stream.
 */
#include "cg_common.h"

/* per-column state, device memory (CG_STATE_BYTES at the head of the work
 * buffer) */
struct bi_state {
    double rr[CG_MAXK];    /* r.r of the recurrence */
    double bb[CG_MAXK];    /* b.b */
    double rho[CG_MAXK];   /* rh.r */
    double alpha[CG_MAXK]; /* of the iteration under way */
    double omega[CG_MAXK];
    double beta[CG_MAXK];
    int status[CG_MAXK];   /* spmv_cg_info.status, or CG_RUNNING */
    int iters[CG_MAXK];    /* full steps applied to x */
};
static_assert(sizeof(bi_state) <= CG_STATE_BYTES, "state block");

/* PRE of the vector kernels */
#define BI_NONE 0   /* z(u) = u */
#define BI_DIAG 1   /* z(u) = rn(minv_i * u), formed where it is used */
#define BI_STORED 2 /* z(u) made by triangular plans between the kernels */

/* z(u) of one element: rn(minv_i * u), or u itself */
template <int PRE>
__device__ __forceinline__ double bi_z(double d, double u) {
#pragma clang fp contract(off)
    if constexpr (PRE == BI_DIAG)
        return d * u;
    else
        return u;
}

/* Rh = R, P = R, Z = z(R), interleaved with ld = K; all columns (nothing is
 * frozen before the first classification) */
template <int K, int PRE>
__global__ void __launch_bounds__(CG_T)
k_bi_first(int M, const double *__restrict__ minv,
           const double *__restrict__ R, double *__restrict__ Rh,
           double *__restrict__ P, double *__restrict__ Z) {
#pragma clang fp contract(off)
    const cg_lanes<K> l;
    CG_SWEEPS(base, M) {
        double r[K], d[K];
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n] < M ? base + l.t[n] : M - 1;
            r[n] = R[i * K + l.j[n]];
            d[n] = 0.0;
            if constexpr (PRE == BI_DIAG)
                d[n] = minv[i];
        }
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n];
            const double z = bi_z<PRE>(d[n], r[n]);
            if (i < M) {
                Rh[i * K + l.j[n]] = r[n];
                P[i * K + l.j[n]] = r[n];
                if constexpr (PRE != BI_STORED)
                    Z[i * K + l.j[n]] = z;
            }
        }
    }
}

/* the running columns: S = R - alpha V in R's place, Z = z(S) */
template <int K, int PRE>
__global__ void __launch_bounds__(CG_T)
k_bi_s(int M, const bi_state *__restrict__ st,
       const double *__restrict__ minv, double *__restrict__ R,
       const double *__restrict__ V, double *__restrict__ Z) {
#pragma clang fp contract(off)
    const cg_lanes<K> l;
    bool running[K];
    cg_running<K>(st, l, running);
    double alpha[K];
#pragma unroll
    for (int n = 0; n < K; ++n)
        alpha[n] = st->alpha[l.j[n]];
    CG_SWEEPS(base, M) {
        double r[K], v[K], d[K];
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n] < M ? base + l.t[n] : M - 1;
            r[n] = R[i * K + l.j[n]];
            v[n] = V[i * K + l.j[n]];
            d[n] = 0.0;
            if constexpr (PRE == BI_DIAG)
                d[n] = minv[i];
        }
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n];
            const double av = alpha[n] * v[n];
            const double sn = r[n] - av;
            const double z = bi_z<PRE>(d[n], sn);
            if (i < M && running[n]) {
                R[i * K + l.j[n]] = sn;
                if constexpr (PRE != BI_STORED)
                    Z[i * K + l.j[n]] = z;
            }
        }
    }
}

/* the partials of T . S and T . T in the dot order -- one pass; every column
 * (the finalising kernel does not look at the sums of a frozen one) */
template <int K>
__global__ void __launch_bounds__(CG_T)
k_bi_tstt(int M, const double *__restrict__ T, const double *__restrict__ S,
          double *__restrict__ part_ts, double *__restrict__ part_tt) {
#pragma clang fp contract(off)
    const cg_lanes<K> l;
    double accs[K], acct[K];
#pragma unroll
    for (int n = 0; n < K; ++n) {
        accs[n] = 0.0;
        acct[n] = 0.0;
    }
    CG_SWEEPS(base, M) {
        double t[K], sv[K];
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n] < M ? base + l.t[n] : M - 1;
            t[n] = T[i * K + l.j[n]];
            sv[n] = S[i * K + l.j[n]];
        }
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const double ts = t[n] * sv[n];
            const double tt = t[n] * t[n];
            const double sums = accs[n] + ts;
            const double sumt = acct[n] + tt;
            if (base + l.t[n] < M) {
                accs[n] = sums;
                acct[n] = sumt;
            }
        }
    }
    slots_to_partial<K>(l, accs, part_ts);
    __syncthreads(); /* the tree's LDS is reused */
    slots_to_partial<K>(l, acct, part_tt);
}

/* fused update of the running columns: X = (X + alpha z(P)) + omega z(S),
 * R = S - omega T (S stands in R), and the partials of R . R and Rh . R in the
 * dot order -- one pass over five vectors and minv */
template <int K, int PRE>
__global__ void __launch_bounds__(CG_T)
k_bi_update(int M, const bi_state *__restrict__ st,
            const double *__restrict__ minv, double *__restrict__ X,
            int64_t ldx, const double *__restrict__ P, double *__restrict__ R,
            const double *__restrict__ T, const double *__restrict__ Rh,
            double *__restrict__ part_rn, double *__restrict__ part_rhon,
            const double *__restrict__ Zp, const double *__restrict__ Zs) {
#pragma clang fp contract(off)
    const cg_lanes<K> l;
    bool running[K];
    cg_running<K>(st, l, running);
    double alpha[K], omega[K], accr[K], acch[K];
#pragma unroll
    for (int n = 0; n < K; ++n) {
        alpha[n] = st->alpha[l.j[n]];
        omega[n] = st->omega[l.j[n]];
        accr[n] = 0.0;
        acch[n] = 0.0;
    }
    CG_SWEEPS(base, M) {
        double x[K], p[K], sv[K], t[K], rh[K], d[K];
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n] < M ? base + l.t[n] : M - 1;
            x[n] = X[i * ldx + l.j[n]];
            /* stored: p holds z(P) and d holds z(S) as they stand in memory;
             * P and minv are not read */
            if constexpr (PRE == BI_STORED)
                p[n] = Zp[i * K + l.j[n]];
            else
                p[n] = P[i * K + l.j[n]];
            sv[n] = R[i * K + l.j[n]];
            t[n] = T[i * K + l.j[n]];
            rh[n] = Rh[i * K + l.j[n]];
            d[n] = 0.0;
            if constexpr (PRE == BI_DIAG)
                d[n] = minv[i];
            if constexpr (PRE == BI_STORED)
                d[n] = Zs[i * K + l.j[n]];
        }
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n];
            const double zp =
                PRE == BI_STORED ? p[n] : bi_z<PRE>(d[n], p[n]);
            const double zs =
                PRE == BI_STORED ? d[n] : bi_z<PRE>(d[n], sv[n]);
            const double ap = alpha[n] * zp;
            const double x1 = x[n] + ap;
            const double os = omega[n] * zs;
            const double xn = x1 + os;
            const double ot = omega[n] * t[n];
            const double rn = sv[n] - ot;
            const double r2 = rn * rn;
            const double hr = rh[n] * rn;
            const double sumr = accr[n] + r2;
            const double sumh = acch[n] + hr;
            if (i < M && running[n]) {
                X[i * ldx + l.j[n]] = xn;
                R[i * K + l.j[n]] = rn;
                accr[n] = sumr;
                acch[n] = sumh;
            }
        }
    }
    slots_to_partial<K>(l, accr, part_rn);
    __syncthreads(); /* the tree's LDS is reused */
    slots_to_partial<K>(l, acch, part_rhon);
}

/* direction update of the running columns: P = R + beta (P - omega V), and
 * Z = z(P) for the next product */
template <int K, int PRE>
__global__ void __launch_bounds__(CG_T)
k_bi_dir(int M, const bi_state *__restrict__ st,
         const double *__restrict__ minv, const double *__restrict__ R,
         const double *__restrict__ V, double *__restrict__ P,
         double *__restrict__ Z) {
#pragma clang fp contract(off)
    const cg_lanes<K> l;
    bool running[K];
    cg_running<K>(st, l, running);
    double omega[K], beta[K];
#pragma unroll
    for (int n = 0; n < K; ++n) {
        omega[n] = st->omega[l.j[n]];
        beta[n] = st->beta[l.j[n]];
    }
    CG_SWEEPS(base, M) {
        double p[K], r[K], v[K], d[K];
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n] < M ? base + l.t[n] : M - 1;
            p[n] = P[i * K + l.j[n]];
            r[n] = R[i * K + l.j[n]];
            v[n] = V[i * K + l.j[n]];
            d[n] = 0.0;
            if constexpr (PRE == BI_DIAG)
                d[n] = minv[i];
        }
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n];
            const double ov = omega[n] * v[n];
            const double pm = p[n] - ov;
            const double bp = beta[n] * pm;
            const double pn = r[n] + bp;
            const double z = bi_z<PRE>(d[n], pn);
            if (i < M && running[n]) {
                P[i * K + l.j[n]] = pn;
                if constexpr (PRE != BI_STORED)
                    Z[i * K + l.j[n]] = z;
            }
        }
    }
}

/* ---- the finalising kernels: ONE workgroup of CG_FINAL_T threads ---- */

/* bb = B.B, rr = R.R, rho = rr; a column starts broken down (a non-finite
 * sum), converged or running */
__global__ void __launch_bounds__(CG_FINAL_T)
k_bi_final_init(int k, int nwg, const double *__restrict__ part_bb,
                const double *__restrict__ part_rr, double tol2,
                bi_state *__restrict__ st) {
    __shared__ double s[CG_FINAL_T];
    for (int j = 0; j < CG_MAXK; ++j) {
        double bb = 0.0, rr = 0.0;
        if (j < k) { /* uniform */
            bb = final_sum(part_bb, nwg, k, j, s);
            rr = final_sum(part_rr, nwg, k, j, s);
        }
        if (threadIdx.x == 0) {
            st->bb[j] = bb;
            st->rr[j] = rr;
            st->rho[j] = rr;
            st->alpha[j] = 0.0;
            st->omega[j] = 0.0;
            st->beta[j] = 0.0;
            st->iters[j] = 0;
            st->status[j] =
                j >= k ? CG_CONVERGED
                : !(cg_finite(rr) && cg_finite(bb)) ? CG_BREAKDOWN
                : rr <= tol2 * bb ? CG_CONVERGED
                                  : CG_RUNNING;
        }
    }
}

/* rv = Rh.V: a running column breaks down, or gets its alpha = rho / rv */
__global__ void __launch_bounds__(CG_FINAL_T)
k_bi_final_alpha(int k, int nwg, const double *__restrict__ part,
                 bi_state *st) {
    __shared__ double s[CG_FINAL_T];
    for (int j = 0; j < k; ++j) {
        if (st->status[j] != CG_RUNNING) /* uniform */
            continue;
        const double rv = final_sum(part, nwg, k, j, s);
        if (threadIdx.x == 0) {
            if (!(rv != 0.0 && cg_finite(rv)))
                st->status[j] = CG_BREAKDOWN;
            else
                st->alpha[j] = st->rho[j] / rv;
        }
    }
}

/* ts = T.S, tt = T.T: a running column breaks down, or gets its omega and
 * counts the step of x that follows */
__global__ void __launch_bounds__(CG_FINAL_T)
k_bi_final_omega(int k, int nwg, const double *__restrict__ part_ts,
                 const double *__restrict__ part_tt, bi_state *st) {
    __shared__ double s[CG_FINAL_T];
    for (int j = 0; j < k; ++j) {
        if (st->status[j] != CG_RUNNING) /* uniform */
            continue;
        const double ts = final_sum(part_ts, nwg, k, j, s);
        const double tt = final_sum(part_tt, nwg, k, j, s);
        if (threadIdx.x == 0) {
            if (!(cg_finite(ts) && cg_finite(tt))) {
                st->status[j] = CG_BREAKDOWN;
            } else {
                st->omega[j] = tt > 0.0 ? ts / tt : 0.0;
                st->iters[j] += 1;
            }
        }
    }
}

/* rn = R.R, rhon = Rh.R after the step: a running column converges, breaks
 * down, or gets its beta = (rhon / rho) (alpha / omega) and the new rho, rr */
__global__ void __launch_bounds__(CG_FINAL_T)
k_bi_final_beta(int k, int nwg, const double *__restrict__ part_rn,
                const double *__restrict__ part_rhon, double tol2,
                bi_state *st) {
#pragma clang fp contract(off)
    __shared__ double s[CG_FINAL_T];
    for (int j = 0; j < k; ++j) {
        if (st->status[j] != CG_RUNNING) /* uniform */
            continue;
        const double rn = final_sum(part_rn, nwg, k, j, s);
        const double rhon = final_sum(part_rhon, nwg, k, j, s);
        if (threadIdx.x == 0) {
            if (rn <= tol2 * st->bb[j]) {
                st->status[j] = CG_CONVERGED;
                st->rr[j] = rn;
            } else if (!cg_finite(rn)) {
                st->status[j] = CG_BREAKDOWN;
            } else {
                const double a = rhon / st->rho[j];
                const double b = st->alpha[j] / st->omega[j];
                st->beta[j] = a * b;
                st->rho[j] = rhon;
                st->rr[j] = rn;
            }
        }
    }
}

/* ------------------------------------------------------------------ */
/* host                                                                 */
/* ------------------------------------------------------------------ */

int64_t bicgstab_work_bytes(int M, int k, int trsv) {
    return solver_work_bytes(trsv ? bicgstab_trsv_work(M, k)
                                  : bicgstab_work(M, k));
}

/* kernel<k, pre>(M, ...): the vector kernels by their PRE */
#define BI_LAUNCH_K(KK, kernel, pre, M, s, ...)                               \
    do {                                                                      \
        if ((pre) == BI_STORED)                                               \
            hipLaunchKernelGGL((kernel<KK, BI_STORED>), dim3(cg_grid(M)),     \
                               dim3(CG_T), 0, s, M, __VA_ARGS__);             \
        else if ((pre) == BI_DIAG)                                            \
            hipLaunchKernelGGL((kernel<KK, BI_DIAG>), dim3(cg_grid(M)),       \
                               dim3(CG_T), 0, s, M, __VA_ARGS__);             \
        else                                                                  \
            hipLaunchKernelGGL((kernel<KK, BI_NONE>), dim3(cg_grid(M)),       \
                               dim3(CG_T), 0, s, M, __VA_ARGS__);             \
    } while (0)
#define BI_LAUNCH(kernel, pre, k, M, s, ...)                                  \
    CG_K_SWITCH(k, BI_LAUNCH_K, kernel, pre, M, s, __VA_ARGS__)

/* The arguments were checked by the caller (engine.hip, bicgstab /
 * bicgstab_trsv): k in 1..8, ldb, ldx >= k, M == N > 0, tol >= 0, maxit >= 0,
 * check_every > 0, live plans of M rows.  plans != NULL (and minv NULL): the
 * stored mode, Z = z(P) in Zp and z(S) in a vector Zs of its own; else Zs is
 * Zp, the one buffer launch_multi reads. */
int bicgstab_solve(const cg_matrix *A, int k, const double *B, int64_t ldb,
                   double *X, int64_t ldx, const double *minv,
                   const cg_plans *plans, double tol, int maxit,
                   int check_every, void *d_work, size_t work_bytes,
                   spmv_cg_info *info, hipStream_t s) {
    const int M = A->M;
    const int pre = plans ? BI_STORED : minv ? BI_DIAG : BI_NONE;
    const solver_work w =
        plans ? bicgstab_trsv_work(M, k) : bicgstab_work(M, k);
    const int nwg = (int)cg_grid(M);
    const double tol2 = tol * tol;
    bi_state *st = NULL;
    double *part0 = NULL, *part1 = NULL;
    double *R = NULL, *Rh = NULL, *P = NULL, *V = NULL, *T = NULL, *Zp = NULL,
           *Zs = NULL;
    bi_state h;
    const int rc = solver_run(
        w, maxit, check_every, d_work, work_bytes, &h, s,
        /* R = B - A X; Rh = P = R, Z = z(P); bb, rr, the first classification */
        [&](void *work) {
            st = (bi_state *)work;
            part0 = solver_part(work, w, 0);
            part1 = solver_part(work, w, 1);
            R = solver_vec(work, w, 0);
            Rh = solver_vec(work, w, 1);
            P = solver_vec(work, w, 2);
            V = solver_vec(work, w, 3);
            T = solver_vec(work, w, 4);
            Zp = solver_vec(work, w, 5);
            Zs = plans ? solver_vec(work, w, 6) : Zp;
            cg_launch_copy(k, M, B, ldb, R, k, s);
            int rc =
                A->axpby(A->handle, A->opts, k, -1.0, 1.0, X, ldx, R, k, s);
            if (rc)
                return rc;
            BI_LAUNCH(k_bi_first, pre, k, M, s, minv, R, Rh, P, Zp);
            if (plans) {
                rc = bi_apply(*plans, k, P, Zp, s);
                if (rc)
                    return rc;
            }
            cg_launch_dot(k, M, B, ldb, B, ldb, part0, s);
            cg_launch_dot(k, M, R, k, R, k, part1, s);
            CG_FINAL(k_bi_final_init, s, k, nwg, part0, part1, tol2, st);
            return 0;
        },
        [&](int) {
            int rc = A->multi(A->handle, A->opts, k, Zp, k, V, k, s);
            if (rc)
                return rc;
            cg_launch_dot(k, M, Rh, k, V, k, part0, s);
            CG_FINAL(k_bi_final_alpha, s, k, nwg, part0, st);
            BI_LAUNCH(k_bi_s, pre, k, M, s, st, minv, R, V, Zs);
            if (plans) {
                rc = bi_apply(*plans, k, R, Zs, s);
                if (rc)
                    return rc;
            }
            rc = A->multi(A->handle, A->opts, k, Zs, k, T, k, s);
            if (rc)
                return rc;
            CG_LAUNCH(k_bi_tstt, k, M, s, T, R, part0, part1);
            CG_FINAL(k_bi_final_omega, s, k, nwg, part0, part1, st);
            /* the stored vectors are arguments of the stored mode alone: the
             * other two never read them (there Zs IS Zp, which two restrict
             * pointers must not be) */
            BI_LAUNCH(k_bi_update, pre, k, M, s, st, minv, X, ldx, P, R, T, Rh,
                      part0, part1, plans ? Zp : (const double *)NULL,
                      plans ? Zs : (const double *)NULL);
            CG_FINAL(k_bi_final_beta, s, k, nwg, part0, part1, tol2, st);
            BI_LAUNCH(k_bi_dir, pre, k, M, s, st, minv, R, V, P, Zp);
            if (plans)
                rc = bi_apply(*plans, k, P, Zp, s);
            return rc;
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
