/*
 * minres_kernels.hip -- MINRES for A X = B on the device (spmv_*_minres,
 * spmv_engine.h), A square and symmetric, definite or not, with an optional
 * positive diagonal preconditioner: k = 1..8 independent systems stored
 * interleaved (X[i * ldx + j]), A a CSR or column-major HLL handle, gfx950
 * (wave64).
 *
 * The one product of an iteration, the initial and the final residual are the
 * handle's launch_multi / launch_axpby (cg_matrix, as in cg_kernels.hip).  The
 * dot is the dot of spmv_cg_dot_shape: the tile, the halving trees and the
 * launch macros come from cg_common.h, k_cg_dot and k_cg_copy from
 * cg_kernels.hip through cg_launch_dot / cg_launch_copy.  Here: the Lanczos
 * recurrence and the Givens rotations of Paige and Saunders as four vector
 * kernels and four finalising kernels, the per-column state, the device
 * square root and the launches of a solve in their order; the refusals, the
 * own work buffer and the bounded host loop are solver_run (solver_host.h), the
 * buffer is minres_work (solver_work.h).
 *
 * ONE ITERATION i = 1, 2, ..., in launch order:
 *   k_mr_v             V = s z(R2), s = 1 / beta                    (2 + d)
 *   launch_multi       Q = A V
 *   k_mr_orth          i >= 2: Q <- Q - (beta / oldb) R1;
 *                      partials of alfa = V . Q            (4; i == 1: 2)
 *   k_mr_final_alfa    breakdown, or alfa / beta
 *   k_mr_res           Rn = Q - (alfa / beta) R2 in R1's place;
 *                      partials of bnew = Rn . z(Rn)                (3 + d)
 *   k_mr_final_givens  breakdown, or the rotation: oldeps, delta, gamma, phi,
 *                      iterations += 1, pp, converged; s and beta / oldb of
 *                      the next iteration
 *   k_mr_step          Wn = ((V - oldeps W1) - delta W2) / gamma in W1's
 *                      place;  X <- X + phi Wn                      (6)
 * In brackets: the vectors of 8 k M bytes a kernel reads and writes, d = the
 * 8 M bytes of minv: 15 vector passes an iteration.  The two residuals and the
 * two directions live in two pairs of buffers; the new member of a pair is
 * written over its oldest, and the host swaps the roles by the parity of i,
 * which all columns share: nothing is copied.
 *
 * PRE.  k_mr_v and k_mr_res are templates over <K, PRE>: PRE false has no minv
 * argument to read and z(u) = u; PRE true forms rn(minv_i * u).
 * rn(1.0 * u) is u, so minv of all 1.0 gives the bits of minv == NULL.
 * FIRST.  k_mr_orth<K, true> is iteration 1: it has no R1 term at all.
 *
 * STATE and FROZEN COLUMNS: as in cg_kernels.hip.  mr_state is written by ONE
 * workgroup (the finalising kernels, thread 0), the vector kernels read it and
 * predicate the stores of a column that is not CG_RUNNING away.  The update of
 * X belongs to the iteration in which a column converges, so k_mr_step goes by
 * `upd`, which k_mr_final_givens sets for the columns that were running and
 * got their rotation, and clears for every other one.  No atomics, no
 * counters, every dependence is a kernel boundary on the stream.
 */
#include "cg_common.h"

/* per-column state, device memory (MR_STATE_BYTES, solver_work.h, at the head
 * of the work buffer) */
struct mr_state {
    double bb[CG_MAXK];     /* b.b */
    double bn2[CG_MAXK];    /* b.z(b) */
    double pp[CG_MAXK];     /* phibar * phibar */
    double rr[CG_MAXK];     /* the true r.r, once, at the end */
    double beta[CG_MAXK];   /* the Lanczos and Givens scalars of the contract */
    double oldb[CG_MAXK];
    double phibar[CG_MAXK];
    double dbar[CG_MAXK];
    double epsln[CG_MAXK];
    double cs[CG_MAXK];
    double sn[CG_MAXK];
    double alfa[CG_MAXK];
    double s[CG_MAXK];      /* 1 / beta: k_mr_v */
    double c1[CG_MAXK];     /* beta / oldb: k_mr_orth */
    double c2[CG_MAXK];     /* alfa / beta: k_mr_res */
    double oldeps[CG_MAXK]; /* k_mr_step */
    double delta[CG_MAXK];
    double gamma[CG_MAXK];
    double phi[CG_MAXK];
    int status[CG_MAXK];    /* spmv_minres_info.status, or CG_RUNNING */
    int iters[CG_MAXK];     /* updates of x applied */
    int upd[CG_MAXK];       /* k_mr_step of this iteration applies */
};
static_assert(sizeof(mr_state) <= MR_STATE_BYTES, "state block");

/* z(u) of one element: rn(minv_i * u), or u itself */
template <bool PRE>
__device__ __forceinline__ double mr_z(double d, double u) {
#pragma clang fp contract(off)
    if constexpr (PRE)
        return d * u;
    else
        return u;
}

/* the partials of U . z(U) in the dot order with a minv, every column (B with
 * its stride and the first residual, before anything is classified; without
 * minv that is k_cg_dot of U with itself) */
template <int K>
__global__ void __launch_bounds__(CG_T)
k_mr_dotz(int M, const double *__restrict__ minv, const double *__restrict__ U,
          int64_t ldu, double *__restrict__ part) {
#pragma clang fp contract(off)
    const cg_lanes<K> l;
    double acc[K];
#pragma unroll
    for (int n = 0; n < K; ++n)
        acc[n] = 0.0;
    CG_SWEEPS(base, M) {
        double u[K], d[K];
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n] < M ? base + l.t[n] : M - 1;
            u[n] = U[i * ldu + l.j[n]];
            d[n] = minv[i];
        }
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const double z = mr_z<true>(d[n], u[n]);
            const double uz = u[n] * z;
            const double sum = acc[n] + uz;
            if (base + l.t[n] < M)
                acc[n] = sum;
        }
    }
    slots_to_partial<K>(l, acc, part);
}

/* the running columns: V = s z(R2) */
template <int K, bool PRE>
__global__ void __launch_bounds__(CG_T)
k_mr_v(int M, const mr_state *__restrict__ st, const double *__restrict__ minv,
       const double *__restrict__ R2, double *__restrict__ V) {
#pragma clang fp contract(off)
    const cg_lanes<K> l;
    bool running[K];
    double s[K];
#pragma unroll
    for (int n = 0; n < K; ++n) {
        running[n] = st->status[l.j[n]] == CG_RUNNING;
        s[n] = st->s[l.j[n]];
    }
    CG_SWEEPS(base, M) {
        double r[K], d[K];
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n] < M ? base + l.t[n] : M - 1;
            r[n] = R2[i * K + l.j[n]];
            d[n] = 0.0;
            if constexpr (PRE)
                d[n] = minv[i];
        }
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n];
            const double z = mr_z<PRE>(d[n], r[n]);
            const double v = s[n] * z;
            if (i < M && running[n])
                V[i * K + l.j[n]] = v;
        }
    }
}

/* the running columns: Q = Q - c1 R1 (FIRST: no such term, Q is not written);
 * the partials of V . Q in the dot order, every column (the finalising kernel
 * does not look at the sums of a frozen one) */
template <int K, bool FIRST>
__global__ void __launch_bounds__(CG_T)
k_mr_orth(int M, const mr_state *__restrict__ st, const double *__restrict__ V,
          const double *__restrict__ R1, double *__restrict__ Q,
          double *__restrict__ part) {
#pragma clang fp contract(off)
    const cg_lanes<K> l;
    bool running[K];
    double c1[K], acc[K];
#pragma unroll
    for (int n = 0; n < K; ++n) {
        running[n] = st->status[l.j[n]] == CG_RUNNING;
        c1[n] = st->c1[l.j[n]];
        acc[n] = 0.0;
    }
    CG_SWEEPS(base, M) {
        double v[K], q[K], r[K];
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n] < M ? base + l.t[n] : M - 1;
            v[n] = V[i * K + l.j[n]];
            q[n] = Q[i * K + l.j[n]];
            r[n] = 0.0;
            if constexpr (!FIRST)
                r[n] = R1[i * K + l.j[n]];
        }
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n];
            double qn = q[n];
            if constexpr (!FIRST) {
                const double cr = c1[n] * r[n];
                qn = q[n] - cr;
                if (i < M && running[n])
                    Q[i * K + l.j[n]] = qn;
            }
            const double vq = v[n] * qn;
            const double sum = acc[n] + vq;
            if (i < M)
                acc[n] = sum;
        }
    }
    slots_to_partial<K>(l, acc, part);
}

/* the running columns: Rn = Q - c2 R2, written over R1; the partials of
 * Rn . z(Rn) in the dot order */
template <int K, bool PRE>
__global__ void __launch_bounds__(CG_T)
k_mr_res(int M, const mr_state *__restrict__ st,
         const double *__restrict__ minv, const double *__restrict__ Q,
         const double *__restrict__ R2, double *__restrict__ Rn,
         double *__restrict__ part) {
#pragma clang fp contract(off)
    const cg_lanes<K> l;
    bool running[K];
    double c2[K], acc[K];
#pragma unroll
    for (int n = 0; n < K; ++n) {
        running[n] = st->status[l.j[n]] == CG_RUNNING;
        c2[n] = st->c2[l.j[n]];
        acc[n] = 0.0;
    }
    CG_SWEEPS(base, M) {
        double q[K], r[K], d[K];
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n] < M ? base + l.t[n] : M - 1;
            q[n] = Q[i * K + l.j[n]];
            r[n] = R2[i * K + l.j[n]];
            d[n] = 0.0;
            if constexpr (PRE)
                d[n] = minv[i];
        }
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n];
            const double cr = c2[n] * r[n];
            const double rn = q[n] - cr;
            const double z = mr_z<PRE>(d[n], rn);
            const double rz = rn * z;
            const double sum = acc[n] + rz;
            if (i < M && running[n]) {
                Rn[i * K + l.j[n]] = rn;
                acc[n] = sum;
            }
        }
    }
    slots_to_partial<K>(l, acc, part);
}

/* the columns with `upd`: Wn = ((V - oldeps W1) - delta W2) / gamma, written
 * over W1 (W1n), and X = X + phi Wn */
template <int K>
__global__ void __launch_bounds__(CG_T)
k_mr_step(int M, const mr_state *__restrict__ st, const double *__restrict__ V,
          double *__restrict__ W1n, const double *__restrict__ W2,
          double *__restrict__ X, int64_t ldx) {
#pragma clang fp contract(off)
    const cg_lanes<K> l;
    bool upd[K];
    double oldeps[K], delta[K], gamma[K], phi[K];
#pragma unroll
    for (int n = 0; n < K; ++n) {
        upd[n] = st->upd[l.j[n]] != 0;
        oldeps[n] = st->oldeps[l.j[n]];
        delta[n] = st->delta[l.j[n]];
        gamma[n] = st->gamma[l.j[n]];
        phi[n] = st->phi[l.j[n]];
    }
    CG_SWEEPS(base, M) {
        double v[K], w1[K], w2[K], x[K];
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n] < M ? base + l.t[n] : M - 1;
            v[n] = V[i * K + l.j[n]];
            w1[n] = W1n[i * K + l.j[n]];
            w2[n] = W2[i * K + l.j[n]];
            x[n] = X[i * ldx + l.j[n]];
        }
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n];
            const double e1 = oldeps[n] * w1[n];
            const double a = v[n] - e1;
            const double d2 = delta[n] * w2[n];
            const double b = a - d2;
            const double wn = b / gamma[n];
            const double pw = phi[n] * wn;
            const double xn = x[n] + pw;
            if (i < M && upd[n]) {
                W1n[i * K + l.j[n]] = wn;
                X[i * ldx + l.j[n]] = xn;
            }
        }
    }
}

/* ---- the finalising kernels: ONE workgroup of CG_FINAL_T threads ---- */

/* bb = B.B, bn2 = B.z(B), b1 = R2.z(R2): a column starts broken down,
 * converged or running with beta = sqrt(b1) */
__global__ void __launch_bounds__(CG_FINAL_T)
k_mr_final_init(int k, int nwg, const double *__restrict__ part_bb,
                const double *__restrict__ part_bn2,
                const double *__restrict__ part_b1, double tol2,
                mr_state *__restrict__ st) {
#pragma clang fp contract(off)
    __shared__ double s[CG_FINAL_T];
    for (int j = 0; j < CG_MAXK; ++j) {
        double bb = 0.0, bn2 = 0.0, b1 = 0.0;
        if (j < k) { /* uniform */
            bb = final_sum(part_bb, nwg, k, j, s);
            bn2 = final_sum(part_bn2, nwg, k, j, s);
            b1 = final_sum(part_b1, nwg, k, j, s);
        }
        if (threadIdx.x == 0) {
            const int status =
                j >= k ? CG_CONVERGED
                : !(b1 >= 0.0 && cg_finite(b1)) ||
                        !(bn2 >= 0.0 && cg_finite(bn2))
                    ? CG_BREAKDOWN
                : b1 <= tol2 * bn2 ? CG_CONVERGED
                                   : CG_RUNNING;
            const double beta = status == CG_RUNNING ? mr_sqrt(b1) : 0.0;
            st->bb[j] = bb;
            st->bn2[j] = bn2;
            st->pp[j] = b1;
            st->rr[j] = 0.0;
            st->beta[j] = beta;
            st->oldb[j] = 0.0;
            st->phibar[j] = beta;
            st->dbar[j] = 0.0;
            st->epsln[j] = 0.0;
            st->cs[j] = -1.0;
            st->sn[j] = 0.0;
            st->alfa[j] = 0.0;
            st->s[j] = status == CG_RUNNING ? 1.0 / beta : 0.0;
            st->c1[j] = 0.0;
            st->c2[j] = 0.0;
            st->oldeps[j] = 0.0;
            st->delta[j] = 0.0;
            st->gamma[j] = 0.0;
            st->phi[j] = 0.0;
            st->iters[j] = 0;
            st->upd[j] = 0;
            st->status[j] = status;
        }
    }
}

/* alfa = V.Q: a running column breaks down, or gets alfa and alfa / beta */
__global__ void __launch_bounds__(CG_FINAL_T)
k_mr_final_alfa(int k, int nwg, const double *__restrict__ part, mr_state *st) {
    __shared__ double s[CG_FINAL_T];
    for (int j = 0; j < k; ++j) {
        if (st->status[j] != CG_RUNNING) /* uniform */
            continue;
        const double alfa = final_sum(part, nwg, k, j, s);
        if (threadIdx.x == 0) {
            if (!cg_finite(alfa)) {
                st->status[j] = CG_BREAKDOWN;
            } else {
                st->alfa[j] = alfa;
                st->c2[j] = alfa / st->beta[j];
            }
        }
    }
}

/* bnew = Rn.z(Rn): a running column breaks down, or gets the next beta and
 * its Givens rotation, counts the step of x that follows (upd), and converges
 * or goes on with s and beta / oldb of the next iteration */
__global__ void __launch_bounds__(CG_FINAL_T)
k_mr_final_givens(int k, int nwg, const double *__restrict__ part, double tol2,
                  mr_state *st) {
#pragma clang fp contract(off)
    __shared__ double s[CG_FINAL_T];
    for (int j = 0; j < k; ++j) {
        if (st->status[j] != CG_RUNNING) { /* uniform */
            if (threadIdx.x == 0)
                st->upd[j] = 0;
            continue;
        }
        const double bnew = final_sum(part, nwg, k, j, s);
        if (threadIdx.x == 0) {
            st->upd[j] = 0;
            if (!(bnew >= 0.0 && cg_finite(bnew))) {
                st->status[j] = CG_BREAKDOWN;
                continue;
            }
            const double oldb = st->beta[j];
            const double beta = mr_sqrt(bnew);
            const double oldeps = st->epsln[j];
            const double cs = st->cs[j], sn = st->sn[j];
            const double dbar = st->dbar[j], alfa = st->alfa[j];
            const double cd = cs * dbar;
            const double sa = sn * alfa;
            const double delta = cd + sa;
            const double sd = sn * dbar;
            const double ca = cs * alfa;
            const double gbar = sd - ca;
            const double epsln = sn * beta;
            const double cb = cs * beta;
            const double gg = gbar * gbar;
            const double b2 = beta * beta;
            const double g2 = gg + b2;
            const double gamma = mr_sqrt(g2);
            if (!(gamma > 0.0 && cg_finite(gamma))) {
                st->status[j] = CG_BREAKDOWN;
                continue;
            }
            const double csn = gbar / gamma;
            const double snn = beta / gamma;
            const double phibar = st->phibar[j];
            const double phi = csn * phibar;
            const double phibarn = snn * phibar;
            const double pp = phibarn * phibarn;
            st->oldb[j] = oldb;
            st->beta[j] = beta;
            st->epsln[j] = epsln;
            st->dbar[j] = -cb;
            st->cs[j] = csn;
            st->sn[j] = snn;
            st->phibar[j] = phibarn;
            st->oldeps[j] = oldeps;
            st->delta[j] = delta;
            st->gamma[j] = gamma;
            st->phi[j] = phi;
            st->s[j] = 1.0 / beta;
            st->c1[j] = beta / oldb;
            st->upd[j] = 1;
            st->iters[j] += 1;
            st->pp[j] = pp;
            if (pp <= tol2 * st->bn2[j])
                st->status[j] = CG_CONVERGED;
            else if (!cg_finite(pp))
                st->status[j] = CG_BREAKDOWN;
        }
    }
}

/* rr = R.R of the true residual, every column */
__global__ void __launch_bounds__(CG_FINAL_T)
k_mr_final_rr(int k, int nwg, const double *__restrict__ part,
              mr_state *__restrict__ st) {
    __shared__ double s[CG_FINAL_T];
    for (int j = 0; j < k; ++j) {
        const double rr = final_sum(part, nwg, k, j, s);
        if (threadIdx.x == 0)
            st->rr[j] = rr;
    }
}

/* TEST HOOK: out[i] = mr_sqrt(in[i]) */
__global__ void __launch_bounds__(CG_T)
k_mr_debug_sqrt(int64_t n, const double *__restrict__ in,
                double *__restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * CG_T + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * CG_T)
        out[i] = mr_sqrt(in[i]);
}

/* ------------------------------------------------------------------ */
/* host                                                                 */
/* ------------------------------------------------------------------ */

int64_t minres_work_bytes(int M, int k) {
    return solver_work_bytes(minres_work(M, k));
}

int minres_debug_sqrt(const double *d_in, double *d_out, int64_t n,
                      hipStream_t s) {
    if (n < 0 || (n > 0 && (!d_in || !d_out)))
        return -EINVAL;
    if (n == 0)
        return 0;
    const int64_t g = (n + CG_T - 1) / CG_T;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_mr_debug_sqrt, dim3((unsigned)(g < CG_NWG ? g : CG_NWG)),
                       dim3(CG_T), 0, s, n, d_in, d_out);
    return hip_errno(hipGetLastError());
}

/* The arguments were checked by the caller (engine.hip, minres): k in 1..8,
 * ldb, ldx >= k, M == N > 0, tol >= 0, maxit >= 0, check_every > 0. */
int minres_solve(const cg_matrix *A, int k, const double *B, int64_t ldb,
                 double *X, int64_t ldx, const double *minv, double tol,
                 int maxit, int check_every, void *d_work, size_t work_bytes,
                 spmv_minres_info *info, hipStream_t s) {
    const int M = A->M;
    const bool pre = minv != NULL;
    const solver_work w = minres_work(M, k);
    const int nwg = (int)cg_grid(M);
    const double tol2 = tol * tol;
    mr_state *st = NULL;
    double *part0 = NULL, *part1 = NULL, *part2 = NULL;
    /* iteration i: R2 = Rb[(i - 1) & 1], R1 and then Rn = Rb[i & 1]; the same
     * with W2, W1 and Wn in Wb */
    double *Rb[2] = {NULL, NULL}, *Wb[2] = {NULL, NULL};
    double *V = NULL, *Q = NULL;
    mr_state h;
    const int rc = solver_run(
        w, maxit, check_every, d_work, work_bytes, &h, s,
        /* R2 = B - A X; W1 = W2 = +0.0; bb, bn2, b1, the first classification
         * (without minv bn2 is bb, sum for sum) */
        [&](void *work) {
            st = (mr_state *)work;
            part0 = solver_part(work, w, 0);
            part1 = solver_part(work, w, 1);
            part2 = solver_part(work, w, 2);
            Rb[0] = solver_vec(work, w, 0);
            Rb[1] = solver_vec(work, w, 1);
            V = solver_vec(work, w, 2);
            Q = solver_vec(work, w, 3);
            Wb[0] = solver_vec(work, w, 4);
            Wb[1] = solver_vec(work, w, 5);
            cg_launch_copy(k, M, B, ldb, Rb[0], k, s);
            const int rc = A->axpby(A->handle, A->opts, k, -1.0, 1.0, X, ldx,
                                    Rb[0], k, s);
            if (rc)
                return rc;
            /* both directions: neighbours, the last two vectors */
            const hipError_t e = hipMemsetAsync(
                Wb[0], 0,
                (size_t)(solver_work_vec(w, 6) - solver_work_vec(w, 4)), s);
            if (e != hipSuccess)
                return hip_errno(e);
            cg_launch_dot(k, M, B, ldb, B, ldb, part0, s);
            if (pre) {
                CG_LAUNCH(k_mr_dotz, k, M, s, minv, B, ldb, part1);
                CG_LAUNCH(k_mr_dotz, k, M, s, minv, Rb[0], (int64_t)k, part2);
            } else {
                cg_launch_dot(k, M, Rb[0], k, Rb[0], k, part2, s);
            }
            CG_FINAL(k_mr_final_init, s, k, nwg, part0, pre ? part1 : part0,
                     part2, tol2, st);
            return 0;
        },
        [&](int i) {
            const double *R2 = Rb[(i - 1) & 1];
            double *R1 = Rb[i & 1];
            CG_LAUNCH_FLAG(k_mr_v, pre, k, M, s, st, minv, R2, V);
            const int rc = A->multi(A->handle, A->opts, k, V, k, Q, k, s);
            if (rc)
                return rc;
            CG_LAUNCH_FLAG(k_mr_orth, i == 1, k, M, s, st, V, R1, Q, part0);
            CG_FINAL(k_mr_final_alfa, s, k, nwg, part0, st);
            CG_LAUNCH_FLAG(k_mr_res, pre, k, M, s, st, minv, Q, R2, R1, part1);
            CG_FINAL(k_mr_final_givens, s, k, nwg, part1, tol2, st);
            CG_LAUNCH(k_mr_step, k, M, s, st, V, Wb[i & 1], Wb[(i - 1) & 1], X,
                      ldx);
            return 0;
        },
        /* the true residual, once: R = B - A X in a buffer no one needs now */
        [&] {
            cg_launch_copy(k, M, B, ldb, Q, k, s);
            const int rc =
                A->axpby(A->handle, A->opts, k, -1.0, 1.0, X, ldx, Q, k, s);
            if (rc)
                return rc;
            cg_launch_dot(k, M, Q, k, Q, k, part0, s);
            CG_FINAL(k_mr_final_rr, s, k, nwg, part0, st);
            return hip_errno(hipGetLastError());
        });
    if (rc)
        return rc;
    for (int j = 0; j < k; ++j) {
        info[j].status = h.status[j];
        info[j].iterations = h.iters[j];
        info[j].pp = h.pp[j];
        info[j].bn2 = h.bn2[j];
        info[j].rr = h.rr[j];
        info[j].bb = h.bb[j];
    }
    return 0;
}
