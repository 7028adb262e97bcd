/*
 * gmres_kernels.hip -- restarted GMRES(m) for A X = B on the device
 * (spmv_*_gmres, spmv_*_gmres_trsv; spmv_engine.h), A square and otherwise
 * arbitrary, with an optional right preconditioner, a diagonal or triangular
 * plans: k = 1..8 independent systems stored interleaved (X[i * ldx + j]), A a
 * CSR or column-major HLL handle, gfx950 (wave64).
 *
 * The product of a step and the residual of a cycle's start are the handle's
 * launch_multi / launch_axpby (cg_matrix, as in cg_kernels.hip).  The dot is
 * the dot of spmv_cg_dot_shape: the tile, the halving trees, the square root
 * and the launch macros come from cg_common.h, k_cg_dot and k_cg_copy from
 * cg_kernels.hip.  Here: the orthogonalisation against the basis -- a
 * multi-vector dot and a multi-vector update -- the scaling and update
 * kernels, the finalising kernels and the launches of a solve in their order.
 * The per-column dense arithmetic is gmres_small.h, the buffer is gmres_work
 * (solver_work.h), the host loop is solver_run (solver_host.h).
 *
 * ONE STEP at position p of a cycle, in launch order (V_0..V_p the basis,
 * Z = z(V_p) stands in its buffer on entry; without a preconditioner
 * launch_multi reads V_p itself):
 *   launch_multi        W = A Z
 *   k_gm_dots  x n      partials of a_i = V_i . W, GM_CHUNK vectors a launch
 *   k_gm_final_dots     the p + 1 sums, one workgroup each
 *   k_gm_orth           W <- W - a_0 V_0 - ... - a_p V_p, one launch
 *   k_gm_dots  x n      partials of c_i = V_i . W
 *   k_gm_final_dots
 *   k_gm_orth           the same with c, and the slot sums of nn = W . W
 *   k_gm_final_step     h = a + c, the rotations, the ladder (gmres_small.h)
 *   k_gm_scale          V_{p+1} = W / h_{p+1};  Z = z(V_{p+1})
 * and at p = restart - 1, instead of the scaling: the update of X
 * (k_gm_final_y, k_gm_update) and the start of the next cycle.  A step reads
 * the basis four times: (p + 1) vectors in each dot and each update.
 *
 * CHUNKS.  A thread holds K accumulators per basis vector, so one launch of
 * k_gm_dots takes GM_CHUNK(K) = min(16, 32 / K) vectors -- at most 32 doubles
 * of sums a lane -- and reads W once per chunk.  Each a_i is a dot of its own
 * in the dot order, so the chunking is not observable.  The update needs no
 * sums: one launch walks the whole basis with W in registers, four vectors of
 * loads in flight.
 *
 * STATE and FROZEN COLUMNS: as in cg_kernels.hip.  gm_state and the column
 * blocks behind it are written by the finalising kernels alone, the vector
 * kernels read them and predicate the stores of a column that is not
 * CG_RUNNING away; X is written by the update alone, for the columns
 * k_gm_final_y gave steps to apply (upd).  No atomics, no counters, no waiting
 * between workgroups: every dependence is a kernel boundary on the stream.
 */
#include "cg_common.h"

/* the head of the state, device memory: what solver_run reads back.  Behind
 * GM_HEAD_BYTES: the blocks of gmres_small.h, 8 columns */
struct gm_state {
    double rr[CG_MAXK];    /* r.r at the start of the cycle; the true one at the end */
    double est[CG_MAXK];   /* g_{p+1}^2 of the last counted step */
    double bb[CG_MAXK];    /* b.b */
    double scale[CG_MAXK]; /* the divisor of k_gm_scale: beta, or h_{p+1} */
    int status[CG_MAXK];   /* spmv_gmres_info.status, or CG_RUNNING */
    int iters[CG_MAXK];    /* counted steps */
    int restarts[CG_MAXK];
    int q[CG_MAXK];        /* counted steps of this cycle not yet in X */
    int upd[CG_MAXK];      /* steps k_gm_update applies now */
};
static_assert(sizeof(gm_state) <= GM_HEAD_BYTES, "state head");

#define GM_PART_DOUBLES (CG_PART_BYTES / 8)

__device__ __forceinline__ double *gm_tail(const gm_state *st) {
    return (double *)((char *)const_cast<gm_state *>(st) + GM_HEAD_BYTES);
}

/* PRE of the vector kernels */
#define GM_NONE 0   /* z(u) = u */
#define GM_DIAG 1   /* z(u) = rn(minv_i * u) */
#define GM_STORED 2 /* z(u) made by triangular plans between the kernels */

/* basis vectors one launch of k_gm_dots takes */
#define GM_CHUNK(K) (32 / (K) < 16 ? 32 / (K) : 16)

/* the partials of V_c . W, c < nv <= C, in the dot order: V_c starts at
 * V + c * vstride, its partials at part + c * GM_PART_DOUBLES.  Every column
 * (the finalising kernel does not look at the sums of a frozen one) */
template <int K, int C>
__global__ void __launch_bounds__(CG_T)
k_gm_dots(int M, int nv, const double *__restrict__ W,
          const double *__restrict__ V, size_t vstride,
          double *__restrict__ part) {
#pragma clang fp contract(off)
    const cg_lanes<K> l;
    double acc[C][K];
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int n = 0; n < K; ++n)
            acc[c][n] = 0.0;
    CG_SWEEPS(base, M) {
        double w[K];
        size_t at[K];
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n] < M ? base + l.t[n] : M - 1;
            at[n] = (size_t)i * K + l.j[n];
            w[n] = W[at[n]];
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            if (c < nv) { /* uniform */
                double v[K];
#pragma unroll
                for (int n = 0; n < K; ++n)
                    v[n] = V[(size_t)c * vstride + at[n]];
#pragma unroll
                for (int n = 0; n < K; ++n) {
                    const double vw = v[n] * w[n];
                    const double sum = acc[c][n] + vw;
                    if (base + l.t[n] < M)
                        acc[c][n] = sum;
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        if (c < nv) { /* uniform */
            slots_to_partial<K>(l, acc[c], part + (size_t)c * GM_PART_DOUBLES);
            __syncthreads(); /* the tree's LDS is reused */
        }
    }
}

/* the running columns: W <- W - s_0 V_0 - ... - s_{nv-1} V_{nv-1}, each
 * product and each difference rounded, in increasing i; s = the sums of pass 1
 * (a) or of pass 2 (c) in the column blocks.  NN: the partials of W . W of the
 * new W in the dot order, every column */
template <int K, bool NN>
__global__ void __launch_bounds__(CG_T)
k_gm_orth(int M, int nv, int m, int second, const gm_state *__restrict__ st,
          const double *__restrict__ V, size_t vstride, double *__restrict__ W,
          double *__restrict__ part_nn) {
#pragma clang fp contract(off)
    __shared__ double sc[GM_MAXM * K];
    const cg_lanes<K> l;
    bool running[K];
    cg_running<K>(st, l, running);
    for (int e = threadIdx.x; e < nv * K; e += CG_T) {
        const gm_col c = gm_col_at(gm_tail(st), m, e % K);
        sc[e] = second ? c.c[e / K] : c.a[e / K];
    }
    __syncthreads();
    double acc[K];
#pragma unroll
    for (int n = 0; n < K; ++n)
        acc[n] = 0.0;
    CG_SWEEPS(base, M) {
        double w[K];
        size_t at[K];
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n] < M ? base + l.t[n] : M - 1;
            at[n] = (size_t)i * K + l.j[n];
            w[n] = W[at[n]];
        }
        for (int i0 = 0; i0 < nv; i0 += 4) {
            double v[4][K];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                /* the last group reads its last vector again: never applied */
                const int i = i0 + u < nv ? i0 + u : nv - 1;
#pragma unroll
                for (int n = 0; n < K; ++n)
                    v[u][n] = V[(size_t)i * vstride + at[n]];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (i0 + u < nv) { /* uniform */
#pragma unroll
                    for (int n = 0; n < K; ++n) {
                        const double sv = sc[(i0 + u) * K + l.j[n]] * v[u][n];
                        w[n] = w[n] - sv;
                    }
                }
            }
        }
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const bool in = base + l.t[n] < M;
            if (in && running[n])
                W[at[n]] = w[n];
            if constexpr (NN) {
                const double ww = w[n] * w[n];
                const double sum = acc[n] + ww;
                if (in)
                    acc[n] = sum;
            }
        }
    }
    if constexpr (NN)
        slots_to_partial<K>(l, acc, part_nn);
}

/* the running columns: dst = src / scale (a division), and Z = z(dst) where
 * z is a multiplication; src may be dst */
template <int K, int PRE>
__global__ void __launch_bounds__(CG_T)
k_gm_scale(int M, const gm_state *__restrict__ st,
           const double *__restrict__ minv, const double *src, double *dst,
           double *__restrict__ Z) {
#pragma clang fp contract(off)
    const cg_lanes<K> l;
    bool running[K];
    cg_running<K>(st, l, running);
    double sc[K];
#pragma unroll
    for (int n = 0; n < K; ++n)
        sc[n] = st->scale[l.j[n]];
    CG_SWEEPS(base, M) {
        double u[K], d[K];
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n] < M ? base + l.t[n] : M - 1;
            u[n] = src[(size_t)i * K + l.j[n]];
            d[n] = 0.0;
            if constexpr (PRE == GM_DIAG)
                d[n] = minv[i];
        }
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n];
            const double v = u[n] / sc[n];
            const double z = d[n] * v;
            if (i < M && running[n]) {
                dst[(size_t)i * K + l.j[n]] = v;
                if constexpr (PRE == GM_DIAG)
                    Z[(size_t)i * K + l.j[n]] = z;
            }
        }
    }
}

/* the columns with steps to apply (upd > 0): U = y_0 V_0, then
 * U = U + y_i V_i for i < upd, each product and sum rounded; X = X + z(U)
 * where z is U or a multiplication, else (GM_STORED) U is stored for the
 * plans and k_gm_addx follows */
template <int K, int PRE>
__global__ void __launch_bounds__(CG_T)
k_gm_update(int M, int m, const gm_state *__restrict__ st,
            const double *__restrict__ minv, const double *__restrict__ V,
            size_t vstride, double *__restrict__ X, int64_t ldx,
            double *__restrict__ U) {
#pragma clang fp contract(off)
    __shared__ double sy[GM_MAXM * K];
    const cg_lanes<K> l;
    int nq[K], qmax = 0;
#pragma unroll
    for (int n = 0; n < K; ++n)
        nq[n] = st->upd[l.j[n]];
#pragma unroll
    for (int j = 0; j < K; ++j)
        qmax = st->upd[j] > qmax ? st->upd[j] : qmax;
    if (qmax == 0) /* uniform */
        return;
    for (int e = threadIdx.x; e < qmax * K; e += CG_T) {
        const gm_col c = gm_col_at(gm_tail(st), m, e % K);
        sy[e] = e / K < st->upd[e % K] ? c.y[e / K] : 0.0;
    }
    __syncthreads();
    CG_SWEEPS(base, M) {
        double u[K], x[K], d[K];
        size_t at[K];
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n] < M ? base + l.t[n] : M - 1;
            at[n] = (size_t)i * K + l.j[n];
            u[n] = 0.0;
            x[n] = 0.0;
            d[n] = 0.0;
            if constexpr (PRE != GM_STORED)
                x[n] = X[i * ldx + l.j[n]];
            if constexpr (PRE == GM_DIAG)
                d[n] = minv[i];
        }
        for (int i0 = 0; i0 < qmax; i0 += 4) {
            double v[4][K];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int i = i0 + s < qmax ? i0 + s : qmax - 1;
#pragma unroll
                for (int n = 0; n < K; ++n)
                    v[s][n] = V[(size_t)i * vstride + at[n]];
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) {
#pragma unroll
                for (int n = 0; n < K; ++n) {
                    const int i = i0 + s;
                    const double yv =
                        sy[(i < qmax ? i : qmax - 1) * K + l.j[n]] * v[s][n];
                    const double sum = u[n] + yv;
                    if (i < nq[n])
                        u[n] = i == 0 ? yv : sum;
                }
            }
        }
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n];
            const double z = PRE == GM_DIAG ? d[n] * u[n] : u[n];
            const double xn = x[n] + z;
            if (i < M && nq[n] > 0) {
                if constexpr (PRE == GM_STORED)
                    U[at[n]] = u[n];
                else
                    X[i * ldx + l.j[n]] = xn;
            }
        }
    }
}

/* GM_STORED, the columns with upd > 0: X = X + Z */
template <int K>
__global__ void __launch_bounds__(CG_T)
k_gm_addx(int M, const gm_state *__restrict__ st, const double *__restrict__ Z,
          double *__restrict__ X, int64_t ldx) {
#pragma clang fp contract(off)
    const cg_lanes<K> l;
    int nq[K];
#pragma unroll
    for (int n = 0; n < K; ++n)
        nq[n] = st->upd[l.j[n]];
    CG_SWEEPS(base, M) {
        double x[K], z[K];
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n] < M ? base + l.t[n] : M - 1;
            x[n] = X[i * ldx + l.j[n]];
            z[n] = Z[(size_t)i * K + l.j[n]];
        }
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n];
            const double xn = x[n] + z[n];
            if (i < M && nq[n] > 0)
                X[i * ldx + l.j[n]] = xn;
        }
    }
}

/* ---- the finalising kernels ---- */

/* The start of a cycle, ONE workgroup.  first: bb = B.B and the records of
 * every column; else only the running columns, restarts += 1.  rr = V0.V0: a
 * column breaks down (a non-finite sum), converges on the true rr, or runs
 * with beta = sqrt(rr) = g_0 = the divisor of V0 */
__global__ void __launch_bounds__(CG_FINAL_T)
k_gm_final_init(int k, int nwg, const double *__restrict__ part_bb,
                const double *__restrict__ part_rr, double tol2, int first,
                int m, gm_state *st) {
#pragma clang fp contract(off)
    __shared__ double s[CG_FINAL_T];
    for (int j = 0; j < CG_MAXK; ++j) {
        const bool look =
            j < k && (first || st->status[j] == CG_RUNNING); /* uniform */
        double bb = 0.0, rr = 0.0;
        if (look && first)
            bb = final_sum(part_bb, nwg, k, j, s);
        if (look)
            rr = final_sum(part_rr, nwg, k, j, s);
        if (threadIdx.x == 0) {
            if (first) {
                st->bb[j] = bb;
                st->rr[j] = 0.0;
                st->est[j] = 0.0;
                st->scale[j] = 0.0;
                st->iters[j] = 0;
                st->restarts[j] = 0;
                st->q[j] = 0;
                st->upd[j] = 0;
                st->status[j] = CG_CONVERGED;
            } else {
                bb = st->bb[j];
            }
            if (look) {
                if (!first)
                    st->restarts[j] += 1;
                st->rr[j] = rr;
                st->est[j] = rr;
                const int status =
                    !(cg_finite(rr) && cg_finite(bb)) ? CG_BREAKDOWN
                    : rr <= tol2 * bb                 ? CG_CONVERGED
                                                      : CG_RUNNING;
                st->status[j] = status;
                if (status == CG_RUNNING) {
                    const double beta = mr_sqrt(rr);
                    gm_col_at(gm_tail(st), m, j).g[0] = beta;
                    st->scale[j] = beta;
                }
            }
        }
    }
}

/* workgroup i: the sums of set i of the partials, for the running columns,
 * into a[i] (pass 1) or c[i] (pass 2) of the column blocks */
__global__ void __launch_bounds__(CG_FINAL_T)
k_gm_final_dots(int k, int nwg, const double *__restrict__ parts, int second,
                int m, gm_state *st) {
    __shared__ double s[CG_FINAL_T];
    const int i = blockIdx.x;
    for (int j = 0; j < k; ++j) {
        if (st->status[j] != CG_RUNNING) /* uniform */
            continue;
        const double v =
            final_sum(parts + (size_t)i * GM_PART_DOUBLES, nwg, k, j, s);
        if (threadIdx.x == 0) {
            const gm_col c = gm_col_at(gm_tail(st), m, j);
            (second ? c.c : c.a)[i] = v;
        }
    }
}

/* The end of step p, ONE workgroup: nn = W.W, then thread j does column j's
 * rotations and ladder (gm_step): breakdown, or the step counts and the
 * column converges on est or gets the divisor of V_{p+1} */
__global__ void __launch_bounds__(CG_FINAL_T)
k_gm_final_step(int k, int nwg, const double *__restrict__ part_nn, int p,
                int m, double tol2, gm_state *st) {
#pragma clang fp contract(off)
    __shared__ double s[CG_FINAL_T];
    __shared__ double snn[CG_MAXK];
    for (int j = 0; j < k; ++j) {
        if (st->status[j] != CG_RUNNING) /* uniform */
            continue;
        const double nn = final_sum(part_nn, nwg, k, j, s);
        if (threadIdx.x == 0)
            snn[j] = nn;
    }
    __syncthreads();
    const int j = threadIdx.x;
    if (j < k && st->status[j] == CG_RUNNING) {
        double est = 0.0, hn = 0.0;
        if (!gm_step(gm_col_at(gm_tail(st), m, j), m, p, snn[j], &est, &hn)) {
            st->status[j] = CG_BREAKDOWN;
        } else {
            st->iters[j] += 1;
            st->q[j] += 1;
            st->est[j] = est;
            if (est <= tol2 * st->bb[j])
                st->status[j] = CG_CONVERGED;
            else
                st->scale[j] = hn;
        }
    }
}

/* thread j: the y of column j's counted steps that are not in X yet, and upd
 * = their number for k_gm_update; q = 0: they are applied once */
__global__ void __launch_bounds__(64)
k_gm_final_y(int k, int m, gm_state *st) {
    const int j = threadIdx.x;
    if (j >= k)
        return;
    const int q = st->q[j];
    if (q > 0)
        gm_back(gm_col_at(gm_tail(st), m, j), m, q);
    st->upd[j] = q;
    st->q[j] = 0;
}

/* rr = R.R of the true residual, every column */
__global__ void __launch_bounds__(CG_FINAL_T)
k_gm_final_rr(int k, int nwg, const double *__restrict__ part,
              gm_state *__restrict__ st) {
    __shared__ double s[CG_FINAL_T];
    for (int j = 0; j < k; ++j) {
        const double rr = final_sum(part, nwg, k, j, s);
        if (threadIdx.x == 0)
            st->rr[j] = rr;
    }
}

/* ------------------------------------------------------------------ */
/* host                                                                 */
/* ------------------------------------------------------------------ */

int64_t gmres_work_bytes(int M, int k, int restart) {
    return solver_work_bytes(gmres_work(M, k, restart));
}

/* kernel<k, pre>(M, ...): the vector kernels by their PRE */
#define GM_LAUNCH_K(KK, kernel, pre, M, s, ...)                               \
    do {                                                                      \
        if ((pre) == GM_STORED)                                               \
            hipLaunchKernelGGL((kernel<KK, GM_STORED>), dim3(cg_grid(M)),     \
                               dim3(CG_T), 0, s, M, __VA_ARGS__);             \
        else if ((pre) == GM_DIAG)                                            \
            hipLaunchKernelGGL((kernel<KK, GM_DIAG>), dim3(cg_grid(M)),       \
                               dim3(CG_T), 0, s, M, __VA_ARGS__);             \
        else                                                                  \
            hipLaunchKernelGGL((kernel<KK, GM_NONE>), dim3(cg_grid(M)),       \
                               dim3(CG_T), 0, s, M, __VA_ARGS__);             \
    } while (0)
#define GM_LAUNCH(kernel, pre, k, M, s, ...)                                  \
    CG_K_SWITCH(k, GM_LAUNCH_K, kernel, pre, M, s, __VA_ARGS__)
/* k_gm_dots<k, GM_CHUNK(k)>(M, ...) */
#define GM_DOTS_K(KK, M, s, ...)                                              \
    hipLaunchKernelGGL((k_gm_dots<KK, GM_CHUNK(KK)>), dim3(cg_grid(M)),       \
                       dim3(CG_T), 0, s, M, __VA_ARGS__)
#define GM_DOTS(k, M, s, ...) CG_K_SWITCH(k, GM_DOTS_K, M, s, __VA_ARGS__)

/* The arguments were checked by the caller (engine.hip, gmres / gmres_trsv):
 * k in 1..8, ldb, ldx >= k, M == N > 0, restart in 1..GM_MAXM, tol >= 0,
 * maxit >= 0, check_every > 0, live plans of M rows.  plans != NULL (and minv
 * NULL): the stored mode. */
int gmres_solve(const cg_matrix *A, int k, const double *B, int64_t ldb,
                double *X, int64_t ldx, const double *minv,
                const cg_plans *plans, int restart, double tol, int maxit,
                int check_every, void *d_work, size_t work_bytes,
                spmv_gmres_info *info, hipStream_t s) {
    const int M = A->M, m = restart;
    const int pre = plans ? GM_STORED : minv ? GM_DIAG : GM_NONE;
    const solver_work w = gmres_work(M, k, m);
    const int nwg = (int)cg_grid(M);
    const size_t vstride = (size_t)M * k;
    const double tol2 = tol * tol;
    gm_state *st = NULL;
    double *parts = NULL, *V = NULL, *W = NULL, *Z = NULL;
    gm_state h;

    /* V0 = B - A X; rr (first: bb too); the classification; V0 /= beta and
     * Z = z(V0) for the columns that run */
    auto begin = [&](int first) {
        cg_launch_copy(k, M, B, ldb, V, k, s);
        int rc = A->axpby(A->handle, A->opts, k, -1.0, 1.0, X, ldx, V, k, s);
        if (rc)
            return rc;
        if (first)
            cg_launch_dot(k, M, B, ldb, B, ldb, parts, s);
        cg_launch_dot(k, M, V, k, V, k, parts + GM_PART_DOUBLES, s);
        CG_FINAL(k_gm_final_init, s, k, nwg, parts, parts + GM_PART_DOUBLES,
                 tol2, first, m, st);
        GM_LAUNCH(k_gm_scale, pre, k, M, s, st, minv, (const double *)V, V, Z);
        if (plans)
            rc = bi_apply(*plans, k, V, Z, s);
        return rc;
    };
    /* one Gram-Schmidt pass against V_0..V_p */
    auto pass = [&](int p, int second) {
        const int chunk = GM_CHUNK(k);
        for (int i0 = 0; i0 <= p; i0 += chunk) {
            const int nv = p + 1 - i0 < chunk ? p + 1 - i0 : chunk;
            GM_DOTS(k, M, s, nv, (const double *)W,
                    (const double *)(V + (size_t)i0 * vstride), vstride,
                    parts + (size_t)i0 * GM_PART_DOUBLES);
        }
        hipLaunchKernelGGL(k_gm_final_dots, dim3(p + 1), dim3(CG_FINAL_T), 0,
                           s, k, nwg, (const double *)parts, second, m, st);
        CG_LAUNCH_FLAG(k_gm_orth, second != 0, k, M, s, p + 1, m, second,
                       (const gm_state *)st, (const double *)V, vstride, W,
                       parts);
    };
    /* X += z(V y) for the columns with counted steps that are not in X */
    auto update = [&] {
        hipLaunchKernelGGL(k_gm_final_y, dim3(1), dim3(64), 0, s, k, m, st);
        GM_LAUNCH(k_gm_update, pre, k, M, s, m, (const gm_state *)st, minv,
                  (const double *)V, vstride, X, ldx, W);
        if (plans) {
            const int rc = bi_apply(*plans, k, W, Z, s);
            if (rc)
                return rc;
            CG_LAUNCH(k_gm_addx, k, M, s, (const gm_state *)st,
                      (const double *)Z, X, ldx);
        }
        return 0;
    };

    const int rc = solver_run(
        w, maxit, check_every, d_work, work_bytes, &h, s,
        [&](void *work) {
            st = (gm_state *)work;
            parts = solver_part(work, w, 0);
            V = solver_vec(work, w, 0);
            W = solver_vec(work, w, 1);
            Z = solver_vec(work, w, 2);
            return begin(1);
        },
        [&](int i) {
            const int p = (i - 1) % m;
            double *Vp = V + (size_t)p * vstride;
            int rc = A->multi(A->handle, A->opts, k,
                              pre == GM_NONE ? Vp : Z, k, W, k, s);
            if (rc)
                return rc;
            pass(p, 0);
            pass(p, 1);
            CG_FINAL(k_gm_final_step, s, k, nwg, (const double *)parts, p, m,
                     tol2, st);
            if (p + 1 < m) {
                GM_LAUNCH(k_gm_scale, pre, k, M, s, st, minv,
                          (const double *)W, Vp + vstride, Z);
                if (plans)
                    rc = bi_apply(*plans, k, Vp + vstride, Z, s);
                return rc;
            }
            rc = update();
            return rc ? rc : begin(0);
        },
        /* the steps of an unfinished cycle, then the true residual, once:
         * R = B - A X in a buffer no one needs now */
        [&] {
            int rc = update();
            if (rc)
                return rc;
            cg_launch_copy(k, M, B, ldb, W, k, s);
            rc = A->axpby(A->handle, A->opts, k, -1.0, 1.0, X, ldx, W, k, s);
            if (rc)
                return rc;
            cg_launch_dot(k, M, W, k, W, k, parts, s);
            CG_FINAL(k_gm_final_rr, s, k, nwg, (const double *)parts, st);
            return hip_errno(hipGetLastError());
        });
    if (rc)
        return rc;
    for (int j = 0; j < k; ++j) {
        info[j].status = h.status[j];
        info[j].iterations = h.iters[j];
        info[j].restarts = h.restarts[j];
        info[j].reserved = 0;
        info[j].rr = h.rr[j];
        info[j].est = h.est[j];
        info[j].bb = h.bb[j];
    }
    return 0;
}
