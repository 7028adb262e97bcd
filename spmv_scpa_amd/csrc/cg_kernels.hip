/*
 * cg_kernels.hip -- conjugate gradients for A X = B on the device, plain
 * (spmv_*_cg, spmv_engine.h) and with a diagonal preconditioner (spmv_*_pcg:
 * the k_pcg_* kernels below, one host loop for both): k = 1..8 independent
 * systems stored interleaved (X[i * ldx + j]), A a CSR or column-major HLL
 * handle, gfx950 (wave64).
 *
 * The product Q = A P and the initial residual are the handle's launch_multi /
 * launch_axpby (two function pointers, cg_matrix); everything else is here:
 * the fixed-order dot, the two fused vector updates, the per-column state and
 * the bounded host loop.  Templates over the number of vectors K, as in
 * multi_kernels.hip.
 *
 * DOT ORDER, a function of M alone (CG_NWG, CG_T are constants of the
 * library, exported to the tests as spmv_cg_dot_shape):
 *   element i belongs to slot i mod (CG_NWG * CG_T); slot s is slot s % CG_T
 *   of workgroup s / CG_T.  A slot starts at 0.0 and adds rn(u_i * v_i) in
 *   increasing i.  The CG_T slots of a workgroup are combined by a halving
 *   tree, s[t] += s[t + h] for h = CG_T / 2 .. 1; the CG_NWG workgroup sums by
 *   the same tree.  Workgroups whose slots hold no element are not launched:
 *   their sum is the 0.0 the tree would have given.
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
#include "hip_common.h"

#define CG_MAXK 8
#define CG_FINAL_T 1024 /* threads of a finalising workgroup, >= CG_NWG */

/* per-column state, device memory (CG_STATE_BYTES at the head of the work
 * buffer) */
struct cg_state {
    double rr[CG_MAXK];    /* r.r of the recurrence */
    double bb[CG_MAXK];    /* b.b */
    double alpha[CG_MAXK]; /* of the iteration under way */
    double beta[CG_MAXK];
    int status[CG_MAXK];   /* spmv_cg_info.status, or CG_RUNNING */
    int iters[CG_MAXK];    /* updates of x applied */
    double rz[CG_MAXK];    /* r.z of the preconditioned recurrence (pcg_solve
                              only; behind the fields cg_solve's kernels use) */
};
static_assert(sizeof(cg_state) <= CG_STATE_BYTES, "state block");
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

/* running[n]: the column of pass n is running */
template <int K>
__device__ __forceinline__ void running_passes(const cg_state *st,
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

/* fused update of the running columns: X += alpha P, R -= alpha Q, and the
 * partials of R.R in the dot order -- one pass */
template <int K>
__global__ void __launch_bounds__(CG_T)
k_cg_update(int M, const cg_state *__restrict__ st, double *__restrict__ X,
            int64_t ldx, const double *__restrict__ P, double *__restrict__ R,
            const double *__restrict__ Q, double *__restrict__ part) {
#pragma clang fp contract(off)
    const cg_lanes<K> l;
    bool running[K];
    running_passes<K>(st, l, running);
    double alpha[K], acc[K];
#pragma unroll
    for (int n = 0; n < K; ++n) {
        alpha[n] = st->alpha[l.j[n]];
        acc[n] = 0.0;
    }
    CG_SWEEPS(base, M) {
        double x[K], p[K], r[K], q[K];
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n] < M ? base + l.t[n] : M - 1;
            x[n] = X[i * ldx + l.j[n]];
            p[n] = P[i * K + l.j[n]];
            r[n] = R[i * K + l.j[n]];
            q[n] = Q[i * K + l.j[n]];
        }
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n];
            const double ap = alpha[n] * p[n];
            const double aq = alpha[n] * q[n];
            const double xn = x[n] + ap;
            const double rn = r[n] - aq;
            const double r2 = rn * rn;
            const double sum = acc[n] + r2;
            if (i < M && running[n]) {
                X[i * ldx + l.j[n]] = xn;
                R[i * K + l.j[n]] = rn;
                acc[n] = sum;
            }
        }
    }
    slots_to_partial<K>(l, acc, part);
}

/* direction update of the running columns: P = R + beta P */
template <int K>
__global__ void __launch_bounds__(CG_T)
k_cg_dir(int M, const cg_state *__restrict__ st, const double *__restrict__ R,
         double *__restrict__ P) {
#pragma clang fp contract(off)
    const cg_lanes<K> l;
    bool running[K];
    running_passes<K>(st, l, running);
    double beta[K];
#pragma unroll
    for (int n = 0; n < K; ++n)
        beta[n] = st->beta[l.j[n]];
    CG_SWEEPS(base, M) {
        double p[K], r[K];
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n] < M ? base + l.t[n] : M - 1;
            p[n] = P[i * K + l.j[n]];
            r[n] = R[i * K + l.j[n]];
        }
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n];
            const double bp = beta[n] * p[n];
            if (i < M && running[n])
                P[i * K + l.j[n]] = r[n] + bp;
        }
    }
}

/* ---- the finalising kernels: ONE workgroup of CG_FINAL_T threads ---- */

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

/* bb = B.B, rr = R.R; a column starts converged, broken down (a non-finite
 * rr or bb) or running */
__global__ void __launch_bounds__(CG_FINAL_T)
k_cg_final_init(int k, int nwg, const double *__restrict__ part_bb,
                const double *__restrict__ part_rr, double tol2,
                cg_state *__restrict__ st) {
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
            st->alpha[j] = 0.0;
            st->beta[j] = 0.0;
            st->iters[j] = 0;
            st->status[j] = j >= k ? CG_CONVERGED
                            : !(cg_finite(rr) && cg_finite(bb)) ? CG_BREAKDOWN
                            : rr <= tol2 * bb ? CG_CONVERGED
                                              : CG_RUNNING;
        }
    }
}

/* pq = P.Q: a running column breaks down, or gets its alpha and counts the
 * update of x that follows */
__global__ void __launch_bounds__(CG_FINAL_T)
k_cg_final_pq(int k, int nwg, const double *__restrict__ part,
              cg_state *st) {
    __shared__ double s[CG_FINAL_T];
    for (int j = 0; j < k; ++j) {
        if (st->status[j] != CG_RUNNING) /* uniform */
            continue;
        const double pq = final_sum(part, nwg, k, j, s);
        if (threadIdx.x == 0) {
            if (!(pq > 0.0 && cg_finite(pq))) {
                st->status[j] = CG_BREAKDOWN;
            } else {
                st->alpha[j] = st->rr[j] / pq;
                st->iters[j] += 1;
            }
        }
    }
}

/* rn = R.R after the update: a running column converges, breaks down, or
 * gets its beta and the new rr */
__global__ void __launch_bounds__(CG_FINAL_T)
k_cg_final_rr(int k, int nwg, const double *__restrict__ part, double tol2,
              cg_state *st) {
    __shared__ double s[CG_FINAL_T];
    for (int j = 0; j < k; ++j) {
        if (st->status[j] != CG_RUNNING) /* uniform */
            continue;
        const double rn = final_sum(part, nwg, k, j, s);
        if (threadIdx.x == 0) {
            if (rn <= tol2 * st->bb[j]) {
                st->status[j] = CG_CONVERGED;
                st->rr[j] = rn;
            } else if (!cg_finite(rn)) {
                st->status[j] = CG_BREAKDOWN;
            } else {
                st->beta[j] = rn / st->rr[j];
                st->rr[j] = rn;
            }
        }
    }
}

/* ------------------------------------------------------------------ */
/* preconditioned CG (spmv_*_pcg): z(R) = rn(minv_i * r_i), per row      */
/* ------------------------------------------------------------------ */
/*
 * Z is never stored: the three kernels that need it recompute it from R and
 * minv[row] -- 8 M bytes per pass instead of 8 k M to write and 8 k M to read.
 * Lane (t, j) of a pass loads minv[row t]: the K lanes of a row read one
 * address, a wavefront's load covers 512 / K consecutive bytes of the lines
 * its neighbours read, and the R / P / Q / X loads keep the layout of
 * cg_lanes.  minv of all 1.0 makes z(R) = R to the bit, rz = rr, and every
 * test below the one of the plain solver.
 */

/* dst = z(src) (P = z(R)) and the partials of src . z(src), both interleaved
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

/* fused update of the running columns: X += alpha P, R -= alpha Q, and the
 * partials of R.R and of R.z(R) in the dot order -- one pass */
template <int K>
__global__ void __launch_bounds__(CG_T)
k_pcg_update(int M, const cg_state *__restrict__ st,
             const double *__restrict__ minv, double *__restrict__ X,
             int64_t ldx, const double *__restrict__ P, double *__restrict__ R,
             const double *__restrict__ Q, double *__restrict__ part_rr,
             double *__restrict__ part_rz) {
#pragma clang fp contract(off)
    const cg_lanes<K> l;
    bool running[K];
    running_passes<K>(st, l, running);
    double alpha[K], acc[K], accz[K];
#pragma unroll
    for (int n = 0; n < K; ++n) {
        alpha[n] = st->alpha[l.j[n]];
        acc[n] = 0.0;
        accz[n] = 0.0;
    }
    CG_SWEEPS(base, M) {
        double x[K], p[K], r[K], q[K], d[K];
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n] < M ? base + l.t[n] : M - 1;
            x[n] = X[i * ldx + l.j[n]];
            p[n] = P[i * K + l.j[n]];
            r[n] = R[i * K + l.j[n]];
            q[n] = Q[i * K + l.j[n]];
            d[n] = minv[i];
        }
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n];
            const double ap = alpha[n] * p[n];
            const double aq = alpha[n] * q[n];
            const double xn = x[n] + ap;
            const double rn = r[n] - aq;
            const double r2 = rn * rn;
            const double z = d[n] * rn;
            const double rz = rn * z;
            const double sum = acc[n] + r2;
            const double sumz = accz[n] + rz;
            if (i < M && running[n]) {
                X[i * ldx + l.j[n]] = xn;
                R[i * K + l.j[n]] = rn;
                acc[n] = sum;
                accz[n] = sumz;
            }
        }
    }
    slots_to_partial<K>(l, acc, part_rr);
    __syncthreads(); /* the tree's LDS is reused */
    slots_to_partial<K>(l, accz, part_rz);
}

/* direction update of the running columns: P = z(R) + beta P */
template <int K>
__global__ void __launch_bounds__(CG_T)
k_pcg_dir(int M, const cg_state *__restrict__ st,
          const double *__restrict__ minv, const double *__restrict__ R,
          double *__restrict__ P) {
#pragma clang fp contract(off)
    const cg_lanes<K> l;
    bool running[K];
    running_passes<K>(st, l, running);
    double beta[K];
#pragma unroll
    for (int n = 0; n < K; ++n)
        beta[n] = st->beta[l.j[n]];
    CG_SWEEPS(base, M) {
        double p[K], r[K], d[K];
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n] < M ? base + l.t[n] : M - 1;
            p[n] = P[i * K + l.j[n]];
            r[n] = R[i * K + l.j[n]];
            d[n] = minv[i];
        }
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n];
            const double z = d[n] * r[n];
            const double bp = beta[n] * p[n];
            if (i < M && running[n])
                P[i * K + l.j[n]] = z + bp;
        }
    }
}

/* bb = B.B, rr = R.R, rz = R.z(R); a column starts broken down (a non-finite
 * sum), converged, broken down (rz not positive) or running */
__global__ void __launch_bounds__(CG_FINAL_T)
k_pcg_final_init(int k, int nwg, const double *__restrict__ part_bb,
                 const double *__restrict__ part_rr,
                 const double *__restrict__ part_rz, double tol2,
                 cg_state *__restrict__ st) {
    __shared__ double s[CG_FINAL_T];
    for (int j = 0; j < CG_MAXK; ++j) {
        double bb = 0.0, rr = 0.0, rz = 0.0;
        if (j < k) { /* uniform */
            bb = final_sum(part_bb, nwg, k, j, s);
            rr = final_sum(part_rr, nwg, k, j, s);
            rz = final_sum(part_rz, nwg, k, j, s);
        }
        if (threadIdx.x == 0) {
            st->bb[j] = bb;
            st->rr[j] = rr;
            st->rz[j] = rz;
            st->alpha[j] = 0.0;
            st->beta[j] = 0.0;
            st->iters[j] = 0;
            st->status[j] =
                j >= k ? CG_CONVERGED
                : !(cg_finite(rr) && cg_finite(bb) && cg_finite(rz))
                    ? CG_BREAKDOWN
                : rr <= tol2 * bb ? CG_CONVERGED
                : !(rz > 0.0)     ? CG_BREAKDOWN
                                  : CG_RUNNING;
        }
    }
}

/* pq = P.Q: a running column breaks down, or gets alpha = rz / pq and counts
 * the update of x that follows */
__global__ void __launch_bounds__(CG_FINAL_T)
k_pcg_final_pq(int k, int nwg, const double *__restrict__ part,
               cg_state *st) {
    __shared__ double s[CG_FINAL_T];
    for (int j = 0; j < k; ++j) {
        if (st->status[j] != CG_RUNNING) /* uniform */
            continue;
        const double pq = final_sum(part, nwg, k, j, s);
        if (threadIdx.x == 0) {
            if (!(pq > 0.0 && cg_finite(pq))) {
                st->status[j] = CG_BREAKDOWN;
            } else {
                st->alpha[j] = st->rz[j] / pq;
                st->iters[j] += 1;
            }
        }
    }
}

/* rn = R.R, zn = R.z(R) after the update: a running column converges, breaks
 * down, or gets beta = zn / rz and the new rr, rz */
__global__ void __launch_bounds__(CG_FINAL_T)
k_pcg_final_rz(int k, int nwg, const double *__restrict__ part_rr,
               const double *__restrict__ part_rz, double tol2, cg_state *st) {
    __shared__ double s[CG_FINAL_T];
    for (int j = 0; j < k; ++j) {
        if (st->status[j] != CG_RUNNING) /* uniform */
            continue;
        const double rn = final_sum(part_rr, nwg, k, j, s);
        const double zn = final_sum(part_rz, nwg, k, j, s);
        if (threadIdx.x == 0) {
            if (rn <= tol2 * st->bb[j]) {
                st->status[j] = CG_CONVERGED;
                st->rr[j] = rn;
            } else if (!cg_finite(rn) || !(zn > 0.0 && cg_finite(zn))) {
                st->status[j] = CG_BREAKDOWN;
            } else {
                st->beta[j] = zn / st->rz[j];
                st->rr[j] = rn;
                st->rz[j] = zn;
            }
        }
    }
}

/* ------------------------------------------------------------------ */
/* host                                                                 */
/* ------------------------------------------------------------------ */

/* state, the sets of partial sums, R, P, Q */
static int64_t work_bytes_of(int M, int k, int parts) {
    if (M < 0 || k < 1 || k > CG_MAXK)
        return -EINVAL;
    return CG_STATE_BYTES + parts * CG_PART_BYTES + 3 * 8 * (int64_t)M * k;
}
int64_t cg_work_bytes(int M, int k) { return work_bytes_of(M, k, 2); }
/* pq, and rn and zn, which are live together */
int64_t pcg_work_bytes(int M, int k) { return work_bytes_of(M, k, 3); }

/* workgroups whose slots hold an element */
static unsigned cg_grid(int M) {
    const int64_t g = ((int64_t)M + CG_T - 1) / CG_T;
    return (unsigned)(g < CG_NWG ? g : CG_NWG);
}

#define CG_K_SWITCH(k, CALL)                                                  \
    switch (k) {                                                              \
    case 1: CALL(1); break;                                                   \
    case 2: CALL(2); break;                                                   \
    case 3: CALL(3); break;                                                   \
    case 4: CALL(4); break;                                                   \
    case 5: CALL(5); break;                                                   \
    case 6: CALL(6); break;                                                   \
    case 7: CALL(7); break;                                                   \
    default: CALL(8); break;                                                  \
    }

static void cg_copy(int k, int M, const double *src, int64_t lds, double *dst,
                    int64_t ldd, hipStream_t s) {
#define CALL(KK)                                                              \
    hipLaunchKernelGGL((k_cg_copy<KK>), dim3(cg_grid(M)), dim3(CG_T), 0, s, M, \
                       src, lds, dst, ldd)
    CG_K_SWITCH(k, CALL)
#undef CALL
}

static void cg_dot(int k, int M, const double *U, int64_t ldu, const double *V,
                   int64_t ldv, double *part, hipStream_t s) {
#define CALL(KK)                                                              \
    hipLaunchKernelGGL((k_cg_dot<KK>), dim3(cg_grid(M)), dim3(CG_T), 0, s, M,  \
                       U, ldu, V, ldv, part)
    CG_K_SWITCH(k, CALL)
#undef CALL
}

static void cg_update(int k, int M, const cg_state *st, double *X, int64_t ldx,
                      const double *P, double *R, const double *Q,
                      double *part, hipStream_t s) {
#define CALL(KK)                                                              \
    hipLaunchKernelGGL((k_cg_update<KK>), dim3(cg_grid(M)), dim3(CG_T), 0, s,  \
                       M, st, X, ldx, P, R, Q, part)
    CG_K_SWITCH(k, CALL)
#undef CALL
}

static void cg_dir(int k, int M, const cg_state *st, const double *R, double *P,
                   hipStream_t s) {
#define CALL(KK)                                                              \
    hipLaunchKernelGGL((k_cg_dir<KK>), dim3(cg_grid(M)), dim3(CG_T), 0, s, M,  \
                       st, R, P)
    CG_K_SWITCH(k, CALL)
#undef CALL
}

static void pcg_first(int k, int M, const double *minv, const double *R,
                      double *P, double *part, hipStream_t s) {
#define CALL(KK)                                                              \
    hipLaunchKernelGGL((k_pcg_first<KK>), dim3(cg_grid(M)), dim3(CG_T), 0, s,  \
                       M, minv, R, P, part)
    CG_K_SWITCH(k, CALL)
#undef CALL
}

static void pcg_update(int k, int M, const cg_state *st, const double *minv,
                       double *X, int64_t ldx, const double *P, double *R,
                       const double *Q, double *part_rr, double *part_rz,
                       hipStream_t s) {
#define CALL(KK)                                                              \
    hipLaunchKernelGGL((k_pcg_update<KK>), dim3(cg_grid(M)), dim3(CG_T), 0, s, \
                       M, st, minv, X, ldx, P, R, Q, part_rr, part_rz)
    CG_K_SWITCH(k, CALL)
#undef CALL
}

static void pcg_dir(int k, int M, const cg_state *st, const double *minv,
                    const double *R, double *P, hipStream_t s) {
#define CALL(KK)                                                              \
    hipLaunchKernelGGL((k_pcg_dir<KK>), dim3(cg_grid(M)), dim3(CG_T), 0, s, M, \
                       st, minv, R, P)
    CG_K_SWITCH(k, CALL)
#undef CALL
}

/* The host loop of both solvers: minv == NULL is the plain one, else the
 * preconditioned one (its kernels, a third set of partial sums).  The
 * arguments were checked by the caller (engine.hip, cg / pcg): k in 1..8,
 * ldb, ldx >= k, M == N > 0, tol >= 0, maxit >= 0, check_every > 0. */
static int solve(const cg_matrix *A, int k, const double *B, int64_t ldb,
                 double *X, int64_t ldx, const double *minv, double tol,
                 int maxit, int check_every, void *d_work, size_t work_bytes,
                 spmv_cg_info *info, hipStream_t s) {
    const int M = A->M;
    const size_t need =
        (size_t)(minv ? pcg_work_bytes(M, k) : cg_work_bytes(M, k));
    if (d_work && (work_bytes < need || ((uintptr_t)d_work & 7)))
        return -EINVAL;
    /* a capturing stream cannot be synchronised: refuse before anything is
     * allocated or enqueued, so the capture stays valid */
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    const hipError_t ce = hipStreamIsCapturing(s, &cap);
    if (ce != hipSuccess) {
        (void)hipGetLastError();
        return ce == hipErrorStreamCaptureImplicit ? -EBUSY : hip_errno(ce);
    }
    if (cap != hipStreamCaptureStatusNone)
        return -EBUSY;

    int rc = 0;
    void *own = NULL;
    cg_state h_st;
    int h_status[CG_MAXK];
    (void)hipGetLastError(); /* an earlier caller's unread error is not ours */
    if (!d_work) {
        HIP_TRY(hipMalloc(&own, need));
        d_work = own;
    }
    {
        cg_state *st = (cg_state *)d_work;
        double *part0 = (double *)((char *)d_work + CG_STATE_BYTES);
        double *part1 = part0 + CG_PART_BYTES / 8;
        double *part2 = part1 + CG_PART_BYTES / 8; /* preconditioned only */
        double *R = minv ? part2 + CG_PART_BYTES / 8 : part2;
        double *P = R + (size_t)M * k;
        double *Q = P + (size_t)M * k;
        const int nwg = (int)cg_grid(M);
        const double tol2 = tol * tol;

        /* R = B - A X; P = R or z(R); bb, rr (, rz) and the first
         * classification */
        cg_copy(k, M, B, ldb, R, k, s);
        rc = A->axpby(A->handle, A->opts, k, -1.0, 1.0, X, ldx, R, k, s);
        if (rc)
            goto fail;
        cg_dot(k, M, B, ldb, B, ldb, part0, s);
        cg_dot(k, M, R, k, R, k, part1, s);
        if (minv) {
            pcg_first(k, M, minv, R, P, part2, s);
            hipLaunchKernelGGL(k_pcg_final_init, dim3(1), dim3(CG_FINAL_T), 0,
                               s, k, nwg, part0, part1, part2, tol2, st);
        } else {
            cg_copy(k, M, R, k, P, k, s);
            hipLaunchKernelGGL(k_cg_final_init, dim3(1), dim3(CG_FINAL_T), 0,
                               s, k, nwg, part0, part1, tol2, st);
        }
        HIP_TRY(hipGetLastError());

        for (int done = 0;;) {
            HIP_TRY(hipMemcpyAsync(h_status, st->status, k * sizeof(int),
                                   hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            bool running = false;
            for (int j = 0; j < k; ++j)
                running = running || h_status[j] == CG_RUNNING;
            if (!running || done >= maxit)
                break;
            const int batch = maxit - done < check_every ? maxit - done
                                                         : check_every;
            for (int it = 0; it < batch; ++it) {
                rc = A->multi(A->handle, A->opts, k, P, k, Q, k, s);
                if (rc)
                    goto fail;
                cg_dot(k, M, P, k, Q, k, part0, s);
                if (minv) {
                    hipLaunchKernelGGL(k_pcg_final_pq, dim3(1),
                                       dim3(CG_FINAL_T), 0, s, k, nwg, part0,
                                       st);
                    pcg_update(k, M, st, minv, X, ldx, P, R, Q, part1, part2,
                               s);
                    hipLaunchKernelGGL(k_pcg_final_rz, dim3(1),
                                       dim3(CG_FINAL_T), 0, s, k, nwg, part1,
                                       part2, tol2, st);
                    pcg_dir(k, M, st, minv, R, P, s);
                } else {
                    hipLaunchKernelGGL(k_cg_final_pq, dim3(1),
                                       dim3(CG_FINAL_T), 0, s, k, nwg, part0,
                                       st);
                    cg_update(k, M, st, X, ldx, P, R, Q, part1, s);
                    hipLaunchKernelGGL(k_cg_final_rr, dim3(1),
                                       dim3(CG_FINAL_T), 0, s, k, nwg, part1,
                                       tol2, st);
                    cg_dir(k, M, st, R, P, s);
                }
            }
            HIP_TRY(hipGetLastError());
            done += batch;
        }
        HIP_TRY(hipMemcpyAsync(&h_st, st, sizeof h_st, hipMemcpyDeviceToHost,
                               s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    for (int j = 0; j < k; ++j) {
        info[j].status =
            h_st.status[j] == CG_RUNNING ? CG_MAXIT : h_st.status[j];
        info[j].iterations = h_st.iters[j];
        info[j].rr = h_st.rr[j];
        info[j].bb = h_st.bb[j];
    }
    if (own)
        rc = hip_errno(hipFree(own));
    return rc;
fail:
    /* nothing of ours may still run when the work buffer goes */
    (void)hipStreamSynchronize(s);
    if (own)
        (void)hipFree(own);
    (void)hipGetLastError();
    return rc;
}

int cg_solve(const cg_matrix *A, int k, const double *B, int64_t ldb, double *X,
             int64_t ldx, double tol, int maxit, int check_every, void *d_work,
             size_t work_bytes, spmv_cg_info *info, hipStream_t s) {
    return solve(A, k, B, ldb, X, ldx, NULL, tol, maxit, check_every, d_work,
                 work_bytes, info, s);
}

/* ... and minv != NULL */
int pcg_solve(const cg_matrix *A, int k, const double *B, int64_t ldb,
              double *X, int64_t ldx, const double *minv, double tol, int maxit,
              int check_every, void *d_work, size_t work_bytes,
              spmv_cg_info *info, hipStream_t s) {
    return solve(A, k, B, ldb, X, ldx, minv, tol, maxit, check_every, d_work,
                 work_bytes, info, s);
}
