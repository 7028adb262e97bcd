/*
 * cg_kernels.hip -- conjugate gradients for A X = B on the device, plain
 * (spmv_*_cg, spmv_engine.h) and with a diagonal preconditioner (spmv_*_pcg):
 * k = 1..8 independent systems stored interleaved (X[i * ldx + j]), A a CSR or
 * column-major HLL handle, gfx950 (wave64).
 *
 * The product Q = A P and the initial residual are the handle's launch_multi /
 * launch_axpby (two function pointers, cg_matrix); everything else is here:
 * the fixed-order dot, the two fused vector updates, the per-column state and
 * the bounded host loop.  Templates over the number of vectors K, as in
 * multi_kernels.hip.
 *
 * The kernels both solvers launch (k_cg_copy, k_cg_dot), the one only the
 * preconditioned solver has (k_pcg_first) and the host loop are in this file.
 * The kernels of an iteration -- update, dir, final_init, final_pq, final_rr /
 * final_rz -- are in cg_body.h, written once and included twice below: the
 * k_cg_* and the k_pcg_* kernel of a pair are one text.
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
    double rz[CG_MAXK];    /* r.z of the preconditioned recurrence (CG_PRE 1
                              only; behind the fields the plain kernels use) */
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

/* ---- helpers of the finalising kernels (cg_body.h) ---- */

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

/* workgroups whose slots hold an element */
static unsigned cg_grid(int M) {
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
/* kernel(...) in one workgroup on stream s: every finalising kernel */
#define CG_FINAL(kernel, s, ...)                                              \
    hipLaunchKernelGGL(kernel, dim3(1), dim3(CG_FINAL_T), 0, s, __VA_ARGS__)

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
};

#define CG_PRE 0
#include "cg_body.h"
#undef CG_PRE
#define CG_PRE 1
#include "cg_body.h"
#undef CG_PRE

/* ------------------------------------------------------------------ */
/* host                                                                 */
/* ------------------------------------------------------------------ */

/* state, the sets of partial sums (pq, rn; preconditioned: and zn, which is
 * live together with rn), R, P, Q */
int64_t cg_work_bytes(int M, int k, int pre) {
    if (M < 0 || k < 1 || k > CG_MAXK)
        return -EINVAL;
    return CG_STATE_BYTES + (pre ? 3 : 2) * CG_PART_BYTES +
           3 * 8 * (int64_t)M * k;
}

/* The host loop of both solvers: minv == NULL is the plain one, else the
 * preconditioned one (the CG_PRE 1 pass of cg_body.h, a third set of partial
 * sums).  The arguments were checked by the caller (engine.hip, cg): k in
 * 1..8, ldb, ldx >= k, M == N > 0, tol >= 0, maxit >= 0, check_every > 0. */
int cg_solve(const cg_matrix *A, int k, const double *B, int64_t ldb, double *X,
             int64_t ldx, const double *minv, double tol, int maxit,
             int check_every, void *d_work, size_t work_bytes,
             spmv_cg_info *info, hipStream_t s) {
    const int M = A->M;
    const size_t need = (size_t)cg_work_bytes(M, k, minv != NULL);
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
        const cg_run c = {k, M, (int)cg_grid(M), tol * tol, st, minv, X, ldx,
                          part0, part1, part2, R, P, Q, s};
        /* the one place the solvers part: which pass of cg_body.h enqueues */
        void (*const start)(const cg_run &) = minv ? pcg_start : cg_start;
        void (*const iterate)(const cg_run &) = minv ? pcg_iterate : cg_iterate;

        /* R = B - A X; bb, rr; P, the first classification */
        CG_LAUNCH(k_cg_copy, k, M, s, B, ldb, R, k);
        rc = A->axpby(A->handle, A->opts, k, -1.0, 1.0, X, ldx, R, k, s);
        if (rc)
            goto fail;
        CG_LAUNCH(k_cg_dot, k, M, s, B, ldb, B, ldb, part0);
        CG_LAUNCH(k_cg_dot, k, M, s, R, k, R, k, part1);
        start(c);
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
                CG_LAUNCH(k_cg_dot, k, M, s, P, k, Q, k, part0);
                iterate(c);
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
