/*
 * cg_body.h -- the kernels of an iteration and the two host functions that
 * enqueue them, written ONCE and included TWICE by cg_kernels.hip (and by
 * nothing else; no include guard):
 *   CG_PRE 0   k_cg_update, k_cg_dir, k_cg_final_init, k_cg_final_pq,
 *              k_cg_final_rr; cg_start, cg_iterate     (spmv_*_cg)
 *   CG_PRE 1   k_pcg_update, k_pcg_dir, k_pcg_final_init, k_pcg_final_pq,
 *              k_pcg_final_rz; pcg_start, pcg_iterate  (spmv_*_pcg): the minv
 *              argument, z(R) = rn(minv_i * r_i) per row, its sum rz and a
 *              third set of partial sums
 * Everything outside an `#if CG_PRE` block is common to both: the frozen-column
 * rule, the clamped unconditional loads, contract(off) and the breakdown
 * ladder exist once, so pcg(ones) == cg to the bit cannot drift.  The
 * preprocessor and not a template switch or a shared __device__ body, because
 * this is the form that leaves every kernel what it was to the byte (DESIGN.md
 * section 17; a template body with `if constexpr` was tried and rescheduled all
 * 16 update kernels).
 *
 * Z is never stored: the three kernels that need it recompute it from R and
 * minv[row] -- 8 M bytes per pass instead of 8 k M to write and 8 k M to read.
 * Lane (t, j) of a pass loads minv[row t]: the K lanes of a row read one
 * address, a wavefront's load covers 512 / K consecutive bytes of the lines
 * its neighbours read, and the R / P / Q / X loads keep the layout of
 * cg_lanes.  minv of all 1.0 makes z(R) = R to the bit, rz = rr, and every
 * test of the preconditioned pass the one of the plain pass.
 */
#if CG_PRE
#define CG_KERNEL(plain, pre) pre
#define CG_PRE_ARG(a) a, /* an argument only the preconditioned pass has */
#define CG_PRE_LAST(a) , a
#else
#define CG_KERNEL(plain, pre) plain
#define CG_PRE_ARG(a)
#define CG_PRE_LAST(a)
#endif

/* fused update of the running columns: X += alpha P, R -= alpha Q, and the
 * partials of R.R (CG_PRE: and of R.z(R)) in the dot order -- one pass */
template <int K>
__global__ void __launch_bounds__(CG_T)
CG_KERNEL(k_cg_update, k_pcg_update)(
        int M, const cg_state *__restrict__ st,
        CG_PRE_ARG(const double *__restrict__ minv)
        double *__restrict__ X, int64_t ldx, const double *__restrict__ P,
        double *__restrict__ R, const double *__restrict__ Q,
#if CG_PRE
        double *__restrict__ part_rr, double *__restrict__ part_rz
#else
        double *__restrict__ part
#endif
        ) {
#pragma clang fp contract(off)
    const cg_lanes<K> l;
    bool running[K];
    cg_running<K>(st, l, running);
    double alpha[K], acc[K];
#if CG_PRE
    double accz[K];
#endif
#pragma unroll
    for (int n = 0; n < K; ++n) {
        alpha[n] = st->alpha[l.j[n]];
        acc[n] = 0.0;
#if CG_PRE
        accz[n] = 0.0;
#endif
    }
    CG_SWEEPS(base, M) {
        double x[K], p[K], r[K], q[K];
#if CG_PRE
        double d[K];
#endif
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n] < M ? base + l.t[n] : M - 1;
            x[n] = X[i * ldx + l.j[n]];
            p[n] = P[i * K + l.j[n]];
            r[n] = R[i * K + l.j[n]];
            q[n] = Q[i * K + l.j[n]];
#if CG_PRE
            d[n] = minv[i];
#endif
        }
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n];
            const double ap = alpha[n] * p[n];
            const double aq = alpha[n] * q[n];
            const double xn = x[n] + ap;
            const double rn = r[n] - aq;
            const double r2 = rn * rn;
#if CG_PRE
            const double z = d[n] * rn;
            const double rz = rn * z;
#endif
            const double sum = acc[n] + r2;
#if CG_PRE
            const double sumz = accz[n] + rz;
#endif
            if (i < M && running[n]) {
                X[i * ldx + l.j[n]] = xn;
                R[i * K + l.j[n]] = rn;
                acc[n] = sum;
#if CG_PRE
                accz[n] = sumz;
#endif
            }
        }
    }
#if CG_PRE
    slots_to_partial<K>(l, acc, part_rr);
    __syncthreads(); /* the tree's LDS is reused */
    slots_to_partial<K>(l, accz, part_rz);
#else
    slots_to_partial<K>(l, acc, part);
#endif
}

/* direction update of the running columns: P = R + beta P (CG_PRE: z(R) for
 * R) */
template <int K>
__global__ void __launch_bounds__(CG_T)
CG_KERNEL(k_cg_dir, k_pcg_dir)(int M, const cg_state *__restrict__ st,
                               CG_PRE_ARG(const double *__restrict__ minv)
                               const double *__restrict__ R,
                               double *__restrict__ P) {
#pragma clang fp contract(off)
    const cg_lanes<K> l;
    bool running[K];
    cg_running<K>(st, l, running);
    double beta[K];
#pragma unroll
    for (int n = 0; n < K; ++n)
        beta[n] = st->beta[l.j[n]];
    CG_SWEEPS(base, M) {
        double p[K], r[K];
#if CG_PRE
        double d[K];
#endif
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n] < M ? base + l.t[n] : M - 1;
            p[n] = P[i * K + l.j[n]];
            r[n] = R[i * K + l.j[n]];
#if CG_PRE
            d[n] = minv[i];
#endif
        }
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const int64_t i = base + l.t[n];
#if CG_PRE
            const double z = d[n] * r[n];
#endif
            const double bp = beta[n] * p[n];
            if (i < M && running[n])
#if CG_PRE
                P[i * K + l.j[n]] = z + bp;
#else
                P[i * K + l.j[n]] = r[n] + bp;
#endif
        }
    }
}

/* ---- the finalising kernels: ONE workgroup of CG_FINAL_T threads ---- */

/* bb = B.B, rr = R.R (CG_PRE: rz = R.z(R)); a column starts broken down (a
 * non-finite sum), converged, (CG_PRE: broken down, rz not positive) or
 * running */
__global__ void __launch_bounds__(CG_FINAL_T)
CG_KERNEL(k_cg_final_init, k_pcg_final_init)(
        int k, int nwg, const double *__restrict__ part_bb,
        const double *__restrict__ part_rr,
        CG_PRE_ARG(const double *__restrict__ part_rz)
        double tol2, cg_state *__restrict__ st) {
    __shared__ double s[CG_FINAL_T];
    for (int j = 0; j < CG_MAXK; ++j) {
        double bb = 0.0, rr = 0.0;
#if CG_PRE
        double rz = 0.0;
#endif
        if (j < k) { /* uniform */
            bb = final_sum(part_bb, nwg, k, j, s);
            rr = final_sum(part_rr, nwg, k, j, s);
#if CG_PRE
            rz = final_sum(part_rz, nwg, k, j, s);
#endif
        }
        if (threadIdx.x == 0) {
            st->bb[j] = bb;
            st->rr[j] = rr;
#if CG_PRE
            st->rz[j] = rz;
#endif
            st->alpha[j] = 0.0;
            st->beta[j] = 0.0;
            st->iters[j] = 0;
            st->status[j] =
                j >= k ? CG_CONVERGED
#if CG_PRE
                : !(cg_finite(rr) && cg_finite(bb) && cg_finite(rz))
                    ? CG_BREAKDOWN
                : rr <= tol2 * bb ? CG_CONVERGED
                : !(rz > 0.0)     ? CG_BREAKDOWN
#else
                : !(cg_finite(rr) && cg_finite(bb)) ? CG_BREAKDOWN
                : rr <= tol2 * bb ? CG_CONVERGED
#endif
                                  : CG_RUNNING;
        }
    }
}

/* pq = P.Q: a running column breaks down, or gets its alpha = rr / pq (CG_PRE:
 * rz / pq) and counts the update of x that follows */
__global__ void __launch_bounds__(CG_FINAL_T)
CG_KERNEL(k_cg_final_pq, k_pcg_final_pq)(int k, int nwg,
                                         const double *__restrict__ part,
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
#if CG_PRE
                st->alpha[j] = st->rz[j] / pq;
#else
                st->alpha[j] = st->rr[j] / pq;
#endif
                st->iters[j] += 1;
            }
        }
    }
}

/* rn = R.R (CG_PRE: zn = R.z(R)) after the update: a running column converges,
 * breaks down, or gets its beta = rn / rr (CG_PRE: zn / rz) and the new rr
 * (, rz) */
__global__ void __launch_bounds__(CG_FINAL_T)
CG_KERNEL(k_cg_final_rr, k_pcg_final_rz)(
        int k, int nwg,
#if CG_PRE
        const double *__restrict__ part_rr, const double *__restrict__ part_rz,
#else
        const double *__restrict__ part,
#endif
        double tol2, cg_state *st) {
    __shared__ double s[CG_FINAL_T];
    for (int j = 0; j < k; ++j) {
        if (st->status[j] != CG_RUNNING) /* uniform */
            continue;
#if CG_PRE
        const double rn = final_sum(part_rr, nwg, k, j, s);
        const double zn = final_sum(part_rz, nwg, k, j, s);
#else
        const double rn = final_sum(part, nwg, k, j, s);
#endif
        if (threadIdx.x == 0) {
            if (rn <= tol2 * st->bb[j]) {
                st->status[j] = CG_CONVERGED;
                st->rr[j] = rn;
#if CG_PRE
            } else if (!cg_finite(rn) || !(zn > 0.0 && cg_finite(zn))) {
                st->status[j] = CG_BREAKDOWN;
            } else {
                st->beta[j] = zn / st->rz[j];
                st->rr[j] = rn;
                st->rz[j] = zn;
            }
#else
            } else if (!cg_finite(rn)) {
                st->status[j] = CG_BREAKDOWN;
            } else {
                st->beta[j] = rn / st->rr[j];
                st->rr[j] = rn;
            }
#endif
        }
    }
}

/* ---- host: what solve() enqueues, in launch order ---- */

/* P = R (CG_PRE: z(R), and the partials of rz); bb, rr (, rz) and the first
 * classification */
static void CG_KERNEL(cg_start, pcg_start)(const cg_run &c) {
#if CG_PRE
    CG_LAUNCH(k_pcg_first, c.k, c.M, c.s, c.minv, c.R, c.P, c.part2);
#else
    CG_LAUNCH(k_cg_copy, c.k, c.M, c.s, c.R, c.k, c.P, c.k);
#endif
    CG_FINAL(CG_KERNEL(k_cg_final_init, k_pcg_final_init), c.s, c.k, c.nwg,
             c.part0, c.part1, CG_PRE_ARG(c.part2) c.tol2, c.st);
}

/* one iteration behind the partials of P.Q in part0 */
static void CG_KERNEL(cg_iterate, pcg_iterate)(const cg_run &c) {
    CG_FINAL(CG_KERNEL(k_cg_final_pq, k_pcg_final_pq), c.s, c.k, c.nwg,
             c.part0, c.st);
    CG_LAUNCH(CG_KERNEL(k_cg_update, k_pcg_update), c.k, c.M, c.s, c.st,
              CG_PRE_ARG(c.minv) c.X, c.ldx, c.P, c.R, c.Q,
              c.part1 CG_PRE_LAST(c.part2));
    CG_FINAL(CG_KERNEL(k_cg_final_rr, k_pcg_final_rz), c.s, c.k, c.nwg,
             c.part1, CG_PRE_ARG(c.part2) c.tol2, c.st);
    CG_LAUNCH(CG_KERNEL(k_cg_dir, k_pcg_dir), c.k, c.M, c.s, c.st,
              CG_PRE_ARG(c.minv) c.R, c.P);
}

#undef CG_KERNEL
#undef CG_PRE_ARG
#undef CG_PRE_LAST
