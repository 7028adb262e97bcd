/*
 * amg_kernels.hip -- the kernels of smoothed-aggregation AMG (spmv_csr_aggregate,
 * spmv_csr_amg_setup, spmv_amg_apply; spmv_engine.h), gfx950 (wave64).  The
 * host arithmetic -- the key of a row, the scratch layout, the launch count --
 * is amg_plan.h; the hierarchy and the cycle's launch list are engine.hip.
 *
 * AGGREGATION (blocks; agg and the info are functions of the pattern, the
 * values, theta and the seed alone):
 *   k_amg_check    rows strictly ascending, columns inside, the diagonal stored
 *                  (a flag word, atomicOr: decides no position); d[i]
 *   k_ag_strong    one byte per entry: rn(a a) >= rn(theta2 |rn(d_i d_j)|),
 *                  j != i; a comparison with a NaN is false
 *   k_ag_init      the undecided key of every row (amg_plan.h)
 *   a ROUND is three launches and one 4-byte read-back, one lane per row:
 *     k_ag_nmax    t1[i] = max(key[i], key[j] over the strong j of row i)
 *     k_ag_nmax    t2[i] = the same of t1
 *     k_ag_decide  an undecided row whose t2 is its own key becomes a root, one
 *                  whose t2 is a root's key becomes out; the new keys go to
 *                  the array that held t1.  The rows still undecided are
 *                  counted per wavefront and added with one integer atomic: a
 *                  COUNT does not depend on the order of arrival
 *     every launch reads what EARLIER launches wrote and writes another array;
 *     the host stops at max_rounds: no device loop is unbounded
 *   k_ag_flag + tr_scan   the roots numbered in row order
 *   k_ag_pass1     a row that is no root joins the strong root of the greatest
 *                  |a|, the first in stored order among equals
 *   k_ag_pass2     a row still free joins the aggregate (of pass 1) of its
 *                  strong neighbour of the greatest |a|, likewise; reads pass
 *                  1's array, writes a new one, flags the rows still free
 *   tr_scan + k_ag_final  those become singletons, numbered behind the roots
 *   k_ag_count, k_ag_max  the largest aggregate (integer atomics on counts)
 * No POSITION comes from an atomic, and no workgroup waits for another.
 *
 * SETUP: k_amg_rho (the Gershgorin bound of D^-1 A: S_i the sequential sum of
 * |a_ij| in stored order, rn(S_i / |d_i|), the maximum by an integer atomicMax
 * on the bit patterns of non-negative doubles, exact in any order; a NaN takes
 * the pattern above every number), k_amg_w (w = rn(omega / d)), k_amg_tent (T:
 * one 1.0 per row at column agg[i]) and k_amg_psmooth (P = T - diag(w) A T in
 * place on the values of A T).
 *
 * CYCLE: the vector kernels of a sweep, element f of the M x k block per
 * thread (row f / k, column f % k: whole cache lines whatever k), contraction
 * off -- every operation is rounded once:
 *   k_amg_first    x = rn(w_i b); r = b
 *   k_amg_update   x = rn(x + rn(w_i r)), r being rn(b - A x) as launch_axpby
 *                  (-1, 1) left it; REFILL: r = b again, for the next product
 * The transfer products are the level handles' launch_multi / launch_axpby.
 *
 * THE FUSED SWEEP, k_amg_sweep: one pass over A_l that reads x_old, b and w
 * and writes x_new = rn(x_old + rn(w_i rn(b - s))) to the OTHER buffer of a
 * ping-pong (a lane gathers x_old of other rows, so it cannot be in place);
 * residual mode: out = rn(b - s), no w.  The walk is k_csr_multi's
 * (multi_body.h), copied: G lanes per row, P rows per lane group, lane `sub`
 * starts from the plain product of entry `sub` and adds entries sub + G, ...
 * with fused multiply-adds, then group_sum<G> -- so s has the bits of
 * launch_multi on the handle, and the epilogue (contraction off) those of
 * launch_axpby(-1, 1) and the vector kernel.  b, x_old's own row and w are
 * loaded FIRST, ahead of IRP (behind the gathers they
 * would be a fourth dependent round trip), spread over the row's G lanes and
 * collected with DPP moves where lane 0 stores.  Rows of more than STREAM_NNZ
 * entries are not this kernel's: a handle that has one (n_long_rb > 0) sweeps
 * by the composition, which gives the same bits.
 */
#include <string.h>
#include <vector>

#include "amg_plan.h"
#include "csr_build.h"

static_assert(AMG_T % WAVE == 0, "whole wavefronts");

/* device scratch of one call: freed on every path */
struct amg_scratch {
    std::vector<void *> blocks;
    ~amg_scratch() {
        for (void *b : blocks)
            (void)hipFree(b);
    }
    /* at least one element, so that no pointer handed to a kernel is NULL */
    template <typename T> hipError_t get(T **out, int64_t count) {
        void *p = NULL;
        const hipError_t e =
            hipMalloc(&p, (size_t)(count > 0 ? count : 1) * sizeof(T));
        if (e == hipSuccess)
            blocks.push_back(p);
        *out = (T *)p;
        return e;
    }
};

/* ------------------------------------------------------------------ */
/* the check and the diagonal                                           */
/* ------------------------------------------------------------------ */

/* d: M doubles or NULL */
__global__ void __launch_bounds__(AMG_T)
k_amg_check(int M, const int *__restrict__ irp, const int *__restrict__ ja,
            const double *__restrict__ as, double *__restrict__ d,
            unsigned *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * AMG_T + threadIdx.x;
    if (i >= M)
        return;
    unsigned bad = 0;
    bool has_diag = false;
    double dv = 0.0;
    int prev = -1;
    for (int64_t e = irp[i], end = irp[i + 1]; e < end; ++e) {
        const int j = ja[e];
        if ((unsigned)j >= (unsigned)M)
            bad |= CSR_BAD_COLUMN;
        if (j <= prev)
            bad |= CSR_BAD_ORDER;
        prev = j;
        if (j == (int)i) {
            has_diag = true;
            dv = as[e];
        }
    }
    if (!has_diag)
        bad |= CSR_BAD_ORDER;
    if (d)
        d[i] = dv;
    if (bad)
        atomicOr(flag, bad);
}

/* 0; -EDOM: a column outside [0, M); -EINVAL: a row not strictly ascending or
 * without its diagonal.  d_diag (M doubles or NULL) receives the diagonal */
int amg_check_dev(const spmv_csr_dev *A, double *d_diag, hipStream_t s) {
    int rc = 0;
    amg_scratch scratch;
    unsigned *d_flag = NULL, flag = 0;
    if (A->M == 0)
        return 0;
    (void)hipGetLastError(); /* an earlier caller's unread error is not ours */
    HIP_TRY(scratch.get(&d_flag, 1));
    HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(unsigned), s));
    hipLaunchKernelGGL(k_amg_check, grid_for(A->M, AMG_T), dim3(AMG_T), 0, s,
                       A->M, A->irp, A->ja, A->as, d_diag, d_flag);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&flag, d_flag, sizeof(unsigned),
                           hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    rc = csr_flags_errno(flag);
fail:
    if (rc)
        (void)hipStreamSynchronize(s);
    return rc;
}

/* ------------------------------------------------------------------ */
/* aggregation                                                          */
/* ------------------------------------------------------------------ */

__global__ void __launch_bounds__(AMG_T)
k_ag_strong(int M, double theta2, const int *__restrict__ irp,
            const int *__restrict__ ja, const double *__restrict__ as,
            const double *__restrict__ d, unsigned char *__restrict__ strong) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * AMG_T + threadIdx.x;
    if (i >= M)
        return;
    const double di = d[i];
    for (int64_t e = irp[i], end = irp[i + 1]; e < end; ++e) {
        const int j = ja[e]; /* inside [0, M): k_amg_check */
        const double a = as[e];
        const double lhs = a * a;
        const double dd = di * d[j];
        const double rhs = theta2 * __builtin_fabs(dd);
        strong[e] = j != (int)i && lhs >= rhs; /* false for a NaN */
    }
}

__global__ void __launch_bounds__(AMG_T)
k_ag_init(int M, uint32_t seed, unsigned long long *__restrict__ key) {
    const int64_t i = (int64_t)blockIdx.x * AMG_T + threadIdx.x;
    if (i < M)
        key[i] = amg_key((uint32_t)i, seed);
}

__global__ void __launch_bounds__(AMG_T)
k_ag_nmax(int M, const int *__restrict__ irp, const int *__restrict__ ja,
          const unsigned char *__restrict__ strong,
          const unsigned long long *__restrict__ in,
          unsigned long long *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * AMG_T + threadIdx.x;
    if (i >= M)
        return;
    unsigned long long m = in[i];
    for (int64_t e = irp[i], end = irp[i + 1]; e < end; ++e)
        if (strong[e]) {
            const unsigned long long v = in[ja[e]];
            m = v > m ? v : m;
        }
    out[i] = m;
}

/* count += the rows still undecided behind this launch; *clear = 0 is the
 * counter of the next round */
__global__ void __launch_bounds__(AMG_T)
k_ag_decide(int M, uint32_t seed, const unsigned long long *__restrict__ key,
            const unsigned long long *__restrict__ t2,
            unsigned long long *__restrict__ out, int *__restrict__ count,
            int *__restrict__ clear) {
    const int64_t i = (int64_t)blockIdx.x * AMG_T + threadIdx.x;
    if (i == 0)
        *clear = 0;
    bool undecided = false;
    if (i < M) {
        unsigned long long k = key[i];
        /* undecided: exactly the row's own first key.  (Row 0 at seed 0 has
         * the key 0 of an out row: once out it is looked at again, sees the
         * root that put it out, and stays out -- it is not counted) */
        if (k == amg_key((uint32_t)i, seed)) {
            const unsigned long long m = t2[i];
            if (m == k)
                k |= AMG_KEY_ROOT;
            else if (amg_key_is_root(m))
                k = 0;
            else
                undecided = true;
        }
        out[i] = k;
    }
    const unsigned long long who = __ballot(undecided);
    if (who && (threadIdx.x & (WAVE - 1)) == (unsigned)__builtin_ctzll(who))
        atomicAdd(count, __popcll(who));
}

/* flag[i] = 1 for a root, i < M; flag[M] = 0 (the scan's total lands there) */
__global__ void __launch_bounds__(AMG_T)
k_ag_flag(int M, const unsigned long long *__restrict__ key,
          int *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * AMG_T + threadIdx.x;
    if (i <= M)
        flag[i] = i < M ? amg_key_is_root(key[i]) : 0;
}

/* rid: the exclusive scan of the root flags */
__global__ void __launch_bounds__(AMG_T)
k_ag_pass1(int M, const int *__restrict__ irp, const int *__restrict__ ja,
           const double *__restrict__ as,
           const unsigned char *__restrict__ strong,
           const unsigned long long *__restrict__ key,
           const int *__restrict__ rid, int *__restrict__ agg1) {
    const int64_t i = (int64_t)blockIdx.x * AMG_T + threadIdx.x;
    if (i >= M)
        return;
    int a = -1;
    if (amg_key_is_root(key[i])) {
        a = rid[i];
    } else {
        double best = -1.0; /* |a| >= 0 of a strong entry: the first one wins */
        for (int64_t e = irp[i], end = irp[i + 1]; e < end; ++e) {
            if (!strong[e])
                continue;
            const int j = ja[e];
            const double v = __builtin_fabs(as[e]);
            if (amg_key_is_root(key[j]) && v > best) {
                best = v;
                a = rid[j];
            }
        }
    }
    agg1[i] = a;
}

/* single[i] = 1 for a row still free, i < M; single[M] = 0 */
__global__ void __launch_bounds__(AMG_T)
k_ag_pass2(int M, const int *__restrict__ irp, const int *__restrict__ ja,
           const double *__restrict__ as,
           const unsigned char *__restrict__ strong,
           const int *__restrict__ agg1, int *__restrict__ agg2,
           int *__restrict__ single) {
    const int64_t i = (int64_t)blockIdx.x * AMG_T + threadIdx.x;
    if (i > M)
        return;
    if (i == M) {
        single[M] = 0;
        return;
    }
    int a = agg1[i];
    if (a < 0) {
        double best = -1.0;
        for (int64_t e = irp[i], end = irp[i + 1]; e < end; ++e) {
            if (!strong[e])
                continue;
            const int aj = agg1[ja[e]];
            const double v = __builtin_fabs(as[e]);
            if (aj >= 0 && v > best) {
                best = v;
                a = aj;
            }
        }
    }
    agg2[i] = a;
    single[i] = a < 0;
}

/* sid: the exclusive scan of the singleton flags */
__global__ void __launch_bounds__(AMG_T)
k_ag_final(int M, int roots, const int *__restrict__ agg2,
           const int *__restrict__ sid, int *__restrict__ agg) {
    const int64_t i = (int64_t)blockIdx.x * AMG_T + threadIdx.x;
    if (i >= M)
        return;
    const int a = agg2[i];
    agg[i] = a >= 0 ? a : roots + sid[i];
}

/* size[agg[i]] += 1: a count; every agg[i] < n was checked by construction
 * (rid < roots, sid < singles), and is checked again here */
__global__ void __launch_bounds__(AMG_T)
k_ag_count(int M, int n, const int *__restrict__ agg, int *__restrict__ size) {
    const int64_t i = (int64_t)blockIdx.x * AMG_T + threadIdx.x;
    if (i >= M)
        return;
    const int a = agg[i];
    if ((unsigned)a < (unsigned)n)
        atomicAdd(size + a, 1);
}

/* *maxv = max(*maxv, v[i]) */
__global__ void __launch_bounds__(AMG_T)
k_ag_max(int n, const int *__restrict__ v, int *__restrict__ maxv) {
    const int64_t first = (int64_t)blockIdx.x * AMG_T + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * AMG_T;
    int m = 0;
    for (int64_t i = first; i < n; i += stride)
        m = max(m, v[i]);
#pragma unroll
    for (int d = WAVE / 2; d > 0; d >>= 1)
        m = max(m, __shfl_down(m, d, WAVE));
    if ((threadIdx.x & (WAVE - 1)) == 0 && m > 0)
        atomicMax(maxv, m);
}

/* the caller has checked the handle: square, f64, with its source */
int amg_aggregate_dev(const spmv_csr_dev *A, double theta2, uint32_t seed,
                      int max_rounds, int *d_agg, spmv_aggregate_info *info,
                      hipStream_t s) {
    int rc = 0;
    const int M = A->M;
    const int64_t NZ = A->NZ;
    amg_scratch scratch;
    spmv_aggregate_info got = {0, 0, 0, 0, 0};
    double *diag = NULL;
    unsigned char *strong = NULL;
    unsigned long long *key[3] = {NULL, NULL, NULL};
    int *counters = NULL, *flag = NULL, *sums = NULL, *agg1 = NULL,
        *agg2 = NULL, *single = NULL, *agg = NULL, *size = NULL;
    int rounds = 0, left = M, roots = 0, singles = 0, widest = 0;
    int cur = 0; /* key[cur] holds the keys */
    const dim3 grid = grid_for(M, AMG_T), wg(AMG_T);
    const dim3 grid1 = grid_for((int64_t)M + 1, AMG_T);
    if (M == 0) {
        if (info)
            *info = got;
        return 0;
    }
    (void)hipGetLastError(); /* an earlier caller's unread error is not ours */
    HIP_TRY(scratch.get(&diag, M));
    rc = amg_check_dev(A, diag, s);
    if (rc)
        return rc;
    HIP_TRY(scratch.get(&strong, NZ));
    for (int n = 0; n < 3; ++n)
        HIP_TRY(scratch.get(&key[n], M));
    HIP_TRY(scratch.get(&counters, 4)); /* three round counters, the maximum */
    HIP_TRY(scratch.get(&flag, (int64_t)M + 1));
    HIP_TRY(scratch.get(&single, (int64_t)M + 1));
    HIP_TRY(scratch.get(&sums, transpose_scan_tiles((int64_t)M + 1)));
    HIP_TRY(scratch.get(&agg1, M));
    HIP_TRY(scratch.get(&agg2, M));
    HIP_TRY(scratch.get(&agg, M));
    HIP_TRY(hipMemsetAsync(counters, 0, 4 * sizeof(int), s));
    hipLaunchKernelGGL(k_ag_strong, grid, wg, 0, s, M, theta2, A->irp, A->ja,
                       A->as, diag, strong);
    hipLaunchKernelGGL(k_ag_init, grid, wg, 0, s, M, seed, key[0]);
    HIP_TRY(hipGetLastError());
    /* the rounds: three launches and one read-back each */
    while (left > 0) {
        if (rounds >= max_rounds) {
            rc = -E2BIG;
            goto fail;
        }
        unsigned long long *k0 = key[cur], *t1 = key[(cur + 1) % 3],
                           *t2 = key[(cur + 2) % 3];
        int now = 0;
        hipLaunchKernelGGL(k_ag_nmax, grid, wg, 0, s, M, A->irp, A->ja, strong,
                           k0, t1);
        hipLaunchKernelGGL(k_ag_nmax, grid, wg, 0, s, M, A->irp, A->ja, strong,
                           t1, t2);
        hipLaunchKernelGGL(k_ag_decide, grid, wg, 0, s, M, seed, k0, t2, t1,
                           counters + rounds % 3, counters + (rounds + 1) % 3);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&now, counters + rounds % 3, sizeof(int),
                               hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        ++rounds;
        cur = (cur + 1) % 3;
        /* the undecided row of the greatest key always leaves */
        if (now < 0 || now >= left) {
            rc = -EIO;
            goto fail;
        }
        left = now;
    }
    hipLaunchKernelGGL(k_ag_flag, grid1, wg, 0, s, M, key[cur], flag);
    tr_scan(flag, (int64_t)M + 1, sums, s);
    hipLaunchKernelGGL(k_ag_pass1, grid, wg, 0, s, M, A->irp, A->ja, A->as,
                       strong, key[cur], flag, agg1);
    hipLaunchKernelGGL(k_ag_pass2, grid1, wg, 0, s, M, A->irp, A->ja, A->as,
                       strong, agg1, agg2, single);
    tr_scan(single, (int64_t)M + 1, sums, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&roots, flag + M, sizeof(int), hipMemcpyDeviceToHost,
                           s));
    HIP_TRY(hipMemcpyAsync(&singles, single + M, sizeof(int),
                           hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (roots < 1 || singles < 0 || (int64_t)roots + singles > M) {
        rc = -EIO;
        goto fail;
    }
    hipLaunchKernelGGL(k_ag_final, grid, wg, 0, s, M, roots, agg2, single, agg);
    HIP_TRY(scratch.get(&size, (int64_t)roots + singles));
    HIP_TRY(hipMemsetAsync(size, 0, ((size_t)roots + singles) * sizeof(int), s));
    hipLaunchKernelGGL(k_ag_count, grid, wg, 0, s, M, roots + singles, agg,
                       size);
    hipLaunchKernelGGL(k_ag_max, dim3(1024), wg, 0, s, roots + singles, size,
                       counters + 3);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&widest, counters + 3, sizeof(int),
                           hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (widest < 1 || widest > M) {
        rc = -EIO;
        goto fail;
    }
    got.aggregates = roots + singles;
    got.roots = roots;
    got.rounds = rounds;
    got.widest = widest;
    got.singletons = singles;
    /* the caller's array last: an error above leaves it untouched */
    if (d_agg) {
        HIP_TRY(hipMemcpyAsync(d_agg, agg, (size_t)M * sizeof(int),
                               hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    if (info)
        *info = got;
fail:
    if (rc) /* nothing of ours is left running when the scratch is freed */
        (void)hipStreamSynchronize(s);
    return rc;
}

/* ------------------------------------------------------------------ */
/* setup: rho, w, T, P                                                  */
/* ------------------------------------------------------------------ */

/* *rho_bits = max over the rows of the bit pattern of rn(S_i / |d_i|) */
__global__ void __launch_bounds__(AMG_T)
k_amg_rho(int M, const int *__restrict__ irp, const double *__restrict__ as,
          const double *__restrict__ d, unsigned long long *__restrict__ rho) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * AMG_T + threadIdx.x;
    unsigned long long bits = 0;
    if (i < M) {
        double sum = 0.0;
        for (int64_t e = irp[i], end = irp[i + 1]; e < end; ++e)
            sum = sum + __builtin_fabs(as[e]);
        const double q = sum / __builtin_fabs(d[i]);
        /* q >= +0.0 or a NaN: above every number, whatever its sign bit */
        bits = q != q ? 0x7ff8000000000000ull
                      : (unsigned long long)__double_as_longlong(q);
    }
#pragma unroll
    for (int s = WAVE / 2; s > 0; s >>= 1) {
        const unsigned long long o = __shfl_down(bits, s, WAVE);
        bits = o > bits ? o : bits;
    }
    if ((threadIdx.x & (WAVE - 1)) == 0 && bits)
        atomicMax(rho, bits);
}

/* in place: w[i] = rn(omega / d[i]) */
__global__ void __launch_bounds__(AMG_T)
k_amg_w(int M, double omega, double *__restrict__ w) {
    const int64_t i = (int64_t)blockIdx.x * AMG_T + threadIdx.x;
    if (i < M)
        w[i] = omega / w[i];
}

/* d_w: M doubles; receives the diagonal, then (amg_w_dev) w.  The caller has
 * run amg_check_dev on A.  Blocks for the one read-back */
int amg_rho_dev(const spmv_csr_dev *A, double *d_w, double *rho,
                hipStream_t s) {
    int rc = 0;
    amg_scratch scratch;
    unsigned *d_flag = NULL;
    unsigned long long *d_rho = NULL, bits = 0;
    (void)hipGetLastError();
    HIP_TRY(scratch.get(&d_rho, 2));
    d_flag = (unsigned *)(d_rho + 1);
    HIP_TRY(hipMemsetAsync(d_rho, 0, 2 * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_amg_check, grid_for(A->M, AMG_T), dim3(AMG_T), 0, s,
                       A->M, A->irp, A->ja, A->as, d_w, d_flag);
    hipLaunchKernelGGL(k_amg_rho, grid_for(A->M, AMG_T), dim3(AMG_T), 0, s,
                       A->M, A->irp, A->as, d_w, d_rho);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&bits, d_rho, sizeof bits, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    memcpy(rho, &bits, sizeof bits);
fail:
    if (rc)
        (void)hipStreamSynchronize(s);
    return rc;
}

int amg_w_dev(int M, double omega, double *d_w, hipStream_t s) {
    hipLaunchKernelGGL(k_amg_w, grid_for(M, AMG_T), dim3(AMG_T), 0, s, M, omega,
                       d_w);
    return hip_errno(hipGetLastError());
}

/* T: irp[i] = i (i <= M), ja[i] = agg[i], as[i] = 1.0 */
__global__ void __launch_bounds__(AMG_T)
k_amg_tent(int M, const int *__restrict__ agg, int *__restrict__ irp,
           int *__restrict__ ja, double *__restrict__ as) {
    const int64_t i = (int64_t)blockIdx.x * AMG_T + threadIdx.x;
    if (i > M)
        return;
    irp[i] = (int)i;
    if (i < M) {
        ja[i] = agg[i];
        as[i] = 1.0;
    }
}

int amg_tentative_dev(int M, const int *d_agg, spmv_csr_dev *T, hipStream_t s) {
    hipLaunchKernelGGL(k_amg_tent, grid_for((int64_t)M + 1, AMG_T), dim3(AMG_T),
                       0, s, M, d_agg, T->irp, T->ja, T->as);
    return hip_errno(hipGetLastError());
}

/* in place on the values of A T: p = rn(t - rn(w_i at)), t = 1.0 at column
 * agg[i] and 0.0 elsewhere */
__global__ void __launch_bounds__(AMG_T)
k_amg_psmooth(int M, const int *__restrict__ irp, const int *__restrict__ ja,
              const int *__restrict__ agg, const double *__restrict__ w,
              double *__restrict__ as) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * AMG_T + threadIdx.x;
    if (i >= M)
        return;
    const double wi = w[i];
    const int own = agg[i];
    for (int64_t e = irp[i], end = irp[i + 1]; e < end; ++e) {
        const double t = ja[e] == own ? 1.0 : 0.0;
        const double wa = wi * as[e];
        as[e] = t - wa;
    }
}

int amg_smooth_p_dev(spmv_csr_dev *AT, const int *d_agg, const double *d_w,
                     hipStream_t s) {
    if (AT->M == 0)
        return 0;
    hipLaunchKernelGGL(k_amg_psmooth, grid_for(AT->M, AMG_T), dim3(AMG_T), 0, s,
                       AT->M, AT->irp, AT->ja, d_agg, d_w, AT->as);
    return hip_errno(hipGetLastError());
}

/* ------------------------------------------------------------------ */
/* the vector kernels of a sweep                                        */
/* ------------------------------------------------------------------ */

/* x = rn(w_i b); r = b (r NULL: x alone).  r has ld = k */
__global__ void __launch_bounds__(AMG_T)
k_amg_first(int64_t total, int k, const double *__restrict__ w,
            const double *__restrict__ b, int64_t ldb, double *__restrict__ x,
            int64_t ldx, double *__restrict__ r) {
#pragma clang fp contract(off)
    const int64_t f = (int64_t)blockIdx.x * AMG_T + threadIdx.x;
    if (f >= total)
        return;
    const int64_t i = f / k;
    const int j = (int)(f - i * k);
    const double bv = b[i * ldb + j];
    x[i * ldx + j] = w[i] * bv;
    if (r) /* uniform: the composed sweep's r = b */
        r[f] = bv;
}

/* x = rn(x + rn(w_i r)); REFILL: r = b */
template <bool REFILL>
__global__ void __launch_bounds__(AMG_T)
k_amg_update(int64_t total, int k, const double *__restrict__ w,
             const double *__restrict__ b, int64_t ldb, double *__restrict__ x,
             int64_t ldx, double *__restrict__ r) {
#pragma clang fp contract(off)
    const int64_t f = (int64_t)blockIdx.x * AMG_T + threadIdx.x;
    if (f >= total)
        return;
    const int64_t i = f / k;
    const int j = (int)(f - i * k);
    /* every load ahead of the arithmetic */
    const double xv = x[i * ldx + j], rv = r[f], wv = w[i];
    double bv = 0.0;
    if (REFILL)
        bv = b[i * ldb + j];
    const double wr = wv * rv;
    x[i * ldx + j] = xv + wr;
    if (REFILL)
        r[f] = bv;
}

void amg_first_dev(int M, int k, const double *w, const double *b, int64_t ldb,
                   double *x, int64_t ldx, double *r, hipStream_t s) {
    const int64_t total = (int64_t)M * k;
    hipLaunchKernelGGL(k_amg_first, grid_for(total, AMG_T), dim3(AMG_T), 0, s,
                       total, k, w, b, ldb, x, ldx, r);
}

void amg_update_dev(int M, int k, int refill, const double *w, const double *b,
                    int64_t ldb, double *x, int64_t ldx, double *r,
                    hipStream_t s) {
    const int64_t total = (int64_t)M * k;
    if (refill)
        hipLaunchKernelGGL((k_amg_update<true>), grid_for(total, AMG_T),
                           dim3(AMG_T), 0, s, total, k, w, b, ldb, x, ldx, r);
    else
        hipLaunchKernelGGL((k_amg_update<false>), grid_for(total, AMG_T),
                           dim3(AMG_T), 0, s, total, k, w, b, ldb, x, ldx, r);
}

/* ------------------------------------------------------------------ */
/* the fused sweep                                                      */
/* ------------------------------------------------------------------ */

template <int K>
__device__ __forceinline__ void amg_xrow(const double *__restrict__ X,
                                         int64_t ldx, int c, double (&xv)[K]) {
    const double *p = X + (int64_t)c * ldx;
#pragma unroll
    for (int j = 0; j < K; ++j)
        xv[j] = p[j];
}

/* the epilogues, contraction off: every operation rounded once */
__device__ __forceinline__ double amg_resid_of(double b, double s) {
#pragma clang fp contract(off)
    return b - s;
}
__device__ __forceinline__ double amg_sweep_of(double x, double w, double b,
                                               double s) {
#pragma clang fp contract(off)
    const double r = b - s;
    const double wr = w * r;
    return x + wr;
}

/* element j of a row's K values lives in lane j % G, slot j / G; the values
 * as lane 0 of the group needs them (DPP row_shl, inside a row of 16; all
 * lanes call) */
template <int G, int K, int YS, int J = 0>
__device__ __forceinline__ void amg_collect(const double (&v)[YS],
                                            double (&out)[K]) {
    if constexpr (J < K) {
        if constexpr (J % G == 0)
            out[J] = v[J / G];
        else
            out[J] = dpp_f64<0x100 + J % G>(v[J / G]);
        amg_collect<G, K, YS, J + 1>(v, out);
    }
}

template <int G, int P, int K, bool SMOOTH>
__global__ void k_amg_sweep(int M, int order, const int *__restrict__ irp,
                            const int *__restrict__ ja,
                            const double *__restrict__ as,
                            const double *__restrict__ X, int64_t ldx,
                            const double *__restrict__ B, int64_t ldb,
                            const double *__restrict__ W,
                            double *__restrict__ OUT, int64_t ldo) {
    constexpr int RPP = WAVE / G; /* rows per pass */
    constexpr int YS = (K + G - 1) / G;
    const int lane = threadIdx.x & (WAVE - 1);
    const int sub = lane & (G - 1);
    const long long bid = order == 1 ? xcd_remap(blockIdx.x, gridDim.x)
                          : order == 2 ? xcd_grouped<long long>(blockIdx.x)
                                       : (long long)blockIdx.x;
    const long long wave_global = (bid * blockDim.x + threadIdx.x) / WAVE;
    const long long rbase = wave_global * (P * RPP) + lane / G;
    /* b, x_old and w FIRST: their addresses need no IRP */
    double bo[P][YS], xo[P][YS], wv[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const long long row = rbase + p * RPP;
        const bool live = row < M;
        const double *br = B + row * ldb;
        const double *xr = X + row * ldx;
#pragma unroll
        for (int s = 0; s < YS; ++s) {
            const bool ld = live && sub + s * G < K;
            bo[p][s] = ld ? ld_stream(br + sub + s * G) : 0.0;
            xo[p][s] = SMOOTH && ld ? xr[sub + s * G] : 0.0;
        }
        wv[p] = SMOOTH && live ? W[row] : 0.0;
    }
    int beg[P], end[P];
    bool mine[P]; /* this kernel writes the row (inside M, not a long row) */
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const long long row = rbase + p * RPP;
        const bool live = row < M;
        beg[p] = live ? irp[row] : 0;
        end[p] = live ? irp[row + 1] : 0;
        mine[p] = live;
        if (end[p] - beg[p] > STREAM_NNZ) { /* never: the launcher's check */
            end[p] = beg[p];
            mine[p] = false;
        }
    }
    int c[P];
    double a[P];
    double acc[P][K];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const bool has = sub < end[p] - beg[p];
        c[p] = has ? ld_stream(ja + beg[p] + sub) : -1;
        a[p] = has ? ld_stream(as + beg[p] + sub) : 0.0;
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
#pragma unroll
        for (int j = 0; j < K; ++j)
            acc[p][j] = 0.0;
        if (c[p] >= 0)
            amg_xrow<K>(X, ldx, c[p], acc[p]);
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const double av = a[p];
#pragma unroll
        for (int j = 0; j < K; ++j) /* the lane's first product: a multiply */
            acc[p][j] = c[p] >= 0 ? av * acc[p][j] : 0.0;
    }
#pragma unroll
    for (int p = 0; p < P; ++p)
        for (int k = sub + G, n = end[p] - beg[p]; k < n; k += G) {
            double xv[K];
            const double av = ld_stream(as + beg[p] + k);
            amg_xrow<K>(X, ldx, ld_stream(ja + beg[p] + k), xv);
#pragma unroll
            for (int j = 0; j < K; ++j)
                acc[p][j] += av * xv[j];
        }
#pragma unroll
    for (int p = 0; p < P; ++p) {
#pragma unroll
        for (int j = 0; j < K; ++j)
            acc[p][j] = group_sum<G>(acc[p][j]);
        double bj[K], xj[K]; /* every lane takes part in the moves */
        amg_collect<G, K, YS>(bo[p], bj);
        if (SMOOTH)
            amg_collect<G, K, YS>(xo[p], xj);
        const long long row = rbase + p * RPP;
        if (sub == 0 && mine[p]) {
            double *yr = OUT + row * ldo;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const double v = SMOOTH ? amg_sweep_of(xj[j], wv[p], bj[j],
                                                       acc[p][j])
                                        : amg_resid_of(bj[j], acc[p][j]);
                __builtin_nontemporal_store(v, yr + j);
            }
        }
    }
}

/* passes per K (independent rows, so free: the bits do not depend on it) */
template <int K> struct amg_shape {
    static constexpr int P = K <= 4 ? 4 : 2;
};

template <int G, int K>
static void amg_sweep_gk(const spmv_csr_dev *A, int threads, bool smooth,
                         const double *X, int64_t ldx, const double *B,
                         int64_t ldb, const double *W, double *OUT, int64_t ldo,
                         hipStream_t s) {
    constexpr int P = amg_shape<K>::P;
    const int rows_per_wave = P * (WAVE / G);
    const long long waves = ((long long)A->M + rows_per_wave - 1) / rows_per_wave;
    const long long wpb = threads / WAVE;
    unsigned grid = (unsigned)((waves + wpb - 1) / wpb);
    if (A->order == 2)
        grid = grouped_grid(grid);
    if (smooth)
        hipLaunchKernelGGL((k_amg_sweep<G, P, K, true>), dim3(grid),
                           dim3(threads), 0, s, A->M, A->order, A->irp, A->ja,
                           A->as, X, ldx, B, ldb, W, OUT, ldo);
    else
        hipLaunchKernelGGL((k_amg_sweep<G, P, K, false>), dim3(grid),
                           dim3(threads), 0, s, A->M, A->order, A->irp, A->ja,
                           A->as, X, ldx, B, ldb, W, OUT, ldo);
}

template <int G>
static void amg_sweep_g(const spmv_csr_dev *A, int threads, int k, bool smooth,
                        const double *X, int64_t ldx, const double *B,
                        int64_t ldb, const double *W, double *OUT, int64_t ldo,
                        hipStream_t s) {
#define CALL(KK)                                                              \
    case KK:                                                                  \
        amg_sweep_gk<G, KK>(A, threads, smooth, X, ldx, B, ldb, W, OUT, ldo,  \
                            s);                                               \
        break;
    switch (k) {
        CALL(1) CALL(2) CALL(3) CALL(4) CALL(5) CALL(6) CALL(7)
    default:
        amg_sweep_gk<G, 8>(A, threads, smooth, X, ldx, B, ldb, W, OUT, ldo, s);
        break;
    }
#undef CALL
}

bool amg_sweep_fusable(const spmv_csr_dev *A) {
    return A->n_long_rb == 0 && A->value_bytes == 8;
}

/* OUT = rn(X + rn(w rn(B - A X))) (W != NULL) or rn(B - A X) (W NULL), k in
 * 1..8, OUT apart from X; the caller has checked amg_sweep_fusable(A).  The
 * lane group is launch_multi's choice for the handle (pick_group, group 0) */
void amg_sweep_dev(const spmv_csr_dev *A, int waves, int k, const double *X,
                   int64_t ldx, const double *B, int64_t ldb, const double *W,
                   double *OUT, int64_t ldo, hipStream_t s) {
    const int threads = waves * WAVE;
    const bool smooth = W != NULL;
#define CALL_G(GG)                                                            \
    amg_sweep_g<GG>(A, threads, k, smooth, X, ldx, B, ldb, W, OUT, ldo, s)
    switch (pick_group(A, 0)) {
    case 2:
        CALL_G(2);
        break;
    case 4:
        CALL_G(4);
        break;
    case 8:
        CALL_G(8);
        break;
    case 16:
        CALL_G(16);
        break;
    default:
        CALL_G(32);
        break;
    }
#undef CALL_G
}
