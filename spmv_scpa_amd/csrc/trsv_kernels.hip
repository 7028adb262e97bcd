/*
 * trsv_kernels.hip -- level-scheduled sparse triangular solve T x = b on the
 * chosen triangle of a CSR handle (spmv_csr_trsv_analyse, spmv_trsv_solve;
 * spmv_engine.h), gfx950 (wave64).  The launch list: trsv_plan.h.
 *
 * ANALYSIS (blocks; every array it leaves in the plan is defined to the byte):
 *   k_trsv_count   one lane per row, in stored order: the number of strict
 *                  entries, the fp64 sum of the entries on the diagonal, a
 *                  flag for a column outside [0, M)
 *   scan, k_trsv_fill   the strict pattern S in row order (column, position
 *                  in A)
 *   csr_transpose_dev(S)   the successor lists: row c of S^T holds the rows
 *                  that wait for c, one entry per stored dependency
 *   Kahn           k_trsv_kahn_init puts the rows without a strict entry into
 *                  the first frontier; k_trsv_kahn_step, ONE launch per level,
 *                  takes one from the counter of every successor of every
 *                  frontier row (integer atomics), stamps level = l + 1 on the
 *                  counter that reaches zero and appends that row to the next
 *                  frontier.  The ORDER inside a frontier comes from an atomic
 *                  and may vary; nothing below reads it: `level` is a pure
 *                  function of the pattern.  The host reads the frontier's
 *                  size back once per level and stops at max_levels: no
 *                  device loop is unbounded.
 *   csr_transpose_dev(M x levels, one entry per row at column level[i])
 *                  its JA is `order` (the stable sort of the rows by level),
 *                  its IRP is level_ptr
 *   scan, k_trsv_gather   the strict entries of row order[p] at position p,
 *                  values moved as raw bits
 *
 * SOLVE: trsv_row below is the result contract of spmv_trsv_solve -- G slots
 * per row, lane g adds rn(a_e * x) for e = g, g + G, ... in order, the
 * group_sum tree, rn(rhs - s), a correctly rounded division; contraction off:
 * every operation is rounded once.  k_trsv_wide runs ONE level over a grid,
 * k_trsv_chain runs a run of thin levels in ONE workgroup with a workgroup
 * barrier between levels.  Both call the same trsv_row, so the bits do not
 * depend on which kernel ran a level, on the workgroup size or on K.
 *
 * There is NO waiting between workgroups: a row's dependencies were written by
 * an earlier kernel of the stream (wide) or by this workgroup before the last
 * barrier (chain: producer and consumer share the CU's vector L1, workgroup
 * scope suffices).  X is read and written through one plain, non-restrict
 * pointer: vector loads only, never the scalar cache, never non-temporal.
 *
 * SWEEP PLANS (spmv_csr_trsv_analyse_sweeps): the analysis stops after
 * k_trsv_fill -- the strict entries stay in row order, one level, no Kahn pass
 * -- and the solve is `sweeps` launches over all rows, k_trsv_first and then
 * k_trsv_sweep, by the route of trsv_plan.h (further down).
 */
#include <algorithm>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "csr_build.h"
#include "trsv_plan.h"

#define TV_T 256 /* lanes of an analysis workgroup */
#define TV_G TRSV_GROUP

static_assert((TV_G & (TV_G - 1)) == 0 && TV_G >= 2 && TV_G <= WAVE,
              "group_sum: a power of two inside a wavefront");
static_assert(TRSV_THREADS % WAVE == 0 && TRSV_THREADS <= 1024 &&
                  TRSV_WIDE_THREADS % WAVE == 0,
              "workgroup sizes");

/* ------------------------------------------------------------------ */
/* analysis                                                             */
/* ------------------------------------------------------------------ */

__device__ __forceinline__ bool trsv_strict(int c, int i, int upper) {
    return upper ? c > i : c < i;
}

template <typename V>
__global__ void __launch_bounds__(TV_T)
k_trsv_count(int M, int upper, const int *__restrict__ irp,
             const int *__restrict__ ja, const V *__restrict__ as,
             int *__restrict__ cnt, double *__restrict__ diag,
             unsigned *__restrict__ flag,
             unsigned long long *__restrict__ zero_diag) {
    const int64_t i = (int64_t)blockIdx.x * TV_T + threadIdx.x;
    if (i >= M)
        return;
    int n = 0;
    double d = 0.0;
    bool bad = false;
    for (int64_t e = irp[i], end = irp[i + 1]; e < end; ++e) {
        const int c = ja[e];
        if ((unsigned)c >= (unsigned)M)
            bad = true;
        else if (c == (int)i)
            d += widen(as[e]);
        else if (trsv_strict(c, (int)i, upper))
            ++n;
    }
    cnt[i] = n;
    diag[i] = d;
    if (bad)
        atomicOr(flag, CSR_BAD_COLUMN);
    if (d == 0.0)
        atomicAdd(zero_diag, 1ull); /* a COUNT: any order of arrival */
}

/* sptr: cnt scanned.  Only after k_trsv_count found every column inside */
__global__ void __launch_bounds__(TV_T)
k_trsv_fill(int M, int upper, const int *__restrict__ irp,
            const int *__restrict__ ja, const int *__restrict__ sptr,
            int *__restrict__ sja, int *__restrict__ spos) {
    const int64_t i = (int64_t)blockIdx.x * TV_T + threadIdx.x;
    if (i >= M)
        return;
    int64_t at = sptr[i];
    const int64_t stop = sptr[i + 1]; /* never written past: the same count */
    for (int64_t e = irp[i], end = irp[i + 1]; e < end && at < stop; ++e) {
        const int c = ja[e];
        if ((unsigned)c < (unsigned)M && trsv_strict(c, (int)i, upper)) {
            sja[at] = c;
            spos[at] = (int)e;
            ++at;
        }
    }
}

__global__ void __launch_bounds__(TV_T)
k_trsv_kahn_init(int M, const int *__restrict__ sptr, int *__restrict__ indeg,
                 int *__restrict__ level, int *__restrict__ iota,
                 int *__restrict__ frontier, int *__restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * TV_T + threadIdx.x;
    if (i > M)
        return;
    iota[i] = (int)i; /* M + 1 of them */
    if (i == M)
        return;
    const int n = sptr[i + 1] - sptr[i];
    indeg[i] = n;
    level[i] = 0;
    if (n == 0) {
        const int at = atomicAdd(count, 1);
        if (at < M)
            frontier[at] = (int)i;
    }
}

/* the nf rows of level `next_level - 1`: every stored dependency on them is
 * taken off its row's counter; a row is appended exactly once, by the arrival
 * that finds 1, so at most M rows are ever appended */
__global__ void __launch_bounds__(TV_T)
k_trsv_kahn_step(int M, const int *__restrict__ frontier, int nf,
                 const int *__restrict__ succ_ptr,
                 const int *__restrict__ succ, int *__restrict__ indeg,
                 int *__restrict__ level, int next_level,
                 int *__restrict__ next, int *__restrict__ next_count,
                 int *__restrict__ clear_count) {
    const int64_t t = (int64_t)blockIdx.x * TV_T + threadIdx.x;
    if (t == 0)
        *clear_count = 0; /* the counter of the level after the next */
    if (t >= nf)
        return;
    const int r = frontier[t];
    for (int64_t e = succ_ptr[r], end = succ_ptr[r + 1]; e < end; ++e) {
        const int w = succ[e];
        if (atomicSub(indeg + w, 1) == 1) {
            level[w] = next_level;
            const int at = atomicAdd(next_count, 1);
            if (at < M)
                next[at] = w;
        }
    }
}

/* rowptr[p] = strict entries of row order[p] (scanned afterwards) */
__global__ void __launch_bounds__(TV_T)
k_trsv_newcnt(int M, const int *__restrict__ order,
              const int *__restrict__ sptr, int *__restrict__ rowptr) {
    const int64_t p = (int64_t)blockIdx.x * TV_T + threadIdx.x;
    if (p >= M)
        return;
    const int r = order[p];
    rowptr[p] = sptr[r + 1] - sptr[r];
}

/* U: the value as raw bits, moved and never computed */
template <typename U>
__global__ void __launch_bounds__(TV_T)
k_trsv_gather(int M, const int *__restrict__ order,
              const int *__restrict__ sptr, const int *__restrict__ sja,
              const int *__restrict__ spos, const U *__restrict__ as,
              const int *__restrict__ rowptr, int *__restrict__ ja_out,
              U *__restrict__ as_out) {
    const int64_t p = (int64_t)blockIdx.x * TV_T + threadIdx.x;
    if (p >= M)
        return;
    const int r = order[p];
    const int64_t src = sptr[r], dst = rowptr[p];
    const int64_t n = min(sptr[r + 1] - sptr[r], rowptr[p + 1] - rowptr[p]);
    for (int64_t j = 0; j < n; ++j) {
        ja_out[dst + j] = sja[src + j];
        as_out[dst + j] = as[spos[src + j]];
    }
}

/* device scratch of one analysis: freed on every path */
struct trsv_scratch {
    std::vector<void *> blocks;
    ~trsv_scratch() {
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

/* an array the plan keeps; counted in P->bytes */
template <typename T>
static hipError_t trsv_keep(spmv_trsv_plan *P, T **out, int64_t count,
                            size_t item = sizeof(T)) {
    const size_t bytes = (size_t)(count > 0 ? count : 1) * item;
    const hipError_t e = hipMalloc((void **)out, bytes);
    if (e == hipSuccess)
        P->bytes += (int64_t)bytes;
    return e;
}

void trsv_free_dev(spmv_trsv_plan *P) {
    (void)hipFree(P->level);
    (void)hipFree(P->order);
    (void)hipFree(P->level_ptr);
    (void)hipFree(P->rowptr);
    (void)hipFree(P->ja);
    (void)hipFree(P->as);
    (void)hipFree(P->diag);
    (void)hipFree(P->sweep_buf[0]);
    (void)hipFree(P->sweep_buf[1]);
    free(P->h_level_ptr);
    free(P->segs);
    P->level = P->order = P->level_ptr = P->rowptr = P->ja = NULL;
    P->as = NULL;
    P->diag = NULL;
    P->sweep_buf[0] = P->sweep_buf[1] = NULL;
    P->h_level_ptr = NULL;
    P->segs = NULL;
}

/* order[i] = i, level[i] = 0: the one level of a sweep plan */
__global__ void __launch_bounds__(TV_T)
k_trsv_natural(int M, int *__restrict__ order, int *__restrict__ level) {
    const int64_t i = (int64_t)blockIdx.x * TV_T + threadIdx.x;
    if (i >= M)
        return;
    order[i] = (int)i;
    level[i] = 0;
}

/* sweeps > 0: a sweep plan (kmax right-hand sides at most) -- the strict
 * entries stay in row order, there is no Kahn pass and max_levels is not read */
int trsv_analyse_dev(const spmv_csr_dev *A, int uplo, int unit, int max_levels,
                     int sweeps, int kmax, spmv_trsv_plan *P, hipStream_t s) {
    int rc = 0;
    const int M = A->M;
    trsv_scratch scratch;
    trsv_sizes z;
    int *cnt = NULL, *sja = NULL, *spos = NULL, *succ_ptr = NULL, *succ = NULL,
        *succ_pos = NULL, *indeg = NULL, *frontier = NULL, *counters = NULL,
        *iota = NULL, *sums = NULL;
    unsigned long long *d_zero = NULL;
    unsigned long long zero = 0;
    int head[4] = {0, 0, 0, 0}; /* counters as the host reads them */
    int snz = 0, levels = 0, nf = 0;
    int64_t placed = 0;
    P->M = M;
    P->uplo = uplo;
    P->unit = unit;
    P->value_bytes = A->value_bytes;
    P->device = A->device;
    P->sweeps = sweeps;
    P->kmax = sweeps ? kmax : 0;
    (void)hipGetLastError(); /* an earlier caller's unread error is not ours */
    HIP_TRY(trsv_keep(P, &P->level_ptr, 1)); /* grown below once levels is known */
    if (M == 0) {
        HIP_TRY(hipMemsetAsync(P->level_ptr, 0, sizeof(int), s));
        HIP_TRY(hipStreamSynchronize(s));
        P->h_level_ptr = (int *)calloc(1, sizeof(int));
        return P->h_level_ptr ? 0 : -ENOMEM;
    }
    rc = trsv_sizes_make(M, A->NZ, 0, &z);
    if (rc)
        return rc;
    HIP_TRY(trsv_keep(P, &P->level, M));
    HIP_TRY(trsv_keep(P, &P->order, M));
    HIP_TRY(trsv_keep(P, &P->rowptr, (int64_t)M + 1));
    HIP_TRY(trsv_keep(P, &P->diag, z.diag));
    HIP_TRY(scratch.get(&cnt, z.cnt));
    HIP_TRY(scratch.get(&counters, z.counters));
    HIP_TRY(scratch.get(&d_zero, 1));
    HIP_TRY(scratch.get(&sums, transpose_scan_tiles((int64_t)M + 1)));
    HIP_TRY(hipMemsetAsync(cnt, 0, (size_t)z.cnt * sizeof(int), s));
    HIP_TRY(hipMemsetAsync(counters, 0, (size_t)z.counters * sizeof(int), s));
    HIP_TRY(hipMemsetAsync(d_zero, 0, sizeof(unsigned long long), s));
    if (A->value_bytes == 4)
        hipLaunchKernelGGL((k_trsv_count<float>), grid_for(M, TV_T), dim3(TV_T),
                           0, s, M, uplo, A->irp, A->ja, A->as32, cnt, P->diag,
                           (unsigned *)(counters + 3), d_zero);
    else
        hipLaunchKernelGGL((k_trsv_count<double>), grid_for(M, TV_T),
                           dim3(TV_T), 0, s, M, uplo, A->irp, A->ja, A->as, cnt,
                           P->diag, (unsigned *)(counters + 3), d_zero);
    tr_scan(cnt, z.cnt, sums, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&snz, cnt + M, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(head, counters, sizeof head, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&zero, d_zero, sizeof zero, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    /* a column outside [0, M): nothing was written for it */
    rc = csr_flags_errno((unsigned)head[3]);
    if (rc)
        goto fail;
    if (snz < 0 || snz > A->NZ) {
        rc = -EIO;
        goto fail;
    }
    P->entries = snz;
    P->zero_diag = (int64_t)zero;
    rc = trsv_sizes_make(M, A->NZ, snz, &z);
    if (rc)
        goto fail;
    HIP_TRY(trsv_keep(P, &P->ja, z.sja));
    HIP_TRY(trsv_keep(P, (char **)&P->as, z.sja, (size_t)A->value_bytes));
    HIP_TRY(scratch.get(&sja, z.sja));
    HIP_TRY(scratch.get(&spos, z.spos));
    hipLaunchKernelGGL(k_trsv_fill, grid_for(M, TV_T), dim3(TV_T), 0, s, M,
                       uplo, A->irp, A->ja, cnt, sja, spos);
    HIP_TRY(hipGetLastError());
    if (sweeps) { /* one level of M rows, the identity order, cnt is rowptr */
        (void)hipFree(P->level_ptr);
        P->level_ptr = NULL;
        P->bytes -= (int64_t)sizeof(int);
        HIP_TRY(trsv_keep(P, &P->level_ptr, 2));
        for (int b = 0; b < trsv_sweep_scratch(sweeps); ++b)
            HIP_TRY(trsv_keep(P, &P->sweep_buf[b], (int64_t)kmax * M));
        P->h_level_ptr = (int *)malloc(2 * sizeof(int));
        if (!P->h_level_ptr) {
            rc = -ENOMEM;
            goto fail;
        }
        P->h_level_ptr[0] = 0;
        P->h_level_ptr[1] = M;
        P->levels = 1;
        P->widest_level = M;
        HIP_TRY(hipMemcpyAsync(P->level_ptr, P->h_level_ptr, 2 * sizeof(int),
                               hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(P->rowptr, cnt, ((size_t)M + 1) * sizeof(int),
                               hipMemcpyDeviceToDevice, s));
        hipLaunchKernelGGL(k_trsv_natural, grid_for(M, TV_T), dim3(TV_T), 0, s,
                           M, P->order, P->level);
        goto gather;
    }
    HIP_TRY(scratch.get(&succ_ptr, z.succ_ptr));
    HIP_TRY(scratch.get(&succ, z.succ));
    HIP_TRY(scratch.get(&succ_pos, z.succ));
    HIP_TRY(scratch.get(&indeg, z.indeg));
    HIP_TRY(scratch.get(&frontier, z.frontier));
    HIP_TRY(scratch.get(&iota, z.iota));
    { /* the successor lists: S^T, the positions riding as 4-byte values */
        spmv_csr_dev S, ST;
        memset(&S, 0, sizeof S);
        memset(&ST, 0, sizeof ST);
        S.M = S.N = M;
        S.NZ = snz;
        S.value_bytes = 4;
        S.irp = cnt;
        S.ja = sja;
        S.as32 = (float *)spos;
        ST.M = ST.N = M;
        ST.NZ = snz;
        ST.value_bytes = 4;
        ST.irp = succ_ptr;
        ST.ja = succ;
        ST.as32 = (float *)succ_pos;
        rc = csr_transpose_dev(&S, &ST, s);
        if (rc)
            goto fail;
    }
    /* Kahn: one launch and one read-back per level */
    hipLaunchKernelGGL(k_trsv_kahn_init, grid_for((int64_t)M + 1, TV_T),
                       dim3(TV_T), 0, s, M, cnt, indeg, P->level, iota,
                       frontier, counters);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&nf, counters, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    while (nf > 0) {
        if (levels >= max_levels) {
            rc = -E2BIG;
            goto fail;
        }
        if (nf > M - placed) {
            rc = -EIO; /* more rows than there are: not a frontier of ours */
            goto fail;
        }
        placed += nf;
        int *const from = frontier + (int64_t)(levels & 1) * M;
        int *const to = frontier + (int64_t)((levels + 1) & 1) * M;
        hipLaunchKernelGGL(k_trsv_kahn_step, grid_for(nf, TV_T), dim3(TV_T), 0,
                           s, M, from, nf, succ_ptr, succ, indeg, P->level,
                           levels + 1, to, counters + (levels + 1) % 3,
                           counters + (levels + 2) % 3);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&nf, counters + (levels + 1) % 3, sizeof(int),
                               hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        ++levels;
    }
    if (placed != M) {
        rc = -EIO; /* a strict triangle has no cycle: every row is placed */
        goto fail;
    }
    P->levels = levels;
    /* order, level_ptr: the transpose of the M x levels matrix with row i's
     * one entry at column level[i] */
    (void)hipFree(P->level_ptr);
    P->level_ptr = NULL;
    P->bytes -= (int64_t)sizeof(int);
    HIP_TRY(trsv_keep(P, &P->level_ptr, (int64_t)levels + 1));
    {
        spmv_csr_dev L, LT;
        memset(&L, 0, sizeof L);
        memset(&LT, 0, sizeof LT);
        L.M = M;
        L.N = levels;
        L.NZ = M;
        L.value_bytes = 4;
        L.irp = iota;
        L.ja = P->level;
        L.as32 = (float *)indeg; /* any M words: moved and never read */
        LT.M = levels;
        LT.N = M;
        LT.NZ = M;
        LT.value_bytes = 4;
        LT.irp = P->level_ptr;
        LT.ja = P->order;
        LT.as32 = (float *)frontier;
        rc = csr_transpose_dev(&L, &LT, s);
        if (rc)
            goto fail;
    }
    /* the copy: rows of one level contiguous */
    HIP_TRY(hipMemsetAsync(P->rowptr + M, 0, sizeof(int), s));
    hipLaunchKernelGGL(k_trsv_newcnt, grid_for(M, TV_T), dim3(TV_T), 0, s, M,
                       P->order, cnt, P->rowptr);
    tr_scan(P->rowptr, (int64_t)M + 1, sums, s);
gather:
    if (A->value_bytes == 4)
        hipLaunchKernelGGL((k_trsv_gather<uint32_t>), grid_for(M, TV_T),
                           dim3(TV_T), 0, s, M, P->order, cnt, sja, spos,
                           (const uint32_t *)A->as32, P->rowptr, P->ja,
                           (uint32_t *)P->as);
    else
        hipLaunchKernelGGL((k_trsv_gather<uint64_t>), grid_for(M, TV_T),
                           dim3(TV_T), 0, s, M, P->order, cnt, sja, spos,
                           (const uint64_t *)A->as, P->rowptr, P->ja,
                           (uint64_t *)P->as);
    HIP_TRY(hipGetLastError());
    if (sweeps) {
        HIP_TRY(hipStreamSynchronize(s));
        return 0;
    }
    P->h_level_ptr = (int *)malloc(((size_t)levels + 1) * sizeof(int));
    if (!P->h_level_ptr) {
        rc = -ENOMEM;
        goto fail;
    }
    HIP_TRY(hipMemcpyAsync(P->h_level_ptr, P->level_ptr,
                           ((size_t)levels + 1) * sizeof(int),
                           hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    {
        for (int l = 0; l < levels; ++l)
            P->widest_level = std::max(
                P->widest_level, P->h_level_ptr[l + 1] - P->h_level_ptr[l]);
        const int64_t n = trsv_segments(P->h_level_ptr, levels, TRSV_SMALL_ROWS,
                                        NULL, 0);
        if (n < 0 || n > INT32_MAX || P->h_level_ptr[levels] != M) {
            rc = -EIO;
            goto fail;
        }
        P->segs = (trsv_segment *)malloc((size_t)(n > 0 ? n : 1) *
                                         sizeof(trsv_segment));
        if (!P->segs) {
            rc = -ENOMEM;
            goto fail;
        }
        P->n_segs = (int)trsv_segments(P->h_level_ptr, levels, TRSV_SMALL_ROWS,
                                       P->segs, n);
    }
fail:
    if (rc) /* nothing of ours is left running when the scratch is freed */
        (void)hipStreamSynchronize(s);
    return rc;
}

/* ------------------------------------------------------------------ */
/* solve                                                                */
/* ------------------------------------------------------------------ */

/* X[c * ldx + 0 .. K): K plain 8-byte loads the compiler pairs into 16-byte
 * ones (multi_kernels.hip: load_xrow), through the pointer X is written by */
template <int K>
__device__ __forceinline__ void trsv_load(const double *X, int64_t ldx, int c,
                                          double (&xv)[K]) {
    const double *p = X + (int64_t)c * ldx;
#pragma unroll
    for (int j = 0; j < K; ++j)
        xv[j] = p[j];
}

/*
 * Position p of the plan (row order[p]) by the TV_G lanes `sub` = 0 .. G - 1
 * of one lane group; `live` = false: the lanes only take part in the moves of
 * the sum.  THE RESULT CONTRACT (spmv_engine.h), every operation rounded once.
 * The gathers read Xin, the row is stored to Xout: the level kernels pass their
 * one X for both, a Jacobi sweep (below) the previous iterate and the next.
 * NATURAL: the position is the row and `order` is not read (sweep plans).
 */
template <int K, typename V, bool NATURAL = false>
__device__ __forceinline__ void
trsv_row(bool live, int64_t p, int sub, int unit, const int *__restrict__ order,
         const int *__restrict__ rowptr, const int *__restrict__ ja,
         const V *__restrict__ as, const double *__restrict__ diag,
         const double *__restrict__ scale, const double *B, int64_t ldb,
         const double *Xin, int64_t ldin, double *Xout, int64_t ldout) {
#pragma clang fp contract(off)
    int row = 0, beg = 0, n = 0;
    if (live) {
        row = NATURAL ? (int)p : order[p];
        beg = rowptr[p];
        n = rowptr[p + 1] - beg;
    }
    /* the right-hand side, the diagonal and the scale need none of X: in
     * flight over the walk */
    double rhs[K], d = 1.0, sc = 1.0;
    const bool writer = live && sub == 0;
#pragma unroll
    for (int j = 0; j < K; ++j)
        rhs[j] = 0.0;
    if (writer) {
        trsv_load<K>(B, ldb, row, rhs);
        if (!unit)
            d = diag[row];
        if (scale)
            sc = scale[row];
    }
    double acc[K];
#pragma unroll
    for (int j = 0; j < K; ++j)
        acc[j] = 0.0;
    ja += beg;
    as += beg;
    int k = sub;
    for (; k + TV_G < n; k += 2 * TV_G) { /* two entries in flight */
        const int c0 = ld_stream(ja + k), c1 = ld_stream(ja + k + TV_G);
        const V a0 = ld_stream(as + k), a1 = ld_stream(as + k + TV_G);
        double x0[K], x1[K];
        trsv_load<K>(Xin, ldin, c0, x0);
        trsv_load<K>(Xin, ldin, c1, x1);
        const double w0 = widen(a0), w1 = widen(a1);
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const double t = w0 * x0[j];
            acc[j] = acc[j] + t;
        }
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const double t = w1 * x1[j];
            acc[j] = acc[j] + t;
        }
    }
    if (k < n) {
        const int c0 = ld_stream(ja + k);
        const double w0 = widen(ld_stream(as + k));
        double x0[K];
        trsv_load<K>(Xin, ldin, c0, x0);
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const double t = w0 * x0[j];
            acc[j] = acc[j] + t;
        }
    }
#pragma unroll
    for (int j = 0; j < K; ++j)
        acc[j] = group_sum<TV_G>(acc[j]); /* every lane takes part */
    if (writer) {
        double *xr = Xout + (int64_t)row * ldout;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            double r = rhs[j];
            if (scale)
                r = sc * r;
            double t = r - acc[j];
            if (!unit)
                t = t / d;
            xr[j] = t;
        }
    }
}

/* one level: positions [first, end) of the plan, G lanes each */
template <int K, typename V>
__global__ void __launch_bounds__(1024)
k_trsv_wide(int first, int end, int unit, const int *__restrict__ order,
            const int *__restrict__ rowptr, const int *__restrict__ ja,
            const V *__restrict__ as, const double *__restrict__ diag,
            const double *__restrict__ scale, const double *B, int64_t ldb,
            double *X, int64_t ldx) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t p = first + t / TV_G;
    trsv_row<K, V>(p < end, p, (int)(threadIdx.x & (TV_G - 1)), unit, order,
                   rowptr, ja, as, diag, scale, B, ldb, X, ldx, X, ldx);
}

/* levels l0 .. l1 by ONE workgroup: the loop bounds are workgroup-uniform, so
 * every lane reaches every barrier */
template <int K, typename V>
__global__ void __launch_bounds__(1024)
k_trsv_chain(int l0, int l1, int unit, const int *__restrict__ level_ptr,
             const int *__restrict__ order, const int *__restrict__ rowptr,
             const int *__restrict__ ja, const V *__restrict__ as,
             const double *__restrict__ diag, const double *__restrict__ scale,
             const double *B, int64_t ldb, double *X, int64_t ldx) {
    const int rows = blockDim.x / TV_G;
    const int mine = threadIdx.x / TV_G, sub = threadIdx.x & (TV_G - 1);
    for (int l = l0; l <= l1; ++l) {
        const int beg = level_ptr[l], end = level_ptr[l + 1];
        for (int64_t base = beg; base < end; base += rows) {
            const int64_t p = base + mine;
            trsv_row<K, V>(p < end, p, sub, unit, order, rowptr, ja, as, diag,
                           scale, B, ldb, X, ldx, X, ldx);
        }
        __syncthreads(); /* the level's X is visible to the workgroup */
    }
}

/*
 * SWEEP PLANS (spmv_csr_trsv_analyse_sweeps): x(1) = D^-1 b, x(m) = D^-1 (b -
 * S x(m-1)).  Every sweep is ONE launch over all M rows that reads only what
 * the launch before it wrote: no waiting between workgroups, no atomics.
 *
 * k_trsv_first: trsv_row with s = +0.0, so the matrix is not read and the sweep
 * is elementwise.  Lanes run over the M * k elements, not over the rows (the
 * tile of cg_common.h): a wavefront's load is 512 consecutive bytes at ld = k.
 * Nothing is kept per column, so k is an argument and the kernel exists once:
 * the workgroup's first element is split into row and column once (uniform),
 * a lane then divides a number below blockDim + k.  Each lane reads its own B
 * before it stores: Xout may be B.
 */
__global__ void __launch_bounds__(1024)
k_trsv_first(int M, int k, int unit, const double *__restrict__ diag,
             const double *__restrict__ scale, const double *B, int64_t ldb,
             double *Xout, int64_t ldout) {
#pragma clang fp contract(off)
    const int64_t f0 = (int64_t)blockIdx.x * blockDim.x;
    const unsigned at = (unsigned)(f0 % k) + threadIdx.x;
    const int64_t row = f0 / k + at / (unsigned)k;
    const int j = (int)(at % (unsigned)k);
    if (row >= M)
        return;
    double r = B[row * ldb + j];
    if (scale)
        r = scale[row] * r;
    double zero = 0.0; /* opaque: the subtraction trsv_row does is done here
                          too (it quietens a signalling NaN), never folded */
    asm volatile("" : "+v"(zero));
    double t = r - zero;
    if (!unit)
        t = t / diag[row];
    Xout[row * ldout + j] = t;
}

/*
 * Row `row` of a sweep by L < G lanes, for plans of short rows (trsv_plan.h:
 * trsv_sweep_lanes; on two strict entries a row G lanes leave six idle and a
 * sweep ran 2 - 3x slower, profiles/trsv_sweeps.md).  The G slots are the
 * contract, the lanes are not: lane `sub` owns the slots sub, sub + L, .., one
 * accumulator each, adds the same products in the same order, and the halving
 * tree runs inside the lane down to h = L and across the L lanes below it --
 * the same additions of the same operands as trsv_row, so the same bits.
 */
template <int K, typename V, int L>
__device__ __forceinline__ void
trsv_row_few(bool live, int64_t row, int sub, int unit,
             const int *__restrict__ rowptr, const int *__restrict__ ja,
             const V *__restrict__ as, const double *__restrict__ diag,
             const double *__restrict__ scale, const double *B, int64_t ldb,
             const double *Xin, int64_t ldin, double *Xout, int64_t ldout) {
#pragma clang fp contract(off)
    constexpr int S = TV_G / L; /* slots of one lane */
    int beg = 0, n = 0;
    if (live) {
        beg = rowptr[row];
        n = rowptr[row + 1] - beg;
    }
    double rhs[K], d = 1.0, sc = 1.0;
    const bool writer = live && sub == 0;
#pragma unroll
    for (int j = 0; j < K; ++j)
        rhs[j] = 0.0;
    if (writer) {
        trsv_load<K>(B, ldb, (int)row, rhs);
        if (!unit)
            d = diag[row];
        if (scale)
            sc = scale[row];
    }
    double acc[S][K];
#pragma unroll
    for (int t = 0; t < S; ++t)
#pragma unroll
        for (int j = 0; j < K; ++j)
            acc[t][j] = 0.0;
    ja += beg;
    as += beg;
    for (int q0 = 0; q0 < n; q0 += TV_G) { /* one round of the G slots */
#pragma unroll
        for (int t = 0; t < S; ++t) {
            const int q = q0 + sub + t * L; /* slot sub + t L */
            if (q < n) {
                const int c = ld_stream(ja + q);
                const double w = widen(ld_stream(as + q));
                double x[K];
                trsv_load<K>(Xin, ldin, c, x);
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    const double p = w * x[j];
                    acc[t][j] = acc[t][j] + p;
                }
            }
        }
    }
#pragma unroll
    for (int h = S / 2; h >= 1; h /= 2) /* p[g] += p[g + h L], inside the lane */
#pragma unroll
        for (int t = 0; t < h; ++t)
#pragma unroll
            for (int j = 0; j < K; ++j)
                acc[t][j] = acc[t][j] + acc[t + h][j];
#pragma unroll
    for (int j = 0; j < K; ++j)
        acc[0][j] = group_sum<L>(acc[0][j]); /* h = L / 2 .. 1 */
    if (writer) {
        double *xr = Xout + row * ldout;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            double r = rhs[j];
            if (scale)
                r = sc * r;
            double t = r - acc[0][j];
            if (!unit)
                t = t / d;
            xr[j] = t;
        }
    }
}

/* sweep m > 1: row i by L = G or TRSV_FEW_LANES lanes, the gathers from the iterate the launch
 * before wrote (never written here), the row to Xout.  In the last sweep Xout
 * is the caller's X and may be B: a row's writer lane holds its rhs before it
 * stores, and no other lane reads that row of B */
template <int K, typename V, int L>
__global__ void __launch_bounds__(1024)
k_trsv_sweep(int M, int unit, const int *__restrict__ rowptr,
             const int *__restrict__ ja, const V *__restrict__ as,
             const double *__restrict__ diag, const double *__restrict__ scale,
             const double *B, int64_t ldb, const double *__restrict__ Xin,
             int64_t ldin, double *Xout, int64_t ldout) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = t / L;
    const int sub = (int)(threadIdx.x & (L - 1));
    if (L == TV_G)
        trsv_row<K, V, true>(i < M, i, sub, unit, NULL, rowptr, ja, as, diag,
                             scale, B, ldb, Xin, ldin, Xout, ldout);
    else
        trsv_row_few<K, V, L>(i < M, i, sub, unit, rowptr, ja, as, diag, scale,
                              B, ldb, Xin, ldin, Xout, ldout);
}

/* the sweeps of a sweep plan by the route of trsv_plan.h; the scratch has
 * ld = K, the caller saw K <= kmax */
template <int K, typename V>
static void trsv_launch_sweeps(const spmv_trsv_plan *P, int waves,
                               const double *B, int64_t ldb, double *X,
                               int64_t ldx, const double *scale,
                               hipStream_t s) {
    const int threads = waves > 0 ? waves * WAVE : TRSV_WIDE_THREADS;
    const V *as = (const V *)P->as;
    double *const buf[3] = {X, P->sweep_buf[0], P->sweep_buf[1]};
    const int64_t ld[3] = {ldx, K, K};
    const int lanes = trsv_sweep_lanes(P->M, P->entries);
    for (int m = 1; m <= P->sweeps; ++m) {
        const trsv_route r = trsv_sweep_route(P->sweeps, m);
        if (m == 1)
            hipLaunchKernelGGL(
                k_trsv_first,
                dim3((unsigned)trsv_ceil_div((int64_t)P->M * K, threads)),
                dim3(threads), 0, s, P->M, K, P->unit, P->diag, scale, B, ldb,
                buf[r.out], ld[r.out]);
        else if (lanes == TV_G)
            hipLaunchKernelGGL(
                (k_trsv_sweep<K, V, TV_G>),
                dim3((unsigned)trsv_sweep_grid(P->M, threads, lanes)),
                dim3(threads), 0, s, P->M, P->unit, P->rowptr, P->ja, as,
                P->diag, scale, B, ldb, buf[r.in], ld[r.in], buf[r.out],
                ld[r.out]);
        else
            hipLaunchKernelGGL(
                (k_trsv_sweep<K, V, TRSV_FEW_LANES>),
                dim3((unsigned)trsv_sweep_grid(P->M, threads, lanes)),
                dim3(threads), 0, s, P->M, P->unit, P->rowptr, P->ja, as,
                P->diag, scale, B, ldb, buf[r.in], ld[r.in], buf[r.out],
                ld[r.out]);
    }
}

template <int K, typename V>
static void trsv_launch(const spmv_trsv_plan *P, int waves, const double *B,
                        int64_t ldb, double *X, int64_t ldx,
                        const double *scale, hipStream_t s) {
    const int wide_t = waves > 0 ? waves * WAVE : TRSV_WIDE_THREADS;
    const int chain_t = waves > 0 ? waves * WAVE : TRSV_THREADS;
    const V *as = (const V *)P->as;
    for (int i = 0; i < P->n_segs; ++i) {
        const trsv_segment &g = P->segs[i];
        if (g.kind == TRSV_WIDE) {
            const int first = P->h_level_ptr[g.first_level];
            const int end = P->h_level_ptr[g.first_level + 1];
            hipLaunchKernelGGL(
                (k_trsv_wide<K, V>),
                dim3((unsigned)trsv_wide_grid(end - first, wide_t)),
                dim3(wide_t), 0, s, first, end, P->unit, P->order, P->rowptr,
                P->ja, as, P->diag, scale, B, ldb, X, ldx);
        } else {
            hipLaunchKernelGGL((k_trsv_chain<K, V>), dim3(1), dim3(chain_t), 0,
                               s, g.first_level, g.last_level, P->unit,
                               P->level_ptr, P->order, P->rowptr, P->ja, as,
                               P->diag, scale, B, ldb, X, ldx);
        }
    }
}

template <typename V>
static void trsv_launch_k(const spmv_trsv_plan *P, int waves, int k,
                          const double *B, int64_t ldb, double *X, int64_t ldx,
                          const double *scale, hipStream_t s) {
    switch (k) {
#define TRSV_CASE(K)                                                          \
    case K:                                                                   \
        if (P->sweeps)                                                        \
            trsv_launch_sweeps<K, V>(P, waves, B, ldb, X, ldx, scale, s);     \
        else                                                                  \
            trsv_launch<K, V>(P, waves, B, ldb, X, ldx, scale, s);            \
        break;
        TRSV_CASE(1)
        TRSV_CASE(2)
        TRSV_CASE(3)
        TRSV_CASE(4)
        TRSV_CASE(5)
        TRSV_CASE(6)
        TRSV_CASE(7)
        TRSV_CASE(8)
#undef TRSV_CASE
    }
}

int trsv_solve_dev(const spmv_trsv_plan *P, int waves, int k, const double *B,
                   int64_t ldb, double *X, int64_t ldx, const double *scale,
                   hipStream_t s) {
    if (P->value_bytes == 4)
        trsv_launch_k<float>(P, waves, k, B, ldb, X, ldx, scale, s);
    else
        trsv_launch_k<double>(P, waves, k, B, ldb, X, ldx, scale, s);
    return hip_errno(hipGetLastError());
}
