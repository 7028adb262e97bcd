/*
 * transpose_kernels.hip -- T = A^T of a CSR handle on the device
 * (spmv_csr_transpose, spmv_csr_symmetry; spmv_engine.h), gfx950 (wave64).
 *
 * The result is defined to the byte: the stable counting sort of A's entries,
 * in stored order, by column.  It is computed as a least-significant-digit
 * radix sort of the pairs (column, position in A) -- one algorithm, the same
 * for a matrix whose entries all sit in one column -- followed by one gather.
 * The geometry (passes, tile, workgroups, counters, scratch) is
 * transpose_plan.h's; every pass is three steps:
 *
 *   k_tr_hist     workgroup w counts the digits of its tile into
 *                 counter[digit * workgroups + w] (LDS integer atomics: a
 *                 COUNT does not depend on the order of arrival)
 *   scan          exclusive scan over the flattened counters (tr_scan of
 *                 csr_build.hip, which also turns the column counts into T's
 *                 IRP)
 *   k_tr_scatter  a key goes to counter[digit][w] + its stable rank among the
 *                 equal digits of the tile.  The tile is walked in strips of
 *                 one key per lane, in order; inside a wavefront the rank is
 *                 popcount(lanes below with the same digit), the match mask
 *                 built from digit_bits 64-bit ballots; wavefronts of a strip
 *                 are combined through per-wavefront digit counts in LDS,
 *                 strips through a running per-digit offset.
 *
 * No POSITION ever comes from the return value of an atomic, so the bytes of
 * T do not depend on scheduling.  The one global atomicAdd counts the entries
 * of each column (T's row lengths).
 *
 * Pass 0 reads A's JA with the position implicit; later passes ping-pong two
 * (key, position) buffers.  The gather reads the source row of position p from
 * a row index expanded out of A's IRP into the buffer the last pass left free
 * (measured against a binary search per sorted position: DESIGN.md
 * section 19) and moves the value as raw bits.
 *
 * Index arithmetic that can reach NZ or 2^digit_bits * workgroups is 64-bit;
 * positions and counts fit 32 bits because IRP is `int`.
 */
#include "csr_build.h"

#define TR_T TRANSPOSE_THREADS
#define TR_WAVES (TR_T / WAVE)
#define TR_RADIX TRANSPOSE_RADIX
#define TR_BITS TRANSPOSE_DIGIT_BITS

static_assert(TR_T == TR_RADIX, "k_tr_scatter: one thread per digit");

__device__ __forceinline__ unsigned tr_digit(unsigned key, int shift) {
    return (key >> shift) & (TR_RADIX - 1);
}

/* ------------------------------------------------------------------ */
/* the sort                                                             */
/* ------------------------------------------------------------------ */

/* cnt[c] += entries of column c (T's row lengths); a column outside [0, N)
 * is not counted and raises the flag: nothing is ever written outside cnt */
__global__ void __launch_bounds__(TR_T)
k_tr_colcount(const int *__restrict__ ja, int64_t NZ, int N,
              int *__restrict__ cnt, unsigned *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * TR_T + threadIdx.x;
    if (i >= NZ)
        return;
    const int c = ld_stream(ja + i);
    if ((unsigned)c < (unsigned)N)
        atomicAdd(cnt + c, 1);
    else
        atomicOr(flag, CSR_BAD_COLUMN);
}

/* FIRST: the keys are A's JA; else the .x of the pairs */
template <bool FIRST>
__device__ __forceinline__ unsigned tr_key(const int *__restrict__ ja,
                                           const uint2 *__restrict__ src,
                                           int64_t i) {
    if (FIRST)
        return (unsigned)ja[i];
    return src[i].x;
}

template <bool FIRST>
__global__ void __launch_bounds__(TR_T)
k_tr_hist(const int *__restrict__ ja, const uint2 *__restrict__ src,
          int64_t NZ, int shift, int64_t workgroups,
          int *__restrict__ counters) {
    __shared__ int cnt[TR_RADIX];
    const int tid = threadIdx.x;
    cnt[tid] = 0;
    __syncthreads();
    const int64_t begin = (int64_t)blockIdx.x * TRANSPOSE_TILE;
    const int64_t end = min(begin + (int64_t)TRANSPOSE_TILE, NZ);
    for (int64_t i = begin + tid; i < end; i += TR_T)
        atomicAdd(&cnt[tr_digit(tr_key<FIRST>(ja, src, i), shift)], 1);
    __syncthreads();
    counters[(int64_t)tid * workgroups + blockIdx.x] = cnt[tid];
}

/* `counters` scanned: counters[digit * workgroups + w] is where the first key
 * of tile w with that digit goes */
template <bool FIRST>
__global__ void __launch_bounds__(TR_T)
k_tr_scatter(const int *__restrict__ ja, const uint2 *__restrict__ src,
             int64_t NZ, int shift, int64_t workgroups,
             const int *__restrict__ counters, uint2 *__restrict__ dst) {
    __shared__ unsigned running[TR_RADIX];      /* next free slot per digit */
    __shared__ unsigned wcnt[TR_WAVES][TR_RADIX]; /* this strip, per wavefront */
    const int tid = threadIdx.x, wave = tid / WAVE;
    running[tid] = (unsigned)counters[(int64_t)tid * workgroups + blockIdx.x];
#pragma unroll
    for (int w = 0; w < TR_WAVES; ++w)
        wcnt[w][tid] = 0;
    __syncthreads();
    const int64_t begin = (int64_t)blockIdx.x * TRANSPOSE_TILE;
    const int64_t end = min(begin + (int64_t)TRANSPOSE_TILE, NZ);
    for (int64_t s0 = begin; s0 < end; s0 += TR_T) { /* workgroup-uniform */
        const int64_t i = s0 + tid;
        const bool valid = i < end;
        uint2 kp = make_uint2(0u, 0u);
        if (valid) {
            if (FIRST)
                kp = make_uint2((unsigned)ja[i], (unsigned)i);
            else
                kp = src[i];
        }
        const unsigned d = tr_digit(kp.x, shift);
        /* lanes of this wavefront that hold a key with my digit */
        unsigned long long mask = __ballot(valid);
#pragma unroll
        for (int b = 0; b < TR_BITS; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long bal = __ballot(bit);
            mask &= bit ? bal : ~bal;
        }
        const unsigned rank = lanes_below(mask);
        if (valid && rank == 0)
            wcnt[wave][d] = (unsigned)__popcll(mask);
        __syncthreads();
        if (valid) {
            unsigned at = running[d] + rank;
#pragma unroll
            for (int w = 0; w < TR_WAVES; ++w)
                at += w < wave ? wcnt[w][d] : 0u;
            dst[at] = kp; /* at < NZ: the counters sum to NZ */
        }
        __syncthreads();
        { /* thread t: digit t */
            unsigned tot = 0;
#pragma unroll
            for (int w = 0; w < TR_WAVES; ++w) {
                tot += wcnt[w][tid];
                wcnt[w][tid] = 0;
            }
            running[tid] += tot;
        }
        __syncthreads();
    }
}

/* rows[p] = the row of A that holds position p, by a binary search in IRP.
 * Neighbouring lanes hold neighbouring positions and walk the same path
 * through IRP, so the loads are shared -- which they are not when the sorted
 * positions are searched for in the gather */
__global__ void __launch_bounds__(TR_T)
k_tr_rows(const int *__restrict__ irp, int M, int64_t NZ,
          int *__restrict__ rows) {
    const int64_t p = (int64_t)blockIdx.x * TR_T + threadIdx.x;
    if (p >= NZ)
        return;
    int lo = 0, hi = M; /* irp[lo] <= p < irp[hi] */
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (irp[mid] <= p)
            lo = mid;
        else
            hi = mid;
    }
    rows[p] = lo;
}

/* T's JA and values from the sorted positions.  U is the value as raw bits
 * (uint64_t / uint32_t): moved, never computed */
template <typename U>
__global__ void __launch_bounds__(TR_T)
k_tr_gather(const uint2 *__restrict__ sorted, int64_t NZ,
            const int *__restrict__ rows, const U *__restrict__ as,
            int *__restrict__ ja_t, U *__restrict__ as_t) {
    const int64_t q = (int64_t)blockIdx.x * TR_T + threadIdx.x;
    if (q >= NZ)
        return;
    const unsigned p = ld_stream(&sorted[q].y); /* < NZ: a permutation */
    ja_t[q] = rows[p];
    as_t[q] = as[p];
}

/* flags |= 1 where the index arrays differ, |= 2 where two values do not
 * compare equal with == (a NaN equals nothing, -0.0 equals 0.0) */
template <typename V>
__global__ void __launch_bounds__(TR_T)
k_tr_equal(const int *__restrict__ ia, const int *__restrict__ ib, int64_t ni,
           const V *__restrict__ va, const V *__restrict__ vb, int64_t nv,
           unsigned *__restrict__ flags) {
    const int64_t first = (int64_t)blockIdx.x * TR_T + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * TR_T;
    unsigned f = 0;
    for (int64_t i = first; i < ni; i += stride)
        f |= ia[i] != ib[i] ? 1u : 0u;
    for (int64_t i = first; i < nv; i += stride)
        f |= va[i] == vb[i] ? 0u : 2u;
    if (f)
        atomicOr(flags, f);
}

/* ------------------------------------------------------------------ */
/* launchers: the arguments were checked by the caller (engine.hip)     */
/* ------------------------------------------------------------------ */

/* the one owner of the scratch: freed on every path */
struct tr_scratch {
    char *base = NULL;
    ~tr_scratch() { (void)hipFree(base); }
};

template <bool FIRST>
static void tr_pass(const transpose_plan &pl, const int *ja, const uint2 *src,
                    uint2 *dst, int64_t NZ, int shift, int *counters, int *sums,
                    hipStream_t s) {
    const dim3 grid((unsigned)pl.workgroups), block(TR_T);
    hipLaunchKernelGGL((k_tr_hist<FIRST>), grid, block, 0, s, ja, src, NZ,
                       shift, pl.workgroups, counters);
    tr_scan(counters, pl.counters, sums, s);
    hipLaunchKernelGGL((k_tr_scatter<FIRST>), grid, block, 0, s, ja, src, NZ,
                       shift, pl.workgroups, counters, dst);
}

/* T (allocated N x M with NZ entries of A's value type: csr_alloc_dev) gets
 * its irp, ja and values.  Blocks until they are there.  -EDOM: a column of A
 * lies outside [0, N) (T's arrays then hold nothing of use) */
int csr_transpose_dev(const spmv_csr_dev *A, spmv_csr_dev *T, hipStream_t s) {
    int rc = 0;
    transpose_plan pl;
    tr_scratch scratch;
    unsigned flag = 0;
    rc = transpose_plan_make(A->N, A->NZ, &pl);
    if (rc)
        return rc;
    (void)hipGetLastError(); /* an earlier caller's unread error is not ours */
    HIP_TRY(hipMemsetAsync(T->irp, 0, ((size_t)A->N + 1) * sizeof(int), s));
    if (A->NZ > 0) {
        const int64_t NZ = A->NZ;
        HIP_TRY(hipMalloc((void **)&scratch.base, (size_t)pl.scratch_bytes));
        uint2 *pairs[2] = {(uint2 *)(scratch.base + pl.off_pairs[0]),
                           (uint2 *)(scratch.base + pl.off_pairs[1])};
        int *counters = (int *)(scratch.base + pl.off_counters);
        int *sums = (int *)(scratch.base + pl.off_sums);
        unsigned *d_flag = (unsigned *)(scratch.base + pl.off_flag);
        HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(unsigned), s));
        hipLaunchKernelGGL(k_tr_colcount,
                           dim3((unsigned)transpose_ceil_div(NZ, TR_T)),
                           dim3(TR_T), 0, s, A->ja, NZ, A->N, T->irp, d_flag);
        tr_scan(T->irp, (int64_t)A->N + 1, sums, s);
        for (int p = 0; p < pl.passes; ++p) {
            const int shift = p * pl.digit_bits;
            if (p == 0)
                tr_pass<true>(pl, A->ja, NULL, pairs[0], NZ, shift, counters,
                              sums, s);
            else
                tr_pass<false>(pl, NULL, pairs[(p - 1) & 1], pairs[p & 1], NZ,
                               shift, counters, sums, s);
        }
        const uint2 *sorted = pairs[(pl.passes - 1) & 1];
        /* the buffer the last pass did not write: NZ ints fit its 8 NZ bytes */
        int *rows = (int *)pairs[pl.passes & 1];
        const dim3 grid((unsigned)transpose_ceil_div(NZ, TR_T)), block(TR_T);
        hipLaunchKernelGGL(k_tr_rows, grid, block, 0, s, A->irp, A->M, NZ,
                           rows);
        if (A->value_bytes == 4)
            hipLaunchKernelGGL((k_tr_gather<uint32_t>), grid, block, 0, s,
                               sorted, NZ, rows, (const uint32_t *)A->as32,
                               T->ja, (uint32_t *)T->as32);
        else
            hipLaunchKernelGGL((k_tr_gather<uint64_t>), grid, block, 0, s,
                               sorted, NZ, rows, (const uint64_t *)A->as,
                               T->ja, (uint64_t *)T->as);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&flag, d_flag, sizeof(unsigned),
                               hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    rc = csr_flags_errno(flag);
fail:
    if (rc) /* nothing of ours is left running when the scratch is freed */
        (void)hipStreamSynchronize(s);
    return rc;
}

/* X and Y have the same shape, entry count and value type: *pattern = their
 * irp and ja are equal, *values = their stored values compare equal too */
int csr_equal_dev(const spmv_csr_dev *X, const spmv_csr_dev *Y, int *pattern,
                  int *values, hipStream_t s) {
    int rc = 0;
    unsigned *d_flags = NULL, flags = 0;
    const int64_t NZ = X->NZ;
    const dim3 grid(4096), block(TR_T);
    (void)hipGetLastError();
    HIP_TRY(hipMalloc((void **)&d_flags, sizeof(unsigned)));
    HIP_TRY(hipMemsetAsync(d_flags, 0, sizeof(unsigned), s));
    /* the two index arrays one after the other; the values ride with ja */
    hipLaunchKernelGGL((k_tr_equal<double>), grid, block, 0, s, X->irp, Y->irp,
                       (int64_t)X->M + 1, (const double *)NULL,
                       (const double *)NULL, (int64_t)0, d_flags);
    if (X->value_bytes == 4)
        hipLaunchKernelGGL((k_tr_equal<float>), grid, block, 0, s, X->ja, Y->ja,
                           NZ, X->as32, Y->as32, NZ, d_flags);
    else
        hipLaunchKernelGGL((k_tr_equal<double>), grid, block, 0, s, X->ja,
                           Y->ja, NZ, X->as, Y->as, NZ, d_flags);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&flags, d_flags, sizeof(unsigned),
                           hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *pattern = !(flags & 1u);
    *values = !(flags & 3u);
fail:
    if (rc)
        (void)hipStreamSynchronize(s);
    (void)hipFree(d_flags);
    return rc;
}
