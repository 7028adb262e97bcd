/*
 * csr_build.hip -- what csr_build.h declares and is not a template: the
 * exclusive scan, the row check, the total of the rows' counts, the step that
 * turns scanned counts into a new handle's irp, and the host clock.  gfx950
 * (wave64).
 */
#include <algorithm>
#include <time.h>

#include "csr_build.h"

#define TR_T TRANSPOSE_THREADS
#define TR_WAVES (TR_T / WAVE)
#define TR_SCAN_U TRANSPOSE_SCAN_PER_THREAD
#define TR_SUMS_T 1024 /* threads of the single workgroup of k_tr_scan_sums */

typedef unsigned long long cb_u64;

double csr_now_ms(void) {
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return 1e3 * (double)t.tv_sec + 1e-6 * (double)t.tv_nsec;
}

/* ------------------------------------------------------------------ */
/* exclusive scan of n ints, in place                                   */
/* ------------------------------------------------------------------ */

/* inclusive scan of v over the wavefront */
__device__ __forceinline__ int tr_wave_scan(int v, int lane) {
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const int t = __shfl_up(v, d, WAVE);
        if (lane >= d)
            v += t;
    }
    return v;
}

/* tile b = ints [b * TRANSPOSE_SCAN_TILE, ...): scanned on its own,
 * sums[b] = its total */
__global__ void __launch_bounds__(TR_T)
k_tr_scan_local(int *__restrict__ data, int64_t n, int *__restrict__ sums) {
    __shared__ int wsum[TR_WAVES];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int64_t base =
        (int64_t)blockIdx.x * TRANSPOSE_SCAN_TILE + (int64_t)tid * TR_SCAN_U;
    int v[TR_SCAN_U];
    int run = 0;
#pragma unroll
    for (int u = 0; u < TR_SCAN_U; ++u) {
        const int t = base + u < n ? data[base + u] : 0;
        v[u] = run;
        run += t;
    }
    const int incl = tr_wave_scan(run, lane);
    if (lane == WAVE - 1)
        wsum[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < TR_WAVES; ++w) {
        before += w < wave ? wsum[w] : 0;
        total += wsum[w];
    }
    const int excl = before + incl - run;
#pragma unroll
    for (int u = 0; u < TR_SCAN_U; ++u)
        if (base + u < n)
            data[base + u] = v[u] + excl;
    if (tid == 0)
        sums[blockIdx.x] = total;
}

/* the m tile sums, scanned in place by ONE workgroup that carries its total
 * from chunk to chunk */
__global__ void __launch_bounds__(TR_SUMS_T)
k_tr_scan_sums(int *__restrict__ sums, int64_t m) {
    __shared__ int wsum[TR_SUMS_T / WAVE];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    int carry = 0;
    for (int64_t b = 0; b < m; b += TR_SUMS_T) { /* workgroup-uniform */
        const int64_t i = b + tid;
        const int x = i < m ? sums[i] : 0;
        const int incl = tr_wave_scan(x, lane);
        if (lane == WAVE - 1)
            wsum[wave] = incl;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < TR_SUMS_T / WAVE; ++w) {
            before += w < wave ? wsum[w] : 0;
            total += wsum[w];
        }
        if (i < m)
            sums[i] = carry + before + incl - x;
        carry += total;
        __syncthreads(); /* wsum is rewritten by the next chunk */
    }
}

__global__ void __launch_bounds__(TR_T)
k_tr_scan_add(int *__restrict__ data, int64_t n, const int *__restrict__ sums) {
    const int64_t base = (int64_t)blockIdx.x * TRANSPOSE_SCAN_TILE +
                         (int64_t)threadIdx.x * TR_SCAN_U;
    const int add = sums[blockIdx.x];
#pragma unroll
    for (int u = 0; u < TR_SCAN_U; ++u)
        if (base + u < n)
            data[base + u] += add;
}

void tr_scan(int *data, int64_t n, int *sums, hipStream_t s) {
    const int64_t tiles = transpose_scan_tiles(n);
    if (tiles == 0)
        return;
    hipLaunchKernelGGL(k_tr_scan_local, dim3((unsigned)tiles), dim3(TR_T), 0, s,
                       data, n, sums);
    if (tiles == 1)
        return; /* one tile: its local scan is the scan */
    hipLaunchKernelGGL(k_tr_scan_sums, dim3(1), dim3(TR_SUMS_T), 0, s, sums,
                       tiles);
    hipLaunchKernelGGL(k_tr_scan_add, dim3((unsigned)tiles), dim3(TR_T), 0, s,
                       data, n, sums);
}

/* ------------------------------------------------------------------ */
/* the row check, the total                                             */
/* ------------------------------------------------------------------ */

/* one lane per entry: column inside [0, N), and above its left neighbour in
 * the same row (K rows) */
__global__ void __launch_bounds__(CSR_BUILD_T)
k_csr_check_rows(const int *__restrict__ irp, const int *__restrict__ ja, int K,
                 int64_t NZ, int N, cb_u64 *__restrict__ flags) {
    const int64_t q = (int64_t)blockIdx.x * CSR_BUILD_T + threadIdx.x;
    if (q >= NZ)
        return;
    const int c = ja[q];
    unsigned f = (unsigned)c < (unsigned)N ? 0u : CSR_BAD_COLUMN;
    int lo = 0, hi = K; /* irp[lo] <= q < irp[hi] */
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (irp[mid] <= q)
            lo = mid;
        else
            hi = mid;
    }
    if (q > irp[lo] && ja[q - 1] >= c)
        f |= CSR_BAD_ORDER;
    if (f)
        atomicOr(flags, (cb_u64)f);
}

int csr_check_rows_dev(const spmv_csr_dev *B, unsigned long long *d_flags,
                       hipStream_t s) {
    if (B->NZ > 0)
        hipLaunchKernelGGL(k_csr_check_rows, grid_for(B->NZ, CSR_BUILD_T),
                           dim3(CSR_BUILD_T), 0, s, B->irp, B->ja, B->M, B->NZ,
                           B->N, d_flags);
    return hip_errno(hipGetLastError());
}

__global__ void __launch_bounds__(CSR_BUILD_T)
k_csr_total(const int *__restrict__ count, int M, cb_u64 *__restrict__ total) {
    __shared__ cb_u64 part[CSR_BUILD_T / WAVE];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const int64_t first = (int64_t)blockIdx.x * CSR_BUILD_T + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * CSR_BUILD_T;
    cb_u64 n = 0;
    for (int64_t r = first; r < M; r += stride)
        n += (cb_u64)count[r];
    n = wave_sum(n);
    if (lane == 0)
        part[wave] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < CSR_BUILD_T / WAVE; ++w)
            n += part[w];
        if (n)
            atomicAdd(total, n);
    }
}

int csr_total_dev(const int *count, int M, unsigned long long *d_total,
                  hipStream_t s) {
    if (M > 0)
        hipLaunchKernelGGL(k_csr_total,
                           dim3((unsigned)std::min<int64_t>(
                               CSR_REDUCE_GRID,
                               transpose_ceil_div(M, CSR_BUILD_T))),
                           dim3(CSR_BUILD_T), 0, s, count, M, d_total);
    return hip_errno(hipGetLastError());
}

int csr_alloc_scanned_dev(int M, int N, int64_t nz, int *count, int *sums,
                          double *scanned_ms, spmv_csr_dev **C, hipStream_t s) {
    spmv_csr_dev *d = NULL;
    tr_scan(count, (int64_t)M + 1, sums, s);
    HIP_RET(hipGetLastError());
    if (scanned_ms) {
        HIP_RET(hipStreamSynchronize(s));
        *scanned_ms = csr_now_ms();
    }
    int rc = csr_alloc_dev(M, N, nz, 8, &d);
    if (rc)
        return rc;
    rc = hip_errno(hipMemcpyAsync(d->irp, count, ((size_t)M + 1) * sizeof(int),
                                  hipMemcpyDeviceToDevice, s));
    if (rc) {
        spmv_csr_release(d);
        return rc;
    }
    *C = d;
    return 0;
}
