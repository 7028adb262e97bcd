/*
 * csr_build.h -- the steps shared by the device operations that build the
 * arrays of a new CSR handle (the product, the sum, the transposition, the
 * factorisations, the colouring, the AMG setup and the triangular analysis;
 * csr_build.hip holds what is not a template).  DESIGN.md "Building a handle
 * on the device" says where a new operation plugs in.  Not installed.
 */
#ifndef SPMV_CSR_BUILD_H
#define SPMV_CSR_BUILD_H

#include "hip_common.h"
#include "transpose_plan.h"

#define CSR_BUILD_T 256 /* lanes of a workgroup of the kernels below */

/* what a structure check raises in its flag word.  Every operation that
 * checks its operand on the device uses these two bits, whatever else its
 * check kernel computes in the same pass */
#define CSR_BAD_COLUMN 1u /* a column outside its range */
#define CSR_BAD_ORDER 2u  /* a row that is not strictly ascending (or, where
                             the operation needs one, without its diagonal) */

/* the flag word as the host API's error: a column outside wins */
static inline int csr_flags_errno(unsigned long long flags) {
    if (flags & CSR_BAD_COLUMN)
        return -EDOM;
    return flags & CSR_BAD_ORDER ? -EINVAL : 0;
}

/* workgroups of `threads` lanes that cover n items, one at least */
static inline dim3 grid_for(int64_t n, int threads) {
    return dim3((unsigned)transpose_ceil_div(n > 0 ? n : 1, threads));
}

/* host clock, ms (the phase times the report tools print) */
double csr_now_ms(void);

/* exclusive scan of n ints in place; sums: transpose_scan_tiles(n) ints of
 * scratch */
void tr_scan(int *data, int64_t n, int *sums, hipStream_t s);

/* *d_flags |= CSR_BAD_COLUMN for a column of B outside [0, B->N), |=
 * CSR_BAD_ORDER for a row that is not strictly ascending; one lane per entry,
 * asynchronous */
int csr_check_rows_dev(const spmv_csr_dev *B, unsigned long long *d_flags,
                       hipStream_t s);

/* *d_total += count[0] + ... + count[M - 1]: a grid-stride loop over at most
 * CSR_REDUCE_GRID workgroups and one atomic a workgroup (add_kernels.hip,
 * k_add_bound, on why not one a wavefront); asynchronous */
#define CSR_REDUCE_GRID 1024
int csr_total_dev(const int *count, int M, unsigned long long *d_total,
                  hipStream_t s);

/*
 * count[0 .. M) holds the rows' lengths, count[M] is 0, and nz, their total,
 * passed the guard of the caller's plan header (an `int` irp can hold it):
 * count is scanned in place (sums: the scan's scratch), *C comes from
 * csr_alloc_dev(M, N, nz, f64) and gets the scanned counts as its irp.
 * scanned_ms: NULL, or the stream is waited for once the scan is enqueued and
 * *scanned_ms receives csr_now_ms() (a phase boundary of the caller's
 * report).  On an error *C is untouched.
 */
int csr_alloc_scanned_dev(int M, int N, int64_t nz, int *count, int *sums,
                          double *scanned_ms, spmv_csr_dev **C, hipStream_t s);

/* f(VA(), VB()) for the stored value types of A and B (f: a generic lambda
 * that instantiates its launcher with decltype of the two) */
template <typename F>
static inline int csr_value_types(const spmv_csr_dev *A, const spmv_csr_dev *B,
                                  F f) {
    if (A->value_bytes == 4)
        return B->value_bytes == 4 ? f(float(), float()) : f(float(), double());
    return B->value_bytes == 4 ? f(double(), float()) : f(double(), double());
}

#if defined(__HIPCC__)
/*
 * The rows of each class as contiguous lists: list[cursor[c] ...] receives
 * the rows r with cls(r) == c.  The host sets cursor[c] to the first place of
 * class c's list (it knows the classes' sizes).  One ballot and one atomic a
 * wavefront and class; the order inside a list comes from that atomic and may
 * differ from run to run -- a list only says which team serves which row.
 */
template <int CLASSES, typename F>
__global__ void __launch_bounds__(CSR_BUILD_T)
k_csr_lists(int M, F cls, unsigned long long *__restrict__ cursor,
            int *__restrict__ list) {
    const int64_t r = (int64_t)blockIdx.x * CSR_BUILD_T + threadIdx.x;
    const int lane = threadIdx.x & (WAVE - 1);
    const int mine = r < M ? cls(r) : -1;
#pragma unroll
    for (int c = 0; c < CLASSES; ++c) {
        const unsigned long long mask = __ballot(mine == c);
        if (!mask) /* wavefront-uniform */
            continue;
        const int leader = __ffsll((long long)mask) - 1;
        unsigned long long base = 0;
        if (lane == leader)
            base = atomicAdd(cursor + c, (unsigned long long)__popcll(mask));
        base = __shfl(base, leader, WAVE);
        if (mine == c) /* base + rank < M: the classes' counts sum to M */
            list[base + lanes_below(mask)] = (int)r;
    }
}

/* cls: a functor passed by value, int operator()(int64_t row) const on the
 * device, in [0, CLASSES) */
template <int CLASSES, typename F>
static inline void csr_lists_dev(int M, F cls, unsigned long long *cursor,
                                 int *list, hipStream_t s) {
    hipLaunchKernelGGL((k_csr_lists<CLASSES, F>), grid_for(M, CSR_BUILD_T),
                       dim3(CSR_BUILD_T), 0, s, M, cls, cursor, list);
}
#endif

#endif /* SPMV_CSR_BUILD_H */
