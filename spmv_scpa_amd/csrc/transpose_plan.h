/*
 * transpose_plan.h -- the host arithmetic of a device-side CSR transposition
 * (spmv_csr_transpose, spmv_engine.h; the kernels: transpose_kernels.hip).
 *
 * Header-only and free of HIP, 64-bit throughout, so that the launcher, the
 * public spmv_transpose_plan() and the tests read the SAME numbers, and so
 * that the arithmetic runs under AddressSanitizer + UBSan on the CPU
 * (tests/asan/transpose_plan_asan.cc).
 *
 * The transposition is a least-significant-digit radix sort of the NZ pairs
 * (column, position) by column: `passes` stable counting sorts on digits of
 * `digit_bits` bits.  In every pass workgroup w owns keys [w * tile,
 * min((w + 1) * tile, NZ)); the counters are kept digit-major,
 * counter[digit * workgroups + w], so that ONE exclusive scan over the
 * flattened array gives every (digit, workgroup) its first output position.
 *
 * Scratch (one allocation, every part at a multiple of 256 bytes):
 *   pair buffers   2 x NZ x 8 bytes  (key, position); pass 0 reads JA itself,
 *                  later passes ping-pong.  The buffer the last pass did NOT
 *                  write then holds the gather's row index (the row of every
 *                  position of A, NZ ints), which is why a single pass has
 *                  two buffers as well
 *   counters       2^digit_bits x workgroups ints
 *   scan sums      one int per TRANSPOSE_SCAN_TILE scanned ints, sized for the
 *                  longer of the two scans (the counters, and the N + 1
 *                  column counts that become the result's IRP)
 *   flag           one word: a column outside [0, N) was met
 */
#ifndef SPMV_TRANSPOSE_PLAN_H
#define SPMV_TRANSPOSE_PLAN_H

#include <errno.h>
#include <stdint.h>

#define TRANSPOSE_DIGIT_BITS 8
#define TRANSPOSE_RADIX (1 << TRANSPOSE_DIGIT_BITS)
#define TRANSPOSE_THREADS 256 /* lanes of a workgroup = keys of a strip */
#define TRANSPOSE_STRIPS 16   /* strips a workgroup walks, in order */
#define TRANSPOSE_TILE (TRANSPOSE_THREADS * TRANSPOSE_STRIPS)
#define TRANSPOSE_SCAN_PER_THREAD 8
#define TRANSPOSE_SCAN_TILE (TRANSPOSE_THREADS * TRANSPOSE_SCAN_PER_THREAD)
#define TRANSPOSE_ALIGN 256

struct transpose_plan {
    int digit_bits;
    int passes;         /* max(1, ceil(bits(N - 1) / digit_bits)) */
    int tile;           /* keys per workgroup */
    int buffers;        /* pair buffers: 0 (NZ = 0) or 2 */
    int64_t workgroups; /* ceil(NZ / tile) */
    int64_t counters;   /* 2^digit_bits * workgroups */
    int64_t scan_sums;  /* ints of the scan's tile sums */
    /* byte offsets into the one scratch allocation */
    int64_t off_pairs[2];
    int64_t off_counters;
    int64_t off_sums;
    int64_t off_flag;
    int64_t scratch_bytes;
};

static inline int64_t transpose_ceil_div(int64_t a, int64_t b) {
    return a / b + (a % b != 0);
}

static inline int64_t transpose_align_up(int64_t bytes) {
    return transpose_ceil_div(bytes, TRANSPOSE_ALIGN) * TRANSPOSE_ALIGN;
}

/* bits needed to write v >= 0: 0 for 0, 1 for 1, 2 for 2 and 3, ... */
static inline int transpose_bits(int64_t v) {
    int b = 0;
    while (v > 0) {
        ++b;
        v >>= 1;
    }
    return b;
}

/* ints of tile sums a scan over n ints needs */
static inline int64_t transpose_scan_tiles(int64_t n) {
    return transpose_ceil_div(n, TRANSPOSE_SCAN_TILE);
}

/* N columns of the source (rows of the result), NZ entries.  -EINVAL for a
 * negative size or an entry count no `int` IRP can hold. */
static inline int transpose_plan_make(int64_t N, int64_t NZ, transpose_plan *p) {
    if (!p || N < 0 || NZ < 0 || N > INT32_MAX || NZ > INT32_MAX)
        return -EINVAL;
    p->digit_bits = TRANSPOSE_DIGIT_BITS;
    const int bits = N > 0 ? transpose_bits(N - 1) : 0;
    p->passes = (bits + TRANSPOSE_DIGIT_BITS - 1) / TRANSPOSE_DIGIT_BITS;
    if (p->passes < 1)
        p->passes = 1;
    p->tile = TRANSPOSE_TILE;
    p->workgroups = transpose_ceil_div(NZ, TRANSPOSE_TILE);
    p->counters = (int64_t)TRANSPOSE_RADIX * p->workgroups;
    p->buffers = NZ == 0 ? 0 : 2;
    const int64_t a = transpose_scan_tiles(p->counters);
    const int64_t b = transpose_scan_tiles(N + 1);
    p->scan_sums = a > b ? a : b;
    int64_t at = 0;
    for (int k = 0; k < 2; ++k) {
        p->off_pairs[k] = at;
        if (k < p->buffers)
            at += transpose_align_up(NZ * 8);
    }
    p->off_counters = at;
    at += transpose_align_up(p->counters * 4);
    p->off_sums = at;
    at += transpose_align_up(p->scan_sums * 4);
    p->off_flag = at;
    at += TRANSPOSE_ALIGN;
    p->scratch_bytes = at;
    return 0;
}

#endif /* SPMV_TRANSPOSE_PLAN_H */
