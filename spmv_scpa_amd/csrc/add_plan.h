/*
 * add_plan.h -- the host arithmetic of a device-side sparse sum
 * C = alpha A + beta B of CSR handles (spmv_csr_add, spmv_engine.h; the
 * kernels: add_kernels.hip).
 *
 * Header-only and free of HIP, 64-bit throughout, so that the launcher, the
 * public spmv_add_shape() and the tests read the SAME numbers, and so that
 * the arithmetic runs under AddressSanitizer + UBSan on the CPU
 * (tests/asan/add_plan_asan.cc).
 *
 * A row r of C is served by the class of its length
 *     len[r] = len_A(r) + len_B(r)
 * (64-bit: two rows of 2^31 - 1 entries).  Class 0: a group of lanes per row,
 * as wide as add_pick_group() says for the mean length (nzA + nzB) / M, the
 * choice pick_group makes for the sub-wave SpMV kernels; ADD_THREADS / width
 * rows a workgroup.  Class 1, for len[r] > ADD_EDGE: a workgroup per row.
 * Both walk a row in chunks of their width and accept any length; `mode`
 * (spmv_add_set_class) puts every row into one of them.
 *
 * Scratch of a sum (one allocation, every part at a multiple of 256):
 *   head     ADD_HEAD_WORDS 64-bit words: flags, widest, the rows of each
 *            class, their fill cursors, the entries of C
 *   count    (M + 1) ints: the rows' union lengths, scanned into C's IRP
 *   list     M ints: the rows of class 0, then those of class 1
 *   sums     the scan's tile sums
 */
#ifndef SPMV_ADD_PLAN_H
#define SPMV_ADD_PLAN_H

#include <errno.h>
#include <stdint.h>

#define ADD_CLASSES 2
#define ADD_THREADS 256 /* lanes of every workgroup */
#define ADD_ALIGN 256
#define ADD_HEAD_WORDS 8
#define ADD_REDUCE_GRID 1024 /* most workgroups of a reduction over the rows */
#define ADD_SCAN_TILE 2048 /* = TRANSPOSE_SCAN_TILE (static_assert in the
                              kernels): ints one scan tile sums */
/* the largest len_A(r) + len_B(r) a lane group serves under the rule */
#define ADD_EDGE 512
/* the widths a lane group may have */
#define ADD_WIDTHS 5
#define ADD_WIDTH_MIN 2
#define ADD_WIDTH_MAX 32

static const int add_width_[ADD_WIDTHS] = {2, 4, 8, 16, 32};

static inline int add_width(int i) { return add_width_[i]; }

static inline int64_t add_ceil_div(int64_t a, int64_t b) {
    return a / b + (a % b != 0);
}

static inline int64_t add_align_up(int64_t bytes) {
    return add_ceil_div(bytes, ADD_ALIGN) * ADD_ALIGN;
}

/* lanes per row of class 0: the smallest width that is not below the mean
 * len (integer arithmetic: width >= entries / M  <=>  width * M >= entries) */
static inline int add_pick_group(int64_t entries, int64_t M) {
    int g = ADD_WIDTH_MIN;
    if (M <= 0 || entries <= 0)
        return g;
    while (g < ADD_WIDTH_MAX && (int64_t)g * M < entries)
        g <<= 1;
    return g;
}

/* the class of a row of len entries (len >= 0).  mode 0: the rule; 1: every
 * row by lane groups; 2: every row by a workgroup */
static inline int add_class(int64_t len, int mode) {
    if (mode == 1)
        return 0;
    if (mode == 2)
        return 1;
    return len <= ADD_EDGE ? 0 : 1;
}

/* workgroups of the launch that serves n rows of class c with lane groups of
 * `width` lanes */
static inline int64_t add_grid(int c, int width, int64_t n) {
    return c == 0 ? add_ceil_div(n, ADD_THREADS / width) : n;
}

/* the entries of C: -EOVERFLOW for more than an `int` IRP can hold */
static inline int add_nz_guard(int64_t nz) {
    if (nz < 0)
        return -EINVAL;
    return nz > INT32_MAX ? -EOVERFLOW : 0;
}

/* columns stored in both operands, from the three entry counts; -EINVAL for
 * counts no union has (nz below the longer operand or above the two) */
static inline int add_matched(int64_t nzA, int64_t nzB, int64_t nz,
                              int64_t *matched) {
    if (!matched || nzA < 0 || nzB < 0 || nzA > INT32_MAX || nzB > INT32_MAX)
        return -EINVAL;
    const int64_t both = nzA + nzB; /* at most 2^32 - 2 */
    if (nz > both || nz < (nzA > nzB ? nzA : nzB))
        return -EINVAL;
    *matched = both - nz;
    return 0;
}

struct add_plan {
    int width; /* lanes of a group of class 0 */
    int64_t off_head, off_count, off_list, off_sums;
    int64_t scratch_bytes;
};

/* A and B are M x N with nzA and nzB entries.  -EINVAL for a size no handle
 * holds */
static inline int add_plan_make(int64_t M, int64_t N, int64_t nzA, int64_t nzB,
                                add_plan *p) {
    if (!p || M < 0 || N < 0 || nzA < 0 || nzB < 0 || M > INT32_MAX ||
        N > INT32_MAX || nzA > INT32_MAX || nzB > INT32_MAX)
        return -EINVAL;
    p->width = add_pick_group(nzA + nzB, M);
    int64_t at = 0;
    p->off_head = at;
    at += add_align_up(ADD_HEAD_WORDS * 8);
    p->off_count = at;
    at += add_align_up((M + 1) * 4);
    p->off_list = at;
    at += add_align_up(M * 4);
    p->off_sums = at;
    at += add_align_up(add_ceil_div(M + 1, ADD_SCAN_TILE) * 4);
    p->scratch_bytes = at;
    return 0;
}

#endif /* SPMV_ADD_PLAN_H */
