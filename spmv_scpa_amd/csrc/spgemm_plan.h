/*
 * spgemm_plan.h -- the host arithmetic of a device-side sparse product
 * C = A B of CSR handles (spmv_csr_spgemm, spmv_engine.h; the kernels:
 * spgemm_kernels.hip).
 *
 * Header-only and free of HIP, 64-bit throughout, so that the launcher, the
 * public spmv_spgemm_shape() and the tests read the SAME numbers, and so that
 * the arithmetic runs under AddressSanitizer + UBSan on the CPU
 * (tests/asan/spgemm_plan_asan.cc).
 *
 * A row r of C is served by the class of its upper bound
 *     ub[r] = sum over the entries (r, k) of A of len(row k of B)
 * (64-bit: the number of products of the row).  Classes 0..2 keep the row's
 * columns in an LDS table of SPGEMM_TABLE(c) slots, worked by a team of
 * SPGEMM_TEAM(c) lanes: part of a wavefront, a wavefront, a workgroup.  A row
 * goes to the first class whose edge holds its ub; the edge is HALF the table,
 * so a table is never more than half full -- and in particular never full:
 * every probe meets its key or an empty slot.  Class 3 is the fallback: one
 * workgroup per row with a dense accumulator of N doubles and N bits in
 * global scratch, run in batches of spgemm_fallback.batch rows so that the
 * scratch stays within SPGEMM_FALLBACK_BYTES (or one row's, if that is more).
 *
 * LDS of one team of class c, in this order (every part 8-byte aligned):
 *   values   table / 2 doubles   the sums of the row's columns, ascending
 *                                (before the walk: the gathered keys)
 *   keys     table ints          the hash set, then the row's keys, sorted
 *   touched  table / 2 bytes     1: the slot's first product has arrived
 *   count    8 bytes             distinct columns (the symbolic pass)
 *
 * Scratch of a product (one allocation, every part at a multiple of 256):
 *   head     SPGEMM_HEAD_WORDS 64-bit words: flags, products, widest, the
 *            rows of each class, their fill cursors, the entries of C
 *   ub       M x 8 bytes
 *   count    (M + 1) ints: the rows' distinct columns, scanned into C's IRP
 *   list     M ints: the rows of class 0, then 1, 2, 3
 *   sums     the scan's tile sums (transpose_scan_tiles(M + 1) ints)
 * and, when class 3 holds a row, a second allocation (spgemm_fallback):
 *   acc      batch x align(8 N) bytes
 *   bits     batch x align(4 ceil(N / 32)) bytes, zero between rows
 */
#ifndef SPMV_SPGEMM_PLAN_H
#define SPMV_SPGEMM_PLAN_H

#include <errno.h>
#include <stdint.h>

#define SPGEMM_CLASSES 4 /* the last one is the fallback */
#define SPGEMM_THREADS 256 /* lanes of every workgroup */
#define SPGEMM_ALIGN 256
#define SPGEMM_HEAD_WORDS 16
#define SPGEMM_SCAN_TILE 2048 /* = TRANSPOSE_SCAN_TILE (static_assert in the
                                 kernels): ints one scan tile sums */
/* most rows of one fallback launch, and the scratch they may take together */
#define SPGEMM_FALLBACK_MAX_BATCH 1024
#define SPGEMM_FALLBACK_BYTES ((int64_t)1 << 30)

/* lanes of a team and slots of its table, per class (the kernels are
 * instantiated with these) */
#define SPGEMM_TEAM0 16
#define SPGEMM_TEAM1 64
#define SPGEMM_TEAM2 SPGEMM_THREADS
#define SPGEMM_TABLE0 64
#define SPGEMM_TABLE1 1024
#define SPGEMM_TABLE2 8192

static const int spgemm_team_[3] = {SPGEMM_TEAM0, SPGEMM_TEAM1, SPGEMM_TEAM2};
static const int spgemm_table_[3] = {SPGEMM_TABLE0, SPGEMM_TABLE1,
                                     SPGEMM_TABLE2};

/* c = 0, 1, 2 */
static inline int spgemm_team(int c) { return spgemm_team_[c]; }
static inline int spgemm_table(int c) { return spgemm_table_[c]; }
/* the largest ub class c serves */
static inline int64_t spgemm_edge(int c) { return spgemm_table_[c] / 2; }
/* LDS bytes of one team, and of a workgroup (SPGEMM_THREADS / team teams) */
static inline int spgemm_team_lds(int c) {
    const int t = spgemm_table_[c];
    return t / 2 * 8 + t * 4 + t / 2 + 8;
}
static inline int spgemm_lds(int c) {
    return spgemm_team_lds(c) * (SPGEMM_THREADS / spgemm_team_[c]);
}

/* the class of a row with ub products (ub >= 0) */
static inline int spgemm_class(int64_t ub) {
    for (int c = 0; c < 3; ++c)
        if (ub <= spgemm_edge(c))
            return c;
    return 3;
}

static inline int64_t spgemm_ceil_div(int64_t a, int64_t b) {
    return a / b + (a % b != 0);
}

static inline int64_t spgemm_align_up(int64_t bytes) {
    return spgemm_ceil_div(bytes, SPGEMM_ALIGN) * SPGEMM_ALIGN;
}

/* workgroups of the launch that serves n rows of class c = 0, 1, 2 */
static inline int64_t spgemm_grid(int c, int64_t n) {
    return spgemm_ceil_div(n, SPGEMM_THREADS / spgemm_team_[c]);
}

/* the entries of C: -EOVERFLOW for more than an `int` IRP can hold */
static inline int spgemm_nz_guard(int64_t nz) {
    if (nz < 0)
        return -EINVAL;
    return nz > INT32_MAX ? -EOVERFLOW : 0;
}

struct spgemm_plan {
    int64_t off_head, off_ub, off_count, off_list, off_sums;
    int64_t scratch_bytes;
};

/* A is M x K, B is K x N.  -EINVAL for a size no handle holds */
static inline int spgemm_plan_make(int64_t M, int64_t K, int64_t N,
                                   spgemm_plan *p) {
    if (!p || M < 0 || K < 0 || N < 0 || M > INT32_MAX || K > INT32_MAX ||
        N > INT32_MAX)
        return -EINVAL;
    int64_t at = 0;
    p->off_head = at;
    at += spgemm_align_up(SPGEMM_HEAD_WORDS * 8);
    p->off_ub = at;
    at += spgemm_align_up(M * 8);
    p->off_count = at;
    at += spgemm_align_up((M + 1) * 4);
    p->off_list = at;
    at += spgemm_align_up(M * 4);
    p->off_sums = at;
    at += spgemm_align_up(spgemm_ceil_div(M + 1, SPGEMM_SCAN_TILE) * 4);
    p->scratch_bytes = at;
    return 0;
}

struct spgemm_fallback {
    int64_t words;      /* 32-bit words of one row's bits: ceil(N / 32) */
    int64_t acc_stride; /* bytes between the accumulators of two slots */
    int64_t bits_stride;
    int64_t batch;      /* rows of one launch (= slots) */
    int64_t launches;   /* ceil(rows / batch) */
    int64_t off_acc, off_bits;
    int64_t scratch_bytes; /* 0 when there is no row to serve */
};

/* `rows` rows of class 3 in a product with N columns */
static inline int spgemm_fallback_make(int64_t N, int64_t rows,
                                       spgemm_fallback *f) {
    if (!f || N < 0 || rows < 0 || N > INT32_MAX || rows > INT32_MAX)
        return -EINVAL;
    f->words = spgemm_ceil_div(N, 32);
    f->acc_stride = spgemm_align_up(N * 8);
    f->bits_stride = spgemm_align_up(f->words * 4);
    const int64_t per_row = f->acc_stride + f->bits_stride;
    int64_t batch = per_row > 0 ? SPGEMM_FALLBACK_BYTES / per_row
                                : SPGEMM_FALLBACK_MAX_BATCH;
    if (batch > SPGEMM_FALLBACK_MAX_BATCH)
        batch = SPGEMM_FALLBACK_MAX_BATCH;
    if (batch > rows)
        batch = rows;
    if (batch < 1 && rows > 0)
        batch = 1; /* one row's scratch, however wide */
    f->batch = batch;
    f->launches = batch > 0 ? spgemm_ceil_div(rows, batch) : 0;
    f->off_acc = 0;
    f->off_bits = batch * f->acc_stride;
    f->scratch_bytes = batch * per_row;
    return 0;
}

/* launch l of the fallback serves rows [*first, *first + *count) of class 3 */
static inline void spgemm_fallback_batch(const spgemm_fallback *f,
                                         int64_t rows, int64_t l,
                                         int64_t *first, int64_t *count) {
    *first = l * f->batch;
    *count = rows - *first < f->batch ? rows - *first : f->batch;
}

#endif /* SPMV_SPGEMM_PLAN_H */
