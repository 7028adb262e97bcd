/*
 * amg_plan.h -- the host arithmetic of smoothed-aggregation AMG on the device
 * (spmv_csr_aggregate, spmv_csr_amg_setup, spmv_amg_apply; spmv_engine.h; the
 * kernels: amg_kernels.hip).
 *
 * Header-only and free of HIP, 64-bit throughout, so that the launcher and the
 * tests read the SAME numbers, and so that the arithmetic runs under
 * AddressSanitizer + UBSan on the CPU (tests/asan/amg_plan_asan.cc).
 *
 * KEY of a row in the rounds of the independent set, one 64-bit word ordered
 * as an unsigned integer:
 *     out         0
 *     undecided   hash << 31 | row                    (bit 63 clear)
 *     root        1 << 63 | hash << 31 | row
 * hash = fmix32(row ^ seed) (32 bits), row < 2^31.  This is the lexicographic
 * order of (state, hash, row) with out < undecided < root wherever the rounds
 * compare: the maximum an undecided row sees holds its own key, so it is never
 * an out key, and two rows never share (hash, row).  (Row 0 at seed 0 has the
 * undecided key 0, equal to every out key: it is then its own maximum exactly
 * when everything it sees is out, which is when it must become a root.)
 *
 * SCRATCH of a hierarchy, one allocation of doubles.  Level l of M_l rows
 * takes four vectors of kmax * M_l doubles, each at a multiple of
 * AMG_ALIGN bytes, in this order:
 *     r    the residual / right-hand side of a sweep
 *     x2   the other buffer of the fused sweep's ping-pong
 *     x    the level's iterate   (level 0: unused, the caller's Z is x)
 *     b    the level's right-hand side (level 0: unused, the caller's R is b)
 * Level 0 keeps only r and x2.
 */
#ifndef SPMV_AMG_PLAN_H
#define SPMV_AMG_PLAN_H

#include <errno.h>
#include <stdint.h>

#define AMG_MAX_LEVELS 32  /* levels a hierarchy may hold */
#define AMG_MAX_K 8        /* right-hand sides of one apply */
#define AMG_MAX_SWEEPS 64  /* sweeps, coarse_sweeps */
#define AMG_ALIGN 256
#define AMG_DEFAULT_MAX_ROUNDS 4096
#define AMG_T 256 /* lanes of every workgroup of amg_kernels.hip */

#define AMG_KEY_ROOT ((uint64_t)1 << 63)

/* the key functions run in the kernels too */
#ifdef __HIPCC__
#define AMG_HD __host__ __device__
#else
#define AMG_HD
#endif

/* the finaliser of murmur3: a bijection of the 32-bit words */
AMG_HD static inline uint32_t amg_fmix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}

/* the undecided key of a row, 0 <= row < 2^31 */
AMG_HD static inline uint64_t amg_key(uint32_t row, uint32_t seed) {
    return (uint64_t)amg_fmix32(row ^ seed) << 31 | (uint64_t)row;
}
AMG_HD static inline int amg_key_is_root(uint64_t key) { return (int)(key >> 63); }
AMG_HD static inline uint32_t amg_key_row(uint64_t key) {
    return (uint32_t)(key & 0x7fffffffu);
}

static inline int amg_max_rounds(int max_rounds) {
    return max_rounds > 0 ? max_rounds : AMG_DEFAULT_MAX_ROUNDS;
}

static inline int64_t amg_ceil_div(int64_t a, int64_t b) {
    return a / b + (a % b != 0);
}

/* workgroups of AMG_T lanes that cover n items; -EOVERFLOW past a grid */
static inline int amg_grid(int64_t n, unsigned *grid) {
    const int64_t g = amg_ceil_div(n > 0 ? n : 1, AMG_T);
    if (g > 0x7fffffff)
        return -EOVERFLOW;
    *grid = (unsigned)g;
    return 0;
}

/* doubles of one scratch vector of a level, a multiple of AMG_ALIGN bytes */
static inline int64_t amg_vec_doubles(int M, int kmax) {
    const int64_t per = AMG_ALIGN / 8;
    return amg_ceil_div((int64_t)M * kmax, per) * per;
}

struct amg_layout {
    int levels;
    int64_t r[AMG_MAX_LEVELS], x2[AMG_MAX_LEVELS], x[AMG_MAX_LEVELS],
        b[AMG_MAX_LEVELS];
    int64_t doubles; /* of the whole scratch */
};

/* rows[l]: M_l, l < levels.  -EINVAL: a count out of range */
static inline int amg_layout_make(const int *rows, int levels, int kmax,
                                  struct amg_layout *out) {
    if (!rows || !out || levels < 1 || levels > AMG_MAX_LEVELS || kmax < 1 ||
        kmax > AMG_MAX_K)
        return -EINVAL;
    int64_t at = 0;
    out->levels = levels;
    for (int l = 0; l < levels; ++l) {
        if (rows[l] < 0)
            return -EINVAL;
        const int64_t v = amg_vec_doubles(rows[l], kmax);
        out->r[l] = at;
        at += v;
        out->x2[l] = at;
        at += v;
        out->x[l] = out->b[l] = -1;
        if (l > 0) {
            out->x[l] = at;
            at += v;
            out->b[l] = at;
            at += v;
        }
    }
    out->doubles = at;
    return 0;
}

/* launches of one level of an apply.  Composed sweep (a product into r and
 * a vector kernel): a level above the coarsest is first, (sweeps - 1) x 2, the
 * residual, the restriction, the prolongation, the refill, sweeps x 2; the
 * coarsest first and (coarse_sweeps - 1) x 2.  Fused sweep (one launch, its
 * residual mode one launch, no refill): 2 sweeps + 3, and coarse_sweeps */
static inline int amg_level_launches(int coarsest, int sweeps,
                                     int coarse_sweeps, int fused) {
    if (coarsest)
        return fused ? coarse_sweeps : 1 + 2 * (coarse_sweeps - 1);
    return fused ? 2 * sweeps + 3 : 4 * sweeps + 3;
}

/* ... and of a whole apply whose levels all sweep the same way */
static inline int amg_apply_launches(int levels, int sweeps, int coarse_sweeps,
                                     int fused) {
    return (levels - 1) * amg_level_launches(0, sweeps, coarse_sweeps, fused) +
           amg_level_launches(1, sweeps, coarse_sweeps, fused);
}

/* The fused sweep is used from this many right-hand sides on: measured on one
 * MI355X (profiles/amg.md) it takes 0.66 / 0.61 of the composed sweep at k =
 * 4 / 8 on the 5-point 3162^2 stencil and 0.94 / 0.97 on the 27-point 215^3
 * one, but 1.02 and 1.11 at k = 1; k = 2 and 3 were not measured and stay
 * with the composition */
#define AMG_FUSED_MIN_K 4
/* mode of spmv_amg_set_fused: 0 never, 1 by the rule above, 2 always */
static inline int amg_use_fused(int mode, int k) {
    return mode == 2 || (mode == 1 && k >= AMG_FUSED_MIN_K);
}

/* where the iterate of a level must START so that it ENDS in `home` after
 * `swaps` ping-pong sweeps: 0 = home, 1 = the other buffer */
static inline int amg_start_buffer(int swaps) { return swaps & 1; }

/* sum of the levels' entries over the entries of level 0 */
static inline double amg_complexity(const int64_t *nz, int levels) {
    int64_t sum = 0;
    for (int l = 0; l < levels; ++l)
        sum += nz[l];
    return levels > 0 && nz[0] > 0 ? (double)sum / (double)nz[0] : 0.0;
}

#endif /* SPMV_AMG_PLAN_H */
