/*
 * trsv_plan.h -- the host arithmetic of the level-scheduled triangular solve
 * (spmv_csr_trsv_analyse, spmv_trsv_solve, spmv_engine.h; the kernels:
 * trsv_kernels.hip).
 *
 * Header-only and free of HIP, so that the launcher, spmv_trsv_info
 * (`launches`) and the tests read the SAME numbers, and so that the arithmetic
 * runs under AddressSanitizer + UBSan on the CPU
 * (tests/asan/trsv_plan_asan.cc).
 *
 * A solve walks the levels 0 .. levels - 1 in order; level l holds the rows
 * order[level_ptr[l] .. level_ptr[l + 1]).  The launches:
 *   TRSV_WIDE   one level of MORE than TRSV_SMALL_ROWS rows, one launch of
 *               ceil(rows / (threads / TRSV_GROUP)) workgroups; the kernel
 *               boundary orders it against its neighbours
 *   TRSV_CHAIN  a MAXIMAL run of consecutive levels of at most
 *               TRSV_SMALL_ROWS rows each, one launch of ONE workgroup that
 *               walks them with a workgroup barrier in between
 * The list is a pure function of level_ptr: no launch depends on a value.
 */
#ifndef SPMV_TRSV_PLAN_H
#define SPMV_TRSV_PLAN_H

#include <errno.h>
#include <stdint.h>

/* the two constants tools/trsv_report.py measured (profiles/trsv.md); -D only
 * for that comparison: G is part of the result contract */
#ifndef TRSV_GROUP
#define TRSV_GROUP 8         /* lanes per row = slots of a row's sum (G) */
#endif
#ifndef TRSV_SMALL_ROWS
#define TRSV_SMALL_ROWS 128  /* a level up to this many rows joins a chain:
                                one pass of the default chain workgroup */
#endif
#define TRSV_THREADS 1024    /* lanes of the chain workgroup by default */
#define TRSV_WIDE_THREADS 256 /* lanes of a wide workgroup by default */
#define TRSV_DEFAULT_MAX_LEVELS (1 << 20)

#define TRSV_WIDE 0
#define TRSV_CHAIN 1

struct trsv_segment {
    int kind;        /* TRSV_WIDE / TRSV_CHAIN */
    int first_level; /* inclusive */
    int last_level;  /* inclusive; == first_level for TRSV_WIDE */
};

static inline int64_t trsv_ceil_div(int64_t a, int64_t b) {
    return a / b + (a % b != 0);
}

/* workgroups of a wide launch over `rows` rows with `threads` lanes each */
static inline int64_t trsv_wide_grid(int64_t rows, int threads) {
    return trsv_ceil_div(rows, threads / TRSV_GROUP);
}

/*
 * The launches of one solve.  level_ptr[0 .. levels] is non-decreasing from 0.
 * Writes at most `cap` segments to out (out may be NULL with cap 0: count
 * only) and returns how many there are; -EINVAL for a NULL level_ptr with
 * levels > 0, negative sizes, small_rows < 0 or a decreasing level_ptr.
 */
static inline int64_t trsv_segments(const int *level_ptr, int levels,
                                    int small_rows, trsv_segment *out,
                                    int64_t cap) {
    if (levels < 0 || small_rows < 0 || cap < 0 || (levels > 0 && !level_ptr) ||
        (cap > 0 && !out))
        return -EINVAL;
    int64_t n = 0;
    int chain_from = -1; /* first level of the open chain run */
    for (int l = 0; l < levels; ++l) {
        const int64_t rows = (int64_t)level_ptr[l + 1] - level_ptr[l];
        if (rows < 0)
            return -EINVAL;
        if (rows <= small_rows) {
            if (chain_from < 0)
                chain_from = l;
            continue;
        }
        if (chain_from >= 0) {
            if (n < cap)
                out[n] = trsv_segment{TRSV_CHAIN, chain_from, l - 1};
            ++n;
            chain_from = -1;
        }
        if (n < cap)
            out[n] = trsv_segment{TRSV_WIDE, l, l};
        ++n;
    }
    if (chain_from >= 0) {
        if (n < cap)
            out[n] = trsv_segment{TRSV_CHAIN, chain_from, levels - 1};
        ++n;
    }
    return n;
}

/*
 * SWEEP PLANS (spmv_csr_trsv_analyse_sweeps): a solve is `sweeps` launches over
 * all rows, x(1) = D^-1 b, x(m) = D^-1 (b - S x(m-1)).  The route says which
 * buffer sweep m (1 .. sweeps) gathers from and which it writes: the caller's X
 * or the plan's scratch T1, T2 (ld = k).  Every sweep reads its right-hand side
 * from B, and nothing but the last sweep writes X, so X may be B.  The
 * launcher, `bytes` and tests/asan/trsv_sweep_asan.cc read this one function.
 */
#define TRSV_FEW_LANES 2   /* lanes per row of a sweep over short rows */
#define TRSV_FEW_ENTRIES 4 /* "short": at most this many strict entries a row
                              on average (measured at 2.0 and at 12.9 only:
                              profiles/trsv_sweeps.md) */
#define TRSV_MAX_SWEEPS 4096
#define TRSV_MAX_K 8
#define TRSV_BUF_NONE (-1) /* the first sweep gathers nothing */
#define TRSV_BUF_X 0
#define TRSV_BUF_T1 1
#define TRSV_BUF_T2 2

struct trsv_route {
    int in;  /* TRSV_BUF_NONE, _T1, _T2: never the buffer `out` names */
    int out; /* TRSV_BUF_X in the last sweep, else _T1 / _T2 alternately */
};

/* scratch vectors of kmax * M doubles a plan of `sweeps` sweeps owns */
static inline int trsv_sweep_scratch(int sweeps) {
    return sweeps < 2 ? 0 : sweeps == 2 ? 1 : 2;
}

/* lanes per row of the sweeps of a plan: a function of the plan alone.  The
 * G slots of a row's sum are the contract, the lanes are not: the bits are the
 * same either way */
static inline int trsv_sweep_lanes(int64_t M, int64_t entries) {
    return entries <= TRSV_FEW_ENTRIES * M ? TRSV_FEW_LANES : TRSV_GROUP;
}

/* workgroups of one sweep over M rows, `lanes` lanes a row, `threads` a group */
static inline int64_t trsv_sweep_grid(int64_t M, int threads, int lanes) {
    return trsv_ceil_div(M, threads / lanes);
}

/* 1 <= m <= sweeps */
static inline trsv_route trsv_sweep_route(int sweeps, int m) {
    trsv_route r;
    r.in = m == 1 ? TRSV_BUF_NONE : (m & 1) ? TRSV_BUF_T2 : TRSV_BUF_T1;
    r.out = m == sweeps ? TRSV_BUF_X : (m & 1) ? TRSV_BUF_T1 : TRSV_BUF_T2;
    return r;
}

/*
 * Element counts of the analysis' device arrays for M rows, NZ stored and
 * SNZ strict entries (the launcher allocates exactly these; the sanitizer
 * program restates the kernels over heap blocks of these sizes).
 */
struct trsv_sizes {
    int64_t cnt;      /* M + 1 ints: strict count per row, scanned in place */
    int64_t diag;     /* M doubles */
    int64_t sja;      /* SNZ ints: strict columns in row order */
    int64_t spos;     /* SNZ ints: their positions in A */
    int64_t succ_ptr; /* M + 1 ints: the strict pattern transposed */
    int64_t succ;     /* SNZ ints */
    int64_t indeg;    /* M ints */
    int64_t frontier; /* 2 x M ints, ping-pong */
    int64_t counters; /* 4 ints: three rotating frontier sizes, the flag */
    int64_t iota;     /* M + 1 ints: row pointer of the M x levels matrix */
};

static inline int trsv_sizes_make(int64_t M, int64_t NZ, int64_t SNZ,
                                  trsv_sizes *z) {
    if (!z || M < 0 || NZ < 0 || SNZ < 0 || SNZ > NZ || M > INT32_MAX - 1 ||
        NZ > INT32_MAX)
        return -EINVAL;
    z->cnt = M + 1;
    z->diag = M;
    z->sja = SNZ;
    z->spos = SNZ;
    z->succ_ptr = M + 1;
    z->succ = SNZ;
    z->indeg = M;
    z->frontier = 2 * M;
    z->counters = 4;
    z->iota = M + 1;
    return 0;
}

#endif /* SPMV_TRSV_PLAN_H */
