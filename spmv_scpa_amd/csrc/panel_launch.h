/*
 * panel_launch.h -- the launch shape of the blocked path's tile kernels
 * (panels.hip, panels_launch_tiles): which kernel family and instantiation a
 * (blocked copy, waves, variant) reaches, with how much LDS, on what grid and
 * in which tile order.
 *
 * Header-only and free of HIP: pure integer logic whose thresholds were
 * expensive to measure, so it runs as a CPU test against a table of plans
 * written out from the code it replaced (tests/asan/panel_launch_asan.cc,
 * tests/test_tune_blocked_asan.py).  The lists of instantiated kernels below
 * are what panels.hip builds its kernel tables from: a plan and the kernels
 * that exist cannot disagree.
 *
 * NUM_XCD and SPMV_VARIANT_TIMING_BITS come from hip_common.h -- included
 * first by panels.hip, handed over as -D macros by the CPU test.
 */
#ifndef SPMV_PANEL_LAUNCH_H
#define SPMV_PANEL_LAUNCH_H

#include <errno.h>
#include <stddef.h>
#include <stdint.h>

#if !defined(NUM_XCD) || !defined(SPMV_VARIANT_TIMING_BITS)
#error "panel_launch.h: include hip_common.h first (or pass its NUM_XCD and SPMV_VARIANT_TIMING_BITS with -D)"
#endif

#define BIG_LDS_BYTES (160 * 1024 - 256) /* most dynamic LDS a launch asks for */

/* what the decision reads of a blocked copy: the head of spmv_panels */
struct panel_shape {
    int sweep;       /* built for the persistent schedule */
    int chain;       /* steps layout, launched as one chain launch */
    int det;         /* spmv_panel_opts.deterministic: ordered LDS additions */
    int wgs_per_cu;  /* sweep: workgroups sharing a CU's LDS */
    int panels;      /* column panels */
    int tiles;       /* row tiles */
    int64_t nnz;     /* entries kept */
    int max_nbk;     /* launches needed = max over tiles */
    int tile_rows;   /* rows per tile (multiple of 32) */
    int lds_min;     /* launch with at least this much dynamic LDS; 0: tile */
    int waves_hint;  /* wavefronts per workgroup when the caller passes 0
                        (set by the autotuner; 0 = the built-in heuristic) */
    int order;       /* steps / chain, which tile a workgroup runs
                        (spmv_panel_opts.tile_order; the selector measures):
                        0 grouped, 1 hardware order, 2 XCD-contiguous ranges */
    int grid;        /* sweep: workgroups of the launch */
    int xcd_max;     /* longest range: the launch has NUM_XCD * xcd_max groups */
    int64_t fit_steps[2]; /* sweep: steps of one pass over every bucket, the sum
                        of ceil(entries / chunk) (an empty bucket: 1), [0]
                        with the chunk of the built-in shape, [1] with
                        PANEL_FIT_CHUNK (counted on the device at the end of
                        a build); 0 = not counted: the built-in shape */
};

enum panel_family { PANEL_SWEEP, PANEL_CHAIN, PANEL_STEPS };

/* one instantiation of a family's kernel.  abl (sweep only): the kernel's
 * timing-ablation arms, 1 = no LDS add, 2 = gathers from one 8 KiB window,
 * 4 = stream from a 192 KiB window, 8 = tall tile aliased into 16384 rows */
struct panel_kernel {
    int threads, q, det, abl;
};

/* THE lists of instantiations: the first *_PRODUCT of each exist in every
 * build, the rest only with -DSPMV_ABLATIONS (`make abl`) */
constexpr panel_kernel PANEL_SWEEP_KERNELS[] = {
    {256, 1, 0, 0},  {256, 1, 1, 0},  {256, 2, 0, 0},  {256, 2, 1, 0},
    {512, 1, 0, 0},  {512, 1, 1, 0},  {512, 2, 0, 0},  {512, 2, 1, 0},
    {1024, 1, 0, 0}, {1024, 1, 1, 0}, {1024, 2, 0, 0}, {1024, 2, 1, 0},
    /* chunks of 4608 slots, which no power of two is a multiple of: 9
     * wavefronts x 2 groups, 6 wavefronts x 3 groups (panel_fit_kernel) */
    {576, 2, 0, 0},  {576, 2, 1, 0},  {384, 3, 0, 0},  {384, 3, 1, 0},
    /* timing ablations (results WRONG by design for 2, 3, 7) */
    {256, 1, 0, 1},  {256, 1, 0, 2},  {256, 1, 0, 3},  {256, 1, 0, 4},
    {256, 1, 0, 7},
    /* tall-tile probe, the production launch shapes */
    {256, 1, 0, 8},  {256, 2, 0, 8},  {512, 1, 0, 8},  {512, 2, 0, 8},
    {1024, 1, 0, 8}, {1024, 2, 0, 8},
};
constexpr int PANEL_SWEEP_PRODUCT = 16;
constexpr int panel_sweep_kernels(bool ablations) {
    return ablations ? (int)(sizeof PANEL_SWEEP_KERNELS / sizeof(panel_kernel))
                     : PANEL_SWEEP_PRODUCT;
}
constexpr panel_kernel PANEL_CHAIN_KERNELS[] = {
    {256, 1, 0, 0}, {256, 2, 0, 0}, {512, 1, 0, 0}, {512, 2, 0, 0},
    {1024, 1, 0, 0},
    {256, 2, 1, 0}, {256, 4, 1, 0}, {512, 2, 1, 0}, {512, 4, 1, 0},
};
constexpr int PANEL_CHAIN_PRODUCT = 9;
constexpr panel_kernel PANEL_STEP_KERNELS[] = {
    {256, 1, 0, 0}, {256, 2, 0, 0}, {512, 1, 0, 0}, {512, 2, 0, 0},
    {1024, 1, 0, 0},
    {256, 2, 1, 0}, {512, 2, 1, 0},
};
constexpr int PANEL_STEP_PRODUCT = 7;

template <int N>
constexpr int panel_kernel_index(const panel_kernel (&list)[N], int n,
                                 const panel_kernel &k) {
    for (int i = 0; i < n && i < N; ++i)
        if (list[i].threads == k.threads && list[i].q == k.q &&
            list[i].det == k.det && list[i].abl == k.abl)
            return i;
    return -1;
}

struct panel_plan {
    int family;     /* panel_family */
    panel_kernel k; /* the instantiation */
    int lag;        /* sweep: panels a workgroup may run ahead of its XCD */
    int stagger;    /* sweep: staggered panel order (tuning bit 12) */
    size_t lds;     /* dynamic LDS bytes */
    unsigned grid;  /* workgroups */
    int order_arg;  /* chain / steps: the kernels' tiles_hw argument */
    int launches;   /* 1; steps: one per step; 0: nothing to launch */
};

/* row in the family's list of the plan's kernel, -1: not instantiated in a
 * build of this flavour */
static inline int panel_plan_row(const panel_plan &p, bool ablations) {
    return p.family == PANEL_SWEEP
               ? panel_kernel_index(PANEL_SWEEP_KERNELS,
                                    panel_sweep_kernels(ablations), p.k)
           : p.family == PANEL_CHAIN
               ? panel_kernel_index(PANEL_CHAIN_KERNELS, PANEL_CHAIN_PRODUCT, p.k)
               : panel_kernel_index(PANEL_STEP_KERNELS, PANEL_STEP_PRODUCT, p.k);
}

/* threads per workgroup of an explicit `waves` (0: none given -> 512) */
static inline int panel_threads_of_waves(int waves) {
    return waves > 8 ? 1024 : waves > 0 && waves < 8 ? 256 : 512;
}

/*
 * Chunk fit.  A bucket of n entries takes ceil(n / chunk) steps of the sweep
 * kernel, each a full set of stream loads and, in ordered mode, a full chain
 * of turns, however few entries the last one holds.  With 2^17-column
 * panels and N / 512 rows per tile a bucket holds 32 * 2^17 / 512 = 8192
 * entries on average whatever N is -- a multiple of every power-of-two chunk,
 * so about half of the buckets spill a few dozen entries into one more step.
 * A chunk of 4608 slots takes such a bucket in two steps.  The rule: a copy
 * that fills a CU by itself and whose COUNTED steps (panel_shape.fit_steps)
 * fall by PANEL_FIT_GAIN_PCT or more takes PANEL_FIT_SHAPE instead of
 * 512 x 2.  Variant bits 16-17 ask for a shape whatever was counted:
 * 1 = 576 x 2, 2 = 384 x 3, 3 = the built-in shape.
 */
constexpr int PANEL_FIT_CHUNK = 4608;
constexpr int PANEL_FIT_GAIN_PCT = 10;
constexpr int PANEL_FIT_VARIANT_SHIFT = 16;
constexpr int PANEL_FIT_VARIANT_BITS = 3 << PANEL_FIT_VARIANT_SHIFT;
/* which = 1: 9 wavefronts x 2 groups, 2: 6 wavefronts x 3 groups */
constexpr panel_kernel panel_fit_kernel(int which) {
    return which == 2 ? panel_kernel{384, 3, 0, 0} : panel_kernel{576, 2, 0, 0};
}
/* the sibling the rule names.  Headline copy, medians of 20 launches, shapes
 * alternating (profiles/sweep_chunk_fit.md), 512 x 2 / 576 x 2 / 384 x 3:
 * ordered additions, a sweep copy's default, 1.4337 / 1.4165 / 1.3941 ms (six
 * hand-offs per chain of turns instead of nine); arrival order 1.4518 /
 * 1.4196 / 1.4307 */
constexpr int PANEL_FIT_SHAPE = 2;

static inline bool panel_fit_pays(const panel_shape &P) {
    return P.fit_steps[0] > 0 && P.fit_steps[1] > 0 &&
           P.fit_steps[1] * 100 <= P.fit_steps[0] * (100 - PANEL_FIT_GAIN_PCT);
}

/*
 * The complete plan of one panels_launch_tiles() call, or -EINVAL.
 * `ablations`: the build carries the experiment arms (-DSPMV_ABLATIONS).
 */
static inline int panel_launch_plan(const panel_shape &P, int waves,
                                    int variant, bool ablations,
                                    panel_plan *out) {
    /* product build: bit 0 flips chain <-> steps, bits 1 / 2 force a tile
     * order, bits 16-17 name a chunk-fit shape of the sweep (spmv_engine.h).
     * Everything else this function understands --
     * lag override (4-6), no phase wait (7), the ABL arms whose result is
     * WRONG by design (8-10), group counts (11), staggered panels (12),
     * group sizes (14-15) -- exists only in a -DSPMV_ABLATIONS build
     * (`make abl`; tools/sweep.py, tools/pmc.sh load that flavour) */
    if (!ablations && (variant & ~(1 | 2 | 4 | PANEL_FIT_VARIANT_BITS |
                                   SPMV_VARIANT_TIMING_BITS)))
        return -EINVAL;
    panel_plan p = {};
    p.lds = (size_t)P.tile_rows * sizeof(double);
    if (ablations && P.sweep && p.lds > (size_t)BIG_LDS_BYTES)
        p.lds = 16384 * sizeof(double); /* tall-tile probe: aliased */
    if (waves <= 0)
        waves = P.waves_hint;
    if ((size_t)P.lds_min > p.lds) /* tuning: caps workgroups per CU */
        p.lds = (size_t)P.lds_min;
    p.launches = 1;
    const bool bit11 = (variant >> 11) & 1; /* tuning: the other group count */
    if (P.sweep) {
        /* variant (tuning): bits 4-6 lag override (1..7), bit 7 no phase
         * wait, bits 8-10 ablations, bit 11 the other group count, bit 12
         * staggered panel order */
        p.family = PANEL_SWEEP;
        p.lag = (variant >> 4) & 7;
        if (p.lag == 0) /* measured best: 6 for 1 MiB panels, 3 for 2 MiB ones,
                           7 when there are hundreds of them (80 M columns:
                           3.30 -> 2.98 ms) */
            p.lag = P.wgs_per_cu == 1 ? 6 : P.panels >= 256 ? 7 : 3;
        if (variant & 128)
            p.lag = 0;
        p.stagger = !!(variant & 4096);
        p.grid = (unsigned)P.grid;
        /* timing ablations (results WRONG by design for 2, 3, 7): compiled
         * only by `make abl` */
        const int abl = ablations ? (variant >> 8) & 7 : 0;
        const int fit = (variant >> PANEL_FIT_VARIANT_SHIFT) & 3;
        if (abl == 5 || abl == 6) {
            /* tall-tile probe, the production launch shapes */
            p.k = {panel_threads_of_waves(waves), abl == 5 ? 2 : 1, 0, 8};
        } else if (abl) {
            p.k = {256, 1, 0, abl};
        } else if (P.wgs_per_cu == 1) {
            /* 512 lanes x 2 groups measured best with the 160 KiB tile
             * (1.53 ms on config 3; 1024 x 1: 1.60); bit 11 flips the groups */
            const int threads = panel_threads_of_waves(waves);
            p.k = {threads, (threads == 1024) != bit11 ? 1 : 2, 0, 0};
            /* nobody asked for a shape and the buckets are of the 512 x 2
             * class: the chunk that fits them (panel_fit_pays) */
            const double per_bucket =
                (double)P.nnz / ((double)P.tiles * (double)P.panels);
            if (waves <= 0 && !bit11 && fit == 0 && per_bucket >= 6000.0 &&
                panel_fit_pays(P))
                p.k = panel_fit_kernel(PANEL_FIT_SHAPE);
        } else if (waves > 0) { /* 2 groups of 4 per lane; bit 11: 1 */
            p.k = {waves < 8 ? 256 : 512, bit11 ? 1 : 2, 0, 0};
        } else {
            /* default: the chunk (threads x groups x 4 slots) that wastes
             * few lanes on the average bucket; 512 x 2 measured best on
             * config 3 (8000 entries per bucket) */
            const double per_bucket =
                (double)P.nnz / ((double)P.tiles * (double)P.panels);
            if (per_bucket >= 6000.0)
                p.k = {512, 2, 0, 0};
            else if (per_bucket >= 3000.0)
                p.k = {512, 1, 0, 0};
            else
                p.k = {256, 1, 0, 0};
        }
        if (p.k.abl == 0 && (fit == 1 || fit == 2))
            p.k = panel_fit_kernel(fit);
        p.k.det = P.det && p.k.abl == 0;
    } else {
        if (P.tiles <= 0 || P.xcd_max <= 0) {
            p.launches = 0;
            *out = p;
            return 0;
        }
        /* Which tile a workgroup runs (workgroups are dealt to the XCDs
         * round-robin).  0 GROUPED (default): groups of 32 consecutive tiles
         * -- one per CU of an XCD -- per XCD, the groups dealt round-robin, so
         * neighbouring tiles share an L2 AND the eight XCDs together advance
         * through one region of the matrix (and through rows of any density
         * together: no XCD idles on a matrix that is denser in one half).
         * 1 HARDWARE order: tile = workgroup index.  2 XCD-CONTIGUOUS ranges
         * of equal work.  Measured (round 2, tile 8192 unless noted; ms):
         *                      grouped  hardware  contiguous
         *   banded 10M x 32     0.615     0.619     0.642
         *   random W = 2^11     0.646     0.642     0.665
         *   random W = 2^17     0.672     0.755     0.654
         *   random W = 2^20     0.925     1.686     0.922   (20448 rows: 0.79 / 1.12 / 0.78)
         *   27-point stencil    0.473     0.485     0.499
         *   skewed rows 8.3M    0.171     0.176     0.174
         * variant bit 1 forces hardware order, bit 2 the contiguous ranges,
         * bits 14-15 a group size of 32 / 64 / 16 (experiments). */
        const int gsel = (variant >> 14) & 3;
        int ord = gsel ? 0 : (variant & 2) ? 1 : (variant & 4) ? 2 : P.order;
        if (ord == 0 && P.tiles >= (1 << 24))
            ord = 2; /* the packed (group, tiles) argument holds 24 bits of tiles */
        const int G = gsel == 2 ? 64 : gsel == 3 ? 16 : 32; /* < 128: 7 bits */
        p.order_arg = ord == 0 ? -((G << 24) | P.tiles) : ord == 1 ? P.tiles : 0;
        p.grid = ord == 0 ? (unsigned)((P.tiles + NUM_XCD * G - 1) /
                                       (NUM_XCD * G)) * NUM_XCD * G
                 : ord == 1 ? (unsigned)P.tiles
                            : (unsigned)(NUM_XCD * P.xcd_max);
        /* variant bit 0 flips the stored mode.  launch `step` of the steps
         * schedule handles the step-th NON-EMPTY bucket of every tile: a
         * matrix whose rows reach over k panels needs k launches, all tiles
         * busy in each of them; step 0 also zeroes the rows of empty tiles */
        const bool chain = P.chain != !!(variant & 1);
        const int steps = P.max_nbk > 0 ? P.max_nbk : 1;
        p.family = chain ? PANEL_CHAIN : PANEL_STEPS;
        if (!chain)
            p.launches = steps;
        const double per_bucket =
            (double)P.nnz / ((double)P.tiles * (double)steps);
        if (bit11) /* tuning: two groups of 4 per lane */
            p.k = {waves > 0 && waves < 8 ? 256 : 512, 2, 0, 0};
        else if (waves > 0 && waves != 8)
            p.k = {waves < 8 ? 256 : 1024, 1, 0, 0};
        else
            p.k = {waves == 8 || per_bucket >= 3000.0 ? 512 : 256, 1, 0, 0};
        /* deterministic: several groups of 4 entries per lane and turn -- the
         * hand-offs of the turn counter are what the mode costs, and they go
         * with the number of turns -- at most 512 lanes.  Four groups when
         * the tile fills a CU's LDS by itself (one workgroup per CU: W = 2^20,
         * 19552-row tiles, 0.797 ms vs 0.900 with two groups and 0.728 in the
         * default mode), two when two or more workgroups share the CU and
         * hide each other's hand-offs (four groups cost them occupancy:
         * 8192-row tiles at W = 2^17 0.690 vs 0.836 ms; default mode 0.604).
         * profiles/r05_det_cost.md.  The steps launches always take two. */
        if (P.det) {
            const bool alone =
                chain && (size_t)P.tile_rows * sizeof(double) > 80 * 1024;
            p.k = {p.k.threads <= 256 ? 256 : 512, alone ? 4 : 2, 1, 0};
        }
    }
    if (panel_plan_row(p, ablations) < 0)
        return -EINVAL;
    *out = p;
    return 0;
}

#endif /* SPMV_PANEL_LAUNCH_H */
