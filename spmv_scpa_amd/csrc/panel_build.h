/*
 * panel_build.h -- the host arithmetic of building a blocked copy
 * (panels.hip, panels_build): the geometry a build derives from (M, N, slots,
 * options, CU count) before its first allocation, the segments of the long
 * rows kept beside the copy, and the tile ranges of the XCDs.
 *
 * Header-only and free of HIP, like panel_launch.h: integer decisions whose
 * thresholds were expensive to measure, so they run as a CPU test against a
 * table of plans written out from the panels_build() they were lifted from
 * (tests/asan/panel_build_asan.cc, tests/test_tune_blocked_asan.py).
 *
 * spmv_panel_opts comes from spmv_engine.h; NUM_XCD (hip_common.h) and
 * BIG_LDS_BYTES (panel_launch.h) from the headers before this one.
 */
#ifndef SPMV_PANEL_BUILD_H
#define SPMV_PANEL_BUILD_H

#include <algorithm>
#include <utility>
#include <vector>

#include "spmv_engine.h"
#include "panel_launch.h"

#define TILE_ROWS_STEPS 4096 /* "steps" schedule default: 32 KiB of LDS */
#define SWEEP_WG_PER_CU 2

/* rows of y one workgroup can hold when `per_cu` of them share a CU's LDS */
static inline int sweep_tile_rows_max(int per_cu) {
    /* the workgroups of a CU share 160 KiB; each carries a 128-byte static
     * ring besides its tile */
    return (int)((160 * 1024 - 128 * per_cu) / per_cu / 8 / 32 * 32);
}

/* tile height of the sweep schedule: the fewest rounds of (grid x tile_max)
 * rows that cover M, rows spread evenly over them */
static inline long long sweep_tile_rows(int M, int grid, int tile_max) {
    const long long rounds = ((long long)M + (long long)grid * tile_max - 1) /
                             ((long long)grid * tile_max);
    const long long wg = (rounds > 0 ? rounds : 1) * grid;
    long long tr = (((long long)M + wg - 1) / wg + 31) / 32 * 32;
    return tr < 32 ? 32 : tr;
}

static inline int bits_for(long long n) { /* smallest b with 2^b >= n */
    int b = 0;
    while ((1ll << b) < n)
        ++b;
    return b;
}

/* everything panels_build() decides before it touches the device */
struct panel_geometry {
    int sweep;       /* built for the persistent schedule */
    int chain;       /* steps layout, launched as one chain launch */
    int tile_rows;   /* rows per tile (multiple of 32) */
    int rbits;       /* bits of the row-in-tile field: 2^rbits >= tile_rows */
    int shift;       /* log2(columns per panel); rbits + shift <= 32 */
    int panels;      /* column panels */
    int tiles;       /* row tiles */
    int grid;        /* sweep: workgroups of the launch, at most the tiles */
    int wgs_per_cu;  /* sweep: workgroups sharing a CU's LDS */
    int reserve_cus; /* sweep: CUs left out of the grid */
    int pmajor;      /* sweep: buckets stored panel-major inside a round */
    int pm_grid;     /* tiles of such a round; 0: bucket ids are tile-major */
    int64_t nbuckets; /* bucket ids in use (the id of dropped slots) */
    int det;         /* ordered LDS additions */
    int order;       /* steps / chain: spmv_panel_opts.tile_order */
    int end_bit;     /* the radix sort runs over key bits [rbits, end_bit) */
};

/*
 * The geometry of one build: 0, -EINVAL (options), -EOVERFLOW (more than the
 * 32-bit tables hold), or what `device_cus` answered when negative.  `o`: the
 * options, already defaulted; `default_sched`: the process default that sched
 * < 0 stands for; `device_cus`: compute units of the device, asked ONLY by a
 * sweep build (steps and chain copies build on any device); `tall_rows`: 0,
 * or the tile height the tall-tile probe of a -DSPMV_ABLATIONS build forces
 * on a sweep copy.
 */
static inline int panel_build_plan(int M, int N, int64_t slots,
                                   const spmv_panel_opts &o, int default_sched,
                                   int (*device_cus)(void), long long tall_rows,
                                   panel_geometry *out) {
    if (slots > (int64_t)INT32_MAX)
        return -EOVERFLOW;
    if (o.struct_size != (int)sizeof(spmv_panel_opts))
        return -EINVAL; /* caller built against another header (ABI note) */
    if (o.sched > 2 || o.panel_cols < 0 || o.tile_rows < 0 ||
        o.sweep_wgs_per_cu < 0 || o.sweep_wgs_per_cu > 8 ||
        o.reserve_cus < 0 || o.lds_min < 0 || o.lds_min > BIG_LDS_BYTES ||
        o.tile_order < 0 || o.tile_order > 2 || o.sweep_layout < -1 ||
        o.sweep_layout > 1 || o.bucket_order < 0 || o.bucket_order > 1 ||
        o.deterministic < 0 || o.deterministic > 2)
        return -EINVAL;
    const int sched = o.sched < 0 ? default_sched : o.sched;
    panel_geometry g = {};
    g.sweep = sched == 1;
    g.chain = sched == 2;
    /* tile height.  steps: the taller the tile, the more entries of a bucket
     * share a line of x (fewer L2 requests) but the fewer workgroups there
     * are and the more LDS each holds; best measured per matrix: 2048 rows
     * for a band of 2^14 columns (0.68 ms), 8192 for 2^17 (0.84), 16384 for
     * 2^20 (1.18) and for skewed rows (0.21) -- spmv_*_autotune tries these.
     * sweep: sweep_tile_rows(). */
    long long tr = TILE_ROWS_STEPS;
    int grid = 0, tile_max = 20448 /* steps: 160 KiB of LDS */;
    int want_shift = 18; /* 2^18 columns = 2 MiB of x: half of an XCD's L2 */
    if (o.panel_cols > 0)
        want_shift = bits_for((long long)o.panel_cols + 1) - 1; /* floor(log2) */
    const int64_t cols = N > 0 ? N : 1;
    if (g.sweep) {
        /* one 1024-lane workgroup per CU with a 160 KiB tile, or two of up
         * to 512 lanes with 80 KiB tiles.  The tall tile halves the panel
         * (row and column index share 32 bits) but puts twice the entries
         * on a line of x, which the column-sorted buckets turn into fewer
         * L2 requests: 1.61 vs 1.77 ms on config 3.  It needs buckets that
         * fill its 4096-slot chunks, so it is taken only above 4000 entries
         * per bucket (80 M columns, 1071 per bucket: 4.85 vs 3.35 ms). */
        int cus = device_cus();
        if (cus < 0)
            return cus;
        if (o.reserve_cus > 0) /* keep at least one XCD's worth of CUs */
            cus = cus - o.reserve_cus >= NUM_XCD ? cus - o.reserve_cus : NUM_XCD;
        g.wgs_per_cu = o.sweep_wgs_per_cu;
        if (g.wgs_per_cu == 0) {
            const long long tr1 = sweep_tile_rows(M, cus, sweep_tile_rows_max(1));
            const int sh = std::min(want_shift, 32 - bits_for(tr1));
            const double tiles1 = (double)(((long long)M + tr1 - 1) / tr1);
            const double panels1 = (double)(((cols - 1) >> sh) + 1);
            /* no rows, no buckets to fill: an empty matrix takes two */
            const bool full = tiles1 > 0
                                  ? (double)slots / (tiles1 * panels1) >= 4000.0
                                  : slots > 0;
            g.wgs_per_cu = full ? 1 : SWEEP_WG_PER_CU;
        }
        grid = cus * g.wgs_per_cu;
        tile_max = sweep_tile_rows_max(g.wgs_per_cu);
        tr = sweep_tile_rows(M, grid, tile_max);
        if (tall_rows > 0) {
            g.wgs_per_cu = 1;
            grid = cus;
            tr = tall_rows;
        }
    } else if (o.tile_rows >= 32 && o.tile_rows <= tile_max) {
        tr = o.tile_rows / 32 * 32;
    }
    g.tile_rows = (int)tr;
    g.rbits = bits_for(tr);
    /* row-in-tile and column-in-panel share a word */
    g.shift = std::min(want_shift, 32 - g.rbits);
    g.panels = (int)(((cols - 1) >> g.shift) + 1);
    g.tiles = (int)(((long long)M + tr - 1) / tr);
    /* bucket tables are indexed with int (hipCUB scan length) */
    if ((uint64_t)(g.tiles > 0 ? g.tiles : 1) * (uint64_t)g.panels >=
        (uint64_t)INT32_MAX)
        return -EOVERFLOW;
    if (g.sweep) {
        g.grid = grid < g.tiles ? grid : (g.tiles > 0 ? g.tiles : 1);
        g.reserve_cus = o.reserve_cus;
        /* panel-major is the default (-1): 1.448 vs 1.464 ms on config 3,
         * 2.88 vs 2.96 ms on one shard of the 80M-column problem, and the
         * masked tail blocks re-read a cached line instead of fetching
         * another bucket */
        g.pmajor = o.sweep_layout != 0;
    }
    /* 0 = default: ordered additions on sweep layouts (free there: the
     * hand-offs hide under the request-bound loop, +-2 %), arrival order on
     * chain / steps (+3..+10 % there); 1 = always, 2 = never */
    g.det = o.deterministic == 1 || (o.deterministic == 0 && g.sweep);
    g.order = g.sweep ? 0 : o.tile_order;
    /* bucket ids: tile-major, or panel-major inside rounds of g.grid tiles */
    g.pm_grid = g.pmajor ? g.grid : 0;
    g.nbuckets = g.pm_grid ? (int64_t)((g.tiles + g.pm_grid - 1) / g.pm_grid) *
                                 g.panels * g.pm_grid
                           : (int64_t)g.tiles * g.panels;
    if ((uint64_t)g.nbuckets >= (uint64_t)INT32_MAX)
        return -EOVERFLOW;
    /* sort only the bits in use: bucket ids up to nbuckets (the id of
     * dropped slots) above `shift` column bits; the row field below them
     * rides along unsorted (entry_key) */
    const int kb = g.shift + g.rbits;
    g.end_bit = kb + 1;
    while (g.end_bit < 64 && (((uint64_t)g.nbuckets) >> (g.end_bit - kb)))
        ++g.end_bit;
    *out = g;
    return 0;
}

/* ---- long rows beside the copy (struct spmv_panels, "LONG ROWS") ---- */
/* threshold: the second launch costs ~8 us; a row inside the copy costs its
 * tile ~1.3 ns per entry of serialised accumulation -- power-law 1M x 3 with
 * one row of 8291 entries: 0.043 ms inside, 0.052 beside; a row of 30 000+
 * entries is worth the launch (4M rows: 0.155 -> 0.127 ms) */
#define PANELS_LONG_ROW 16384
#ifndef PANELS_LONG_SEG
#define PANELS_LONG_SEG 1024
#endif
#define PANELS_LONG_MAX 4096 /* more such rows than this: keep them inside */

struct panel_long_seg { /* laid out as the int2 the kernel reads */
    int row;   /* index into the list of long rows */
    int first; /* first entry, counted over all long rows */
};
static_assert(sizeof(panel_long_seg) == 2 * sizeof(int), "uploaded as int2");

struct panel_long_rows {
    std::vector<int> row;  /* [n] row index, ascending */
    std::vector<int> ptr;  /* [n + 1] first entry of each */
    std::vector<int> seg0; /* [n] first segment of each */
    std::vector<panel_long_seg> seg; /* PANELS_LONG_SEG entries each */
    int64_t nnz;
};

/* `list` as the device wrote it: [0] the number of long rows (it may exceed
 * PANELS_LONG_MAX, pairs beyond that were not stored), then (row, length)
 * pairs in any order.  false: nothing goes beside the copy -- there are no
 * such rows, too many, or more entries in them than an int indexes */
static inline bool panel_long_segments(const int *list, panel_long_rows *out) {
    if (list[0] <= 0 || list[0] > PANELS_LONG_MAX)
        return false;
    std::vector<std::pair<int, int>> rows; /* (row, length) */
    for (int k = 0; k < list[0]; ++k)
        rows.push_back({list[1 + 2 * k], list[2 + 2 * k]});
    std::sort(rows.begin(), rows.end());
    *out = panel_long_rows();
    int64_t at = 0;
    for (size_t h = 0; h < rows.size(); ++h) {
        if (at + rows[h].second > (int64_t)INT32_MAX)
            return false; /* keep them inside */
        out->row.push_back(rows[h].first);
        out->ptr.push_back((int)at);
        out->seg0.push_back((int)out->seg.size());
        for (int64_t b = 0; b < rows[h].second; b += PANELS_LONG_SEG)
            out->seg.push_back({(int)h, (int)(at + b)});
        at += rows[h].second;
    }
    out->ptr.push_back((int)at);
    out->nnz = at;
    return true;
}

/* ---- steps / chain: contiguous tile ranges of about equal entry counts, one
 * per XCD.  st[0 .. tiles]: start slot of every tile and the end of the last
 * one; fills xcd_first[0 .. NUM_XCD] and returns the longest range ---- */
static inline int panel_xcd_ranges(const int64_t *st, int tiles, int *xcd_first) {
    const int64_t total = st[tiles] - st[0];
    xcd_first[0] = 0;
    for (int k = 1; k < NUM_XCD; ++k) {
        /* first tile whose start reaches k/8 of the entries; every tile
         * also counts one slot so that empty tiles spread evenly */
        const double want = (double)(total + tiles) * k / NUM_XCD;
        int lo = xcd_first[k - 1], hi = tiles;
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if ((double)(st[mid] - st[0] + mid) < want)
                lo = mid + 1;
            else
                hi = mid;
        }
        xcd_first[k] = lo;
    }
    xcd_first[NUM_XCD] = tiles;
    int xcd_max = 0;
    for (int k = 0; k < NUM_XCD; ++k)
        xcd_max = std::max(xcd_max, xcd_first[k + 1] - xcd_first[k]);
    return xcd_max;
}

#endif /* SPMV_PANEL_BUILD_H */
