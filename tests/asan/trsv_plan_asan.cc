// CPU test of the triangular solve's host arithmetic
// (spmv_scpa_amd/csrc/trsv_plan.h) under ASan + UBSan.
//
// 1. The launch list at its edges: no level, one level, a level of exactly
//    small_rows rows and of one more, runs at both ends, empty levels, the
//    count-only call, a cap shorter than the list, the refusals.
// 2. Seeded random level_ptr: the segments cover every level once and in
//    order, a wide segment is one level of more than small_rows rows, a chain
//    is a MAXIMAL run of the others, the count equals the list.
// 3. The analysis restated on the host with the kernels' index arithmetic --
//    count, scan, fill, the successor lists, Kahn with frontiers and rotating
//    counters, the stable sort by level, the gather -- every array a heap
//    block of exactly the size trsv_sizes_make plans: an index outside it is
//    an ASan report.  The result is compared with the definitions.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "trsv_plan.h"

static int failures;
#define CHECK(cond, ...)                                                       \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::printf("FAILED %s: ", #cond);                                 \
            std::printf(__VA_ARGS__);                                          \
            std::printf("\n");                                                 \
            ++failures;                                                        \
        }                                                                      \
    } while (0)

static uint64_t rng_state = 88172645463325252ULL;
static uint64_t rnd(void) {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

// the invariants of a launch list, for any level_ptr
static void check_list(const std::vector<int> &level_ptr, int small) {
    const int levels = (int)level_ptr.size() - 1;
    const int64_t n = trsv_segments(level_ptr.data(), levels, small, NULL, 0);
    CHECK(n >= 0 && n <= levels, "count %lld of %d levels", (long long)n, levels);
    if (n < 0)
        return;
    // a heap block of exactly n segments
    trsv_segment *seg = new trsv_segment[(size_t)n ? (size_t)n : 1];
    CHECK(trsv_segments(level_ptr.data(), levels, small, seg, n) == n, "fill");
    int next = 0;
    for (int64_t i = 0; i < n; ++i) {
        CHECK(seg[i].first_level == next, "segment %lld starts at %d, not %d",
              (long long)i, seg[i].first_level, next);
        CHECK(seg[i].last_level >= seg[i].first_level && seg[i].last_level < levels,
              "segment %lld ends at %d", (long long)i, seg[i].last_level);
        if (seg[i].last_level < seg[i].first_level || seg[i].last_level >= levels)
            break;
        for (int l = seg[i].first_level; l <= seg[i].last_level; ++l) {
            const int rows = level_ptr[l + 1] - level_ptr[l];
            if (seg[i].kind == TRSV_WIDE)
                CHECK(rows > small && seg[i].last_level == seg[i].first_level,
                      "wide level %d of %d rows", l, rows);
            else
                CHECK(seg[i].kind == TRSV_CHAIN && rows <= small,
                      "chain level %d of %d rows", l, rows);
        }
        if (i > 0) // maximal: two chains never touch
            CHECK(!(seg[i].kind == TRSV_CHAIN && seg[i - 1].kind == TRSV_CHAIN),
                  "chains %lld and %lld touch", (long long)i - 1, (long long)i);
        next = seg[i].last_level + 1;
    }
    CHECK(next == levels, "covered %d of %d levels", next, levels);
    if (n > 1) { // a cap shorter than the list: the count, nothing past cap
        trsv_segment *few = new trsv_segment[(size_t)n - 1];
        CHECK(trsv_segments(level_ptr.data(), levels, small, few, n - 1) == n,
              "short cap");
        delete[] few;
    }
    delete[] seg;
}

static std::vector<int> ptr_of(const std::vector<int> &rows) {
    std::vector<int> p(rows.size() + 1, 0);
    for (size_t i = 0; i < rows.size(); ++i)
        p[i + 1] = p[i] + rows[i];
    return p;
}

static int64_t count_of(const std::vector<int> &rows, int small) {
    const std::vector<int> p = ptr_of(rows);
    check_list(p, small);
    return trsv_segments(p.data(), (int)rows.size(), small, NULL, 0);
}

static void check_edges(void) {
    const int L = TRSV_SMALL_ROWS;
    CHECK((TRSV_GROUP & (TRSV_GROUP - 1)) == 0 && TRSV_GROUP >= 2, "group");
    CHECK((L & (L - 1)) == 0 && (TRSV_THREADS & (TRSV_THREADS - 1)) == 0,
          "powers of two");
    CHECK(TRSV_THREADS % TRSV_GROUP == 0 && TRSV_WIDE_THREADS % TRSV_GROUP == 0,
          "lane groups fill a workgroup");
    const int zero = 0;
    CHECK(trsv_segments(&zero, 0, L, NULL, 0) == 0, "no level");
    CHECK(trsv_segments(NULL, 0, L, NULL, 0) == 0, "no level, no array");
    CHECK(count_of({1}, L) == 1 && count_of({L}, L) == 1, "one thin level");
    CHECK(count_of({L + 1}, L) == 1, "one wide level");
    CHECK(count_of({5, L - 1}, L) == 1 && count_of({5, L}, L) == 1, "fan");
    CHECK(count_of({5, L + 1}, L) == 2 && count_of({5, 3 * L + 5}, L) == 2,
          "fan, wide");
    CHECK(count_of({3, 2, L + 7, 4, 1}, L) == 3, "sandwich");
    CHECK(count_of({L + 1, L + 1, L + 1}, L) == 3, "wide only");
    CHECK(count_of({L + 1, 1, L + 1, 1, 1, L + 1}, L) == 5, "alternating");
    CHECK(count_of({0, 0, L + 1, 0}, L) == 3, "empty levels are thin");
    CHECK(count_of(std::vector<int>(6323, 1), L) == 1, "6323 thin levels");
    CHECK(count_of({7, 9}, 0) == 2, "small_rows 0: every level wide");
    const int bad[3] = {0, 5, 3};
    CHECK(trsv_segments(bad, 2, L, NULL, 0) == -EINVAL, "decreasing");
    CHECK(trsv_segments(NULL, 1, L, NULL, 0) == -EINVAL, "NULL level_ptr");
    CHECK(trsv_segments(&zero, -1, L, NULL, 0) == -EINVAL, "levels < 0");
    CHECK(trsv_segments(&zero, 0, -1, NULL, 0) == -EINVAL, "small_rows < 0");
    CHECK(trsv_segments(bad, 1, L, NULL, 1) == -EINVAL, "cap without out");
    CHECK(trsv_wide_grid(1, 256) == 1 && trsv_wide_grid(256 / TRSV_GROUP, 256) == 1 &&
              trsv_wide_grid(256 / TRSV_GROUP + 1, 256) == 2 &&
              trsv_wide_grid(INT32_MAX, 64) ==
                  ((int64_t)INT32_MAX + 64 / TRSV_GROUP - 1) / (64 / TRSV_GROUP),
          "wide grid");
    trsv_sizes z;
    CHECK(trsv_sizes_make(-1, 0, 0, &z) == -EINVAL &&
              trsv_sizes_make(1, 1, 2, &z) == -EINVAL &&
              trsv_sizes_make(1, 1, 1, NULL) == -EINVAL &&
              trsv_sizes_make(INT32_MAX, 0, 0, &z) == -EINVAL &&
              trsv_sizes_make(1, (int64_t)INT32_MAX + 1, 0, &z) == -EINVAL,
          "sizes refused");
    CHECK(trsv_sizes_make(INT32_MAX - 1, INT32_MAX, INT32_MAX, &z) == 0 &&
              z.frontier == 2 * (int64_t)(INT32_MAX - 1) && z.cnt == INT32_MAX,
          "largest sizes do not wrap");
}

static void check_random(int n) {
    for (int k = 0; k < n; ++k) {
        const int levels = (int)(rnd() % 40);
        const int small = (int)(rnd() % 3 == 0 ? rnd() % 8 : TRSV_SMALL_ROWS);
        std::vector<int> rows((size_t)levels);
        for (auto &r : rows)
            r = (int)(rnd() % 4 == 0 ? small + 1 + rnd() % 5
                                     : rnd() % (uint64_t)(small + 1));
        count_of(rows, small);
    }
}

// ---- the analysis, with the kernels' index arithmetic ----
static void scan_exclusive(int *data, int64_t n) {
    int run = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int t = data[i];
        data[i] = run;
        run += t;
    }
}

static bool strict(int c, int i, int upper) { return upper ? c > i : c < i; }

static void check_analysis(int M, int max_row, int upper) {
    // a matrix with both triangles, unsorted, duplicates, some rows without a
    // diagonal
    std::vector<int> irp((size_t)M + 1, 0), ja;
    std::vector<double> as;
    for (int i = 0; i < M; ++i) {
        const int n = (int)(rnd() % (uint64_t)(max_row + 1));
        for (int e = 0; e < n; ++e) {
            ja.push_back((int)(rnd() % (uint64_t)M));
            as.push_back((double)(rnd() % 1000) / 8.0 - 60.0);
        }
        irp[(size_t)i + 1] = (int)ja.size();
    }
    const int64_t NZ = (int64_t)ja.size();
    trsv_sizes z;
    CHECK(trsv_sizes_make(M, NZ, 0, &z) == 0, "sizes");
    // k_trsv_count
    int *cnt = new int[(size_t)z.cnt]();
    double *diag = new double[(size_t)z.diag ? (size_t)z.diag : 1];
    for (int i = 0; i < M; ++i) {
        int n = 0;
        double d = 0.0;
        for (int64_t e = irp[i]; e < irp[i + 1]; ++e) {
            const int c = ja[(size_t)e];
            if (c == i)
                d += as[(size_t)e];
            else if (strict(c, i, upper))
                ++n;
        }
        cnt[i] = n;
        diag[i] = d;
    }
    scan_exclusive(cnt, z.cnt);
    const int snz = cnt[M];
    CHECK(trsv_sizes_make(M, NZ, snz, &z) == 0, "sizes with SNZ");
    auto block = [](int64_t n) { return new int[(size_t)n ? (size_t)n : 1]; };
    int *sja = block(z.sja), *spos = block(z.spos);
    for (int i = 0; i < M; ++i) { // k_trsv_fill
        int64_t at = cnt[i];
        const int64_t stop = cnt[i + 1];
        for (int64_t e = irp[i]; e < irp[i + 1] && at < stop; ++e)
            if (strict(ja[(size_t)e], i, upper)) {
                sja[at] = ja[(size_t)e];
                spos[at] = (int)e;
                ++at;
            }
        CHECK(at == stop, "row %d filled to %lld of %lld", i, (long long)at,
              (long long)stop);
    }
    // the successor lists: the stable transposition of the strict pattern
    int *succ_ptr = new int[(size_t)z.succ_ptr](), *succ = block(z.succ);
    for (int64_t e = 0; e < snz; ++e)
        ++succ_ptr[sja[e]];
    scan_exclusive(succ_ptr, z.succ_ptr);
    {
        std::vector<int> at(succ_ptr, succ_ptr + M);
        for (int i = 0; i < M; ++i)
            for (int64_t e = cnt[i]; e < cnt[i + 1]; ++e)
                succ[at[(size_t)sja[e]]++] = i;
    }
    // Kahn: k_trsv_kahn_init, then one k_trsv_kahn_step per level
    int *indeg = block(z.indeg), *frontier = block(z.frontier);
    int *counters = new int[(size_t)z.counters]();
    int *iota = new int[(size_t)z.iota];
    std::vector<int> level((size_t)M, -1);
    for (int i = 0; i <= M; ++i) {
        iota[i] = i;
        if (i == M)
            break;
        indeg[i] = cnt[i + 1] - cnt[i];
        level[(size_t)i] = 0;
        if (indeg[i] == 0)
            frontier[counters[0]++] = i;
    }
    int levels = 0, nf = counters[0];
    int64_t placed = 0;
    while (nf > 0) {
        CHECK(levels < M, "more levels than rows");
        placed += nf;
        int *from = frontier + (int64_t)(levels & 1) * M;
        int *to = frontier + (int64_t)((levels + 1) & 1) * M;
        int *next_count = counters + (levels + 1) % 3;
        counters[(levels + 2) % 3] = 0;
        // the frontier in REVERSE: its order must not matter
        for (int t = nf - 1; t >= 0; --t) {
            const int r = from[t];
            for (int64_t e = succ_ptr[r]; e < succ_ptr[r + 1]; ++e) {
                const int w = succ[e];
                if (indeg[w]-- == 1) {
                    level[(size_t)w] = levels + 1;
                    to[(*next_count)++] = w;
                }
            }
        }
        nf = *next_count;
        ++levels;
    }
    CHECK(placed == M, "placed %lld of %d rows", (long long)placed, M);
    // level by its definition
    std::vector<int> want((size_t)M, 0);
    for (int s = 0; s < M; ++s) {
        const int i = upper ? M - 1 - s : s;
        for (int64_t e = irp[i]; e < irp[i + 1]; ++e)
            if (strict(ja[(size_t)e], i, upper))
                want[(size_t)i] = std::max(want[(size_t)i],
                                           1 + want[(size_t)ja[(size_t)e]]);
    }
    CHECK(level == want, "levels of M %d", M);
    CHECK(levels == (M ? *std::max_element(want.begin(), want.end()) + 1 : 0),
          "level count %d", levels);
    // order, level_ptr: the counting sort of the rows by level
    int *level_ptr = new int[(size_t)levels + 1]();
    int *order = block(M), *rowptr = new int[(size_t)M + 1]();
    for (int i = 0; i < M; ++i)
        ++level_ptr[level[(size_t)i]];
    scan_exclusive(level_ptr, (int64_t)levels + 1);
    {
        std::vector<int> at(level_ptr, level_ptr + levels);
        for (int i = 0; i < M; ++i)
            order[at[(size_t)level[(size_t)iota[i]]]++] = iota[i];
    }
    std::vector<int> sorted((size_t)M);
    std::iota(sorted.begin(), sorted.end(), 0);
    std::stable_sort(sorted.begin(), sorted.end(), [&](int a, int b) {
        return level[(size_t)a] < level[(size_t)b];
    });
    CHECK(std::equal(sorted.begin(), sorted.end(), order), "order");
    CHECK(level_ptr[levels] == M, "level_ptr ends at %d", level_ptr[levels]);
    // k_trsv_newcnt, scan, k_trsv_gather
    for (int p = 0; p < M; ++p)
        rowptr[p] = cnt[order[p] + 1] - cnt[order[p]];
    scan_exclusive(rowptr, (int64_t)M + 1);
    CHECK(rowptr[M] == snz, "rowptr ends at %d of %d", rowptr[M], snz);
    int *pja = block(z.sja);
    double *pas = new double[(size_t)z.sja ? (size_t)z.sja : 1];
    for (int p = 0; p < M; ++p) {
        const int r = order[p];
        const int64_t src = cnt[r], dst = rowptr[p];
        const int64_t n = std::min(cnt[r + 1] - cnt[r], rowptr[p + 1] - rowptr[p]);
        for (int64_t j = 0; j < n; ++j) {
            pja[dst + j] = sja[src + j];
            pas[dst + j] = as[(size_t)spos[src + j]];
        }
    }
    bool same = true;
    for (int p = 0; p < M; ++p) { // against the definition of the copy
        const int i = order[p];
        int64_t at = rowptr[p];
        for (int64_t e = irp[i]; e < irp[i + 1]; ++e)
            if (strict(ja[(size_t)e], i, upper)) {
                same = same && pja[at] == ja[(size_t)e] && pas[at] == as[(size_t)e];
                ++at;
            }
        same = same && at == rowptr[p + 1];
    }
    CHECK(same, "copy of M %d", M);
    // the launch list of these levels
    check_list(std::vector<int>(level_ptr, level_ptr + levels + 1),
               TRSV_SMALL_ROWS);
    check_list(std::vector<int>(level_ptr, level_ptr + levels + 1), 3);
    delete[] cnt;
    delete[] diag;
    delete[] sja;
    delete[] spos;
    delete[] succ_ptr;
    delete[] succ;
    delete[] indeg;
    delete[] frontier;
    delete[] counters;
    delete[] iota;
    delete[] level_ptr;
    delete[] order;
    delete[] rowptr;
    delete[] pja;
    delete[] pas;
}

int main(int argc, char **argv) {
    const int n = argc > 1 ? std::atoi(argv[1]) : 2000;
    check_edges();
    check_random(n);
    for (int upper = 0; upper < 2; ++upper) {
        check_analysis(0, 0, upper);
        check_analysis(1, 3, upper);
        check_analysis(2, 4, upper);
        check_analysis(65, 0, upper);    // no entry at all
        check_analysis(300, 2, upper);
        check_analysis(1000, 12, upper);
        check_analysis(5000, 6, upper);
        check_analysis(40, 200, upper);  // rows far longer than the matrix
    }
    if (failures) {
        std::printf("%d checks FAILED\n", failures);
        return 1;
    }
    std::printf("launch lists hold, levels and copies are the definitions "
                "(%d random lists)\n", n);
    return 0;
}
