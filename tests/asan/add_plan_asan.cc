/*
 * The host arithmetic of the sparse sum (spmv_scpa_amd/csrc/add_plan.h)
 * under AddressSanitizer + UBSan: seeded (M, N, nzA, nzB, len-vector) inputs.
 *
 *   - every row is in exactly one class, in every mode; the lists of the two
 *     classes laid one after the other fill the list exactly
 *   - the group width is one of the widths, the smallest that is not below
 *     the mean, for entry counts up to 2^32 - 2
 *   - grids in 64 bits: enough teams for the rows, none to spare
 *   - the parts of the scratch are aligned, in order and do not overlap
 *   - the overflow guard and the matched count at nzA + nzB around INT32_MAX
 *
 * usage: add_plan_asan [inputs]
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "add_plan.h"

static int failures = 0;
#define CHECK(cond)                                                           \
    do {                                                                      \
        if (!(cond)) {                                                        \
            ++failures;                                                       \
            fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                     \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd(void) {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}
static int64_t below(int64_t n) { return n > 0 ? (int64_t)(rnd() % (uint64_t)n) : 0; }

static int64_t pick_size(void) {
    switch (rnd() % 6) {
    case 0: return below(4);
    case 1: return below(300);
    case 2: return below(100000);
    case 3: return INT32_MAX - below(3);
    case 4: return ((int64_t)1 << (rnd() % 31)) + below(3) - 1;
    default: return below(INT32_MAX);
    }
}

static int64_t pick_len(void) {
    switch (rnd() % 5) {
    case 0: return 0;
    case 1: return ADD_EDGE + below(3) - 1; /* e - 1, e, e + 1 */
    case 2: return below(2 * ADD_EDGE);
    case 3: return 2 * (int64_t)INT32_MAX - below(3); /* two full rows */
    default: return (int64_t)(rnd() >> (rnd() % 30 + 32));
    }
}

static void check_constants(void) {
    CHECK(ADD_THREADS % 64 == 0);
    CHECK(add_width(0) == ADD_WIDTH_MIN);
    CHECK(add_width(ADD_WIDTHS - 1) == ADD_WIDTH_MAX);
    for (int i = 0; i < ADD_WIDTHS; ++i) {
        const int w = add_width(i);
        CHECK((w & (w - 1)) == 0 && ADD_THREADS % w == 0 && w <= 32);
        CHECK(i == 0 || w == 2 * add_width(i - 1));
    }
    CHECK(ADD_EDGE >= ADD_WIDTH_MAX);
    CHECK(add_class(ADD_EDGE - 1, 0) == 0);
    CHECK(add_class(ADD_EDGE, 0) == 0);
    CHECK(add_class(ADD_EDGE + 1, 0) == 1);
    CHECK(add_class(0, 0) == 0 && add_class(INT64_MAX, 0) == 1);
    CHECK(add_class(INT64_MAX, 1) == 0 && add_class(0, 2) == 1);
}

static void check_guards(void) {
    const int64_t top = INT32_MAX;
    int64_t m = -1;
    CHECK(add_nz_guard(0) == 0);
    CHECK(add_nz_guard(top - 1) == 0);
    CHECK(add_nz_guard(top) == 0);
    CHECK(add_nz_guard(top + 1) == -EOVERFLOW);
    CHECK(add_nz_guard(2 * top) == -EOVERFLOW);
    CHECK(add_nz_guard(INT64_MAX) == -EOVERFLOW);
    CHECK(add_nz_guard(-1) == -EINVAL);
    /* nzA + nzB around INT32_MAX: the union may or may not fit */
    for (int64_t d = -2; d <= 2; ++d) {
        const int64_t nzA = top / 2 + 1, nzB = top - nzA + d; /* sum top + d */
        /* disjoint patterns: nz = nzA + nzB */
        CHECK(add_nz_guard(nzA + nzB) == (d > 0 ? -EOVERFLOW : 0));
        CHECK(add_matched(nzA, nzB, nzA + nzB, &m) == 0 && m == 0);
        /* one pattern inside the other: nz is the longer operand's, however
         * large the sum of the two */
        const int64_t more = nzA > nzB ? nzA : nzB, less = nzA + nzB - more;
        CHECK(add_nz_guard(more) == 0);
        CHECK(add_matched(nzA, nzB, more, &m) == 0 && m == less);
        CHECK(add_matched(nzA, nzB, nzA + nzB + 1, &m) == -EINVAL);
        CHECK(add_matched(nzA, nzB, more - 1, &m) == -EINVAL);
    }
    CHECK(add_matched(top, top, top, &m) == 0 && m == top);
    CHECK(add_matched(top, top, 2 * top, &m) == 0 && m == 0);
    CHECK(add_nz_guard(2 * top) == -EOVERFLOW);
    CHECK(add_matched(top + 1, 0, top + 1, &m) == -EINVAL);
    CHECK(add_matched(0, -1, 0, &m) == -EINVAL);
    CHECK(add_matched(1, 1, 1, NULL) == -EINVAL);
    add_plan p;
    CHECK(add_plan_make(-1, 1, 0, 0, &p) == -EINVAL);
    CHECK(add_plan_make(1, -1, 0, 0, &p) == -EINVAL);
    CHECK(add_plan_make(top + 1, 1, 0, 0, &p) == -EINVAL);
    CHECK(add_plan_make(1, top + 1, 0, 0, &p) == -EINVAL);
    CHECK(add_plan_make(1, 1, top + 1, 0, &p) == -EINVAL);
    CHECK(add_plan_make(1, 1, 0, top + 1, &p) == -EINVAL);
    CHECK(add_plan_make(1, 1, 0, 0, NULL) == -EINVAL);
    CHECK(add_plan_make(top, top, top, top, &p) == 0 && p.width == 2);
    CHECK(add_plan_make(1, top, top, top, &p) == 0 && p.width == 32);
    CHECK(add_plan_make(0, 0, 0, 0, &p) == 0 && p.width == 2);
}

static void check_input(void) {
    const int64_t M = rnd() % 4 ? below(3000) : pick_size();
    const int64_t N = pick_size();
    const int64_t nzA = pick_size(), nzB = rnd() % 3 ? pick_size() : nzA;
    add_plan p;
    CHECK(add_plan_make(M, N, nzA, nzB, &p) == 0);
    /* the width: one of the widths, the smallest not below the mean */
    int found = -1;
    for (int i = 0; i < ADD_WIDTHS; ++i)
        if (add_width(i) == p.width)
            found = i;
    CHECK(found >= 0);
    CHECK(p.width == add_pick_group(nzA + nzB, M));
    if (M > 0 && found >= 0) {
        const unsigned __int128 entries = (unsigned __int128)(nzA + nzB);
        if (found < ADD_WIDTHS - 1)
            CHECK((unsigned __int128)p.width * (unsigned __int128)M >= entries ||
                  nzA + nzB == 0);
        if (found > 0)
            CHECK((unsigned __int128)add_width(found - 1) *
                      (unsigned __int128)M < entries);
    }
    /* the scratch: aligned, in order, every part as long as it has to be */
    const int64_t off[5] = {p.off_head, p.off_count, p.off_list, p.off_sums,
                            p.scratch_bytes};
    const int64_t need[4] = {ADD_HEAD_WORDS * 8, (M + 1) * 4, M * 4,
                             add_ceil_div(M + 1, ADD_SCAN_TILE) * 4};
    CHECK(off[0] == 0);
    for (int i = 0; i < 4; ++i) {
        CHECK(off[i] % ADD_ALIGN == 0);
        CHECK(off[i] + need[i] <= off[i + 1]);
    }
    CHECK(p.scratch_bytes > 0);
    /* the rows: one class each in every mode; the lists tile [0, rows) */
    const int64_t rows = M < 3000 ? M : 3000; /* a sample of a huge M */
    std::vector<int64_t> len((size_t)rows);
    for (int64_t r = 0; r < rows; ++r)
        len[(size_t)r] = pick_len();
    for (int mode = 0; mode < 3; ++mode) {
        int64_t in_class[ADD_CLASSES] = {0, 0};
        for (int64_t r = 0; r < rows; ++r) {
            const int c = add_class(len[(size_t)r], mode);
            CHECK(c >= 0 && c < ADD_CLASSES);
            if (mode == 0)
                CHECK((c == 0) == (len[(size_t)r] <= ADD_EDGE));
            else
                CHECK(c == mode - 1);
            ++in_class[c];
        }
        std::vector<char> listed((size_t)rows, 0);
        int64_t at = 0;
        for (int c = 0; c < ADD_CLASSES; ++c) {
            const int64_t g = add_grid(c, p.width, in_class[c]);
            const int64_t teams = c == 0 ? ADD_THREADS / p.width : 1;
            CHECK(g >= 0 && g * teams >= in_class[c]);
            CHECK(in_class[c] == 0 || (g - 1) * teams < in_class[c]);
            for (int64_t i = 0; i < in_class[c]; ++i)
                listed[(size_t)(at + i)]++;
            at += in_class[c];
        }
        CHECK(at == rows);
        for (int64_t r = 0; r < rows; ++r)
            CHECK(listed[(size_t)r] == 1);
    }
    /* the largest grids a handle can ask for */
    CHECK(add_grid(0, ADD_WIDTH_MAX, INT32_MAX) ==
          add_ceil_div(INT32_MAX, ADD_THREADS / ADD_WIDTH_MAX));
    CHECK(add_grid(1, p.width, INT32_MAX) == INT32_MAX);
}

int main(int argc, char **argv) {
    const long inputs = argc > 1 ? atol(argv[1]) : 4000;
    check_constants();
    check_guards();
    for (long i = 0; i < inputs; ++i)
        check_input();
    if (failures) {
        printf("%d checks FAILED\n", failures);
        return 1;
    }
    printf("%ld inputs: every row in one class, the guards hold\n", inputs);
    return 0;
}
