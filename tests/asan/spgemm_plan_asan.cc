/*
 * The host arithmetic of the sparse product (spmv_scpa_amd/csrc/spgemm_plan.h)
 * under AddressSanitizer + UBSan: seeded (M, K, N, ub-vector) inputs.
 *
 *   - every row is in exactly one class, and classes 0..2 hold it in a table
 *     strictly larger than its ub (in fact at least twice as large)
 *   - the LDS of a workgroup holds its teams' parts, aligned and in bounds
 *   - the parts of the scratch are aligned, in order and do not overlap; the
 *     class lists laid one after the other fill the list exactly
 *   - the fallback's batches cover every wide row once, its slots do not
 *     overlap and stay within the bound (or are one row's)
 *   - the guards hold at INT32_MAX - 1, INT32_MAX, INT32_MAX + 1 and for ub
 *     sums beyond 2^32
 *
 * usage: spgemm_plan_asan [inputs]
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "spgemm_plan.h"

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

static int64_t pick_ub(void) {
    const int c = (int)(rnd() % 3);
    switch (rnd() % 5) {
    case 0: return 0;
    case 1: return spgemm_edge(c) + below(3) - 1; /* e - 1, e, e + 1 */
    case 2: return below(2 * spgemm_edge(2));
    case 3: return ((int64_t)1 << 32) + below(1000);
    default: return (int64_t)(rnd() >> (rnd() % 40 + 2));
    }
}

static void check_classes(void) {
    CHECK(SPGEMM_THREADS % 64 == 0);
    for (int c = 0; c < 3; ++c) {
        const int t = spgemm_table(c), team = spgemm_team(c);
        CHECK((t & (t - 1)) == 0);
        CHECK(spgemm_edge(c) * 2 == t && spgemm_edge(c) < t);
        CHECK(c == 0 || spgemm_edge(c) > spgemm_edge(c - 1));
        CHECK(SPGEMM_THREADS % team == 0);
        CHECK(team <= 64 || team == SPGEMM_THREADS);
        /* the parts of a team: values, keys, touched, count */
        const int64_t values = 0, keys = t / 2 * 8, touched = keys + t * 4,
                      count = touched + t / 2;
        CHECK(values % 8 == 0 && keys % 8 == 0 && count % 8 == 0);
        CHECK(count + 8 == spgemm_team_lds(c));
        CHECK(spgemm_team_lds(c) % 8 == 0);
        CHECK(spgemm_lds(c) ==
              spgemm_team_lds(c) * (SPGEMM_THREADS / team));
        CHECK(spgemm_lds(c) <= 160 * 1024 - 256);
        CHECK(spgemm_class(spgemm_edge(c) - 1) == c);
        CHECK(spgemm_class(spgemm_edge(c)) == c);
        CHECK(spgemm_class(spgemm_edge(c) + 1) == c + 1);
    }
    CHECK(spgemm_class(0) == 0);
    CHECK(spgemm_class(INT64_MAX) == 3);
}

static void check_guards(void) {
    CHECK(spgemm_nz_guard(0) == 0);
    CHECK(spgemm_nz_guard((int64_t)INT32_MAX - 1) == 0);
    CHECK(spgemm_nz_guard((int64_t)INT32_MAX) == 0);
    CHECK(spgemm_nz_guard((int64_t)INT32_MAX + 1) == -EOVERFLOW);
    CHECK(spgemm_nz_guard((int64_t)46341 * 46341) == -EOVERFLOW);
    CHECK(spgemm_nz_guard(((int64_t)1 << 32) + 5) == -EOVERFLOW);
    CHECK(spgemm_nz_guard(INT64_MAX) == -EOVERFLOW);
    CHECK(spgemm_nz_guard(-1) == -EINVAL);
    spgemm_plan p;
    spgemm_fallback f;
    CHECK(spgemm_plan_make(-1, 1, 1, &p) == -EINVAL);
    CHECK(spgemm_plan_make(1, (int64_t)INT32_MAX + 1, 1, &p) == -EINVAL);
    CHECK(spgemm_plan_make(1, 1, (int64_t)INT32_MAX + 1, &p) == -EINVAL);
    CHECK(spgemm_plan_make((int64_t)INT32_MAX + 1, 1, 1, &p) == -EINVAL);
    CHECK(spgemm_plan_make(INT32_MAX, INT32_MAX, INT32_MAX, &p) == 0);
    CHECK(spgemm_plan_make(1, 1, 1, NULL) == -EINVAL);
    CHECK(spgemm_fallback_make(-1, 1, &f) == -EINVAL);
    CHECK(spgemm_fallback_make((int64_t)INT32_MAX + 1, 1, &f) == -EINVAL);
    CHECK(spgemm_fallback_make(INT32_MAX, INT32_MAX, &f) == 0);
    CHECK(f.batch == 1 && f.launches == INT32_MAX);
}

static void check_input(void) {
    const int64_t M = rnd() % 4 ? below(3000) : pick_size();
    const int64_t K = pick_size(), N = pick_size();
    spgemm_plan p;
    CHECK(spgemm_plan_make(M, K, N, &p) == 0);
    /* the scratch: aligned, in order, every part as long as it has to be */
    const int64_t off[6] = {p.off_head, p.off_ub,   p.off_count,
                            p.off_list, p.off_sums, p.scratch_bytes};
    const int64_t need[5] = {SPGEMM_HEAD_WORDS * 8, M * 8, (M + 1) * 4, M * 4,
                             spgemm_ceil_div(M + 1, SPGEMM_SCAN_TILE) * 4};
    CHECK(off[0] == 0);
    for (int i = 0; i < 5; ++i) {
        CHECK(off[i] % SPGEMM_ALIGN == 0);
        CHECK(off[i] + need[i] <= off[i + 1]);
    }
    CHECK(p.scratch_bytes > 0);
    /* the rows: one class each; the lists tile [0, rows) */
    const int64_t rows = M < 3000 ? M : 3000; /* a sample of a huge M */
    std::vector<int64_t> ub((size_t)rows);
    int64_t in_class[SPGEMM_CLASSES] = {0, 0, 0, 0};
    unsigned __int128 sum = 0;
    for (int64_t r = 0; r < rows; ++r) {
        ub[(size_t)r] = pick_ub();
        sum += (unsigned __int128)ub[(size_t)r];
        const int c = spgemm_class(ub[(size_t)r]);
        CHECK(c >= 0 && c < SPGEMM_CLASSES);
        int holds = 0;
        for (int k = 0; k < 3; ++k)
            holds += ub[(size_t)r] <= spgemm_edge(k) &&
                     (k == 0 || ub[(size_t)r] > spgemm_edge(k - 1));
        holds += ub[(size_t)r] > spgemm_edge(2);
        CHECK(holds == 1);
        if (c < 3)
            CHECK(spgemm_table(c) > ub[(size_t)r]);
        ++in_class[c];
    }
    CHECK(sum >= (unsigned __int128)0); /* 128-bit: the sum itself is fine */
    std::vector<char> listed((size_t)rows, 0);
    int64_t at = 0;
    for (int c = 0; c < SPGEMM_CLASSES; ++c) {
        if (c < 3) {
            const int64_t g = spgemm_grid(c, in_class[c]);
            const int64_t teams = SPGEMM_THREADS / spgemm_team(c);
            CHECK(g * teams >= in_class[c]);
            CHECK(in_class[c] == 0 || (g - 1) * teams < in_class[c]);
        }
        for (int64_t i = 0; i < in_class[c]; ++i)
            listed[(size_t)(at + i)]++;
        at += in_class[c];
    }
    CHECK(at == rows);
    for (int64_t r = 0; r < rows; ++r)
        CHECK(listed[(size_t)r] == 1);
    /* the fallback: every wide row in one batch, slots apart */
    const int64_t wide = rnd() % 3 ? in_class[3] : below(INT32_MAX);
    spgemm_fallback f;
    CHECK(spgemm_fallback_make(N, wide, &f) == 0);
    CHECK(f.words * 32 >= N && (f.words - 1) * 32 < N);
    CHECK(f.acc_stride >= N * 8 && f.acc_stride % SPGEMM_ALIGN == 0);
    CHECK(f.bits_stride >= f.words * 4 && f.bits_stride % SPGEMM_ALIGN == 0);
    CHECK(f.batch <= SPGEMM_FALLBACK_MAX_BATCH && f.batch <= wide);
    if (wide == 0) {
        CHECK(f.batch == 0 && f.launches == 0 && f.scratch_bytes == 0);
    } else {
        CHECK(f.batch >= 1);
        CHECK(f.scratch_bytes <= SPGEMM_FALLBACK_BYTES || f.batch == 1);
        CHECK(f.off_acc == 0 && f.off_bits == f.batch * f.acc_stride);
        CHECK(f.off_bits % SPGEMM_ALIGN == 0);
        CHECK(f.off_bits + f.batch * f.bits_stride == f.scratch_bytes);
        CHECK(f.launches == spgemm_ceil_div(wide, f.batch));
        int64_t covered = 0, first = 0, count = 0;
        const int64_t walk = f.launches < 5000 ? f.launches : 5000;
        for (int64_t l = 0; l < walk; ++l) {
            spgemm_fallback_batch(&f, wide, l, &first, &count);
            CHECK(first == covered && count >= 1 && count <= f.batch);
            covered += count;
        }
        if (walk == f.launches) {
            CHECK(covered == wide);
        } else { /* the last one */
            spgemm_fallback_batch(&f, wide, f.launches - 1, &first, &count);
            CHECK(first + count == wide && count >= 1 && count <= f.batch);
        }
    }
}

int main(int argc, char **argv) {
    const long inputs = argc > 1 ? atol(argv[1]) : 4000;
    check_classes();
    check_guards();
    for (long i = 0; i < inputs; ++i)
        check_input();
    if (failures) {
        printf("%d checks FAILED\n", failures);
        return 1;
    }
    printf("%ld inputs: every row in one class, every batch covered once\n",
           inputs);
    return 0;
}
