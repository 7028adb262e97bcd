/*
 * The host arithmetic of smoothed-aggregation AMG (spmv_scpa_amd/csrc/
 * amg_plan.h) under AddressSanitizer + UBSan: seeded inputs.
 *
 *   - the key of a row: bit 63 clear, the row comes back, two rows of one
 *     seed never share a key, a root's key is above every undecided key and
 *     every undecided key is at or above the out key 0; the order of two
 *     undecided keys is the order of (hash, row)
 *   - the scratch layout: every vector of every level aligned, in order,
 *     not overlapping, inside the allocation -- checked by WRITING every
 *     element of every vector of a real allocation of small hierarchies, and
 *     by arithmetic for level sizes up to INT32_MAX
 *   - the grid of a launch covers its items and refuses what no grid holds
 *   - the launch count of an apply equals a count of the launch list
 *   - the refusals of amg_layout_make
 *
 * usage: amg_plan_asan [inputs]
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "amg_plan.h"

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
static int64_t below(int64_t n) {
    return n > 0 ? (int64_t)(rnd() % (uint64_t)n) : 0;
}

static int pick_rows(void) {
    switch (rnd() % 5) {
    case 0: return (int)below(4);
    case 1: return (int)below(300);
    case 2: return (int)below(100000);
    case 3: return INT32_MAX - (int)below(3);
    default: return (int)below(INT32_MAX);
    }
}

static void check_keys(void) {
    const uint32_t seed = (uint32_t)rnd();
    const uint32_t a = (uint32_t)below((int64_t)1 << 31);
    const uint32_t b = (uint32_t)below((int64_t)1 << 31);
    const uint64_t ka = amg_key(a, seed), kb = amg_key(b, seed);
    CHECK(!amg_key_is_root(ka) && amg_key_row(ka) == a);
    CHECK(amg_key_is_root(ka | AMG_KEY_ROOT));
    CHECK(amg_key_row(ka | AMG_KEY_ROOT) == a);
    CHECK((ka | AMG_KEY_ROOT) > kb);
    CHECK((a == b) == (ka == kb));
    const uint32_t ha = amg_fmix32(a ^ seed), hb = amg_fmix32(b ^ seed);
    CHECK((ka < kb) == (ha < hb || (ha == hb && a < b)));
    /* the largest row and the largest hash stay below bit 63 */
    CHECK(!amg_key_is_root((uint64_t)0xffffffffu << 31 | 0x7fffffffu));
    CHECK(amg_max_rounds(0) == AMG_DEFAULT_MAX_ROUNDS);
    CHECK(amg_max_rounds(7) == 7);
}

/* the launch list of spmv_amg_apply, counted: a sweep is one launch (fused)
 * or a product and a vector kernel; the refill exists only for the latter */
static int count_launches(int levels, int sweeps, int coarse, int fused) {
    const int per = fused ? 1 : 2;
    int n = 0;
    for (int l = 0; l < levels; ++l) {
        ++n; /* first */
        if (l == levels - 1) {
            n += per * (coarse - 1);
            break;
        }
        n += per * (sweeps - 1);
        n += 2; /* residual, restriction */
    }
    for (int l = levels - 2; l >= 0; --l)
        n += 1 + (fused ? 0 : 1) + per * sweeps; /* prolongation, refill */
    return n;
}

static void check_layout(bool real) {
    const int levels = 1 + (int)below(AMG_MAX_LEVELS);
    const int kmax = 1 + (int)below(AMG_MAX_K);
    int rows[AMG_MAX_LEVELS];
    for (int l = 0; l < levels; ++l)
        rows[l] = real ? (int)below(2000) : pick_rows();
    struct amg_layout lay;
    CHECK(amg_layout_make(rows, levels, kmax, &lay) == 0);
    CHECK(lay.levels == levels);
    int64_t at = 0;
    const int64_t per = AMG_ALIGN / 8;
    for (int l = 0; l < levels; ++l) {
        const int64_t v = amg_vec_doubles(rows[l], kmax);
        CHECK(v % per == 0 && v >= (int64_t)rows[l] * kmax && v >= 0);
        CHECK(lay.r[l] == at && lay.r[l] % per == 0);
        at += v;
        CHECK(lay.x2[l] == at);
        at += v;
        if (l == 0) {
            CHECK(lay.x[l] == -1 && lay.b[l] == -1);
            continue;
        }
        CHECK(lay.x[l] == at);
        at += v;
        CHECK(lay.b[l] == at);
        at += v;
    }
    CHECK(lay.doubles == at);
    if (real) { /* every element of every vector, in a real allocation */
        std::vector<double> scratch((size_t)lay.doubles);
        double *base = scratch.data();
        for (int l = 0; l < levels; ++l) {
            const int64_t n = (int64_t)rows[l] * kmax;
            for (int64_t i = 0; i < n; ++i) {
                base[lay.r[l] + i] += 1.0;
                base[lay.x2[l] + i] += 1.0;
                if (l) {
                    base[lay.x[l] + i] += 1.0;
                    base[lay.b[l] + i] += 1.0;
                }
            }
        }
        for (double d : scratch)
            CHECK(d == 0.0 || d == 1.0); /* no element written twice */
    }
    const int sweeps = 1 + (int)below(AMG_MAX_SWEEPS);
    const int coarse = 1 + (int)below(AMG_MAX_SWEEPS);
    for (int fused = 0; fused < 2; ++fused)
        CHECK(amg_apply_launches(levels, sweeps, coarse, fused) ==
              count_launches(levels, sweeps, coarse, fused));
    /* the iterate ends at home whatever the number of swaps */
    const int swaps = (int)below(200);
    CHECK(((amg_start_buffer(swaps) + swaps) & 1) == 0);
}

static void check_grid(void) {
    const int64_t n = rnd() % 4 ? below((int64_t)8 * INT32_MAX + 10)
                                : below(1000);
    unsigned g = 0;
    const int rc = amg_grid(n, &g);
    CHECK(rc == 0); /* M * k <= 8 * INT32_MAX items always have a grid */
    CHECK((int64_t)g * AMG_T >= n && g >= 1);
    CHECK(((int64_t)g - 1) * AMG_T < (n > 0 ? n : 1));
    CHECK(amg_grid((int64_t)AMG_T * 0x7fffffff + 1, &g) == -EOVERFLOW);
}

static void check_refusals(void) {
    int rows[2] = {5, -1};
    struct amg_layout lay;
    CHECK(amg_layout_make(NULL, 1, 1, &lay) == -EINVAL);
    CHECK(amg_layout_make(rows, 1, 1, NULL) == -EINVAL);
    CHECK(amg_layout_make(rows, 0, 1, &lay) == -EINVAL);
    CHECK(amg_layout_make(rows, AMG_MAX_LEVELS + 1, 1, &lay) == -EINVAL);
    CHECK(amg_layout_make(rows, 1, 0, &lay) == -EINVAL);
    CHECK(amg_layout_make(rows, 1, AMG_MAX_K + 1, &lay) == -EINVAL);
    CHECK(amg_layout_make(rows, 2, 1, &lay) == -EINVAL);
    CHECK(amg_layout_make(rows, 1, 8, &lay) == 0 && lay.doubles == 128);
    const int64_t nz[3] = {10, 3, 1};
    CHECK(amg_complexity(nz, 3) == 1.4);
    CHECK(amg_complexity(nz, 0) == 0.0);
}

int main(int argc, char **argv) {
    const int inputs = argc > 1 ? atoi(argv[1]) : 4000;
    check_refusals();
    for (int i = 0; i < inputs; ++i) {
        check_keys();
        check_layout(i % 8 == 0);
        check_grid();
    }
    if (failures) {
        printf("amg_plan_asan: %d FAILED\n", failures);
        return 1;
    }
    printf("amg_plan_asan: %d inputs, every vector in its own part of the "
           "scratch\n", inputs);
    return 0;
}
