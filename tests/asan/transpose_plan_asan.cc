// CPU test of the transposition's host arithmetic
// (spmv_scpa_amd/csrc/transpose_plan.h) under ASan + UBSan.
//
// 1. The plan at the edges of every quantity: pass counts around the digit
//    boundaries, workgroups around the tile, the scratch layout (parts in
//    order, aligned, inside the allocation), no 32-bit wrap at the largest
//    handle, the refusals.
// 2. Seeded random (N, NZ): the same invariants, and scratch monotone in NZ.
// 3. The sort restated on the host with the plan's numbers and the kernels'
//    index arithmetic (counter[digit * workgroups + w], the three-launch scan
//    over TRANSPOSE_SCAN_TILE ints, base + stable rank), every array a
//    heap block of exactly the planned size: an index outside it is an ASan
//    report.  The result is compared with std::stable_sort.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "transpose_plan.h"

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

static void check_layout(int64_t N, int64_t NZ) {
    transpose_plan p;
    const int rc = transpose_plan_make(N, NZ, &p);
    CHECK(rc == 0, "rc %d at N %lld NZ %lld", rc, (long long)N, (long long)NZ);
    if (rc)
        return;
    const int d = p.digit_bits;
    CHECK(d == TRANSPOSE_DIGIT_BITS && p.tile == TRANSPOSE_TILE, "constants");
    // passes: the smallest count whose digits hold N - 1, at least 1
    CHECK(p.passes >= 1 && p.passes <= (31 + d - 1) / d, "passes %d", p.passes);
    if (N > 1) {
        CHECK(((N - 1) >> (int64_t)(p.passes * d)) == 0 || p.passes * d >= 63,
              "N %lld does not fit %d passes", (long long)N, p.passes);
        CHECK(p.passes == 1 || ((N - 1) >> ((p.passes - 1) * d)) != 0,
              "N %lld needs fewer than %d passes", (long long)N, p.passes);
    } else {
        CHECK(p.passes == 1, "N %lld: %d passes", (long long)N, p.passes);
    }
    CHECK(p.workgroups * p.tile >= NZ && NZ > (p.workgroups - 1) * p.tile,
          "workgroups %lld for NZ %lld", (long long)p.workgroups,
          (long long)NZ);
    CHECK(p.counters == p.workgroups << d, "counters");
    CHECK(p.buffers == (NZ == 0 ? 0 : 2), "buffers %d", p.buffers);
    CHECK(p.scan_sums >= transpose_scan_tiles(p.counters) &&
              p.scan_sums >= transpose_scan_tiles(N + 1),
          "scan sums");
    // the parts: in order, aligned, large enough, inside the allocation
    const int64_t pair_bytes = NZ * 8;
    int64_t at = 0;
    for (int k = 0; k < 2; ++k) {
        CHECK(p.off_pairs[k] == at, "pairs[%d] at %lld", k,
              (long long)p.off_pairs[k]);
        if (k < p.buffers)
            at += transpose_align_up(pair_bytes);
    }
    CHECK(p.off_counters == at, "counters at");
    CHECK(p.off_sums - p.off_counters >= p.counters * 4, "counters size");
    CHECK(p.off_flag - p.off_sums >= p.scan_sums * 4, "sums size");
    CHECK(p.scratch_bytes - p.off_flag >= 4, "flag size");
    CHECK(p.off_counters % TRANSPOSE_ALIGN == 0 &&
              p.off_sums % TRANSPOSE_ALIGN == 0 &&
              p.off_flag % TRANSPOSE_ALIGN == 0 &&
              p.scratch_bytes % TRANSPOSE_ALIGN == 0,
          "alignment");
    CHECK(p.scratch_bytes >= p.buffers * pair_bytes + p.counters * 4,
          "scratch %lld", (long long)p.scratch_bytes);
}

static int passes_of(int64_t N) {
    transpose_plan p;
    return transpose_plan_make(N, 0, &p) ? -1 : p.passes;
}

static void check_edges(void) {
    const int d = TRANSPOSE_DIGIT_BITS;
    CHECK(passes_of(0) == 1 && passes_of(1) == 1 && passes_of(2) == 1, "small");
    for (int k = 1; k * d < 31; ++k) {
        CHECK(passes_of((int64_t)1 << (k * d)) == k, "2^%d", k * d);
        CHECK(passes_of(((int64_t)1 << (k * d)) + 1) == k + 1, "2^%d + 1",
              k * d);
    }
    CHECK(passes_of(INT32_MAX) == (31 + d - 1) / d, "INT32_MAX");
    transpose_plan p;
    CHECK(transpose_plan_make(-1, 0, &p) == -EINVAL, "N < 0");
    CHECK(transpose_plan_make(0, -1, &p) == -EINVAL, "NZ < 0");
    CHECK(transpose_plan_make((int64_t)INT32_MAX + 1, 0, &p) == -EINVAL, "N");
    CHECK(transpose_plan_make(1, (int64_t)INT32_MAX + 1, &p) == -EINVAL, "NZ");
    CHECK(transpose_plan_make(1, 1, NULL) == -EINVAL, "NULL");
    const int64_t t = TRANSPOSE_TILE;
    const int64_t nzs[] = {0, 1, 63, 64, 65, t - 1, t, t + 1, 3 * t + 17,
                           320000000, INT32_MAX};
    const int64_t ns[] = {0, 1, 2, 255, 256, 257, 65536, 65537,
                          (1 << 24) + 1, 10000000, INT32_MAX};
    for (int64_t nz : nzs)
        for (int64_t n : ns)
            check_layout(n, nz);
    // the largest handle, written out: no 32-bit wrap anywhere
    CHECK(transpose_plan_make(INT32_MAX, INT32_MAX, &p) == 0, "largest");
    const int64_t wgs = ((int64_t)INT32_MAX + t - 1) / t;
    CHECK(p.workgroups == wgs, "workgroups %lld", (long long)p.workgroups);
    CHECK(p.counters == wgs * TRANSPOSE_RADIX, "counters");
    const int64_t sums = ((int64_t)INT32_MAX + 1) / TRANSPOSE_SCAN_TILE;
    CHECK(p.scan_sums == sums, "scan sums %lld", (long long)p.scan_sums);
    const int64_t want = 2 * transpose_align_up((int64_t)INT32_MAX * 8) +
                         wgs * TRANSPOSE_RADIX * 4 + sums * 4 + TRANSPOSE_ALIGN;
    CHECK(p.scratch_bytes == want, "scratch %lld want %lld",
          (long long)p.scratch_bytes, (long long)want);
    CHECK(p.scratch_bytes > ((int64_t)1 << 35), "wrapped");
}

static void check_random(int n) {
    for (int k = 0; k < n; ++k) {
        const int64_t N = (int64_t)(rnd() >> (33 + rnd() % 31));
        const int64_t NZ = (int64_t)(rnd() >> (33 + rnd() % 31));
        check_layout(N, NZ);
        transpose_plan a, b;
        if (NZ < INT32_MAX && !transpose_plan_make(N, NZ, &a) &&
            !transpose_plan_make(N, NZ + 1, &b))
            CHECK(b.scratch_bytes >= a.scratch_bytes, "not monotone at %lld",
                  (long long)NZ);
    }
}

// ---- the sort, with the kernels' index arithmetic ----
static void scan_exclusive(int *data, int64_t n, int *sums) {
    const int64_t tiles = transpose_scan_tiles(n);
    for (int64_t b = 0; b < tiles; ++b) { // k_tr_scan_local
        int run = 0;
        for (int64_t i = b * TRANSPOSE_SCAN_TILE;
             i < std::min(n, (b + 1) * TRANSPOSE_SCAN_TILE); ++i) {
            const int t = data[i];
            data[i] = run;
            run += t;
        }
        sums[b] = run;
    }
    if (tiles <= 1)
        return;
    int carry = 0; // k_tr_scan_sums
    for (int64_t b = 0; b < tiles; ++b) {
        const int t = sums[b];
        sums[b] = carry;
        carry += t;
    }
    for (int64_t b = 0; b < tiles; ++b) // k_tr_scan_add
        for (int64_t i = b * TRANSPOSE_SCAN_TILE;
             i < std::min(n, (b + 1) * TRANSPOSE_SCAN_TILE); ++i)
            data[i] += sums[b];
}

static void check_sort(int64_t N, int64_t NZ, int hub_percent) {
    transpose_plan p;
    if (transpose_plan_make(N, NZ, &p)) {
        CHECK(false, "plan");
        return;
    }
    std::vector<int> ja((size_t)NZ);
    for (auto &c : ja)
        c = (int)(rnd() % 100 < (uint64_t)hub_percent ? N / 2 : rnd() % N);
    // each part a heap block of exactly the planned size
    const size_t pair_ints = (size_t)(NZ * 2);
    int *pairs[2] = {new int[pair_ints ? pair_ints : 1],
                     new int[pair_ints ? pair_ints : 1]};
    int *counters = new int[(size_t)p.counters ? (size_t)p.counters : 1];
    int *sums = new int[(size_t)p.scan_sums ? (size_t)p.scan_sums : 1];
    int *irp = new int[(size_t)N + 1]();
    for (int c : ja)
        ++irp[c];
    scan_exclusive(irp, N + 1, sums);
    CHECK(irp[N] == NZ && irp[0] == 0, "irp");
    for (int pass = 0; pass < p.passes; ++pass) {
        const int shift = pass * p.digit_bits;
        const int *src = pass ? pairs[(pass - 1) & 1] : NULL;
        int *dst = pairs[pass & 1];
        auto key = [&](int64_t i) { return pass ? src[2 * i] : ja[(size_t)i]; };
        auto digit = [&](int64_t i) {
            return ((unsigned)key(i) >> shift) & (TRANSPOSE_RADIX - 1);
        };
        for (int64_t w = 0; w < p.workgroups; ++w) {
            int cnt[TRANSPOSE_RADIX] = {0};
            for (int64_t i = w * p.tile; i < std::min(NZ, (w + 1) * p.tile); ++i)
                ++cnt[digit(i)];
            for (int dg = 0; dg < TRANSPOSE_RADIX; ++dg)
                counters[(int64_t)dg * p.workgroups + w] = cnt[dg];
        }
        scan_exclusive(counters, p.counters, sums);
        for (int64_t w = 0; w < p.workgroups; ++w) {
            unsigned running[TRANSPOSE_RADIX];
            for (int dg = 0; dg < TRANSPOSE_RADIX; ++dg)
                running[dg] = (unsigned)counters[(int64_t)dg * p.workgroups + w];
            for (int64_t i = w * p.tile; i < std::min(NZ, (w + 1) * p.tile);
                 ++i) {
                const unsigned at = running[digit(i)]++;
                dst[2 * (size_t)at] = key(i);
                dst[2 * (size_t)at + 1] = pass ? src[2 * i + 1] : (int)i;
            }
        }
    }
    const int *sorted = pairs[(p.passes - 1) & 1];
    std::vector<int> order((size_t)NZ);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(),
                     [&](int a, int b) { return ja[a] < ja[b]; });
    bool same = true;
    for (int64_t q = 0; q < NZ; ++q)
        same = same && sorted[2 * q + 1] == order[(size_t)q] &&
               sorted[2 * q] == ja[(size_t)order[(size_t)q]];
    CHECK(same, "sort of N %lld NZ %lld", (long long)N, (long long)NZ);
    delete[] pairs[0];
    delete[] pairs[1];
    delete[] counters;
    delete[] sums;
    delete[] irp;
}

int main(int argc, char **argv) {
    const int n = argc > 1 ? std::atoi(argv[1]) : 2000;
    check_edges();
    check_random(n);
    const int64_t t = TRANSPOSE_TILE;
    const int64_t ns[] = {1, 2, 255, 256, 257, 65537, (1 << 24) + 1};
    const int64_t nzs[] = {0, 1, 65, t - 1, t, t + 1, 3 * t + 17};
    for (int64_t N : ns)
        for (int64_t NZ : nzs)
            check_sort(N, NZ, N > 2 ? 30 : 0);
    check_sort(1000, 40 * t + 5, 100); // one column holds every entry
    check_sort(70000, 600 * t + 1, 33); // counters beyond one scan tile
    if (failures) {
        std::printf("%d checks FAILED\n", failures);
        return 1;
    }
    std::printf("plans hold, sorts are stable (%d random plans)\n", n);
    return 0;
}
