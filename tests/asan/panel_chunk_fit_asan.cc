// CPU test of the sweep's chunk-fit rule (spmv_scpa_amd/csrc/panel_launch.h,
// "Chunk fit") under ASan + UBSan.
//
// 1. The rule on both sides of its threshold, with the counted steps zeroed,
//    and beside every way of asking for a shape (waves, waves_hint, variant
//    bit 11, variant bits 16-17, two workgroups per CU, small buckets).
// 2. Seeded random shapes WITH counted steps: every plan names a kernel that
//    the product flavour instantiates, and a copy without counted steps plans
//    what the same copy planned before the field existed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

// NUM_XCD and SPMV_VARIANT_TIMING_BITS (hip_common.h) come as -D macros
#include "panel_launch.h"

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

// the headline's copy: one workgroup per CU, 77 panels, 512 tiles of 19552
// rows, 32 entries per row, ordered additions
static panel_shape headline(void) {
    panel_shape s = {};
    s.sweep = 1;
    s.det = 1;
    s.wgs_per_cu = 1;
    s.panels = 77;
    s.tiles = 512;
    s.nnz = 320000000LL;
    s.tile_rows = 19552;
    s.grid = 256;
    return s;
}

static panel_kernel plan_of(const panel_shape &s, int waves, int variant,
                            bool abl = false) {
    panel_plan p = {};
    const int rc = panel_launch_plan(s, waves, variant, abl, &p);
    CHECK(rc == 0, "rc %d (waves %d, variant %d)", rc, waves, variant);
    CHECK(panel_plan_row(p, abl) >= 0, "<%d, %d, %d, %d> not instantiated",
          p.k.threads, p.k.q, p.k.det, p.k.abl);
    return p.k;
}

static bool is(const panel_kernel &k, int threads, int q, int det) {
    return k.threads == threads && k.q == q && k.det == det && k.abl == 0;
}

static void check_rule(void) {
    const panel_kernel fit = panel_fit_kernel(PANEL_FIT_SHAPE);
    CHECK(fit.threads * fit.q * 4 == PANEL_FIT_CHUNK, "%d x %d", fit.threads,
          fit.q);
    CHECK(panel_fit_kernel(1).threads * panel_fit_kernel(1).q * 4 ==
                  PANEL_FIT_CHUNK &&
              panel_fit_kernel(2).threads * panel_fit_kernel(2).q * 4 ==
                  PANEL_FIT_CHUNK,
          "a sibling's chunk is not %d", PANEL_FIT_CHUNK);
    panel_shape s = headline();
    // not counted: the built-in shape
    CHECK(is(plan_of(s, 0, 0), 512, 2, 1), "zeroed field");
    // the threshold: 10 % fewer steps, exactly / one step short of it
    s.fit_steps[0] = 100000;
    s.fit_steps[1] = 90000;
    CHECK(is(plan_of(s, 0, 0), fit.threads, fit.q, 1), "at the threshold");
    CHECK(is(plan_of(s, 0, SPMV_VARIANT_TIMING_BITS), fit.threads, fit.q, 1),
          "timing bit");
    s.fit_steps[1] = 90001;
    CHECK(is(plan_of(s, 0, 0), 512, 2, 1), "just under the threshold");
    s.fit_steps[1] = 100000;
    CHECK(is(plan_of(s, 0, 0), 512, 2, 1), "no gain");
    s.fit_steps[1] = 120000;
    CHECK(is(plan_of(s, 0, 0), 512, 2, 1), "a loss");
    // the headline's own counts (about 194 -> 153 steps per tile and round)
    s.fit_steps[0] = 99400;
    s.fit_steps[1] = 78848;
    CHECK(is(plan_of(s, 0, 0), fit.threads, fit.q, 1), "headline, ordered");
    s.det = 0;
    CHECK(is(plan_of(s, 0, 0), fit.threads, fit.q, 0), "headline, arrival order");
    s.det = 1;
    // half of the field missing: not counted
    s.fit_steps[0] = 0;
    CHECK(is(plan_of(s, 0, 0), 512, 2, 1), "only [1] set");
    s.fit_steps[0] = 99400;
    s.fit_steps[1] = 0;
    CHECK(is(plan_of(s, 0, 0), 512, 2, 1), "only [0] set");
    s.fit_steps[1] = 78848;
    // an explicit request keeps its meaning
    CHECK(is(plan_of(s, 8, 0), 512, 2, 1), "waves 8");
    CHECK(is(plan_of(s, 4, 0), 256, 2, 1), "waves 4");
    CHECK(is(plan_of(s, 6, 0), 256, 2, 1), "waves 6");
    CHECK(is(plan_of(s, 9, 0), 1024, 1, 1), "waves 9");
    CHECK(is(plan_of(s, 16, 0), 1024, 1, 1), "waves 16");
    s.waves_hint = 8;
    CHECK(is(plan_of(s, 0, 0), 512, 2, 1), "waves_hint 8");
    s.waves_hint = 16;
    CHECK(is(plan_of(s, 0, 0), 1024, 1, 1), "waves_hint 16");
    s.waves_hint = 0;
    CHECK(is(plan_of(s, 0, 1 << 11, true), 512, 1, 1), "variant bit 11");
    CHECK(is(plan_of(s, 0, 3 << 16), 512, 2, 1), "variant: built-in shape");
    CHECK(is(plan_of(s, 0, 1 << 16), 576, 2, 1), "variant: 576 x 2");
    CHECK(is(plan_of(s, 0, 2 << 16), 384, 3, 1), "variant: 384 x 3");
    CHECK(is(plan_of(s, 16, 2 << 16), 384, 3, 1), "variant beats waves");
    // ... also on a copy without counted steps
    s.fit_steps[0] = s.fit_steps[1] = 0;
    CHECK(is(plan_of(s, 0, 1 << 16), 576, 2, 1), "variant, zeroed field");
    CHECK(is(plan_of(s, 0, 2 << 16), 384, 3, 1), "variant, zeroed field");
    s.fit_steps[0] = 99400;
    s.fit_steps[1] = 78848;
    // the ablation arms keep their kernels
    CHECK(plan_of(s, 0, 1 << 8, true).abl == 1, "ablation arm 1");
    CHECK(plan_of(s, 0, (1 << 8) | (1 << 16), true).abl == 1,
          "ablation arm 1 with a fit request");
    // outside the rule's class: two workgroups per CU, small buckets
    s.wgs_per_cu = 2;
    CHECK(is(plan_of(s, 0, 0), 512, 2, 1), "two workgroups per CU");
    s.wgs_per_cu = 1;
    s.nnz = (int64_t)5999 * s.tiles * s.panels;
    CHECK(is(plan_of(s, 0, 0), 512, 2, 1), "5999 entries per bucket");
    s.nnz = (int64_t)6000 * s.tiles * s.panels;
    CHECK(is(plan_of(s, 0, 0), fit.threads, fit.q, 1), "6000 entries per bucket");
    // chain / steps copies never read the field
    panel_shape c = {};
    c.chain = 1;
    c.panels = 8;
    c.tiles = 1221;
    c.nnz = 7326000LL;
    c.max_nbk = 3;
    c.tile_rows = 8192;
    c.xcd_max = 153;
    const panel_kernel before = plan_of(c, 0, 0);
    c.fit_steps[0] = 100;
    c.fit_steps[1] = 1;
    const panel_kernel after = plan_of(c, 0, 0);
    CHECK(before.threads == after.threads && before.q == after.q,
          "chain copy: <%d, %d> became <%d, %d>", before.threads, before.q,
          after.threads, after.q);
}

static uint64_t st;
static uint64_t rnd(void) {
    uint64_t z = (st += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static int pick(int n) { return (int)(rnd() % (uint64_t)n); }

static void scenario(uint64_t seed) {
    st = seed;
    const bool abl = rnd() & 1;
    panel_shape s = {};
    s.sweep = pick(4) != 0;
    s.chain = pick(2);
    s.det = pick(2);
    s.wgs_per_cu = 1 + pick(2);
    s.panels = 1 + pick(400);
    s.tiles = 1 + pick(5000);
    s.max_nbk = pick(s.panels + 1);
    s.nnz = (int64_t)(rnd() % 12000) * s.tiles * (s.sweep ? s.panels : 3);
    s.tile_rows = 32 * (1 + pick(639));
    s.waves_hint = pick(2) ? 0 : pick(17);
    s.grid = 8 * (1 + pick(64));
    s.xcd_max = (s.tiles + NUM_XCD - 1) / NUM_XCD + pick(3);
    const int waves = pick(3) ? 0 : pick(18) - 1;
    int variant = pick(8) | (pick(2) ? SPMV_VARIANT_TIMING_BITS : 0) |
                  (pick(3) ? 0 : pick(4) << PANEL_FIT_VARIANT_SHIFT);
    if (abl)
        variant |= (int)(rnd() & rnd() & 0xDFF0);
    panel_plan legacy = {};
    int rc = panel_launch_plan(s, waves, variant, abl, &legacy);
    CHECK(rc == 0, "seed %llu: rc %d", (unsigned long long)seed, rc);
    // any counts at all, the absurd included
    s.fit_steps[0] = pick(5) ? (int64_t)(rnd() % 4000000) : (pick(2) ? 0 : INT64_MAX / 200);
    s.fit_steps[1] = pick(5) ? (int64_t)(rnd() % 4000000) : (pick(2) ? 0 : INT64_MAX / 200);
    panel_plan p = {};
    rc = panel_launch_plan(s, waves, variant, abl, &p);
    CHECK(rc == 0, "seed %llu: rc %d", (unsigned long long)seed, rc);
    if (rc || !p.launches)
        return;
    CHECK(panel_plan_row(p, abl) >= 0, "seed %llu: <%d, %d, %d, %d>",
          (unsigned long long)seed, p.k.threads, p.k.q, p.k.det, p.k.abl);
    CHECK(abl || panel_plan_row(p, false) >= 0, "seed %llu",
          (unsigned long long)seed);
    CHECK(p.k.det == (s.det && p.k.abl == 0), "seed %llu: det %d",
          (unsigned long long)seed, p.k.det);
    // the counts change the kernel's shape and nothing else, and only to the
    // named sibling, only where nobody asked for a shape
    const bool changed =
        p.k.threads != legacy.k.threads || p.k.q != legacy.k.q;
    CHECK(p.family == legacy.family && p.lag == legacy.lag &&
              p.lds == legacy.lds && p.grid == legacy.grid &&
              p.launches == legacy.launches && p.k.abl == legacy.k.abl,
          "seed %llu: more than the shape changed", (unsigned long long)seed);
    if (changed) {
        const panel_kernel fit = panel_fit_kernel(PANEL_FIT_SHAPE);
        const int eff_waves = waves > 0 ? waves : s.waves_hint;
        CHECK(p.k.threads == fit.threads && p.k.q == fit.q,
              "seed %llu: <%d, %d>", (unsigned long long)seed, p.k.threads,
              p.k.q);
        CHECK(s.sweep && s.wgs_per_cu == 1 && eff_waves <= 0 &&
                  !(variant & (1 << 11)) &&
                  !(variant & PANEL_FIT_VARIANT_BITS) && panel_fit_pays(s) &&
                  legacy.k.threads == 512 && legacy.k.q == 2,
              "seed %llu: the rule fired outside its class",
              (unsigned long long)seed);
    }
}

int main(int argc, char **argv) {
    const int n = argc > 1 ? std::atoi(argv[1]) : 4000;
    check_rule();
    for (int i = 0; i < n; ++i)
        scenario(0xc4f17ull + (uint64_t)i * 7919u);
    if (failures) {
        std::printf("chunk fit: %d FAILED checks\n", failures);
        return 1;
    }
    std::printf("chunk fit: the rule holds on both sides of its threshold, %d "
                "random inputs, every plan names an instantiated kernel\n", n);
    return 0;
}
