// CPU test of the solvers' work-buffer layout
// (spmv_scpa_amd/csrc/solver_work.h) under ASan + UBSan.
//
// For each of the six buffers (cg, pcg, pcg_trsv, bicgstab, cgls, minres),
// k = 1..8, M and N in {0, 1, 255, 256, 257, 1000} (cgls with M != N too, both
// ways round):
// 1. the regions -- state, sets of partial sums, vectors -- are 8-byte aligned,
//    in order and disjoint, the state region holds the solver's state size,
//    the last region ends exactly at the total;
// 2. the total is the closed formula the solvers' *_work_bytes used to state,
//    written out here;
// 3. over a heap block of exactly the total, the first and the last byte of
//    every region are written: a region past the end is an ASan report.
// Then the total at M = N = 2^31 - 1, k = 8 (no allocation) and the refusals.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "solver_work.h"

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

static const int64_t PART = 65536; // 1024 workgroup sums of 8 columns

struct expect {
    const char *name;
    int64_t state, parts, vectors; // what the layout must describe
    int64_t total;                 // the closed formula
};

static int layouts;

static void check_layout(const solver_work &w, const expect &e, int64_t M,
                         int64_t N, int k) {
    ++layouts;
    const int64_t total = solver_work_bytes(w);
    CHECK(total == e.total, "%s M %lld N %lld k %d: %lld bytes, not %lld",
          e.name, (long long)M, (long long)N, k, (long long)total,
          (long long)e.total);
    CHECK(w.state_bytes == e.state && w.parts == e.parts &&
              w.vectors == e.vectors && w.vectors <= SOLVER_WORK_MAXV,
          "%s: state %lld, %d parts, %d vectors", e.name,
          (long long)w.state_bytes, w.parts, w.vectors);
    if (total < 0 || total != e.total)
        return;
    // the regions in order: [begin, end)
    int64_t begin[1 + 8 + SOLVER_WORK_MAXV], end[1 + 8 + SOLVER_WORK_MAXV];
    int n = 0;
    begin[n] = 0;
    end[n++] = solver_work_part(w, 0);
    CHECK(end[0] == e.state, "%s: the state region holds %lld bytes", e.name,
          (long long)end[0]);
    for (int i = 0; i < w.parts; ++i) {
        begin[n] = solver_work_part(w, i);
        end[n++] = solver_work_part(w, i + 1);
        CHECK(end[n - 1] - begin[n - 1] == PART, "%s: part %d", e.name, i);
    }
    CHECK(solver_work_part(w, w.parts) == solver_work_vec(w, 0),
          "%s: the vectors follow the parts", e.name);
    for (int i = 0; i < w.vectors; ++i) {
        begin[n] = solver_work_vec(w, i);
        end[n++] = solver_work_vec(w, i + 1);
        CHECK(end[n - 1] - begin[n - 1] == 8 * w.rows[i] * k,
              "%s: vector %d of %lld rows", e.name, i, (long long)w.rows[i]);
    }
    for (int r = 0; r < n; ++r) {
        CHECK(begin[r] % 8 == 0 && end[r] % 8 == 0, "%s: region %d aligned",
              e.name, r);
        CHECK(begin[r] <= end[r], "%s: region %d runs backwards", e.name, r);
        CHECK(begin[r] == (r ? end[r - 1] : 0),
              "%s: region %d starts at %lld, not where %d ends", e.name, r,
              (long long)begin[r], r - 1);
    }
    CHECK(end[n - 1] == total, "%s: the last region ends at %lld of %lld",
          e.name, (long long)end[n - 1], (long long)total);
    // a heap block of exactly the total: the first and last byte of each region
    unsigned char *block = (unsigned char *)std::malloc((size_t)total);
    CHECK(block != NULL, "%s: %lld bytes", e.name, (long long)total);
    if (!block)
        return;
    for (int r = 0; r < n; ++r)
        if (end[r] > begin[r]) {
            block[begin[r]] = (unsigned char)r;
            block[end[r] - 1] = (unsigned char)r;
        }
    for (int r = 0; r < n; ++r) // disjoint: no region wrote into another
        if (end[r] > begin[r])
            CHECK(block[begin[r]] == r && block[end[r] - 1] == r,
                  "%s: region %d was overwritten", e.name, r);
    std::free(block);
}

static void check_all(int64_t M, int64_t N, int k) {
    const int64_t vm = 8 * M * k, vn = 8 * N * k;
    if (M == N) {
        check_layout(cg_work((int)M, k, 0),
                     expect{"cg", 512, 2, 3, 512 + 2 * 65536 + 3 * 8 * M * k}, M,
                     N, k);
        check_layout(cg_work((int)M, k, 1),
                     expect{"pcg", 512, 3, 3, 512 + 3 * 65536 + 3 * 8 * M * k},
                     M, N, k);
        check_layout(
            cg_work((int)M, k, 2),
            expect{"pcg_trsv", 512, 3, 4, 512 + 3 * 65536 + 4 * 8 * M * k}, M, N,
            k);
        check_layout(
            bicgstab_work((int)M, k),
            expect{"bicgstab", 512, 2, 6, 512 + 2 * 65536 + 6 * 8 * M * k}, M, N,
            k);
        check_layout(
            minres_work((int)M, k),
            expect{"minres", 2048, 3, 6, 2048 + 3 * 65536 + 6 * 8 * M * k}, M, N,
            k);
    }
    const solver_work ls = cgls_work((int)M, (int)N, k);
    check_layout(ls,
                 expect{"cgls", 512, 3, 4,
                        512 + 3 * 65536 + 8 * (int64_t)k * (2 * M + 2 * N)},
                 M, N, k);
    // R, Q of M rows, then S, P of N rows
    CHECK(solver_work_vec(ls, 1) - solver_work_vec(ls, 0) == vm &&
              solver_work_vec(ls, 2) - solver_work_vec(ls, 1) == vm &&
              solver_work_vec(ls, 3) - solver_work_vec(ls, 2) == vn &&
              solver_work_vec(ls, 4) - solver_work_vec(ls, 3) == vn,
          "cgls M %lld N %lld k %d: two lengths", (long long)M, (long long)N, k);
}

static void check_largest(void) {
    const int big = INT32_MAX, k = 8;
    const int64_t v = 8 * (int64_t)INT32_MAX * 8; // one vector: 2^37 - 64
    CHECK(v == 137438953408LL, "a vector of 2^31 - 1 rows");
    CHECK(solver_work_bytes(cg_work(big, k, 0)) == 512 + 2 * PART + 3 * v, "cg");
    CHECK(solver_work_bytes(cg_work(big, k, 1)) == 512 + 3 * PART + 3 * v,
          "pcg");
    CHECK(solver_work_bytes(cg_work(big, k, 2)) == 512 + 3 * PART + 4 * v,
          "pcg_trsv");
    CHECK(solver_work_bytes(bicgstab_work(big, k)) == 512 + 2 * PART + 6 * v &&
              512 + 2 * PART + 6 * v == 824633852032LL,
          "bicgstab");
    CHECK(solver_work_bytes(cgls_work(big, big, k)) == 512 + 3 * PART + 4 * v,
          "cgls");
    CHECK(solver_work_bytes(minres_work(big, k)) == 2048 + 3 * PART + 6 * v,
          "minres");
    // the last vector of the largest buffer starts where five end
    const solver_work w = minres_work(big, k);
    CHECK(solver_work_vec(w, 5) == 2048 + 3 * PART + 5 * v, "last vector");
}

static void check_refusals(void) {
    for (int k : {0, 9, -1}) {
        CHECK(solver_work_bytes(cg_work(10, k, 0)) == -EINVAL, "cg k %d", k);
        CHECK(solver_work_bytes(cg_work(10, k, 1)) == -EINVAL, "pcg k %d", k);
        CHECK(solver_work_bytes(cg_work(10, k, 2)) == -EINVAL, "pcgt k %d", k);
        CHECK(solver_work_bytes(bicgstab_work(10, k)) == -EINVAL, "bi k %d", k);
        CHECK(solver_work_bytes(cgls_work(10, 7, k)) == -EINVAL, "ls k %d", k);
        CHECK(solver_work_bytes(minres_work(10, k)) == -EINVAL, "mr k %d", k);
    }
    for (int pre = 0; pre < 3; ++pre)
        CHECK(solver_work_bytes(cg_work(-1, 1, pre)) == -EINVAL, "cg M < 0");
    CHECK(solver_work_bytes(bicgstab_work(-1, 1)) == -EINVAL, "bi M < 0");
    CHECK(solver_work_bytes(minres_work(-5, 8)) == -EINVAL, "mr M < 0");
    CHECK(solver_work_bytes(cgls_work(-1, 4, 1)) == -EINVAL, "ls M < 0");
    CHECK(solver_work_bytes(cgls_work(4, -1, 1)) == -EINVAL, "ls N < 0");
    CHECK(solver_work_bytes(cgls_work(0, 0, 1)) == 512 + 3 * PART, "ls empty");
}

int main(void) {
    const int64_t sizes[] = {0, 1, 255, 256, 257, 1000};
    for (int k = 1; k <= 8; ++k)
        for (int64_t M : sizes)
            for (int64_t N : sizes)
                check_all(M, N, k);
    check_largest();
    check_refusals();
    if (failures) {
        std::printf("%d checks FAILED\n", failures);
        return 1;
    }
    std::printf("%d layouts hold: aligned, in order, disjoint, ending at the "
                "stated size\n", layouts);
    return 0;
}
