// CPU test of the work buffer of spmv_*_bicgstab_trsv
// (spmv_scpa_amd/csrc/solver_work.h, bicgstab_trsv_work) under ASan + UBSan.
//
// For k = 1..8 and M in {0, 1, 255, 256, 257, 1000}:
// 1. the state block, the two sets of partial sums and the SEVEN vectors (R,
//    Rh, P, V, T, Zp, Zs) are 8-byte aligned, in order and disjoint, and the
//    last one ends exactly at solver_work_bytes;
// 2. the total is the closed formula of the header, written out here, and
//    bicgstab_work next to it keeps its six vectors and its size to the byte;
// 3. over a heap block of exactly the total, the first and the last byte of
//    every region are written: a region past the end is an ASan report.
// Then the total at M = 2^31 - 1, k = 8 (no allocation) and the refusals.
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
static const int64_t STATE = 512;
static const int VECTORS = 7;

static int layouts;

static void check_layout(int64_t M, int k) {
    ++layouts;
    const solver_work w = bicgstab_trsv_work((int)M, k);
    const int64_t total = solver_work_bytes(w);
    const int64_t want = STATE + 2 * PART + VECTORS * 8 * M * k;
    CHECK(total == want, "M %lld k %d: %lld bytes, not %lld", (long long)M, k,
          (long long)total, (long long)want);
    CHECK(w.k == k && w.state_bytes == STATE && w.parts == 2 &&
              w.vectors == VECTORS && VECTORS <= SOLVER_WORK_MAXV,
          "state %lld, %d parts, %d vectors", (long long)w.state_bytes,
          w.parts, w.vectors);
    // bicgstab's own buffer: six vectors, one vector shorter
    const solver_work b = bicgstab_work((int)M, k);
    CHECK(b.vectors == 6 &&
              solver_work_bytes(b) == STATE + 2 * PART + 6 * 8 * M * k &&
              total - solver_work_bytes(b) == 8 * M * k,
          "bicgstab_work changed at M %lld k %d", (long long)M, k);
    if (total != want)
        return;
    // the regions in order: [begin, end)
    int64_t begin[1 + 2 + VECTORS], end[1 + 2 + VECTORS];
    int n = 0;
    begin[n] = 0;
    end[n++] = solver_work_part(w, 0);
    for (int i = 0; i < w.parts; ++i) {
        begin[n] = solver_work_part(w, i);
        end[n++] = solver_work_part(w, i + 1);
        CHECK(end[n - 1] - begin[n - 1] == PART, "part %d", i);
    }
    CHECK(solver_work_part(w, w.parts) == solver_work_vec(w, 0),
          "the vectors follow the parts");
    for (int i = 0; i < w.vectors; ++i) {
        begin[n] = solver_work_vec(w, i);
        end[n++] = solver_work_vec(w, i + 1);
        CHECK(w.rows[i] == M && end[n - 1] - begin[n - 1] == 8 * M * k,
              "vector %d of %lld rows", i, (long long)w.rows[i]);
    }
    CHECK(n == 1 + 2 + VECTORS, "%d regions", n);
    for (int r = 0; r < n; ++r) {
        CHECK(begin[r] % 8 == 0 && end[r] % 8 == 0, "region %d aligned", r);
        CHECK(begin[r] <= end[r], "region %d runs backwards", r);
        CHECK(begin[r] == (r ? end[r - 1] : 0),
              "region %d starts at %lld, not where %d ends", r,
              (long long)begin[r], r - 1);
    }
    CHECK(end[n - 1] == total, "the last region ends at %lld of %lld",
          (long long)end[n - 1], (long long)total);
    // a heap block of exactly the total: the first and last byte of each region
    unsigned char *block = (unsigned char *)std::malloc((size_t)total);
    CHECK(block != NULL, "%lld bytes", (long long)total);
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
                  "region %d was overwritten", r);
    std::free(block);
}

int main(void) {
    const int64_t sizes[] = {0, 1, 255, 256, 257, 1000};
    for (int k = 1; k <= 8; ++k)
        for (int64_t M : sizes)
            check_layout(M, k);
    // the largest buffer: no allocation, the arithmetic alone
    const int64_t v = 8 * (int64_t)INT32_MAX * 8; // one vector: 2^37 - 64
    const solver_work big = bicgstab_trsv_work(INT32_MAX, 8);
    CHECK(solver_work_bytes(big) == STATE + 2 * PART + 7 * v, "2^31 - 1 rows");
    CHECK(solver_work_vec(big, 6) == STATE + 2 * PART + 6 * v, "last vector");
    for (int k : {0, 9, -1})
        CHECK(solver_work_bytes(bicgstab_trsv_work(10, k)) == -EINVAL, "k %d",
              k);
    CHECK(solver_work_bytes(bicgstab_trsv_work(-1, 1)) == -EINVAL, "M < 0");
    if (failures) {
        std::printf("%d checks FAILED\n", failures);
        return 1;
    }
    std::printf("%d layouts hold: seven vectors, aligned, in order, disjoint, "
                "ending at the stated size\n", layouts);
    return 0;
}
