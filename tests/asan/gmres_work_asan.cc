// CPU test of the work buffer of spmv_*_gmres (spmv_scpa_amd/csrc/solver_work.h,
// gmres_work) and of the per-column dense arithmetic (gmres_small.h) under
// ASan + UBSan.
//
// For k = 1..8, restart in {1, 30, 64} and M in {0, 1, 255, 256, 257, 1000}:
// 1. the state (the head and the column blocks of gmres_small.h for 8
//    columns), the restart + 1 sets of partial sums, the basis as ONE vector of
//    (restart + 1) M rows, W and Z are 8-byte aligned, in order and disjoint,
//    and Z ends exactly at solver_work_bytes;
// 2. the total is base(restart) + (restart + 3) * 8 * k * M, base the same for
//    every k and M;
// 3. over a heap block of exactly the total, the first and the last byte of
//    every region and of every basis vector (element i * M * k) are written.
// Then the total at M = 2^31 - 1, k = 8, restart = 64 and the refusals.
//
// gmres_small.h: the seven arrays of the 8 column blocks tile the state behind
// its head; gm_step / gm_back over heap blocks of exactly gm_col_doubles(m)
// doubles, at m = 1, 5 and 64 with all m positions used, against a Givens QR
// and a back substitution written out here in long double; the breakdowns and
// the h_{p+1} == 0 rule.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <vector>

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
static const int64_t HEAD = 512;

static int64_t state_of(int m) {
    return HEAD + 8 * 8 * ((int64_t)m * m + 6 * m + 4);
}

static int layouts;

static void check_layout(int64_t M, int k, int m) {
    ++layouts;
    const solver_work w = gmres_work((int)M, k, m);
    const int64_t total = solver_work_bytes(w);
    const int64_t base = state_of(m) + (m + 1) * PART;
    const int64_t want = base + (int64_t)(m + 3) * 8 * M * k;
    CHECK(total == want, "M %lld k %d m %d: %lld bytes, not %lld", (long long)M,
          k, m, (long long)total, (long long)want);
    CHECK(solver_work_bytes(gmres_work(0, k, m)) == base, "base of k %d", k);
    CHECK(w.k == k && w.state_bytes == state_of(m) && w.parts == m + 1 &&
              w.vectors == 3 && w.vectors <= SOLVER_WORK_MAXV,
          "state %lld, %d parts, %d vectors", (long long)w.state_bytes,
          w.parts, w.vectors);
    CHECK(w.rows[0] == (int64_t)(m + 1) * M && w.rows[1] == M && w.rows[2] == M,
          "rows %lld %lld %lld", (long long)w.rows[0], (long long)w.rows[1],
          (long long)w.rows[2]);
    if (total != want)
        return;
    std::vector<int64_t> begin, end;
    begin.push_back(0);
    end.push_back(solver_work_part(w, 0));
    for (int i = 0; i < w.parts; ++i) {
        begin.push_back(solver_work_part(w, i));
        end.push_back(solver_work_part(w, i + 1));
        CHECK(end.back() - begin.back() == PART, "part %d", i);
    }
    CHECK(solver_work_part(w, w.parts) == solver_work_vec(w, 0),
          "the vectors follow the parts");
    // the basis vectors, each where the kernels look for it
    for (int i = 0; i <= m; ++i) {
        begin.push_back(solver_work_vec(w, 0) + 8 * (int64_t)((size_t)i * M * k));
        end.push_back(begin.back() + 8 * M * k);
    }
    CHECK(end.back() == solver_work_vec(w, 1), "W follows the basis");
    for (int i = 1; i < 3; ++i) {
        begin.push_back(solver_work_vec(w, i));
        end.push_back(solver_work_vec(w, i + 1));
        CHECK(end.back() - begin.back() == 8 * M * k, "vector %d", i);
    }
    const int n = (int)begin.size();
    for (int r = 0; r < n; ++r) {
        CHECK(begin[r] % 8 == 0 && end[r] % 8 == 0, "region %d aligned", r);
        CHECK(begin[r] <= end[r], "region %d runs backwards", r);
        CHECK(begin[r] == (r ? end[r - 1] : 0), "region %d starts at %lld", r,
              (long long)begin[r]);
    }
    CHECK(end[n - 1] == total, "the last region ends at %lld of %lld",
          (long long)end[n - 1], (long long)total);
    unsigned char *block = (unsigned char *)std::malloc((size_t)total);
    CHECK(block != NULL, "%lld bytes", (long long)total);
    if (!block)
        return;
    for (int r = 0; r < n; ++r)
        if (end[r] > begin[r]) {
            block[begin[r]] = (unsigned char)r;
            block[end[r] - 1] = (unsigned char)r;
        }
    for (int r = 0; r < n; ++r)
        if (end[r] > begin[r])
            CHECK(block[begin[r]] == (unsigned char)r &&
                      block[end[r] - 1] == (unsigned char)r,
                  "region %d was overwritten", r);
    // the column blocks tile the state behind its head
    double *tail = (double *)(block + HEAD);
    const double *at = tail;
    for (int j = 0; j < 8; ++j) {
        const gm_col c = gm_col_at(tail, m, j);
        CHECK(c.r == at && c.cs == c.r + m * m && c.sn == c.cs + m &&
                  c.g == c.sn + m && c.a == c.g + m + 1 &&
                  c.c == c.a + m + 1 && c.y == c.c + m + 2,
              "column %d", j);
        at = c.y + m;
    }
    CHECK((const unsigned char *)at == block + w.state_bytes,
          "the column blocks end with the state");
    std::free(block);
}

// ---- gmres_small.h against a long double Givens QR ----

static double hval(int i, int l) { // entry (i, l) of an upper Hessenberg H
    return i == l ? 3.0 + 0.25 * l : i == l + 1 ? 0.5 + 0.125 * l
                                                : 1.0 / (1 + i + 2 * l);
}

static int columns;

static void check_small(int m) {
    // one block of exactly gm_col_doubles(m) doubles on the heap
    double *blk = (double *)std::malloc(gm_col_doubles(m) * sizeof(double));
    for (size_t i = 0; i < gm_col_doubles(m); ++i)
        blk[i] = NAN;
    const gm_col c = gm_col_at(blk, m, 0);
    const double beta = 1.75;
    c.g[0] = beta;
    // the reference: rotated factor R, g, in long double
    std::vector<long double> R((size_t)m * m, 0.0L), cs(m), sn(m), g(m + 1);
    g[0] = beta;
    double prev = beta * beta;
    for (int p = 0; p < m; ++p) {
        ++columns;
        // the sums as two passes would give them: a the bulk, c a correction
        for (int i = 0; i <= p; ++i) {
            c.a[i] = hval(i, p);
            c.c[i] = std::ldexp(hval(i, p), -40);
        }
        const double hn = hval(p + 1, p);
        double est = -1.0, div = -1.0;
        const int ok = gm_step(c, m, p, hn * hn, &est, &div);
        CHECK(ok == 1, "m %d step %d broke down", m, p);
        std::vector<long double> h(p + 2);
        for (int i = 0; i <= p; ++i)
            h[i] = (long double)c.a[i] + std::ldexp((long double)hval(i, p), -40);
        h[p + 1] = std::sqrt((long double)(hn * hn));
        for (int i = 0; i < p; ++i) {
            const long double t = cs[i] * h[i] + sn[i] * h[i + 1];
            h[i + 1] = cs[i] * h[i + 1] - sn[i] * h[i];
            h[i] = t;
        }
        const long double d = std::sqrt(h[p] * h[p] + h[p + 1] * h[p + 1]);
        cs[p] = h[p] / d;
        sn[p] = h[p + 1] / d;
        for (int i = 0; i < p; ++i)
            R[(size_t)p * m + i] = h[i];
        R[(size_t)p * m + p] = d;
        g[p + 1] = -sn[p] * g[p];
        g[p] = cs[p] * g[p];
        // p + 2 roundings of size 2^-53 at the most on each path, and slack
        const double tol = 1e-15 * (p + 2) * 8;
        for (int i = 0; i <= p; ++i) {
            const double want = (double)R[(size_t)p * m + i];
            CHECK(std::fabs(c.r[(size_t)p * m + i] - want) <=
                      tol * (1.0 + std::fabs(want)), "m %d r(%d,%d)", m, i, p);
        }
        CHECK(std::fabs(c.cs[p] - (double)cs[p]) <= tol &&
                  std::fabs(c.sn[p] - (double)sn[p]) <= tol, "rotation %d", p);
        CHECK(std::fabs(c.g[p] - (double)g[p]) <= tol * beta &&
                  std::fabs(c.g[p + 1] - (double)g[p + 1]) <= tol * beta,
              "g at step %d", p);
        CHECK(est == c.g[p + 1] * c.g[p + 1] && est <= prev,
              "est %g after %g at step %d", est, prev, p);
        CHECK(div == hn, "the divisor of step %d", p);
        prev = est;
    }
    // y of q = m and of q = (m + 1) / 2 steps
    for (int q : {m, (m + 1) / 2}) {
        gm_back(c, m, q);
        std::vector<long double> y(q);
        for (int i = q - 1; i >= 0; --i) {
            long double s = 0.0L;
            for (int l = i + 1; l < q; ++l)
                s += R[(size_t)l * m + i] * y[l];
            y[i] = (g[i] - s) / R[(size_t)i * m + i];
        }
        for (int i = 0; i < q; ++i)
            CHECK(std::fabs(c.y[i] - (double)y[i]) <=
                      1e-12 * (1.0 + std::fabs((double)y[i])),
                  "m %d q %d y[%d] = %g, not %g", m, q, i, c.y[i], (double)y[i]);
    }
    std::free(blk);
}

static void check_rules(void) {
    const int m = 3;
    double *blk = (double *)std::calloc(gm_col_doubles(m), sizeof(double));
    const gm_col c = gm_col_at(blk, m, 0);
    double est = -1.0, div = -1.0;
    c.g[0] = 2.0;
    // a non-finite sum, a non-finite nn, d == 0: no step, nothing written
    c.a[0] = INFINITY;
    c.c[0] = 0.0;
    CHECK(gm_step(c, m, 0, 1.0, &est, &div) == 0, "inf in h");
    c.a[0] = 1.0;
    CHECK(gm_step(c, m, 0, NAN, &est, &div) == 0, "nan in nn");
    c.a[0] = 0.0;
    c.c[0] = 0.0;
    CHECK(gm_step(c, m, 0, 0.0, &est, &div) == 0, "d == 0");
    c.a[0] = 1e200;
    c.c[0] = 0.0;
    CHECK(gm_step(c, m, 0, 1.0, &est, &div) == 0, "d overflows");
    CHECK(c.g[0] == 2.0 && c.g[1] == 0.0 && c.r[0] == 0.0 && est == -1.0,
          "a breakdown wrote something");
    // h_{p+1} == 0 with a != 0: s = 0, est = 0 by arithmetic
    c.a[0] = 4.0;
    c.c[0] = 0.0;
    CHECK(gm_step(c, m, 0, 0.0, &est, &div) == 1 && est == 0.0 && div == 0.0 &&
              c.sn[0] == 0.0 && c.cs[0] == 1.0 && c.r[0] == 4.0 &&
              c.g[0] == 2.0,
          "h_{p+1} == 0");
    gm_back(c, m, 1);
    CHECK(c.y[0] == 0.5, "y of the one step: %g", c.y[0]);
    gm_back(c, m, 0); // nothing to do, nothing touched
    std::free(blk);
}

int main(void) {
    const int64_t sizes[] = {0, 1, 255, 256, 257, 1000};
    for (int k = 1; k <= 8; ++k)
        for (int m : {1, 30, 64})
            for (int64_t M : sizes)
                check_layout(M, k, m);
    // the largest buffer: no allocation, the arithmetic alone
    const solver_work big = gmres_work(INT32_MAX, 8, GM_MAXM);
    const int64_t v = 8 * (int64_t)INT32_MAX * 8;
    CHECK(solver_work_bytes(big) == state_of(64) + 65 * PART + 67 * v,
          "2^31 - 1 rows");
    CHECK(solver_work_vec(big, 2) == state_of(64) + 65 * PART + 66 * v, "Z");
    for (int k : {0, 9, -1})
        CHECK(solver_work_bytes(gmres_work(10, k, 30)) == -EINVAL, "k %d", k);
    for (int m : {0, -1, 65})
        CHECK(solver_work_bytes(gmres_work(10, 1, m)) == -EINVAL, "m %d", m);
    CHECK(solver_work_bytes(gmres_work(-1, 1, 30)) == -EINVAL, "M < 0");
    for (int m : {1, 5, 64})
        check_small(m);
    check_rules();
    if (failures) {
        std::printf("%d checks FAILED\n", failures);
        return 1;
    }
    std::printf("%d layouts hold: the state, the parts, the basis, W and Z, "
                "aligned, in order, disjoint, ending at the stated size\n",
                layouts);
    std::printf("%d Hessenberg columns match the long double rotations\n",
                columns);
    return 0;
}
