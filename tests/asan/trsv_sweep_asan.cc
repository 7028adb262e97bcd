/*
 * The route of a sweep plan (trsv_plan.h: trsv_sweep_route,
 * trsv_sweep_scratch) as a stand-alone host program under AddressSanitizer +
 * UBSan: for sweeps 1..6 and 4096, in place and not, no sweep reads the buffer
 * it writes, B is never written before the last sweep, and the scratch count
 * is min(sweeps - 1, 2); then the sweeps themselves, restated over heap blocks
 * of exactly the scratch sizes on a small triangle, against forward
 * substitution once sweeps >= levels.
 */
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "trsv_plan.h"

static int failures = 0;
#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c);         \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

/* the strict lower triangle of a small matrix: row i depends on i - 1 (i % 4
 * != 0) and on i - 4; 3 x 4 -> levels up to 6 */
struct triangle {
    int M;
    std::vector<int> rowptr, ja;
    std::vector<double> as, diag;
};

static triangle make_triangle(int M) {
    triangle t;
    t.M = M;
    t.rowptr.push_back(0);
    for (int i = 0; i < M; ++i) {
        if (i % 4) {
            t.ja.push_back(i - 1);
            t.as.push_back(-1.0 - 0.125 * (i % 3));
        }
        if (i >= 4) {
            t.ja.push_back(i - 4);
            t.as.push_back(-0.5 - 0.0625 * (i % 5));
        }
        t.rowptr.push_back((int)t.ja.size());
        t.diag.push_back(4.0 + 0.25 * (i % 7));
    }
    return t;
}

/* row i of one sweep: TRSV_GROUP slots, the halving tree, rn(rhs - s), the
 * division; in == NULL is the first sweep (s = +0.0, the matrix is not read) */
static void sweep_row(const triangle &t, int i, int k, const double *B,
                      int64_t ldb, const double *in, int64_t ldin, double *out,
                      int64_t ldout) {
    for (int j = 0; j < k; ++j) {
        double slot[TRSV_GROUP];
        for (int g = 0; g < TRSV_GROUP; ++g)
            slot[g] = 0.0;
        if (in)
            for (int e = t.rowptr[i]; e < t.rowptr[i + 1]; ++e) {
                const int g = (e - t.rowptr[i]) % TRSV_GROUP;
                slot[g] = slot[g] + t.as[e] * in[(int64_t)t.ja[e] * ldin + j];
            }
        for (int h = TRSV_GROUP / 2; h >= 1; h /= 2)
            for (int g = 0; g < h; ++g)
                slot[g] = slot[g] + slot[g + h];
        const double rhs = B[(int64_t)i * ldb + j]; /* read before the store */
        out[(int64_t)i * ldout + j] = (rhs - slot[0]) / t.diag[i];
    }
}

/* one solve by the route; the scratch blocks are exactly kmax * M doubles and
 * are used with ld = k, as the launcher does */
static void solve(const triangle &t, int sweeps, int kmax, int k,
                  const double *B, int64_t ldb, double *X, int64_t ldx) {
    double *T[2] = {NULL, NULL};
    for (int b = 0; b < trsv_sweep_scratch(sweeps); ++b)
        T[b] = (double *)std::malloc(sizeof(double) * (size_t)kmax * t.M);
    double *const buf[3] = {X, T[0], T[1]};
    const int64_t ld[3] = {ldx, k, k};
    for (int m = 1; m <= sweeps; ++m) {
        const trsv_route r = trsv_sweep_route(sweeps, m);
        CHECK(r.out == TRSV_BUF_X || buf[r.out] != NULL);
        CHECK(r.in == TRSV_BUF_NONE || buf[r.in] != NULL);
        for (int i = 0; i < t.M; ++i)
            sweep_row(t, i, k, B, ldb,
                      r.in == TRSV_BUF_NONE ? NULL : buf[r.in],
                      r.in == TRSV_BUF_NONE ? 0 : ld[r.in], buf[r.out],
                      ld[r.out]);
    }
    std::free(T[0]);
    std::free(T[1]);
}

static void check_route(int sweeps, int *routes) {
    const int scratch = trsv_sweep_scratch(sweeps);
    CHECK(scratch == std::min(sweeps - 1, 2));
    bool used[3] = {false, false, false};
    int last_out = TRSV_BUF_NONE;
    for (int m = 1; m <= sweeps; ++m) {
        const trsv_route r = trsv_sweep_route(sweeps, m);
        CHECK(r.in != r.out);                         /* never its own input */
        CHECK(r.in == last_out);      /* what the launch before it wrote */
        CHECK((r.in == TRSV_BUF_NONE) == (m == 1));
        CHECK(r.in != TRSV_BUF_X);    /* X may be B: no sweep gathers from it */
        CHECK((r.out == TRSV_BUF_X) == (m == sweeps)); /* B lives until then */
        CHECK(r.out >= TRSV_BUF_X && r.out <= TRSV_BUF_T2);
        CHECK(r.out == TRSV_BUF_X || r.out <= scratch); /* a block it owns */
        used[r.out] = true;
        last_out = r.out;
        ++*routes;
    }
    CHECK(last_out == TRSV_BUF_X);
    CHECK((int)used[TRSV_BUF_T1] + (int)used[TRSV_BUF_T2] == scratch);
}

int main() {
    int routes = 0;
    const int counts[] = {1, 2, 3, 4, 5, 6, TRSV_MAX_SWEEPS};
    for (int sweeps : counts)
        check_route(sweeps, &routes);
    std::printf("%d routed sweeps hold\n", routes);

    const triangle t = make_triangle(12);
    const int M = t.M, kmax = 3;
    int solves = 0;
    for (int k = 1; k <= kmax; ++k) {
        const int64_t ldb = k + 1;
        std::vector<double> B((size_t)M * ldb);
        for (size_t i = 0; i < B.size(); ++i)
            B[i] = 0.5 + 0.03125 * (double)((i * 7) % 13);
        /* forward substitution with the same row function: every row reads
         * final values, gathered from the array it writes */
        std::vector<double> exact((size_t)M * k);
        for (int i = 0; i < M; ++i)
            sweep_row(t, i, k, B.data(), ldb, exact.data(), k, exact.data(), k);
        for (int sweeps = 1; sweeps <= 8; ++sweeps) {
            /* out of place, in a heap block of exactly M * k doubles */
            double *X = (double *)std::malloc(sizeof(double) * (size_t)M * k);
            solve(t, sweeps, kmax, k, B.data(), ldb, X, k);
            /* in place: X is B */
            std::vector<double> XB(B);
            solve(t, sweeps, kmax, k, XB.data(), ldb, XB.data(), ldb);
            for (int i = 0; i < M; ++i)
                for (int j = 0; j < k; ++j)
                    CHECK(std::memcmp(&XB[(size_t)i * ldb + j],
                                      &X[(size_t)i * k + j], 8) == 0);
            for (int i = 0; i < M; ++i) /* the padding column was not written */
                CHECK(XB[(size_t)i * ldb + k] == B[(size_t)i * ldb + k]);
            if (sweeps >= 6) /* the levels of this triangle */
                CHECK(std::memcmp(X, exact.data(), sizeof(double) * M * k) == 0);
            else
                CHECK(std::memcmp(X, exact.data(), sizeof(double) * M * k) != 0);
            std::free(X);
            solves += 2;
        }
    }
    std::printf("%d restated solves hold\n", solves);
    if (failures)
        std::printf("FAILED %d checks\n", failures);
    return failures ? 1 : 0;
}
