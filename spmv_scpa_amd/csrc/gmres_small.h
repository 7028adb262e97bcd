/*
 * gmres_small.h -- the per-column dense arithmetic of restarted GMRES
 * (gmres_kernels.hip; spmv_*_gmres): the rotated Hessenberg factor, the
 * rotations, g, and the back substitution, exactly as the result contract in
 * spmv_engine.h writes them.  One rounding per operation, no fused
 * multiply-add, correctly rounded divisions and square roots.
 *
 * Header-only and free of HIP: the finalising kernels call it for one column
 * per thread, and tests/asan/gmres_work_asan.cc runs the same text on the CPU
 * under AddressSanitizer + UBSan (compile with -ffp-contract=off where the
 * compiler does not know the clang pragma).
 *
 * The block of one column, m = restart, in doubles:
 *   r[m * m]   column l of the rotated factor at r[l * m + i], i <= l
 *   cs[m], sn[m]   the rotations
 *   g[m + 1]   the rotated right-hand side
 *   a[m + 1]   in: the sums of Gram-Schmidt pass 1
 *   c[m + 2]   in: the sums of pass 2;  gm_step makes h = a + c here and puts
 *              h_{p+1} behind it
 *   y[m]       the solution of the triangular system (gm_back)
 */
#ifndef SPMV_GMRES_SMALL_H
#define SPMV_GMRES_SMALL_H

#include <stddef.h>

#define GM_MAXM 64 /* restart, at most */

#if defined(__HIPCC__)
#define GM_HD __host__ __device__ static inline
#else
#define GM_HD static inline
#endif
#if defined(__clang__)
#define GM_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define GM_NO_CONTRACT
#endif

struct gm_col {
    double *r, *cs, *sn, *g, *a, *c, *y;
};

/* doubles of one column's block */
GM_HD size_t gm_col_doubles(int m) {
    return (size_t)m * m + 6 * (size_t)m + 4;
}

/* column j's block in a tail of 8 blocks */
GM_HD gm_col gm_col_at(double *tail, int m, int j) {
    double *b = tail + (size_t)j * gm_col_doubles(m);
    gm_col c;
    c.r = b;
    c.cs = c.r + (size_t)m * m;
    c.sn = c.cs + m;
    c.g = c.sn + m;
    c.a = c.g + (m + 1);
    c.c = c.a + (m + 1);
    c.y = c.c + (m + 2);
    return c;
}

GM_HD bool gm_finite(double v) {
    return __builtin_fabs(v) <= 1.7976931348623157e308; /* false for NaN */
}

/*
 * Position p of a cycle: a[0..p], c[0..p] hold the sums of the two passes, nn
 * is dot(W, W) behind them.  Returns 0 on a breakdown (nothing of the factor
 * or g is written: the step does not count), else 1 with column p of the
 * factor, rotation p, g[p], g[p + 1] written, *est = rn(g[p+1] * g[p+1]) and
 * *hn = h_{p+1}, the divisor of the next basis vector.
 */
GM_HD int gm_step(const gm_col &k, int m, int p, double nn, double *est,
                  double *hn) {
    GM_NO_CONTRACT
    double *h = k.c;
    bool ok = gm_finite(nn);
    for (int i = 0; i <= p; ++i) {
        h[i] = k.a[i] + k.c[i];
        ok = ok && gm_finite(h[i]);
    }
    h[p + 1] = __builtin_sqrt(nn);
    if (!ok)
        return 0;
    for (int i = 0; i < p; ++i) {
        const double ch = k.cs[i] * h[i];
        const double sh1 = k.sn[i] * h[i + 1];
        const double t = ch + sh1;
        const double ch1 = k.cs[i] * h[i + 1];
        const double sh = k.sn[i] * h[i];
        h[i + 1] = ch1 - sh;
        h[i] = t;
    }
    const double a = h[p], b = h[p + 1];
    const double aa = a * a;
    const double bb = b * b;
    const double d2 = aa + bb;
    const double d = __builtin_sqrt(d2);
    if (!gm_finite(d) || d == 0.0)
        return 0;
    const double c = a / d;
    const double s = b / d;
    const double ca = c * a;
    const double sb = s * b;
    for (int i = 0; i < p; ++i)
        k.r[(size_t)p * m + i] = h[i];
    k.r[(size_t)p * m + p] = ca + sb;
    k.cs[p] = c;
    k.sn[p] = s;
    const double sg = s * k.g[p];
    const double cg = c * k.g[p];
    k.g[p + 1] = -sg;
    k.g[p] = cg;
    *est = k.g[p + 1] * k.g[p + 1];
    *hn = b;
    return 1;
}

/* y[0..q) of the q counted steps, from i = q - 1 down: s = 0.0, then
 * s = rn(s + rn(r_il * y_l)) for l = i + 1 .. q - 1, and
 * y_i = rn(rn(g_i - s) / r_ii) */
GM_HD void gm_back(const gm_col &k, int m, int q) {
    GM_NO_CONTRACT
    for (int i = q - 1; i >= 0; --i) {
        double s = 0.0;
        for (int l = i + 1; l < q; ++l) {
            const double ry = k.r[(size_t)l * m + i] * k.y[l];
            s = s + ry;
        }
        const double t = k.g[i] - s;
        k.y[i] = t / k.r[(size_t)i * m + i];
    }
}

#endif /* SPMV_GMRES_SMALL_H */
