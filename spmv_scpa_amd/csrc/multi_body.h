/*
 * multi_body.h -- the four kernels of multi_kernels.hip, written ONCE and
 * included TWICE by that file (and by nothing else; no include guard):
 *   MULTI_AXPBY 0   k_csr_multi, k_csr_multi_long, k_hll_multi,
 *                   k_hll_multi_wide:  Y = A X  (spmv_*_launch_multi)
 *   MULTI_AXPBY 1   k_csr_axpby, k_csr_axpby_long, k_hll_axpby,
 *                   k_hll_axpby_wide:  Y = alpha A X + beta Y, two more kernel
 *                   arguments and the epilogue axpby_of() where the store is
 *                   (spmv_*_launch_axpby)
 * Everything outside an `#if MULTI_AXPBY` block is common to both, so the sum
 * the epilogue is applied to is the sum the plain kernel stores.  The
 * preprocessor and not a template switch or a shared __device__ body, because
 * this is the form that leaves the 128 plain kernels what they were to the
 * byte: the MULTI_AXPBY 0 pass is, token for token, the
 * kernels as they stood before the epilogue existed.
 *
 * y_old is loaded only when beta != 0 (a uniform branch: beta == 0 never
 * reads Y).  k_csr_axpby issues the loads FIRST, ahead of every other load: a
 * wavefront of it lives for three dependent memory round trips, and y_old
 * behind the last gather was a fourth (measured).  The
 * other three walk many entries per lane and load y_old after the walk, where
 * it costs no register through it: k_hll_axpby just before the store, the
 * side kernels ahead of their reduction.
 */
#if MULTI_AXPBY
#define MULTI_KERNEL(plain, axpby) axpby
#define MULTI_EP_PARAMS , double alpha, double beta
#else
#define MULTI_KERNEL(plain, axpby) plain
#define MULTI_EP_PARAMS
#endif

/* ------------------------------------------------------------------ */
/* CSR: G lanes per row, P rows per lane group, K accumulators per row  */
/* ------------------------------------------------------------------ */
template <int G, int P, int K, typename V>
__global__ void MULTI_KERNEL(k_csr_multi, k_csr_axpby)(
                            int M, int order, const int *__restrict__ irp,
                            const int *__restrict__ ja,
                            const V *__restrict__ as,
                            const double *__restrict__ X, int64_t ldx,
                            double *__restrict__ Y, int64_t ldy
                            MULTI_EP_PARAMS) {
    constexpr int RPP = WAVE / G; /* rows per pass */
    const int lane = threadIdx.x & (WAVE - 1);
    const int sub = lane & (G - 1);
    /* order 0: hardware, 1: XCD-contiguous equal ranges, 2: grouped (grid
     * padded to a multiple of NUM_XCD x XCD_GROUP; rows beyond M are masked) */
    const long long bid = order == 1 ? xcd_remap(blockIdx.x, gridDim.x)
                          : order == 2 ? xcd_grouped<long long>(blockIdx.x)
                                       : (long long)blockIdx.x;
    const long long wave_global = (bid * blockDim.x + threadIdx.x) / WAVE;
    const long long rbase = wave_global * (P * RPP) + lane / G;
#if MULTI_AXPBY
    /* y_old FIRST: its address needs no IRP, and behind the gathers it would
     * be a fourth dependent round trip of a wavefront that lives for three.
     * Lane `sub` of a row's G lanes holds elements sub, sub + G, ... of the
     * row (YS values per pass instead of K in every lane); lane 0 collects
     * them with DPP moves where it stores (lane_yold) */
    constexpr int YS = (K + G - 1) / G;
    const bool reads_y = beta != 0.0;
    double yo[P][YS];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const long long row = rbase + p * RPP;
        const double *yr = Y + row * ldy;
        const bool ld = reads_y && row < M;
#pragma unroll
        for (int s = 0; s < YS; ++s)
            yo[p][s] = ld && sub + s * G < K ? ld_stream(yr + sub + s * G) : 0.0;
    }
#endif

    int beg[P], end[P];
    bool mine[P]; /* this kernel writes the row (inside M, not a long row) */
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const long long row = rbase + p * RPP;
        const bool live = row < M;
        beg[p] = live ? irp[row] : 0;
        end[p] = live ? irp[row + 1] : 0;
        mine[p] = live;
        if (end[p] - beg[p] > STREAM_NNZ) { /* k_csr_multi_long's row */
            end[p] = beg[p];
            mine[p] = false;
        }
    }
    int c[P];
    V a[P];
    double acc[P][K];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        /* offsets relative to the row's first entry: beg + sub (+ G below)
         * must not be formed in 32 bits next to INT32_MAX */
        const bool has = sub < end[p] - beg[p];
        c[p] = has ? ld_stream(ja + beg[p] + sub) : -1;
        a[p] = has ? ld_stream(as + beg[p] + sub) : V(0);
    }
    /* the gathers of all P passes are issued before the first product waits */
#pragma unroll
    for (int p = 0; p < P; ++p) {
#pragma unroll
        for (int j = 0; j < K; ++j)
            acc[p][j] = 0.0;
        if (c[p] >= 0)
            load_xrow<K>(X, ldx, c[p], acc[p]);
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const double av = widen(a[p]);
#pragma unroll
        for (int j = 0; j < K; ++j) /* the lane's first product: a multiply */
            acc[p][j] = c[p] >= 0 ? av * acc[p][j] : 0.0;
    }
#pragma unroll
    for (int p = 0; p < P; ++p)
        for (int k = sub + G, n = end[p] - beg[p]; k < n; k += G) {
            double xv[K];
            const double av = widen(ld_stream(as + beg[p] + k));
            load_xrow<K>(X, ldx, ld_stream(ja + beg[p] + k), xv);
#pragma unroll
            for (int j = 0; j < K; ++j)
                acc[p][j] += av * xv[j];
        }
#pragma unroll
    for (int p = 0; p < P; ++p) {
#pragma unroll
        for (int j = 0; j < K; ++j)
            acc[p][j] = group_sum<G>(acc[p][j]);
#if MULTI_AXPBY
        double yj[K]; /* every lane takes part in the moves */
        lane_yold<G, K, YS>(yo[p], yj);
#endif
        const long long row = rbase + p * RPP;
        if (sub == 0 && mine[p]) {
            double *yr = Y + row * ldy;
#if MULTI_AXPBY
            /* a select, not a branch: the branch was measured slower here
             * (K = 8: 1.31 against 1.11 x launch_multi at beta == 0) */
#pragma unroll
            for (int j = 0; j < K; ++j)
                acc[p][j] = reads_y ? axpby_of(alpha, acc[p][j], beta, yj[j])
                                    : scaled_of(alpha, acc[p][j]);
#endif
#pragma unroll
            for (int j = 0; j < K; ++j)
                __builtin_nontemporal_store(acc[p][j], yr + j);
        }
    }
}

/*
 * The rows of more than STREAM_NNZ entries: workgroup g takes range
 * long_rb[g] of the stream table and, when that is the FIRST range of its
 * row (a row beyond STREAM_LONG_ROW entries owns several), sums the whole
 * row: thread t adds entries t, t + 256, ... in order (four in flight), a
 * wavefront tree, then the four wavefronts' partial sums in wavefront order.
 */
template <int K, typename V>
__global__ void __launch_bounds__(MULTI_LONG_THREADS)
    MULTI_KERNEL(k_csr_multi_long, k_csr_axpby_long)(
                     const int *__restrict__ long_rb,
                     const int2 *__restrict__ rowblk,
                     const int *__restrict__ irp, const int *__restrict__ ja,
                     const V *__restrict__ as, const double *__restrict__ X,
                     int64_t ldx, double *__restrict__ Y, int64_t ldy
                     MULTI_EP_PARAMS) {
    constexpr int NT = MULTI_LONG_THREADS, U = 4;
    __shared__ double part[NT / WAVE][K];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int rb = long_rb[blockIdx.x];
    const int row = rowblk[rb].x;
    const int beg = irp[row];
    if (rowblk[rb].y != beg)
        return; /* a later segment of the same row: workgroup-uniform */
    const int n = irp[row + 1] - beg;
    ja += beg;
    as += beg;
    double acc[K];
#pragma unroll
    for (int j = 0; j < K; ++j)
        acc[j] = 0.0;
    /* 64-bit: a row may hold close to INT32_MAX entries, k + u * NT more */
    for (int64_t k = tid; k < n; k += U * NT) {
        int c[U];
        V v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool on = k + u * NT < n;
            c[u] = on ? ld_stream(ja + k + u * NT) : -1;
            v[u] = on ? ld_stream(as + k + u * NT) : V(0);
        }
        double xv[U][K];
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (c[u] >= 0)
                load_xrow<K>(X, ldx, c[u], xv[u]);
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (c[u] >= 0) {
                const double av = widen(v[u]);
#pragma unroll
                for (int j = 0; j < K; ++j)
                    acc[j] += av * xv[u][j];
            }
    }
#if MULTI_AXPBY
    /* thread j < K stores Y[row][j]: its y_old is in flight over the trees
     * and the barrier */
    const bool reads_y = beta != 0.0;
    double yo = 0.0;
    if (reads_y && tid < K)
        yo = ld_stream(Y + (int64_t)row * ldy + tid);
#endif
#pragma unroll
    for (int j = 0; j < K; ++j) {
        acc[j] = group_sum<WAVE>(acc[j]);
        if (lane == 0)
            part[tid / WAVE][j] = acc[j];
    }
    __syncthreads();
    if (tid < K) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < NT / WAVE; ++w)
            t += part[w][tid];
#if MULTI_AXPBY
        t = reads_y ? axpby_of(alpha, t, beta, yo) : scaled_of(alpha, t);
#endif
        Y[(int64_t)row * ldy + tid] = t;
    }
}

/* ------------------------------------------------------------------ */
/* HLL, column-major: lane per row, U columns in flight, K accumulators */
/* ------------------------------------------------------------------ */
template <int K, int U, typename V>
__global__ void MULTI_KERNEL(k_hll_multi, k_hll_axpby)(
                            int M, int nb, int order,
                            const int64_t *__restrict__ off,
                            const int *__restrict__ ja,
                            const V *__restrict__ as,
                            const double *__restrict__ X, int64_t ldx,
                            double *__restrict__ Y, int64_t ldy
                            MULTI_EP_PARAMS) {
    /* order 2: groups of XCD_GROUP workgroups per XCD; else hardware */
    const long long wg = order == 2 ? xcd_grouped<long long>(blockIdx.x)
                                    : (long long)blockIdx.x;
    const long long t = wg * blockDim.x + threadIdx.x;
    if (t / HACK >= nb)
        return;
    const int b = (int)(t / HACK), i = (int)(t % HACK);
    const int rows = min(HACK, M - b * HACK);
    if (i >= rows)
        return;
    const int64_t o = off[b];
    const int w = hack_block_width(off, b, rows);
    if (w > HLL_WIDE)
        return; /* k_hll_multi_wide's block */
    const int *cj = ja + o + i;
    const V *ca = as + o + i;
    double acc[K];
#pragma unroll
    for (int j = 0; j < K; ++j)
        acc[j] = 0.0;
    int cJ[U];
    V cA[U];
    const int nfull = w / U;
    if (nfull > 0) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            cJ[u] = ld_stream(cj + u * rows);
            cA[u] = ld_stream(ca + u * rows);
        }
    }
    for (int c = 0; c < nfull; ++c) {
        double xv[U][K];
        V av[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            load_xrow<K>(X, ldx, cJ[u], xv[u]);
            av[u] = cA[u];
        }
        if (c + 1 < nfull) { /* the next columns' stream behind the gathers */
            const int *nj = cj + (size_t)(c + 1) * U * rows;
            const V *na = ca + (size_t)(c + 1) * U * rows;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                cJ[u] = ld_stream(nj + u * rows);
                cA[u] = ld_stream(na + u * rows);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const double a = widen(av[u]);
#pragma unroll
            for (int j = 0; j < K; ++j)
                acc[j] += a * xv[u][j];
        }
    }
    for (int jc = nfull * U; jc < w; ++jc) {
        double xv[K];
        const double a = widen(ld_stream(ca + (size_t)jc * rows));
        load_xrow<K>(X, ldx, ld_stream(cj + (size_t)jc * rows), xv);
#pragma unroll
        for (int j = 0; j < K; ++j)
            acc[j] += a * xv[j];
    }
    double *yr = Y + ((int64_t)b * HACK + i) * ldy;
#if MULTI_AXPBY
    /* the row's y_old after the walk: it costs no register through it, and
     * loading it first was measured no faster */
    if (beta != 0.0) {
        double yo[K];
#pragma unroll
        for (int j = 0; j < K; ++j)
            yo[j] = ld_stream(yr + j);
#pragma unroll
        for (int j = 0; j < K; ++j)
            acc[j] = axpby_of(alpha, acc[j], beta, yo[j]);
    } else {
#pragma unroll
        for (int j = 0; j < K; ++j)
            acc[j] = scaled_of(alpha, acc[j]);
    }
#endif
#pragma unroll
    for (int j = 0; j < K; ++j)
        __builtin_nontemporal_store(acc[j], yr + j);
}

/*
 * The hack blocks of more than HLL_WIDE columns: workgroup g looks at segment
 * g of the handle's segment table and, when that is the FIRST segment of its
 * block, sums the whole block: thread (row i, column lane cl) adds columns
 * cl, cl + 8, ... in order, then the eight column lanes of a row are added in
 * lane order out of LDS.
 */
template <int K, int U, typename V>
__global__ void __launch_bounds__(256)
    MULTI_KERNEL(k_hll_multi_wide, k_hll_axpby_wide)(
                     int M, const int4 *__restrict__ seg,
                     const int64_t *__restrict__ off,
                     const int *__restrict__ ja, const V *__restrict__ as,
                     const double *__restrict__ X, int64_t ldx,
                     double *__restrict__ Y, int64_t ldy MULTI_EP_PARAMS) {
    __shared__ double red[8][K][HACK];
    const int tid = threadIdx.x;
    const int4 sg = seg[blockIdx.x];
    if (sg.z != 0)
        return; /* not the block's first segment: workgroup-uniform */
    const int b = sg.x;
    const int rows = min(HACK, M - b * HACK);
    const int64_t o = off[b];
    const int w = hack_block_width(off, b, rows);
    const int i = tid & 31, cl = tid >> 5;
    double acc[K];
#pragma unroll
    for (int j = 0; j < K; ++j)
        acc[j] = 0.0;
    if (i < rows) {
        const int64_t base = o + i;
        /* 64-bit column arithmetic: w may sit next to INT32_MAX */
        for (int64_t jc = cl; jc < w; jc += 8 * U) {
            int c[U];
            V v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t col = jc + 8 * u;
                const bool on = col < w;
                c[u] = on ? ld_stream(ja + base + col * rows) : -1;
                v[u] = on ? ld_stream(as + base + col * rows) : V(0);
            }
            double xv[U][K];
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (c[u] >= 0)
                    load_xrow<K>(X, ldx, c[u], xv[u]);
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (c[u] >= 0) {
                    const double a = widen(v[u]);
#pragma unroll
                    for (int j = 0; j < K; ++j)
                        acc[j] += a * xv[u][j];
                }
        }
    }
#if MULTI_AXPBY
    /* thread (vector cl, row i) stores Y[row][cl]: its y_old is in flight over
     * the LDS reduction */
    const bool reads_y = beta != 0.0;
    double yo = 0.0;
    if (reads_y && cl < K && i < rows)
        yo = ld_stream(Y + ((int64_t)b * HACK + i) * ldy + cl);
#endif
#pragma unroll
    for (int j = 0; j < K; ++j)
        red[cl][j][i] = acc[j];
    __syncthreads();
    /* thread (vector j = tid / 32, row i): 32 * K <= 256 threads take part */
    if (cl < K && i < rows) {
        double t = 0.0;
#pragma unroll
        for (int c = 0; c < 8; ++c)
            t += red[c][cl][i];
#if MULTI_AXPBY
        t = reads_y ? axpby_of(alpha, t, beta, yo) : scaled_of(alpha, t);
#endif
        Y[((int64_t)b * HACK + i) * ldy + cl] = t;
    }
}

#undef MULTI_KERNEL
#undef MULTI_EP_PARAMS
