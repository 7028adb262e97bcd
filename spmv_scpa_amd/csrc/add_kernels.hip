/*
 * add_kernels.hip -- C = alpha A + beta B of two CSR handles on the device
 * (spmv_csr_add; spmv_engine.h), and its two companions: a handle made from
 * a device vector (spmv_csr_from_diag) and a two-sided diagonal scaling
 * (spmv_csr_scale).  gfx950 (wave64).
 *
 * The sum is defined to the byte (spmv_engine.h): row r of C holds the union
 * of the two rows' columns, once each, ascending; a column stored in A only
 * holds ta = rn(alpha a), one stored in B only tb = rn(beta b), one stored in
 * both rn(ta + tb) -- every operation rounded on its own (this file is
 * compiled with contraction off: no fused multiply-add).
 *
 * The geometry (size classes, widths, scratch) is add_plan.h's; the steps
 * every builder of a handle shares are csr_build.h's.  The launches, in order
 * -- the kernel boundary is the only ordering between workgroups, nothing
 * waits on another workgroup:
 *
 *   csr_check_rows_dev (A, B)
 *   k_add_bound    the rows beyond the class edge and the widest row, over
 *                  all rows (integer atomics, one pair a workgroup: a COUNT
 *                  and a MAXIMUM do not depend on the order of arrival)
 *   csr_lists_dev  the rows of each class (the length rule), listed -- only
 *                  when both classes hold rows
 *   k_add_count_*  len_A + len_B - matches per row (reads IRP and JA only)
 *   csr_total_dev, csr_alloc_scanned_dev      C's IRP
 *   k_add_rows_*   JA and AS of C
 *
 * Both row kernels are a merge of two ascending index lists BY RANK, searched
 * in place: a row is at most a few cache lines that the lanes of its team
 * have just touched, so the probes of the binary search hit the L1 (DESIGN.md
 * s.30 on LDS staging).  The entries of a row are numbered k = 0 .. len_A +
 * len_B - 1, A's first; a team walks them in chunks of its width.  Lane k
 * finds the rank p of its column in the OTHER row (lower bound) and whether
 * the column is stored there.  Entry i of A lands at
 *     i + p - (matched entries of A before i),
 * an unmatched entry j of B at
 *     j + p - (matched entries of B before j);
 * the two prefix counts agree because both rows ascend.  Inside a chunk the
 * prefix is a population count over a ballot, across chunks it is carried in
 * a register.  A matched pair is written by its A-side lane, which reads b at
 * the rank it found; the B-side lane writes nothing.  So every slot of C is
 * written exactly once, by one lane, from a computed position: no atomics.
 *
 * Every device loop is bounded by a row length or log2 of one.  A store is
 * guarded by the row's end in C's IRP (never taken for rows that passed the
 * check), so nothing is ever written out of bounds.
 */
#include <algorithm>
#include <string.h>

#include "add_plan.h"
#include "csr_build.h"

/* every product and every sum is rounded on its own */
#pragma clang fp contract(off)

#define AD_T ADD_THREADS
#define AD_WAVES (AD_T / WAVE)

static_assert(ADD_SCAN_TILE == TRANSPOSE_SCAN_TILE,
              "add_plan.h sizes the scan's sums for tr_scan");
static_assert(ADD_WIDTH_MAX <= 32, "a group's ballot bits fit 32 bits");

typedef unsigned long long ad_u64;

/* the 64-bit words of the head */
enum {
    AD_FLAGS = 0,  /* 1: a column outside [0, N), 2: a row not ascending */
    AD_WIDEST = 1, /* max of len_A + len_B */
    AD_ROWS = 2,   /* [2] rows per class; only [1] is counted */
    AD_CURSOR = 4, /* [2] next free place of each class's list */
    AD_NZ = 6      /* entries of C */
};
static_assert(AD_NZ < ADD_HEAD_WORDS, "the head holds every word");

/* first place of row[0 .. n) (ascending) that holds c or more: at most
 * log2(n) + 1 probes */
__device__ __forceinline__ int ad_lower_bound(const int *__restrict__ row,
                                              int n, int c) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (row[mid] < c)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

/* ------------------------------------------------------------------ */
/* bounds, the class of a row                                           */
/* ------------------------------------------------------------------ */

/* the workgroup's sum and maximum of v in thread 0 (all threads call) */
__device__ __forceinline__ void ad_block_sum_max(ad_u64 &sum, ad_u64 &most) {
    __shared__ ad_u64 part[2][AD_WAVES];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    most = wave_max(most);
    sum = wave_sum(sum);
    if (lane == 0) {
        part[0][wave] = sum;
        part[1][wave] = most;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < AD_WAVES; ++w) {
            sum += part[0][w];
            most = part[1][w] > most ? part[1][w] : most;
        }
}

/* class 0 serves len <= edge (the modes of spmv_add_set_class: an edge above
 * or below every length).  The rows beyond the edge are counted, the others
 * are the rest of M.  A grid-stride loop and ONE pair of atomics a workgroup:
 * an atomic a wavefront on one address was 3.6 ms for 10M rows */
__global__ void __launch_bounds__(AD_T)
k_add_bound(int M, const int *__restrict__ irp_a, const int *__restrict__ irp_b,
            int64_t edge, ad_u64 *__restrict__ head) {
    const int64_t first = (int64_t)blockIdx.x * AD_T + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * AD_T;
    ad_u64 wide = 0, most = 0;
    for (int64_t r = first; r < M; r += stride) {
        const int64_t len = ((int64_t)irp_a[r + 1] - irp_a[r]) +
                            ((int64_t)irp_b[r + 1] - irp_b[r]);
        wide += len > edge;
        most = (ad_u64)len > most ? (ad_u64)len : most;
    }
    ad_block_sum_max(wide, most);
    if (threadIdx.x == 0) {
        if (wide)
            atomicAdd(head + AD_ROWS + 1, wide);
        if (most)
            atomicMax(head + AD_WIDEST, most);
    }
}

/* the class of a row, for csr_lists_dev */
struct ad_row_class {
    const int *irp_a, *irp_b;
    int64_t edge;
    __device__ int operator()(int64_t r) const {
        return ((int64_t)irp_a[r + 1] - irp_a[r]) +
                           ((int64_t)irp_b[r + 1] - irp_b[r]) <=
                       edge
                   ? 0
                   : 1;
    }
};

/* ------------------------------------------------------------------ */
/* class 0: a group of G lanes per row                                  */
/* ------------------------------------------------------------------ */

/* list NULL: item i is row i (one class holds every row) */
template <int G>
__global__ void __launch_bounds__(AD_T)
k_add_count_group(const int *__restrict__ list, int64_t n_list,
                  const int *__restrict__ irp_a, const int *__restrict__ ja_a,
                  const int *__restrict__ irp_b, const int *__restrict__ ja_b,
                  int *__restrict__ count) {
    constexpr int TEAMS = AD_T / G;
    const int team = threadIdx.x / G, gl = threadIdx.x % G;
    const int64_t item = (int64_t)blockIdx.x * TEAMS + team;
    const bool live = item < n_list; /* group-uniform */
    int r = 0, a0 = 0, la = 0, b0 = 0, lb = 0;
    if (live) {
        r = list ? list[item] : (int)item;
        a0 = irp_a[r];
        la = irp_a[r + 1] - a0;
        b0 = irp_b[r];
        lb = irp_b[r + 1] - b0;
    }
    int matches = 0;
    if (lb > 0)
        for (int i = gl; i < la; i += G) {
            const int c = ja_a[a0 + i];
            const int p = ad_lower_bound(ja_b + b0, lb, c);
            matches += p < lb && ja_b[b0 + p] == c;
        }
#pragma unroll
    for (int d = G / 2; d > 0; d >>= 1)
        matches += __shfl_down(matches, d, G);
    if (live && gl == 0)
        count[r] = (int)((int64_t)la + lb - matches);
}

template <int G, typename VA, typename VB>
__global__ void __launch_bounds__(AD_T)
k_add_rows_group(const int *__restrict__ list, int64_t n_list, double alpha,
                 const int *__restrict__ irp_a, const int *__restrict__ ja_a,
                 const VA *__restrict__ as_a, double beta,
                 const int *__restrict__ irp_b, const int *__restrict__ ja_b,
                 const VB *__restrict__ as_b, const int *__restrict__ irp_c,
                 int *__restrict__ ja_c, double *__restrict__ as_c) {
    constexpr int TEAMS = AD_T / G;
    constexpr unsigned GMASK = G == 32 ? 0xffffffffu : (1u << G) - 1u;
    const int team = threadIdx.x / G, gl = threadIdx.x % G;
    const int lane = threadIdx.x & (WAVE - 1);
    const int gbase = lane - gl; /* the group's first lane in the wavefront */
    const unsigned below = (1u << gl) - 1u;
    const int64_t item = (int64_t)blockIdx.x * TEAMS + team;
    int a0 = 0, la = 0, b0 = 0, lb = 0, c0 = 0, ce = 0;
    if (item < n_list) { /* group-uniform */
        const int r = list ? list[item] : (int)item;
        a0 = irp_a[r];
        la = irp_a[r + 1] - a0;
        b0 = irp_b[r];
        lb = irp_b[r + 1] - b0;
        c0 = irp_c[r];
        ce = irp_c[r + 1];
    }
    const int64_t len = (int64_t)la + lb;
    int carry_a = 0, carry_b = 0; /* matched entries of A / of B so far */
    /* wavefront-uniform trips: the ballots are taken by all 64 lanes */
    for (int64_t k0 = 0; __any(k0 < len); k0 += G) {
        const int64_t k = k0 + gl;
        const bool on = k < len, side_a = k < la;
        int at = 0, c = 0, p = 0;
        bool match = false;
        if (on) {
            if (side_a) {
                at = (int)k;
                c = ja_a[a0 + at];
                p = ad_lower_bound(ja_b + b0, lb, c);
                match = p < lb && ja_b[b0 + p] == c;
            } else {
                at = (int)(k - la);
                c = ja_b[b0 + at];
                p = ad_lower_bound(ja_a + a0, la, c);
                match = p < la && ja_a[a0 + p] == c;
            }
        }
        const unsigned ma =
            (unsigned)(__ballot(on && side_a && match) >> gbase) & GMASK;
        const unsigned mb =
            (unsigned)(__ballot(on && !side_a && match) >> gbase) & GMASK;
        if (on && (side_a || !match)) {
            const int before = side_a ? carry_a + __popc(ma & below)
                                      : carry_b + __popc(mb & below);
            const int64_t pos = (int64_t)c0 + at + p - before;
            double v;
            if (side_a) {
                v = alpha * widen(as_a[a0 + at]);
                if (match) {
                    const double tb = beta * widen(as_b[b0 + p]);
                    v = v + tb;
                }
            } else {
                v = beta * widen(as_b[b0 + at]);
            }
            if (pos < ce) { /* always: the count pass counted this union */
                ja_c[pos] = c;
                as_c[pos] = v;
            }
        }
        carry_a += __popc(ma);
        carry_b += __popc(mb);
    }
}

/* ------------------------------------------------------------------ */
/* class 1: a workgroup per row                                         */
/* ------------------------------------------------------------------ */

__global__ void __launch_bounds__(AD_T)
k_add_count_wg(const int *__restrict__ list, const int *__restrict__ irp_a,
               const int *__restrict__ ja_a, const int *__restrict__ irp_b,
               const int *__restrict__ ja_b, int *__restrict__ count) {
    __shared__ int wsum[AD_WAVES];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int r = list ? list[blockIdx.x] : (int)blockIdx.x;
    const int a0 = irp_a[r], la = irp_a[r + 1] - a0;
    const int b0 = irp_b[r], lb = irp_b[r + 1] - b0;
    int matches = 0;
    if (lb > 0)
        for (int64_t i = tid; i < la; i += AD_T) {
            const int c = ja_a[a0 + i];
            const int p = ad_lower_bound(ja_b + b0, lb, c);
            matches += p < lb && ja_b[b0 + p] == c;
        }
    matches = (int)wave_sum((ad_u64)matches);
    if (lane == 0)
        wsum[wave] = matches;
    __syncthreads();
    if (tid == 0) {
        int all = 0;
#pragma unroll
        for (int w = 0; w < AD_WAVES; ++w)
            all += wsum[w];
        count[r] = (int)((int64_t)la + lb - all);
    }
}

template <typename VA, typename VB>
__global__ void __launch_bounds__(AD_T)
k_add_rows_wg(const int *__restrict__ list, double alpha,
              const int *__restrict__ irp_a, const int *__restrict__ ja_a,
              const VA *__restrict__ as_a, double beta,
              const int *__restrict__ irp_b, const int *__restrict__ ja_b,
              const VB *__restrict__ as_b, const int *__restrict__ irp_c,
              int *__restrict__ ja_c, double *__restrict__ as_c) {
    __shared__ int wsum[2][AD_WAVES];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int r = list ? list[blockIdx.x] : (int)blockIdx.x;
    const int a0 = irp_a[r], la = irp_a[r + 1] - a0;
    const int b0 = irp_b[r], lb = irp_b[r + 1] - b0;
    const int c0 = irp_c[r], ce = irp_c[r + 1];
    const int64_t len = (int64_t)la + lb;
    int carry_a = 0, carry_b = 0;
    for (int64_t k0 = 0; k0 < len; k0 += AD_T) { /* workgroup-uniform */
        const int64_t k = k0 + tid;
        const bool on = k < len, side_a = k < la;
        int at = 0, c = 0, p = 0;
        bool match = false;
        if (on) {
            if (side_a) {
                at = (int)k;
                c = ja_a[a0 + at];
                p = ad_lower_bound(ja_b + b0, lb, c);
                match = p < lb && ja_b[b0 + p] == c;
            } else {
                at = (int)(k - la);
                c = ja_b[b0 + at];
                p = ad_lower_bound(ja_a + a0, la, c);
                match = p < la && ja_a[a0 + p] == c;
            }
        }
        const ad_u64 ma = __ballot(on && side_a && match);
        const ad_u64 mb = __ballot(on && !side_a && match);
        if (lane == 0) {
            wsum[0][wave] = __popcll(ma);
            wsum[1][wave] = __popcll(mb);
        }
        __syncthreads();
        int before_a = 0, before_b = 0, all_a = 0, all_b = 0;
#pragma unroll
        for (int w = 0; w < AD_WAVES; ++w) {
            before_a += w < wave ? wsum[0][w] : 0;
            before_b += w < wave ? wsum[1][w] : 0;
            all_a += wsum[0][w];
            all_b += wsum[1][w];
        }
        if (on && (side_a || !match)) {
            const int before =
                side_a ? carry_a + before_a + (int)lanes_below(ma)
                       : carry_b + before_b + (int)lanes_below(mb);
            const int64_t pos = (int64_t)c0 + at + p - before;
            double v;
            if (side_a) {
                v = alpha * widen(as_a[a0 + at]);
                if (match) {
                    const double tb = beta * widen(as_b[b0 + p]);
                    v = v + tb;
                }
            } else {
                v = beta * widen(as_b[b0 + at]);
            }
            if (pos < ce) { /* always: the count pass counted this union */
                ja_c[pos] = c;
                as_c[pos] = v;
            }
        }
        carry_a += all_a;
        carry_b += all_b;
        __syncthreads(); /* wsum is rewritten by the next chunk */
    }
}

/* ------------------------------------------------------------------ */
/* launcher: the arguments were checked by the caller (engine.hip)      */
/* ------------------------------------------------------------------ */

/* the one owner of the scratch: freed on every path */
struct ad_scratch {
    char *base = NULL;
    ~ad_scratch() { (void)hipFree(base); }
};

/* the last successful sum of this process, for tools/add_report.py: host-clock
 * ms of the checks, of the count pass and the scan, and of the allocation and
 * the fill pass (the caller adds the finishing of the handle to the last) */
static double g_ad_phase_ms[3];
void csr_add_last_phases(double ms[3]) {
    for (int i = 0; i < 3; ++i)
        ms[i] = g_ad_phase_ms[i];
}
void csr_add_finish_ms(double ms) { g_ad_phase_ms[2] += ms; }

struct ad_args {
    const spmv_csr_dev *A, *B;
    double alpha, beta;
    int width;
    const int *list[ADD_CLASSES]; /* NULL: the identity */
    int64_t rows[ADD_CLASSES];
    int *count;
    spmv_csr_dev *C;
};

template <int G> static void ad_count_group(const ad_args &g, hipStream_t s) {
    hipLaunchKernelGGL((k_add_count_group<G>),
                       dim3((unsigned)add_grid(0, G, g.rows[0])), dim3(AD_T), 0,
                       s, g.list[0], g.rows[0], g.A->irp, g.A->ja, g.B->irp,
                       g.B->ja, g.count);
}

static int ad_count(const ad_args &g, hipStream_t s) {
    if (g.rows[0] > 0)
        switch (g.width) {
        case 2: ad_count_group<2>(g, s); break;
        case 4: ad_count_group<4>(g, s); break;
        case 8: ad_count_group<8>(g, s); break;
        case 16: ad_count_group<16>(g, s); break;
        case 32: ad_count_group<32>(g, s); break;
        default: return -EINVAL;
        }
    if (g.rows[1] > 0)
        hipLaunchKernelGGL(k_add_count_wg, dim3((unsigned)g.rows[1]),
                           dim3(AD_T), 0, s, g.list[1], g.A->irp, g.A->ja,
                           g.B->irp, g.B->ja, g.count);
    return hip_errno(hipGetLastError());
}

template <int G, typename VA, typename VB>
static void ad_rows_group(const ad_args &g, hipStream_t s) {
    hipLaunchKernelGGL((k_add_rows_group<G, VA, VB>),
                       dim3((unsigned)add_grid(0, G, g.rows[0])), dim3(AD_T), 0,
                       s, g.list[0], g.rows[0], g.alpha, g.A->irp, g.A->ja,
                       values_of<VA>(g.A), g.beta, g.B->irp, g.B->ja,
                       values_of<VB>(g.B), g.C->irp, g.C->ja, g.C->as);
}

template <typename VA, typename VB>
static int ad_rows(const ad_args &g, hipStream_t s) {
    if (g.rows[0] > 0)
        switch (g.width) {
        case 2: ad_rows_group<2, VA, VB>(g, s); break;
        case 4: ad_rows_group<4, VA, VB>(g, s); break;
        case 8: ad_rows_group<8, VA, VB>(g, s); break;
        case 16: ad_rows_group<16, VA, VB>(g, s); break;
        case 32: ad_rows_group<32, VA, VB>(g, s); break;
        default: return -EINVAL;
        }
    if (g.rows[1] > 0)
        hipLaunchKernelGGL((k_add_rows_wg<VA, VB>), dim3((unsigned)g.rows[1]),
                           dim3(AD_T), 0, s, g.list[1], g.alpha, g.A->irp,
                           g.A->ja, values_of<VA>(g.A), g.beta, g.B->irp,
                           g.B->ja, values_of<VB>(g.B), g.C->irp, g.C->ja,
                           g.C->as);
    return hip_errno(hipGetLastError());
}

/* *out (M x N, f64, allocated once the entries of C are known) gets its
 * irp, ja and values.  Blocks.  -EDOM: a column outside [0, N); -EINVAL: a row
 * that is not strictly ascending; -EOVERFLOW: more than INT32_MAX entries.  On
 * an error *out and *info are untouched and everything is freed. */
int csr_add_dev(double alpha, const spmv_csr_dev *A, double beta,
                const spmv_csr_dev *B, int mode, spmv_csr_dev **out,
                spmv_add_info *info, hipStream_t s) {
    int rc = 0;
    const int M = A->M, N = A->N;
    add_plan pl;
    ad_scratch scratch;
    spmv_csr_dev *Cm = NULL;
    ad_u64 h[ADD_HEAD_WORDS];
    ad_u64 cursor[ADD_CLASSES];
    ad_u64 *head = NULL;
    int *count = NULL, *list = NULL, *sums = NULL;
    int64_t nz = 0, matched = 0;
    ad_args g;
    double t0 = csr_now_ms(), t1 = 0, t2 = 0;
    const dim3 block(AD_T);
    /* the reduction over the rows: grid-stride, an atomic a workgroup */
    const dim3 reduce_grid(
        (unsigned)std::min<int64_t>(ADD_REDUCE_GRID, add_ceil_div(M, AD_T)));
    /* class 0 serves len <= edge */
    const int64_t edge = mode == 1 ? INT64_MAX : mode == 2 ? -1 : ADD_EDGE;
    rc = add_plan_make(M, N, A->NZ, B->NZ, &pl);
    if (rc)
        return rc;
    (void)hipGetLastError(); /* an earlier caller's unread error is not ours */
    HIP_TRY(hipMalloc((void **)&scratch.base, (size_t)pl.scratch_bytes));
    head = (ad_u64 *)(scratch.base + pl.off_head);
    count = (int *)(scratch.base + pl.off_count);
    list = (int *)(scratch.base + pl.off_list);
    sums = (int *)(scratch.base + pl.off_sums);
    HIP_TRY(hipMemsetAsync(head, 0, ADD_HEAD_WORDS * 8, s));
    HIP_TRY(hipMemsetAsync(count, 0, ((size_t)M + 1) * sizeof(int), s));
    /* 1. the checks of both operands (one pass when B is A), the classes */
    rc = csr_check_rows_dev(A, head + AD_FLAGS, s);
    if (!rc && B != A)
        rc = csr_check_rows_dev(B, head + AD_FLAGS, s);
    if (rc)
        goto fail;
    if (M > 0)
        hipLaunchKernelGGL(k_add_bound, reduce_grid, block, 0, s, M, A->irp,
                           B->irp, edge, head);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h, head, sizeof h, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    t1 = csr_now_ms();
    rc = csr_flags_errno(h[AD_FLAGS]);
    if (rc)
        goto fail;
    g.A = A;
    g.B = B;
    g.alpha = alpha;
    g.beta = beta;
    g.width = pl.width;
    g.count = count;
    g.C = NULL;
    g.rows[1] = (int64_t)h[AD_ROWS + 1];
    g.rows[0] = M - g.rows[1];
    if (g.rows[0] < 0) {
        rc = -EIO;
        goto fail;
    }
    /* 2. the lists of the two classes, one after the other -- or none, when
     * one class holds every row */
    g.list[0] = g.list[1] = NULL;
    if (g.rows[0] > 0 && g.rows[1] > 0) {
        cursor[0] = 0;
        cursor[1] = (ad_u64)g.rows[0];
        HIP_TRY(hipMemcpyAsync(head + AD_CURSOR, cursor, sizeof cursor,
                               hipMemcpyHostToDevice, s));
        csr_lists_dev<ADD_CLASSES>(M, ad_row_class{A->irp, B->irp, edge},
                                   head + AD_CURSOR, list, s);
        g.list[0] = list;
        g.list[1] = list + g.rows[0];
    }
    /* 3. the union lengths, their total: the one thing that can still refuse
     * the sum */
    rc = ad_count(g, s);
    if (rc)
        goto fail;
    rc = csr_total_dev(count, M, head + AD_NZ, s);
    if (rc)
        goto fail;
    HIP_TRY(hipMemcpyAsync(h, head, sizeof h, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    nz = (int64_t)h[AD_NZ];
    rc = add_nz_guard(nz);
    if (!rc)
        rc = add_matched(A->NZ, B->NZ, nz, &matched);
    /* 4. C, its IRP (the scan ends the second phase), the fill pass */
    if (!rc)
        rc = csr_alloc_scanned_dev(M, N, nz, count, sums, &t2, &Cm, s);
    if (rc)
        goto fail;
    g.C = Cm;
    rc = csr_value_types(A, B, [&](auto va, auto vb) {
        return ad_rows<decltype(va), decltype(vb)>(g, s);
    });
    if (rc)
        goto fail;
    HIP_TRY(hipStreamSynchronize(s));
    g_ad_phase_ms[0] = t1 - t0;
    g_ad_phase_ms[1] = t2 - t1;
    g_ad_phase_ms[2] = csr_now_ms() - t2;
    if (info) {
        info->nz = (int)nz;
        info->matched = matched;
        info->widest = (int64_t)h[AD_WIDEST];
        info->rows_in_bin[0] = g.rows[0];
        info->rows_in_bin[1] = g.rows[1];
    }
    *out = Cm;
    return 0;
fail: /* nothing of ours is left running when the scratch is freed */
    (void)hipStreamSynchronize(s);
    spmv_csr_release(Cm); /* NULL: ignored */
    return rc;
}

/* ------------------------------------------------------------------ */
/* the companions: one streaming kernel each                            */
/* ------------------------------------------------------------------ */

/* row i holds the one entry (i, i); the value's bits are copied */
__global__ void __launch_bounds__(AD_T)
k_add_from_diag(int M, const ad_u64 *__restrict__ diag, int *__restrict__ irp,
                int *__restrict__ ja, ad_u64 *__restrict__ as) {
    const int64_t i = (int64_t)blockIdx.x * AD_T + threadIdx.x;
    if (i <= M)
        irp[i] = (int)i;
    if (i < M) {
        ja[i] = (int)i;
        as[i] = diag ? diag[i] : 0x3ff0000000000000ull; /* 1.0 */
    }
}

int csr_from_diag_dev(const double *d_diag, spmv_csr_dev *D, hipStream_t s) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_add_from_diag,
                       grid_for((int64_t)D->M + 1, AD_T), dim3(AD_T), 0, s,
                       D->M, (const ad_u64 *)d_diag, D->irp, D->ja,
                       (ad_u64 *)D->as);
    HIP_RET(hipGetLastError());
    HIP_RET(hipStreamSynchronize(s));
    return 0;
}

/* one lane per entry q: out[q] = rn(rn(l[row] a) r[col]), either factor
 * optional.  The row is found in IRP only when l is given.  A column outside
 * [0, N) is not looked up and raises the flag */
template <typename V>
__global__ void __launch_bounds__(AD_T)
k_add_scale(const int *__restrict__ irp, const int *__restrict__ ja,
            const V *__restrict__ as, int M, int64_t NZ, int N,
            const double *__restrict__ l, const double *__restrict__ r,
            double *__restrict__ out, unsigned *__restrict__ flag) {
    const int64_t q = (int64_t)blockIdx.x * AD_T + threadIdx.x;
    if (q >= NZ)
        return;
    double v = widen(ld_stream(as + q));
    if (l) {
        int lo = 0, hi = M; /* irp[lo] <= q < irp[hi] */
        while (hi - lo > 1) {
            const int mid = lo + (hi - lo) / 2;
            if (irp[mid] <= q)
                lo = mid;
            else
                hi = mid;
        }
        v = l[lo] * v;
    }
    if (r) {
        const int c = ld_stream(ja + q);
        if ((unsigned)c < (unsigned)N)
            v = v * r[c];
        else
            atomicOr(flag, CSR_BAD_COLUMN);
    }
    out[q] = v;
}

/* S has A's shape and entry count and owns f64 values; its irp and ja are
 * copied from A's.  Blocks.  -EDOM: d_right given and a column outside */
int csr_scale_dev(const spmv_csr_dev *A, const double *d_left,
                  const double *d_right, spmv_csr_dev *S, hipStream_t s) {
    int rc = 0;
    unsigned *d_flag = NULL, flag = 0;
    (void)hipGetLastError();
    HIP_TRY(hipMemcpyAsync(S->irp, A->irp, ((size_t)A->M + 1) * sizeof(int),
                           hipMemcpyDeviceToDevice, s));
    if (A->NZ > 0) {
        const dim3 grid = grid_for(A->NZ, AD_T);
        HIP_TRY(hipMemcpyAsync(S->ja, A->ja, (size_t)A->NZ * sizeof(int),
                               hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipMalloc((void **)&d_flag, sizeof(unsigned)));
        HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(unsigned), s));
        if (A->value_bytes == 4)
            hipLaunchKernelGGL((k_add_scale<float>), grid, dim3(AD_T), 0, s,
                               A->irp, A->ja, A->as32, A->M, A->NZ, A->N,
                               d_left, d_right, S->as, d_flag);
        else
            hipLaunchKernelGGL((k_add_scale<double>), grid, dim3(AD_T), 0, s,
                               A->irp, A->ja, A->as, A->M, A->NZ, A->N, d_left,
                               d_right, S->as, d_flag);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&flag, d_flag, sizeof flag,
                               hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    rc = csr_flags_errno(flag);
fail:
    if (rc)
        (void)hipStreamSynchronize(s);
    (void)hipFree(d_flag);
    return rc;
}
