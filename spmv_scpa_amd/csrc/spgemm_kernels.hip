/*
 * spgemm_kernels.hip -- C = A B of two CSR handles on the device
 * (spmv_csr_spgemm; spmv_engine.h), gfx950 (wave64).
 *
 * The result is defined to the bit (spmv_engine.h): row r of C holds every
 * column that a product of the walk "entries p of A's row r in stored order,
 * entries q of B's row JA_A[p] in stored order" meets, once, ascending; its
 * value is the sequential sum of the column's products in walk order, the
 * first product initialising the sum, every product and sum rounded on its
 * own (this file is compiled with contraction off: no fused multiply-add).
 *
 * The geometry (size classes, tables, LDS, scratch, batches) is
 * spgemm_plan.h's; the steps every builder of a handle shares are
 * csr_build.h's.  The launches, in order -- the kernel boundary is the only
 * ordering between workgroups, nothing waits on another workgroup:
 *
 *   csr_check_rows_dev (B)
 *   k_sg_bound     one lane per row of A: ub[r], A's columns inside [0, K),
 *                  and the totals (integer atomics: a SUM, a MAXIMUM and a
 *                  COUNT do not depend on the order of arrival)
 *   csr_lists_dev  the rows of each class (sg_class of ub[r]), listed
 *   k_sg_rows<.., false>, k_sg_fb_count      symbolic: distinct columns per row
 *   csr_total_dev, csr_alloc_scanned_dev     C's IRP
 *   k_sg_rows<.., true>, k_sg_fb_rows        numeric: JA and AS of C
 *
 * Classes 0..2 (k_sg_rows): a team of lanes owns the row.  The columns go into
 * an LDS hash SET (atomicCAS on the key: membership has no order; linear
 * probing, at most `table` probes, the table never more than half full).  The
 * numeric pass gathers the n keys of the set, sorts them (bitonic over the
 * next power of two, padded with INT32_MAX, above every column), which leaves
 * the row's columns ascending in slots 0..n-1, and then walks A's entries p
 * ONE AFTER THE OTHER with the lanes spread over q.  B's rows are strictly
 * ascending, so the lanes of one step meet distinct columns, i.e. distinct
 * slots (found by a binary search in the sorted keys): plain LDS loads and
 * stores, no atomics on values, and a "touched" byte per slot tells the first
 * product from the later ones.
 *
 * Class 3 (k_sg_fb_*): one workgroup per row, a dense accumulator of N
 * doubles and N bits in global scratch, the same walk.  The compaction is a
 * scan over the bits, which gives the ascending order for free and costs
 * O(N) per row.  The bits are cleared on the way out, so the next batch
 * finds them zero; the accumulator needs no clearing (a value is read only
 * after its bit was set in the same row).
 *
 * Every device loop is bounded by a row length, a table size or N.  A column
 * outside its range is skipped here (and refused by the launcher before
 * anything is allocated for C), so nothing is ever written out of bounds.
 */
#include <string.h>

#include "csr_build.h"
#include "spgemm_plan.h"

/* every product and every sum is rounded on its own */
#pragma clang fp contract(off)

#define SG_T SPGEMM_THREADS
#define SG_WAVES (SG_T / WAVE)
#define SG_EMPTY 0x7fffffff /* INT32_MAX: no column (columns are < N) */

static_assert(SPGEMM_SCAN_TILE == TRANSPOSE_SCAN_TILE,
              "spgemm_plan.h sizes the scan's sums for tr_scan");

typedef unsigned long long sg_u64;

/* the 64-bit words of the head */
enum {
    SG_FLAGS = 0,    /* 1: a column outside its range, 2: B not ascending */
    SG_PRODUCTS = 1, /* sum of ub */
    SG_WIDEST = 2,   /* max of ub */
    SG_ROWS = 3,     /* [4] rows per class */
    SG_CURSOR = 7,   /* [4] next free place of each class's list */
    SG_NZ = 11       /* entries of C */
};
static_assert(SG_NZ < SPGEMM_HEAD_WORDS, "the head holds every word");

__device__ __forceinline__ int sg_class(int64_t ub) {
    return ub <= SPGEMM_TABLE0 / 2   ? 0
           : ub <= SPGEMM_TABLE1 / 2 ? 1
           : ub <= SPGEMM_TABLE2 / 2 ? 2
                                     : 3;
}

/* the class of a row, for csr_lists_dev */
struct sg_row_class {
    const int64_t *ub;
    __device__ int operator()(int64_t r) const { return sg_class(ub[r]); }
};

/* ------------------------------------------------------------------ */
/* bounds                                                               */
/* ------------------------------------------------------------------ */

__global__ void __launch_bounds__(SG_T)
k_sg_bound(int M, int K, const int *__restrict__ irp_a,
           const int *__restrict__ ja_a, const int *__restrict__ irp_b,
           int64_t *__restrict__ ub, sg_u64 *__restrict__ head) {
    const int64_t r = (int64_t)blockIdx.x * SG_T + threadIdx.x;
    const int lane = threadIdx.x & (WAVE - 1);
    const bool valid = r < M;
    int64_t u = 0;
    bool bad = false;
    if (valid) {
        const int pe = irp_a[r + 1];
        for (int p = irp_a[r]; p < pe; ++p) {
            const int k = ja_a[p];
            if ((unsigned)k < (unsigned)K)
                u += irp_b[k + 1] - irp_b[k];
            else
                bad = true;
        }
        ub[r] = u;
    }
    const int cls = valid ? sg_class(u) : -1;
#pragma unroll
    for (int c = 0; c < SPGEMM_CLASSES; ++c) {
        const sg_u64 mask = __ballot(cls == c);
        if (mask && lane == __ffsll((long long)mask) - 1)
            atomicAdd(head + SG_ROWS + c, (sg_u64)__popcll(mask));
    }
    const sg_u64 most = wave_max((sg_u64)u);
    const sg_u64 sum = wave_sum((sg_u64)u);
    const sg_u64 anybad = __ballot(bad);
    if (lane == 0) {
        if (sum)
            atomicAdd(head + SG_PRODUCTS, sum);
        if (most)
            atomicMax(head + SG_WIDEST, most);
        if (anybad)
            atomicOr(head + SG_FLAGS, (sg_u64)1);
    }
}

/* ------------------------------------------------------------------ */
/* classes 0..2: a team of lanes and an LDS table per row               */
/* ------------------------------------------------------------------ */

/* everything the team wrote to LDS before is visible to it after */
template <int TEAM> __device__ __forceinline__ void sg_sync(void) {
    if (TEAM > WAVE) {
        __syncthreads();
    } else { /* the team is (part of) one wavefront */
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
}

template <int TEAM, int TAB, bool NUMERIC, typename VA, typename VB>
__global__ void __launch_bounds__(SG_T)
k_sg_rows(const int *__restrict__ list, int64_t n_list,
          const int *__restrict__ irp_a, const int *__restrict__ ja_a,
          const VA *__restrict__ as_a, const int *__restrict__ irp_b,
          const int *__restrict__ ja_b, const VB *__restrict__ as_b, int K,
          int N, int *__restrict__ count, const int *__restrict__ irp_c,
          int *__restrict__ ja_c, double *__restrict__ as_c) {
    static_assert(TEAM <= WAVE || TEAM == SG_T,
                  "a team is inside a wavefront or the whole workgroup");
    static_assert((TAB & (TAB - 1)) == 0, "the probe and the sort mask by TAB");
    extern __shared__ double sg_lds[];
    constexpr int TEAMS = SG_T / TEAM;
    constexpr int BYTES = TAB / 2 * 8 + TAB * 4 + TAB / 2 + 8;
    const int team = threadIdx.x / TEAM, lane = threadIdx.x % TEAM;
    const int64_t item = (int64_t)blockIdx.x * TEAMS + team;
    if (item >= n_list) /* team-uniform; TEAM == SG_T: the grid is n_list */
        return;
    char *const mine = (char *)sg_lds + (size_t)team * BYTES;
    double *const vals = (double *)mine;
    int *const keys = (int *)(mine + TAB / 2 * 8);
    unsigned char *const touched = (unsigned char *)(keys + TAB);
    int *const cnt = (int *)(touched + TAB / 2);
    const int r = list[item];
    const int pa = irp_a[r], pe = irp_a[r + 1];

    for (int i = lane; i < TAB; i += TEAM)
        keys[i] = SG_EMPTY;
    if (lane == 0)
        *cnt = 0;
    sg_sync<TEAM>();
    /* the set of the row's columns */
    for (int p = pa; p < pe; ++p) { /* team-uniform */
        const int k = ja_a[p];
        if ((unsigned)k >= (unsigned)K)
            continue;
        const int qe = irp_b[k + 1];
        for (int q = irp_b[k] + lane; q < qe; q += TEAM) {
            const int c = ja_b[q];
            if ((unsigned)c >= (unsigned)N)
                continue;
            unsigned h = (unsigned)c & (TAB - 1);
            for (int probe = 0; probe < TAB; ++probe) {
                const int old = atomicCAS(&keys[h], SG_EMPTY, c);
                if (old == SG_EMPTY) {
                    if (!NUMERIC)
                        atomicAdd(cnt, 1);
                    break;
                }
                if (old == c)
                    break;
                h = (h + 1) & (TAB - 1);
            }
        }
    }
    sg_sync<TEAM>();
    if constexpr (!NUMERIC) {
        if (lane == 0)
            count[r] = *cnt;
        return;
    } else {
        const int c0 = irp_c[r];
        /* = the row's distinct columns; never beyond the values' slots */
        const int n = min(irp_c[r + 1] - c0, TAB / 2);
        /* the n keys are gathered (into the values' slots, free until the
         * walk) in whatever order the lanes arrive -- the place comes from an
         * atomic, and the sort below forgets it: the keys are distinct -- so
         * that only the next power of two is sorted, not the whole table */
        int *const dense = (int *)vals;
        for (int i = lane; i < TAB; i += TEAM) {
            const int k = keys[i];
            if (k != SG_EMPTY) {
                const int at = atomicAdd(cnt, 1);
                if (at < TAB / 2) /* always: n <= ub <= TAB / 2 */
                    dense[at] = k;
            }
        }
        sg_sync<TEAM>();
        int P = 2;
        while (P < n) /* at most log2(TAB) steps; P <= TAB / 2 */
            P <<= 1;
        for (int i = lane; i < P; i += TEAM)
            keys[i] = i < n ? dense[i] : SG_EMPTY;
        sg_sync<TEAM>();
        /* bitonic sort of keys[0..P): pair t of a step is (i, i | j) */
        for (int k2 = 2; k2 <= P; k2 <<= 1) { /* team-uniform */
            for (int j = k2 >> 1; j > 0; j >>= 1) {
                for (int t = lane; t < P / 2; t += TEAM) {
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                    const int x = i | j;
                    const int a = keys[i], b = keys[x];
                    if ((a > b) == ((i & k2) == 0)) {
                        keys[i] = b;
                        keys[x] = a;
                    }
                }
                sg_sync<TEAM>();
            }
        }
        for (int i = lane; i < n; i += TEAM) {
            ja_c[c0 + i] = keys[i];
            touched[i] = 0;
        }
        sg_sync<TEAM>();
        /* the walk: steps p in order, the lanes of a step on distinct slots */
        for (int p = pa; p < pe; ++p) { /* team-uniform */
            const int k = ja_a[p];
            if ((unsigned)k >= (unsigned)K)
                continue;
            const double a = widen(as_a[p]);
            const int qe = irp_b[k + 1];
            for (int q = irp_b[k] + lane; q < qe; q += TEAM) {
                const int c = ja_b[q];
                const double t = a * widen(as_b[q]);
                int lo = 0, hi = n;
                while (lo < hi) { /* at most log2(TAB) steps */
                    const int mid = (lo + hi) >> 1;
                    if (keys[mid] < c)
                        lo = mid + 1;
                    else
                        hi = mid;
                }
                if (lo < n && keys[lo] == c) {
                    vals[lo] = touched[lo] ? vals[lo] + t : t;
                    touched[lo] = 1;
                }
            }
            sg_sync<TEAM>();
        }
        for (int i = lane; i < n; i += TEAM)
            as_c[c0 + i] = vals[i];
    }
}

/* ------------------------------------------------------------------ */
/* class 3: a workgroup, N doubles and N bits of global scratch per row */
/* ------------------------------------------------------------------ */

__device__ __forceinline__ unsigned sg_load_word(const unsigned *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

/* workgroup b: row list[b], bits slot b */
__global__ void __launch_bounds__(SG_T)
k_sg_fb_count(const int *__restrict__ list, const int *__restrict__ irp_a,
              const int *__restrict__ ja_a, const int *__restrict__ irp_b,
              const int *__restrict__ ja_b, int K, int N, unsigned *bits,
              int64_t bits_stride, int64_t words, int *__restrict__ count) {
    __shared__ int total;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int r = list[blockIdx.x];
    unsigned *const mine = bits + (int64_t)blockIdx.x * bits_stride;
    if (tid == 0)
        total = 0;
    const int pe = irp_a[r + 1];
    for (int p = irp_a[r]; p < pe; ++p) { /* workgroup-uniform */
        const int k = ja_a[p];
        if ((unsigned)k >= (unsigned)K)
            continue;
        const int qb = irp_b[k], qe = irp_b[k + 1];
        for (int q0 = qb; q0 < qe; q0 += SG_T) { /* workgroup-uniform */
            const int q = q0 + tid;
            int word = -1;
            unsigned m = 0;
            if (q < qe) {
                const int c = ja_b[q];
                if ((unsigned)c < (unsigned)N) {
                    word = c >> 5;
                    m = 1u << (c & 31);
                }
            }
            /* neighbouring lanes hold ascending columns: the bits of one
             * word are gathered in the last lane of its run (a run is at
             * most 32 lanes), which alone goes to memory */
#pragma unroll
            for (int d = 1; d < 32; d <<= 1) {
                const int ow = __shfl_up(word, d, WAVE);
                const unsigned om = __shfl_up(m, d, WAVE);
                if (lane >= d && ow == word)
                    m |= om;
            }
            const int next = __shfl_down(word, 1, WAVE);
            if (word >= 0 && (lane == WAVE - 1 || next != word))
                atomicOr(mine + word, m);
        }
    }
    __syncthreads();
    int n = 0;
    for (int64_t w = tid; w < words; w += SG_T) {
        const unsigned v = sg_load_word(mine + w);
        if (v) {
            n += __popc(v);
            mine[w] = 0u;
        }
    }
    n = (int)wave_sum((sg_u64)n);
    if (lane == 0 && n)
        atomicAdd(&total, n);
    __syncthreads();
    if (tid == 0)
        count[r] = total;
}

template <typename VA, typename VB>
__global__ void __launch_bounds__(SG_T)
k_sg_fb_rows(const int *__restrict__ list, const int *__restrict__ irp_a,
             const int *__restrict__ ja_a, const VA *__restrict__ as_a,
             const int *__restrict__ irp_b, const int *__restrict__ ja_b,
             const VB *__restrict__ as_b, int K, int N, double *acc,
             int64_t acc_stride, unsigned *bits, int64_t bits_stride,
             int64_t words, const int *__restrict__ irp_c,
             int *__restrict__ ja_c, double *__restrict__ as_c) {
    __shared__ int wsum[SG_WAVES];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int r = list[blockIdx.x];
    unsigned *const mine = bits + (int64_t)blockIdx.x * bits_stride;
    double *const sums = acc + (int64_t)blockIdx.x * acc_stride;
    const int pe = irp_a[r + 1];
    for (int p = irp_a[r]; p < pe; ++p) { /* workgroup-uniform */
        const int k = ja_a[p];
        if ((unsigned)k >= (unsigned)K)
            continue;
        const double a = widen(as_a[p]);
        const int qe = irp_b[k + 1];
        for (int q = irp_b[k] + tid; q < qe; q += SG_T) {
            const int c = ja_b[q];
            if ((unsigned)c >= (unsigned)N)
                continue;
            const double t = a * widen(as_b[q]);
            const unsigned bit = 1u << (c & 31);
            /* the lanes of one step hold distinct columns: the old bit says
             * whether an EARLIER step met this column */
            const bool was = atomicOr(mine + (c >> 5), bit) & bit;
            sums[c] = was ? sums[c] + t : t;
        }
        __syncthreads(); /* step p + 1 reads what step p wrote */
    }
    __syncthreads();
    /* compaction: thread t owns words [t * chunk, (t + 1) * chunk) */
    const int64_t chunk = (words + SG_T - 1) / SG_T;
    const int64_t w0 = min((int64_t)tid * chunk, words);
    const int64_t w1 = min(w0 + chunk, words);
    int n = 0;
    for (int64_t w = w0; w < w1; ++w)
        n += __popc(sg_load_word(mine + w));
    int incl = n;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const int t = __shfl_up(incl, d, WAVE);
        if (lane >= d)
            incl += t;
    }
    if (lane == WAVE - 1)
        wsum[wave] = incl;
    __syncthreads();
    int before = 0;
#pragma unroll
    for (int w = 0; w < SG_WAVES; ++w)
        before += w < wave ? wsum[w] : 0;
    const int end = irp_c[r + 1];
    int at = irp_c[r] + before + incl - n;
    for (int64_t w = w0; w < w1; ++w) {
        unsigned v = sg_load_word(mine + w);
        if (!v)
            continue;
        mine[w] = 0u;
        while (v) { /* at most 32 bits */
            const int c = (int)(w * 32) + __ffs((int)v) - 1;
            v &= v - 1;
            if (at < end) { /* always: the symbolic pass counted these bits */
                ja_c[at] = c;
                as_c[at] = sums[c];
            }
            ++at;
        }
    }
}

/* ------------------------------------------------------------------ */
/* launcher: the arguments were checked by the caller (engine.hip)      */
/* ------------------------------------------------------------------ */

/* the one owner of the scratch and of the fallback's events: freed on every
 * path */
struct sg_scratch {
    char *base = NULL, *fallback = NULL;
    hipEvent_t ev[4] = {NULL, NULL, NULL, NULL};
    ~sg_scratch() {
        (void)hipFree(base);
        (void)hipFree(fallback);
        for (int i = 0; i < 4; ++i)
            if (ev[i])
                (void)hipEventDestroy(ev[i]);
    }
};

/* the last successful product of this process, for tools/spgemm_report.py:
 * host-clock ms up to the first read-back (checks, bounds), up to the second
 * (lists, symbolic pass) and up to the end (scan, allocation, numeric pass),
 * and the part of the last two that the fallback's launches took (events) */
static double g_sg_phase_ms[4];
void csr_spgemm_last_phases(double ms[4]) {
    for (int i = 0; i < 4; ++i)
        ms[i] = g_sg_phase_ms[i];
}

struct sg_args {
    const spmv_csr_dev *A, *B;
    const int *list;
    int *count;
    const int *irp_c;
    int *ja_c;
    double *as_c;
};

template <int TEAM, int TAB, bool NUMERIC, typename VA, typename VB>
static int sg_launch_class(int c, const sg_args &g, int64_t first, int64_t n,
                           hipStream_t s) {
    if (n == 0)
        return 0;
    auto kernel = k_sg_rows<TEAM, TAB, NUMERIC, VA, VB>;
    const size_t lds = (size_t)spgemm_lds(c);
    if (lds > 64 * 1024) /* per device, per call: a one-off setup path */
        HIP_RET(hipFuncSetAttribute((const void *)kernel,
                                    hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds));
    hipLaunchKernelGGL(kernel, dim3((unsigned)spgemm_grid(c, n)), dim3(SG_T),
                       lds, s, g.list + first, n, g.A->irp, g.A->ja,
                       values_of<VA>(g.A), g.B->irp, g.B->ja,
                       values_of<VB>(g.B), g.A->N, g.B->N, g.count, g.irp_c,
                       g.ja_c, g.as_c);
    return hip_errno(hipGetLastError());
}

template <bool NUMERIC, typename VA, typename VB>
static int sg_launch_tables(const sg_args &g, const int64_t *first,
                            const int64_t *rows, hipStream_t s) {
    int rc = sg_launch_class<SPGEMM_TEAM0, SPGEMM_TABLE0, NUMERIC, VA, VB>(
        0, g, first[0], rows[0], s);
    if (!rc)
        rc = sg_launch_class<SPGEMM_TEAM1, SPGEMM_TABLE1, NUMERIC, VA, VB>(
            1, g, first[1], rows[1], s);
    if (!rc)
        rc = sg_launch_class<SPGEMM_TEAM2, SPGEMM_TABLE2, NUMERIC, VA, VB>(
            2, g, first[2], rows[2], s);
    return rc;
}

template <typename VA, typename VB>
static int sg_numeric(const sg_args &g, const int64_t *first,
                      const int64_t *rows, const spgemm_fallback &fb,
                      double *acc, unsigned *bits, hipEvent_t *ev,
                      hipStream_t s) {
    int rc = sg_launch_tables<true, VA, VB>(g, first, rows, s);
    if (rc)
        return rc;
    if (fb.launches)
        HIP_RET(hipEventRecord(ev[2], s));
    for (int64_t l = 0; l < fb.launches; ++l) {
        int64_t b0, bn;
        spgemm_fallback_batch(&fb, rows[3], l, &b0, &bn);
        hipLaunchKernelGGL((k_sg_fb_rows<VA, VB>), dim3((unsigned)bn),
                           dim3(SG_T), 0, s, g.list + first[3] + b0, g.A->irp,
                           g.A->ja, values_of<VA>(g.A), g.B->irp, g.B->ja,
                           values_of<VB>(g.B), g.A->N, g.B->N, acc,
                           fb.acc_stride / 8, bits, fb.bits_stride / 4,
                           fb.words, g.irp_c, g.ja_c, g.as_c);
    }
    if (fb.launches)
        HIP_RET(hipEventRecord(ev[3], s));
    return hip_errno(hipGetLastError());
}

/* *out (M x N, f64, allocated once the entries of C are known) gets its
 * irp, ja and values.  Blocks.  -EDOM: a column outside its range; -EINVAL: a
 * row of B that is not strictly ascending; -EOVERFLOW: more than INT32_MAX
 * entries.  On an error *out is untouched and everything is freed. */
int csr_spgemm_dev(const spmv_csr_dev *A, const spmv_csr_dev *B,
                   spmv_csr_dev **out, spmv_spgemm_info *info, hipStream_t s) {
    int rc = 0;
    const int M = A->M, K = A->N, N = B->N;
    spgemm_plan pl;
    spgemm_fallback fb;
    sg_scratch scratch;
    spmv_csr_dev *Cm = NULL;
    sg_u64 h[SPGEMM_HEAD_WORDS];
    int64_t rows[SPGEMM_CLASSES], first[SPGEMM_CLASSES];
    sg_u64 cursor[SPGEMM_CLASSES];
    sg_u64 *head = NULL;
    int64_t *ub = NULL;
    int *count = NULL, *list = NULL, *sums = NULL;
    double *acc = NULL;
    unsigned *bits = NULL;
    int64_t nz = 0;
    sg_args g;
    double t0 = csr_now_ms(), t1 = 0, t2 = 0;
    float fb_sym = 0.f, fb_num = 0.f;
    const dim3 block(SG_T);
    rc = spgemm_plan_make(M, K, N, &pl);
    if (rc)
        return rc;
    memset(&fb, 0, sizeof fb);
    (void)hipGetLastError(); /* an earlier caller's unread error is not ours */
    HIP_TRY(hipMalloc((void **)&scratch.base, (size_t)pl.scratch_bytes));
    head = (sg_u64 *)(scratch.base + pl.off_head);
    ub = (int64_t *)(scratch.base + pl.off_ub);
    count = (int *)(scratch.base + pl.off_count);
    list = (int *)(scratch.base + pl.off_list);
    sums = (int *)(scratch.base + pl.off_sums);
    HIP_TRY(hipMemsetAsync(head, 0, SPGEMM_HEAD_WORDS * 8, s));
    HIP_TRY(hipMemsetAsync(count, 0, ((size_t)M + 1) * sizeof(int), s));
    /* 1. the checks and the bounds */
    rc = csr_check_rows_dev(B, head + SG_FLAGS, s);
    if (rc)
        goto fail;
    if (M > 0)
        hipLaunchKernelGGL(k_sg_bound, grid_for(M, SG_T), block, 0, s, M, K,
                           A->irp, A->ja, B->irp, ub, head);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h, head, sizeof h, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    t1 = csr_now_ms();
    rc = csr_flags_errno(h[SG_FLAGS]);
    if (rc)
        goto fail;
    /* 2. the lists of the classes, one after the other */
    for (int c = 0, at = 0; c < SPGEMM_CLASSES; ++c) {
        rows[c] = (int64_t)h[SG_ROWS + c];
        first[c] = at;
        cursor[c] = (sg_u64)at;
        at += (int)rows[c];
    }
    if (rows[0] + rows[1] + rows[2] + rows[3] != M) {
        rc = -EIO;
        goto fail;
    }
    if (M > 0) {
        HIP_TRY(hipMemcpyAsync(head + SG_CURSOR, cursor, sizeof cursor,
                               hipMemcpyHostToDevice, s));
        csr_lists_dev<SPGEMM_CLASSES>(M, sg_row_class{ub}, head + SG_CURSOR,
                                      list, s);
    }
    g.A = A;
    g.B = B;
    g.list = list;
    g.count = count;
    g.irp_c = NULL;
    g.ja_c = NULL;
    g.as_c = NULL;
    /* 3. symbolic: the distinct columns of every row */
    rc = sg_launch_tables<false, double, double>(g, first, rows, s);
    if (rc)
        goto fail;
    rc = spgemm_fallback_make(N, rows[3], &fb);
    if (rc)
        goto fail;
    if (rows[3] > 0) {
        HIP_TRY(hipMalloc((void **)&scratch.fallback,
                          (size_t)fb.scratch_bytes));
        acc = (double *)(scratch.fallback + fb.off_acc);
        bits = (unsigned *)(scratch.fallback + fb.off_bits);
        HIP_TRY(hipMemsetAsync(bits, 0, (size_t)(fb.batch * fb.bits_stride),
                               s));
        for (int i = 0; i < 4; ++i)
            HIP_TRY(hipEventCreate(&scratch.ev[i]));
        HIP_TRY(hipEventRecord(scratch.ev[0], s));
        for (int64_t l = 0; l < fb.launches; ++l) {
            int64_t b0, bn;
            spgemm_fallback_batch(&fb, rows[3], l, &b0, &bn);
            hipLaunchKernelGGL(k_sg_fb_count, dim3((unsigned)bn), block, 0, s,
                               list + first[3] + b0, A->irp, A->ja, B->irp,
                               B->ja, K, N, bits, fb.bits_stride / 4, fb.words,
                               count);
        }
        HIP_TRY(hipEventRecord(scratch.ev[1], s));
    }
    /* 4. C's IRP, and the one thing that can still refuse the product */
    rc = csr_total_dev(count, M, head + SG_NZ, s);
    if (rc)
        goto fail;
    HIP_TRY(hipMemcpyAsync(h, head, sizeof h, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    t2 = csr_now_ms();
    nz = (int64_t)h[SG_NZ];
    rc = spgemm_nz_guard(nz);
    if (!rc)
        rc = csr_alloc_scanned_dev(M, N, nz, count, sums, NULL, &Cm, s);
    if (rc)
        goto fail;
    /* 5. numeric */
    g.irp_c = Cm->irp;
    g.ja_c = Cm->ja;
    g.as_c = Cm->as;
    rc = csr_value_types(A, B, [&](auto va, auto vb) {
        return sg_numeric<decltype(va), decltype(vb)>(g, first, rows, fb, acc,
                                                      bits, scratch.ev, s);
    });
    if (rc)
        goto fail;
    HIP_TRY(hipStreamSynchronize(s));
    if (rows[3] > 0) {
        HIP_TRY(hipEventElapsedTime(&fb_sym, scratch.ev[0], scratch.ev[1]));
        HIP_TRY(hipEventElapsedTime(&fb_num, scratch.ev[2], scratch.ev[3]));
    }
    g_sg_phase_ms[0] = t1 - t0;
    g_sg_phase_ms[1] = t2 - t1;
    g_sg_phase_ms[2] = csr_now_ms() - t2;
    g_sg_phase_ms[3] = (double)fb_sym + (double)fb_num;
    if (info) {
        info->products = (int64_t)h[SG_PRODUCTS];
        info->widest = (int64_t)h[SG_WIDEST];
        for (int c = 0; c < SPGEMM_CLASSES; ++c)
            info->rows_in_bin[c] = rows[c];
        info->nz = (int)nz;
    }
    *out = Cm;
    return 0;
fail: /* nothing of ours is left running when the scratch is freed */
    (void)hipStreamSynchronize(s);
    spmv_csr_release(Cm); /* NULL: ignored */
    return rc;
}
