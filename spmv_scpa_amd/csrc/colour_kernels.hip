/*
 * colour_kernels.hip -- a deterministic distance-1 colouring of a square CSR
 * handle, B = P A Q^T as a new handle, and the permutation of interleaved
 * vector blocks (spmv_csr_colour, spmv_csr_permute, spmv_permute_vectors;
 * spmv_engine.h), gfx950 (wave64).
 *
 * COLOURING (blocks; colour, new_of_old and the info are functions of the
 * pattern and the seed alone):
 *   csr_transpose_dev(pattern of A)   the rows of A^T: row i of A and row i of
 *                  A^T together list every neighbour of i, whichever side
 *                  stores the edge.  The same call answers -EDOM for a column
 *                  outside [0, N), so the rounds never index past an array
 *   k_co_round     Jones-Plassmann, ONE launch and one 4-byte read-back per
 *                  round, one lane per row.  A round reads the colours of the
 *                  EARLIER launches from `in` and writes `out` (two arrays,
 *                  swapped by the host): a lane never reads a word a lane of
 *                  its own launch writes.  A row whose neighbours of higher
 *                  priority all have a colour in `in` takes the smallest
 *                  colour none of them has: one walk of the two rows per
 *                  window of 64 colours, a 64-bit mask, at most
 *                  ceil((deg + 1) / 64) windows because first-fit never
 *                  passes deg.  The count of rows a round coloured is summed
 *                  per wavefront and added with one integer atomic: a COUNT
 *                  does not depend on the order of arrival.  The host stops
 *                  at max_rounds: no device loop is unbounded
 *   k_co_max       the largest colour (one integer atomicMax per wavefront)
 *   csr_transpose_dev(M x colours, one entry per row at column colour[i])
 *                  its JA is the stable sort of the rows by colour, its IRP
 *                  the first position of every colour: the radix sort of
 *                  spmv_csr_transpose, as the plan order of the triangular
 *                  analysis
 *   k_co_invert    new_of_old[order[p]] = p
 * No POSITION comes from an atomic, and no workgroup waits for another.
 *
 * PERMUTATION of a handle: the two stable sorts of the contract are two
 * transpositions with a relabelling before each,
 *   A' = A with column c written as q[c]      (k_co_relabel)
 *   T  = A'^T      N x M, scratch: row q[c] lists its source rows ascending,
 *                  duplicates in source order
 *   T' = T with column r written as p[r]      (k_co_relabel, in place)
 *   B  = T'^T      row p[r] ascending by new column, stably
 * so with both arrays NULL B is (A^T)^T.  Values ride as raw bits through
 * both gathers.  k_co_perm_scatter / k_co_perm_verify check an array before
 * anything is allocated for B: the inverse is scattered and compared back; the
 * flag word is an atomicOr and decides no position.
 *
 * VECTORS: k_co_vectors, thread f of the grid moves element f of the M x k
 * block (row f / k, column f % k): the lanes of a wavefront cover the k
 * doubles of consecutive rows contiguously, so the side that is not gathered
 * is whole cache lines, whatever k and the leading dimensions.
 */
#include <string.h>
#include <vector>

#include "csr_build.h"

#define CO_T 256 /* lanes of a workgroup */

static_assert(CO_T % WAVE == 0, "k_co_round, k_co_max: whole wavefronts");

/* the finaliser of murmur3: a bijection of the 32-bit words */
__device__ __forceinline__ uint32_t co_fmix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}

/* ------------------------------------------------------------------ */
/* colouring                                                            */
/* ------------------------------------------------------------------ */

__global__ void __launch_bounds__(CO_T)
k_co_iota(int n, int *__restrict__ iota) {
    const int64_t i = (int64_t)blockIdx.x * CO_T + threadIdx.x;
    if (i < n)
        iota[i] = (int)i;
}

/* One walk of a row for window [lo, lo + 64): *mask |= the colours of the
 * neighbours of higher priority; false as soon as one of them has no colour
 * in `in`.  Every column is inside [0, M): csr_transpose_dev checked A's, and
 * the columns of A^T are rows of A. */
__device__ __forceinline__ bool
co_walk(const int *__restrict__ ja, int64_t beg, int64_t end, int i,
        uint32_t hi, uint32_t seed, int lo, const int *__restrict__ in,
        unsigned long long *mask) {
    for (int64_t e = beg; e < end; ++e) {
        const int j = ja[e];
        if (j == i || co_fmix32((uint32_t)j ^ seed) < hi)
            continue; /* the diagonal is no edge; h is a bijection: no ties */
        const int cj = in[j];
        if (cj < 0)
            return false;
        const unsigned d = (unsigned)(cj - lo);
        if (d < 64u)
            *mask |= 1ull << d;
    }
    return true;
}

/* in / out: the colour of every row, -1 = none yet.  count += the rows this
 * launch coloured; *clear = 0 is the counter of the next launch */
__global__ void __launch_bounds__(CO_T)
k_co_round(int M, uint32_t seed, const int *__restrict__ irp,
           const int *__restrict__ ja, const int *__restrict__ tirp,
           const int *__restrict__ tja, const int *__restrict__ in,
           int *__restrict__ out, int *__restrict__ count,
           int *__restrict__ clear) {
    const int64_t t = (int64_t)blockIdx.x * CO_T + threadIdx.x;
    if (t == 0)
        *clear = 0;
    bool fresh = false;
    if (t < M) {
        const int i = (int)t;
        int colour = in[i];
        if (colour < 0) {
            const uint32_t hi = co_fmix32((uint32_t)i ^ seed);
            const int64_t b0 = irp[i], e0 = irp[i + 1];
            const int64_t b1 = tirp[i], e1 = tirp[i + 1];
            /* first-fit never passes deg: windows >= 1 of them suffice */
            const int64_t windows = ((e0 - b0) + (e1 - b1) + 1 + 63) / 64;
            for (int64_t w = 0; w < windows; ++w) {
                unsigned long long mask = 0;
                const int lo = (int)(w * 64);
                if (!co_walk(ja, b0, e0, i, hi, seed, lo, in, &mask) ||
                    !co_walk(tja, b1, e1, i, hi, seed, lo, in, &mask))
                    break; /* a neighbour of higher priority is not coloured */
                if (~mask) {
                    colour = lo + __builtin_ctzll(~mask);
                    fresh = true;
                    break;
                }
            }
        }
        out[i] = colour;
    }
    const unsigned long long who = __ballot(fresh);
    if (who && (threadIdx.x & (WAVE - 1)) == (unsigned)__builtin_ctzll(who))
        atomicAdd(count, __popcll(who));
}

/* *maxc = max(*maxc, colour[i]) */
__global__ void __launch_bounds__(CO_T)
k_co_max(int M, const int *__restrict__ colour, int *__restrict__ maxc) {
    const int64_t first = (int64_t)blockIdx.x * CO_T + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * CO_T;
    int m = -1;
    for (int64_t i = first; i < M; i += stride)
        m = max(m, colour[i]);
#pragma unroll
    for (int d = WAVE / 2; d > 0; d >>= 1)
        m = max(m, __shfl_down(m, d, WAVE));
    if ((threadIdx.x & (WAVE - 1)) == 0 && m >= 0)
        atomicMax(maxc, m);
}

/* order: a permutation of 0 .. M-1 (the JA of a transposition) */
__global__ void __launch_bounds__(CO_T)
k_co_invert(int M, const int *__restrict__ order,
            int *__restrict__ new_of_old) {
    const int64_t p = (int64_t)blockIdx.x * CO_T + threadIdx.x;
    if (p >= M)
        return;
    const int r = order[p];
    if ((unsigned)r < (unsigned)M)
        new_of_old[r] = (int)p;
}

/* device scratch of one call: freed on every path */
struct co_scratch {
    std::vector<void *> blocks;
    ~co_scratch() {
        for (void *b : blocks)
            (void)hipFree(b);
    }
    /* at least one element, so that no pointer handed to a kernel is NULL */
    template <typename T> hipError_t get(T **out, int64_t count) {
        void *p = NULL;
        const hipError_t e =
            hipMalloc(&p, (size_t)(count > 0 ? count : 1) * sizeof(T));
        if (e == hipSuccess)
            blocks.push_back(p);
        *out = (T *)p;
        return e;
    }
};

/* a CSR view of arrays somebody else owns, for csr_transpose_dev */
static spmv_csr_dev co_view(int M, int N, int64_t NZ, int value_bytes,
                            int *irp, int *ja, void *values) {
    spmv_csr_dev v;
    memset(&v, 0, sizeof v);
    v.M = M;
    v.N = N;
    v.NZ = NZ;
    v.value_bytes = value_bytes;
    v.irp = irp;
    v.ja = ja;
    if (value_bytes == 4)
        v.as32 = (float *)values;
    else
        v.as = (double *)values;
    return v;
}

int csr_colour_dev(const spmv_csr_dev *A, uint32_t seed, int max_rounds,
                   int *d_colour, int *d_new_of_old, spmv_colour_info *info,
                   hipStream_t s) {
    int rc = 0;
    const int M = A->M;
    const int64_t NZ = A->NZ;
    co_scratch scratch;
    spmv_colour_info got = {0, 0, 0, 0};
    int *tirp = NULL, *tja = NULL, *ride = NULL, *buf[2] = {NULL, NULL},
        *counters = NULL, *iota = NULL, *cptr = NULL, *order = NULL;
    int rounds = 0, fresh = 0, maxc = -1;
    int64_t done = 0;
    std::vector<int> h_cptr;
    if (M == 0) {
        if (info)
            *info = got;
        return 0;
    }
    (void)hipGetLastError(); /* an earlier caller's unread error is not ours */
    /* the rows of A^T; the positions ride as 4-byte values nobody reads */
    HIP_TRY(scratch.get(&tirp, (int64_t)M + 1));
    HIP_TRY(scratch.get(&tja, NZ));
    HIP_TRY(scratch.get(&ride, NZ > M ? NZ : M));
    {
        spmv_csr_dev S = co_view(M, M, NZ, 4, A->irp, A->ja, A->ja);
        spmv_csr_dev ST = co_view(M, M, NZ, 4, tirp, tja, ride);
        rc = csr_transpose_dev(&S, &ST, s); /* -EDOM: a column outside */
        if (rc)
            goto fail;
    }
    HIP_TRY(scratch.get(&buf[0], M));
    HIP_TRY(scratch.get(&buf[1], M));
    HIP_TRY(scratch.get(&counters, 4)); /* three round counters, the maximum */
    HIP_TRY(hipMemsetAsync(buf[0], 0xff, (size_t)M * sizeof(int), s));
    HIP_TRY(hipMemsetAsync(counters, 0, 3 * sizeof(int), s));
    HIP_TRY(hipMemsetAsync(counters + 3, 0xff, sizeof(int), s));
    /* Jones-Plassmann: one launch and one read-back per round */
    while (done < M) {
        if (rounds >= max_rounds) {
            rc = -E2BIG;
            goto fail;
        }
        hipLaunchKernelGGL(k_co_round, grid_for(M, CO_T), dim3(CO_T), 0, s, M,
                           seed, A->irp, A->ja, tirp, tja, buf[rounds & 1],
                           buf[(rounds + 1) & 1], counters + rounds % 3,
                           counters + (rounds + 1) % 3);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&fresh, counters + rounds % 3, sizeof(int),
                               hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        ++rounds;
        /* the uncoloured row of the highest priority always gets a colour */
        if (fresh <= 0 || fresh > M - done) {
            rc = -EIO;
            goto fail;
        }
        done += fresh;
    }
    {
        const int *colour = buf[rounds & 1];
        hipLaunchKernelGGL(k_co_max, dim3(1024), dim3(CO_T), 0, s, M, colour,
                           counters + 3);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&maxc, counters + 3, sizeof(int),
                               hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (maxc < 0 || maxc >= M) {
            rc = -EIO;
            goto fail;
        }
        got.colours = maxc + 1;
        got.rounds = rounds;
        /* the rows by (colour, row): the transpose of the M x colours matrix
         * with row i's one entry at column colour[i] */
        HIP_TRY(scratch.get(&iota, (int64_t)M + 1));
        HIP_TRY(scratch.get(&cptr, (int64_t)got.colours + 1));
        HIP_TRY(scratch.get(&order, M));
        hipLaunchKernelGGL(k_co_iota, grid_for((int64_t)M + 1, CO_T),
                           dim3(CO_T), 0, s, M + 1, iota);
        HIP_TRY(hipGetLastError());
        spmv_csr_dev L = co_view(M, got.colours, M, 4, iota, (int *)colour,
                                 buf[(rounds + 1) & 1]);
        spmv_csr_dev LT = co_view(got.colours, M, M, 4, cptr, order, ride);
        rc = csr_transpose_dev(&L, &LT, s);
        if (rc)
            goto fail;
        h_cptr.resize((size_t)got.colours + 1);
        HIP_TRY(hipMemcpyAsync(h_cptr.data(), cptr,
                               h_cptr.size() * sizeof(int),
                               hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (h_cptr[0] != 0 || h_cptr[got.colours] != M) {
            rc = -EIO;
            goto fail;
        }
        got.narrowest = M;
        for (int c = 0; c < got.colours; ++c) {
            const int n = h_cptr[c + 1] - h_cptr[c];
            got.widest = n > got.widest ? n : got.widest;
            got.narrowest = n < got.narrowest ? n : got.narrowest;
        }
        /* the caller's arrays last: an error above leaves them untouched */
        if (d_colour)
            HIP_TRY(hipMemcpyAsync(d_colour, colour, (size_t)M * sizeof(int),
                                   hipMemcpyDeviceToDevice, s));
        if (d_new_of_old) {
            hipLaunchKernelGGL(k_co_invert, grid_for(M, CO_T), dim3(CO_T), 0, s,
                               M, order, d_new_of_old);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipStreamSynchronize(s));
    }
    if (info)
        *info = got;
fail:
    if (rc) /* nothing of ours is left running when the scratch is freed */
        (void)hipStreamSynchronize(s);
    return rc;
}

/* ------------------------------------------------------------------ */
/* permutation of a handle                                              */
/* ------------------------------------------------------------------ */

/* inv[perm[i]] = i where perm[i] is inside [0, n); flag |= 1 where it is not.
 * Two equal entries both store: either may stay, k_co_perm_verify sees it */
__global__ void __launch_bounds__(CO_T)
k_co_perm_scatter(int n, const int *__restrict__ perm, int *__restrict__ inv,
                  unsigned *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * CO_T + threadIdx.x;
    if (i >= n)
        return;
    const int v = perm[i];
    if ((unsigned)v < (unsigned)n)
        inv[v] = (int)i;
    else
        atomicOr(flag, 1u);
}

/* flag |= 2 where the inverse does not lead back: a repeated entry */
__global__ void __launch_bounds__(CO_T)
k_co_perm_verify(int n, const int *__restrict__ perm,
                 const int *__restrict__ inv, unsigned *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * CO_T + threadIdx.x;
    if (i >= n)
        return;
    const int v = perm[i];
    if ((unsigned)v < (unsigned)n && inv[v] != (int)i)
        atomicOr(flag, 2u);
}

/* 0: perm is a permutation of 0 .. n-1; -EDOM: an entry outside; -EINVAL: a
 * repeated entry */
static int co_check_perm(const int *perm, int n, hipStream_t s) {
    int rc = 0;
    co_scratch scratch;
    int *inv = NULL;
    unsigned *d_flag = NULL, flag = 0;
    if (!perm || n == 0)
        return 0;
    HIP_TRY(scratch.get(&inv, n));
    HIP_TRY(scratch.get(&d_flag, 1));
    HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(unsigned), s));
    hipLaunchKernelGGL(k_co_perm_scatter, grid_for(n, CO_T), dim3(CO_T), 0, s,
                       n, perm, inv, d_flag);
    hipLaunchKernelGGL(k_co_perm_verify, grid_for(n, CO_T), dim3(CO_T), 0, s, n,
                       perm, inv, d_flag);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&flag, d_flag, sizeof(unsigned),
                           hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (flag & 1u)
        rc = -EDOM;
    else if (flag & 2u)
        rc = -EINVAL;
fail:
    if (rc)
        (void)hipStreamSynchronize(s);
    return rc;
}

/* dst[e] = map[src[e]]; an index outside [0, n) is passed on as it is, for
 * the transposition that follows to refuse (dst may be src) */
__global__ void __launch_bounds__(CO_T)
k_co_relabel(int64_t NZ, int n, const int *__restrict__ map, const int *src,
             int *dst) {
    const int64_t e = (int64_t)blockIdx.x * CO_T + threadIdx.x;
    if (e >= NZ)
        return;
    const int c = src[e];
    dst[e] = (unsigned)c < (unsigned)n ? map[c] : c;
}

int csr_permute_dev(const spmv_csr_dev *A, const int *p, const int *q,
                    spmv_csr_dev **out, hipStream_t s) {
    int rc = 0;
    const int M = A->M, N = A->N, vb = A->value_bytes;
    const int64_t NZ = A->NZ;
    co_scratch scratch;
    spmv_csr_dev *B = NULL;
    int *ja1 = NULL, *tirp = NULL, *tja = NULL;
    char *tval = NULL;
    void *aval = vb == 4 ? (void *)A->as32 : (void *)A->as;
    (void)hipGetLastError(); /* an earlier caller's unread error is not ours */
    rc = co_check_perm(p, M, s);
    if (rc)
        return rc;
    rc = co_check_perm(q, N, s);
    if (rc)
        return rc;
    HIP_TRY(scratch.get(&tirp, (int64_t)N + 1));
    HIP_TRY(scratch.get(&tja, NZ));
    HIP_TRY(scratch.get(&tval, NZ * vb));
    if (q && NZ > 0) {
        HIP_TRY(scratch.get(&ja1, NZ));
        hipLaunchKernelGGL(k_co_relabel, grid_for(NZ, CO_T), dim3(CO_T), 0, s,
                           NZ, N, q, A->ja, ja1);
        HIP_TRY(hipGetLastError());
    }
    {
        spmv_csr_dev A1 = co_view(M, N, NZ, vb, A->irp, ja1 ? ja1 : A->ja, aval);
        spmv_csr_dev T = co_view(N, M, NZ, vb, tirp, tja, tval);
        rc = csr_transpose_dev(&A1, &T, s); /* -EDOM: a column outside */
        if (rc)
            goto fail;
        if (p && NZ > 0) { /* T's columns are rows of A: all inside [0, M) */
            hipLaunchKernelGGL(k_co_relabel, grid_for(NZ, CO_T), dim3(CO_T), 0,
                               s, NZ, M, p, tja, tja);
            HIP_TRY(hipGetLastError());
        }
        rc = csr_alloc_dev(M, N, NZ, vb, &B);
        if (rc)
            goto fail;
        rc = csr_transpose_dev(&T, B, s);
        if (rc)
            goto fail;
    }
    *out = B;
    return 0;
fail:
    (void)hipStreamSynchronize(s);
    spmv_csr_release(B); /* NULL: ignored */
    return rc;
}

/* ------------------------------------------------------------------ */
/* permutation of interleaved vectors                                   */
/* ------------------------------------------------------------------ */

template <bool INVERSE>
__global__ void __launch_bounds__(CO_T)
k_co_vectors(int64_t total, int k, const int *__restrict__ p,
             const double *__restrict__ in, int64_t ldin,
             double *__restrict__ out, int64_t ldout) {
    const int64_t f = (int64_t)blockIdx.x * CO_T + threadIdx.x;
    if (f >= total)
        return;
    const int64_t r = f / k;
    const int j = (int)(f - r * k);
    const int64_t pr = p[r];
    /* the bits are moved: a load and a store, no arithmetic */
    if (INVERSE)
        out[r * ldout + j] = in[pr * ldin + j];
    else
        out[pr * ldout + j] = in[r * ldin + j];
}

/* the arguments were checked by the caller; M > 0 */
int permute_vectors_dev(const int *p, int M, int k, int inverse,
                        const double *in, int64_t ldin, double *out,
                        int64_t ldout, hipStream_t s) {
    const int64_t total = (int64_t)M * k;
    if (inverse)
        hipLaunchKernelGGL((k_co_vectors<true>), grid_for(total, CO_T),
                           dim3(CO_T), 0, s, total, k, p, in, ldin, out, ldout);
    else
        hipLaunchKernelGGL((k_co_vectors<false>), grid_for(total, CO_T),
                           dim3(CO_T), 0, s, total, k, p, in, ldin, out, ldout);
    return hip_errno(hipGetLastError());
}
