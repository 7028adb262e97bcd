/*
 * engine.hip -- device management, matrix upload / generation / conversion,
 * launch dispatch, event timing and the one-shot C-ABI entry points
 * (API: include/spmv_engine.h, hip_csr.h, hip_hll.h).
 *
 * Everything here is host code around the kernels of csr_kernels.hip and
 * hll_kernels.hip.  There is no CPU fallback: without a usable GPU every
 * entry point returns -ENODEV.
 */
#include <algorithm>
#include <cmath>
#include <functional>
#include <mutex>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <thread>
#include <time.h>
#include <unordered_map>
#include <vector>

#include "add_plan.h"
#include "amg_plan.h"
#include "csr_build.h"
#include "err.h"
#include "hip_common.h"
#include "hip_csr.h"
#include "hip_hll.h"
#include "mat_ref.h"
#include "spgemm_plan.h"
#include "spmv_synth.h"
#include "stream_table.h"
#include "transpose_plan.h"
#include "trsv_plan.h"
#include "tune_blocked.h"
#include "utils.h"

/* Process defaults behind set_*_waves_per_block (the reference's seam sets
 * them before every call).  0 = never set: the launch then picks by size --
 * 512-lane workgroups measured best on 10M-row matrices, 256-lane ones on
 * launches that last only a few workgroup lifetimes (1M x 16, flushed:
 * thread-per-row HLL 0.0383 vs 0.0435 ms, sub-wave CSR 0.0447 vs 0.0461; a
 * pure 192 MB stream likewise prefers many small workgroups,
 * profiles/r03_microbench_small.txt). */
int g_csr_waves = 0;
int g_hll_waves = 0;

static int default_waves(int user_default, long long rows) {
    return user_default > 0 ? user_default : rows < 2000000 ? 4 : 8;
}

/*
 * Live handles.  spmv_csr_release / spmv_hll_release free host memory
 * (free(d), the blocked copy's descriptor): a binding that released a handle
 * twice -- an explicit release() followed by a finaliser, two wrappers around
 * one handle, a finaliser running after an atexit sweep -- would corrupt the
 * host heap.  Every handle is therefore entered here when it is created,
 * together with a process-wide GENERATION number (1, 2, 3 ... never reused),
 * and
 *   - every public entry point that takes a handle checks it first (-EBADF for
 *     a pointer that is not, or no longer, a live handle -- before anything is
 *     allocated or dereferenced);
 *   - a release of anything that is not in the set is ignored AND COUNTED
 *     (spmv_ignored_releases(); one line on stderr per ignored release after
 *     spmv_set_debug(1)), so a double release stays visible;
 *   - spmv_*_release_checked(h, generation) releases only when the live handle
 *     at that address still carries the generation the caller was given at
 *     creation (spmv_handle_generation): a stale wrapper cannot release a NEW
 *     handle that calloc happened to place at the old address.  Bindings with
 *     finalisers (the Python one) use this form.
 * The set and its mutex are heap objects that are never destroyed, so a
 * release that arrives during static destruction still finds them.
 */
struct live_set {
    std::mutex mu;
    std::unordered_map<const void *, uint64_t> handles; /* -> generation */
    uint64_t next_gen = 1;
    long ignored = 0;
    int debug = 0;
};
static live_set &live(void) {
    static live_set *s = new live_set();
    return *s;
}
static void live_add(const void *h) {
    std::lock_guard<std::mutex> g(live().mu);
    live().handles[h] = live().next_gen++;
}
static void live_ignored(const void *h, const char *why) {
    /* caller holds the mutex */
    ++live().ignored;
    if (live().debug)
        fprintf(stderr, "spmv_scpa_amd: release of %p ignored (%s)\n", h, why);
}
/* true exactly once per handle: the caller then owns the teardown.  gen != 0:
 * only when the live handle at this address has that generation */
static bool live_take(const void *h, uint64_t gen = 0) {
    std::lock_guard<std::mutex> g(live().mu);
    auto it = live().handles.find(h);
    if (it == live().handles.end()) {
        live_ignored(h, "not a live handle: released before, or never one");
        return false;
    }
    if (gen && it->second != gen) {
        live_ignored(h, "stale generation: the address now holds a newer handle");
        return false;
    }
    live().handles.erase(it);
    return true;
}
static bool live_has(const void *h) {
    std::lock_guard<std::mutex> g(live().mu);
    return live().handles.count(h) == 1;
}
/* first statement of every public entry point that takes a handle */
#define HANDLE_OK(h)                                                          \
    do {                                                                      \
        if (!(h))                                                             \
            return -EINVAL;                                                   \
        if (!live_has(h))                                                     \
            return -EBADF; /* released, or never a handle */                  \
    } while (0)

/* false after spmv_*_release_source(): what reads ja answers -ENODATA */
static bool has_source(const spmv_csr_dev *A) { return A->ja || A->NZ == 0; }
static bool has_source(const spmv_hll_dev *H) {
    return H->ja || H->off16 || H->slots == 0;
}

/* the blocked path as a candidate: tune_blocked.h with panels.hip's
 * operations (the same template runs under ASan with mock copies) */
struct panels_ops {
    static void free(spmv_panels *p) { panels_free(p); }
    static void set_chain(spmv_panels *p, int v) { panels_set_chain(p, v); }
    static void set_waves(spmv_panels *p, int v) { panels_set_waves(p, v); }
    static void set_order(spmv_panels *p, int v) { panels_set_order(p, v); }
    static int balanced_tile_rows(int M, int max_rows) {
        return panels_balanced_tile_rows(M, max_rows);
    }
    static const char *build_phases(void) { return panels_last_build_phases(); }
    static double now_s(void) {
        struct timespec t;
        clock_gettime(CLOCK_MONOTONIC, &t);
        return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
    }
};

/* what the selector did, kept in the handle (spmv_*_tune_log) */
struct tune_log {
    std::string text;
    void operator()(const char *line) {
        text += line;
        text += '\n';
    }
    char *release(void) const { return strdup(text.c_str()); }
};

extern "C" {

/* 0.3: spmv_panel_opts.bucket_order; 0.4: spmv_panel_opts.struct_size (first
 * field), spmv_*_release_checked, handle checks on every entry point;
 * 0.7: fp32-stored values (spmv_*_upload_f32, spmv_csr_to_f32,
 * spmv_*_value_bytes) */
const char *spmv_version(void) { return "spmv_scpa_amd 0.7 gfx950"; }

/* HIP_VERSION of the headers this library was compiled against, and of the
 * runtime it is bound to now (hipRuntimeGetVersion; needs no device).  The
 * binding compares them: a process that maps torch's bundled runtime runs
 * this library on THAT build of HIP (__init__.py). */
int spmv_hip_build_version(void) { return HIP_VERSION; }
int spmv_hip_runtime_version(void) {
    int v = 0;
    return hipRuntimeGetVersion(&v) == hipSuccess ? v : -EIO;
}

/* "product", or "ablations" for a -DSPMV_ABLATIONS build (make abl): only
 * that flavour understands the experiment bits of spmv_launch_opts.variant */
const char *spmv_build_flavour(void) {
#ifdef SPMV_ABLATIONS
    return "ablations";
#else
    return "product";
#endif
}

int spmv_live_handles(void) {
    std::lock_guard<std::mutex> g(live().mu);
    return (int)live().handles.size();
}

long spmv_ignored_releases(void) {
    std::lock_guard<std::mutex> g(live().mu);
    return live().ignored;
}

void spmv_set_debug(int on) {
    std::lock_guard<std::mutex> g(live().mu);
    live().debug = on ? 1 : 0;
}

uint64_t spmv_handle_generation(const void *handle) {
    std::lock_guard<std::mutex> g(live().mu);
    auto it = live().handles.find(handle);
    return it == live().handles.end() ? 0 : it->second;
}

/*
 * TEST HOOK: overwrite every last-arriver counter of the handle (the long
 * rows of the CSR kernels / the wide hack blocks of the HLL kernels / the long
 * rows beside a blocked copy) with what an INCOMPLETE launch leaves behind:
 * a foreign launch number and a count.  The next launches must not care
 * (epoch_arrive, hip_common.h).  Returns the counters touched, < 0 on error.
 */
static int stale_arrivals(unsigned long long *cnt, int n, spmv_panels *P) {
    if (cnt && n > 0)
        HIP_RET(hipMemset(cnt, 0x01, (size_t)n * sizeof(unsigned long long)));
    else
        n = 0;
    const int p = panels_debug_stale_arrivals(P);
    return p < 0 ? p : n + p;
}

int spmv_csr_debug_stale_arrivals(spmv_csr_dev *A) {
    HANDLE_OK(A);
    return stale_arrivals(A->seg_count, A->n_rowblk, A->panels);
}

int spmv_hll_debug_stale_arrivals(spmv_hll_dev *H) {
    HANDLE_OK(H);
    return stale_arrivals(H->wide_cnt, H->n_wide_seg, H->panels);
}

/* 1..16; 0 (or less) returns to the size-based default above */
void set_csr_waves_per_block(int waves) {
    g_csr_waves = waves < 1 ? 0 : (waves > 16 ? 16 : waves);
}

void set_hll_waves_per_block(int waves) {
    g_hll_waves = waves < 1 ? 0 : (waves > 16 ? 16 : waves);
}

/* ------------------------------------------------------------------ */
/* devices and raw memory                                               */
/* ------------------------------------------------------------------ */

int spmv_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
        return 0;
    return n;
}

int spmv_set_device(int device) {
    if (spmv_device_count() == 0)
        return -ENODEV;
    HIP_RET(hipSetDevice(device));
    return 0;
}

int spmv_get_device(void) {
    int d = 0;
    if (spmv_device_count() == 0)
        return -ENODEV;
    HIP_RET(hipGetDevice(&d));
    return d;
}

int spmv_device_info(int device, char *name, size_t len, int *compute_units,
                     size_t *hbm_bytes) {
    if (spmv_device_count() == 0)
        return -ENODEV;
    hipDeviceProp_t p;
    HIP_RET(hipGetDeviceProperties(&p, device));
    if (name && len)
        snprintf(name, len, "%s (%s)", p.name, p.gcnArchName);
    if (compute_units)
        *compute_units = p.multiProcessorCount;
    if (hbm_bytes)
        *hbm_bytes = p.totalGlobalMem;
    return 0;
}

/* "0000:c1:00.0": which physical card a rank drives (multi-GPU lines) */
int spmv_device_pci_bus_id(int device, char *buf, size_t len) {
    if (!buf || len < 16)
        return -EINVAL;
    if (spmv_device_count() == 0)
        return -ENODEV;
    HIP_RET(hipDeviceGetPCIBusId(buf, (int)len, device));
    return 0;
}

int spmv_dev_mem_info(size_t *free_bytes, size_t *total_bytes) {
    if (spmv_device_count() == 0)
        return -ENODEV;
    size_t f = 0, t = 0;
    HIP_RET(hipMemGetInfo(&f, &t));
    if (free_bytes)
        *free_bytes = f;
    if (total_bytes)
        *total_bytes = t;
    return 0;
}

int spmv_dev_malloc(void **dptr, size_t bytes) {
    if (!dptr)
        return -EINVAL;
    *dptr = NULL;
    if (spmv_device_count() == 0)
        return -ENODEV;
    HIP_RET(hipMalloc(dptr, bytes ? bytes : 16));
    return 0;
}

int spmv_dev_free(void *dptr) {
    if (!dptr)
        return 0;
    HIP_RET(hipFree(dptr));
    return 0;
}

int spmv_dev_memset(void *dptr, int byte, size_t bytes, void *stream) {
    HIP_RET(hipMemsetAsync(dptr, byte, bytes, (hipStream_t)stream));
    return 0;
}

int spmv_copy_h2d(void *dst, const void *src, size_t bytes) {
    if (bytes == 0)
        return 0;
    HIP_RET(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return 0;
}

int spmv_copy_d2h(void *dst, const void *src, size_t bytes) {
    if (bytes == 0)
        return 0;
    HIP_RET(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return 0;
}

int spmv_stream_sync(void *stream) {
    HIP_RET(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

int spmv_device_sync(void) {
    HIP_RET(hipDeviceSynchronize());
    return 0;
}

/* the reference's GPU timer (cuda_timer.cu:15-21) as plain handles: an event
 * pair recorded on the launch stream around whatever the caller enqueues */
int spmv_event_create(void **ev) {
    if (!ev)
        return -EINVAL;
    hipEvent_t e = NULL;
    HIP_RET(hipEventCreate(&e));
    *ev = (void *)e;
    return 0;
}

int spmv_event_record(void *ev, void *stream) {
    if (!ev)
        return -EINVAL;
    HIP_RET(hipEventRecord((hipEvent_t)ev, (hipStream_t)stream));
    return 0;
}

int spmv_event_elapsed_ms(void *start, void *stop, float *ms) {
    if (!start || !stop || !ms)
        return -EINVAL;
    HIP_RET(hipEventSynchronize((hipEvent_t)stop));
    HIP_RET(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
    return 0;
}

int spmv_event_destroy(void *ev) {
    if (ev)
        HIP_RET(hipEventDestroy((hipEvent_t)ev));
    return 0;
}

/* ---- streams and hipGraph capture of stream-ordered launches ---- */
int spmv_stream_create(void **stream) {
    if (!stream)
        return -EINVAL;
    hipStream_t s = NULL;
    HIP_RET(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = (void *)s;
    return 0;
}

int spmv_stream_destroy(void *stream) {
    if (stream)
        HIP_RET(hipStreamDestroy((hipStream_t)stream));
    return 0;
}

int spmv_graph_begin_capture(void *stream) {
    if (!stream)
        return -EINVAL; /* the legacy default stream cannot be captured */
    HIP_RET(hipStreamBeginCapture((hipStream_t)stream,
                                  hipStreamCaptureModeThreadLocal));
    return 0;
}

int spmv_graph_end_capture(void *stream, void **graph_exec) {
    if (!stream || !graph_exec)
        return -EINVAL;
    hipGraph_t g = NULL;
    hipGraphExec_t e = NULL;
    HIP_RET(hipStreamEndCapture((hipStream_t)stream, &g));
    hipError_t err = hipGraphInstantiate(&e, g, NULL, NULL, 0);
    (void)hipGraphDestroy(g);
    if (err != hipSuccess)
        return hip_errno(err);
    *graph_exec = (void *)e;
    return 0;
}

/* ... and the topology of what was captured: a single chain of n nodes has
 * n - 1 edges, one root and a largest fan-out of 1 (0 for n <= 1) */
int spmv_graph_end_capture_shape(void *stream, void **graph_exec, int *nodes,
                                 int *edges, int *roots, int *max_fanout) {
    if (!stream || !graph_exec)
        return -EINVAL;
    hipGraph_t g = NULL;
    hipGraphExec_t e = NULL;
    HIP_RET(hipStreamEndCapture((hipStream_t)stream, &g));
    size_t nn = 0, ne = 0, nr = 0;
    int fan = 0;
    hipError_t err = hipGraphGetNodes(g, NULL, &nn);
    if (err == hipSuccess)
        err = hipGraphGetEdges(g, NULL, NULL, &ne);
    if (err == hipSuccess)
        err = hipGraphGetRootNodes(g, NULL, &nr);
    if (err == hipSuccess && ne > 0) {
        std::vector<hipGraphNode_t> from(ne), to(ne);
        err = hipGraphGetEdges(g, from.data(), to.data(), &ne);
        if (err == hipSuccess) {
            std::unordered_map<hipGraphNode_t, int> out;
            for (size_t i = 0; i < ne; ++i)
                fan = std::max(fan, ++out[from[i]]);
        }
    }
    if (err == hipSuccess)
        err = hipGraphInstantiate(&e, g, NULL, NULL, 0);
    (void)hipGraphDestroy(g);
    if (err != hipSuccess)
        return hip_errno(err);
    if (nodes)
        *nodes = (int)nn;
    if (edges)
        *edges = (int)ne;
    if (roots)
        *roots = (int)nr;
    if (max_fanout)
        *max_fanout = fan;
    *graph_exec = (void *)e;
    return 0;
}

int spmv_graph_launch(void *graph_exec, void *stream) {
    if (!graph_exec)
        return -EINVAL;
    HIP_RET(hipGraphLaunch((hipGraphExec_t)graph_exec, (hipStream_t)stream));
    return 0;
}

int spmv_graph_destroy(void *graph_exec) {
    if (graph_exec)
        HIP_RET(hipGraphExecDestroy((hipGraphExec_t)graph_exec));
    return 0;
}

} /* extern "C" */

/* ------------------------------------------------------------------ */
/* device-side synthetic generation (include/spmv_synth.h)              */
/* ------------------------------------------------------------------ */

__global__ void k_fill_x(double *x, int64_t n, uint64_t seed, int64_t first) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        x[i] = synth_x(seed, first + i);
}

__global__ void k_synth_lens(synth_spec s, int *lens) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < s.M)
        lens[i] = synth_row_len(&s, s.row0 + i);
}

/* Rows of the power-law family and the hub row draw every column on its own
 * (synth_col_strat: stratified, ascending by construction), so a long one
 * can be filled by many lanes instead of one walking 10^5..10^8 entries (a
 * hub row of 131 072 entries was 79 ms of generation, one of 2.7e8 three
 * minutes) -- the same functions per entry, the same matrix. */
#define SYNTH_PARALLEL_ROW 4096
__host__ __device__ static inline bool synth_row_is_parallel(const synth_spec *s,
                                                             int64_t g, int len) {
    return len > SYNTH_PARALLEL_ROW &&
           (s->kind == SYNTH_POWERLAW ||
            (s->kind == SYNTH_HUB && g == synth_hub_row(s)));
}

/*
 * One lane per row, one workgroup per SYNTH_WG consecutive rows -- whose
 * entries are ONE contiguous range of JA / AS.  The range is generated in
 * LDS, every row at its final position relative to the range start (a padding
 * word per 32 -- SYNTH_AT -- keeps lanes that walk rows of 32 entries out of
 * each other's bank; the insertion sort of the random families runs there),
 * and then written out by the whole workgroup with consecutive lanes on
 * consecutive entries.  Round 4 let every lane write its own row straight to
 * HBM: 64 lanes x 4-byte stores to 64 different lines per instruction --
 * 130 GB of write traffic for a 3.84 GB matrix, 36 ms
 * (profiles/r04_wn_hll_tile_panels.md).  A range that does not fit the LDS
 * budget (`cap` entries: long rows among the 128) falls back to direct
 * stores; the same functions per entry either way, the same matrix.
 */
#define SYNTH_WG 128
#define SYNTH_SKEW 5
__global__ void __launch_bounds__(SYNTH_WG)
    k_synth_rows(synth_spec s, const int *__restrict__ irp, int *ja, double *as,
                 int cap) {
    extern __shared__ double synth_lds[];
    const int r0 = blockIdx.x * SYNTH_WG;
    const int r1 = min(r0 + SYNTH_WG, s.M);
    const int i = r0 + (int)threadIdx.x;
    const int beg0 = irp[r0];
    const int total = irp[r1] - beg0;
    int beg = 0, len = 0;
    bool mine = false;
    if (i < r1) {
        beg = irp[i];
        len = irp[i + 1] - beg;
        mine = !synth_row_is_parallel(&s, s.row0 + i, len); /* k_synth_long_rows */
    }
    /* A row left to k_synth_long_rows (longer than SYNTH_PARALLEL_ROW = 4096
     * entries, which can be BELOW cap: up to 12288) would leave its part of
     * the staged range unwritten, and the write-out loop would copy that
     * uninitialised LDS to ja / as -- harmless only as long as
     * k_synth_long_rows runs later on the same stream and overwrites it
     * (ADVICE r05).  No such ordering dependency: a workgroup that holds such
     * a row is not staged. */
    const int skipped = __syncthreads_or(i < r1 && !mine);
    if (total > cap || skipped) { /* workgroup-uniform: direct stores */
        if (mine)
            synth_fill_row(&s, s.row0 + i, len, ja + beg, as + beg);
        return;
    }
    double *vals = synth_lds;
    int *cols = (int *)(synth_lds + SYNTH_AT(cap, SYNTH_SKEW) + 1);
    if (mine)
        synth_fill_row_at(&s, s.row0 + i, len, cols, vals, beg - beg0,
                          SYNTH_SKEW);
    __syncthreads();
    /* every row of the range was generated above (none left to
     * k_synth_long_rows in a staged workgroup) */
    for (int p = (int)threadIdx.x; p < total; p += SYNTH_WG) {
        ja[beg0 + p] = cols[SYNTH_AT(p, SYNTH_SKEW)];
        as[beg0 + p] = vals[SYNTH_AT(p, SYNTH_SKEW)];
    }
}

/* grid (long rows, chunks): the workgroups of a row stride over its entries */
__global__ void k_synth_long_rows(synth_spec s, const int *irp,
                                  const int *rows, int *ja, double *as) {
    const int i = rows[blockIdx.x];
    const int64_t g = s.row0 + i;
    const int beg = irp[i], len = irp[i + 1] - beg;
    int64_t lo = 0, hi = s.N;
    if (s.kind != SYNTH_HUB)
        synth_window(&s, g, &lo, &hi);
    int *cols = ja + beg;
    double *vals = as + beg;
    for (int64_t j = (int64_t)blockIdx.y * blockDim.x + threadIdx.x; j < len;
         j += (int64_t)gridDim.y * blockDim.x) {
        cols[j] = synth_col_strat(&s, g, (int)j, len, lo, hi);
        vals[j] = synth_val(&s, g, (int)j);
    }
}

/* CSR -> HLL on the device: per-block width, then slot fill */
__global__ void k_block_width(int M, const int *irp, int *width) {
    int row = blockIdx.x * blockDim.x + threadIdx.x;
    int len = row < M ? irp[row + 1] - irp[row] : 0;
#pragma unroll
    for (int d = 16; d > 0; d >>= 1)
        len = max(len, __shfl_down(len, d, 32));
    if ((threadIdx.x & 31) == 0 && row < M)
        width[row / 32] = len;
}

/* a hack block is as wide as its longest row: with one lane per row the 32
 * lanes of a hub block walk 10^5..10^8 slots each (93 ms of a 1M-row
 * conversion).  Blocks beyond HLL_FILL_WIDE columns are filled a lane per
 * SLOT instead (grid: wide blocks x chunks) -- same slots, same pad rule */
#define HLL_FILL_WIDE 2048
template <typename V>
__global__ void k_hll_fill_wide(int M, int col_major, const int *wide_blocks,
                                const int *irp, const int *cja,
                                const V *cas, const int64_t *off, int *ja,
                                V *as, unsigned *padmask) {
    const int b = wide_blocks[blockIdx.x];
    const int rows = min(32, M - b * 32);
    const int64_t o = off[b];
    const int64_t n = off[b + 1] - o;
    const int w = (int)(n / rows);
    for (int64_t q = (int64_t)blockIdx.y * blockDim.x + threadIdx.x; q < n;
         q += (int64_t)gridDim.y * blockDim.x) {
        const int i = col_major ? (int)(q % rows) : (int)(q / w);
        const int j = col_major ? (int)(q / rows) : (int)(q % w);
        const int beg = irp[b * 32 + i], len = irp[b * 32 + i + 1] - beg;
        const int64_t t = o + q;
        if (j < len) {
            ja[t] = cja[beg + j];
            as[t] = cas[beg + j];
        } else { /* pad -> the row's last valid column, or 0 (hip_hll.h) */
            ja[t] = len > 0 ? cja[beg + len - 1] : 0;
            as[t] = V(0);
            atomicOr(padmask + (t >> 5), 1u << (t & 31));
        }
    }
}

/*
 * HLL_FILL_BLOCKS hack blocks (128 rows) per workgroup.  Their CSR entries
 * are one contiguous range of cja / cas: it is staged in LDS with whole-line
 * loads (skewed a word per 32 so that lanes reading 32 different rows'
 * j-th entries do not meet in one bank), then the workgroup walks the SLOTS
 * of its blocks, consecutive lanes on consecutive slots in either layout --
 * whole-line stores -- taking each slot's entry out of LDS.  Round 4's lane
 * per row read cja / cas with a stride of the row length: 65.9 GB read to
 * write 3.84 GB (profiles/r04_wn_hll_tile_panels.md).  A group whose entries
 * exceed the LDS budget reads them from global memory instead (same slot
 * walk); blocks wider than HLL_FILL_WIDE are k_hll_fill_wide's.  The pad
 * bits of 64 consecutive slots are OR-ed in with at most three atomics per
 * wavefront.
 */
#define HLL_FILL_BLOCKS 4
#define HLL_FILL_SKEW 5
template <typename V>
__global__ void __launch_bounds__(256)
    k_hll_fill(int M, int nb, int col_major, const int *__restrict__ irp,
               const int *__restrict__ cja, const V *__restrict__ cas,
               const int64_t *__restrict__ off, int *ja, V *as,
               unsigned *padmask, int cap) {
    extern __shared__ double fill_lds[];
    __shared__ int s_irp[HLL_FILL_BLOCKS * 32 + 1];
    const int b0 = blockIdx.x * HLL_FILL_BLOCKS;
    const int b1 = min(b0 + HLL_FILL_BLOCKS, nb);
    const int r0 = b0 * 32, r1 = min(b1 * 32, M);
    for (int k = (int)threadIdx.x; k <= r1 - r0; k += 256)
        s_irp[k] = irp[r0 + k];
    __syncthreads();
    const int beg0 = s_irp[0];
    const int total = s_irp[r1 - r0] - beg0;
    const bool staged = total <= cap;
    V *vals = (V *)fill_lds; /* the budget is sized for 8-byte values */
    int *cols = (int *)(fill_lds + SYNTH_AT(cap, HLL_FILL_SKEW) + 1);
    if (staged) {
        for (int p = (int)threadIdx.x; p < total; p += 256) {
            cols[SYNTH_AT(p, HLL_FILL_SKEW)] = cja[beg0 + p];
            vals[SYNTH_AT(p, HLL_FILL_SKEW)] = cas[beg0 + p];
        }
        __syncthreads();
    }
    const int lane = (int)threadIdx.x & 63;
    for (int b = b0; b < b1; ++b) {
        const int rows = min(32, M - b * 32);
        const int64_t o = off[b];
        const int64_t n = off[b + 1] - o;
        const int w = (int)(n / rows);
        if (w > HLL_FILL_WIDE)
            continue; /* k_hll_fill_wide */
        /* whole wavefronts enter every round: the pad ballot needs all lanes */
        for (int64_t q0 = 0; q0 < n; q0 += 256) {
            const int64_t q = q0 + (int64_t)threadIdx.x;
            bool pad = false;
            if (q < n) {
                const int i = col_major ? (int)(q % rows) : (int)(q / w);
                const int j = col_major ? (int)(q / rows) : (int)(q % w);
                const int rb = s_irp[(b - b0) * 32 + i] - beg0;
                const int len = s_irp[(b - b0) * 32 + i + 1] - beg0 - rb;
                /* pad -> the row's last valid column, or 0 (hip_hll.h) */
                pad = j >= len;
                const int p = rb + (pad ? len - 1 : j);
                int c = 0;
                V v = V(0);
                if (p >= rb) { /* len > 0 */
                    c = staged ? cols[SYNTH_AT(p, HLL_FILL_SKEW)] : cja[beg0 + p];
                    if (!pad)
                        v = staged ? vals[SYNTH_AT(p, HLL_FILL_SKEW)]
                                   : cas[beg0 + p];
                }
                ja[o + q] = c;
                as[o + q] = v;
            }
            const unsigned long long m = __ballot(pad);
            if (m) { /* slots t0 .. t0 + 63 of this wavefront: <= 3 words */
                const int64_t t0 = o + q0 + ((int64_t)threadIdx.x & ~63);
                const int sh = (int)(t0 & 31);
                unsigned word = 0;
                if (lane == 0)
                    word = (unsigned)(m << sh);
                else if (lane == 1)
                    word = (unsigned)(sh ? m >> (32 - sh) : m >> 32);
                else if (lane == 2)
                    word = sh ? (unsigned)(m >> (64 - sh)) : 0u;
                if (lane < 3 && word)
                    atomicOr(padmask + (t0 >> 5) + lane, word);
            }
        }
    }
}

/*
 * fp64 -> fp32 of a matrix's values: the C cast, i.e. IEEE round to nearest
 * even in the default rounding mode.  A value below FLT_MIN becomes an fp32
 * SUBNORMAL (gradual underflow: hipcc compiles gfx950 kernels with fp32
 * denormals on, .amdhsa_float_denorm_mode_32 = 3, so v_cvt_f32_f64 writes
 * them and the SpMV kernels' v_cvt_f64_f32 reads them back); NaN and +-inf
 * pass through.  A FINITE value that rounds to +-inf raises `*overflow` (an
 * ordinary global atomic): the caller answers -ERANGE.
 */
__global__ void k_narrow_f32(const double *__restrict__ src,
                             float *__restrict__ dst, size_t n,
                             unsigned *overflow) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    bool over = false;
    for (; i < n; i += stride) {
        const double v = src[i];
        const float f = (float)v;
        dst[i] = f;
        over |= isinf(f) && isfinite(v);
    }
    if (over)
        atomicOr(overflow, 1u);
}

/* the same conversion on the host (uploads); -ERANGE as above */
static int narrow_values(const double *src, size_t n, float *dst) {
    bool over = false;
    for (size_t i = 0; i < n; ++i) {
        const float f = (float)src[i];
        dst[i] = f;
        over |= std::isinf(f) && std::isfinite(src[i]);
    }
    return over ? -ERANGE : 0;
}

/* n host values into a handle's value array at entry `at`: as they are
 * (as64) or narrowed (as32) */
static int put_values(double *as64, float *as32, int64_t at, const double *src,
                      size_t n) {
    if (!n)
        return 0;
    if (as64) {
        HIP_RET(hipMemcpy(as64 + at, src, n * sizeof(double),
                          hipMemcpyHostToDevice));
        return 0;
    }
    float *tmp = (float *)malloc(n * sizeof(float));
    if (!tmp)
        return -ENOMEM;
    int rc = narrow_values(src, n, tmp);
    if (!rc)
        rc = hip_errno(hipMemcpy(as32 + at, tmp, n * sizeof(float),
                                 hipMemcpyHostToDevice));
    free(tmp);
    return rc;
}

/* scratch sweep used to push a small working set out of the Infinity Cache:
 * read-modify-write form (round 1 / 2; kept for A/B, variant bit 29) */
__global__ void k_flush(double *buf, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride)
        buf[i] = buf[i] * 1.0000001 + 1.0;
}

/* read-only form, the default since round 3: evicts just the same (reads
 * allocate in L2 and in the Infinity Cache) but leaves no DIRTY lines behind.
 * The read-modify-write flush left up to 256 MiB of dirty scratch in the
 * caches, and its write-back competed with the reads of the launch being
 * timed -- traffic that belongs to the flush, not to the SpMV: 1M x 16
 * banded, flushed, same run (gpurun r3c2): CSR stream 0.0433 ms after the RMW
 * flush / 0.0423 read-only / 0.0369 not flushed; thread-per-row HLL 0.0411 /
 * 0.0375 / 0.0337; sub-wave CSR 0.0546 / 0.0492 / 0.0479. */
__global__ void k_flush_ro(const double *buf, size_t n, double *sink) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    double acc = 0.0;
    for (; i < n; i += stride)
        acc += buf[i];
    if (acc == 1.2345e300) /* never: the buffer holds zeros */
        *sink = acc;
}

/* ------------------------------------------------------------------ */
/* row-block table of the CSR stream kernel (host, O(M))                */
/* ------------------------------------------------------------------ */
static int finish_csr_handle(spmv_csr_dev *d, const int *host_irp) {
    int rc = 0;
    std::vector<int> tab, ent;
    std::vector<unsigned char> mode;
    std::vector<int> tmp;
    bool segs = false;
    if (!host_irp) {
        tmp.resize((size_t)d->M + 1);
        HIP_TRY(hipMemcpy(tmp.data(), d->irp, ((size_t)d->M + 1) * sizeof(int),
                          hipMemcpyDeviceToHost));
        host_irp = tmp.data();
    }
    stream_table_build(host_irp, d->M, STREAM_NNZ, STREAM_ROWS, STREAM_ROW_T,
                       STREAM_LONG_ROW, STREAM_SEG, tab, ent, mode,
                       &d->max_row_len, &segs);
    {
        /* constant row length?  (O(M) over the host copy of IRP) */
        /* (IRP[r] = r * len is what the kernel then computes: only for an
         * IRP that starts at 0) */
        int len = d->M > 0 && host_irp[0] == 0 ? host_irp[1] - host_irp[0] : 0;
        for (int r = 1; r < d->M && len > 0; ++r)
            if (host_irp[r + 1] - host_irp[r] != len)
                len = 0;
        d->uniform_len = len;
    }
    d->n_rowblk = (int)tab.size() - 1;
    {
        /* (first row, first entry) per range: the kernel learns both with one
         * load instead of a load of the row and a dependent load of IRP */
        std::vector<int> tab2(tab.size() * 2);
        for (size_t k = 0; k < tab.size(); ++k) {
            tab2[2 * k] = tab[k];
            tab2[2 * k + 1] = ent[k];
        }
        HIP_TRY(hipMalloc((void **)&d->rowblk, tab2.size() * sizeof(int)));
        HIP_TRY(hipMemcpy(d->rowblk, tab2.data(), tab2.size() * sizeof(int),
                          hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMalloc((void **)&d->rowblk_mode, mode.size()));
    HIP_TRY(hipMemcpy(d->rowblk_mode, mode.data(), mode.size(),
                      hipMemcpyHostToDevice));
    {
        /* ranges holding (a segment of) one row of more than STREAM_NNZ
         * entries: what kernels 0-3 leave to k_csr_long_seg */
        std::vector<int> lrb;
        for (int k = 0; k < d->n_rowblk; ++k)
            if (mode[(size_t)k] == 2 || ent[(size_t)k + 1] - ent[(size_t)k] > STREAM_NNZ)
                lrb.push_back(k);
        d->n_long_rb = (int)lrb.size();
        if (!lrb.empty()) {
            HIP_TRY(hipMalloc((void **)&d->long_rb, lrb.size() * sizeof(int)));
            HIP_TRY(hipMemcpy(d->long_rb, lrb.data(), lrb.size() * sizeof(int),
                              hipMemcpyHostToDevice));
        }
    }
    if (segs) { /* partial sums + arrival counters of the long rows' ranges */
        const size_t n = (size_t)d->n_rowblk + 1;
        HIP_TRY(hipMalloc((void **)&d->seg_partial, n * sizeof(double)));
        HIP_TRY(hipMalloc((void **)&d->seg_count,
                          n * sizeof(unsigned long long)));
        HIP_TRY(hipMemset(d->seg_partial, 0, n * sizeof(double)));
        HIP_TRY(hipMemset(d->seg_count, 0, n * sizeof(unsigned long long)));
    }
fail:
    return rc;
}

int csr_alloc_dev(int M, int N, int64_t NZ, int value_bytes,
                  spmv_csr_dev **out) {
    int rc = 0;
    spmv_csr_dev *d = (spmv_csr_dev *)calloc(1, sizeof *d);
    if (!d)
        return -ENOMEM;
    live_add(d);
    d->M = M;
    d->N = N;
    d->NZ = NZ;
    d->value_bytes = value_bytes;
    /* workgroup orders before tuning (csr_kernels.hip): grouped runs for
     * matrices of >= 2M rows (banded 10M x 32: stream kernel 0.652 ms
     * grouped / 0.683 hardware, sub-wave 0.843 / 0.905 / 0.885 contiguous),
     * below: hardware order for the stream kernel (1M x 16: 0.0462 vs
     * 0.0471), contiguous ranges for the sub-wave kernel (0.0536 vs 0.0548) */
    d->order = M >= 2000000 ? 2 : 1;
    d->stream_grouped = M >= 2000000;
    HIP_TRY(hipGetDevice(&d->device));
    HIP_TRY(hipMalloc((void **)&d->irp, ((size_t)M + 1) * sizeof(int)));
    /* + slack: the stream kernel's 16-byte loads of the last range may read
     * up to 2048 + 3 entries past NZ (never used) */
    HIP_TRY(hipMalloc((void **)&d->ja, ((size_t)NZ + 2056) * sizeof(int)));
    if (value_bytes == 4) /* the slack holds for the fp32 array too */
        HIP_TRY(hipMalloc((void **)&d->as32, ((size_t)NZ + 2056) * sizeof(float)));
    else
        HIP_TRY(hipMalloc((void **)&d->as, ((size_t)NZ + 2056) * sizeof(double)));
    *out = d;
    return 0;
fail:
    spmv_csr_release(d);
    return rc;
}

/* The tail of every operation that makes a new handle on the device.  rc:
 * what making it answered; d: the handle, holding irp, ja and values when rc
 * is 0 (NULL when it was never allocated).  Finishes it and publishes it to
 * *out; on any failure it is released and *out is untouched */
static int publish_csr_handle(int rc, spmv_csr_dev *d, spmv_csr_dev **out) {
    if (!rc)
        rc = finish_csr_handle(d, NULL);
    if (rc) {
        spmv_csr_release(d); /* NULL: ignored */
        return rc;
    }
    *out = d;
    return 0;
}

/* the one body of spmv_csr_ic0 and spmv_csr_ilu0: `factor` is ic0_factor_dev
 * or ilu0_factor_dev, Info its record */
template <typename Info>
static int csr_factor(const spmv_csr_dev *A, double shift, int max_levels,
                      int (*factor)(const spmv_csr_dev *, double, int, int,
                                    spmv_csr_dev **, Info *, hipStream_t),
                      spmv_csr_dev **out, Info *info) {
    if (out)
        *out = NULL; /* on ANY error, the argument checks included */
    if (!A || !out || !(shift >= 0.0) || !std::isfinite(shift) ||
        max_levels < 0)
        return -EINVAL;
    if (spmv_device_count() == 0)
        return -ENODEV; /* no handle can be live: the more useful answer */
    HANDLE_OK(A);
    if (A->M != A->N)
        return -EINVAL;
    if (A->value_bytes != 8)
        return -ENOTSUP;
    if (!has_source(A))
        return -ENODATA; /* spmv_csr_release_source() */
    spmv_csr_dev *d = NULL;
    Info got;
    int rc = factor(A, shift, max_levels ? max_levels : TRSV_DEFAULT_MAX_LEVELS,
                    g_csr_waves, &d, &got, 0);
    rc = publish_csr_handle(rc, d, out);
    if (!rc && info)
        *info = got;
    return rc;
}

extern "C" {

int spmv_dev_fill_synth(double *d_x, int64_t n, uint64_t seed, int64_t first,
                        void *stream) {
    if (n <= 0)
        return 0;
    hipLaunchKernelGGL(k_fill_x, dim3((unsigned)((n + 255) / 256)), dim3(256),
                       0, (hipStream_t)stream, d_x, n, seed, first);
    return hip_errno(hipGetLastError());
}

/* ------------------------------------------------------------------ */
/* CSR handle                                                           */
/* ------------------------------------------------------------------ */

static void teardown(spmv_csr_dev *d) {
    (void)hipFree(d->irp);
    (void)hipFree(d->ja);
    (void)hipFree(d->as);
    (void)hipFree(d->as32);
    (void)hipFree(d->rowblk);
    (void)hipFree(d->rowblk_mode);
    (void)hipFree(d->seg_partial);
    (void)hipFree(d->seg_count);
    (void)hipFree(d->long_rb);
    panels_free(d->panels);
    free(d->tune_log);
    free(d);
}

static int csr_upload(const sparse_csr *A, int value_bytes, spmv_csr_dev **out) {
    if (!A || !out || A->M < 0 || A->NZ < 0)
        return -EINVAL;
    *out = NULL;
    if (spmv_device_count() == 0)
        return -ENODEV;
    spmv_csr_dev *d = NULL;
    int rc = csr_alloc_dev(A->M, A->N, A->NZ, value_bytes, &d);
    if (rc)
        return rc;
    HIP_TRY(hipMemcpy(d->irp, A->IRP, ((size_t)A->M + 1) * sizeof(int),
                      hipMemcpyHostToDevice));
    if (A->NZ > 0) {
        HIP_TRY(hipMemcpy(d->ja, A->JA, (size_t)A->NZ * sizeof(int),
                          hipMemcpyHostToDevice));
        rc = put_values(d->as, d->as32, 0, A->AS, (size_t)A->NZ);
        if (rc)
            goto fail;
    }
    rc = finish_csr_handle(d, A->IRP);
    if (rc)
        goto fail;
    *out = d;
    return 0;
fail:
    spmv_csr_release(d);
    return rc;
}

int spmv_csr_upload(const sparse_csr *A, spmv_csr_dev **out) {
    return csr_upload(A, 8, out);
}

int spmv_csr_upload_f32(const sparse_csr *A, spmv_csr_dev **out) {
    return csr_upload(A, 4, out);
}

/* a new handle with the pattern of A and its values narrowed on the device */
int spmv_csr_to_f32(const spmv_csr_dev *A, spmv_csr_dev **out) {
    if (!A || !out)
        return -EINVAL;
    *out = NULL;
    if (spmv_device_count() == 0)
        return -ENODEV; /* no handle can be live: the more useful answer */
    HANDLE_OK(A);
    if (A->value_bytes == 4)
        return -EINVAL;
    if (!has_source(A))
        return -ENODATA; /* spmv_csr_release_source() */
    spmv_csr_dev *d = NULL;
    unsigned *d_over = NULL, over = 0;
    int rc = csr_alloc_dev(A->M, A->N, A->NZ, 4, &d);
    if (rc)
        return rc;
    HIP_TRY(hipMemcpy(d->irp, A->irp, ((size_t)A->M + 1) * sizeof(int),
                      hipMemcpyDeviceToDevice));
    if (A->NZ > 0) {
        HIP_TRY(hipMemcpy(d->ja, A->ja, (size_t)A->NZ * sizeof(int),
                          hipMemcpyDeviceToDevice));
        HIP_TRY(hipMalloc((void **)&d_over, sizeof(unsigned)));
        HIP_TRY(hipMemset(d_over, 0, sizeof(unsigned)));
        hipLaunchKernelGGL(k_narrow_f32, dim3(4096), dim3(256), 0, 0, A->as,
                           d->as32, (size_t)A->NZ, d_over);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(&over, d_over, sizeof(unsigned),
                          hipMemcpyDeviceToHost));
        if (over)
            rc = -ERANGE;
    }
fail:
    (void)hipFree(d_over);
    return publish_csr_handle(rc, d, out);
}

/* the geometry a transposition of N columns and NZ entries would use
 * (transpose_plan.h); host arithmetic, no device needed */
int spmv_transpose_plan(int N, int64_t NZ, int *passes, int *digit_bits,
                        int *tile, int64_t *workgroups,
                        int64_t *scratch_bytes) {
    transpose_plan pl;
    int rc = transpose_plan_make(N, NZ, &pl);
    if (rc)
        return rc;
    if (passes)
        *passes = pl.passes;
    if (digit_bits)
        *digit_bits = pl.digit_bits;
    if (tile)
        *tile = pl.tile;
    if (workgroups)
        *workgroups = pl.workgroups;
    if (scratch_bytes)
        *scratch_bytes = pl.scratch_bytes;
    return 0;
}

/* a new N x M handle: A's entries in the stable order by column
 * (transpose_kernels.hip) */
int spmv_csr_transpose(const spmv_csr_dev *A, spmv_csr_dev **out) {
    if (!A || !out)
        return -EINVAL;
    *out = NULL;
    if (spmv_device_count() == 0)
        return -ENODEV; /* no handle can be live: the more useful answer */
    HANDLE_OK(A);
    if (!has_source(A))
        return -ENODATA; /* spmv_csr_release_source() */
    spmv_csr_dev *d = NULL;
    int rc = csr_alloc_dev(A->N, A->M, A->NZ, A->value_bytes, &d);
    if (rc)
        return rc;
    return publish_csr_handle(csr_transpose_dev(A, d, 0), d, out);
}

/* L of A ~ L L^T on A's lower triangle, a new M x M f64 handle
 * (ic0_kernels.hip) */
int spmv_csr_ic0(const spmv_csr_dev *A, double shift, int max_levels,
                 spmv_csr_dev **out, spmv_ic0_info *info) {
    return csr_factor(A, shift, max_levels, ic0_factor_dev, out, info);
}

/* L and U of A ~ L U on A's pattern, a new M x M f64 handle
 * (ilu0_kernels.hip) */
int spmv_csr_ilu0(const spmv_csr_dev *A, double shift, int max_levels,
                  spmv_csr_dev **out, spmv_ilu0_info *info) {
    return csr_factor(A, shift, max_levels, ilu0_factor_dev, out, info);
}

/* the constants of the sparse product (spgemm_plan.h); host arithmetic */
int spmv_spgemm_shape(int64_t *edges, int *tables, int *teams, int *lds_bytes,
                      int *fallback_batch, int64_t *fallback_bytes) {
    for (int c = 0; c < SPGEMM_CLASSES - 1; ++c) {
        if (edges)
            edges[c] = spgemm_edge(c);
        if (tables)
            tables[c] = spgemm_table(c);
        if (teams)
            teams[c] = spgemm_team(c);
        if (lds_bytes)
            lds_bytes[c] = spgemm_lds(c);
    }
    if (fallback_batch)
        *fallback_batch = SPGEMM_FALLBACK_MAX_BATCH;
    if (fallback_bytes)
        *fallback_bytes = SPGEMM_FALLBACK_BYTES;
    return 0;
}

void spmv_spgemm_last_phases(double ms[4]) {
    if (ms)
        csr_spgemm_last_phases(ms);
}

/* a new M x N f64 handle C = A B (spgemm_kernels.hip) */
int spmv_csr_spgemm(const spmv_csr_dev *A, const spmv_csr_dev *B,
                    spmv_csr_dev **out, spmv_spgemm_info *info) {
    if (out)
        *out = NULL; /* on ANY error, the argument checks included */
    if (!A || !B || !out)
        return -EINVAL;
    if (spmv_device_count() == 0)
        return -ENODEV; /* no handle can be live: the more useful answer */
    HANDLE_OK(A);
    HANDLE_OK(B);
    if (A->N != B->M)
        return -EINVAL;
    if (!has_source(A) || !has_source(B))
        return -ENODATA; /* spmv_csr_release_source() */
    spmv_csr_dev *d = NULL;
    spmv_spgemm_info got;
    int rc = csr_spgemm_dev(A, B, &d, &got, 0);
    rc = publish_csr_handle(rc, d, out);
    if (!rc && info)
        *info = got;
    return rc;
}

/* the constants of the sparse sum (add_plan.h); host arithmetic */
int spmv_add_shape(int64_t *edge, int *widths, int *n_widths, int *threads) {
    if (edge)
        *edge = ADD_EDGE;
    if (widths)
        for (int i = 0; i < ADD_WIDTHS; ++i)
            widths[i] = add_width(i);
    if (n_widths)
        *n_widths = ADD_WIDTHS;
    if (threads)
        *threads = ADD_THREADS;
    return 0;
}

/* MEASUREMENT (spmv_add_set_class): which class serves the rows of a sum */
static int g_add_class = 0;

int spmv_add_set_class(int mode) {
    const int was = g_add_class;
    if (mode < 0 || mode > 2)
        return -EINVAL;
    g_add_class = mode;
    return was;
}

void spmv_add_last_phases(double ms[3]) {
    if (ms)
        csr_add_last_phases(ms);
}

/* a new M x N f64 handle C = alpha A + beta B (add_kernels.hip) */
int spmv_csr_add(double alpha, const spmv_csr_dev *A, double beta,
                 const spmv_csr_dev *B, spmv_csr_dev **out,
                 spmv_add_info *info) {
    if (out)
        *out = NULL; /* on ANY error, the argument checks included */
    if (!A || !B || !out || !std::isfinite(alpha) || !std::isfinite(beta))
        return -EINVAL;
    if (spmv_device_count() == 0)
        return -ENODEV; /* no handle can be live: the more useful answer */
    HANDLE_OK(A);
    HANDLE_OK(B);
    if (A->M != B->M || A->N != B->N)
        return -EINVAL;
    if (!has_source(A) || !has_source(B))
        return -ENODATA; /* spmv_csr_release_source() */
    spmv_csr_dev *d = NULL;
    spmv_add_info got;
    int rc = csr_add_dev(alpha, A, beta, B, g_add_class, &d, &got, 0);
    const double t = csr_now_ms();
    rc = publish_csr_handle(rc, d, out);
    if (rc)
        return rc;
    csr_add_finish_ms(csr_now_ms() - t);
    if (info)
        *info = got;
    return 0;
}

/* a new M x M f64 handle with the one entry (i, i) = d_diag[i] per row */
int spmv_csr_from_diag(int M, const double *d_diag, spmv_csr_dev **out) {
    if (out)
        *out = NULL;
    if (!out || M < 0)
        return -EINVAL;
    if (spmv_device_count() == 0)
        return -ENODEV;
    spmv_csr_dev *d = NULL;
    int rc = csr_alloc_dev(M, M, M, 8, &d);
    if (rc)
        return rc;
    return publish_csr_handle(csr_from_diag_dev(d_diag, d, 0), d, out);
}

/* a new f64 handle with A's pattern and the values l_i a r_j */
int spmv_csr_scale(const spmv_csr_dev *A, const double *d_left,
                   const double *d_right, spmv_csr_dev **out) {
    if (out)
        *out = NULL;
    if (!A || !out || (!d_left && !d_right))
        return -EINVAL;
    if (spmv_device_count() == 0)
        return -ENODEV; /* no handle can be live: the more useful answer */
    HANDLE_OK(A);
    if (!has_source(A))
        return -ENODATA; /* spmv_csr_release_source() */
    spmv_csr_dev *d = NULL;
    int rc = csr_alloc_dev(A->M, A->N, A->NZ, 8, &d);
    if (rc)
        return rc;
    return publish_csr_handle(csr_scale_dev(A, d_left, d_right, d, 0), d, out);
}

/* PT (A P): the two products, the intermediate released */
int spmv_csr_galerkin(const spmv_csr_dev *A, const spmv_csr_dev *P,
                      const spmv_csr_dev *PT, spmv_csr_dev **out,
                      spmv_spgemm_info *info) {
    if (out)
        *out = NULL;
    if (!A || !P || !out)
        return -EINVAL;
    spmv_csr_dev *AP = NULL, *T = NULL;
    int rc = spmv_csr_spgemm(A, P, &AP, NULL);
    if (!rc && !PT) {
        rc = spmv_csr_transpose(P, &T);
        PT = T;
    }
    if (!rc)
        rc = spmv_csr_spgemm(PT, AP, out, info);
    spmv_csr_release(T); /* NULL: ignored */
    spmv_csr_release(AP);
    return rc;
}

/* 0: not symmetric, 1: the pattern is, 2: the stored values are too */
int spmv_csr_symmetry(const spmv_csr_dev *A, int *out) {
    if (!A || !out)
        return -EINVAL;
    *out = 0;
    if (spmv_device_count() == 0)
        return -ENODEV;
    HANDLE_OK(A);
    if (!has_source(A))
        return -ENODATA; /* spmv_csr_release_source() */
    if (A->M != A->N)
        return 0;
    spmv_csr_dev *T = NULL, *C = NULL;
    int pattern = 0, values = 0;
    int rc = spmv_csr_transpose(A, &T);
    if (!rc)
        rc = spmv_csr_transpose(T, &C);
    if (!rc)
        rc = csr_equal_dev(C, T, &pattern, &values, 0);
    spmv_csr_release(C); /* NULL: ignored */
    spmv_csr_release(T);
    if (rc)
        return rc;
    *out = values ? 2 : pattern ? 1 : 0;
    return 0;
}

/* ------------------------------------------------------------------ */
/* colouring and permutation (colour_kernels.hip)                       */
/* ------------------------------------------------------------------ */

#define COLOUR_DEFAULT_MAX_ROUNDS 4096

int spmv_csr_colour(const spmv_csr_dev *A, uint32_t seed, int max_rounds,
                    int *d_colour, int *d_new_of_old, spmv_colour_info *info) {
    if (!A || max_rounds < 0)
        return -EINVAL;
    if (spmv_device_count() == 0)
        return -ENODEV; /* no handle can be live: the more useful answer */
    HANDLE_OK(A);
    if (A->M != A->N)
        return -EINVAL;
    if (!has_source(A))
        return -ENODATA; /* spmv_csr_release_source() */
    return csr_colour_dev(A, seed,
                          max_rounds ? max_rounds : COLOUR_DEFAULT_MAX_ROUNDS,
                          d_colour, d_new_of_old, info, 0);
}

/* a new M x N handle B = P A Q^T: two relabelled transpositions */
int spmv_csr_permute(const spmv_csr_dev *A, const int *d_row_new_of_old,
                     const int *d_col_new_of_old, spmv_csr_dev **out) {
    if (!A || !out)
        return -EINVAL;
    *out = NULL;
    if (spmv_device_count() == 0)
        return -ENODEV; /* no handle can be live: the more useful answer */
    HANDLE_OK(A);
    if (!has_source(A))
        return -ENODATA; /* spmv_csr_release_source() */
    spmv_csr_dev *d = NULL;
    return publish_csr_handle(
        csr_permute_dev(A, d_row_new_of_old, d_col_new_of_old, &d, 0), d, out);
}

int spmv_permute_vectors(const int *d_new_of_old, int M, int k, int inverse,
                         const double *d_in, int64_t ldin, double *d_out,
                         int64_t ldout, void *stream) {
    if (k < 1 || k > 8 || M < 0)
        return -EINVAL;
    if (ldin == 0)
        ldin = k;
    if (ldout == 0)
        ldout = k;
    if (ldin < k || ldout < k || !d_in || !d_out || d_in == d_out ||
        !d_new_of_old)
        return -EINVAL;
    if (spmv_device_count() == 0)
        return -ENODEV;
    if (M == 0)
        return 0;
    return permute_vectors_dev(d_new_of_old, M, k, inverse != 0, d_in, ldin,
                               d_out, ldout, (hipStream_t)stream);
}

/* ------------------------------------------------------------------ */
/* triangular solve (trsv_kernels.hip, trsv_plan.h)                     */
/* ------------------------------------------------------------------ */

void spmv_trsv_shape(int *group, int *small_rows, int *threads) {
    if (group)
        *group = TRSV_GROUP;
    if (small_rows)
        *small_rows = TRSV_SMALL_ROWS;
    if (threads)
        *threads = TRSV_THREADS;
}

void spmv_trsv_release(spmv_trsv_plan *P) {
    if (!P || !live_take(P))
        return;
    trsv_free_dev(P);
    free(P);
}

void spmv_trsv_release_checked(spmv_trsv_plan *P, uint64_t generation) {
    if (!P || !live_take(P, generation))
        return;
    trsv_free_dev(P);
    free(P);
}

/* NULL -> -EINVAL; not a live plan -> -EBADF, or -ENODEV without a device */
#define PLAN_OK(P)                                                            \
    do {                                                                      \
        if (!(P))                                                             \
            return -EINVAL;                                                   \
        if (!live_has(P))                                                     \
            return spmv_device_count() == 0 ? -ENODEV : -EBADF;               \
    } while (0)

/* both kinds of plan; the caller has checked the numbers */
static int trsv_analyse(const spmv_csr_dev *A, int uplo, int unit,
                        int max_levels, int sweeps, int kmax,
                        spmv_trsv_plan **out) {
    *out = NULL;
    if (spmv_device_count() == 0)
        return -ENODEV; /* no handle can be live: the more useful answer */
    HANDLE_OK(A);
    if (A->M != A->N)
        return -EINVAL;
    if (!has_source(A))
        return -ENODATA; /* spmv_csr_release_source() */
    spmv_trsv_plan *P = (spmv_trsv_plan *)calloc(1, sizeof *P);
    if (!P)
        return -ENOMEM;
    const int rc = trsv_analyse_dev(
        A, uplo, unit, max_levels ? max_levels : TRSV_DEFAULT_MAX_LEVELS, sweeps,
        kmax, P, 0);
    if (rc) {
        trsv_free_dev(P);
        free(P);
        return rc;
    }
    live_add(P);
    *out = P;
    return 0;
}

int spmv_csr_trsv_analyse(const spmv_csr_dev *A, int uplo, int unit,
                          int max_levels, spmv_trsv_plan **out) {
    if (!A || !out || uplo < 0 || uplo > 1 || unit < 0 || unit > 1 ||
        max_levels < 0)
        return -EINVAL;
    return trsv_analyse(A, uplo, unit, max_levels, 0, 0, out);
}

int spmv_csr_trsv_analyse_sweeps(const spmv_csr_dev *A, int uplo, int unit,
                                 int sweeps, int kmax, spmv_trsv_plan **out) {
    if (!A || !out || uplo < 0 || uplo > 1 || unit < 0 || unit > 1 ||
        sweeps < 1 || sweeps > TRSV_MAX_SWEEPS || kmax < 1 || kmax > TRSV_MAX_K)
        return -EINVAL;
    return trsv_analyse(A, uplo, unit, 0, sweeps, kmax, out);
}

int spmv_trsv_sweeps(const spmv_trsv_plan *P, int *sweeps, int *kmax) {
    PLAN_OK(P);
    if (sweeps)
        *sweeps = P->sweeps;
    if (kmax)
        *kmax = P->kmax;
    return 0;
}

int spmv_trsv_info(const spmv_trsv_plan *P, int *M, int *levels,
                   int64_t *entries, int *widest_level, int64_t *zero_diag,
                   int *launches, int64_t *bytes) {
    PLAN_OK(P);
    if (M)
        *M = P->M;
    if (levels)
        *levels = P->levels;
    if (entries)
        *entries = P->entries;
    if (widest_level)
        *widest_level = P->widest_level;
    if (zero_diag)
        *zero_diag = P->zero_diag;
    if (launches)
        *launches = P->sweeps ? P->sweeps : P->n_segs;
    if (bytes)
        *bytes = P->bytes;
    return 0;
}

int spmv_trsv_download(const spmv_trsv_plan *P, int *level, int *order,
                       int *level_ptr, int *rowptr, int *ja, double *as,
                       double *diag) {
    PLAN_OK(P);
    const size_t M = (size_t)P->M, nz = (size_t)P->entries;
    if (level_ptr)
        HIP_RET(hipMemcpy(level_ptr, P->level_ptr,
                          ((size_t)P->levels + 1) * sizeof(int),
                          hipMemcpyDeviceToHost));
    if (M == 0) {
        if (rowptr)
            rowptr[0] = 0;
        return 0;
    }
    if (level)
        HIP_RET(hipMemcpy(level, P->level, M * sizeof(int),
                          hipMemcpyDeviceToHost));
    if (order)
        HIP_RET(hipMemcpy(order, P->order, M * sizeof(int),
                          hipMemcpyDeviceToHost));
    if (rowptr)
        HIP_RET(hipMemcpy(rowptr, P->rowptr, (M + 1) * sizeof(int),
                          hipMemcpyDeviceToHost));
    if (diag)
        HIP_RET(hipMemcpy(diag, P->diag, M * sizeof(double),
                          hipMemcpyDeviceToHost));
    if (ja && nz)
        HIP_RET(hipMemcpy(ja, P->ja, nz * sizeof(int), hipMemcpyDeviceToHost));
    if (as && nz) {
        if (P->value_bytes == 4) { /* widened on the host: exact */
            std::vector<float> narrow(nz);
            HIP_RET(hipMemcpy(narrow.data(), P->as, nz * sizeof(float),
                              hipMemcpyDeviceToHost));
            for (size_t i = 0; i < nz; ++i)
                as[i] = (double)narrow[i];
        } else {
            HIP_RET(hipMemcpy(as, P->as, nz * sizeof(double),
                              hipMemcpyDeviceToHost));
        }
    }
    return 0;
}

int spmv_trsv_solve(const spmv_trsv_plan *P, const spmv_launch_opts *opts, int k,
                    const double *d_B, int64_t ldb, double *d_X, int64_t ldx,
                    const double *d_scale, void *stream) {
    PLAN_OK(P);
    if (k < 1 || k > 8)
        return -EINVAL;
    if (ldb == 0)
        ldb = k;
    if (ldx == 0)
        ldx = k;
    if (ldb < k || ldx < k || !d_B || !d_X)
        return -EINVAL;
    if (opts) {
        if (opts->waves_per_block < 0 || opts->waves_per_block > 16 ||
            opts->group || opts->variant)
            return -EINVAL;
        for (int r : opts->reserved)
            if (r)
                return -EINVAL;
    }
    if (P->sweeps && k > P->kmax)
        return -EINVAL; /* the scratch of a sweep plan holds kmax columns */
    if (P->M == 0)
        return 0;
    return trsv_solve_dev(P, opts ? opts->waves_per_block : 0, k, d_B, ldb, d_X,
                          ldx, d_scale, (hipStream_t)stream);
}

int spmv_csr_generate(int kind, int M, int N, int K, int64_t W, int64_t row0,
                      uint64_t seed, spmv_csr_dev **out) {
    if (!out || M < 0 || N <= 0 || K <= 0 || kind < SYNTH_BANDED ||
        kind > SYNTH_KIND_LAST || (kind == SYNTH_BANDED && N < K))
        return -EINVAL;
    *out = NULL;
    if (spmv_device_count() == 0)
        return -ENODEV;
    synth_spec s = {kind, M, N, K, W, row0, seed};
    int rc = 0;
    spmv_csr_dev *d = NULL;
    /* row lengths on the device, prefix sum on the host (O(M) ints) */
    std::vector<int> irp((size_t)M + 1, 0);
    if (M > 0) {
        int *d_len = NULL;
        HIP_RET(hipMalloc((void **)&d_len, (size_t)M * sizeof(int)));
        hipLaunchKernelGGL(k_synth_lens, dim3((M + 255) / 256), dim3(256), 0,
                           0, s, d_len);
        hipError_t e = hipMemcpy(irp.data() + 1, d_len, (size_t)M * sizeof(int),
                                 hipMemcpyDeviceToHost);
        (void)hipFree(d_len);
        if (e != hipSuccess)
            return hip_errno(e);
    }
    int64_t nz = 0;
    for (int i = 0; i < M; ++i) {
        nz += irp[(size_t)i + 1];
        if (nz > INT32_MAX)
            return -EOVERFLOW;
        irp[(size_t)i + 1] = (int)nz;
    }
    rc = csr_alloc_dev(M, N, nz, 8, &d);
    if (rc)
        return rc;
    HIP_TRY(hipMemcpy(d->irp, irp.data(), ((size_t)M + 1) * sizeof(int),
                      hipMemcpyHostToDevice));
    if (M > 0) {
        /* LDS budget of a 128-row range: the nominal row length with a
         * quarter of slack (the ragged family's longest row) + 8, at most
         * 12288 entries (147 KiB); heavier ranges store directly */
        const int per_row = K + K / 4 + 8;
        const int cap = (int)std::min<long long>(12288, (long long)SYNTH_WG * per_row);
        const size_t lds = ((size_t)SYNTH_AT(cap, SYNTH_SKEW) + 1) * 12 + 16;
        if (lds > 64 * 1024) /* per device, per call: a one-off setup path */
            HIP_TRY(hipFuncSetAttribute(
                (const void *)k_synth_rows,
                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_synth_rows, dim3((M + SYNTH_WG - 1) / SYNTH_WG),
                           dim3(SYNTH_WG), lds, 0, s, d->irp, d->ja, d->as, cap);
    }
    HIP_TRY(hipGetLastError());
    {
        std::vector<int> long_rows;
        int longest = 0;
        for (int i = 0; i < M; ++i) {
            const int len = irp[(size_t)i + 1] - irp[i];
            if (synth_row_is_parallel(&s, row0 + i, len)) {
                long_rows.push_back(i);
                longest = std::max(longest, len);
            }
        }
        if (!long_rows.empty()) {
            int *d_rows = NULL;
            HIP_TRY(hipMalloc((void **)&d_rows, long_rows.size() * sizeof(int)));
            hipError_t e = hipMemcpy(d_rows, long_rows.data(),
                                     long_rows.size() * sizeof(int),
                                     hipMemcpyHostToDevice);
            if (e == hipSuccess) {
                const int chunks = std::min(1024, (longest + 4095) / 4096);
                hipLaunchKernelGGL(k_synth_long_rows,
                                   dim3((unsigned)long_rows.size(), chunks),
                                   dim3(256), 0, 0, s, d->irp, d_rows, d->ja,
                                   d->as);
                e = hipGetLastError();
                if (e == hipSuccess)
                    e = hipDeviceSynchronize();
            }
            (void)hipFree(d_rows);
            if (e != hipSuccess) {
                rc = hip_errno(e);
                goto fail;
            }
        }
    }
    HIP_TRY(hipDeviceSynchronize());
    rc = finish_csr_handle(d, irp.data());
    if (rc)
        goto fail;
    *out = d;
    return 0;
fail:
    spmv_csr_release(d);
    return rc;
}

int spmv_csr_shape(const spmv_csr_dev *A, int *M, int *N, int64_t *NZ) {
    HANDLE_OK(A);
    if (M)
        *M = A->M;
    if (N)
        *N = A->N;
    if (NZ)
        *NZ = A->NZ;
    return 0;
}

int64_t spmv_csr_algorithmic_bytes(const spmv_csr_dev *A) {
    HANDLE_OK(A);
    return (4 + A->value_bytes) * A->NZ + 4 * ((int64_t)A->M + 1) +
           8 * (int64_t)A->M + 8 * (int64_t)A->N;
}

int spmv_csr_download(const spmv_csr_dev *A, sparse_csr **out) {
    HANDLE_OK(A);
    if (!out)
        return -EINVAL;
    if (!has_source(A))
        return -ENODATA; /* spmv_csr_release_source() */
    if (A->NZ > INT32_MAX)
        return -EOVERFLOW;
    sparse_csr *h = csr_alloc("device", A->M, A->N, (int)A->NZ);
    if (IS_ERR(h))
        return PTR_ERR(h);
    int rc = 0;
    HIP_TRY(hipMemcpy(h->IRP, A->irp, ((size_t)A->M + 1) * sizeof(int),
                      hipMemcpyDeviceToHost));
    if (A->NZ > 0) {
        HIP_TRY(hipMemcpy(h->JA, A->ja, (size_t)A->NZ * sizeof(int),
                          hipMemcpyDeviceToHost));
        if (A->value_bytes == 4) { /* widened back: exact */
            std::vector<float> f((size_t)A->NZ);
            HIP_TRY(hipMemcpy(f.data(), A->as32, (size_t)A->NZ * sizeof(float),
                              hipMemcpyDeviceToHost));
            for (size_t k = 0; k < (size_t)A->NZ; ++k)
                h->AS[k] = (double)f[k];
        } else {
            HIP_TRY(hipMemcpy(h->AS, A->as, (size_t)A->NZ * sizeof(double),
                              hipMemcpyDeviceToHost));
        }
    }
    *out = h;
    return 0;
fail:
    csr_free(h);
    return rc;
}

/* ------------------------------------------------------------------ */
/* HLL handle                                                           */
/* ------------------------------------------------------------------ */

static void teardown(spmv_hll_dev *d) {
    (void)hipFree(d->ja);
    (void)hipFree(d->as);
    (void)hipFree(d->as32);
    (void)hipFree(d->off);
    (void)hipFree(d->padmask);
    (void)hipFree(d->base16);
    (void)hipFree(d->off16);
    (void)hipFree(d->wide_seg);
    (void)hipFree(d->wide_part);
    (void)hipFree(d->wide_cnt);
    panels_free(d->panels);
    free(d->tune_log);
    free(d);
}

/* index_bytes 4: ja + padmask; 2: base16 + off16 instead (a compact handle,
 * spmv_hll_to_index16) */
static int hll_alloc_dev(int M, int N, int64_t NZ, int nb, int col_major,
                         int value_bytes, const int64_t *host_off,
                         spmv_hll_dev **out, int index_bytes = 4) {
    int rc = 0;
    spmv_hll_dev *d = (spmv_hll_dev *)calloc(1, sizeof *d);
    if (!d)
        return -ENOMEM;
    live_add(d);
    d->M = M;
    d->N = N;
    d->NZ = NZ;
    d->nb = nb;
    d->value_bytes = value_bytes;
    d->index_bytes = index_bytes;
    d->col_major = col_major ? 1 : 0;
    d->slots = host_off[nb];
    /* before tuning: grouped order for matrices of >= 2M rows (banded
     * 10M x 32: 0.589 ms grouped / 0.622 hardware / 0.651 contiguous),
     * hardware order below (1M x 16: 0.0399 / 0.0426 / 0.0421) */
    d->order = nb >= 65536 ? 2 : 0;
    /* per XCD a contiguous run of hack blocks holding about 1/8 of the slots
     * (each block also counts 32 slots, so empty blocks spread evenly) */
    d->xcd_blk.first[0] = 0;
    for (int k = 1; k < NUM_XCD; ++k) {
        const double want =
            ((double)host_off[nb] + 32.0 * nb) * k / NUM_XCD;
        int lo = d->xcd_blk.first[k - 1], hi = nb;
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if ((double)host_off[mid] + 32.0 * mid < want)
                lo = mid + 1;
            else
                hi = mid;
        }
        d->xcd_blk.first[k] = (lo + 1) & ~1; /* block pairs stay together */
        if (d->xcd_blk.first[k] > nb)
            d->xcd_blk.first[k] = nb;
    }
    d->xcd_blk.first[NUM_XCD] = nb;
    HIP_TRY(hipGetDevice(&d->device));
    /* +64 slots of slack: vector loads of the last chunk stay in bounds */
    if (index_bytes == 2) {
        HIP_TRY(hipMalloc((void **)&d->off16,
                          ((size_t)d->slots + 64) * sizeof(unsigned short)));
        HIP_TRY(hipMalloc((void **)&d->base16, ((size_t)nb + 1) * sizeof(int)));
    } else {
        HIP_TRY(hipMalloc((void **)&d->ja, ((size_t)d->slots + 64) * sizeof(int)));
    }
    if (value_bytes == 4)
        HIP_TRY(hipMalloc((void **)&d->as32, ((size_t)d->slots + 64) * sizeof(float)));
    else
        HIP_TRY(hipMalloc((void **)&d->as, ((size_t)d->slots + 64) * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&d->off, ((size_t)nb + 1) * sizeof(int64_t)));
    if (index_bytes != 2) {
        const size_t words = ((size_t)d->slots + 31) / 32 + 1;
        HIP_TRY(hipMalloc((void **)&d->padmask, words * sizeof(unsigned)));
        HIP_TRY(hipMemset(d->padmask, 0, words * sizeof(unsigned)));
    }
    HIP_TRY(hipMemcpy(d->off, host_off, ((size_t)nb + 1) * sizeof(int64_t),
                      hipMemcpyHostToDevice));
    {
        /* segments of the wide blocks (hip_common.h, HLL_WIDE / HLL_WSEG) */
        std::vector<int4> seg;
        for (int b = 0; b < nb; ++b) {
            const int rows = std::min(HACK_SIZE, M - b * HACK_SIZE);
            const int64_t w = rows > 0 ? (host_off[b + 1] - host_off[b]) / rows : 0;
            if (w <= HLL_WIDE)
                continue;
            /* segments of HLL_WSEG columns, at most HLL_WSEG_MAX of them:
             * wider ones then (multiples of 8 columns) */
            int nseg = (int)std::min<int64_t>((w + HLL_WSEG - 1) / HLL_WSEG,
                                              HLL_WSEG_MAX);
            const int segw = (int)(((w + nseg - 1) / nseg + 7) / 8 * 8);
            nseg = (int)((w + segw - 1) / segw);
            for (int k = 0; k < nseg; ++k)
                seg.push_back(make_int4(b, segw, k, nseg));
        }
        d->n_wide_seg = (int)seg.size();
        if (!seg.empty()) {
            HIP_TRY(hipMalloc((void **)&d->wide_seg, seg.size() * sizeof(int4)));
            HIP_TRY(hipMemcpy(d->wide_seg, seg.data(), seg.size() * sizeof(int4),
                              hipMemcpyHostToDevice));
            HIP_TRY(hipMalloc((void **)&d->wide_part,
                              seg.size() * HACK_SIZE * sizeof(double)));
            HIP_TRY(hipMalloc((void **)&d->wide_cnt,
                              seg.size() * sizeof(unsigned long long)));
            HIP_TRY(hipMemset(d->wide_part, 0,
                              seg.size() * HACK_SIZE * sizeof(double)));
            HIP_TRY(hipMemset(d->wide_cnt, 0,
                              seg.size() * sizeof(unsigned long long)));
        }
    }
    *out = d;
    return 0;
fail:
    spmv_hll_release(d);
    return rc;
}

static int hll_upload(const sparse_hll *H, int is_col_major, int value_bytes,
                      spmv_hll_dev **out) {
    if (!H || !out || H->hack_size != HACK_SIZE)
        return -EINVAL;
    *out = NULL;
    if (spmv_device_count() == 0)
        return -ENODEV;
    const int nb = H->num_blocks;
    std::vector<int64_t> off((size_t)nb + 1, 0);
    int maxw = 0;
    for (int b = 0; b < nb; ++b) {
        off[(size_t)b + 1] =
            off[b] + (int64_t)H->blocks[b].M * H->blocks[b].max_NZ;
        maxw = std::max(maxw, H->blocks[b].max_NZ);
    }
    spmv_hll_dev *d = NULL;
    int rc = hll_alloc_dev(H->M, H->N, H->NZ, nb, is_col_major, value_bytes,
                           off.data(), &d);
    if (rc)
        return rc;
    d->max_width = maxw;
    if (d->slots > 0) {
        if (hll_is_contiguous(H)) { /* slab-backed: two copies */
            HIP_TRY(hipMemcpy(d->ja, H->blocks[0].JA,
                              (size_t)d->slots * sizeof(int),
                              hipMemcpyHostToDevice));
            rc = put_values(d->as, d->as32, 0, H->blocks[0].AS,
                            (size_t)d->slots);
            if (rc)
                goto fail;
        } else {
            /* blocks allocated one by one (the reference's csr_to_hll): pack
             * them into two host slabs in parallel, then two copies -- a copy
             * pair per block is 625 000 hipMemcpy calls at config 3.  Without
             * the host memory for the slabs: block by block after all. */
            int *pj = (int *)malloc((size_t)d->slots * sizeof(int));
            double *pa = (double *)malloc((size_t)d->slots * sizeof(double));
            if (pj && pa) {
                hll_pack_slabs(H, off.data(), pj, pa);
                hipError_t e = hipMemcpy(d->ja, pj, (size_t)d->slots * sizeof(int),
                                         hipMemcpyHostToDevice);
                if (e == hipSuccess)
                    rc = put_values(d->as, d->as32, 0, pa, (size_t)d->slots);
                free(pj);
                free(pa);
                HIP_TRY(e);
                if (rc)
                    goto fail;
            } else {
                free(pj);
                free(pa);
                for (int b = 0; b < nb; ++b) {
                    size_t n = (size_t)(off[(size_t)b + 1] - off[b]);
                    if (!n)
                        continue;
                    HIP_TRY(hipMemcpy(d->ja + off[b], H->blocks[b].JA,
                                      n * sizeof(int), hipMemcpyHostToDevice));
                    rc = put_values(d->as, d->as32, off[b], H->blocks[b].AS, n);
                    if (rc)
                        goto fail;
                }
            }
        }
        rc = hll_fix_pads_dev(d, 0);
        if (rc)
            goto fail;
        HIP_TRY(hipDeviceSynchronize());
    }
    *out = d;
    return 0;
fail:
    spmv_hll_release(d);
    return rc;
}

int spmv_hll_upload(const sparse_hll *H, int is_col_major,
                    spmv_hll_dev **out) {
    return hll_upload(H, is_col_major, 8, out);
}

int spmv_hll_upload_f32(const sparse_hll *H, int is_col_major,
                        spmv_hll_dev **out) {
    return hll_upload(H, is_col_major, 4, out);
}

} /* extern "C" */

/* V = the value type of BOTH handles: the conversion carries it along */
template <typename V>
static int hll_from_csr(const spmv_csr_dev *A, const V *A_as, int is_col_major,
                        spmv_hll_dev **out) {
    HANDLE_OK(A);
    if (!out)
        return -EINVAL;
    if (!has_source(A))
        return -ENODATA;
    *out = NULL;
    const int M = A->M, nb = (M + 31) / 32;
    int rc = 0;
    int *d_w = NULL;
    spmv_hll_dev *d = NULL;
    std::vector<int> w((size_t)nb, 0);
    std::vector<int64_t> off((size_t)nb + 1, 0);
    int maxw = 0;
    if (nb > 0) {
        HIP_TRY(hipMalloc((void **)&d_w, (size_t)nb * sizeof(int)));
        hipLaunchKernelGGL(k_block_width, dim3((M + 255) / 256), dim3(256), 0,
                           0, M, A->irp, d_w);
        HIP_TRY(hipMemcpy(w.data(), d_w, (size_t)nb * sizeof(int),
                          hipMemcpyDeviceToHost));
    }
    for (int b = 0; b < nb; ++b) {
        int rows = std::min(32, M - b * 32);
        off[(size_t)b + 1] = off[b] + (int64_t)rows * w[b];
        maxw = std::max(maxw, w[b]);
    }
    rc = hll_alloc_dev(M, A->N, A->NZ, nb, is_col_major, (int)sizeof(V),
                       off.data(), &d);
    if (rc)
        goto fail;
    d->max_width = maxw;
    if (M > 0) {
        V *d_as = sizeof(V) == 4 ? (V *)d->as32 : (V *)d->as;
        {
            /* LDS budget of a group of 128 rows: mean row length + 25 % + 8
             * per row, 2048..12288 entries; heavier groups read global */
            const long long mean = M > 0 ? (A->NZ + M - 1) / M : 0;
            const int cap = (int)std::max<long long>(
                2048, std::min<long long>(
                          12288, HLL_FILL_BLOCKS * 32 * (mean + mean / 4 + 8)));
            const size_t lds = ((size_t)SYNTH_AT(cap, HLL_FILL_SKEW) + 1) * 12 + 16;
            if (lds > 64 * 1024)
                HIP_TRY(hipFuncSetAttribute(
                    (const void *)k_hll_fill<V>,
                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(k_hll_fill<V>,
                               dim3((nb + HLL_FILL_BLOCKS - 1) / HLL_FILL_BLOCKS),
                               dim3(256), lds, 0, M, nb, d->col_major, A->irp,
                               A->ja, A_as, d->off, d->ja, d_as, d->padmask,
                               cap);
        }
        HIP_TRY(hipGetLastError());
        std::vector<int> wide;
        for (int b = 0; b < nb; ++b)
            if (w[b] > HLL_FILL_WIDE)
                wide.push_back(b);
        if (!wide.empty()) {
            /* d_w (the widths) has done its job: reuse it for the list */
            HIP_TRY(hipMemcpy(d_w, wide.data(), wide.size() * sizeof(int),
                              hipMemcpyHostToDevice));
            const int64_t most = (int64_t)32 * maxw;
            const int chunks = (int)std::min<int64_t>(1024, (most + 8191) / 8192);
            hipLaunchKernelGGL(k_hll_fill_wide<V>,
                               dim3((unsigned)wide.size(), chunks), dim3(256), 0,
                               0, M, d->col_major, d_w, A->irp, A->ja, A_as,
                               d->off, d->ja, d_as, d->padmask);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipDeviceSynchronize());
    }
    (void)hipFree(d_w);
    *out = d;
    return 0;
fail:
    (void)hipFree(d_w);
    spmv_hll_release(d);
    return rc;
}

extern "C" {

int spmv_hll_from_csr(const spmv_csr_dev *A, int is_col_major,
                      spmv_hll_dev **out) {
    HANDLE_OK(A);
    if (A->value_bytes == 4)
        return hll_from_csr(A, (const float *)A->as32, is_col_major, out);
    return hll_from_csr(A, (const double *)A->as, is_col_major, out);
}

/* NULL -> -EINVAL; not a live handle -> -EBADF, or -ENODEV when there is no
 * GPU at all (no handle can be live then: the more useful answer) */
#define HLL16_HANDLE_OK(h)                                                    \
    do {                                                                      \
        if (!(h))                                                             \
            return -EINVAL;                                                   \
        if (!live_has(h))                                                     \
            return spmv_device_count() == 0 ? -ENODEV : -EBADF;               \
    } while (0)

int spmv_hll_index_bytes(const spmv_hll_dev *H) {
    HLL16_HANDLE_OK(H);
    return H->index_bytes == 2 ? 2 : 4;
}

/* a new handle with the pattern and the values of H, the columns stored as
 * one base per hack block + 16-bit offsets (hll_kernels.hip) */
int spmv_hll_to_index16(const spmv_hll_dev *H, spmv_hll_dev **out) {
    if (!H || !out)
        return -EINVAL;
    *out = NULL;
    HLL16_HANDLE_OK(H);
    if (!H->col_major || H->index_bytes == 2)
        return -EINVAL;
    if (!H->ja && H->slots > 0)
        return -ENODATA; /* spmv_hll_release_source() */
    if (H->n_wide_seg > 0)
        return -ENOTSUP; /* hub rows: not the class this format is for */
    int rc = 0;
    spmv_hll_dev *d = NULL;
    unsigned *d_over = NULL, over = 0;
    std::vector<int64_t> off((size_t)H->nb + 1, 0);
    if (H->nb > 0)
        HIP_RET(hipMemcpy(off.data(), H->off,
                          ((size_t)H->nb + 1) * sizeof(int64_t),
                          hipMemcpyDeviceToHost));
    rc = hll_alloc_dev(H->M, H->N, H->NZ, H->nb, 1, H->value_bytes, off.data(),
                       &d, 2);
    if (rc)
        return rc;
    d->max_width = H->max_width;
    d->order = H->order;
    if (H->slots > 0) {
        if (H->value_bytes == 4)
            HIP_TRY(hipMemcpy(d->as32, H->as32, (size_t)H->slots * sizeof(float),
                              hipMemcpyDeviceToDevice));
        else
            HIP_TRY(hipMemcpy(d->as, H->as, (size_t)H->slots * sizeof(double),
                              hipMemcpyDeviceToDevice));
    }
    HIP_TRY(hipMalloc((void **)&d_over, sizeof(unsigned)));
    HIP_TRY(hipMemset(d_over, 0, sizeof(unsigned)));
    rc = hll16_convert_dev(H, d, d_over, 0);
    if (rc)
        goto fail;
    HIP_TRY(hipMemcpy(&over, d_over, sizeof(unsigned), hipMemcpyDeviceToHost));
    if (over) {
        rc = -ERANGE; /* some block's valid columns span more than 65 536 */
        goto fail;
    }
    HIP_TRY(hipDeviceSynchronize());
    (void)hipFree(d_over);
    *out = d;
    return 0;
fail:
    (void)hipFree(d_over);
    spmv_hll_release(d);
    return rc;
}

/* tests: base[nb] and off16[slots] as stored */
int spmv_hll_download_index16(const spmv_hll_dev *H, int *base,
                              uint16_t *off16) {
    HLL16_HANDLE_OK(H);
    if (H->index_bytes != 2)
        return -EINVAL;
    if ((H->nb > 0 && !base) || (H->slots > 0 && !off16))
        return -EINVAL;
    if (H->nb > 0)
        HIP_RET(hipMemcpy(base, H->base16, (size_t)H->nb * sizeof(int),
                          hipMemcpyDeviceToHost));
    if (H->slots > 0)
        HIP_RET(hipMemcpy(off16, H->off16, (size_t)H->slots * sizeof(uint16_t),
                          hipMemcpyDeviceToHost));
    return 0;
}

int spmv_hll_shape(const spmv_hll_dev *H, int *M, int *N, int64_t *NZ,
                   int *num_blocks, int64_t *slots, int *is_col_major) {
    HANDLE_OK(H);
    if (M)
        *M = H->M;
    if (N)
        *N = H->N;
    if (NZ)
        *NZ = H->NZ;
    if (num_blocks)
        *num_blocks = H->nb;
    if (slots)
        *slots = H->slots;
    if (is_col_major)
        *is_col_major = H->col_major;
    return 0;
}

int64_t spmv_hll_algorithmic_bytes(const spmv_hll_dev *H) {
    HANDLE_OK(H);
    if (H->index_bytes == 2) /* 2-byte offsets, and a 4-byte base per block */
        return (2 + H->value_bytes) * H->slots + 4 * (int64_t)H->nb +
               12 * (int64_t)H->nb + 8 * (int64_t)H->M + 8 * (int64_t)H->N;
    return (4 + H->value_bytes) * H->slots + 12 * (int64_t)H->nb +
           8 * (int64_t)H->M + 8 * (int64_t)H->N;
}

/* what ONE launch of `kernel` has to move at least: the direct kernels read
 * every stored slot, padding included (12 S); the blocked copy (kernel 4)
 * holds the true entries only, so it is priced on NZ -- else a padded matrix
 * (S = 10 NZ on a power-law one) would show the blocked kernel above 100 % */
int64_t spmv_hll_kernel_bytes(const spmv_hll_dev *H, int kernel) {
    HANDLE_OK(H);
    if (kernel != SPMV_HLL_KERNEL_PANELS || H->index_bytes == 2)
        return spmv_hll_algorithmic_bytes(H);
    return (4 + H->value_bytes) * H->NZ + 12 * (int64_t)H->nb +
           8 * (int64_t)H->M + 8 * (int64_t)H->N;
}

} /* extern "C" */

/* ------------------------------------------------------------------ */
/* one body for both handle types                                      */
/* ------------------------------------------------------------------ */

/* where the two formats differ */
/* compact handles (16-bit column offsets, spmv_hll_to_index16): HLL only */
static bool is_compact(const spmv_csr_dev *) { return false; }
static bool is_compact(const spmv_hll_dev *H) { return H->index_bytes == 2; }
static int units(const spmv_csr_dev *A) { return A->M; }  /* launch ranges: */
static int units(const spmv_hll_dev *H) { return H->nb; } /* rows / blocks */
static int blocked_kernel(const spmv_csr_dev *) {
    return SPMV_CSR_KERNEL_PANELS;
}
static int blocked_kernel(const spmv_hll_dev *) {
    return SPMV_HLL_KERNEL_PANELS;
}
static int64_t algorithmic_bytes(const spmv_csr_dev *A) {
    return spmv_csr_algorithmic_bytes(A);
}
static int64_t algorithmic_bytes(const spmv_hll_dev *H) {
    return spmv_hll_algorithmic_bytes(H);
}
static int build_from(const spmv_csr_dev *A, int panel_cols, int sched,
                      int tile_rows, spmv_panels **out) {
    return panels_from_csr(A, panel_cols, sched, tile_rows, out);
}
static int build_from(const spmv_hll_dev *H, int panel_cols, int sched,
                      int tile_rows, spmv_panels **out) {
    return panels_from_hll(H, panel_cols, sched, tile_rows, out);
}
static int build_from(const spmv_csr_dev *A, const spmv_panel_opts *o,
                      spmv_panels **out) {
    return panels_from_csr_opts(A, o, out);
}
static int build_from(const spmv_hll_dev *H, const spmv_panel_opts *o,
                      spmv_panels **out) {
    return panels_from_hll_opts(H, o, out);
}
static void free_source(spmv_csr_dev *A) {
    (void)hipFree(A->ja);
    (void)hipFree(A->as);
    (void)hipFree(A->as32);
    A->ja = NULL;
    A->as = NULL;
    A->as32 = NULL;
}
static void free_source(spmv_hll_dev *H) {
    (void)hipFree(H->ja);
    (void)hipFree(H->as);
    (void)hipFree(H->as32);
    (void)hipFree(H->padmask);
    H->ja = NULL;
    H->as = NULL;
    H->as32 = NULL;
    H->padmask = NULL;
}
static int launch_direct(const spmv_csr_dev *A, int kernel,
                         const spmv_launch_opts *opts, const double *d_x,
                         double *d_y, int r0, int r1, hipStream_t s) {
    return csr_launch_kernel(A, kernel,
                             pick_waves(opts, default_waves(g_csr_waves, A->M)),
                             opts ? opts->group : 0, opts ? opts->variant : 0,
                             d_x, d_y, r0, r1, s);
}
static int launch_direct(const spmv_hll_dev *H, int kernel,
                         const spmv_launch_opts *opts, const double *d_x,
                         double *d_y, int b0, int b1, hipStream_t s) {
    int waves = pick_waves(opts, default_waves(g_hll_waves, H->M));
    if (kernel == 1 && waves > 8)
        waves = 8; /* 6 KiB of LDS per wavefront, stay under 64 KiB.  Compact
                      handles (5 / 3 KiB per wavefront) keep the clamp: 16
                      wavefronts of fp64 values are 80 KiB all the same, and a
                      compact launch then has the workgroup shape of its
                      4-byte twin, whatever waves_per_block asks for */
    return hll_launch_kernel(H, kernel, waves, opts ? opts->variant : 0, d_x,
                             d_y, b0, b1, s);
}

template <typename D> static void release(D *d) {
    if (d && live_take(d)) /* else: ignored, counted (spmv_ignored_releases) */
        teardown(d);
}

template <typename D> static void release_checked(D *d, uint64_t generation) {
    if (d && generation && live_take(d, generation))
        teardown(d);
}

/* rows (CSR) or hack blocks (HLL) [begin, end) */
template <typename D>
static int launch_range(const D *d, int kernel, const spmv_launch_opts *opts,
                        const double *d_x, double *d_y, int begin, int end,
                        void *stream) {
    HANDLE_OK(d);
    if (kernel == blocked_kernel(d)) {
        if (!d->panels || begin != 0 || end != units(d))
            return -EINVAL; /* build panels first; whole matrix only */
        return panels_launch(d->panels, d->M,
                             opts ? opts->waves_per_block : 0,
                             opts ? opts->variant : 0, d_x, d_y,
                             (hipStream_t)stream);
    }
    if (!has_source(d))
        return -ENODATA; /* spmv_*_release_source(): blocked path only */
    return launch_direct(d, kernel, opts, d_x, d_y, begin, end,
                         (hipStream_t)stream);
}

template <typename D>
static int launch(const D *d, int kernel, const spmv_launch_opts *opts,
                  const double *d_x, double *d_y, void *stream) {
    HANDLE_OK(d);
    return launch_range(d, kernel, opts, d_x, d_y, 0, units(d), stream);
}

/* ---- Y = A X, 1..8 interleaved vectors (multi_kernels.hip) ---- */
static bool multi_group_ok(const spmv_csr_dev *, int g) {
    return g == 0 || (g >= 2 && g <= 32 && (g & (g - 1)) == 0);
}
static bool multi_group_ok(const spmv_hll_dev *, int) { return true; }
/* the multi-vector HLL kernel is the column-major one */
static bool multi_layout_ok(const spmv_csr_dev *) { return true; }
static bool multi_layout_ok(const spmv_hll_dev *H) { return H->col_major != 0; }
static int multi_direct(const spmv_csr_dev *A, const spmv_launch_opts *opts,
                        int k, const double *X, int64_t ldx, double *Y,
                        int64_t ldy, hipStream_t s) {
    return csr_launch_multi(A, pick_waves(opts, default_waves(g_csr_waves, A->M)),
                            opts ? opts->group : 0, k, X, ldx, Y, ldy, s);
}
static int multi_direct(const spmv_hll_dev *H, const spmv_launch_opts *opts,
                        int k, const double *X, int64_t ldx, double *Y,
                        int64_t ldy, hipStream_t s) {
    return hll_launch_multi(H, pick_waves(opts, default_waves(g_hll_waves, H->M)),
                            k, X, ldx, Y, ldy, s);
}
static int axpby_direct(const spmv_csr_dev *A, const spmv_launch_opts *opts,
                        int k, double alpha, double beta, const double *X,
                        int64_t ldx, double *Y, int64_t ldy, hipStream_t s) {
    return csr_launch_axpby(A, pick_waves(opts, default_waves(g_csr_waves, A->M)),
                            opts ? opts->group : 0, k, alpha, beta, X, ldx, Y,
                            ldy, s);
}
static int axpby_direct(const spmv_hll_dev *H, const spmv_launch_opts *opts,
                        int k, double alpha, double beta, const double *X,
                        int64_t ldx, double *Y, int64_t ldy, hipStream_t s) {
    return hll_launch_axpby(H, pick_waves(opts, default_waves(g_hll_waves, H->M)),
                            k, alpha, beta, X, ldx, Y, ldy, s);
}
static int64_t matrix_bytes(const spmv_csr_dev *A) {
    return (4 + A->value_bytes) * A->NZ + 4 * ((int64_t)A->M + 1);
}
static int64_t matrix_bytes(const spmv_hll_dev *H) {
    return (4 + H->value_bytes) * H->slots + 12 * (int64_t)H->nb;
}

/* the checks of launch_multi and launch_axpby, one copy: 0 = launch (ldx, ldy
 * resolved), 1 = nothing to do (M == 0), negative = the refusal */
template <typename D>
static int multi_check(const D *d, const spmv_launch_opts *opts, int k,
                       const double *d_X, int64_t *ldx, double *d_Y,
                       int64_t *ldy) {
    if (!d)
        return -EINVAL;
    if (!live_has(d)) /* without a device no handle can be live: -ENODEV is
                         the more useful answer (as spmv_csr_to_f32) */
        return spmv_device_count() == 0 ? -ENODEV : -EBADF;
    if (is_compact(d))
        return -ENOTSUP; /* the multi-vector kernels read 4-byte columns */
    if (k < 1 || k > 8)
        return -EINVAL;
    if (*ldx == 0)
        *ldx = k;
    if (*ldy == 0)
        *ldy = k;
    if (*ldx < k || *ldy < k || !d_X || !d_Y)
        return -EINVAL;
    if (opts) {
        if (opts->waves_per_block < 0 || opts->waves_per_block > 16 ||
            !multi_group_ok(d, opts->group) || opts->variant)
            return -EINVAL;
        for (int r : opts->reserved)
            if (r)
                return -EINVAL;
    }
    if (!multi_layout_ok(d))
        return -EINVAL;
    if (!has_source(d))
        return -ENODATA; /* spmv_*_release_source() */
    return d->M == 0 ? 1 : 0;
}

template <typename D>
static int launch_multi(const D *d, const spmv_launch_opts *opts, int k,
                        const double *d_X, int64_t ldx, double *d_Y,
                        int64_t ldy, void *stream) {
    const int rc = multi_check(d, opts, k, d_X, &ldx, d_Y, &ldy);
    if (rc)
        return rc < 0 ? rc : 0;
    return multi_direct(d, opts, k, d_X, ldx, d_Y, ldy, (hipStream_t)stream);
}

/* Y = alpha A X + beta Y in place: launch_multi's checks, launch shape and
 * kernels, with the epilogue at the store */
template <typename D>
static int launch_axpby(const D *d, const spmv_launch_opts *opts, int k,
                        double alpha, double beta, const double *d_X,
                        int64_t ldx, double *d_Y, int64_t ldy, void *stream) {
    const int rc = multi_check(d, opts, k, d_X, &ldx, d_Y, &ldy);
    if (rc)
        return rc < 0 ? rc : 0;
    return axpby_direct(d, opts, k, alpha, beta, d_X, ldx, d_Y, ldy,
                        (hipStream_t)stream);
}

/* what one launch_multi has to move at least: the matrix once, k vectors */
template <typename D> static int64_t multi_bytes(const D *d, int k) {
    HANDLE_OK(d);
    if (is_compact(d))
        return -ENOTSUP;
    if (k < 1 || k > 8)
        return -EINVAL;
    return matrix_bytes(d) + 8 * (int64_t)k * d->M + 8 * (int64_t)k * d->N;
}

/* ... and one launch_axpby: the same, and Y once more when it is read */
template <typename D>
static int64_t axpby_bytes(const D *d, int k, int reads_y) {
    const int64_t b = multi_bytes(d, k);
    return b < 0 || !reads_y ? b : b + 8 * (int64_t)k * d->M;
}

/* ---- conjugate gradients (cg_kernels.hip): the checked entry point ---- */
template <typename D>
static int cg_multi_of(const void *h, const spmv_launch_opts *opts, int k,
                       const double *X, int64_t ldx, double *Y, int64_t ldy,
                       hipStream_t s) {
    return multi_direct((const D *)h, opts, k, X, ldx, Y, ldy, s);
}
template <typename D>
static int cg_axpby_of(const void *h, const spmv_launch_opts *opts, int k,
                       double alpha, double beta, const double *X, int64_t ldx,
                       double *Y, int64_t ldy, hipStream_t s) {
    return axpby_direct((const D *)h, opts, k, alpha, beta, X, ldx, Y, ldy, s);
}

template <typename D>
static cg_matrix cg_matrix_of(const D *d, const spmv_launch_opts *opts) {
    return cg_matrix{d, opts, d->M, cg_multi_of<D>, cg_axpby_of<D>};
}

/*
 * The checks of every solver, in their order: launch_multi's of the handle and
 * the vectors (ldb, ldx resolved), and, for a pair, of dt, the second handle of
 * cgls; the refusals all solvers share (one handle: the matrix is square);
 * then own(), what only this solver refuses (a negative code, or 0).  A matrix
 * without rows (cgls: or columns) has nothing to solve: k zero-filled records.
 * check_every 0 becomes the default.  Returns a negative code, 1 (answered:
 * the caller returns 0) or 0 (solve).
 */
template <typename D, typename Info, typename Own>
static int solver_check(const D *d, const spmv_launch_opts *opts, int k,
                        const double *d_B, int64_t *ldb, double *d_X,
                        int64_t *ldx, double tol, int maxit, int *check_every,
                        Info *info, Own own, const D *dt = NULL,
                        bool pair = false) {
    int64_t ldb_t = *ldb, ldx_t = *ldx;
    const int rc = multi_check(d, opts, k, d_B, ldb, d_X, ldx);
    if (rc < 0)
        return rc;
    const int rct =
        pair ? multi_check(dt, opts, k, d_B, &ldb_t, d_X, &ldx_t) : 0;
    if (rct < 0)
        return rct;
    if ((!pair && d->M != d->N) || !(tol >= 0.0) || maxit < 0 ||
        *check_every < 0 || !info)
        return -EINVAL;
    const int orc = own();
    if (orc)
        return orc;
    if (rc || rct) {
        for (int j = 0; j < k; ++j)
            info[j] = Info{};
        return 1;
    }
    if (!*check_every)
        *check_every = 8;
    return 0;
}

/* pre: spmv_*_pcg, which needs d_minv; spmv_*_cg passes NULL */
template <typename D>
static int cg(const D *d, const spmv_launch_opts *opts, int k,
              const double *d_B, int64_t ldb, double *d_X, int64_t ldx,
              bool pre, const double *d_minv, double tol, int maxit,
              int check_every, void *d_work, size_t work_bytes,
              spmv_cg_info *info, void *stream) {
    const int rc = solver_check(
        d, opts, k, d_B, &ldb, d_X, &ldx, tol, maxit, &check_every, info,
        [&] { return pre && !d_minv ? -EINVAL : 0; });
    if (rc)
        return rc < 0 ? rc : 0;
    const cg_matrix A = cg_matrix_of(d, opts);
    return cg_solve(&A, k, d_B, ldb, d_X, ldx, d_minv, NULL, tol, maxit,
                    check_every, d_work, work_bytes, info, (hipStream_t)stream);
}

/* the checks spmv_*_pcg_trsv, spmv_*_bicgstab_trsv and spmv_*_gmres_trsv add
 * for their plans */
static int plans_check(int M, int k, const spmv_trsv_plan *first,
                       const spmv_trsv_plan *second, const double *d_scale) {
    if (!first || (d_scale && !second))
        return -EINVAL;
    if (!live_has(first) || (second && !live_has(second)))
        return -EBADF;
    if (first->M != M || (second && second->M != M))
        return -EINVAL;
    if ((first->sweeps && first->kmax < k) ||
        (second && second->sweeps && second->kmax < k))
        return -EINVAL;
    return 0;
}

/* spmv_*_pcg_trsv: cg's checks, then the plans'; the plans run with an opts
 * that carries only the caller's waves_per_block */
template <typename D>
static int cg_trsv(const D *d, const spmv_launch_opts *opts, int k,
                   const double *d_B, int64_t ldb, double *d_X, int64_t ldx,
                   const spmv_trsv_plan *first, const spmv_trsv_plan *second,
                   const double *d_scale, double tol, int maxit,
                   int check_every, void *d_work, size_t work_bytes,
                   spmv_cg_info *info, void *stream) {
    const int rc = solver_check(
        d, opts, k, d_B, &ldb, d_X, &ldx, tol, maxit, &check_every, info,
        [&] { return plans_check(d->M, k, first, second, d_scale); });
    if (rc)
        return rc < 0 ? rc : 0;
    const cg_matrix A = cg_matrix_of(d, opts);
    const cg_plans pl = {first, second, d_scale,
                         opts ? opts->waves_per_block : 0};
    return cg_solve(&A, k, d_B, ldb, d_X, ldx, NULL, &pl, tol, maxit,
                    check_every, d_work, work_bytes, info, (hipStream_t)stream);
}

/* ------------------------------------------------------------------ */
/* smoothed-aggregation AMG (amg_kernels.hip, amg_plan.h)               */
/* ------------------------------------------------------------------ */

struct amg_level {
    const spmv_csr_dev *A; /* level 0: borrowed; below: owned */
    spmv_csr_dev *P, *PT;  /* NULL on the coarsest level */
    double *w;             /* M doubles */
    double rho, omega;
    int rounds, aggregates;
};
struct spmv_amg {
    int levels, sweeps, coarse_sweeps, kmax, M;
    amg_level lv[AMG_MAX_LEVELS];
    amg_layout lay;
    double *scratch;
    uint64_t fine_gen; /* the generation of lv[0].A at setup */
};
static_assert(AMG_MAX_LEVELS == SPMV_AMG_MAX_LEVELS && AMG_MAX_K == 8,
              "amg_plan.h and spmv_engine.h agree");

static double g_amg_phases[6];

static void amg_teardown(spmv_amg *H) {
    for (int l = 0; l < H->levels; ++l) {
        amg_level &L = H->lv[l];
        (void)hipFree(L.w);
        spmv_csr_release(L.P); /* NULL: ignored */
        spmv_csr_release(L.PT);
        if (l > 0)
            spmv_csr_release((spmv_csr_dev *)L.A);
    }
    (void)hipFree(H->scratch);
    free(H);
}

/* the caller has checked A (live, square, f64, with its source) and the
 * numbers */
static int amg_setup(const spmv_csr_dev *A0, double theta, int sweeps,
                     int coarse_sweeps, int min_rows, int max_levels,
                     uint32_t seed, int kmax, spmv_amg **out) {
    int rc = 0;
    double ph[6] = {0, 0, 0, 0, 0, 0};
    int rows[AMG_MAX_LEVELS];
    int *d_agg = NULL;
    spmv_csr_dev *T = NULL;
    const spmv_csr_dev *A = A0;
    double t = csr_now_ms();
    const auto lap = [&](int phase) {
        const double n = csr_now_ms();
        ph[phase] += n - t;
        t = n;
    };
    spmv_amg *H = (spmv_amg *)calloc(1, sizeof *H);
    if (!H)
        return -ENOMEM;
    H->sweeps = sweeps;
    H->coarse_sweeps = coarse_sweeps;
    H->kmax = kmax;
    H->M = A0->M;
    H->lv[0].A = A0;
    H->fine_gen = spmv_handle_generation(A0);
    H->levels = 1;
    rc = amg_check_dev(A0, NULL, 0);
    if (rc)
        goto fail;
    for (int l = 0;; ++l) {
        amg_level &L = H->lv[l];
        spmv_aggregate_info ai;
        spmv_csr_dev *C = NULL, *raw = NULL; /* raw: T before it is finished */
        rows[l] = A->M;
        HIP_TRY(hipMalloc((void **)&L.w,
                          (size_t)(A->M > 0 ? A->M : 1) * sizeof(double)));
        rc = amg_rho_dev(A, L.w, &L.rho, 0);
        if (rc)
            goto fail;
        if (!std::isfinite(L.rho) || !(L.rho > 0.0)) {
            rc = -EDOM;
            goto fail;
        }
        L.omega = (4.0 / 3.0) / L.rho;
        rc = amg_w_dev(A->M, L.omega, L.w, 0);
        if (rc)
            goto fail;
        lap(0);
        if (A->M <= min_rows || l + 1 == max_levels)
            break;
        HIP_TRY(hipMalloc((void **)&d_agg, (size_t)A->M * sizeof(int)));
        rc = amg_aggregate_dev(A, theta * theta, seed, AMG_DEFAULT_MAX_ROUNDS,
                               d_agg, &ai, 0);
        if (rc)
            goto fail;
        L.rounds = ai.rounds;
        L.aggregates = ai.aggregates;
        lap(1);
        if (ai.aggregates == A->M)
            break;
        rc = csr_alloc_dev(A->M, ai.aggregates, A->M, 8, &raw);
        if (!rc)
            rc = amg_tentative_dev(A->M, d_agg, raw, 0);
        rc = publish_csr_handle(rc, raw, &T);
        if (!rc)
            rc = spmv_csr_spgemm(A, T, &L.P, NULL);
        if (!rc)
            rc = amg_smooth_p_dev(L.P, d_agg, L.w, 0);
        if (rc)
            goto fail;
        spmv_csr_release(T);
        T = NULL;
        (void)hipFree(d_agg); /* waits for the smoothing */
        d_agg = NULL;
        lap(2);
        rc = spmv_csr_transpose(L.P, &L.PT);
        if (rc)
            goto fail;
        lap(3);
        rc = spmv_csr_galerkin(A, L.P, L.PT, &C, NULL);
        if (rc)
            goto fail;
        H->lv[l + 1].A = C;
        H->levels = l + 2;
        A = C;
        lap(4);
    }
    rc = amg_layout_make(rows, H->levels, kmax, &H->lay);
    if (rc)
        goto fail;
    HIP_TRY(hipMalloc((void **)&H->scratch,
                      (size_t)(H->lay.doubles > 0 ? H->lay.doubles : 1) *
                          sizeof(double)));
    HIP_TRY(hipStreamSynchronize(0));
    lap(5);
    memcpy(g_amg_phases, ph, sizeof ph);
    live_add(H);
    *out = H;
    return 0;
fail:
    (void)hipStreamSynchronize(0);
    (void)hipFree(d_agg);
    spmv_csr_release(T); /* NULL: ignored */
    amg_teardown(H);
    return rc;
}

/* MEASUREMENT (spmv_amg_set_fused): 0 makes every level sweep by the
 * composition, 2 by the fused kernel wherever it can run, 1 (the default) by
 * the measured rule of amg_plan.h (amg_use_fused); the bits are the same */
static int g_amg_fused = 1;

static bool amg_level_fused(const spmv_amg *H, int l, int k) {
    return amg_use_fused(g_amg_fused, k) && amg_sweep_fusable(H->lv[l].A);
}

/* Z = V(R): the launch list of spmv_amg_apply (spmv_engine.h).  The caller
 * has checked everything; waves 0 = the default of every level's launch.
 *
 * A level sweeps by the fused kernel (amg_sweep_dev: x_new to the other buffer
 * of a ping-pong, `cur` and `alt` below) unless its handle has long rows; then
 * by the composition (launch_axpby(-1, 1) into an r that holds b, and the
 * vector kernel, in place).  Both give the same bits.  Level 0's iterate must
 * END in the caller's Z: it starts in the buffer that the level's swaps lead
 * back from (amg_start_buffer). */
static int amg_cycle(const spmv_amg *H, int waves, int k, const double *R,
                     int64_t ldr, double *Z, int64_t ldz, hipStream_t s) {
    spmv_launch_opts o;
    memset(&o, 0, sizeof o);
    o.waves_per_block = waves;
    int rc = 0;
    const int last = H->levels - 1;
    struct view {
        const double *b;
        double *cur, *alt, *r; /* the iterate, the other buffer, r (ld = k) */
        int64_t ldb, ldcur, ldalt;
        bool fused;
        int w; /* workgroup size of the fused sweep, in wavefronts */
    } v[AMG_MAX_LEVELS];
    for (int l = 0; l <= last; ++l) {
        view &t = v[l];
        t.fused = amg_level_fused(H, l, k);
        t.w = pick_waves(&o, default_waves(g_csr_waves, H->lv[l].A->M));
        t.b = l ? H->scratch + H->lay.b[l] : R;
        t.ldb = l ? k : ldr;
        t.r = H->scratch + H->lay.r[l];
        t.cur = l ? H->scratch + H->lay.x[l] : Z;
        t.ldcur = l ? k : ldz;
        t.alt = H->scratch + H->lay.x2[l];
        t.ldalt = k;
        const int swaps = !t.fused ? 0
                          : l == last ? H->coarse_sweeps - 1
                                      : 2 * H->sweeps - 1;
        if (amg_start_buffer(swaps)) {
            std::swap(t.cur, t.alt);
            std::swap(t.ldcur, t.ldalt);
        }
    }
    /* n sweeps.  Composed: behind an r that holds b; refill_last: r = b
     * behind the last one too */
    const auto sweeps = [&](int l, int n, bool refill_last) {
        const amg_level &L = H->lv[l];
        view &t = v[l];
        for (int i = 0; i < n && !rc; ++i) {
            if (t.fused) {
                amg_sweep_dev(L.A, t.w, k, t.cur, t.ldcur, t.b, t.ldb, L.w,
                              t.alt, t.ldalt, s);
                std::swap(t.cur, t.alt);
                std::swap(t.ldcur, t.ldalt);
                continue;
            }
            rc = axpby_direct(L.A, &o, k, -1.0, 1.0, t.cur, t.ldcur, t.r, k, s);
            amg_update_dev(L.A->M, k, i + 1 < n || refill_last, L.w, t.b, t.ldb,
                           t.cur, t.ldcur, t.r, s);
        }
    };
    for (int l = 0; l <= last && !rc; ++l) {
        const amg_level &L = H->lv[l];
        view &t = v[l];
        amg_first_dev(L.A->M, k, L.w, t.b, t.ldb, t.cur, t.ldcur,
                      t.fused ? NULL : t.r, s);
        if (l == last) {
            sweeps(l, H->coarse_sweeps - 1, false);
            break;
        }
        sweeps(l, H->sweeps - 1, true);
        if (rc)
            break;
        if (t.fused) /* r = b - A x: the residual mode */
            amg_sweep_dev(L.A, t.w, k, t.cur, t.ldcur, t.b, t.ldb, NULL, t.r, k,
                          s);
        else
            rc = axpby_direct(L.A, &o, k, -1.0, 1.0, t.cur, t.ldcur, t.r, k, s);
        if (!rc) /* b_c = PT r */
            rc = multi_direct(L.PT, &o, k, t.r, k, (double *)v[l + 1].b, k, s);
    }
    for (int l = last - 1; l >= 0 && !rc; --l) {
        const amg_level &L = H->lv[l];
        view &t = v[l];
        /* x += P x_c */
        rc = axpby_direct(L.P, &o, k, 1.0, 1.0, v[l + 1].cur, v[l + 1].ldcur,
                          t.cur, t.ldcur, s);
        if (!t.fused)
            cg_launch_copy(k, L.A->M, t.b, t.ldb, t.r, k, s);
        sweeps(l, H->sweeps, false);
    }
    if (!rc)
        rc = hip_errno(hipGetLastError());
    return rc;
}

/* the borrowed fine handle is still the one the hierarchy was built from: a
 * live handle at that address WITH THE GENERATION it had at setup (an address
 * the allocator gave to a newer handle is not it) */
static bool amg_fine_alive(const spmv_amg *H) {
    return spmv_handle_generation(H->lv[0].A) == H->fine_gen;
}

/* NULL -> -EINVAL; not a live hierarchy -> -EBADF, or -ENODEV without a
 * device; a hierarchy whose A_0 was released -> -EBADF */
static int amg_ok(const spmv_amg *H) {
    if (!H)
        return -EINVAL;
    if (!live_has(H))
        return spmv_device_count() == 0 ? -ENODEV : -EBADF;
    if (!amg_fine_alive(H))
        return -EBADF;
    if (!has_source(H->lv[0].A))
        return -ENODATA;
    return 0;
}

static int amg_apply(const spmv_amg *H, const spmv_launch_opts *opts, int k,
                     const double *d_R, int64_t ldr, double *d_Z, int64_t ldz,
                     void *stream) {
    const int ok = amg_ok(H);
    if (ok)
        return ok;
    if (k < 1 || k > H->kmax)
        return -EINVAL;
    if (ldr == 0)
        ldr = k;
    if (ldz == 0)
        ldz = k;
    if (ldr < k || ldz < k || !d_R || !d_Z || d_R == d_Z)
        return -EINVAL;
    if (opts) {
        if (opts->waves_per_block < 0 || opts->waves_per_block > 16 ||
            opts->group || opts->variant)
            return -EINVAL;
        for (int r : opts->reserved)
            if (r)
                return -EINVAL;
    }
    (void)hipGetLastError(); /* an earlier caller's unread error is not ours */
    return amg_cycle(H, opts ? opts->waves_per_block : 0, k, d_R, ldr, d_Z,
                     ldz, (hipStream_t)stream);
}

static int amg_apply_of(const void *ctx, int waves, int k, const double *R,
                        double *Z, hipStream_t s) {
    return amg_cycle((const spmv_amg *)ctx, waves, k, R, k, Z, k, s);
}

/* spmv_*_pcg_amg: cg_trsv with the cycle of H where that has the plans */
template <typename D>
static int cg_amg(const D *d, const spmv_launch_opts *opts, int k,
                  const double *d_B, int64_t ldb, double *d_X, int64_t ldx,
                  const spmv_amg *H, double tol, int maxit, int check_every,
                  void *d_work, size_t work_bytes, spmv_cg_info *info,
                  void *stream) {
    const int rc = solver_check(
        d, opts, k, d_B, &ldb, d_X, &ldx, tol, maxit, &check_every, info, [&] {
            if (!H)
                return -EINVAL;
            if (!live_has(H) || !amg_fine_alive(H))
                return -EBADF;
            if (H->M != d->M || k > H->kmax)
                return -EINVAL;
            return has_source(H->lv[0].A) ? 0 : -ENODATA;
        });
    if (rc)
        return rc < 0 ? rc : 0;
    const cg_matrix A = cg_matrix_of(d, opts);
    const cg_plans pl = {NULL, NULL, NULL, opts ? opts->waves_per_block : 0,
                         amg_apply_of, H};
    return cg_solve(&A, k, d_B, ldb, d_X, ldx, NULL, &pl, tol, maxit,
                    check_every, d_work, work_bytes, info, (hipStream_t)stream);
}

/* BiCGStab (bicgstab_kernels.hip): cg's checks and cg's view of the matrix;
 * d_minv may be NULL (no preconditioner) */
template <typename D>
static int bicgstab(const D *d, const spmv_launch_opts *opts, int k,
                    const double *d_B, int64_t ldb, double *d_X, int64_t ldx,
                    const double *d_minv, double tol, int maxit,
                    int check_every, void *d_work, size_t work_bytes,
                    spmv_cg_info *info, void *stream) {
    const int rc = solver_check(d, opts, k, d_B, &ldb, d_X, &ldx, tol, maxit,
                                &check_every, info, [] { return 0; });
    if (rc)
        return rc < 0 ? rc : 0;
    const cg_matrix A = cg_matrix_of(d, opts);
    return bicgstab_solve(&A, k, d_B, ldb, d_X, ldx, d_minv, NULL, tol, maxit,
                          check_every, d_work, work_bytes, info,
                          (hipStream_t)stream);
}

/* spmv_*_bicgstab_trsv: bicgstab's checks, then the plans' as cg_trsv's */
template <typename D>
static int bicgstab_trsv(const D *d, const spmv_launch_opts *opts, int k,
                         const double *d_B, int64_t ldb, double *d_X,
                         int64_t ldx, const spmv_trsv_plan *first,
                         const spmv_trsv_plan *second, const double *d_scale,
                         double tol, int maxit, int check_every, void *d_work,
                         size_t work_bytes, spmv_cg_info *info, void *stream) {
    const int rc = solver_check(
        d, opts, k, d_B, &ldb, d_X, &ldx, tol, maxit, &check_every, info,
        [&] { return plans_check(d->M, k, first, second, d_scale); });
    if (rc)
        return rc < 0 ? rc : 0;
    const cg_matrix A = cg_matrix_of(d, opts);
    const cg_plans pl = {first, second, d_scale,
                         opts ? opts->waves_per_block : 0};
    return bicgstab_solve(&A, k, d_B, ldb, d_X, ldx, NULL, &pl, tol, maxit,
                          check_every, d_work, work_bytes, info,
                          (hipStream_t)stream);
}

/* GMRES(restart) (gmres_kernels.hip): bicgstab's checks, then restart in
 * 1..GM_MAXM; d_minv may be NULL (no preconditioner) */
template <typename D>
static int gmres(const D *d, const spmv_launch_opts *opts, int k,
                 const double *d_B, int64_t ldb, double *d_X, int64_t ldx,
                 const double *d_minv, int restart, double tol, int maxit,
                 int check_every, void *d_work, size_t work_bytes,
                 spmv_gmres_info *info, void *stream) {
    const int rc = solver_check(
        d, opts, k, d_B, &ldb, d_X, &ldx, tol, maxit, &check_every, info,
        [&] { return restart < 1 || restart > GM_MAXM ? -EINVAL : 0; });
    if (rc)
        return rc < 0 ? rc : 0;
    const cg_matrix A = cg_matrix_of(d, opts);
    return gmres_solve(&A, k, d_B, ldb, d_X, ldx, d_minv, NULL, restart, tol,
                       maxit, check_every, d_work, work_bytes, info,
                       (hipStream_t)stream);
}

/* spmv_*_gmres_trsv: gmres's checks, then the plans' as cg_trsv's */
template <typename D>
static int gmres_trsv(const D *d, const spmv_launch_opts *opts, int k,
                      const double *d_B, int64_t ldb, double *d_X, int64_t ldx,
                      const spmv_trsv_plan *first,
                      const spmv_trsv_plan *second, const double *d_scale,
                      int restart, double tol, int maxit, int check_every,
                      void *d_work, size_t work_bytes, spmv_gmres_info *info,
                      void *stream) {
    const int rc = solver_check(
        d, opts, k, d_B, &ldb, d_X, &ldx, tol, maxit, &check_every, info, [&] {
            return restart < 1 || restart > GM_MAXM
                       ? -EINVAL
                       : plans_check(d->M, k, first, second, d_scale);
        });
    if (rc)
        return rc < 0 ? rc : 0;
    const cg_matrix A = cg_matrix_of(d, opts);
    const cg_plans pl = {first, second, d_scale,
                         opts ? opts->waves_per_block : 0};
    return gmres_solve(&A, k, d_B, ldb, d_X, ldx, NULL, &pl, restart, tol,
                       maxit, check_every, d_work, work_bytes, info,
                       (hipStream_t)stream);
}

/* CGLS (cgls_kernels.hip): both handles go through cg's checks, A first, with
 * the one opts; that AT is the transpose of A is not checked, only its shape */
template <typename D>
static int cgls(const D *d, const D *dt, const spmv_launch_opts *opts, int k,
                const double *d_B, int64_t ldb, double *d_X, int64_t ldx,
                double damp, double tol, int maxit, int check_every,
                void *d_work, size_t work_bytes, spmv_cgls_info *info,
                void *stream) {
    const int rc = solver_check(
        d, opts, k, d_B, &ldb, d_X, &ldx, tol, maxit, &check_every, info,
        [&] {
            return dt->M != d->N || dt->N != d->M || !(damp >= 0.0) ? -EINVAL
                                                                    : 0;
        },
        dt, true);
    if (rc)
        return rc < 0 ? rc : 0;
    const cg_matrix A = cg_matrix_of(d, opts);
    const cg_matrix AT = cg_matrix_of(dt, opts);
    return cgls_solve(&A, &AT, k, d_B, ldb, d_X, ldx, damp, tol, maxit,
                      check_every, d_work, work_bytes, info,
                      (hipStream_t)stream);
}

/* MINRES (minres_kernels.hip): bicgstab's checks and cg's view of the matrix;
 * d_minv may be NULL (no preconditioner) */
template <typename D>
static int minres(const D *d, const spmv_launch_opts *opts, int k,
                  const double *d_B, int64_t ldb, double *d_X, int64_t ldx,
                  const double *d_minv, double tol, int maxit, int check_every,
                  void *d_work, size_t work_bytes, spmv_minres_info *info,
                  void *stream) {
    const int rc = solver_check(d, opts, k, d_B, &ldb, d_X, &ldx, tol, maxit,
                                &check_every, info, [] { return 0; });
    if (rc)
        return rc < 0 ? rc : 0;
    const cg_matrix A = cg_matrix_of(d, opts);
    return minres_solve(&A, k, d_B, ldb, d_X, ldx, d_minv, tol, maxit,
                        check_every, d_work, work_bytes, info,
                        (hipStream_t)stream);
}

/* ---- the diagonal (diag_kernels.hip): launch_multi's handle checks ---- */
static int diag_direct(const spmv_csr_dev *A, double *out, int invert,
                       hipStream_t s) {
    return csr_diag(A, out, invert, s);
}
static int diag_direct(const spmv_hll_dev *H, double *out, int invert,
                       hipStream_t s) {
    return hll_diag(H, out, invert, s);
}
template <typename D>
static int diag(const D *d, double *d_out, int invert, void *stream) {
    int64_t ldx = 1, ldy = 1; /* one vector; d_out stands for both pointers */
    const int rc = multi_check(d, (const spmv_launch_opts *)NULL, 1, d_out, &ldx,
                               d_out, &ldy);
    if (rc)
        return rc < 0 ? rc : 0;
    return diag_direct(d, d_out, invert, (hipStream_t)stream);
}

/* a new blocked copy in place of the old one: `build(&d->panels)` */
template <typename D, typename Build> static int rebuild(D *d, Build build) {
    if (d->value_bytes == 4)
        return -ENOTSUP; /* the blocked copy's 12-byte entries hold fp64 values */
    if (is_compact(d))
        return -ENOTSUP; /* ... and is built from 4-byte columns and padmask */
    if (!has_source(d))
        return -ENODATA;
    panels_free(d->panels);
    d->panels = NULL;
    return build(&d->panels);
}

template <typename D> static int build_panels(D *d, int panel_cols) {
    HANDLE_OK(d);
    return rebuild(d, [&](spmv_panels **out) {
        return build_from(d, panel_cols, -1, 0, out);
    });
}

template <typename D>
static int build_panels_opts(D *d, const spmv_panel_opts *opts) {
    HANDLE_OK(d);
    return rebuild(d,
                   [&](spmv_panels **out) { return build_from(d, opts, out); });
}

/* explicit schedule (0 steps, 1 sweep, 2 chain) and tile height (0: default;
 * ignored by sweep): ranks of a multi-GPU job build what rank 0 tuned */
template <typename D>
static int build_panels_as(D *d, int panel_cols, int sched, int tile_rows) {
    HANDLE_OK(d);
    if (sched < 0 || sched > 2)
        return -EINVAL;
    return rebuild(d, [&](spmv_panels **out) {
        return build_from(d, panel_cols, sched, tile_rows, out);
    });
}

/* same schedule and tile height as `model`'s blocked copy (shards of one
 * matrix: tune one, build the others alike) */
template <typename D> static int build_panels_like(D *d, const D *model) {
    HANDLE_OK(d);
    HANDLE_OK(model);
    if (!model->panels)
        return -EINVAL;
    int rc = rebuild(d, [&](spmv_panels **out) {
        spmv_panel_opts o;
        panels_get_opts(model->panels, &o);
        return build_from(d, &o, out);
    });
    if (!rc)
        panels_set_waves(d->panels, panels_waves(model->panels));
    return rc;
}

template <typename D>
static int info_of(const D *d, int *steps, int *tiles, int *panels,
                       int64_t *entries) {
    HANDLE_OK(d);
    const spmv_panels *P = d->panels;
    if (!P)
        return -ENOENT; /* not built */
    if (steps)
        *steps = panels_steps(P);
    if (tiles)
        *tiles = panels_tiles(P);
    if (panels)
        *panels = panels_count(P);
    if (entries)
        *entries = panels_nnz(P);
    return 0;
}

/*
 * Keep only the blocked copy: frees JA/AS (12 B per entry), so a handle that
 * runs the blocked path costs the same HBM as the format it came from.
 * Afterwards only the PANELS kernel id can be launched; the direct kernels,
 * download, conversion and further build_panels calls return -ENODATA.
 */
template <typename D> static int release_source(D *d) {
    HANDLE_OK(d);
    if (!d->panels)
        return -ENOENT; /* nothing else could run the matrix */
    free_source(d);
    return 0;
}

template <typename D> static int value_bytes_of(const D *d) {
    HANDLE_OK(d);
    return d->value_bytes;
}

template <typename D> static int schedule_of(const D *d) {
    HANDLE_OK(d);
    if (!d->panels)
        return -ENOENT;
    return panels_is_sweep(d->panels) ? 1 : panels_is_chain(d->panels) ? 2 : 0;
}

template <typename D>
static int describe_of(const D *d, char *buf, size_t len) {
    HANDLE_OK(d);
    return d->panels ? panels_describe(d->panels, buf, len) : -ENOENT;
}

template <typename D> static int tile_rows_of(const D *d) {
    HANDLE_OK(d);
    return d->panels ? panels_tile_rows(d->panels) : -ENOENT;
}

/* The layout of the blocked copy as build options + the launch's waves hint:
 * build_panels_opts(o) followed by panels_set_waves(waves) on another handle
 * of the same matrix reproduces exactly what the selector settled on (the
 * profiling passes of a workload pin the layout of the un-profiled run this
 * way: under the counters' serialised launches the selector may pick another
 * candidate).  The caller sets o->struct_size = sizeof *o first. */
template <typename D>
static int layout_of(const D *d, spmv_panel_opts *o, int *waves) {
    HANDLE_OK(d);
    if (!o || o->struct_size != (int)sizeof *o)
        return -EINVAL;
    if (!d->panels)
        return -ENOENT;
    panels_get_opts(d->panels, o);
    if (waves)
        *waves = panels_waves(d->panels);
    return 0;
}

/* waves per workgroup of the blocked launch (0: the kernel's default) */
template <typename D> static int set_waves_of(D *d, int waves) {
    HANDLE_OK(d);
    if (!d->panels)
        return -ENOENT;
    if (waves < 0 || waves > 16)
        return -EINVAL;
    panels_set_waves(d->panels, waves);
    return 0;
}

/* sweep copies: the steps counted at the build (panel_launch.h "Chunk fit") */
template <typename D>
static int fit_steps_of(const D *d, int64_t *builtin, int64_t *fit) {
    HANDLE_OK(d);
    if (!d->panels)
        return -ENOENT;
    if (!builtin || !fit)
        return -EINVAL;
    panels_fit_steps(d->panels, builtin, fit);
    return 0;
}

template <typename D>
static int set_fit_steps_of(D *d, int64_t builtin, int64_t fit) {
    HANDLE_OK(d);
    if (!d->panels)
        return -ENOENT;
    if (builtin < 0 || fit < 0)
        return -EINVAL;
    panels_set_fit_steps(d->panels, builtin, fit);
    return 0;
}

/* which tile kernel the blocked launch with these options would run */
template <typename D>
static int plan_of(const D *d, const spmv_launch_opts *opts, int *threads,
                   int *groups, int *ordered) {
    HANDLE_OK(d);
    if (!d->panels)
        return -ENOENT;
    if (!threads || !groups || !ordered)
        return -EINVAL;
    return panels_plan_kernel(d->panels, opts ? opts->waves_per_block : 0,
                              opts ? opts->variant : 0, threads, groups,
                              ordered);
}

/* ------------------------------------------------------------------ */
/* event-timed loops                                                    */
/* ------------------------------------------------------------------ */

#define SPMV_VARIANT_FLUSH_RMW (1 << 29) /* A/B: the read-modify-write flush */

/* scratch buffer of the cache flush; a selector run owns one for all its
 * timed loops */
struct flush_scratch {
    double *buf = NULL;
    size_t bytes = 0;
    int reserve(size_t want) {
        if (want <= bytes)
            return 0;
        (void)hipFree(buf);
        buf = NULL;
        bytes = 0;
        HIP_RET(hipMalloc((void **)&buf, want));
        HIP_RET(hipMemset(buf, 0, want));
        bytes = want;
        return 0;
    }
    ~flush_scratch() { (void)hipFree(buf); }
};

template <typename Launch>
static int timed_loop(Launch launch, int warmup, int iters, size_t flush_bytes,
                      double *ms_each, hipStream_t s, bool flush_rmw = false,
                      flush_scratch *shared = NULL) {
    int rc = 0;
    hipEvent_t e0 = NULL, e1 = NULL;
    flush_scratch own;
    flush_scratch *sc = shared ? shared : &own;
    double *scratch = NULL;
    size_t nflush = flush_bytes / sizeof(double);
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    if (nflush) {
        rc = sc->reserve(nflush * sizeof(double));
        if (rc)
            goto fail;
        scratch = sc->buf;
    }
    for (int it = -warmup; it < iters; ++it) {
        if (nflush && flush_rmw)
            hipLaunchKernelGGL(k_flush, dim3(2048), dim3(256), 0, s, scratch,
                               nflush);
        else if (nflush)
            hipLaunchKernelGGL(k_flush_ro, dim3(2048), dim3(256), 0, s,
                               scratch, nflush, scratch);
        HIP_TRY(hipEventRecord(e0, s));
        rc = launch();
        if (rc)
            goto fail;
        HIP_TRY(hipEventRecord(e1, s));
        HIP_TRY(hipEventSynchronize(e1));
        if (it >= 0) {
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
            ms_each[it] = (double)ms;
        }
    }
fail:
    if (e0)
        (void)hipEventDestroy(e0);
    if (e1)
        (void)hipEventDestroy(e1);
    return rc;
}

template <typename D>
static int time_launches(const D *d, int kernel, const spmv_launch_opts *opts,
                         const double *d_x, double *d_y, int warmup, int iters,
                         size_t flush_bytes, double *ms_each, void *stream) {
    HANDLE_OK(d); /* before the scratch buffer of the flush is allocated */
    if (iters < 0 || warmup < 0 || (iters && !ms_each))
        return -EINVAL;
    return timed_loop(
        [&]() { return launch(d, kernel, opts, d_x, d_y, stream); },
        warmup, iters, flush_bytes, ms_each, (hipStream_t)stream,
        opts && (opts->variant & SPMV_VARIANT_FLUSH_RMW));
}


/* ------------------------------------------------------------------ */
/* kernel selection by measurement                                      */
/* ------------------------------------------------------------------ */

static double median_of(std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return v.empty() ? 0.0 : v[v.size() / 2];
}

/* Candidates are timed in the regime they will run in.  A matrix whose
 * working set fits the 256 MiB Infinity Cache would otherwise be tuned on
 * cache hits (config 2, 212 MB: the blocked copy won cached, 0.0479 vs
 * 0.0463 ms for the stream kernel flushed) while an application that touches
 * anything else between two products -- and the benchmark, SURVEY 8d: "MALL
 * flushed between iterations for working sets < 512 MB" -- sees HBM. */
static size_t tune_flush_bytes(int64_t algorithmic_bytes) {
    return algorithmic_bytes < ((int64_t)512 << 20) ? (size_t)1 << 30 : 0;
}

/* what the phases of one selector run share */
struct tune_run {
    const double *d_x;
    double *d_y;
    size_t flush;
    /* ONE scratch buffer for the cache flush of every timed loop (a 1 GiB
     * hipMalloc + memset + hipFree per loop otherwise) */
    flush_scratch scratch;
    std::vector<double> ms = std::vector<double>(5);
    int best = -1;
    double bms = 1e300;
    tune_log log;
    char line[200];
    double t_begin;
    tune_run(const double *x, double *y, size_t f)
        : d_x(x), d_y(y), flush(f), t_begin(panels_ops::now_s()) {}
    template <typename Launch> int time(Launch l, int warm, int iters) {
        return timed_loop(l, warm, iters, flush, ms.data(), NULL, false,
                          &scratch);
    }
};

/* One selector run: the format's direct kernels (`direct`: times them, fills
 * d->tune_ms, t.best / t.bms and logs its line), then the blocked
 * candidates, then the result. */
template <typename D, typename Direct>
static int autotune(D *d, const double *d_x, double *d_y, int allow_panels,
                    int *best_kernel, double *best_ms, Direct direct) {
    HANDLE_OK(d);
    if (!best_kernel)
        return -EINVAL;
    tune_run t(d_x, d_y, tune_flush_bytes(algorithmic_bytes(d)));
    memset(d->tune_ms, 0, sizeof d->tune_ms);
    int rc = t.scratch.reserve(t.flush);
    if (rc)
        return rc;
    rc = direct(d, t);
    if (rc)
        return rc;
    if (d->value_bytes == 4) {
        t.log("blocked path: not available for f32 values (direct kernels "
              "only)");
        allow_panels = 0;
    }
    if (is_compact(d)) {
        t.log("blocked path: skipped, not available for 16-bit column offsets "
              "(direct kernels only)");
        allow_panels = 0;
    }
    if (allow_panels) {
        const double stream_ms =
            (double)algorithmic_bytes(d) / 7.0e9; /* at 7 TB/s */
        panels_pool_begin(); /* candidates reuse each other's blocks */
        rc = tune_blocked<spmv_panels, panels_ops>(
            &d->panels, d->M, d->M > 0 ? (double)d->NZ / d->M : 0.0, stream_ms,
            &t.bms,
            [&](int sched, int tile_rows, spmv_panels **out) {
                return build_from(d, 0, sched, tile_rows, out);
            },
            [&](double *m) {
                int r = t.time(
                    [&]() {
                        return launch(d, blocked_kernel(d), NULL, d_x, d_y,
                                      NULL);
                    },
                    1, 5);
                *m = median_of(t.ms);
                return r;
            },
            [&](const char *l) { t.log(l); }); /* by reference */
        panels_pool_end();
        if (rc < 0)
            return rc;
        if (rc > 0) {
            t.best = blocked_kernel(d);
            d->tune_ms[t.best] = t.bms;
        }
    }
    snprintf(t.line, sizeof t.line, "total %.3f s",
             panels_ops::now_s() - t.t_begin);
    t.log(t.line);
    free(d->tune_log);
    d->tune_log = t.log.release();
    *best_kernel = t.best;
    if (best_ms)
        *best_ms = t.bms;
    return 0;
}

/* HLL candidates: kernels 1 and 2 (col-major) or 3 and 0 (row-major), the
 * col-major ones in their three workgroup orders */
static int hll_direct(spmv_hll_dev *H, tune_run &t) {
    const int cand_cm[2] = {1, 2}, cand_rm[2] = {3, 0};
    const int *cand = H->col_major ? cand_cm : cand_rm;
    int best_order = H->order;
    int iters = 5, warm = 1;
    {
        /* probe: ONE launch of the first candidate.  Beyond 10 ms (a hack
         * block as wide as a hub row of 10^5 entries: 40-60 ms per launch)
         * every configuration gets a single launch and no warm-up -- the
         * blocked copy is what such a matrix will run anyway */
        spmv_launch_opts o;
        memset(&o, 0, sizeof o);
        o.variant = 1;
        int rc = t.time(
            [&]() {
                return spmv_hll_launch(H, cand[0], &o, t.d_x, t.d_y, NULL);
            },
            0, 1);
        if (rc)
            return rc;
        if (t.ms[0] > 10.0) {
            iters = 1;
            warm = 0;
        }
    }
    for (int k = 0; k < 2; ++k)
        for (int order = 0; order < 3; ++order) { /* the workgroup orders */
            if (!H->col_major && order > 0)
                continue; /* the row-major kernels have one order */
            spmv_launch_opts o;
            memset(&o, 0, sizeof o);
            o.variant = 1 << order; /* bit 0 hardware, 1 ranges, 2 grouped */
            /* 5 launches each -- 1 once a launch has run beyond 10 ms (a hack
             * block as wide as a hub row of 10^5 entries: 40-60 ms per
             * launch, 1.8 s for the six combinations otherwise) */
            int rc = t.time(
                [&]() {
                    return spmv_hll_launch(H, cand[k], &o, t.d_x, t.d_y, NULL);
                },
                warm, iters);
            if (rc)
                return rc;
            double m = median_of(
                std::vector<double>(t.ms.begin(), t.ms.begin() + iters));
            if (m > 10.0)
                iters = 1;
            if (H->tune_ms[cand[k]] == 0.0 || m < H->tune_ms[cand[k]])
                H->tune_ms[cand[k]] = m;
            /* another order has to win by 2 % over hardware order */
            if (m < (order == 0 || t.best != cand[k] ? t.bms : 0.98 * t.bms)) {
                t.bms = m;
                t.best = cand[k];
                best_order = order;
            }
        }
    H->order = best_order;
    snprintf(t.line, sizeof t.line,
             "direct kernels: %.3f s; slots / nnz = %.3f (padding of the "
             "format), widest hack block %d",
             panels_ops::now_s() - t.t_begin,
             H->NZ > 0 ? (double)H->slots / (double)H->NZ : 0.0, H->max_width);
    t.log(t.line);
    return 0;
}

/*
 * CSR candidates.  Always: the sub-wave kernel (three workgroup orders) and
 * the stream kernel (two).  By the shape of the rows:
 *   wave_row    (1)  mean row length >= 48 (a 64-lane wavefront per row wastes
 *                    its lanes below that);
 *   thread_row  (0)  mean row length < 6 -- the reference's plots show its
 *                    thread-per-row kernel winning on roadNet / amazon
 *                    (cuda_csr.cu:19-31), so the selector
 *                    MEASURES it on such matrices instead of assuming;
 *   block_row   (3)  longest row > 64 x the mean (cuda_csr.cu:96-140: the
 *                    kernel for very long rows; it pays a workgroup per row).
 *                    Both extras are timed with ONE launch first and dropped
 *                    there when that runs beyond 20x the best so far.
 * profiles/r04_autotune_irregular.txt records what wins where.
 */
static int csr_direct(spmv_csr_dev *A, tune_run &t) {
    const double mean = A->M > 0 ? (double)A->NZ / A->M : 0.0;
    const int cand[5] = {4, 2, 1, 0, 3}; /* stream first: it is never the slow one */
    int rc = 0;
    /* 5 launches per configuration -- 1 once any launch has run beyond 10 ms
     * (a hub row of 10^5 entries under the sub-wave kernel: 46 ms x 3 orders
     * x 6 launches was most of a 1.2 s selector run) */
    int iters_cap = 5;
    auto time_k = [&](int kernel, int variant, int iters, double *m) {
        spmv_launch_opts o;
        memset(&o, 0, sizeof o);
        o.variant = variant;
        iters = std::min(iters, iters_cap);
        int r = t.time(
            [&]() {
                return spmv_csr_launch(A, kernel, &o, t.d_x, t.d_y, NULL);
            },
            1, iters);
        *m = median_of(std::vector<double>(t.ms.begin(), t.ms.begin() + iters));
        if (*m > 10.0)
            iters_cap = 1;
        return r;
    };
    for (int k = 0; k < 5; ++k) {
        if (cand[k] == 1 && mean < 48.0)
            continue; /* a wavefront per row wastes lanes on short rows */
        if (cand[k] == 0 && !(mean < 6.0))
            continue; /* a lane per row: very short rows only */
        if (cand[k] == 3 && !(A->M > 0 && (double)A->max_row_len > 64.0 * mean))
            continue; /* a workgroup per row: a far longer row than the rest */
        double m;
        if (cand[k] == 2) { /* the sub-wave kernel in its three orders */
            static const int bit[3] = {1, 2, 32};
            double mo[3];
            for (int order = 0; order < 3; ++order) {
                rc = time_k(2, bit[order], 5, &mo[order]);
                if (rc)
                    return rc;
            }
            int pick = 0;
            for (int order = 1; order < 3; ++order)
                if (mo[order] < mo[pick])
                    pick = order;
            A->order = pick;
            m = mo[pick];
        } else if (cand[k] == 4) { /* the stream kernel in its two orders */
            double mo[2];
            for (int grp = 0; grp < 2; ++grp) {
                rc = time_k(4, grp ? 32 : 64, 5, &mo[grp]);
                if (rc)
                    return rc;
            }
            A->stream_grouped = mo[1] < mo[0];
            m = mo[A->stream_grouped];
        } else if (cand[k] == 3 || cand[k] == 0) {
            /* one launch first: a workgroup per row over millions of short
             * rows, or one lane walking a row of 10^5 entries, can be orders
             * of magnitude off -- then one sample is the answer */
            rc = time_k(cand[k], 0, 1, &m);
            if (!rc && m < 20.0 * t.bms)
                rc = time_k(cand[k], 0, cand[k] == 3 ? 2 : 5, &m);
            if (rc)
                return rc;
        } else {
            rc = time_k(cand[k], 0, 5, &m);
            if (rc)
                return rc;
        }
        A->tune_ms[cand[k]] = m;
        if (m < t.bms) {
            t.bms = m;
            t.best = cand[k];
        }
    }
    snprintf(t.line, sizeof t.line,
             "direct kernels: %.3f s; mean row %.2f, longest %d; ms: "
             "thread_row %.4f wave_row %.4f subwave_row %.4f block_row %.4f "
             "stream %.4f (0 = not a candidate)",
             panels_ops::now_s() - t.t_begin, mean, A->max_row_len,
             A->tune_ms[0], A->tune_ms[1], A->tune_ms[2], A->tune_ms[3],
             A->tune_ms[4]);
    t.log(t.line);
    return 0;
}

/* per-kernel medians of the last spmv_*_autotune (ms; 0 = not a candidate),
 * kernel ids 0 .. n-1 */
template <typename D> static int tune_times(const D *d, double *ms, int n) {
    HANDLE_OK(d);
    if (!ms || n < 0)
        return -EINVAL;
    for (int k = 0; k < n; ++k)
        ms[k] = k < 8 ? d->tune_ms[k] : 0.0;
    return 0;
}

/* what the last spmv_*_autotune did, one line per phase with host-clock
 * seconds (build / timing per blocked candidate); -ENOENT before any */
template <typename D>
static int copy_tune_log(const D *d, char *buf, size_t len) {
    HANDLE_OK(d);
    if (!buf || !len)
        return -EINVAL;
    if (!d->tune_log)
        return -ENOENT; /* never tuned */
    snprintf(buf, len, "%s", d->tune_log);
    return 0;
}

/* The exported twins (include/spmv_engine.h): spmv_csr_* and spmv_hll_*
 * forward to the one body above; `range` names the partial launch
 * (launch_rows: rows, launch_blocks: hack blocks) */
#define HANDLE_API(fmt, D, range)                                              \
    void spmv_##fmt##_release(D *d) { release(d); }                            \
    void spmv_##fmt##_release_checked(D *d, uint64_t generation) {             \
        release_checked(d, generation);                                        \
    }                                                                          \
    int spmv_##fmt##_launch(const D *d, int kernel,                            \
                            const spmv_launch_opts *opts, const double *d_x,   \
                            double *d_y, void *stream) {                       \
        return launch(d, kernel, opts, d_x, d_y, stream);                      \
    }                                                                          \
    int spmv_##fmt##_##range(const D *d, int kernel,                           \
                             const spmv_launch_opts *opts, const double *d_x,  \
                             double *d_y, int begin, int end, void *stream) {  \
        return launch_range(d, kernel, opts, d_x, d_y, begin, end, stream);    \
    }                                                                          \
    int spmv_##fmt##_launch_multi(const D *d, const spmv_launch_opts *opts,    \
                                  int k, const double *d_X, int64_t ldx,       \
                                  double *d_Y, int64_t ldy, void *stream) {    \
        return launch_multi(d, opts, k, d_X, ldx, d_Y, ldy, stream);           \
    }                                                                          \
    int64_t spmv_##fmt##_multi_bytes(const D *d, int k) {                      \
        return multi_bytes(d, k);                                              \
    }                                                                          \
    int spmv_##fmt##_launch_axpby(const D *d, const spmv_launch_opts *opts,    \
                                  int k, double alpha, double beta,            \
                                  const double *d_X, int64_t ldx,              \
                                  double *d_Y, int64_t ldy, void *stream) {    \
        return launch_axpby(d, opts, k, alpha, beta, d_X, ldx, d_Y, ldy,       \
                            stream);                                           \
    }                                                                          \
    int64_t spmv_##fmt##_axpby_bytes(const D *d, int k, int reads_y) {         \
        return axpby_bytes(d, k, reads_y);                                     \
    }                                                                          \
    int spmv_##fmt##_cg(const D *d, const spmv_launch_opts *opts, int k,       \
                        const double *d_B, int64_t ldb, double *d_X,           \
                        int64_t ldx, double tol, int maxit, int check_every,   \
                        void *d_work, size_t work_bytes, spmv_cg_info *info,   \
                        void *stream) {                                        \
        return cg(d, opts, k, d_B, ldb, d_X, ldx, false, NULL, tol, maxit,     \
                  check_every, d_work, work_bytes, info, stream);              \
    }                                                                          \
    int spmv_##fmt##_pcg(const D *d, const spmv_launch_opts *opts, int k,      \
                         const double *d_B, int64_t ldb, double *d_X,          \
                         int64_t ldx, const double *d_minv, double tol,        \
                         int maxit, int check_every, void *d_work,             \
                         size_t work_bytes, spmv_cg_info *info,                \
                         void *stream) {                                       \
        return cg(d, opts, k, d_B, ldb, d_X, ldx, true, d_minv, tol, maxit,    \
                  check_every, d_work, work_bytes, info, stream);              \
    }                                                                          \
    int spmv_##fmt##_pcg_trsv(                                                 \
        const D *d, const spmv_launch_opts *opts, int k, const double *d_B,    \
        int64_t ldb, double *d_X, int64_t ldx, const spmv_trsv_plan *first,    \
        const spmv_trsv_plan *second, const double *d_scale, double tol,       \
        int maxit, int check_every, void *d_work, size_t work_bytes,           \
        spmv_cg_info *info, void *stream) {                                    \
        return cg_trsv(d, opts, k, d_B, ldb, d_X, ldx, first, second,          \
                       d_scale, tol, maxit, check_every, d_work, work_bytes,   \
                       info, stream);                                          \
    }                                                                          \
    int spmv_##fmt##_pcg_amg(                                                  \
        const D *d, const spmv_launch_opts *opts, int k, const double *d_B,    \
        int64_t ldb, double *d_X, int64_t ldx, const spmv_amg *H, double tol,  \
        int maxit, int check_every, void *d_work, size_t work_bytes,           \
        spmv_cg_info *info, void *stream) {                                    \
        return cg_amg(d, opts, k, d_B, ldb, d_X, ldx, H, tol, maxit,           \
                      check_every, d_work, work_bytes, info, stream);          \
    }                                                                          \
    int spmv_##fmt##_bicgstab(const D *d, const spmv_launch_opts *opts,        \
                              int k, const double *d_B, int64_t ldb,           \
                              double *d_X, int64_t ldx, const double *d_minv,  \
                              double tol, int maxit, int check_every,          \
                              void *d_work, size_t work_bytes,                 \
                              spmv_cg_info *info, void *stream) {              \
        return bicgstab(d, opts, k, d_B, ldb, d_X, ldx, d_minv, tol, maxit,    \
                        check_every, d_work, work_bytes, info, stream);        \
    }                                                                          \
    int spmv_##fmt##_bicgstab_trsv(                                            \
        const D *d, const spmv_launch_opts *opts, int k, const double *d_B,    \
        int64_t ldb, double *d_X, int64_t ldx, const spmv_trsv_plan *first,    \
        const spmv_trsv_plan *second, const double *d_scale, double tol,       \
        int maxit, int check_every, void *d_work, size_t work_bytes,           \
        spmv_cg_info *info, void *stream) {                                    \
        return bicgstab_trsv(d, opts, k, d_B, ldb, d_X, ldx, first, second,    \
                             d_scale, tol, maxit, check_every, d_work,         \
                             work_bytes, info, stream);                        \
    }                                                                          \
    int spmv_##fmt##_gmres(const D *d, const spmv_launch_opts *opts, int k,    \
                           const double *d_B, int64_t ldb, double *d_X,        \
                           int64_t ldx, const double *d_minv, int restart,     \
                           double tol, int maxit, int check_every,             \
                           void *d_work, size_t work_bytes,                    \
                           spmv_gmres_info *info, void *stream) {              \
        return gmres(d, opts, k, d_B, ldb, d_X, ldx, d_minv, restart, tol,     \
                     maxit, check_every, d_work, work_bytes, info, stream);    \
    }                                                                          \
    int spmv_##fmt##_gmres_trsv(                                               \
        const D *d, const spmv_launch_opts *opts, int k, const double *d_B,    \
        int64_t ldb, double *d_X, int64_t ldx, const spmv_trsv_plan *first,    \
        const spmv_trsv_plan *second, const double *d_scale, int restart,      \
        double tol, int maxit, int check_every, void *d_work,                  \
        size_t work_bytes, spmv_gmres_info *info, void *stream) {              \
        return gmres_trsv(d, opts, k, d_B, ldb, d_X, ldx, first, second,       \
                          d_scale, restart, tol, maxit, check_every, d_work,   \
                          work_bytes, info, stream);                           \
    }                                                                          \
    int spmv_##fmt##_cgls(const D *d, const D *dt,                             \
                          const spmv_launch_opts *opts, int k,                 \
                          const double *d_B, int64_t ldb, double *d_X,         \
                          int64_t ldx, double damp, double tol, int maxit,     \
                          int check_every, void *d_work, size_t work_bytes,    \
                          spmv_cgls_info *info, void *stream) {                \
        return cgls(d, dt, opts, k, d_B, ldb, d_X, ldx, damp, tol, maxit,      \
                    check_every, d_work, work_bytes, info, stream);            \
    }                                                                          \
    int spmv_##fmt##_minres(const D *d, const spmv_launch_opts *opts, int k,   \
                            const double *d_B, int64_t ldb, double *d_X,       \
                            int64_t ldx, const double *d_minv, double tol,     \
                            int maxit, int check_every, void *d_work,          \
                            size_t work_bytes, spmv_minres_info *info,         \
                            void *stream) {                                    \
        return minres(d, opts, k, d_B, ldb, d_X, ldx, d_minv, tol, maxit,      \
                      check_every, d_work, work_bytes, info, stream);          \
    }                                                                          \
    int spmv_##fmt##_diag(const D *d, double *d_out, int invert,               \
                          void *stream) {                                      \
        return diag(d, d_out, invert, stream);                                 \
    }                                                                          \
    int spmv_##fmt##_time(const D *d, int kernel,                              \
                          const spmv_launch_opts *opts, const double *d_x,     \
                          double *d_y, int warmup, int iters,                  \
                          size_t flush_bytes, double *ms_each, void *stream) { \
        return time_launches(d, kernel, opts, d_x, d_y, warmup, iters,         \
                             flush_bytes, ms_each, stream);                    \
    }                                                                          \
    int spmv_##fmt##_build_panels(D *d, int panel_cols) {                      \
        return build_panels(d, panel_cols);                                    \
    }                                                                          \
    int spmv_##fmt##_build_panels_opts(D *d, const spmv_panel_opts *opts) {    \
        return build_panels_opts(d, opts);                                     \
    }                                                                          \
    int spmv_##fmt##_build_panels_as(D *d, int panel_cols, int sched,          \
                                     int tile_rows) {                          \
        return build_panels_as(d, panel_cols, sched, tile_rows);               \
    }                                                                          \
    int spmv_##fmt##_build_panels_like(D *d, const D *model) {                 \
        return build_panels_like(d, model);                                    \
    }                                                                          \
    int spmv_##fmt##_panels_info(const D *d, int *steps, int *tiles,           \
                                 int *panels, int64_t *entries) {              \
        return info_of(d, steps, tiles, panels, entries);                      \
    }                                                                          \
    int spmv_##fmt##_release_source(D *d) { return release_source(d); }        \
    int spmv_##fmt##_value_bytes(const D *d) { return value_bytes_of(d); }     \
    int spmv_##fmt##_panels_schedule(const D *d) { return schedule_of(d); }    \
    int spmv_##fmt##_panels_describe(const D *d, char *buf, size_t len) {      \
        return describe_of(d, buf, len);                                       \
    }                                                                          \
    int spmv_##fmt##_panels_tile_rows(const D *d) { return tile_rows_of(d); }  \
    int spmv_##fmt##_panels_layout(const D *d, spmv_panel_opts *o,             \
                                   int *waves) {                               \
        return layout_of(d, o, waves);                                         \
    }                                                                          \
    int spmv_##fmt##_panels_set_waves(D *d, int waves) {                       \
        return set_waves_of(d, waves);                                         \
    }                                                                          \
    int spmv_##fmt##_panels_fit_steps(const D *d, int64_t *builtin,            \
                                      int64_t *fit) {                          \
        return fit_steps_of(d, builtin, fit);                                  \
    }                                                                          \
    int spmv_##fmt##_panels_set_fit_steps(D *d, int64_t builtin,               \
                                          int64_t fit) {                       \
        return set_fit_steps_of(d, builtin, fit);                              \
    }                                                                          \
    int spmv_##fmt##_panels_plan(const D *d, const spmv_launch_opts *opts,     \
                                 int *threads, int *groups, int *ordered) {    \
        return plan_of(d, opts, threads, groups, ordered);                     \
    }                                                                          \
    int spmv_##fmt##_autotune(D *d, const double *d_x, double *d_y,            \
                              int allow_panels, int *best_kernel,              \
                              double *best_ms) {                               \
        return autotune(d, d_x, d_y, allow_panels, best_kernel, best_ms,       \
                        fmt##_direct);                                         \
    }                                                                          \
    int spmv_##fmt##_tune_times(const D *d, double *ms, int n) {               \
        return tune_times(d, ms, n);                                           \
    }                                                                          \
    int spmv_##fmt##_tune_log(const D *d, char *buf, size_t len) {             \
        return copy_tune_log(d, buf, len);                                     \
    }

extern "C" {

HANDLE_API(csr, spmv_csr_dev, launch_rows)
HANDLE_API(hll, spmv_hll_dev, launch_blocks)

/* ---- smoothed-aggregation AMG: the checked entry points ---- */
int spmv_csr_aggregate(const spmv_csr_dev *A, double theta, uint32_t seed,
                       int max_rounds, int *d_agg, spmv_aggregate_info *info) {
    if (!A || !(theta >= 0.0) || !std::isfinite(theta) || max_rounds < 0)
        return -EINVAL;
    if (spmv_device_count() == 0)
        return -ENODEV; /* no handle can be live: the more useful answer */
    HANDLE_OK(A);
    if (A->M != A->N)
        return -EINVAL;
    if (A->value_bytes != 8)
        return -ENOTSUP;
    if (!has_source(A))
        return -ENODATA; /* spmv_csr_release_source() */
    return amg_aggregate_dev(A, theta * theta, seed, amg_max_rounds(max_rounds),
                             d_agg, info, 0);
}

int spmv_csr_amg_setup(const spmv_csr_dev *A, double theta, int sweeps,
                       int coarse_sweeps, int min_rows, int max_levels,
                       uint32_t seed, int kmax, spmv_amg **out) {
    if (out)
        *out = NULL; /* on ANY error, the argument checks included */
    if (!A || !out || !(theta >= 0.0) || !std::isfinite(theta) || sweeps < 1 ||
        sweeps > AMG_MAX_SWEEPS || coarse_sweeps < 1 ||
        coarse_sweeps > AMG_MAX_SWEEPS || min_rows < 1 || max_levels < 0 ||
        max_levels > AMG_MAX_LEVELS || kmax < 1 || kmax > AMG_MAX_K)
        return -EINVAL;
    if (spmv_device_count() == 0)
        return -ENODEV; /* no handle can be live: the more useful answer */
    HANDLE_OK(A);
    if (A->M != A->N)
        return -EINVAL;
    if (A->value_bytes != 8)
        return -ENOTSUP;
    if (!has_source(A))
        return -ENODATA; /* spmv_csr_release_source() */
    return amg_setup(A, theta, sweeps, coarse_sweeps, min_rows,
                     max_levels ? max_levels : 16, seed, kmax, out);
}

int spmv_amg_info(const spmv_amg *H, spmv_amg_summary *out) {
    if (!H || !out)
        return -EINVAL;
    if (!live_has(H))
        return spmv_device_count() == 0 ? -ENODEV : -EBADF;
    memset(out, 0, sizeof *out);
    out->levels = H->levels;
    out->sweeps = H->sweeps;
    out->coarse_sweeps = H->coarse_sweeps;
    out->kmax = H->kmax;
    /* level 0 is borrowed: its numbers were the handle's when it was live */
    const bool fine = amg_fine_alive(H);
    for (int l = 0; l < H->levels; ++l) {
        const amg_level &L = H->lv[l];
        out->rows[l] = l || fine ? L.A->M : H->M;
        out->entries[l] = l || fine ? L.A->NZ : 0;
        out->rounds[l] = L.rounds;
        out->aggregates[l] = L.aggregates;
        out->rho[l] = L.rho;
        out->omega[l] = L.omega;
        out->launches += amg_level_launches(
            l == H->levels - 1, H->sweeps, H->coarse_sweeps,
            (l || fine) && amg_level_fused(H, l, H->kmax));
    }
    out->complexity = amg_complexity(out->entries, H->levels);
    out->scratch_bytes = H->lay.doubles * 8;
    return 0;
}

int spmv_amg_level(const spmv_amg *H, int level, const spmv_csr_dev **A,
                   const spmv_csr_dev **P, const spmv_csr_dev **PT,
                   const double **d_w) {
    if (!H)
        return -EINVAL;
    if (!live_has(H))
        return spmv_device_count() == 0 ? -ENODEV : -EBADF;
    if (level < 0 || level >= H->levels)
        return -EINVAL;
    const amg_level &L = H->lv[level];
    if (A)
        *A = L.A;
    if (P)
        *P = L.P;
    if (PT)
        *PT = L.PT;
    if (d_w)
        *d_w = L.w;
    return 0;
}

int spmv_amg_set_fused(int on) {
    const int was = g_amg_fused;
    if (on < 0 || on > 2)
        return -EINVAL;
    g_amg_fused = on;
    return was;
}

void spmv_amg_last_phases(double ms[6]) {
    if (ms)
        memcpy(ms, g_amg_phases, sizeof g_amg_phases);
}

void spmv_amg_release(spmv_amg *H) {
    if (H && live_take(H))
        amg_teardown(H);
}

void spmv_amg_release_checked(spmv_amg *H, uint64_t generation) {
    if (H && generation && live_take(H, generation))
        amg_teardown(H);
}

int spmv_amg_apply(const spmv_amg *H, const spmv_launch_opts *opts, int k,
                   const double *d_R, int64_t ldr, double *d_Z, int64_t ldz,
                   void *stream) {
    return amg_apply(H, opts, k, d_R, ldr, d_Z, ldz, stream);
}

int64_t spmv_cg_work_bytes(int M, int k) { return cg_work_bytes(M, k, 0); }
int64_t spmv_pcg_work_bytes(int M, int k) { return cg_work_bytes(M, k, 1); }
int64_t spmv_pcg_trsv_work_bytes(int M, int k) {
    return cg_work_bytes(M, k, 2);
}
int64_t spmv_bicgstab_work_bytes(int M, int k) {
    return bicgstab_work_bytes(M, k, 0);
}
int64_t spmv_bicgstab_trsv_work_bytes(int M, int k) {
    return bicgstab_work_bytes(M, k, 1);
}
int64_t spmv_gmres_work_bytes(int M, int k, int restart) {
    return gmres_work_bytes(M, k, restart);
}
int64_t spmv_cgls_work_bytes(int M, int N, int k) {
    return cgls_work_bytes(M, N, k);
}
int64_t spmv_minres_work_bytes(int M, int k) {
    return minres_work_bytes(M, k);
}
int spmv_debug_sqrt(const double *d_in, double *d_out, int64_t n,
                    void *stream) {
    return minres_debug_sqrt(d_in, d_out, n, (hipStream_t)stream);
}
void spmv_cg_dot_shape(int *workgroups, int *threads) {
    if (workgroups)
        *workgroups = CG_NWG;
    if (threads)
        *threads = CG_T;
}

/* ------------------------------------------------------------------ */
/* one-shot entry points: the reference's seam (hip_csr.h / hip_hll.h)  */
/* upload -> one event-timed launch -> download -> release              */
/* (reference cuda_csr.cu:210-234, cuda_hll.cu:235-260)                 */
/* ------------------------------------------------------------------ */

/*
 * Opt-in "keep the last upload" behind the seam (spmv_seam_cache, hip_csr.h).
 * The reference's driver calls the seam 27 times per matrix on the SAME A /
 * H_row / H_col and the same x (main.c:258-354), and every call allocates,
 * uploads and frees the whole matrix (cuda_csr.cu:180-205; HLL: per hack
 * block, cuda_hll.cu:161-206): config 2 through this seam is 6.3 ms of wall
 * time around a 0.044 ms kernel.  With the cache on, a call whose matrix is
 * the one uploaded last (same pointers, shape, and a 64-bit fingerprint of
 * the arrays' heads and tails) reuses the device copy, its x / y buffers and
 * -- level 2 -- the uploaded x when its fingerprint is unchanged.  Three
 * slots: CSR, row-major HLL, col-major HLL (what one run of the driver
 * holds).  A different matrix replaces its slot; level 0 releases all.
 */
struct seam_slot {
    const void *host;      /* the caller's struct */
    int device;            /* the HIP device the copy lives on: a call made
                              with another device current is a miss (the
                              uncached path and the reference's seam always
                              use the current device) */
    uint64_t print;        /* fingerprint of the matrix */
    mat_ref dev;           /* the device copy */
    double *d_x, *d_y;
    int M, N;
    const double *x_host;  /* level 2: the x that d_x holds */
    uint64_t x_print;
    bool x_valid;
};
static struct {
    std::mutex mu;
    int level;
    seam_slot slot[3];
    long hits, misses;
} g_seam;

static uint64_t fp_mix(uint64_t h, uint64_t v) {
    h ^= v + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
    h *= 0xBF58476D1CE4E5B9ull;
    return h ^ (h >> 29);
}

/* head, tail and 64 strided samples of an array of n 4- or 8-byte items */
static uint64_t fp_array(uint64_t h, const void *p, size_t n, size_t item) {
    h = fp_mix(h, (uint64_t)(uintptr_t)p);
    h = fp_mix(h, n);
    if (!p || !n)
        return h;
    const unsigned char *b = (const unsigned char *)p;
    auto at = [&](size_t i) {
        uint64_t v = 0;
        memcpy(&v, b + i * item, item);
        h = fp_mix(h, v);
    };
    const size_t edge = n < 64 ? n : 64;
    for (size_t i = 0; i < edge; ++i)
        at(i);
    for (size_t i = n - edge; i < n; ++i)
        at(i);
    const size_t step = n / 64 ? n / 64 : 1;
    for (size_t i = 0; i < n; i += step)
        at(i);
    return h;
}

/*
 * Level 3: EVERY byte of the arrays, every call -- the one level that cannot
 * return a stale result whatever the caller changed in place.  Four
 * independent multiply-rotate lanes per 1 MiB chunk (instruction-level
 * parallelism), chunks hashed by up to 8 host threads and combined in order.
 * Priced on config 2 (212 MB of IRP / JA / AS + 8 MB of x): see DESIGN.md.
 */
static uint64_t fp_chunk(const unsigned char *b, size_t bytes) {
    uint64_t h[4] = {0x9E3779B97F4A7C15ull, 0xC2B2AE3D27D4EB4Full,
                     0x165667B19E3779F9ull, 0x27D4EB2F165667C5ull};
    size_t i = 0;
    for (; i + 32 <= bytes; i += 32) {
        uint64_t v[4];
        memcpy(v, b + i, 32);
        for (int k = 0; k < 4; ++k) {
            h[k] = (h[k] ^ v[k]) * 0xFF51AFD7ED558CCDull;
            h[k] = (h[k] << 29) | (h[k] >> 35);
        }
    }
    uint64_t tail = 0, out = fp_mix(fp_mix(h[0], h[1]), fp_mix(h[2], h[3]));
    for (; i < bytes; ++i) {
        tail = (tail << 8) | b[i];
        if ((i & 7) == 7) {
            out = fp_mix(out, tail);
            tail = 0;
        }
    }
    return fp_mix(out, tail ^ bytes);
}

static uint64_t fp_full(uint64_t h, const void *p, size_t n, size_t item) {
    h = fp_mix(h, (uint64_t)(uintptr_t)p);
    h = fp_mix(h, n);
    if (!p || !n)
        return h;
    const unsigned char *b = (const unsigned char *)p;
    const size_t bytes = n * item, CH = (size_t)1 << 20;
    const size_t chunks = (bytes + CH - 1) / CH;
    std::vector<uint64_t> part(chunks);
    int T = spmv_host_threads();
    T = T > 8 ? 8 : T;
    if ((size_t)T > chunks / 4)
        T = (int)(chunks / 4); /* at least 4 MiB per thread */
    auto work = [&](size_t c0, size_t c1) {
        for (size_t c = c0; c < c1; ++c)
            part[c] = fp_chunk(b + c * CH, std::min(CH, bytes - c * CH));
    };
    if (T <= 1) {
        work(0, chunks);
    } else {
        std::vector<std::thread> th;
        for (int t = 1; t < T; ++t)
            th.emplace_back(work, chunks * t / T, chunks * (t + 1) / T);
        work(0, chunks / T);
        for (std::thread &t : th)
            t.join();
    }
    for (uint64_t v : part)
        h = fp_mix(h, v);
    return h;
}

/* the fingerprint of one array at the cache's current level (g_seam.mu held) */
static uint64_t fp_level(uint64_t h, const void *p, size_t n, size_t item);

/* releases what the slot holds, with the device that owns it current */
static void seam_drop(seam_slot *c) {
    int cur = -1;
    const bool held = c->dev || c->d_x || c->d_y;
    if (held && hipGetDevice(&cur) == hipSuccess && cur != c->device)
        (void)hipSetDevice(c->device);
    else
        cur = -1;
    if (c->dev)
        c->dev.release();
    (void)hipFree(c->d_x);
    (void)hipFree(c->d_y);
    if (cur >= 0)
        (void)hipSetDevice(cur);
    memset(c, 0, sizeof *c);
}

void spmv_seam_cache(int level) {
    std::lock_guard<std::mutex> g(g_seam.mu);
    const int old = g_seam.level;
    g_seam.level = level < 0 ? 0 : (level > 3 ? 3 : level);
    /* the fingerprints of levels 1 / 2 (samples) and 3 (every byte) are
     * different functions: what is held was keyed under the old one */
    if (g_seam.level == 0 || (old != 0 && (old == 3) != (g_seam.level == 3)))
        for (seam_slot &c : g_seam.slot)
            seam_drop(&c);
}

static uint64_t fp_level(uint64_t h, const void *p, size_t n, size_t item) {
    return g_seam.level >= 3 ? fp_full(h, p, n, item) : fp_array(h, p, n, item);
}

/* Targeted invalidate: `host` = a matrix struct (sparse_csr* / sparse_hll*)
 * handed to the seam earlier -> its device copy is dropped (the next call
 * uploads again); `host` = an x vector -> the next call uploads x again;
 * NULL -> everything held is dropped, the level stays.  For a caller that
 * edits a matrix or x IN PLACE and runs level 1 / 2 (sampled fingerprints).
 * Returns how many slots it touched. */
int spmv_seam_cache_invalidate(const void *host) {
    std::lock_guard<std::mutex> g(g_seam.mu);
    int n = 0;
    for (seam_slot &c : g_seam.slot) {
        if (!c.dev)
            continue;
        if (!host || c.host == host) {
            seam_drop(&c);
            ++n;
        } else if (c.x_host == host && c.x_valid) {
            c.x_valid = false;
            ++n;
        }
    }
    return n;
}

int spmv_seam_cache_stats(long *hits, long *misses) {
    std::lock_guard<std::mutex> g(g_seam.mu);
    if (hits)
        *hits = g_seam.hits;
    if (misses)
        *misses = g_seam.misses;
    int held = 0;
    for (const seam_slot &c : g_seam.slot)
        held += c.dev ? 1 : 0;
    return held;
}

static int one_shot_vectors(int M, int N, const double *x, double **d_x,
                            double **d_y) {
    int rc = 0;
    *d_x = *d_y = NULL;
    HIP_TRY(hipMalloc((void **)d_x, std::max<size_t>(N, 1) * sizeof(double)));
    HIP_TRY(hipMalloc((void **)d_y, std::max<size_t>(M, 1) * sizeof(double)));
    if (N > 0)
        HIP_TRY(hipMemcpy(*d_x, x, (size_t)N * sizeof(double),
                          hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(*d_y, 0, std::max<size_t>(M, 1) * sizeof(double)));
fail:
    return rc;
}

/* the cached form of upload + vectors: slot `which` (0 CSR, 1 HLL row-major,
 * 2 HLL col-major); `upload` builds the device copy on a miss */
static int seam_acquire(int which, const void *host, uint64_t print, int M,
                        int N, const double *x,
                        const std::function<int(seam_slot *)> &upload,
                        seam_slot **out) {
    int rc = 0;
    seam_slot *c = &g_seam.slot[which];
    int dev = 0;
    HIP_RET(hipGetDevice(&dev));
    const bool hit = c->dev && c->host == host && c->print == print &&
                     c->M == M && c->N == N && c->device == dev;
    if (!hit) {
        seam_drop(c);
        ++g_seam.misses;
        c->device = dev;
        rc = upload(c);
        if (rc) {
            seam_drop(c);
            return rc;
        }
        c->host = host;
        c->print = print;
        c->M = M;
        c->N = N;
        HIP_TRY(hipMalloc((void **)&c->d_x,
                          std::max<size_t>(N, 1) * sizeof(double)));
        HIP_TRY(hipMalloc((void **)&c->d_y,
                          std::max<size_t>(M, 1) * sizeof(double)));
    } else {
        ++g_seam.hits;
    }
    {
        const uint64_t xp = g_seam.level >= 2
                                ? fp_level(0x78, x, (size_t)N, sizeof(double))
                                : 0;
        if (!(g_seam.level >= 2 && c->x_valid && c->x_host == x &&
              c->x_print == xp)) {
            if (N > 0)
                HIP_TRY(hipMemcpy(c->d_x, x, (size_t)N * sizeof(double),
                                  hipMemcpyHostToDevice));
            c->x_host = x;
            c->x_print = xp;
            c->x_valid = g_seam.level >= 2;
        }
    }
    HIP_TRY(hipMemsetAsync(c->d_y, 0, std::max<size_t>(M, 1) * sizeof(double),
                           0));
    *out = c;
    return 0;
fail:
    seam_drop(c);
    return rc;
}

} /* extern "C" */

/* a seam call once its arguments are checked: with the cache on (the
 * caller's `fingerprint` of the matrix, under g_seam.mu) the device copy of
 * slot `which`, else an upload -> vectors -> one timed launch -> y download
 * -> release of its own.  `what` names the format in the spmv_set_debug
 * timing line of the cached call (NULL: no line). */
template <typename D, typename Print, typename Upload>
static double one_shot(int which, const void *host, int M, int N,
                       const double *x, double *y, void *arg, int kernel,
                       Print fingerprint, Upload upload, const char *what) {
    const spmv_launch_opts *opts = (const spmv_launch_opts *)arg;
    double ms = 0.0;
    int rc = 0;
    {
        std::unique_lock<std::mutex> g(g_seam.mu);
        if (g_seam.level > 0) {
            const double t0s = panels_ops::now_s();
            const uint64_t fp = fingerprint();
            seam_slot *c = NULL;
            const double t1 = panels_ops::now_s();
            rc = seam_acquire(which, host, fp, M, N, x,
                              [&](seam_slot *s) {
                                  D *d = NULL;
                                  const int r = upload(&d);
                                  s->dev = mat_ref::of(d);
                                  return r;
                              },
                              &c);
            const double t2 = panels_ops::now_s();
            if (!rc)
                rc = time_launches((const D *)c->dev.h, kernel, opts, c->d_x,
                                   c->d_y, 0, 1, 0, &ms, NULL);
            const double t3 = panels_ops::now_s();
            if (!rc && M > 0)
                rc = spmv_copy_d2h(y, c->d_y, (size_t)M * sizeof(double));
            /* where a cached call spends its host time */
            if (what && live().debug)
                fprintf(stderr,
                        "spmv seam cache (%s): fingerprint %.3f ms, acquire "
                        "%.3f, launch + sync %.3f, y download %.3f\n",
                        what, (t1 - t0s) * 1e3, (t2 - t1) * 1e3,
                        (t3 - t2) * 1e3, (panels_ops::now_s() - t3) * 1e3);
            return rc ? (double)rc : ms;
        }
    }
    D *d = NULL;
    double *d_x = NULL, *d_y = NULL;
    rc = upload(&d);
    if (rc)
        return rc;
    rc = one_shot_vectors(M, N, x, &d_x, &d_y);
    if (!rc)
        rc = time_launches(d, kernel, opts, d_x, d_y, 0, 1, 0, &ms, NULL);
    if (!rc && M > 0)
        rc = spmv_copy_d2h(y, d_y, (size_t)M * sizeof(double));
    (void)hipFree(d_x);
    (void)hipFree(d_y);
    release(d);
    return rc ? (double)rc : ms;
}

extern "C" {

static double csr_one_shot(const sparse_csr *A, const double *x, double *y,
                           void *arg, int kernel) {
    if (!A || !x || !y)
        return -EINVAL;
    return one_shot<spmv_csr_dev>(
        0, A, A->M, A->N, x, y, arg, kernel,
        [&]() {
            uint64_t fp = fp_mix(fp_mix(fp_mix(0x637372, (uint64_t)A->M),
                                        (uint64_t)A->N), (uint64_t)A->NZ);
            fp = fp_level(fp, A->IRP, (size_t)A->M + 1, sizeof(int));
            fp = fp_level(fp, A->JA, (size_t)A->NZ, sizeof(int));
            return fp_level(fp, A->AS, (size_t)A->NZ, sizeof(double));
        },
        [&](spmv_csr_dev **out) { return spmv_csr_upload(A, out); }, "csr");
}

static double hll_one_shot(const sparse_hll *H, const double *x, double *y,
                           void *arg, int kernel, int col_major) {
    if (!H || !x || !y)
        return -EINVAL;
    return one_shot<spmv_hll_dev>(
        col_major ? 2 : 1, H, H->M, H->N, x, y, arg, kernel,
        [&]() {
            uint64_t fp = fp_mix(fp_mix(fp_mix(0x686c6c, (uint64_t)H->M),
                                        (uint64_t)H->N), (uint64_t)H->NZ);
            fp = fp_mix(fp, (uint64_t)H->num_blocks);
            fp = fp_mix(fp, (uint64_t)(uintptr_t)H->blocks);
            /* first, middle and last hack block: shape + array fingerprints
             * (level 3: EVERY block, every byte) */
            const int pick[3] = {0, H->num_blocks / 2, H->num_blocks - 1};
            const int npick = g_seam.level >= 3 ? H->num_blocks
                                                : (H->num_blocks > 0 ? 3 : 0);
            for (int k = 0; k < npick; ++k) {
                const ellpack_block *b =
                    &H->blocks[g_seam.level >= 3 ? k : pick[k]];
                const size_t n = (size_t)b->M * (size_t)b->max_NZ;
                fp = fp_mix(fp, ((uint64_t)b->M << 32) | (uint32_t)b->max_NZ);
                if (g_seam.level >= 3) { /* small arrays: no thread spawn */
                    fp = fp_mix(fp, fp_chunk((const unsigned char *)b->JA,
                                             n * sizeof(int)));
                    fp = fp_mix(fp, fp_chunk((const unsigned char *)b->AS,
                                             n * sizeof(double)));
                } else {
                    fp = fp_array(fp, b->JA, n, sizeof(int));
                    fp = fp_array(fp, b->AS, n, sizeof(double));
                }
            }
            return fp;
        },
        [&](spmv_hll_dev **out) { return spmv_hll_upload(H, col_major, out); },
        NULL);
}

double csr_spmv_hip_thread_row(const sparse_csr *A, const double *x, double *y,
                               void *arg) {
    return csr_one_shot(A, x, y, arg, 0);
}
double csr_spmv_hip_wave_row(const sparse_csr *A, const double *x, double *y,
                             void *arg) {
    return csr_one_shot(A, x, y, arg, 1);
}
double csr_spmv_hip_subwave_row(const sparse_csr *A, const double *x,
                                double *y, void *arg) {
    return csr_one_shot(A, x, y, arg, 2);
}
double csr_spmv_hip_block_row(const sparse_csr *A, const double *x, double *y,
                              void *arg) {
    return csr_one_shot(A, x, y, arg, 3);
}
double csr_spmv_hip_stream(const sparse_csr *A, const double *x, double *y,
                           void *arg) {
    return csr_one_shot(A, x, y, arg, 4);
}

double hll_spmv_hip_threads_row_major(const sparse_hll *H, const double *x,
                                      double *y, void *arg) {
    return hll_one_shot(H, x, y, arg, 0, 0);
}
double hll_spmv_hip_threads_col_major(const sparse_hll *H, const double *x,
                                      double *y, void *arg) {
    return hll_one_shot(H, x, y, arg, 1, 1);
}
double hll_spmv_hip_wave_block(const sparse_hll *H, const double *x, double *y,
                               void *arg) {
    return hll_one_shot(H, x, y, arg, 2, 1);
}
double hll_spmv_hip_subwave_row(const sparse_hll *H, const double *x,
                                double *y, void *arg) {
    return hll_one_shot(H, x, y, arg, 3, 0);
}

/* ------------------------------------------------------------------ */
/* the reference's own symbol names (include/spmv_ref_abi.h)            */
/* ------------------------------------------------------------------ */
void set_csr_warps_per_block(int w) { set_csr_waves_per_block(w); }
void set_hll_warps_per_block(int w) { set_hll_waves_per_block(w); }

double csr_spmv_cuda_thread_row(const sparse_csr *A, const double *x,
                                double *y, void *unused) {
    (void)unused;
    return csr_one_shot(A, x, y, NULL, 0);
}
double csr_spmv_cuda_warp_row(const sparse_csr *A, const double *x, double *y,
                              void *unused) {
    (void)unused;
    return csr_one_shot(A, x, y, NULL, 1);
}
double csr_spmv_cuda_halfwarp_row(const sparse_csr *A, const double *x,
                                  double *y, void *unused) {
    (void)unused;
    return csr_one_shot(A, x, y, NULL, 2);
}
double csr_spmv_cuda_block_row(const sparse_csr *A, const double *x, double *y,
                               void *unused) {
    (void)unused;
    return csr_one_shot(A, x, y, NULL, 3);
}
double csr_spmv_cuda_halfwarp_row_text(const sparse_csr *A, const double *x,
                                       double *y, void *unused) {
    (void)unused;
    return csr_one_shot(A, x, y, NULL, 4);
}
double hll_spmv_cuda_threads_row_major(const sparse_hll *H, const double *x,
                                       double *y, void *unused) {
    (void)unused;
    return hll_one_shot(H, x, y, NULL, 0, 0);
}
double hll_spmv_cuda_threads_col_major(const sparse_hll *H, const double *x,
                                       double *y, void *unused) {
    (void)unused;
    return hll_one_shot(H, x, y, NULL, 1, 1);
}
double hll_spmv_cuda_warp_block(const sparse_hll *H, const double *x,
                                double *y, void *unused) {
    (void)unused;
    return hll_one_shot(H, x, y, NULL, 2, 1);
}
double hll_spmv_cuda_halfwarp_row(const sparse_hll *H, const double *x,
                                  double *y, void *unused) {
    (void)unused;
    return hll_one_shot(H, x, y, NULL, 3, 0);
}

} /* extern "C" */

/* ------------------------------------------------------------------ */
/* mat_ref (mat_ref.h): either format through the same bodies          */
/* ------------------------------------------------------------------ */

template <typename F> static auto on(const mat_ref &m, F f) {
    return m.is_hll ? f(m.hll()) : f(m.csr());
}

int64_t mat_ref::algorithmic_bytes() const {
    return on(*this, [&](auto *d) { return ::algorithmic_bytes(d); });
}
int mat_ref::launch(int kernel, const double *d_x, double *d_y,
                    void *stream) const {
    return on(*this, [&](auto *d) {
        return ::launch(d, kernel, NULL, d_x, d_y, stream);
    });
}
int mat_ref::launch_rows(int kernel, const double *d_x, double *d_y, int r0,
                         int r1, void *stream) const {
    if (is_hll)
        return launch_range(hll(), kernel, NULL, d_x, d_y, r0 / HACK_SIZE,
                            (r1 + HACK_SIZE - 1) / HACK_SIZE, stream);
    return launch_range(csr(), kernel, NULL, d_x, d_y, r0, r1, stream);
}
int mat_ref::autotune(const double *d_x, double *d_y, int allow_panels,
                      int *best_kernel, double *best_ms) const {
    if (is_hll)
        return ::autotune(hll(), d_x, d_y, allow_panels, best_kernel,
                          best_ms, hll_direct);
    return ::autotune(csr(), d_x, d_y, allow_panels, best_kernel, best_ms,
                      csr_direct);
}
int mat_ref::build_panels_opts(const spmv_panel_opts *opts) const {
    return on(*this, [&](auto *d) { return ::build_panels_opts(d, opts); });
}
int mat_ref::build_panels_like(mat_ref model) const {
    if (model.is_hll != is_hll)
        return -EINVAL;
    return on(*this, [&](auto *d) {
        return ::build_panels_like(d, (decltype(d))model.h);
    });
}
int mat_ref::panels_layout(spmv_panel_opts *o, int *waves) const {
    return on(*this, [&](auto *d) { return layout_of(d, o, waves); });
}
int mat_ref::panels_schedule(void) const {
    return on(*this, [&](auto *d) { return schedule_of(d); });
}
int mat_ref::panels_tile_rows(void) const {
    return on(*this, [&](auto *d) { return tile_rows_of(d); });
}
int mat_ref::panels_describe(char *buf, size_t len) const {
    return on(*this, [&](auto *d) { return describe_of(d, buf, len); });
}
void mat_ref::release(void) const {
    on(*this, [&](auto *d) { ::release(d); });
}
