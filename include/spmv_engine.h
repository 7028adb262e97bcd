/*
 * spmv_engine.h -- persistent device-side API under the one-shot entry
 * points of hip_csr.h / hip_hll.h.
 *
 * The reference uploads the whole matrix on every call and times a single
 * un-warmed launch (cuda_csr.cu:180-234; one cudaMalloc pair and three
 * copies PER HACK BLOCK for HLL, cuda_hll.cu:161-206).  Here a matrix is
 * uploaded once into a device handle, launched any number of times on a
 * caller-supplied HIP stream with device-resident x and y, and released.
 * The one-shot functions are thin wrappers over this API.
 *
 * Plain C ABI: opaque handles, raw device pointers (e.g. a torch tensor's
 * data_ptr()), `void *stream` = hipStream_t (NULL = default stream).
 * Every function returns 0 or a negative errno; nothing falls back to the
 * CPU: without a GPU they return -ENODEV.
 *
 * Device layout
 *   CSR   IRP int32[M+1], JA int32[NZ], AS f64[NZ]          (as on host)
 *         + row-block table for the nnz-balanced stream kernel
 *   HLL   ja int32[S], as f64[S]  one slab each, S = sum_b M_b*max_NZ_b,
 *         block b at slot offset off[b]; off int64[nb+1]; pads rewritten
 *         (hip_hll.h).  Row- or col-major inside a block, chosen at upload.
 *
 * Value type of a handle: f64 (AS as above) or f32 (AS stored as float[NZ] /
 * float[S], spmv_*_upload_f32 / spmv_csr_to_f32): 8 instead of 12 bytes per
 * entry.  x, y, every product and every sum stay fp64, in the same order: the
 * result is that of the fp32-rounded matrix, computed in fp64.
 *
 * Algorithmic bytes per launch (used for roofline.achieved):
 *   CSR   12*NZ + 4*(M+1) + 8*M + 8*N
 *   HLL   12*S + 12*nb + 8*M + 8*N
 *   f32 handles: 8*NZ + 4*(M+1) + 8*M + 8*N  /  8*S + 12*nb + 8*M + 8*N
 *   compact HLL handles (spmv_hll_to_index16): (2 + value bytes)*S + 16*nb
 *   + 8*M + 8*N
 */
#ifndef SPMV_ENGINE_H
#define SPMV_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#include "csr.h"
#include "hll.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct spmv_launch_opts {
    int waves_per_block; /* 1..16; 0 = process default (set_*_waves_per_block) */
    int group;           /* lanes per row of the sub-wave kernels; 0 = auto */
    int variant;         /* tuning bit-field, 0 = default.  Workgroup -> XCD
                            order of the direct kernels: bit 0 hardware
                            (round-robin) order, bit 1 XCD-contiguous ranges
                            of equal work, grouped runs of 32 workgroups per
                            XCD: bit 2 (HLL kernels 1 / 2) / bit 5 (CSR
                            sub-wave and stream kernels; bit 6: stream kernel
                            in hardware order); none of them: the handle's
                            order (what spmv_*_autotune measured faster;
                            before tuning: grouped from 2M rows up).  CSR
                            stream kernel: bit 4 = 4- / 8-byte loads only.
                            CSR sub-wave kernel: bit 9 = load IRP even when
                            every row has one length (A/B of the constant-
                            row-length path).  Timed loops: bit 29 = the
                            read-modify-write cache flush of rounds 1 / 2.
                            Blocked path: bit 0 launches a chain copy as steps
                            and vice versa, bits 1 / 2 force the tile order
                            (else spmv_panel_opts.tile_order), bits 16-17
                            name the sweep kernel's chunk: 1 = 576 lanes x 2
                            groups, 2 = 384 x 3 (4608 slots both), 3 = the
                            built-in shape.  Any other bit:
                            -EINVAL, except in an ablations build
                            (spmv_build_flavour) */
    int reserved[5];     /* must be 0 */
} spmv_launch_opts;

/* ---- devices ---- */
int spmv_device_count(void); /* 0 when there is no usable GPU */
int spmv_set_device(int device);
int spmv_get_device(void);   /* current device or negative errno */
/* name (<= len-1 chars), compute units, HBM bytes */
int spmv_device_info(int device, char *name, size_t len, int *compute_units,
                     size_t *hbm_bytes);

/* PCI bus id of a device, "dddd:bb:dd.f" (len >= 16) */
int spmv_device_pci_bus_id(int device, char *buf, size_t len);

/* free / total bytes of HBM on the current device (leak checks) */
int spmv_dev_mem_info(size_t *free_bytes, size_t *total_bytes);

/* ---- raw device memory, for hosts without their own allocator ---- */
int spmv_dev_malloc(void **dptr, size_t bytes);
int spmv_dev_free(void *dptr);
int spmv_dev_memset(void *dptr, int byte, size_t bytes, void *stream);
int spmv_copy_h2d(void *dst_dev, const void *src_host, size_t bytes);
int spmv_copy_d2h(void *dst_host, const void *src_dev, size_t bytes);
int spmv_stream_sync(void *stream);
int spmv_device_sync(void); /* every stream of the current device */
/* GPU timer (reference src/cuda_timer.cu:15-21): events recorded on a stream
 * around whatever the caller enqueues; elapsed_ms waits for `stop` */
int spmv_event_create(void **ev);
int spmv_event_record(void *ev, void *stream);
int spmv_event_elapsed_ms(void *start, void *stop, float *ms);
int spmv_event_destroy(void *ev);
/* Streams, and a hipGraph of whatever is enqueued on one between begin and
 * end: every launch of this API is stream-ordered and capturable (the main
 * kernel, the side launch of long rows / wide hack blocks, the sweep
 * schedule's memset + persistent kernel, the steps schedule's launch
 * sequence), so a solver that iterates y = A x records the launches once and
 * replays them -- x is read where it lives.  Launch each kernel id once
 * eagerly before capturing it (one-off function attributes).  Limits of a
 * replay: INTEGRATION.md "Contracts". */
int spmv_stream_create(void **stream);  /* non-blocking stream */
int spmv_stream_destroy(void *stream);
int spmv_graph_begin_capture(void *stream); /* not the default (NULL) stream */
int spmv_graph_end_capture(void *stream, void **graph_exec);
/* the same, and the topology of what was captured (any out-pointer may be
 * NULL): a single chain of n nodes has n - 1 edges, one root and a largest
 * fan-out of 1.  Added after 0.7; detect it by the symbol. */
int spmv_graph_end_capture_shape(void *stream, void **graph_exec, int *nodes,
                                 int *edges, int *roots, int *max_fanout);
int spmv_graph_launch(void *graph_exec, void *stream);
int spmv_graph_destroy(void *graph_exec);
/* x[i] = synth_x(seed, first + i) generated on the device */
int spmv_dev_fill_synth(double *d_x, int64_t n, uint64_t seed, int64_t first,
                        void *stream);

/*
 * Extra kernel id of both formats: the 2-D blocked path (no reference
 * counterpart, panels.hip).  The entries are additionally stored bucketed by
 * (row tile, column panel of up to 2^18 columns = 2 MiB of x), 12 B each:
 * a row tile's slice of y accumulates in LDS while the x gathers of a panel
 * stay inside the XCD L2s.  Default schedule "sweep": one persistent launch,
 * every workgroup keeps its tile in LDS across all panels, per-XCD phase
 * counters (bounded waits) keep the workgroups on neighbouring panels.
 * Pays off only when rows reach far beyond an L2 of x (3.6x on config 3 with
 * columns anywhere; slower on matrices with locality -- use
 * spmv_*_autotune); costs 12 B per entry of extra HBM.  Build with
 * spmv_*_build_panels() first (panel_cols = 0: default width), then launch
 * this id (whole matrix only).  opts.variant carries tuning bits
 * (panels.hip), opts.waves_per_block < 8 selects 256-lane workgroups.
 */
#define SPMV_CSR_KERNEL_PANELS 5
#define SPMV_HLL_KERNEL_PANELS 4

/*
 * Explicit build options of the blocked copy (spmv_*_build_panels_opts).
 * Everything a build depends on travels in this struct -- the library reads
 * no environment variable and, apart from the process default schedule of
 * spmv_set_panel_schedule(), keeps no mutable global: two host threads may
 * build and launch different handles concurrently.  Initialise with
 * spmv_panel_opts_default(); 0 means "default" in every field except
 * `struct_size`, `sched` and `sweep_layout` (-1).
 */
typedef struct spmv_panel_opts {
    int struct_size;      /* sizeof(spmv_panel_opts) of the header the caller
                             was compiled with: a build call refuses any other
                             value (-EINVAL), so a caller built against an
                             older, shorter struct fails loudly instead of
                             having the library read past it.  ABI: the struct
                             grew in library versions 0.3 (bucket_order),
                             0.4 (this field, first) and 0.5 (deterministic,
                             last; 0.6: its values 0 / 1 / 2; 0.7 added
                             functions only: the f32 handles); spmv_version()
                             tells which library is loaded.  Fill the struct with
                             spmv_panel_opts_default() and then set fields */
    int sched;            /* -1 process default, 0 steps, 1 sweep, 2 chain */
    int panel_cols;       /* columns per panel (rounded down to 2^k); 0: 2^18 */
    int tile_rows;        /* rows per tile of steps / chain (32..20448); 0: 4096;
                             the sweep schedule sizes its own tiles */
    int sweep_wgs_per_cu; /* sweep: workgroups sharing a CU's LDS (1..8);
                             0: chosen per matrix */
    int reserve_cus;      /* sweep: compute units left OUT of the persistent
                             grid so that another kernel (RCCL's all-gather of
                             the previous shard) runs beside it; 0: none */
    int lds_min;          /* launch with at least this many bytes of dynamic
                             LDS (caps workgroups per CU); 0: the tile */
    int tile_order;       /* steps / chain, which tile a workgroup runs:
                             0 = grouped (default: groups of 32 consecutive
                             tiles per XCD, groups dealt round-robin --
                             neighbours share an L2 and the chip advances
                             through one region), 1 = hardware order (tile =
                             workgroup index), 2 = XCD-contiguous ranges of
                             equal work.  spmv_*_autotune measures all three */
    int sweep_layout;     /* sweep: 0 = buckets stored tile-major (a workgroup
                             streams one contiguous region), 1 (and -1 =
                             default) = panel-major inside a round (what the
                             chip reads at one time is one compact region).
                             NOTE: the only field whose "default" is -1; a
                             zero-initialised struct asks for layout 0 */
    int bucket_order;     /* steps / chain, the order in which a tile visits
                             its non-empty buckets: 0 = default (ascending
                             panels; when every tile's panels lie within a
                             span K smaller than the number of panels -- a
                             band -- ascending (panel mod K), so that the
                             neighbouring tiles an XCD runs together sit on
                             at most two panels of x at a time), 1 = always
                             ascending panels */
    int deterministic;    /* bitwise-reproducible launches (added in 0.5,
                             last; tri-state since 0.6): 0 = default, 1 = on,
                             2 = off.  Without it the wavefronts of a
                             workgroup add their products into the tile's LDS
                             slice of y with ds_add_f64 as they come: the
                             ORDER of the additions to one row, and so the
                             last bits of y, vary from launch to launch (held
                             to 1e-12 of the row scale).  With it they add
                             chunk by chunk, one wavefront after the other (an
                             LDS turn counter, no barrier): every row's
                             additions happen in one fixed order -- the same
                             bits on every launch of the copy, as the
                             reference's kernels (cuda_hll.cu:49-72, csr.c:
                             201-216) and the nine direct kernels give.
                             DEFAULT: on for sweep layouts, where it is free
                             (+-2 %: the hand-offs hide under the
                             request-bound loop), off for chain / steps
                             (+3..+10 % there, DESIGN.md: opt-in with 1).
                             spmv_*_autotune builds its candidates with the
                             default, so the blocked copy it keeps on a matrix
                             whose columns reach anywhere is reproducible */
} spmv_panel_opts;

/* every field at its default (struct_size set, sched -1, sweep_layout -1,
 * the rest 0) -- the one place the defaults live */
void spmv_panel_opts_default(spmv_panel_opts *opts);

/* ---- CSR handle ---- */
typedef struct spmv_csr_dev spmv_csr_dev;

int spmv_csr_upload(const sparse_csr *A, spmv_csr_dev **out);
/*
 * f32 handles (library version 0.7): the values are stored as fp32, converted
 * with the C cast (IEEE round to nearest even) -- on the host by the uploads,
 * on the device by spmv_csr_to_f32 (a new handle with the same pattern; the
 * f64 source stays valid; how a spmv_csr_generate()d matrix gets there;
 * -EINVAL on an f32 source).  A finite value that rounds to +-inf: -ERANGE,
 * nothing is created.  NaN and +-inf pass through; values below FLT_MIN
 * become fp32 subnormals and are read back as such (no flush to zero).
 * Every direct kernel id, launch_rows / launch_blocks, the timed loops,
 * graph capture, download (widened back) and autotune (direct kernels only,
 * allow_panels ignored, one line in the tune log says so) work on an f32
 * handle; spmv_hll_from_csr of an f32 CSR handle gives an f32 HLL handle.
 * The blocked path does not: spmv_*_build_panels* return -ENOTSUP, and the
 * PANELS kernel id -EINVAL as on any handle without a copy.  The one-shot
 * seam, the reference ABI names and spmv_mgpu.h create f64 handles only.
 */
int spmv_csr_upload_f32(const sparse_csr *A, spmv_csr_dev **out);
int spmv_csr_to_f32(const spmv_csr_dev *A, spmv_csr_dev **out);
int spmv_csr_value_bytes(const spmv_csr_dev *A); /* 8 or 4 */
/*
 * Transposition on the device: spmv_csr_transpose makes a NEW, ordinary CSR
 * handle T = A^T -- N x M for an M x N source, the same NZ, the same value
 * type (f64 or f32) -- that owns all its arrays.  A is unchanged and may be
 * released afterwards.  Every kernel id, launch_multi, launch_axpby, diag,
 * autotune, the blocked path, spmv_hll_from_csr, spmv_csr_to_f32 and the
 * solvers work on T as on any handle: y = A^T x is a launch of T.
 *
 * THE RESULT IS DEFINED TO THE BYTE: it is the stable counting sort of A's
 * entries, in stored order, by column.  With rows[k] the row of A's k-th
 * stored entry and `order` the stable argsort of JA:
 *     IRP_T[c] = number of entries with a column below c   (IRP_T[N] = NZ)
 *     JA_T = rows[order],  AS_T = AS[order]
 * So row c of T lists its source rows in ascending order; duplicate entries
 * (r, c) keep their source order; values are moved, never computed (NaN
 * payloads, infinities, -0.0 and subnormals arrive with their bits); explicit
 * zeros stay; duplicates are NOT summed.  (A^T)^T is A with every row stably
 * ordered by column -- A itself, byte for byte, when A's rows are sorted.  The
 * bytes do not depend on scheduling: no position comes from an atomic.
 *
 * Errors, in this order: NULL A or out -EINVAL; no device -ENODEV; a dead
 * handle -EBADF; after spmv_csr_release_source -ENODATA; a column of A
 * outside [0, N) -EDOM; a failed allocation -ENOMEM.  On any error nothing is
 * created and *out is NULL.  M, N or NZ may be 0 (T's IRP is then N + 1
 * zeros).  The call blocks until T is complete.
 *
 * Peak device memory: T itself (4 (N + 1) + (4 + value bytes) NZ bytes and
 * the launch tables of any handle) plus the scratch that
 * spmv_transpose_plan reports, freed before the call returns: two buffers of
 * 8 NZ bytes and the counters, 4 * 2^digit_bits bytes per workgroup.  spmv_transpose_plan is host arithmetic and needs no
 * device; any out-pointer may be NULL; -EINVAL for N < 0 or NZ < 0 (or NZ
 * beyond INT32_MAX, which no handle holds).
 *   passes      max(1, ceil(bits(N - 1) / digit_bits)) counting sorts
 *   tile        entries one workgroup owns in each of them
 *   workgroups  ceil(NZ / tile)
 *
 * spmv_csr_symmetry: *out = 0 (none), 1 (the pattern is symmetric) or 2 (the
 * stored values are too).  M != N gives 0.  Otherwise T = A^T and C = T^T are
 * built and released; IRP and JA of C and T equal gives at least 1, and the
 * stored values comparing equal with == as well gives 2: a NaN is never
 * symmetric, -0.0 equals 0.0.  Entries are compared POSITION BY POSITION
 * after the stable ordering; duplicates are not summed, so a matrix that
 * stores (r, c) twice and (c, r) once is not pattern-symmetric, and two
 * duplicates whose values are swapped in the mirror entry do not compare
 * equal although their sums would.  Peak memory: two transposes and one
 * scratch.  Errors as spmv_csr_transpose.  spmv_*_cg / spmv_*_pcg do not
 * call it.
 */
int spmv_csr_transpose(const spmv_csr_dev *A, spmv_csr_dev **out);
int spmv_transpose_plan(int N, int64_t NZ, int *passes, int *digit_bits,
                        int *tile, int64_t *workgroups, int64_t *scratch_bytes);
int spmv_csr_symmetry(const spmv_csr_dev *A, int *out);
/*
 * Level-scheduled sparse triangular solve T x = b (added after 0.7; detect it
 * by the symbol).  spmv_csr_trsv_analyse makes a PLAN from one triangle of a
 * square CSR handle (f64 or f32 values; rows may be unsorted, hold duplicates
 * and explicit zeros, and store both triangles: only the entries of the
 * chosen triangle are used, so the lower plan of a full matrix is the
 * Gauss-Seidel operator D + L).  The plan copies what it needs: A is unchanged
 * and may be released afterwards.  uplo: 0 lower, 1 upper.  unit: 0 = divide
 * by the stored diagonal, 1 = unit diagonal (the solve never reads the stored
 * one; the plan's diag and zero_diag are what they are for unit = 0).
 * max_levels: 0 = the library default, 1 << 20.
 *
 * THE PLAN IS DEFINED TO THE BYTE and does not depend on scheduling:
 *   strict entries of row i: its stored entries with column < i (lower) or
 *       > i (upper), in stored order; duplicates are kept and not summed;
 *       explicit zeros are dependencies (the analysis never looks at a value)
 *   diag[i]:  the fp64 sum, starting from 0.0, of the stored entries in column
 *       i, in stored order (f32 values widened first); 0.0 where the row
 *       stores none.  zero_diag counts the rows with diag == 0.0: it is
 *       information, not an error
 *   level[i]: 0 when row i has no strict entry, else 1 + the largest level of
 *       its strict columns
 *   order:    the stable sort of 0 .. M-1 by level (rows ascending inside a
 *       level); level_ptr[l] = number of rows with a level below l
 *   rowptr / ja / as: the strict entries of row order[p] at position p, in
 *       stored order, in A's value type, the bits moved and never computed
 * The levels come from Kahn's algorithm on the device, one launch and one
 * 4-byte read-back per level (integer atomics on counters; no POSITION that
 * reaches the plan comes from an atomic), the order from the radix sort of
 * spmv_csr_transpose.  The analysis stops with -E2BIG as soon as it would
 * open level max_levels -- a tridiagonal matrix has M levels and is not what
 * a level-scheduled solve is for; no device loop is unbounded.
 *
 * Errors, in this order: NULL A or out, uplo / unit outside 0..1, max_levels
 * < 0 -EINVAL; no device -ENODEV; a dead handle -EBADF; M != N -EINVAL; after
 * spmv_csr_release_source -ENODATA; a column outside [0, N) -EDOM; more than
 * max_levels levels -E2BIG; a failed allocation -ENOMEM.  On any error nothing
 * is created and *out is NULL; all scratch is freed on every path.  M == 0
 * gives a valid plan with 0 levels.  The call blocks.  Plans count in
 * spmv_live_handles() and have a generation (spmv_handle_generation) like
 * every handle; spmv_trsv_release ignores NULL and anything that is not a
 * live plan.
 *
 * spmv_trsv_info: any out-pointer may be NULL.  entries = strict entries,
 * widest_level = rows of the largest level, launches = kernel launches of one
 * solve, bytes = device memory the plan owns.  spmv_trsv_download (tests):
 * level[M], order[M], level_ptr[levels + 1], rowptr[M + 1], ja[entries],
 * as[entries] (widened to fp64), diag[M]; any pointer may be NULL.
 * spmv_trsv_shape: the library constants G = group (lanes and sum slots per
 * row, a power of two), small_rows, threads (lanes of the chain workgroup).
 *
 * spmv_trsv_solve: X = T^-1 B for k = 1..8 interleaved right-hand sides in the
 * layout of spmv_*_launch_multi (ldb, ldx >= k; 0 = k; only columns 0..k-1 of
 * rows 0..M-1 are touched).  Asynchronous on `stream` and capturable: the
 * sequence of launches is a function of the plan alone and the host reads
 * nothing back.  d_X == d_B with ldx == ldb is allowed (in place); any other
 * overlap is undefined.  opts: waves_per_block as in launch_multi (0..16);
 * group, variant and reserved must be 0.  d_scale: M doubles or NULL.
 * Argument errors are the -EINVAL cases of launch_multi; a dead plan -EBADF.
 *
 * THE RESULT IS DEFINED TO THE BIT.  Every operation is rounded once, no
 * fused multiply-add.  For row i, column j, strict entries e_0 .. e_{n-1} in
 * the plan's order:
 *     p_g (g < G) starts at 0.0 and adds rn(a_e * X[c_e, j]) for e = g mod G,
 *         in increasing e
 *     p[g] += p[g + h] for h = G/2 .. 1;  s = p[0]
 *     rhs = B[i, j], or rn(scale_i * B[i, j]) when d_scale is given
 *     X[i, j] = rn(rhs - s) for unit, else rn(rn(rhs - s) / diag_i), a
 *         correctly rounded division
 * So X does not depend on waves_per_block, on k, on the other columns or on
 * which kernel ran a level; a d_scale of ones gives the bits of NULL; a zero
 * diagonal or a non-finite b is plain arithmetic (inf / NaN in that row and
 * its dependents only), never a fault.  d_scale makes symmetric Gauss-Seidel
 * z = (D+U)^-1 D (D+L)^-1 r two solves with no pass in between.
 *
 * Two kernels: a level of more than small_rows rows is one launch over its
 * rows, G lanes per row; a maximal run of consecutive levels of at most
 * small_rows rows each is one launch of ONE workgroup that walks them with a
 * workgroup barrier in between.  There is NO waiting between workgroups of
 * any kind -- no flags, no spins, no grid barrier, no dependency counters in
 * the solve: the kernel boundary on the stream is the only cross-workgroup
 * ordering.
 *
 * Plans are the preconditioner of spmv_*_pcg_trsv and spmv_*_bicgstab_trsv,
 * and spmv_csr_ic0 / spmv_csr_ilu0 make the factors to build them from (all
 * below).  Not in scope: HLL handles, compact (16-bit) handles, the blocked
 * path, a plan as the preconditioner of minres, f32 or HLL input to the
 * factorisations, ILU with fill or a threshold, and any treatment of deep
 * chains beyond the -E2BIG cap.
 */
typedef struct spmv_trsv_plan spmv_trsv_plan;
int spmv_csr_trsv_analyse(const spmv_csr_dev *A, int uplo, int unit,
                          int max_levels, spmv_trsv_plan **out);
int spmv_trsv_info(const spmv_trsv_plan *P, int *M, int *levels,
                   int64_t *entries, int *widest_level, int64_t *zero_diag,
                   int *launches, int64_t *bytes);
int spmv_trsv_download(const spmv_trsv_plan *P, int *level, int *order,
                       int *level_ptr, int *rowptr, int *ja, double *as,
                       double *diag);
void spmv_trsv_shape(int *group, int *small_rows, int *threads);
void spmv_trsv_release(spmv_trsv_plan *P);
void spmv_trsv_release_checked(spmv_trsv_plan *P, uint64_t generation);
int spmv_trsv_solve(const spmv_trsv_plan *P, const spmv_launch_opts *opts, int k,
                    const double *d_B, int64_t ldb, double *d_X, int64_t ldx,
                    const double *d_scale, void *stream);
/*
 * SWEEP PLANS: the triangular solve by a fixed number of Jacobi sweeps (added
 * after 0.7; detect it by the symbol).  With T = D + S (S the strict part),
 *     x(1) = D^-1 b,    x(m) = D^-1 (b - S x(m-1)),  m = 2 .. sweeps,
 * X = x(sweeps): an APPROXIMATE solve (Anzt, Chow, Dongarra 2015) whose cost
 * is `sweeps` launches over all rows whatever the ordering and the depth of
 * the dependency graph.  S is nilpotent, so sweeps >= levels of the exact plan
 * of the same triangle IS the exact solve, to the bit (below).
 *
 * spmv_csr_trsv_analyse_sweeps: A, uplo, unit as spmv_csr_trsv_analyse (f64 or
 * f32 values, unsorted rows, duplicates, explicit zeros, both triangles
 * stored).  sweeps in 1..4096; kmax in 1..8, the most right-hand sides one
 * solve of this plan may take.  The plan owns the strict entries IN ROW ORDER
 * -- order is the identity and rowptr / ja / as / diag are defined as above
 * with that order -- and min(sweeps - 1, 2) scratch vectors of 8 * kmax * M
 * bytes.  No levels are computed: no launch or read-back per level, and a deep
 * chain (a tridiagonal matrix) gets a usable plan, -E2BIG cannot occur.
 * Errors, in this order: NULL A or out, uplo / unit outside 0..1, sweeps
 * outside 1..4096, kmax outside 1..8 -EINVAL; then those of
 * spmv_csr_trsv_analyse from "no device" on.  Nothing is created on an error;
 * M == 0 gives a valid plan.  The plan is a spmv_trsv_plan in every respect:
 * live handle, generation, spmv_trsv_release*.
 *
 * spmv_trsv_sweeps: sweeps and kmax of a plan, 0 and 0 for an exact plan.
 * spmv_trsv_info of a sweep plan: levels = 1 (0 for M == 0), widest_level = M,
 * launches = sweeps, bytes with the scratch.  spmv_trsv_download: level all 0,
 * order the identity, level_ptr = [0, M].
 *
 * spmv_trsv_solve of a sweep plan: the same arguments and checks, then k >
 * kmax -EINVAL.  Asynchronous and capturable, the launches a function of the
 * plan alone; d_X == d_B with ldx == ldb is allowed.  A SOLVE WRITES THE
 * PLAN'S SCRATCH: two solves of one sweep plan must not overlap in time.  On
 * one stream, or ordered by events, is fine; concurrent use of one sweep plan
 * (two streams, two threads, two graphs in flight) is undefined.  Exact plans
 * have no such state.
 *
 * THE RESULT IS DEFINED TO THE BIT.  With row(i; Xin) the row function of
 * spmv_trsv_solve above -- G slots over the strict entries in stored order,
 * the halving tree, rhs, rn(rhs - s), the division unless unit, no fused
 * multiply-add -- and the gathers X[c_e, j] taken from Xin:
 *     x(1)[i] = row(i) with s = +0.0 (the matrix is not read)
 *     x(m)[i] = row(i; x(m-1)),  m = 2 .. sweeps
 * A sweep reads only what the launch before it wrote: no waiting between
 * workgroups, no atomics.  X depends on neither k, waves_per_block, kmax,
 * in-place use, nor the run.  A row of level l of the exact plan is final
 * after sweep l + 1, so sweeps >= levels gives the exact solve's bits for any
 * B, NaN and inf included; a NaN in row r of B reaches exactly the rows within
 * sweeps - 1 dependency steps of r; a zero diagonal is plain arithmetic.
 *
 * Every solver that takes plans takes sweep plans unchanged, with one more
 * refusal after "a plan whose M is not A's": a sweep plan with kmax < k is
 * -EINVAL.  For spmv_*_pcg_trsv give both plans THE SAME sweeps: then z(r) =
 * B^T B r (IC) or B^T D B r (SGS) with B = P_s(D^-1 S) D^-1, symmetric positive
 * definite.  Unequal counts make the preconditioner nonsymmetric and CG may
 * end with its breakdown status; this is not checked.
 */
int spmv_csr_trsv_analyse_sweeps(const spmv_csr_dev *A, int uplo, int unit,
                                 int sweeps, int kmax, spmv_trsv_plan **out);
int spmv_trsv_sweeps(const spmv_trsv_plan *P, int *sweeps, int *kmax);
/*
 * Zero-fill incomplete Cholesky A ~ L L^T on the device (added after 0.7;
 * detect it by the symbol).  A: a square CSR handle with f64 values.  Only the
 * entries with column <= row are read: the upper triangle may be present,
 * absent or wrong.  Within that lower triangle every row must be strictly
 * ascending by column (so no duplicates) and must store its diagonal; a device
 * check answers -EINVAL otherwise, before anything is allocated for the
 * result.  spmv_csr_transpose twice sorts the rows of a handle.  *out is a new,
 * ordinary f64 CSR handle L, M x M, whose pattern is that lower triangle, rows
 * ascending, the diagonal last in each row: launch, launch_multi, transpose,
 * trsv_analyse, download and release work on it as on any handle.  A is
 * unchanged.  The call blocks.  shift >= 0 factors A + shift * diag(A).
 * max_levels: as spmv_csr_trsv_analyse (0 = 1 << 20).
 *
 * Errors, in this order: NULL A or out, a non-finite or negative shift,
 * max_levels < 0 -EINVAL; no device -ENODEV; a dead handle -EBADF; M != N
 * -EINVAL; f32 values -ENOTSUP; after spmv_csr_release_source -ENODATA; a
 * column outside [0, N) -EDOM; the ordering / diagonal check -EINVAL; more
 * than max_levels levels -E2BIG; a failed allocation -ENOMEM.  On any error
 * nothing is created, *out is NULL, and all scratch is freed on every path.
 * M == 0 gives a valid empty handle.  A pivot that is not positive is NOT an
 * error: it is plain arithmetic (the square root of a negative number is NaN
 * and reaches exactly the dependent rows) and is counted in bad_pivots, as
 * zero_diag is in a plan.  info may be NULL.
 *
 * THE RESULT IS DEFINED TO THE BIT.  Every operation is rounded once, no fused
 * multiply-add, an IEEE division, the correctly rounded square root of
 * spmv_*_minres.  For row i with lower columns c_0 < ... < c_{n-1} < i, in
 * increasing t:
 *     j = c_t
 *     s = 0.0;  for every column m < j stored in both row i and row j, in
 *               increasing m:  s = rn(s + rn(L_im * L_jm))
 *     L_ij = rn(rn(a_ij - s) / L_jj)
 * then
 *     s = 0.0;  for t = 0 .. n-1:  s = rn(s + rn(L_it * L_it))
 *     d = rn(rn(a_ii + rn(shift * a_ii)) - s)
 *     L_ii = sqrt(d);  bad_pivots counts the rows with !(d > 0), NaN included
 * shift = 0 leaves a finite a_ii unchanged.  The sums are sequential by
 * contract (one lane walks a row, merging it with the row of each strict
 * column), so the bits depend neither on set_csr_waves_per_block, which sizes
 * the workgroups here, nor on which kernel ran a level, nor on the run.
 *
 * The levels of L's rows are those of the strict lower pattern of A, from the
 * analysis of spmv_csr_trsv_analyse, and the launches are its launch list: a
 * level of more than small_rows rows is one launch, a maximal run of thinner
 * levels one launch of ONE workgroup with a workgroup barrier between levels.
 * No waiting between workgroups of any kind; every device loop is bounded by a
 * row length.  info: levels and launches of the factorisation, entries = the
 * stored entries of L.
 */
typedef struct spmv_ic0_info {
    int levels, launches; /* of the factorisation */
    int64_t entries;      /* stored entries of L */
    int64_t bad_pivots;   /* rows whose pivot d was not > 0 (NaN included) */
} spmv_ic0_info;
int spmv_csr_ic0(const spmv_csr_dev *A, double shift, int max_levels,
                 spmv_csr_dev **out, spmv_ic0_info *info /* may be NULL */);
/*
 * Zero-fill incomplete LU A ~ L U on the device, for a matrix that is not
 * symmetric (added after 0.7; detect it by the symbol).  A: a square CSR handle
 * with f64 values.  Every row, over the WHOLE row and not only its lower part,
 * must be strictly ascending by column (so no duplicates) and must store its
 * diagonal; a device check answers -EINVAL otherwise, before anything is
 * allocated for the result.  spmv_csr_transpose twice sorts the rows of a
 * handle.  *out is a new, ordinary f64 CSR handle, M x M, with exactly A's
 * pattern: the entries with column < row are L (its unit diagonal is implied
 * and not stored), the entries with column >= row are U.  launch,
 * launch_multi, transpose, trsv_analyse, download and release work on it as on
 * any handle, and ONE handle gives both plans of the preconditioner:
 *     lower = spmv_csr_trsv_analyse(LU, 0, unit = 1)    L z' = r
 *     upper = spmv_csr_trsv_analyse(LU, 1, unit = 0)    U z  = z'
 * A is unchanged.  The call blocks.  shift >= 0 factors A + shift * diag(A).
 * max_levels: as spmv_csr_trsv_analyse (0 = 1 << 20).
 *
 * Errors, in this order: NULL A or out, a non-finite or negative shift,
 * max_levels < 0 -EINVAL; no device -ENODEV; a dead handle -EBADF; M != N
 * -EINVAL; f32 values -ENOTSUP; after spmv_csr_release_source -ENODATA; a
 * column outside [0, N) -EDOM; the ordering / diagonal check -EINVAL; more
 * than max_levels levels -E2BIG; a failed allocation -ENOMEM.  On any error
 * nothing is created, *out is NULL, and all scratch is freed on every path.
 * M == 0 gives a valid empty handle.  A pivot that is zero or not finite is
 * NOT an error: it is plain arithmetic (the inf / NaN of the division reaches
 * exactly the dependent rows) and is counted in bad_pivots.  info may be NULL.
 *
 * THE RESULT IS DEFINED TO THE BIT.  Every operation is rounded once, no fused
 * multiply-add, an IEEE division.  Row i has the columns c_0 < ... < c_{n-1},
 * its diagonal at position d, and working values w_t = a_{i,c_t}:
 *     w_d = rn(a_ii + rn(shift * a_ii))
 *     for t = 0 .. d-1, in increasing t:       j = c_t
 *         l = rn(w_t / u_jj);   w_t = l
 *         for every column m > j stored in both row i and row j:
 *             w_m = rn(w_m - rn(l * u_jm))
 * Row i of the result is w; bad_pivots counts the rows whose final w_d is 0 or
 * not finite.  shift = 0 leaves a finite a_ii unchanged.  For one t every w_m
 * is touched at most once, and t increases: each entry receives its updates in
 * increasing j, so the bits are a function of A and shift alone.  They depend
 * neither on how many lanes work on a row, nor on set_csr_waves_per_block,
 * which sizes the workgroups here, nor on which kernel ran a level, nor on the
 * run.  (Unlike spmv_csr_ic0, whose sums force one lane per row, the updates
 * of one t are independent: a group of lanes shares a row, each lane owning
 * every G-th position of it.)
 *
 * The levels of the rows are those of the strict lower pattern of A, from the
 * analysis of spmv_csr_trsv_analyse, and the launches are its launch list, as
 * for spmv_csr_ic0: a level of more than small_rows rows is one launch, a
 * maximal run of thinner levels one launch of ONE workgroup with a workgroup
 * barrier between levels.  No waiting between workgroups of any kind; every
 * device loop is bounded by a row length.  info: levels and launches of the
 * factorisation, entries = the stored entries of the result (= those of A).
 * A multicolour ordering (spmv_csr_colour, spmv_csr_permute below; the
 * colouring reads A and A^T, so the pattern need not be symmetric) brings the
 * levels of the factorisation and of both plans down to the colours.
 */
typedef struct spmv_ilu0_info {
    int levels, launches; /* of the factorisation */
    int64_t entries;      /* stored entries of LU (= those of A) */
    int64_t bad_pivots;   /* rows whose final u_ii is 0 or not finite */
} spmv_ilu0_info;
int spmv_csr_ilu0(const spmv_csr_dev *A, double shift, int max_levels,
                  spmv_csr_dev **out, spmv_ilu0_info *info /* may be NULL */);
/*
 * A multicolour ordering on the device (added after 0.7; detect it by the
 * symbols): a plan has one level per colour at most once the rows of a colour
 * are numbered together, so the launches of a triangular solve fall from the
 * depth of the natural order to a handful.  Three calls: spmv_csr_colour finds
 * the ordering, spmv_csr_permute applies it to a handle, spmv_permute_vectors
 * carries B and X between the two numberings.
 *
 * spmv_csr_colour: a distance-1 colouring of a square CSR handle (f64 or f32
 * values; only the pattern is read; rows may be unsorted and hold duplicates
 * and explicit zeros).  d_colour, d_new_of_old: M ints on the device each,
 * either may be NULL; info may be NULL.  max_rounds: 0 = the default, 4096.
 *
 * THE RESULT IS A FUNCTION OF THE PATTERN AND `seed` ALONE, defined to the
 * byte:
 *   graph     i ~ j iff i != j and (i, j) or (j, i) is stored.  An explicit
 *       zero is an edge, the diagonal is none, a duplicate is one edge.  A
 *       pattern that is not symmetric is not an error: adjacency is read from
 *       A and from A^T
 *   priority  h(i) = fmix32((uint32_t)i ^ seed), the finaliser of murmur3:
 *       h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35;
 *       h ^= h >> 16, in 32 bits.  A bijection: priorities are distinct, there
 *       is no tie rule.  (The row index as the priority would make the rounds
 *       the levels of the natural order.)
 *   colour[i] the smallest integer >= 0 that is not the colour of a neighbour
 *       j with h(j) > h(i): first-fit in decreasing priority
 *   round[i]  1 when no neighbour has a higher priority, else 1 + the largest
 *       round of those that have; info->rounds = the largest round
 *   new_of_old  the inverse of the stable sort of 0 .. M-1 by colour (rows
 *       ascending inside a colour).  In B = P A P^T a row of colour c has its
 *       strict lower entries in colours < c only, so both triangular plans of
 *       B have at most info->colours levels
 *   info      colours, rounds, widest / narrowest = the rows of the largest /
 *       smallest colour
 * The device runs Jones-Plassmann, one launch and one 4-byte read-back per
 * round, as Kahn's algorithm in spmv_csr_trsv_analyse: round r colours exactly
 * the rows with round[i] == r.  A round reads the colours earlier launches
 * wrote from one array and writes another, so a lane never reads a word that a
 * lane of its own launch writes, and info->rounds and the launch sequence are
 * reproducible.  One lane per row; the smallest free colour is found with one
 * walk of the row per window of 64 colours (a 64-bit mask), at most
 * ceil((deg + 1) / 64) of them.  Every device loop is bounded by a row length
 * or that count; no waiting between workgroups of any kind.  The order is the
 * radix sort of spmv_csr_transpose; no position comes from an atomic.
 *
 * Errors, in this order: NULL A or max_rounds < 0 -EINVAL; no device -ENODEV;
 * a dead handle -EBADF; M != N -EINVAL; after spmv_csr_release_source
 * -ENODATA; a column outside [0, N) -EDOM; more than max_rounds rounds -E2BIG
 * (a clique of n rows needs n rounds and n colours: a colouring is not for
 * that); a failed allocation -ENOMEM.  On any error the two arrays are not
 * written, *info is not written, all scratch is freed and
 * spmv_live_handles() is unchanged.  M == 0 gives 0 colours and 0 rounds.  The
 * call blocks.  Peak device memory, freed before the call returns: the pattern
 * of A^T (4 (M + 1) + 8 NZ bytes; built by the transposition of
 * spmv_csr_transpose, with its scratch of spmv_transpose_plan(M, NZ) while it
 * runs), two colour arrays and three more of M ints.
 *
 * spmv_csr_permute: *out = B = P A Q^T, a NEW, ordinary M x N handle of A's
 * value type that owns its arrays; A may be rectangular and is unchanged.
 * d_row_new_of_old: M ints on the device, p[r] = the new number of row r;
 * d_col_new_of_old: N ints, q[c] likewise; NULL = the identity.  The symmetric
 * permutation passes one array twice.
 *
 * THE RESULT IS DEFINED TO THE BYTE: row p[r] of B holds the entries of row r
 * of A with column c written as q[c], STABLY SORTED BY NEW COLUMN -- what two
 * stable sorts of A's entries in stored order give, first by q[c], then by
 * p[r].  Duplicates keep their source order and are not summed; explicit zeros
 * stay; values are moved with their bits (NaN payloads, -0.0, subnormals).  A
 * source without duplicates gives strictly ascending rows, which is what
 * spmv_csr_ic0 demands.  With both arrays NULL, B is (A^T)^T.  It is computed
 * as two transpositions with a relabelling before each; no position comes from
 * an atomic.  Every kernel id, launch_multi, spmv_hll_from_csr,
 * spmv_csr_to_f32, transpose, trsv_analyse, ic0, the solvers, download and
 * release work on B as on any handle.
 *
 * Errors: those of spmv_csr_transpose up to -ENODATA, in its order; then,
 * before anything is allocated for the result, a device check of each array,
 * rows first (the inverse is scattered and compared back): an entry outside
 * its range -EDOM, a repeated entry -EINVAL; then a column of A outside [0, N)
 * -EDOM; a failed allocation -ENOMEM.  On any error nothing is created and
 * *out is NULL.  M, N or NZ may be 0.  The call blocks.  Peak device memory
 * besides A and B, freed before the call returns: the intermediate N x M
 * matrix (4 (N + 1) + (4 + value bytes) NZ), 4 NZ for the relabelled columns
 * and the scratch of spmv_transpose_plan.
 *
 * spmv_permute_vectors: k = 1..8 interleaved vectors in the layout of
 * spmv_*_launch_multi (ldin, ldout >= k; 0 = k; only columns 0..k-1 of rows
 * 0..M-1 are touched).  inverse == 0: out[p[r], j] = in[r, j] (into the new
 * numbering); otherwise out[r, j] = in[p[r], j] (back).  The bits are moved.
 * Asynchronous on `stream` and capturable.  -EINVAL: k outside 1..8, M < 0, a
 * leading dimension below k, a NULL pointer, d_in == d_out; -ENODEV without a
 * GPU.  The array is TRUSTED (spmv_csr_permute is where a permutation is
 * checked); any other overlap of in and out is undefined.  The lanes cover
 * the k doubles of consecutive rows contiguously, so the side that is not
 * gathered moves whole cache lines.
 *
 * Not in scope: HLL and compact (16-bit) handles as input, distance-2
 * colouring, balancing the sizes of the colours, RCM or any bandwidth
 * ordering, plans inside minres, ILU with fill, and fusing a plan's solve with
 * its neighbours in the iteration.
 */
typedef struct spmv_colour_info {
    int colours, rounds;   /* rounds = kernel rounds = longest priority chain */
    int widest, narrowest; /* rows of the largest / smallest colour */
} spmv_colour_info;
int spmv_csr_colour(const spmv_csr_dev *A, uint32_t seed, int max_rounds,
                    int *d_colour /* M ints or NULL */,
                    int *d_new_of_old /* M ints or NULL */,
                    spmv_colour_info *info /* or NULL */);
int spmv_csr_permute(const spmv_csr_dev *A,
                     const int *d_row_new_of_old /* M or NULL */,
                     const int *d_col_new_of_old /* N or NULL */,
                     spmv_csr_dev **out);
int spmv_permute_vectors(const int *d_new_of_old, int M, int k, int inverse,
                         const double *d_in, int64_t ldin, double *d_out,
                         int64_t ldout, void *stream);
/*
 * The sparse product on the device: spmv_csr_spgemm makes a NEW, ordinary
 * M x N CSR handle C = A B from an M x K handle A and a K x N handle B.  Each
 * operand is f64 or f32-stored (f32 values are widened exactly); C is f64 and
 * owns all its arrays.  A may be B itself; both are unchanged and may be
 * released afterwards.  Every kernel id, launch_multi, spmv_hll_from_csr,
 * spmv_csr_to_f32, transpose, trsv_analyse, ic0 / ilu0, the solvers, download
 * and release work on C as on any handle.
 *
 * THE RESULT IS DEFINED TO THE BIT.  For row r, walk A's stored entries p of
 * that row in stored order; for each p, walk the stored entries q of B's row
 * JA_A[p] in stored order.  Each pair gives one product
 *     t = rn(AS_A[p] * AS_B[q])        with column JA_B[q].
 * Row r of C holds every column that occurs, once, in ascending order; the
 * value of a column is the SEQUENTIAL sum of its products in that walk order:
 * s = t1, then s = rn(s + ti).  The first product initialises the sum -- there
 * is no 0.0 +, so a lone -0.0 keeps its sign -- and nothing is fused: no
 * multiply-add anywhere.  An entry exists because a product exists: exact
 * cancellation and explicit zeros store a 0.0, inf * 0 stores a NaN in that
 * entry and nowhere else.  An empty row of B contributes nothing; a row with
 * no products is empty.  A may have unsorted rows, duplicates (two steps of
 * the walk) and explicit zeros.  THE ROWS OF B MUST BE STRICTLY ASCENDING BY
 * COLUMN (what spmv_csr_permute and a double spmv_csr_transpose give for a
 * source without duplicates): that is what lets the lanes of one step p write
 * distinct slots without atomics on values.  The bits do not depend on
 * scheduling, nor on which size class served a row.
 *
 * How: the rows are put into four size classes by their number of products
 * ub[r] = sum over the entries (r, k) of A of len(row k of B) (64-bit).
 * Classes 0..2 keep a row's columns in an LDS table worked by 16 lanes, a
 * wavefront or a workgroup; the last class is the fallback for wider rows (hub
 * rows, A A^T of anything with a dense column): one workgroup per row with N
 * doubles and N bits of global scratch, in batches, which costs O(N) per such
 * row.  A symbolic pass counts the distinct columns, a scan gives C's IRP, a
 * numeric pass writes JA and AS.  No workgroup waits for another.
 * spmv_spgemm_shape reports the constants (host arithmetic, no device; any
 * out-pointer may be NULL): edges[c] the largest ub of class c = 0..2,
 * tables[c] the slots of its table (twice the edge: never more than half
 * full), teams[c] its lanes, lds_bytes[c] the dynamic LDS of its workgroups,
 * and the fallback's bounds -- at most *fallback_batch rows a launch, their
 * scratch together at most *fallback_bytes (or one row's, when that is more).
 *
 * Errors, in this order: NULL A, B or out -EINVAL; no device -ENODEV; a dead
 * handle -EBADF; A.N != B.M -EINVAL; either handle after
 * spmv_csr_release_source -ENODATA; a column of A outside [0, K) or of B
 * outside [0, N) -EDOM; a row of B not strictly ascending -EINVAL (a device
 * check, before anything is allocated for the result); more than INT32_MAX
 * entries in C -EOVERFLOW (known after the symbolic pass, before C is
 * allocated); a failed allocation -ENOMEM.  On any error nothing is created,
 * *out is NULL, *info is not written, all scratch is freed and
 * spmv_live_handles() is unchanged.  M, K, N or either NZ may be 0.  The call
 * blocks.  Peak device memory besides A, B and C, freed before the call
 * returns: 16 M bytes and, when the fallback serves a row, its scratch.
 *
 * spmv_csr_galerkin: *out = PT (A P), two products and nothing else, so its
 * bits are those of the two products.  PT NULL: P^T is built by
 * spmv_csr_transpose and released.  The intermediate A P is released.  Errors
 * as the calls it is made of; info (or NULL) describes the SECOND product.
 *
 * Not in scope: a masked or filtered product, reuse of a symbolic pass, HLL
 * and compact handles as operands, an f32 result (spmv_csr_to_f32 makes one),
 * B with duplicates or unsorted rows.  (C = alpha A + beta B: spmv_csr_add
 * below.)
 */
typedef struct spmv_spgemm_info {
    int64_t products;       /* sum over entries (r,k) of A of len(row k of B) */
    int64_t widest;         /* most products of one row */
    int64_t rows_in_bin[4]; /* rows handled by each size class, last = fallback */
    int nz;                 /* entries of C */
} spmv_spgemm_info;
int spmv_csr_spgemm(const spmv_csr_dev *A, const spmv_csr_dev *B,
                    spmv_csr_dev **out, spmv_spgemm_info *info /* or NULL */);
int spmv_spgemm_shape(int64_t *edges /* [3] */, int *tables /* [3] */,
                      int *teams /* [3] */, int *lds_bytes /* [3] */,
                      int *fallback_batch, int64_t *fallback_bytes);
/* MEASUREMENT (tools/spgemm_report.py): host-clock ms of the last successful
 * spmv_csr_spgemm of this process -- [0] checks and bounds, [1] class lists
 * and symbolic pass, [2] scan, allocation of C and numeric pass, [3] the part
 * of [1] and [2] spent in the fallback's launches.  Not thread-safe. */
void spmv_spgemm_last_phases(double ms[4]);
int spmv_csr_galerkin(const spmv_csr_dev *A, const spmv_csr_dev *P,
                      const spmv_csr_dev *PT /* or NULL */, spmv_csr_dev **out,
                      spmv_spgemm_info *info /* or NULL */);
/*
 * The sparse sum on the device: spmv_csr_add makes a NEW, ordinary M x N CSR
 * handle C = alpha A + beta B from two M x N handles.  Each operand is f64 or
 * f32-stored (f32 values are widened exactly); C is f64 and owns all its
 * arrays.  B may be A itself; both are unchanged and may be released
 * afterwards.  Everything that works on a handle works on C.  The call blocks.
 *
 * THE RESULT IS DEFINED TO THE BYTE.  THE ROWS OF BOTH OPERANDS MUST BE
 * STRICTLY ASCENDING BY COLUMN (what spmv_csr_permute and a double
 * spmv_csr_transpose give for a source without duplicates).  Row r of C holds
 * the union of the two rows' columns, once each, ascending; the pattern never
 * depends on the values.  With ta = rn(alpha a) and tb = rn(beta b), the value
 * of a column is
 *     ta              stored in A only,
 *     tb              stored in B only,
 *     rn(ta + tb)     stored in both, ta the left operand.
 * Each operation is rounded once; nothing is fused: no multiply-add anywhere.
 * So cancellation and explicit zeros store a 0.0 (A - A has A's pattern full
 * of +0.0), a lone -0.0 under alpha = 1 keeps its sign, alpha == 0 is no
 * special case (the union stays, 0 * inf is a NaN in that entry only), and
 * inf - inf is a NaN in that entry and nowhere else.  The bytes do not depend
 * on scheduling, nor on which size class served a row.
 *
 * How: two passes over the rows, each a merge of two ascending index lists by
 * rank.  The count pass reads only IRP and JA and writes len_A + len_B -
 * matches per row; the exclusive scan of the transposition makes C's IRP; the
 * total comes back in one small read-back before C is allocated; the fill
 * pass writes JA and AS.  Every position is computed, none comes from an
 * atomic: entry i of A's row lands at i + lower_bound_B(column) - (matched
 * entries of A before i), an unmatched entry j of B at j +
 * lower_bound_A(column) - (matched entries of B before j); a matched pair is
 * written by its A-side lane.  Every slot of C is written exactly once, by
 * one lane.  No workgroup waits for another.  Two size classes by len_A(r) +
 * len_B(r): up to *edge a group of lanes per row (its width one of widths[],
 * the smallest that is not below the mean (NZ_A + NZ_B) / M), beyond it a
 * workgroup of *threads lanes per row; both walk a row in chunks of their
 * width and carry the matched-prefix count across chunks.  spmv_add_shape
 * reports these constants (host arithmetic, no device; any out-pointer may be
 * NULL; widths has room for 8 ints, *n_widths of them are written).
 *
 * spmv_add_set_class is for MEASUREMENT and for the tests: 0 the rule above,
 * 1 every row by lane groups, 2 every row by the workgroup class.  Returns the
 * previous mode, -EINVAL for another value.  The bytes of C do not depend on
 * it.  Not thread-safe.  Mode 2 is one workgroup per row, whatever its length:
 * meant for matrices of at most 2^24 rows (a larger launch is refused by the
 * runtime, -EINVAL, and creates nothing).  spmv_add_last_phases: host-clock ms of the last
 * successful spmv_csr_add of this process -- [0] checks, [1] count and scan,
 * [2] allocation, fill and the finishing of the handle.  Not thread-safe.
 *
 * Errors, in this order: NULL A, B or out, or a non-finite alpha or beta
 * -EINVAL; no device -ENODEV; a dead handle -EBADF; shapes differ -EINVAL;
 * either handle after spmv_csr_release_source -ENODATA; a column outside
 * [0, N) -EDOM; a row of either operand not strictly ascending -EINVAL (a
 * device check, before anything is allocated for the result); more than
 * INT32_MAX entries in C -EOVERFLOW (before C is allocated); a failed
 * allocation -ENOMEM.  On any error nothing is created, *out is NULL, *info
 * is not written, all scratch is freed and spmv_live_handles() is unchanged.
 * M, N or either NZ may be 0.  Peak device memory besides A, B and C, freed
 * before the call returns: about 8 M bytes.
 *
 * Two companions, each one streaming kernel and a new ordinary f64 handle:
 *
 * spmv_csr_from_diag: the M x M handle with the one entry (i, i) per row, its
 * value the bits of d_diag[i] (a NaN or 0.0 is stored as it is), or 1.0 when
 * d_diag is NULL.  M == 0 is fine; M < 0 or NULL out -EINVAL; no device
 * -ENODEV.  A - sigma I is spmv_csr_add(1, A, -sigma, I).
 *
 * spmv_csr_scale: a handle with A's IRP and JA byte for byte (rows may be
 * unsorted; duplicates and explicit zeros are kept) and the values
 * rn(rn(l_i a) r_j) for entry (i, j); with d_left only rn(l_i a), with
 * d_right only rn(a r_j).  d_left holds M, d_right N doubles on the device.
 * A may be f32-stored and of any shape.  Both vectors NULL -EINVAL; otherwise
 * the errors of spmv_csr_to_f32 (-EINVAL, -ENODEV, -EBADF, -ENODATA,
 * -ENOMEM), and -EDOM when d_right is given and a column lies outside [0, N).
 *
 * Not in scope: a sum into an existing handle or the reuse of a pattern for
 * new values, operands with unsorted rows or duplicates, HLL, compact or f32
 * results, pruning of zeros, a masked sum, more than two operands.
 */
typedef struct spmv_add_info {
    int nz;                 /* entries of C */
    int64_t matched;        /* columns stored in both operands, over all rows */
    int64_t widest;         /* largest len_A(r) + len_B(r) */
    int64_t rows_in_bin[2]; /* rows served by each size class */
} spmv_add_info;
int spmv_csr_add(double alpha, const spmv_csr_dev *A, double beta,
                 const spmv_csr_dev *B, spmv_csr_dev **out,
                 spmv_add_info *info /* or NULL */);
int spmv_add_shape(int64_t *edge, int *widths /* [8] */, int *n_widths,
                   int *threads);
int spmv_add_set_class(int mode);
void spmv_add_last_phases(double ms[3]);
int spmv_csr_from_diag(int M, const double *d_diag /* device, or NULL: 1.0 */,
                       spmv_csr_dev **out);
int spmv_csr_scale(const spmv_csr_dev *A, const double *d_left,
                   const double *d_right, spmv_csr_dev **out);
/* Build a synthetic matrix (spmv_synth.h) directly in device memory. */
int spmv_csr_generate(int kind, int M, int N, int K, int64_t W, int64_t row0,
                      uint64_t seed, spmv_csr_dev **out);
/* y[0..M) = A * x on `stream`; asynchronous. kernel = 0..4 (hip_csr.h).
 * Launches of one handle must be stream-ordered (the sweep schedule of the
 * blocked path keeps per-handle phase counters); different handles are
 * independent.
 * opts.variant (tuning): see spmv_launch_opts. */
int spmv_csr_launch(const spmv_csr_dev *A, int kernel,
                    const spmv_launch_opts *opts, const double *d_x,
                    double *d_y, void *stream);
/* rows [row_begin, row_end) only; d_y still indexed from row 0.  The stream
 * kernel (4) owns a row-block table of the WHOLE matrix: on a proper sub-range
 * the sub-wave kernel (2) runs instead -- correct, but without the stream
 * kernel's long-row handling; callers that chunk a shard (dist.py, mgpu.hip)
 * therefore launch whole shards when the pick is kernel 4 */
int spmv_csr_launch_rows(const spmv_csr_dev *A, int kernel,
                         const spmv_launch_opts *opts, const double *d_x,
                         double *d_y, int row_begin, int row_end,
                         void *stream);
int spmv_csr_build_panels(spmv_csr_dev *A, int panel_cols);
int spmv_csr_build_panels_opts(spmv_csr_dev *A, const spmv_panel_opts *opts);
/* schedule the NEXT spmv_*_build_panels() calls prepare: 1 = "sweep" (one
 * persistent launch over all panels with phase counters; for rows that reach
 * far beyond an L2 of x; initial value), 2 = "chain" (one launch, a workgroup
 * walks its tile's non-empty buckets; for banded / clustered / skewed
 * matrices), 0 = "steps" (same layout as chain, one launch per non-empty
 * panel step).  -EINVAL otherwise.  spmv_*_autotune tries them all and
 * spmv_*_build_panels_opts / _as name the schedule explicitly. */
int spmv_set_panel_schedule(int sched);
/* geometry of the blocked copy: kernel launches per SpMV (steps), row
 * tiles, column panels, entries kept; -ENOENT when it is not built */
int spmv_csr_panels_info(const spmv_csr_dev *A, int *steps, int *tiles,
                         int *panels, int64_t *entries);
/* blocked copy with the schedule and tile height of `model`'s (shards of one
 * matrix: autotune one, build the others alike) */
int spmv_csr_build_panels_like(spmv_csr_dev *A, const spmv_csr_dev *model);
/* schedule of the blocked copy: 0 steps, 1 sweep, 2 chain; -ENOENT if none */
int spmv_csr_panels_schedule(const spmv_csr_dev *A);
int spmv_csr_panels_tile_rows(const spmv_csr_dev *A); /* -ENOENT if none */
/* one line of text: schedule, tiles x rows, panels x columns, bucket order,
 * launch shape of the blocked copy; -ENOENT if none */
int spmv_csr_panels_describe(const spmv_csr_dev *A, char *buf, size_t len);
/* blocked copy in an explicit schedule (0 steps, 1 sweep, 2 chain) and tile
 * height (0: default; sweep sizes its own tiles): the ranks of a multi-GPU
 * job build what rank 0 tuned */
int spmv_csr_build_panels_as(spmv_csr_dev *A, int panel_cols, int sched,
                             int tile_rows);
/* keep only the blocked copy: frees JA/AS, so the handle costs the HBM of
 * the format it came from (12 B per entry).  Afterwards only the PANELS
 * kernel id runs; the direct kernels, download, conversion and further
 * builds return -ENODATA.  -ENOENT when no blocked copy was built. */
int spmv_csr_release_source(spmv_csr_dev *A);
int spmv_csr_shape(const spmv_csr_dev *A, int *M, int *N, int64_t *NZ);
int64_t spmv_csr_algorithmic_bytes(const spmv_csr_dev *A);
/* download the device arrays into a host CSR (tests; generated matrices) */
int spmv_csr_download(const spmv_csr_dev *A, sparse_csr **out);
void spmv_csr_release(spmv_csr_dev *A);

/* ---- HLL handle ---- */
typedef struct spmv_hll_dev spmv_hll_dev;

int spmv_hll_upload(const sparse_hll *H, int is_col_major, spmv_hll_dev **out);
/* values stored as fp32 (see spmv_csr_upload_f32) */
int spmv_hll_upload_f32(const sparse_hll *H, int is_col_major,
                        spmv_hll_dev **out);
int spmv_hll_value_bytes(const spmv_hll_dev *H); /* 8 or 4 */
/*
 * Index type of a column-major handle (added after 0.7; spmv_version() is
 * unchanged, callers detect the feature by the symbol).  4: JA int32[S] as
 * above.  2: a "compact" handle -- one base column per hack block and a 16-bit
 * offset per slot,
 *     column of slot t of block b = base[b] + off16[t],
 * 10 bytes per slot instead of 12 (f64 values), 6 instead of 8 (f32).  For
 * matrices whose hack blocks (32 consecutive rows) each keep their columns in
 * a window of 65 536: bands, 2-D stencils, 3-D stencils while
 * 2 nx ny < 65 536.
 *
 * spmv_hll_to_index16 makes a new compact handle on the device with the
 * pattern, the slot order, off[] and the value type (f64 or f32) of H; H stays
 * valid.  base[b] is the smallest column among the non-pad slots of block b (0
 * for a block of width 0).  A pad slot whose rewritten column lies outside
 * [base, base + 65535] -- the column-0 pad of an empty row -- is stored as
 * offset 0.  Errors (after the dead-handle contract below; without a GPU
 * -ENODEV): -EINVAL row-major or already compact source; -ENODATA source
 * after spmv_hll_release_source(); -ENOTSUP a hack block wider than 512
 * columns (hub rows: their side launch is not built for compact handles);
 * -ERANGE the valid columns of some block span more than 65 536.  Nothing is
 * created on any error.
 *
 * Order: for finite x, y of a compact handle has the bits of
 * spmv_hll_launch(H, 1) (and so of kernel 2) on its source, for either kernel
 * id, every workgroup order, every waves_per_block and both value types:
 * acc = 0.0, one fused multiply-add per column in column order, pads
 * included.  NON-FINITE x: a pad's product is 0.0 * x[its column]; on a
 * compact handle a non-finite x[base[b]] therefore reaches the EMPTY rows of
 * block b (NaN instead of 0.0), where a 4-byte handle lets a non-finite x[0]
 * reach them.
 *
 * On a compact handle: spmv_hll_launch / _launch_blocks / _time with kernel
 * ids 1 and 2 (ids 0, 3 and PANELS: -EINVAL), streams and graph capture,
 * spmv_hll_autotune (kernels 1 / 2 in the three orders; allow_panels ignored,
 * one line in the tune log says so), _shape, _value_bytes, _algorithmic_bytes
 * / _kernel_bytes ((2 + value_bytes) S + 4 nb for the bases + 12 nb + 8 M +
 * 8 N), release / release_checked.  spmv_hll_build_panels*,
 * spmv_hll_launch_multi, spmv_hll_multi_bytes, spmv_hll_launch_axpby,
 * spmv_hll_axpby_bytes, spmv_hll_cg, spmv_hll_pcg, spmv_hll_bicgstab,
 * spmv_hll_cgls (in either position), spmv_hll_minres and spmv_hll_diag:
 * -ENOTSUP.  The handle owns no 4-byte JA and no pad bitmap.  The one-shot seam, the reference ABI names
 * and spmv_mgpu.h create 4-byte handles only.
 */
int spmv_hll_to_index16(const spmv_hll_dev *H, spmv_hll_dev **out);
int spmv_hll_index_bytes(const spmv_hll_dev *H); /* 4 or 2 */
/* tests: base[nb], off16[slots] as stored (-EINVAL on a 4-byte handle) */
int spmv_hll_download_index16(const spmv_hll_dev *H, int *base, uint16_t *off16);
/* CSR -> HLL conversion on the device (reference hll.c:19-95 semantics,
 * pads already rewritten); the CSR handle stays valid.  The HLL handle has
 * the CSR handle's value type. */
int spmv_hll_from_csr(const spmv_csr_dev *A, int is_col_major,
                      spmv_hll_dev **out);
/* kernel = 0..3 (hip_hll.h); the handle's layout must match the kernel
 * (0,3 row-major; 1,2 col-major) else -EINVAL. */
int spmv_hll_launch(const spmv_hll_dev *H, int kernel,
                    const spmv_launch_opts *opts, const double *d_x,
                    double *d_y, void *stream);
/* hack blocks [blk_begin, blk_end) only */
int spmv_hll_launch_blocks(const spmv_hll_dev *H, int kernel,
                           const spmv_launch_opts *opts, const double *d_x,
                           double *d_y, int blk_begin, int blk_end,
                           void *stream);
/* HLL source: pad slots (JA == -1 on the host; remembered in a bitmap when
 * the pads are rewritten at upload) are dropped; explicit zeros are kept,
 * as from a CSR source */
int spmv_hll_build_panels(spmv_hll_dev *H, int panel_cols);
int spmv_hll_build_panels_opts(spmv_hll_dev *H, const spmv_panel_opts *opts);
int spmv_hll_panels_info(const spmv_hll_dev *H, int *steps, int *tiles,
                         int *panels, int64_t *entries);
int spmv_hll_build_panels_like(spmv_hll_dev *H, const spmv_hll_dev *model);
int spmv_hll_panels_schedule(const spmv_hll_dev *H);
/* the blocked copy's layout as build options + the launch's waves hint (set
 * o->struct_size first; -ENOENT: no copy): spmv_*_build_panels_opts(o) and
 * spmv_*_panels_set_waves(waves) on a handle of the same matrix rebuild
 * exactly what spmv_*_autotune settled on */
int spmv_csr_panels_layout(const spmv_csr_dev *A, spmv_panel_opts *o, int *waves);
int spmv_hll_panels_layout(const spmv_hll_dev *H, spmv_panel_opts *o, int *waves);
int spmv_csr_panels_set_waves(spmv_csr_dev *A, int waves); /* 0..16 */
int spmv_hll_panels_set_waves(spmv_hll_dev *H, int waves);
/* sweep copies.  fit_steps: the steps one launch takes over all buckets with
 * the chunk of the built-in launch shape and with the 4608-slot chunk, counted
 * on the device at the end of the build; a copy whose second count is at
 * least 10 % lower launches the 4608-slot shape unless waves_per_block or
 * the variant ask for another.  set_fit_steps(h, 0, 0) makes the copy one
 * whose steps were never counted: the built-in shape (this is what a
 * layout string without chunk_fit rebuilds).  panels_plan: threads per
 * workgroup, groups of 4 entries per lane and ordered additions (0 / 1) of
 * the tile kernel that a blocked launch with `opts` (may be NULL) would run;
 * nothing is launched.  -ENOENT: no copy. */
int spmv_csr_panels_fit_steps(const spmv_csr_dev *A, int64_t *builtin, int64_t *fit);
int spmv_hll_panels_fit_steps(const spmv_hll_dev *H, int64_t *builtin, int64_t *fit);
int spmv_csr_panels_set_fit_steps(spmv_csr_dev *A, int64_t builtin, int64_t fit);
int spmv_hll_panels_set_fit_steps(spmv_hll_dev *H, int64_t builtin, int64_t fit);
int spmv_csr_panels_plan(const spmv_csr_dev *A, const spmv_launch_opts *opts,
                         int *threads, int *groups, int *ordered);
int spmv_hll_panels_plan(const spmv_hll_dev *H, const spmv_launch_opts *opts,
                         int *threads, int *groups, int *ordered);
int spmv_hll_panels_tile_rows(const spmv_hll_dev *H);
int spmv_hll_panels_describe(const spmv_hll_dev *H, char *buf, size_t len);
int spmv_hll_build_panels_as(spmv_hll_dev *H, int panel_cols, int sched,
                             int tile_rows);
int spmv_hll_release_source(spmv_hll_dev *H);
int spmv_hll_shape(const spmv_hll_dev *H, int *M, int *N, int64_t *NZ,
                   int *num_blocks, int64_t *slots, int *is_col_major);
int64_t spmv_hll_algorithmic_bytes(const spmv_hll_dev *H);
/* bytes one launch of `kernel` must move: spmv_hll_algorithmic_bytes (12 per
 * STORED slot, 8 in an f32 handle) for the direct kernels; for SPMV_HLL_KERNEL_PANELS, whose
 * copy stores no padding, 12 per true entry (+ 12 nb + 8 M + 8 N as before).
 * Equal when the format pads nothing (the headline matrix). */
int64_t spmv_hll_kernel_bytes(const spmv_hll_dev *H, int kernel);
void spmv_hll_release(spmv_hll_dev *H);

/*
 * Timed loops: `warmup` untimed launches, then `iters` launches each
 * bracketed by its own hipEvent pair on `stream`; ms_each[iters] receives
 * the per-launch kernel times.  flush_bytes > 0 streams a scratch buffer of
 * that size between iterations (outside the timed region) so that matrices
 * smaller than the 256 MiB Infinity Cache are read from HBM.  The sweep only
 * READS the scratch buffer (no dirty lines whose write-back would overlap the
 * timed launch); opts.variant bit 29 selects the read-modify-write sweep of
 * rounds 1 / 2 for comparison.
 */
int spmv_csr_time(const spmv_csr_dev *A, int kernel,
                  const spmv_launch_opts *opts, const double *d_x, double *d_y,
                  int warmup, int iters, size_t flush_bytes, double *ms_each,
                  void *stream);
int spmv_hll_time(const spmv_hll_dev *H, int kernel,
                  const spmv_launch_opts *opts, const double *d_x, double *d_y,
                  int warmup, int iters, size_t flush_bytes, double *ms_each,
                  void *stream);

/*
 * Several right-hand sides in one launch (added after 0.7; spmv_version() is
 * unchanged, callers detect the feature by the symbol).
 *
 * Y[r*ldy + j] = sum_c A[r][c] * X[c*ldx + j],  j = 0..k-1,  1 <= k <= 8.
 * X: N rows of ldx doubles, Y: M rows of ldy doubles (row-major,
 * "interleaved"); ldx, ldy >= k (0 = k).  Only columns 0..k-1 of a row of Y
 * are written.  X and Y must not overlap.  Whole matrix only.  Asynchronous
 * on `stream`, stream-ordered and capturable like every other launch.  The
 * matrix is read once for all k products and the k values of a column are one
 * request to one cache line (16-byte loads of pairs, whatever ldx and the
 * alignment of d_X are).  Both value types of a handle.
 *
 * Order: column j of Y has the bits of spmv_csr_launch(A, 2, opts with the
 * same group) / spmv_hll_launch(H, 1) on the contiguous vector X[:, j], for
 * every row of at most 2048 entries / hack block of at most 512 columns;
 * longer rows and wider blocks are summed by one workgroup each in a fixed
 * order (reproducible, within 1e-12 of the row scale sum |a x|).
 *
 * opts may be NULL; waves_per_block and (CSR) group as in the single-vector
 * launch; variant and reserved must be 0 (the workgroup order is the
 * handle's and never changes a result).  -EINVAL: NULL handle, k outside
 * 1..8, ldx / ldy below k, NULL d_X / d_Y, waves_per_block outside 0..16, a
 * group that is not 0, 2, 4, 8, 16 or 32, a nonzero variant / reserved word,
 * a row-major HLL handle.  -EBADF: not a live handle (-ENODEV when there is
 * no GPU at all).  -ENODATA after spmv_*_release_source().  M == 0: returns 0
 * and launches nothing.
 */
int spmv_csr_launch_multi(const spmv_csr_dev *A, const spmv_launch_opts *opts,
                          int k, const double *d_X, int64_t ldx,
                          double *d_Y, int64_t ldy, void *stream);
int spmv_hll_launch_multi(const spmv_hll_dev *H, const spmv_launch_opts *opts,
                          int k, const double *d_X, int64_t ldx,
                          double *d_Y, int64_t ldy, void *stream);
/* bytes one launch_multi must move: (4 + value_bytes) * NZ (slots for HLL) +
 * the index / offset arrays as in spmv_*_algorithmic_bytes + 8*k*M + 8*k*N;
 * -EINVAL for k outside 1..8 */
int64_t spmv_csr_multi_bytes(const spmv_csr_dev *A, int k);
int64_t spmv_hll_multi_bytes(const spmv_hll_dev *H, int k);

/*
 * Y = alpha * A X + beta * Y in place, for the same 1..8 interleaved vectors
 * (added after 0.7; spmv_version() is unchanged, detect it by the symbol):
 *
 * Y[r*ldy + j] = alpha * (sum_c A[r][c] * X[c*ldx + j]) + beta * Y[r*ldy + j].
 *
 * Layout, strides (0 = k), opts, the handle checks and every error code are
 * those of spmv_*_launch_multi above -- one function checks both (a compact
 * handle: -ENOTSUP; a row-major HLL handle: -EINVAL; after
 * spmv_*_release_source(): -ENODATA; not a live handle: -EBADF / -ENODEV;
 * M == 0: returns 0 and launches nothing).  The kernels are launch_multi's
 * with an epilogue where the store is, in the lane or workgroup that owns the
 * element: one pass over the matrix, no second pass over Y.  alpha and beta
 * are passed by value and any double is accepted; a captured graph holds the
 * values it was captured with.
 *
 * Result contract, to the bit.  Let s be what spmv_*_launch_multi stores for
 * the element on the same handle with the same opts (every row: the sums of
 * long rows and wide hack blocks are fixed-order too), rn() one rounding to
 * fp64:
 *   beta == 0:  Y = rn(alpha * s).  The old Y is NOT read: a NaN or inf in it
 *               does not propagate and the memory may be uninitialised.
 *   beta != 0:  Y = rn(rn(alpha * s) + rn(beta * y_old)): two products and
 *               one sum, each rounded once, no fused multiply-add across them.
 * So alpha = 1, beta = 0 gives the bits of launch_multi, and alpha = -1,
 * beta = 1 gives y_old - s correctly rounded.  There is no special case for
 * alpha == 0: the matrix is still read and 0 * NaN is NaN.  Only columns
 * 0..k-1 of rows 0..M-1 of Y are read or written.  X and Y must not overlap.
 */
int spmv_csr_launch_axpby(const spmv_csr_dev *A, const spmv_launch_opts *opts,
                          int k, double alpha, double beta,
                          const double *d_X, int64_t ldx,
                          double *d_Y, int64_t ldy, void *stream);
int spmv_hll_launch_axpby(const spmv_hll_dev *H, const spmv_launch_opts *opts,
                          int k, double alpha, double beta,
                          const double *d_X, int64_t ldx,
                          double *d_Y, int64_t ldy, void *stream);
/* bytes one launch_axpby must move: spmv_*_multi_bytes(k), and 8*k*M more
 * when reads_y != 0 (beta != 0: Y is read as well as written); -EINVAL and
 * -ENOTSUP where multi_bytes answers so */
int64_t spmv_csr_axpby_bytes(const spmv_csr_dev *A, int k, int reads_y);
int64_t spmv_hll_axpby_bytes(const spmv_hll_dev *H, int k, int reads_y);

/*
 * Conjugate gradients on the device for A X = B (added after 0.7;
 * spmv_version() is unchanged, detect it by the symbol).  A: square, symmetric
 * positive definite, a CSR or column-major HLL handle of either value type.
 * X, B: k = 1..8 interleaved vectors as in spmv_*_launch_multi; the k systems
 * are independent: each column has its own scalars, its own convergence and
 * its own status, and one launch_multi per iteration serves them all.  No
 * preconditioner here: spmv_*_pcg below takes a diagonal one.
 *
 * d_X holds the initial guess on entry and the iterate on return; d_B is not
 * written.  ldb, ldx >= k (0 = k); only columns 0..k-1 of rows 0..M-1 of X
 * are read or written.  d_work == NULL: the library allocates and frees
 * spmv_cg_work_bytes(M, k) bytes of device memory for the call; otherwise the
 * caller's buffer is used (8-byte aligned, at least that many bytes, else
 * -EINVAL) and a caller who solves repeatedly pays no allocation.  info: k
 * entries in host memory.
 *
 * The call enqueues on `stream` and synchronises that stream at its checks:
 * it BLOCKS and returns once the last check is done.  It cannot be captured
 * into a graph: a stream that is capturing gets -EBUSY and nothing is
 * enqueued.  The host enqueues check_every iterations (0 = 8), copies back k
 * status words and synchronises, stops when no column is running or maxit is
 * reached, and never enqueues an iteration beyond maxit.
 *
 * Checks: the handle, opts, k, the strides and the two pointers are checked by
 * the function that serves launch_multi and launch_axpby, with the same
 * answers (dead handle -EBADF / -ENODEV, compact handle -ENOTSUP, row-major
 * HLL -EINVAL, after spmv_*_release_source() -ENODATA).  Additionally
 * -EINVAL: M != N, a tol that is negative or NaN, maxit < 0, check_every < 0,
 * NULL info.  M == 0: returns 0 with every info[j] = {0, 0, 0.0, 0.0}.
 *
 * Result contract, to the bit.  Every operation below is rounded once, no
 * fused multiply-add crosses a * and a +.  tol2 = tol * tol on the host.
 *
 *   R = B;  R = (-1) A X + 1 R  by the handle's launch_axpby;  P = R
 *   bb = dot(B, B);  rr = dot(R, R)
 *   column j: status 2 (iterations 0) if rr_j or bb_j is not finite, else
 *             converged (iterations 0) if rr_j <= tol2 * bb_j, else running
 *   repeat at most maxit times:
 *       Q = A P  by the handle's launch_multi (all k columns, same opts)
 *       pq = dot(P, Q)
 *       running column with !(pq_j > 0 and finite): status 2, frozen
 *       running column: alpha = rr / pq;  X = X + alpha * P;
 *                       R = R - alpha * Q;  iterations += 1
 *       rn = dot(R, R)
 *       running column: rn_j <= tol2 * bb_j -> status 0, frozen (rr_j = rn_j)
 *                       rn_j not finite     -> status 2, frozen
 *       running column: beta = rn / rr;  P = R + beta * P;  rr = rn
 *   columns still running: status 1
 *
 * X, R, P and rr of a frozen column are never written again, whatever happens
 * to the other columns and however many more iterations were enqueued before
 * the host noticed.  So X, iterations, status and rr do not depend on
 * check_every, on d_work being NULL or supplied, or on waves_per_block, and
 * column j of a k-column solve has the bits of the k = 1 solve of B[:, j],
 * X0[:, j].
 *
 * dot(u, v), per column, in an order that depends on M alone (not on k, the
 * device or a launch shape): with NWG workgroups of T threads
 * (spmv_cg_dot_shape: 1024, 256), element i belongs to slot i mod (NWG * T);
 * a slot starts at 0.0 and adds rn(u_i * v_i) in increasing i; the T slots
 * t = 0..T-1 of workgroup w (slots w T + t) are combined by a halving tree,
 * s[t] += s[t + h] for h = T/2 .. 1; the NWG workgroup sums by the same tree.
 */
typedef struct spmv_cg_info {
    int status;      /* 0 converged, 1 maxit reached, 2 breakdown */
    int iterations;  /* updates of x applied to this column */
    double rr;       /* last r.r of the recurrence for this column */
    double bb;       /* b.b */
} spmv_cg_info;

int64_t spmv_cg_work_bytes(int M, int k); /* -EINVAL: M < 0, k outside 1..8 */
void spmv_cg_dot_shape(int *workgroups, int *threads);
int spmv_csr_cg(const spmv_csr_dev *A, const spmv_launch_opts *opts, int k,
                const double *d_B, int64_t ldb, double *d_X, int64_t ldx,
                double tol, int maxit, int check_every,
                void *d_work, size_t work_bytes,
                spmv_cg_info *info, void *stream);
int spmv_hll_cg(const spmv_hll_dev *H, const spmv_launch_opts *opts, int k,
                const double *d_B, int64_t ldb, double *d_X, int64_t ldx,
                double tol, int maxit, int check_every,
                void *d_work, size_t work_bytes,
                spmv_cg_info *info, void *stream);

/*
 * The diagonal of a handle (added after 0.7; detect it by the symbol).
 * d_out[r], r < min(M, N), is the fp64 sum of the stored entries of row r
 * whose column is r: the sum starts from 0.0, an f32 handle widens each value
 * first.  A row that stores no diagonal entry gives 0.0; a row that stores it
 * once gives that value exactly; a row that stores it more than once gives a
 * sum whose order is fixed for the handle and does not depend on the launch
 * (which order is not specified).  HLL pads carry the value 0.0 and v + 0.0
 * keeps the bits of v, so a column-major HLL handle gives the bits of the CSR
 * handle it was made from.  invert != 0 stores rn(1.0 / d) instead -- one
 * correctly rounded division, inf for a zero diagonal: the Jacobi
 * preconditioner spmv_*_pcg takes.  Only d_out[0 .. min(M, N)) is written.
 * Asynchronous on `stream`, capturable.
 *
 * The handle is checked by the function that serves launch_multi, launch_axpby
 * and cg, with the same answers: dead handle -EBADF / -ENODEV, compact handle
 * -ENOTSUP, row-major HLL -EINVAL, after spmv_*_release_source() -ENODATA.
 * NULL d_out: -EINVAL.  M == 0: returns 0.
 */
int spmv_csr_diag(const spmv_csr_dev *A, double *d_out, int invert,
                  void *stream);
int spmv_hll_diag(const spmv_hll_dev *H, double *d_out, int invert,
                  void *stream);

/*
 * Preconditioned conjugate gradients with a diagonal preconditioner (added
 * after 0.7; detect it by the symbol): spmv_*_cg with z = M^-1 r applied as
 * z_i = minv_i * r_i.  d_minv: M doubles, one per row, shared by the k columns,
 * never written.  Any positive vector is allowed; spmv_*_diag(invert = 1)
 * gives Jacobi.
 *
 * d_X, d_B, the strides, d_work (spmv_pcg_work_bytes(M, k) bytes: the state,
 * three sets of partial sums, R, P and Q), the blocking, -EBUSY on a capturing
 * stream, check_every, maxit, M == 0 and the argument checks are those of
 * spmv_*_cg above, word for word.  One check is added: NULL d_minv, -EINVAL.
 *
 * Result contract, to the bit.  Every operation is rounded once, no fused
 * multiply-add; dot is the dot of spmv_cg_dot_shape; z(R) is the vector with
 * z_i = rn(minv_i * r_i) in every column.
 *
 *   R = B;  R = (-1) A X + 1 R  by launch_axpby;  P = z(R)
 *   bb = dot(B, B);  rr = dot(R, R);  rz = dot(R, z(R))
 *   column j: status 2 (iterations 0) if rr, bb or rz is not finite,
 *             else converged (iterations 0) if rr <= tol2 * bb,
 *             else status 2 if not rz > 0,  else running
 *   repeat at most maxit times:
 *       Q = A P  by launch_multi;  pq = dot(P, Q)
 *       running column with !(pq > 0 and finite): status 2, frozen
 *       running column: alpha = rz / pq;  X = X + alpha * P;
 *                       R = R - alpha * Q;  iterations += 1
 *       rn = dot(R, R);  zn = dot(R, z(R))          (the updated R)
 *       running column: rn <= tol2 * bb -> status 0, frozen (rr = rn)
 *                       rn not finite or !(zn > 0 and finite)
 *                                       -> status 2, frozen
 *       running column: beta = zn / rz;  P = z(R) + beta * P;
 *                       rr = rn;  rz = zn
 *   columns still running: status 1
 *
 * Frozen columns are never written again, exactly as in spmv_*_cg: X, the
 * iteration counts, the statuses and rr do not depend on check_every, on the
 * owner of the work buffer, on waves_per_block, or on the other columns.
 * minv of all 1.0 gives z(R) = R and rz = rr, every test above reduces to
 * cg's, and the call returns the bits of spmv_*_cg on the same handle (X,
 * status, iterations, rr, bb): a property of the contract, not a special
 * case.  Z is never stored: z(R) is recomputed in the kernels that use it.
 */
int64_t spmv_pcg_work_bytes(int M, int k); /* -EINVAL: M < 0, k outside 1..8 */
int spmv_csr_pcg(const spmv_csr_dev *A, const spmv_launch_opts *opts, int k,
                 const double *d_B, int64_t ldb, double *d_X, int64_t ldx,
                 const double *d_minv,
                 double tol, int maxit, int check_every,
                 void *d_work, size_t work_bytes,
                 spmv_cg_info *info, void *stream);
int spmv_hll_pcg(const spmv_hll_dev *H, const spmv_launch_opts *opts, int k,
                 const double *d_B, int64_t ldb, double *d_X, int64_t ldx,
                 const double *d_minv,
                 double tol, int maxit, int check_every,
                 void *d_work, size_t work_bytes,
                 spmv_cg_info *info, void *stream);

/*
 * Conjugate gradients preconditioned by triangular plans (added after 0.7;
 * detect it by the symbol): spmv_*_pcg with Z = z(R) made by spmv_trsv_solve
 * instead of a multiplication by minv, in two steps:
 *     spmv_trsv_solve(first, k, R -> Z, no scale)
 *     if second is not NULL: spmv_trsv_solve(second, k, Z -> Z in place,
 *                                            d_scale)
 * always for all k columns, with an opts that carries only the caller's
 * waves_per_block.  Symmetric Gauss-Seidel is (the lower plan of A, the upper
 * plan of A, diag(A)); IC(0) is (the lower plan of L = spmv_csr_ic0(A), the
 * upper plan of spmv_csr_transpose(L), NULL).  The plans and d_scale are never
 * written and may serve any number of solves.
 *
 * Everything else is spmv_*_pcg word for word: the handles, the interleaved
 * k = 1..8 systems, the blocking, -EBUSY on a capturing stream, check_every,
 * maxit, M == 0, the records and the frozen-column rule.  d_work:
 * spmv_pcg_trsv_work_bytes(M, k) bytes, pcg's and one vector Z (ld = k).
 * Checks added after pcg's, in this order: NULL first -EINVAL; d_scale without
 * second -EINVAL; a dead plan -EBADF; a plan whose M is not A's -EINVAL.
 *
 * The recurrence is that of spmv_*_pcg with the stored Z where pcg has z(R):
 * P = Z;  rz = dot(R, Z);  after the update rn = dot(R, R), Z = z(R),
 * zn = dot(R, Z), beta = zn / rz, P = Z + beta * P -- the same classification
 * ladder, the same dot order, every operation rounded once.  Z is scratch: a
 * frozen column's Z may hold anything, and nothing of it reaches X, R, P or
 * the state.  Two properties of the contract, not special cases: a plan of the
 * identity (or a unit plan without strict entries) returns the bits of
 * spmv_*_cg; a plan of a diagonal matrix of powers of two returns the bits of
 * spmv_*_pcg with minv = 1 / d.  A NaN in a factor makes rz NaN: status 2 with
 * 0 iterations.
 *
 * The price: every iteration adds the launches of the plans (spmv_trsv_info),
 * 3.4-4.4 us each.  On a stencil in natural order that is far more than the
 * iteration of spmv_*_pcg it replaces; it pays where the level count is small
 * (a multicolour ordering: spmv_csr_colour and spmv_csr_permute above make
 * one) or the iteration count falls by more than the
 * launches cost (profiles/ic0.md).
 */
int64_t spmv_pcg_trsv_work_bytes(int M, int k); /* as spmv_pcg_work_bytes */
int spmv_csr_pcg_trsv(const spmv_csr_dev *A, const spmv_launch_opts *opts,
                      int k, const double *d_B, int64_t ldb, double *d_X,
                      int64_t ldx, const spmv_trsv_plan *first,
                      const spmv_trsv_plan *second, const double *d_scale,
                      double tol, int maxit, int check_every, void *d_work,
                      size_t work_bytes, spmv_cg_info *info, void *stream);
int spmv_hll_pcg_trsv(const spmv_hll_dev *H, const spmv_launch_opts *opts,
                      int k, const double *d_B, int64_t ldb, double *d_X,
                      int64_t ldx, const spmv_trsv_plan *first,
                      const spmv_trsv_plan *second, const double *d_scale,
                      double tol, int maxit, int check_every, void *d_work,
                      size_t work_bytes, spmv_cg_info *info, void *stream);

/*
 * Smoothed-aggregation algebraic multigrid on the device, and conjugate
 * gradients preconditioned by one V cycle (added after 0.7; spmv_version() is
 * unchanged, detect them by the symbols).  Everything is defined to the
 * integer or to the bit; tests/_amg.py restates it in numpy.
 *
 * AGGREGATION.  spmv_csr_aggregate: A square, f64, with its source, every row
 * strictly ascending by column and holding its diagonal.  theta2 = theta *
 * theta is formed on the host.  Entry (i, j), j != i, is STRONG iff
 *     rn(a_ij * a_ij) >= rn(theta2 * |rn(d_i * d_j)|)
 * (d the stored diagonal; a comparison with a NaN is false, so a NaN entry is
 * never strong; theta == 0 makes every stored off-diagonal with a finite
 * d_i d_j strong, explicit zeros included).  Only row i's own entries are
 * read: nothing assumes symmetry, the neighbours of i are the strong columns
 * of row i.
 *   Roots: a maximal independent set of distance 2 in that graph by parallel
 * rounds (Bell, Dalton, Olson 2012).  Row i carries the tuple (state,
 * fmix32(i ^ seed), i), ordered lexicographically with out < undecided < root.
 * A round takes the maximum over a row and its neighbours twice (the second
 * time of the first maxima) and decides: an undecided row whose distance-2
 * maximum is its own tuple becomes a root, one whose maximum is a root becomes
 * out.  One round is three launches and one 4-byte read-back of the number of
 * undecided rows; every launch reads arrays earlier launches wrote and writes
 * another; no workgroup waits for another.  More than max_rounds rounds (0:
 * 4096) is -E2BIG.
 *   Aggregates, in this order.  Roots are numbered in ascending row order.
 * Pass 1: a row that is no root joins the root among its strong neighbours of
 * the greatest |a_ij|, the first in stored order among equals.  Pass 2: a row
 * still free joins the aggregate its strong neighbour of the greatest |a_ij|
 * (the first among equals) had AFTER pass 1.  Pass 3: rows still free become
 * singletons, numbered behind the roots in row order.  (A row put out has a
 * root within two strong steps, and the row between them joined in pass 1: as
 * defined here pass 3 finds no row; it is kept as the guard of that argument.)
 *   d_agg: M ints or NULL.  info (or NULL): aggregates = roots + singletons,
 * rounds, widest = the rows of the largest aggregate.  M == 0: zeros.
 *   Errors, in this order: NULL A, theta not finite or negative, max_rounds
 * < 0 -EINVAL; no device -ENODEV; a dead handle -EBADF; not square -EINVAL; an
 * f32 handle -ENOTSUP; after spmv_csr_release_source -ENODATA; a column
 * outside [0, M) -EDOM; a row not strictly ascending or without its diagonal
 * -EINVAL (a device check, before anything else is allocated); -E2BIG;
 * -ENOMEM.  On any error d_agg and *info are not written and all scratch is
 * freed.  The call blocks.
 *
 * SETUP.  spmv_csr_amg_setup builds a hierarchy from A_0 = A (the checks of
 * spmv_csr_aggregate; sweeps and coarse_sweeps in 1..64, min_rows >= 1,
 * max_levels in 1..32 or 0 = 16, kmax in 1..8, else -EINVAL).  Per level l of
 * M_l rows:
 *   1. rho = max_i rn(S_i / |d_i|), S_i the sequential sum of |a_ij| in stored
 *      order from 0.0: the Gershgorin bound of D^-1 A (a maximum is exact in
 *      any order).  A rho that is not finite or not positive is -EDOM (so is
 *      M == 0).
 *   2. omega = (4.0 / 3.0) / rho on the host; w_i = rn(omega / d_i).
 *   3. The level is the coarsest when M_l <= min_rows, or it is the
 *      max_levels-th, or the aggregation (theta, seed) gives M_l aggregates.
 *   4. Otherwise T is M_l x aggregates with one 1.0 per row at column agg[i];
 *      AT = spmv_csr_spgemm(A_l, T);  P = T - diag(w) AT in place on AT's
 *      values, p = rn(t - rn(w_i * at)) with t = 1.0 at column agg[i] and 0.0
 *      elsewhere;  PT = spmv_csr_transpose(P);  A_{l+1} =
 *      spmv_csr_galerkin(A_l, P, PT).
 * The hierarchy owns A_1.., every P and PT (ordinary live handles: they count
 * in spmv_live_handles() until the hierarchy is released), w, and one scratch
 * allocation of four vectors of kmax * M_l doubles per level (two on level
 * 0).  It BORROWS A_0: releasing A makes every later apply -EBADF.  On any
 * error nothing is left allocated and spmv_live_handles() is what it was.
 * spmv_amg_info: the numbers of the hierarchy (any level beyond `levels` is
 * zero; rounds and aggregates of the coarsest level are 0 when it was not
 * aggregated); spmv_amg_level: the borrowed handles and w of level l (P and PT
 * NULL on the coarsest); any out-pointer may be NULL.  spmv_amg_last_phases:
 * host-clock ms of the last successful setup of this process -- [0] rho and w,
 * [1] aggregation, [2] T, A T and the smoothing, [3] the transposition, [4] the
 * Galerkin product, [5] scratch and bookkeeping.  Not thread-safe.
 *
 * THE CYCLE.  spmv_amg_apply: Z = V(R) for k <= kmax interleaved vectors (ldr,
 * ldz >= k; 0 = k), asynchronous on `stream` and capturable: the launches are
 * a function of the hierarchy and k alone.  Two applies of one hierarchy must
 * not overlap in time (they share its scratch).  At level l with right-hand
 * side b:
 *   1. x = rn(w_i * b_i)
 *   2. sweeps - 1 times  x <- rn(x + rn(w_i * rn(b - s))),  s = the row of
 *      A_l x
 *   3. on the coarsest level the same with coarse_sweeps for sweeps; return
 *   4. r = rn(b - s);  b_c = PT r;  x_c from level l + 1;
 *      x <- rn(x + (P x_c));  sweeps more sweeps.
 * Every s and both transfer products have the bits of spmv_csr_launch_multi on
 * that level's handle (group 0), rn(b - s) is what spmv_csr_launch_axpby(-1,
 * 1) stores and rn(x + P x_c) what launch_axpby(1, 1) stores; nothing else is
 * fused: no multiply-add outside those products.  The bits depend on neither
 * k, nor waves_per_block, nor the other columns.  A sweep is either ONE
 * launch of the fused kernel (amg_kernels.hip: the walk of launch_multi, then
 * x_new = rn(x_old + rn(w_i rn(b - s))) written to the other buffer of a
 * ping-pong; its residual mode stores rn(b - s)) or the composition it
 * replaces, launch_axpby into r followed by one vector kernel -- the same bits
 * either way.  Which one is a measured rule (profiles/amg.md): the fused
 * kernel for k >= 4, the composition below, and always the composition on a
 * level whose handle holds a row of more than 2048 entries.
 * spmv_amg_set_fused(mode) overrides the rule for the process (MEASUREMENT and
 * tests; not thread-safe): 0 the composition everywhere, 2 the fused kernel
 * wherever it can run, 1 the rule; returns the previous mode, -EINVAL for
 * another value.  spmv_amg_summary.launches is the count at k = kmax.  opts: waves_per_block
 * only (group, variant, reserved 0).  Errors: NULL H, d_R or d_Z, k outside
 * 1..kmax, a leading dimension below k, d_R == d_Z, bad opts -EINVAL; a dead
 * hierarchy, or one whose A_0 was released -EBADF (-ENODEV without a device).
 *
 * THE SOLVER.  spmv_*_pcg_amg is spmv_*_pcg_trsv word for word with
 * Z = spmv_amg_apply(H, R) where that has the plans' solves: the handles (the
 * fine matrix may be HLL; H was built from a CSR handle of the same rows), the
 * blocking, check_every, the records, the frozen-column rule, d_work of
 * spmv_pcg_trsv_work_bytes(M, k) bytes.  Checks added after pcg's, in this
 * order: NULL H -EINVAL; a dead hierarchy -EBADF; H's M is not A's -EINVAL;
 * k > kmax -EINVAL.
 *
 * Not in scope: AMG inside bicgstab / gmres / minres, W or K cycles, Chebyshev
 * or Gauss-Seidel smoothing, a direct coarse solve, strength-filtered
 * smoothing, f32 or HLL levels, reuse of a pattern for new values.
 */
typedef struct spmv_aggregate_info {
    int aggregates, roots, rounds;
    int widest;     /* rows of the largest aggregate */
    int singletons; /* aggregates made by pass 3 */
} spmv_aggregate_info;
int spmv_csr_aggregate(const spmv_csr_dev *A, double theta, uint32_t seed,
                       int max_rounds, int *d_agg /* M ints or NULL */,
                       spmv_aggregate_info *info /* or NULL */);

#define SPMV_AMG_MAX_LEVELS 32
typedef struct spmv_amg spmv_amg;
typedef struct spmv_amg_summary {
    int levels, sweeps, coarse_sweeps, kmax;
    int rows[SPMV_AMG_MAX_LEVELS];
    int rounds[SPMV_AMG_MAX_LEVELS];
    int aggregates[SPMV_AMG_MAX_LEVELS];
    int launches; /* of one apply */
    int64_t entries[SPMV_AMG_MAX_LEVELS];
    double rho[SPMV_AMG_MAX_LEVELS], omega[SPMV_AMG_MAX_LEVELS];
    double complexity; /* sum of entries / entries[0] */
    int64_t scratch_bytes;
} spmv_amg_summary;
int spmv_csr_amg_setup(const spmv_csr_dev *A, double theta, int sweeps,
                       int coarse_sweeps, int min_rows, int max_levels,
                       uint32_t seed, int kmax, spmv_amg **out);
int spmv_amg_info(const spmv_amg *H, spmv_amg_summary *out);
int spmv_amg_level(const spmv_amg *H, int level, const spmv_csr_dev **A,
                   const spmv_csr_dev **P, const spmv_csr_dev **PT,
                   const double **d_w);
void spmv_amg_last_phases(double ms[6]);
int spmv_amg_set_fused(int mode);
void spmv_amg_release(spmv_amg *H);
void spmv_amg_release_checked(spmv_amg *H, uint64_t generation);
int spmv_amg_apply(const spmv_amg *H, const spmv_launch_opts *opts, int k,
                   const double *d_R, int64_t ldr, double *d_Z, int64_t ldz,
                   void *stream);
int spmv_csr_pcg_amg(const spmv_csr_dev *A, const spmv_launch_opts *opts,
                     int k, const double *d_B, int64_t ldb, double *d_X,
                     int64_t ldx, const spmv_amg *H, double tol, int maxit,
                     int check_every, void *d_work, size_t work_bytes,
                     spmv_cg_info *info, void *stream);
int spmv_hll_pcg_amg(const spmv_hll_dev *A, const spmv_launch_opts *opts,
                     int k, const double *d_B, int64_t ldb, double *d_X,
                     int64_t ldx, const spmv_amg *H, double tol, int maxit,
                     int check_every, void *d_work, size_t work_bytes,
                     spmv_cg_info *info, void *stream);

/*
 * BiCGStab on the device for A X = B with a nonsymmetric A (added after 0.7;
 * spmv_version() is unchanged, detect it by the symbol).  A: square, otherwise
 * arbitrary, a CSR or column-major HLL handle of either value type.  Only A x
 * is used (two launch_multi per iteration), never a transposed product.
 * k = 1..8 independent systems stored interleaved as in spmv_*_launch_multi.
 *
 * d_minv: M doubles, one per row, shared by the k columns, never written: a
 * RIGHT diagonal preconditioner, A M^-1 (M x) = b with z(u)_i = minv_i * u_i.
 * Any sign is allowed; spmv_*_diag(invert = 1) gives Jacobi.  NULL: none.
 *
 * d_X, d_B, the strides, the spmv_cg_info records (iterations counts the full
 * steps applied to X), the blocking, -EBUSY on a capturing stream before
 * anything is allocated or enqueued, check_every (0 = 8), maxit, d_work (NULL:
 * the library allocates and frees it; else 8-byte aligned and at least
 * spmv_bicgstab_work_bytes(M, k) bytes, else -EINVAL), M == 0 and the argument
 * checks are those of spmv_*_pcg above, word for word, except that d_minv may
 * be NULL.  spmv_bicgstab_work_bytes(M, k) = a base that depends on neither
 * argument (the state block, two sets of partial sums) + 6 * 8 * k * M: R,
 * the shadow residual Rh, P, V, T and the preconditioned vector launch_multi
 * reads.
 *
 * Result contract, to the bit.  Every operation is rounded once, no fused
 * multiply-add, divisions are correctly rounded; dot is the dot of
 * spmv_cg_dot_shape; z(U) is rn(minv_i * u_i) in every column, U itself
 * without d_minv; tol2 = tol * tol on the host.
 *
 *   R = B;  R = (-1) A X + 1 R  by the handle's launch_axpby;  Rh = R;  P = R
 *   bb = dot(B, B);  rr = dot(R, R);  rho = rr
 *   column j: status 2 (iterations 0) if rr or bb is not finite,
 *             else converged (iterations 0) if rr <= tol2 * bb, else running
 *   repeat at most maxit times:
 *       Z = z(P);  V = A Z   by launch_multi (all k columns, the caller's opts)
 *       rv = dot(Rh, V)
 *       running column with !(rv != 0 and finite): status 2, frozen
 *       running column: alpha = rho / rv;  S = R - alpha * V
 *       Zs = z(S);  T = A Zs  by launch_multi
 *       ts = dot(T, S);  tt = dot(T, T)
 *       running column with ts or tt not finite: status 2, frozen
 *       running column: omega = tt > 0 ? ts / tt : 0.0
 *                       X = (X + alpha * Z) + omega * Zs
 *                       R = S - omega * T;   iterations += 1
 *       rn = dot(R, R);  rhon = dot(Rh, R)
 *       running column: rn <= tol2 * bb -> status 0, frozen (rr = rn)
 *                       rn not finite   -> status 2, frozen
 *       running column: beta = (rhon / rho) * (alpha / omega)
 *                       P = R + beta * (P - omega * V);  rho = rhon;  rr = rn
 *   columns still running: status 1
 *
 * omega == 0 and rhon == 0 get no rule of their own: they make beta infinite,
 * NaN or zero, and plain arithmetic carries the column to the rv test of the
 * next iteration, or on.  S == 0 exactly makes tt == 0, omega = 0 and R = 0:
 * the column converges in that step.
 *
 * X, iterations, status and rr of a frozen column are never written again,
 * however many iterations were enqueued after it stopped and whatever the
 * other columns hold.  So the results do not depend on check_every, on who
 * owns the work buffer, on waves_per_block or on the other columns, and
 * column j of a k-column solve has the bits of the k = 1 solve of that column.
 * d_minv of all 1.0 gives the bits of d_minv == NULL (rn(1.0 * u) = u): a
 * property of the contract.  The internal vectors are not observable: S lives
 * in R's storage, Z and Zs share one buffer.
 */
int64_t spmv_bicgstab_work_bytes(int M, int k); /* -EINVAL: M < 0, k outside 1..8 */
int spmv_csr_bicgstab(const spmv_csr_dev *A, const spmv_launch_opts *opts,
                      int k, const double *d_B, int64_t ldb, double *d_X,
                      int64_t ldx, const double *d_minv,
                      double tol, int maxit, int check_every,
                      void *d_work, size_t work_bytes,
                      spmv_cg_info *info, void *stream);
int spmv_hll_bicgstab(const spmv_hll_dev *H, const spmv_launch_opts *opts,
                      int k, const double *d_B, int64_t ldb, double *d_X,
                      int64_t ldx, const double *d_minv,
                      double tol, int maxit, int check_every,
                      void *d_work, size_t work_bytes,
                      spmv_cg_info *info, void *stream);

/*
 * BiCGStab preconditioned by triangular plans (added after 0.7; detect it by
 * the symbol): spmv_*_bicgstab word for word, with two differences.  The right
 * preconditioner z(U) is made by spmv_trsv_solve instead of a multiplication
 * by minv, in two steps:
 *     spmv_trsv_solve(first, k, U -> Z, no scale)
 *     if second is not NULL: spmv_trsv_solve(second, k, Z -> Z in place,
 *                                            d_scale)
 * always for all k columns, with an opts that carries only the caller's
 * waves_per_block.  ILU(0) is (the unit lower plan of LU = spmv_csr_ilu0(A),
 * the upper plan of the same LU, NULL); symmetric Gauss-Seidel is (the lower
 * plan of A, the upper plan of A, diag(A)).  The plans and d_scale are never
 * written and may serve any number of solves.
 *
 * And z IS STORED: spmv_*_bicgstab forms z(P) and z(S) again from minv where
 * it updates X, a plan cannot be asked twice for the price of a
 * multiplication.  Zp = z(P) and Zs = z(S) are two vectors, both live at the
 * update, so d_work holds spmv_bicgstab_trsv_work_bytes(M, k) bytes: the base
 * of spmv_bicgstab_work_bytes + 7 * 8 * k * M (R, Rh, P, V, T, Zp, Zs).  One
 * iteration, in launch order:
 *     V = A Zp;  rv;  alpha;  S = R - alpha V (in R);  Zs = z(S)
 *     T = A Zs;  ts, tt;  omega;  X = (X + alpha Zp) + omega Zs, R = S - omega T
 *     rn, rhon;  beta;  P = R + beta (P - omega V);  Zp = z(P)
 * the first Zp = z(P) behind P = R of the set-up.  The recurrence, the
 * classification ladder, the dot order and the roundings are those of
 * spmv_*_bicgstab above with the stored vectors where it has z(.).  A frozen
 * column's Z may hold anything, and nothing of it reaches X, R, P or the
 * state.
 *
 * Everything else is spmv_*_bicgstab: the handles, the interleaved k = 1..8
 * systems, the blocking, -EBUSY on a capturing stream, check_every, maxit,
 * M == 0, the records and the frozen-column rule.  Checks added after
 * bicgstab's, in this order (those of spmv_*_pcg_trsv): NULL first -EINVAL;
 * d_scale without second -EINVAL; a dead plan -EBADF; a plan whose M is not
 * A's -EINVAL.  A plan solve that is refused ends the solve with its code.
 *
 * Two properties of the contract, not special cases: a unit plan without
 * strict entries (or a plan of the identity) returns the bits of
 * spmv_*_bicgstab with d_minv == NULL; a plan of a diagonal matrix of powers
 * of two returns the bits of spmv_*_bicgstab with d_minv = 1 / d.  A NaN in a
 * factor makes rv NaN: the running columns end with status 2, never a fault.
 *
 * The price is that of spmv_*_pcg_trsv, twice: every iteration adds the
 * launches of the plans two times (profiles/ilu0.md).
 */
int64_t spmv_bicgstab_trsv_work_bytes(int M, int k); /* as spmv_bicgstab_work_bytes */
int spmv_csr_bicgstab_trsv(const spmv_csr_dev *A, const spmv_launch_opts *opts,
                           int k, const double *d_B, int64_t ldb, double *d_X,
                           int64_t ldx, const spmv_trsv_plan *first,
                           const spmv_trsv_plan *second, const double *d_scale,
                           double tol, int maxit, int check_every,
                           void *d_work, size_t work_bytes,
                           spmv_cg_info *info, void *stream);
int spmv_hll_bicgstab_trsv(const spmv_hll_dev *H, const spmv_launch_opts *opts,
                           int k, const double *d_B, int64_t ldb, double *d_X,
                           int64_t ldx, const spmv_trsv_plan *first,
                           const spmv_trsv_plan *second, const double *d_scale,
                           double tol, int maxit, int check_every,
                           void *d_work, size_t work_bytes,
                           spmv_cg_info *info, void *stream);

/*
 * Restarted GMRES(m) on the device for A X = B with a nonsymmetric A (added
 * after 0.7; detect it by the symbol).  One product and one preconditioner
 * apply per Arnoldi step, a residual estimate that never grows within a
 * cycle, and no breakdown other than a singular matrix or a non-finite
 * number.  The handles (f64 and f32 CSR, column-major HLL; -ENOTSUP on a
 * handle with 16-bit offsets), the interleaved k = 1..8 systems and the
 * strides, d_minv (a RIGHT diagonal preconditioner, NULL: none), the
 * blocking, -EBUSY on a capturing stream, check_every (0 = 8), M == 0, d_work
 * (NULL: the library allocates and frees it) and the argument checks in their
 * order are those of spmv_*_bicgstab above, word for word; then restart
 * outside 1..64 is -EINVAL, and for the _trsv pair the plan checks of
 * spmv_*_bicgstab_trsv follow, in that order.  maxit counts Arnoldi steps over
 * all cycles.
 *
 * spmv_gmres_work_bytes(M, k, m) = base(m) + (m + 3) * 8 * k * M, the same in
 * all three preconditioner modes: base(m) holds the state (a head and, for 8
 * columns, the rotated Hessenberg factor, the rotations and g: it depends on m
 * alone) and m + 1 sets of partial sums; then the basis V_0..V_m as one vector
 * of (m + 1) M rows, W and Z.
 *
 * Result contract, to the bit.  Every operation is rounded once, no fused
 * multiply-add, divisions and square roots are correctly rounded; dot is the
 * dot of spmv_cg_dot_shape; z(U) is U, rn(minv_i * u_i), or the two plan
 * solves of spmv_*_bicgstab_trsv; tol2 = tol * tol on the host.
 *
 *   START (and every restart, for the columns still running):
 *     V_0 = B;  V_0 = (-1) A X + 1 V_0  by the handle's launch_axpby
 *     bb = dot(B, B) (once);  rr = dot(V_0, V_0);  est = rr
 *     status 2 if rr or bb is not finite, else converged if rr <= tol2 * bb,
 *     else running: beta = sqrt(rr);  g_0 = beta;  V_0 = V_0 / beta
 *   STEP at position p = 0 .. m - 1 of a cycle, running columns:
 *     W = A z(V_p)  by launch_multi (all k columns, the caller's opts)
 *     a_i = dot(V_i, W), i = 0..p;  then W = W - a_i * V_i in increasing i
 *     c_i = dot(V_i, W) of the new W;  then W = W - c_i * V_i likewise
 *     h_i = a_i + c_i;  nn = dot(W, W);  h_{p+1} = sqrt(nn)
 *     a non-finite h_i or nn: status 2, the step does not count
 *     for i < p:  t = c_i * h_i + s_i * h_{i+1}
 *                 h_{i+1} = c_i * h_{i+1} - s_i * h_i;  h_i = t
 *     a = h_p;  b = h_{p+1};  d = sqrt(a * a + b * b)
 *     d not finite or d == 0: status 2, the step does not count
 *     c_p = a / d;  s_p = b / d;  r_ip = h_i (i < p);  r_pp = c_p * a + s_p * b
 *     g_{p+1} = -(s_p * g_p);  g_p = c_p * g_p
 *     iterations += 1;  est = g_{p+1} * g_{p+1}
 *     est <= tol2 * bb: converged, else V_{p+1} = W / h_{p+1}
 *   UPDATE after position m - 1 and once more when the call returns, for
 *   every column with q > 0 counted steps of this cycle not yet in X:
 *     for i = q - 1 .. 0:  s = 0.0;  s = s + r_il * y_l for l = i + 1 .. q - 1
 *                          y_i = (g_i - s) / r_ii
 *     U = y_0 * V_0;  U = U + y_i * V_i for i = 1 .. q - 1;  X = X + z(U)
 *   after position m - 1 a column still running restarts (restarts += 1) and
 *   converges there on the true rr.  Columns still running at the end:
 *   status 1.  rr is then dot(R, R) of R = B - A X by launch_axpby, for every
 *   column.
 *
 * h_{p+1} == 0 with a != 0 gets no rule of its own: s_p = 0, est = 0 and the
 * column converges.  A matrix whose stored values are all 0.0 gives d == 0 in
 * the first step: status 2, 0 iterations, X untouched.
 *
 * A column that left the running state receives exactly one more write to X:
 * the update of the steps it completed in its last cycle, at the next restart
 * boundary or when the call returns, whichever comes first, with the same
 * bits.  Nothing else of it is written.  So the results do not depend on k,
 * check_every, on who owns the work buffer, on waves_per_block, on the other
 * columns or on how the basis is cut into launches.  d_minv of all 1.0, a plan
 * of the identity, and a plan of a diagonal of powers of two against
 * d_minv = 1 / d give the same bits, by arithmetic.
 */
typedef struct spmv_gmres_info {
    int status;      /* 0 converged, 1 maxit reached, 2 breakdown */
    int iterations;  /* Arnoldi steps whose update reached X */
    int restarts;    /* cycles begun after the first */
    int reserved;
    double rr;       /* true r.r, r = b - A x, computed once when the call returns */
    double est;      /* last squared residual estimate of the recurrence */
    double bb;       /* b.b */
} spmv_gmres_info;

int64_t spmv_gmres_work_bytes(int M, int k, int restart); /* -EINVAL: M < 0, k outside 1..8, restart outside 1..64 */
int spmv_csr_gmres(const spmv_csr_dev *A, const spmv_launch_opts *opts, int k,
                   const double *d_B, int64_t ldb, double *d_X, int64_t ldx,
                   const double *d_minv, int restart, double tol, int maxit,
                   int check_every, void *d_work, size_t work_bytes,
                   spmv_gmres_info *info, void *stream);
int spmv_hll_gmres(const spmv_hll_dev *H, const spmv_launch_opts *opts, int k,
                   const double *d_B, int64_t ldb, double *d_X, int64_t ldx,
                   const double *d_minv, int restart, double tol, int maxit,
                   int check_every, void *d_work, size_t work_bytes,
                   spmv_gmres_info *info, void *stream);
int spmv_csr_gmres_trsv(const spmv_csr_dev *A, const spmv_launch_opts *opts,
                        int k, const double *d_B, int64_t ldb, double *d_X,
                        int64_t ldx, const spmv_trsv_plan *first,
                        const spmv_trsv_plan *second, const double *d_scale,
                        int restart, double tol, int maxit, int check_every,
                        void *d_work, size_t work_bytes,
                        spmv_gmres_info *info, void *stream);
int spmv_hll_gmres_trsv(const spmv_hll_dev *H, const spmv_launch_opts *opts,
                        int k, const double *d_B, int64_t ldb, double *d_X,
                        int64_t ldx, const spmv_trsv_plan *first,
                        const spmv_trsv_plan *second, const double *d_scale,
                        int restart, double tol, int maxit, int check_every,
                        void *d_work, size_t work_bytes,
                        spmv_gmres_info *info, void *stream);

/*
 * CGLS on the device for rectangular least squares (added after 0.7;
 * spmv_version() is unchanged, detect it by the symbol): per column,
 *   min ||A x - b||^2 + damp^2 ||x||^2,
 * that is min ||A x - b|| for a tall A, the minimum-norm solution for a wide
 * one (from d_X = 0), and the Tikhonov-regularised problem for damp > 0.
 * Bjorck's form: A^T A is never formed.  A is M x N and AT is N x M, its
 * transpose as a handle of its own (spmv_csr_transpose, and spmv_hll_from_csr
 * of that for an HLL pair); both CSR or both column-major HLL, each of either
 * value type.  That AT really is the transpose of A is NOT checked, just as
 * spmv_*_cg does not check symmetry: only the shapes are.  One iteration is
 * one launch_multi of A and one of AT.
 *
 * d_B has M rows and d_X has N rows, both of k = 1..8 interleaved columns as
 * in spmv_*_launch_multi (ldb, ldx >= k, 0 = k).  d_X holds the initial guess
 * on entry and the iterate on return; d_B is never written.  damp >= 0.
 *
 * Both handles are checked by the function that serves launch_multi, A first,
 * with its answers (NULL -EINVAL, dead handle -EBADF / -ENODEV, compact handle
 * -ENOTSUP, row-major HLL -EINVAL, after spmv_*_release_source() -ENODATA);
 * the one `opts` is validated against both handles and used for both
 * products.  Then -EINVAL: AT->M != A->N or AT->N != A->M, damp or tol
 * negative or NaN, maxit < 0, check_every < 0, NULL info, a d_work that is not
 * 8-byte aligned or holds fewer than spmv_cgls_work_bytes(M, N, k) bytes.
 * M == 0 or N == 0: returns 0 with every record zeroed and nothing enqueued.
 * The blocking, -EBUSY on a capturing stream before anything is allocated or
 * enqueued, check_every (0 = 8) and a NULL d_work (the library allocates and
 * frees it) are those of spmv_*_cg above, word for word.
 * spmv_cgls_work_bytes(M, N, k) = a base that depends on no argument (the
 * state block, three sets of partial sums) + 8 * k * (2 M + 2 N): R and Q of
 * M rows, S and P of N rows.
 *
 * Result contract, to the bit.  Every operation is rounded once, no fused
 * multiply-add, divisions are correctly rounded; dot_L(U, V) is the dot of
 * spmv_cg_dot_shape over L rows, its order a function of that length alone;
 * tol2 = tol * tol and d2 = damp * damp on the host.  With damp == 0 there is
 * no d2 term at all (the lines marked `damp:` do not exist): another
 * instantiation of the kernels, not a multiplication by zero.
 *
 *   R = B;  R = (-1) A X + 1 R   by A's launch_axpby              (M rows)
 *   W = AT B  by AT's launch_multi;  atb = dot_N(W, W)
 *   S = AT R  by AT's launch_multi;  damp: S = S - d2 * X         (N rows)
 *   P = S;  ss = dot_N(S, S)
 *   column j: status 2 (iterations 0) if ss or atb is not finite,
 *             else converged (iterations 0) if ss <= tol2 * atb, else running
 *   repeat at most maxit times:
 *       Q = A P  by A's launch_multi (all k columns, the caller's opts)
 *       delta = dot_M(Q, Q);   damp: delta = delta + d2 * dot_N(P, P)
 *       running column with !(delta > 0 and finite): status 2, frozen
 *       running column: alpha = ss / delta;  X = X + alpha * P;
 *                       R = R - alpha * Q;  iterations += 1
 *       S = AT R  by AT's launch_multi;   damp: S = S - d2 * X
 *       sn = dot_N(S, S)
 *       running column: sn <= tol2 * atb -> status 0, frozen (ss = sn)
 *                       sn not finite    -> status 2, frozen
 *       running column: beta = sn / ss;  P = S + beta * P;  ss = sn
 *   columns still running: status 1
 *   rr = dot_M(R, R), once, after the loop, for every column
 *
 * X, R, P, ss, the status and the count of a frozen column are never written
 * again; S and Q are scratch, the products rewrite all k columns of them.  So
 * X and the records do not depend on check_every, on who owns the work buffer,
 * on waves_per_block or on the other columns, and column j of a k-column solve
 * has the bits of the k = 1 solve of that column.  ss is tested against atb,
 * not against r.r: a b orthogonal to the range of A (atb == 0) is converged
 * at once with X untouched.
 */
typedef struct spmv_cgls_info {
    int status;      /* 0 converged, 1 maxit reached, 2 breakdown */
    int iterations;  /* updates of x applied to this column */
    double ss;       /* last s.s of the recurrence, s = A^T r - damp^2 x */
    double atb;      /* (A^T b).(A^T b): what ss is tested against */
    double rr;       /* r.r of the recurrence's R when the call returns */
} spmv_cgls_info;

int64_t spmv_cgls_work_bytes(int M, int N, int k); /* -EINVAL: M < 0, N < 0, k outside 1..8 */
int spmv_csr_cgls(const spmv_csr_dev *A, const spmv_csr_dev *AT,
                  const spmv_launch_opts *opts, int k,
                  const double *d_B, int64_t ldb, double *d_X, int64_t ldx,
                  double damp, double tol, int maxit, int check_every,
                  void *d_work, size_t work_bytes,
                  spmv_cgls_info *info, void *stream);
int spmv_hll_cgls(const spmv_hll_dev *H, const spmv_hll_dev *HT,
                  const spmv_launch_opts *opts, int k,
                  const double *d_B, int64_t ldb, double *d_X, int64_t ldx,
                  double damp, double tol, int maxit, int check_every,
                  void *d_work, size_t work_bytes,
                  spmv_cgls_info *info, void *stream);

/*
 * MINRES on the device for A X = B with a symmetric A that need not be
 * definite: KKT and saddle-point matrices, shifted stencils (added after 0.7;
 * spmv_version() is unchanged, detect it by the symbol).  A: square and
 * symmetric -- symmetry is NOT checked, as in spmv_*_cg -- a CSR or
 * column-major HLL handle of either value type.  One launch_multi per
 * iteration and a three-term recurrence (Paige and Saunders); the residual
 * norm of the recurrence falls monotonically.  k = 1..8 independent systems
 * stored interleaved as in spmv_*_launch_multi.
 *
 * d_minv: M doubles, one per row, shared by the k columns, never written: a
 * diagonal preconditioner, z(u)_i = minv_i * u_i.  It must be POSITIVE where
 * given (a column whose u.z(u) is negative or not finite is a breakdown);
 * spmv_*_diag(invert = 1) gives Jacobi where the diagonal is positive, a
 * saddle-point caller passes 1 / |d| with 1 where d == 0.  NULL: none.
 *
 * d_X, d_B, the strides, the blocking, -EBUSY on a capturing stream before
 * anything is allocated or enqueued, check_every (0 = 8), maxit, d_work (NULL:
 * the library allocates and frees it; else 8-byte aligned and at least
 * spmv_minres_work_bytes(M, k) bytes, else -EINVAL), M == 0 (returns 0 with
 * zeroed records) and the argument checks (the handle, opts, k, strides and
 * pointers by the function that serves launch_multi; M != N, a negative or NaN
 * tol, maxit < 0, check_every < 0, NULL info: -EINVAL) are those of
 * spmv_*_bicgstab above, word for word.  spmv_minres_work_bytes(M, k) = a base
 * that depends on neither argument (the state block, three sets of partial
 * sums) + 6 * 8 * k * M: two residual buffers, V, Q and two direction
 * buffers.  The host rotates the two pairs by the parity of the iteration
 * number, which all columns share: nothing is copied.
 *
 * Result contract, to the bit.  Every operation is rounded once, no fused
 * multiply-add crosses a * and a +, divisions and square roots are correctly
 * rounded; dot is the dot of spmv_cg_dot_shape; z(U)_i = rn(minv_i * u_i) in
 * every column, U itself without d_minv; tol2 = tol * tol on the host.
 *
 *   R2 = B;  R2 = (-1) A X + 1 R2  by the handle's launch_axpby;  W1 = W2 = +0.0
 *   bb = dot(B, B);  bn2 = dot(B, z(B));  b1 = dot(R2, z(R2))
 *   column j: status 2 (iterations 0) if !(b1 >= 0 and finite) or !(bn2 >= 0 and finite),
 *             else converged (iterations 0) if b1 <= tol2 * bn2, else running with
 *             beta = sqrt(b1); phibar = beta; dbar = 0; epsln = 0; cs = -1; sn = 0
 *   repeat at most maxit times, i = 1, 2, ...:
 *       s = 1 / beta;  V = s * z(R2)                    (rn(s * rn(minv_i * r_i)))
 *       Q = A V   by launch_multi (all k columns, the caller's opts)
 *       i >= 2:  Q = Q - (beta / oldb) * R1             (i == 1: the term does not exist --
 *                                                        another instantiation, not a zero)
 *       alfa = dot(V, Q)
 *       running column with alfa not finite: status 2, frozen
 *       Rn = Q - (alfa / beta) * R2;   bnew = dot(Rn, z(Rn));   R1 = R2;  R2 = Rn
 *       running column with !(bnew >= 0 and finite): status 2, frozen
 *       oldb = beta;  beta = sqrt(bnew);  oldeps = epsln
 *       delta = cs*dbar + sn*alfa;  gbar = sn*dbar - cs*alfa;  epsln = sn*beta;  dbar = -(cs*beta)
 *       gamma = sqrt(gbar*gbar + beta*beta)
 *       running column with !(gamma > 0 and finite): status 2, frozen
 *       cs = gbar/gamma;  sn = beta/gamma;  phi = cs*phibar;  phibar = sn*phibar
 *       Wn = ((V - oldeps*W1) - delta*W2) / gamma;  W1 = W2;  W2 = Wn
 *       X = X + phi*Wn;  iterations += 1;  pp = phibar*phibar
 *       running column: pp <= tol2 * bn2 -> status 0, frozen;  pp not finite -> status 2, frozen
 *   columns still running: status 1
 *   R = B - A X by launch_axpby;  rr = dot(R, R), once, for every column
 *
 * pp of a column that made no iteration is b1.  The W recurrence is the same
 * three-term expression in every iteration, the first two included: the zero
 * buffers are read and multiplied, so the sign of a zero is what the
 * arithmetic gives.  A column frozen before the X update of an iteration does
 * not get that update.  X, iterations, status and pp of a frozen column are
 * never written again, however many iterations were enqueued after it stopped
 * and whatever the other columns hold.  So the results do not depend on
 * check_every, on who owns the work buffer, on waves_per_block or on the other
 * columns, and column j of a k-column solve has the bits of the k = 1 solve
 * of that column.  d_minv of all 1.0 gives the bits of d_minv == NULL.
 * beta == 0 has no rule of its own: phibar becomes 0 and the column converges
 * in that step.  The internal vectors are not observable.  The stopping test
 * is in the norm the recurrence has, the M^-1 norm (the 2-norm without a
 * preconditioner); rr and bb give the caller the true figure.
 */
typedef struct spmv_minres_info {
    int status;      /* 0 converged, 1 maxit reached, 2 breakdown */
    int iterations;  /* updates of x applied to this column */
    double pp;       /* last phibar*phibar: the recurrence's residual estimate, squared, in the M^-1 norm */
    double bn2;      /* dot(B, z(B)): what pp is tested against */
    double rr;       /* true r.r, r = b - A x, computed once when the call returns */
    double bb;       /* b.b */
} spmv_minres_info;

int64_t spmv_minres_work_bytes(int M, int k); /* -EINVAL: M < 0, k outside 1..8 */
int spmv_csr_minres(const spmv_csr_dev *A, const spmv_launch_opts *opts, int k,
                    const double *d_B, int64_t ldb, double *d_X, int64_t ldx,
                    const double *d_minv, double tol, int maxit,
                    int check_every, void *d_work, size_t work_bytes,
                    spmv_minres_info *info, void *stream);
int spmv_hll_minres(const spmv_hll_dev *H, const spmv_launch_opts *opts, int k,
                    const double *d_B, int64_t ldb, double *d_X, int64_t ldx,
                    const double *d_minv, double tol, int maxit,
                    int check_every, void *d_work, size_t work_bytes,
                    spmv_minres_info *info, void *stream);
/* TEST HOOK: d_out[i] = the square root the MINRES kernels take of d_in[i],
 * i < n, asynchronous on `stream` (-EINVAL: n < 0, a NULL pointer with n > 0);
 * the contract asks for the correctly rounded one */
int spmv_debug_sqrt(const double *d_in, double *d_out, int64_t n, void *stream);

/*
 * Pick the fastest kernel for this matrix by measurement (5 launches each):
 * the coalesced kernels of the handle's layout and, when allow_panels != 0
 * and those run well below the stream rate, the 2-D blocked path (built on
 * demand, released again if it loses).  d_y is scratch.
 */
int spmv_csr_autotune(spmv_csr_dev *A, const double *d_x, double *d_y,
                      int allow_panels, int *best_kernel, double *best_ms);
int spmv_hll_autotune(spmv_hll_dev *H, const double *d_x, double *d_y,
                      int allow_panels, int *best_kernel, double *best_ms);

/* per-kernel medians (ms) of the last spmv_*_autotune on this handle, kernel
 * ids 0 .. n-1 (0.0: not a candidate for this matrix), and what the selector
 * did: one text line per phase with host-clock seconds -- direct kernels,
 * every blocked candidate (build s, configurations timed, s, best ms), total
 * (-ENOENT before any autotune) */
int spmv_csr_tune_times(const spmv_csr_dev *A, double *ms, int n);
int spmv_hll_tune_times(const spmv_hll_dev *H, double *ms, int n);
int spmv_csr_tune_log(const spmv_csr_dev *A, char *buf, size_t len);
int spmv_hll_tune_log(const spmv_hll_dev *H, char *buf, size_t len);

/*
 * Dead-handle contract.  Every entry point that takes a handle checks it
 * first: NULL -> -EINVAL, a pointer that is not (or no longer) a live handle
 * -> -EBADF, before anything is allocated or dereferenced
 * (spmv_*_algorithmic_bytes return the code as a negative byte count).
 * spmv_*_release() of such a pointer is ignored AND counted:
 * spmv_ignored_releases() returns the count, spmv_set_debug(1) adds one line
 * on stderr per ignored release (the library reads no environment variable;
 * the Python binding passes SPMV_DEBUG on).  spmv_live_handles(): handles
 * created and not yet released (CSR + HLL, one-shot calls included while they
 * run).
 *
 * Address reuse: a released handle's address may be handed out again by the
 * allocator.  Every handle therefore carries a process-wide generation
 * (1, 2, 3, ... never reused; spmv_handle_generation, 0 for a pointer that is
 * not live), and spmv_*_release_checked(h, generation) releases only the
 * handle that was created with that generation -- a stale wrapper object
 * (finaliser, atexit sweep) cannot release a newer handle that happens to live
 * at the old address.  Bindings with finalisers should use the checked form.
 */
int spmv_live_handles(void);
long spmv_ignored_releases(void);
void spmv_set_debug(int on);
uint64_t spmv_handle_generation(const void *handle);
void spmv_csr_release_checked(spmv_csr_dev *A, uint64_t generation);
void spmv_hll_release_checked(spmv_hll_dev *H, uint64_t generation);

/* Library self-description: "spmv_scpa_amd <version> gfx950". */
const char *spmv_version(void);
/* TEST HOOKS: leave in every last-arriver counter of the handle (long rows,
 * wide hack blocks, the long rows beside a blocked copy) what a launch that
 * never completed would have left.  Later launches must give the right y all
 * the same: the counters carry the launch's number and an arrival that finds
 * another number starts from zero.  Returns the counters touched. */
int spmv_csr_debug_stale_arrivals(spmv_csr_dev *A);
int spmv_hll_debug_stale_arrivals(spmv_hll_dev *H);

/* HIP_VERSION (major * 10^7 + minor * 10^5 + patch) of the headers the library
 * was built with / of the runtime the process has bound it to (-EIO when the
 * runtime does not answer).  Majors must agree. */
int spmv_hip_build_version(void);
int spmv_hip_runtime_version(void);
/* "product", or "ablations": built with -DSPMV_ABLATIONS (`make abl` ->
 * lib/libspmv_scpa_amd_abl.so), the only flavour that accepts the experiment
 * bits of spmv_launch_opts.variant (timing ablations, some of which compute a
 * WRONG y by design; pipeline depths, phase lags, group sizes).  The product
 * library answers -EINVAL to any bit that is not documented above. */
const char *spmv_build_flavour(void);

#ifdef __cplusplus
}
#endif
#endif /* SPMV_ENGINE_H */
