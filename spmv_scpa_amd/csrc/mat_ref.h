/*
 * mat_ref.h -- internal: a reference to a CSR or an HLL device handle, and
 * the operations that mgpu.hip (and the seam) run on either format.  They are
 * implemented in engine.hip on the same code as the public spmv_csr_* /
 * spmv_hll_* entry points and make the same handle checks.
 */
#ifndef SPMV_MAT_REF_H
#define SPMV_MAT_REF_H

#include "hip_common.h"

struct mat_ref {
    bool is_hll; /* which handle type h is */
    void *h;     /* spmv_csr_dev * / spmv_hll_dev *; NULL: no matrix */

    static mat_ref of(spmv_csr_dev *A) { return {false, A}; }
    static mat_ref of(spmv_hll_dev *H) { return {true, H}; }
    explicit operator bool() const { return h != NULL; }
    spmv_csr_dev *csr() const { return (spmv_csr_dev *)h; }
    spmv_hll_dev *hll() const { return (spmv_hll_dev *)h; }

    int blocked_kernel() const {
        return is_hll ? SPMV_HLL_KERNEL_PANELS : SPMV_CSR_KERNEL_PANELS;
    }
    int64_t nz() const { return is_hll ? hll()->NZ : csr()->NZ; }
    /* stored entries: HLL slots (padding included), CSR entries */
    int64_t stored() const { return is_hll ? hll()->slots : csr()->NZ; }
    int64_t algorithmic_bytes() const;

    int launch(int kernel, const double *d_x, double *d_y, void *stream) const;
    /* rows [r0, r1): HLL runs hack blocks r0 / 32 .. ceil(r1 / 32) */
    int launch_rows(int kernel, const double *d_x, double *d_y, int r0, int r1,
                    void *stream) const;
    int autotune(const double *d_x, double *d_y, int allow_panels,
                 int *best_kernel, double *best_ms) const;
    int build_panels_opts(const spmv_panel_opts *opts) const;
    int build_panels_like(mat_ref model) const; /* model: the same format */
    int panels_layout(spmv_panel_opts *o, int *waves) const;
    int panels_schedule(void) const;
    int panels_tile_rows(void) const;
    int panels_describe(char *buf, size_t len) const;
    void release(void) const;
};

#endif /* SPMV_MAT_REF_H */
