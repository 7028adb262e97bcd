/*
 * solver_host.h -- the host side every device-resident solver shares
 * (cg_solve, bicgstab_solve, cgls_solve, minres_solve), written once.  A solver
 * gives its buffer (solver_work.h) and three callables with its launches:
 *   start(work)  the set-up, up to the first classification; `work` is the
 *                buffer the launches use (the caller's or our own)
 *   iterate(i)   iteration i = 1, 2, ... (MINRES rotates its buffers by i)
 *   finish()     what follows the loop: the true residual of CGLS and MINRES,
 *                with its hipGetLastError; nothing for the others
 * Each returns 0 or the code that ends the solve: a refused product, or a
 * refused plan of spmv_*_pcg_trsv (cg_solve used to look at that behind the
 * batch; returned from iterate it ends the batch early, with the same code).
 *
 * A short or misaligned caller's buffer is refused first (-EINVAL), then a
 * capturing stream (-EBUSY: it cannot be synchronised), before anything is
 * allocated or enqueued, so the capture stays valid.  The loop reads the k
 * statuses back (one copy, one synchronise), stops when no column is
 * CG_RUNNING or maxit iterations are enqueued, and else enqueues
 * min(maxit - done, check_every) more with one hipGetLastError behind them.
 *
 * State: the solver's state struct, at the head of the buffer, with an
 * int status[CG_MAXK].  On 0 *h_st is the state after the solve, a column
 * still CG_RUNNING set to CG_MAXIT, for the solver's records; on any error (a
 * failed hipFree of the own buffer included) the records stay untouched.
 */
#ifndef SPMV_SOLVER_HOST_H
#define SPMV_SOLVER_HOST_H

#include "hip_common.h"

/* the regions of a work buffer as the kernels take them */
static inline double *solver_part(void *work, const solver_work &w, int i) {
    return (double *)((char *)work + solver_work_part(w, i));
}
static inline double *solver_vec(void *work, const solver_work &w, int i) {
    return (double *)((char *)work + solver_work_vec(w, i));
}

template <typename State, typename Start, typename Iterate, typename Finish>
static int solver_run(const solver_work &w, int maxit, int check_every,
                      void *d_work, size_t work_bytes, State *h_st,
                      hipStream_t s, Start start, Iterate iterate,
                      Finish finish) {
    const int k = w.k;
    const size_t need = (size_t)solver_work_bytes(w);
    if (d_work && (work_bytes < need || ((uintptr_t)d_work & 7)))
        return -EINVAL;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    const hipError_t ce = hipStreamIsCapturing(s, &cap);
    if (ce != hipSuccess) {
        (void)hipGetLastError();
        return ce == hipErrorStreamCaptureImplicit ? -EBUSY : hip_errno(ce);
    }
    if (cap != hipStreamCaptureStatusNone)
        return -EBUSY;

    int rc = 0;
    void *own = NULL;
    int h_status[CG_MAXK];
    (void)hipGetLastError(); /* an earlier caller's unread error is not ours */
    if (!d_work) {
        HIP_TRY(hipMalloc(&own, need));
        d_work = own;
    }
    {
        const State *st = (const State *)d_work;
        rc = start(d_work);
        if (rc)
            goto fail;
        HIP_TRY(hipGetLastError());

        for (int done = 0;;) {
            HIP_TRY(hipMemcpyAsync(h_status, st->status, k * sizeof(int),
                                   hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            bool running = false;
            for (int j = 0; j < k; ++j)
                running = running || h_status[j] == CG_RUNNING;
            if (!running || done >= maxit)
                break;
            const int batch = maxit - done < check_every ? maxit - done
                                                         : check_every;
            for (int it = 0; it < batch; ++it) {
                rc = iterate(done + it + 1);
                if (rc)
                    goto fail;
            }
            HIP_TRY(hipGetLastError());
            done += batch;
        }
        rc = finish();
        if (rc)
            goto fail;
        HIP_TRY(hipMemcpyAsync(h_st, st, sizeof *h_st, hipMemcpyDeviceToHost,
                               s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    for (int j = 0; j < k; ++j)
        if (h_st->status[j] == CG_RUNNING)
            h_st->status[j] = CG_MAXIT;
    if (own)
        rc = hip_errno(hipFree(own));
    return rc;
fail:
    /* nothing of ours may still run when the work buffer goes */
    (void)hipStreamSynchronize(s);
    if (own)
        (void)hipFree(own);
    (void)hipGetLastError();
    return rc;
}

#endif /* SPMV_SOLVER_HOST_H */
