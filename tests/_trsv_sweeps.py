"""Sweep plans (spmv_csr_trsv_analyse_sweeps; spmv_engine.h): the triangular
solve by a fixed number of Jacobi sweeps, restated in numpy.  No GPU here.

reference_sweeps    x(1) = row(i) with s = +0.0, x(m) = row(i; x(m-1)): the
                    row loop of tests/_trsv.py reference_solve with the
                    gathers taken from the PREVIOUS iterate
fast_sweeps         the same with all rows of a sweep taken together (they
                    never meet): the same operations on the same operands, so
                    the same bits, in a fraction of the time
sweeps_apply        apply(R) of two sweep plans, in the shape of
                    tests/_pcg_trsv.py plans_apply
steps_from          how many dependency steps each row is away from row r

A plan is one of tests/_trsv.py reference_plan.  Its rows are kept there in
level order, the device keeps a sweep plan's in row order: the strict entries
of a row and their stored order are the same either way, and nothing else is
read.
"""
import numpy as np


def reference_sweeps(plan, B, scale, G, sweeps, unit=False):
    """X (M, k) after `sweeps` sweeps, one rounding per operation"""
    order, rowptr, ja, vals = (plan[n] for n in ("order", "rowptr", "ja", "as"))
    diag = plan["diag"]
    B = np.asarray(B, np.float64)
    M, k = B.shape
    X = np.zeros((M, k))
    with np.errstate(all="ignore"):
        for m in range(1, sweeps + 1):
            prev, X = X, np.zeros((M, k))
            for p in range(M):
                i = order[p]
                slot = np.zeros((G, k))
                if m > 1:  # the first sweep does not read the matrix
                    for e in range(rowptr[p], rowptr[p + 1]):
                        g = (e - rowptr[p]) % G
                        slot[g] = slot[g] + vals[e] * prev[ja[e]]
                h = G // 2
                while h >= 1:
                    slot[:h] = slot[:h] + slot[h:2 * h]
                    h //= 2
                rhs = B[i] if scale is None else scale[i] * B[i]
                t = rhs - slot[0]
                X[i] = t if unit else t / diag[i]
    return X


def fast_sweeps(plan, B, scale, group, sweeps, unit=False):
    """reference_sweeps, one sweep at a time"""
    order, rowptr, ja, vals = (plan[n] for n in ("order", "rowptr", "ja", "as"))
    diag = plan["diag"]
    B = np.asarray(B, np.float64)
    M, k = B.shape
    beg = rowptr[:-1].astype(np.int64)
    n = np.diff(rowptr)
    X = np.zeros((M, k))
    with np.errstate(all="ignore"):
        rhs = B[order] if scale is None else scale[order][:, None] * B[order]
        for m in range(1, sweeps + 1):
            slot = np.zeros((M, group, k))
            for q in range(int(n.max()) if M and m > 1 else 0):
                act = np.flatnonzero(n > q)
                e = beg[act] + q
                g = q % group
                slot[act, g] = slot[act, g] + vals[e][:, None] * X[ja[e]]
            h = group // 2
            while h >= 1:
                slot[:, :h] = slot[:, :h] + slot[:, h:2 * h]
                h //= 2
            t = rhs - slot[:, 0]
            X = np.zeros((M, k))
            X[order] = t if unit else t / diag[order][:, None]
    return X


def sweeps_apply(first, second, scale, group, sweeps, solve=fast_sweeps):
    """apply(R) of a _trsv solver given two sweep plans of `sweeps` sweeps
    each: first and second are (plan, unit); second may be None"""
    def apply(R):
        Z = solve(first[0], R, None, group, sweeps, first[1])
        if second is not None:
            Z = solve(second[0], Z, scale, group, sweeps, second[1])
        return Z
    return apply


def steps_from(plan, r):
    """steps[i] = the length of the shortest dependency path from row r to row
    i (0 for r itself), -1 where there is none: after s sweeps a NaN in b_r
    has reached exactly the rows with 0 <= steps < s"""
    M = len(plan["order"])
    steps = np.full(M, -1, np.int64)
    steps[r] = 0
    for p in range(M):  # in level order: dependencies come first
        i = plan["order"][p]
        if i == r:
            continue
        d = steps[plan["ja"][plan["rowptr"][p]:plan["rowptr"][p + 1]]]
        d = d[d >= 0]
        if len(d):
            steps[i] = d.min() + 1
    return steps
