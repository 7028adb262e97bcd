"""The sparse sum's contract and test shapes on the CPU (tests/_add.py; the
device side: tests/test_gpu_sparse_add.py): the symbols of the C ABI and of the
binding, the argument checks that need no device, the numpy restatement
against dense integer arithmetic, the structural facts, and the shapes held
to what they are for."""
import ctypes as C
import errno

import numpy as np
import pytest

import _add as AD
import spmv_scpa_amd as S

NEG0 = 0x8000_0000_0000_0000


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def integer_valued(mat, seed):
    rng = np.random.default_rng(seed)
    return mat[:4] + (rng.integers(-9, 10, len(mat[4])).astype(np.float64),)


def test_the_headers_and_the_binding_declare_the_entry_points():
    assert S.check_symbols()
    for name in ("spmv_csr_add", "spmv_add_shape", "spmv_add_set_class",
                 "spmv_add_last_phases", "spmv_csr_from_diag",
                 "spmv_csr_scale"):
        assert name in S.declared_symbols(), name
    for name in ("add", "from_diag", "scale"):
        assert callable(getattr(S.CsrDevice, name))
    info = S.AddInfo()
    assert [f[0] for f in info._fields_] == ["nz", "matched", "widest",
                                             "rows_in_bin"]
    assert len(info.rows_in_bin) == 2
    shape = S.add_shape()
    assert shape["widths"] == sorted(set(shape["widths"]))
    assert all(w & (w - 1) == 0 and 2 <= w <= 32 for w in shape["widths"])
    assert shape["threads"] % 64 == 0 and shape["edge"] >= shape["widths"][-1]


def test_null_and_non_finite_arguments_are_refused_before_the_device():
    junk = C.cast(C.create_string_buffer(512), C.c_void_p)
    info = S.AddInfo()
    info.nz = -77
    add = S._lib.spmv_csr_add

    def refused(alpha, a, beta, b, with_out=True):
        out = C.c_void_p(1234)
        rc = add(alpha, a, beta, b, C.byref(out) if with_out else None,
                 C.byref(info))
        assert rc == -errno.EINVAL, rc
        assert (out.value is None) == with_out and info.nz == -77

    refused(1.0, None, 1.0, junk)
    refused(1.0, junk, 1.0, None)
    refused(1.0, junk, 1.0, junk, with_out=False)
    for bad in (np.inf, -np.inf, np.nan):
        refused(bad, junk, 1.0, junk)
        refused(1.0, junk, bad, junk)
    out = C.c_void_p(1234)
    assert S._lib.spmv_csr_from_diag(-1, None, C.byref(out)) == -errno.EINVAL
    assert out.value is None
    assert S._lib.spmv_csr_from_diag(3, None, None) == -errno.EINVAL
    out = C.c_void_p(1234)
    assert S._lib.spmv_csr_scale(junk, None, None,
                                 C.byref(out)) == -errno.EINVAL
    assert out.value is None
    assert S._lib.spmv_csr_scale(None, junk, None,
                                 C.byref(out)) == -errno.EINVAL
    assert S._lib.spmv_csr_scale(junk, junk, None, None) == -errno.EINVAL
    if S.device_count() == 0:  # then: no device, before a handle is looked at
        out = C.c_void_p(1234)
        assert add(1.0, junk, 1.0, junk, C.byref(out),
                   C.byref(info)) == -errno.ENODEV
        assert out.value is None and info.nz == -77
        assert S._lib.spmv_csr_from_diag(3, None,
                                         C.byref(out)) == -errno.ENODEV
        assert S._lib.spmv_csr_scale(junk, junk, None,
                                     C.byref(out)) == -errno.ENODEV
    # the measurement switch: the previous mode comes back
    was = S.add_set_class(2)
    assert S.add_set_class(1) == 2 and S.add_set_class(was) == 1
    with pytest.raises(OSError) as ei:
        S.add_set_class(3)
    assert ei.value.errno == errno.EINVAL
    assert S._lib.spmv_add_set_class(-1) == -errno.EINVAL
    assert S.add_set_class(was) == was


def test_the_restatement_equals_dense_integer_sums():
    cases = [AD.overlap(), AD.disjoint(40, 31), AD.degenerate()["M = 1"],
             AD.degenerate()["N = 1"], AD.degenerate()["A empty"]]
    for k, (A, B) in enumerate(cases):
        A, B = integer_valued(A, 10 + k), integer_valued(B, 20 + k)
        for alpha, beta in ((1.0, 1.0), (2.0, -3.0), (-1.0, 0.0)):
            I, J, V = AD.reference(alpha, A, beta, B)
            want = alpha * AD.dense(A) + beta * AD.dense(B)
            assert np.array_equal(AD.dense((A[0], A[1], I, J, V)), want)


def test_the_structural_facts():
    for A, B in (AD.overlap(), AD.disjoint(), AD.long_against_one(),
                 AD.wide_n()) + tuple(AD.degenerate().values()):
        I, J, V = AD.reference(0.5, A, -2.0, B)
        M, N = A[0], A[1]
        assert len(I) == M + 1 and I[0] == 0 and I[-1] == len(J) == len(V)
        assert I.dtype == J.dtype == np.int32
        rows = np.repeat(np.arange(M), np.diff(I))
        assert np.all((np.diff(J) > 0) | (np.diff(rows) > 0))  # ascending
        keys = rows.astype(np.int64) * max(N, 1) + J
        assert np.array_equal(keys, np.union1d(AD.keys_of(A), AD.keys_of(B)))
        assert len(J) == len(A[3]) + len(B[3]) - AD.matched(A, B)
        # the pattern does not depend on the values
        zeros = AD.reference(0.0, A, 0.0, B)
        assert np.array_equal(zeros[0], I) and np.array_equal(zeros[1], J)
    A, B = AD.overlap()
    la, lb = np.diff(A[2]), np.diff(B[2])
    assert np.any((la == 0) & (lb > 0)) and np.any((la > 0) & (lb == 0))
    assert np.any((la == 0) & (lb == 0)) and 0 < AD.matched(A, B) < len(A[3])
    A, B = AD.disjoint()
    assert AD.matched(A, B) == 0 and len(A[3]) and len(B[3])
    A, B = AD.wide_n()
    assert A[1] == 2 ** 24 + 1 and AD.matched(A, B) >= 4
    assert AD.reference(1, A, 1, B)[1].max() == 2 ** 24


def test_a_minus_a_and_the_special_values():
    A, _ = AD.overlap()
    I, J, V = AD.reference(1.0, A, -1.0, A)
    assert np.array_equal(I, A[2]) and np.array_equal(J, A[3])
    assert not bits(V).any()  # +0.0 everywhere
    sp = AD.special()
    I, J, V = AD.reference(*sp["zeros"])
    assert J.tolist() == [0, 1, 2, 3]
    assert bits(V).tolist() == [NEG0, NEG0, NEG0, 0]
    I, J, V = AD.reference(*sp["inf - inf"])
    assert np.isnan(V).tolist() == [True, False, False, False, False, False]
    assert V[3] == -np.inf and V[5] == 4.0
    I, J, V = AD.reference(*sp["alpha = 0"])
    assert J.tolist() == [0, 1, 2, 3, 4, 5, 7]  # the union stays
    assert np.isnan(V).tolist() == [True, False, False, True, False, False,
                                    False]
    assert V[1] == 2.0 and bits(V[2:3])[0] == NEG0 and V[6] == 2.0
    I, J, V = AD.reference(*sp["subnormal"])
    assert V[0] == 2.0 ** -1071 + 2.0 ** -1070 and V[3] == 2.0 ** -1074
    assert V[1] == 1.5 * 2.0 ** -1070 and V[2] == 2.0 ** -1071
    I, J, V = AD.reference(*sp["nan"])
    assert np.isnan(V).tolist() == [False, True] + [False] * 5


def test_the_edge_shapes_sit_at_their_edges():
    shape = S.add_shape()
    for w in shape["widths"]:
        A, B, what = AD.edges(w)
        assert AD.pick_group(A, B, shape) == w
        L = AD.lens(A, B)
        assert [(int(np.diff(A[2])[r]), int(np.diff(B[2])[r]))
                for r in range(len(what))] == [(a, b) for a, b, _ in what]
        seen = set(L[:len(what)].tolist())
        for m in (w, 2 * w, 64, shape["threads"], shape["edge"]):
            assert {m - 1, m, m + 1} <= seen
        assert {way for _, _, way in what} == set(AD.WAYS)
        n1 = AD.rows_in_bin(A, B, shape)[1]
        assert n1 == int(np.count_nonzero(L == shape["edge"] + 1)) > 0
        assert AD.rows_in_bin(A, B, shape, 1) == (A[0], 0)
        assert AD.rows_in_bin(A, B, shape, 2) == (0, A[0])
        # the four placements are what they say
        for r, (la, lb, way) in enumerate(what):
            a = A[3][A[2][r]:A[2][r + 1]]
            b = B[3][B[2][r]:B[2][r + 1]]
            both = np.intersect1d(a, b)
            if way == "none" or not (la and lb):
                assert len(both) == 0 or way == "all"
            elif way == "all":
                assert len(both) == min(la, lb)
            elif way == "first":
                assert both.tolist() == [a[0]] and a[0] == b[0]
            else:
                assert both.tolist() == [a[-1]] and a[-1] == b[-1]
    A, B = AD.long_against_one()
    assert AD.matched(A, B) == 2 and AD.lens(A, B).min() > shape["edge"]
    A, want = AD.shifted_stencil()
    assert want[2][0] == 4.0 - 1.3 and np.count_nonzero(want[2] != A[4]) == A[0]
