"""CPU suite of tests/special_values.py: the order-independent reference that tests/test_gpu_special_values.py holds the kernels to is itself
checked here -- against a brute-force loop, against the oracle's arithmetic on finite data and on closed-form corner cases -- and the
committed seeds are shown to meet the conditions the GPU tests rely on (share of poisoned rows, every class present, clean rows next to,
in a 4-group with and in a tile with poisoned ones; exact subnormal sums)."""
import math

import numpy as np
import pytest

import special_values as sv

ABS = ((1.0, 0.0), (-0.75, 0.0), (2.0, 0.5))


def brute(alpha, beta, rowptr, cols, vals, x, y0):
    out = []
    for i in range(len(rowptr) - 1):
        ps = []
        for j in range(rowptr[i], rowptr[i + 1]):
            a, b = float(vals[j]), float(x[cols[j]])
            if math.isnan(a) or math.isnan(b) or (math.isinf(a) and b == 0) or (math.isinf(b) and a == 0):
                ps.append(math.nan)
            elif math.isinf(a) or math.isinf(b):
                ps.append(math.copysign(math.inf, math.copysign(1.0, a) * math.copysign(1.0, b)))
            else:
                prod = a * b  # (an overflow is its Inf)
                ps.append(prod)
        if any(math.isnan(p) for p in ps) or (math.inf in ps and -math.inf in ps):
            s = math.nan
        elif math.inf in ps:
            s = math.inf
        elif -math.inf in ps:
            s = -math.inf
        else:
            s = math.fsum(ps)
        if math.isnan(s):
            r = math.nan
        elif math.isinf(s):
            r = math.nan if alpha == 0 else math.copysign(math.inf, s * alpha)
        else:
            r = alpha * s
        if beta != 0:
            t = beta * float(y0[i]) if not (math.isinf(y0[i]) or math.isnan(y0[i])) else (math.nan if math.isnan(y0[i]) else math.copysign(math.inf, beta * y0[i]))
            if math.isnan(r) or math.isnan(t) or (math.isinf(r) and math.isinf(t) and r != t):
                r = math.nan
            else:
                r = r + t
        out.append(r)
    return np.array(out)


def same_class(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def test_classifier_against_a_brute_force_loop():
    rng = np.random.default_rng(11)
    for trial in range(60):
        m, n = int(rng.integers(1, 40)), int(rng.integers(1, 30))
        lens = rng.integers(0, 7, m)
        rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        nnz = int(rowptr[-1])
        cols = rng.integers(0, n, nnz).astype(np.int32)
        vals, x, y0 = rng.uniform(-1, 1, nnz), rng.standard_normal(n), rng.standard_normal(m)
        for arr in (vals, x, y0):
            k = int(rng.integers(0, 4))
            if arr.size and k:
                arr[rng.integers(0, arr.size, k)] = rng.choice([np.inf, -np.inf, np.nan, 0.0], k)
        for alpha, beta in ABS + ((1.0, 1.0), (-2.0, -1.0)):
            ref, scale = sv.classify(alpha, beta, rowptr, cols, vals, x, y0)
            want = brute(alpha, beta, rowptr, cols, vals, x, y0)
            assert np.array_equal(np.isnan(ref), np.isnan(want)), (trial, alpha, beta)
            f = np.isfinite(want)
            assert np.array_equal(ref[~f & ~np.isnan(want)], want[~f & ~np.isnan(want)]), (trial, alpha, beta)
            assert np.all(np.abs(ref[f] - want[f]) <= 4e-16 * np.maximum(scale[f], 0)), (trial, alpha, beta)
            assert sv.mismatches(want, ref, scale).size == 0


def test_classifier_against_the_oracle_on_finite_inputs(oracle):
    case = sv.matrix_m()
    rng = np.random.default_rng(3)
    x, y0 = rng.standard_normal(case.n), rng.standard_normal(case.m)
    for alpha, beta in ABS + ((0.5, -2.0),):
        ref, scale = sv.classify(alpha, beta, case.rowptr, case.cols, case.vals, x, y0)
        h = oracle.host_spmv(alpha, beta, case.rowptr, case.cols, case.vals, x, y0)
        assert np.all(np.isfinite(ref))
        sv.check(h, ref, scale, ("oracle", alpha, beta))
        assert oracle.scaled_error(ref, h, alpha, beta, case.rowptr, case.cols, case.vals, x, y0) <= sv.SCALED_TOL
        # the scale is the oracle gate's own
        import scipy.sparse as sp
        want = abs(alpha) * (sp.csr_matrix((np.abs(case.vals), case.cols, case.rowptr), shape=(case.m, case.n)) @ np.abs(x)) + np.abs(beta * y0)
        assert np.allclose(scale, want, rtol=1e-13, atol=0)


def test_closed_form_corner_cases():
    inf, nan = np.inf, np.nan
    # rows: 0*Inf | +Inf and -Inf | overflow | only +Inf | only -Inf | finite | empty
    rowptr = np.array([0, 2, 4, 5, 7, 8, 10, 10], dtype=np.int32)
    cols = np.array([0, 1, 0, 2, 3, 0, 1, 2, 1, 4], dtype=np.int32)
    vals = np.array([0.0, 1.0, 1.0, 1.0, sv.BIG_VALUE, 2.0, 3.0, 5.0, 0.5, 0.25])
    x = np.array([inf, 1.0, -inf, sv.BIG_X, 4.0])
    y_nan = np.full(7, nan)
    ref, _ = sv.classify(1.0, 0.0, rowptr, cols, vals, x, y_nan)  # beta == 0 over a NaN y: never read
    assert same_class(ref, np.array([nan, nan, inf, inf, -inf, 1.5, 0.0]))
    ref, _ = sv.classify(-0.75, 0.0, rowptr, cols, vals, x, y_nan)  # a negative alpha flips an Inf
    assert same_class(ref, np.array([nan, nan, -inf, -inf, inf, -1.125, 0.0]))
    y0 = np.array([1.0, 1.0, -inf, inf, 1.0, nan, -inf])  # a non-finite y0 with beta != 0
    ref, scale = sv.classify(2.0, 0.5, rowptr, cols, vals, x, y0)
    assert same_class(ref, np.array([nan, nan, nan, inf, -inf, nan, -inf]))
    ref, scale = sv.classify(2.0, 0.5, rowptr, cols, vals, x, np.arange(7.0))
    assert ref[5] == 2.0 * 1.5 + 0.5 * 5 and scale[5] == 2.0 * 1.5 + 2.5 and ref[6] == 3.0
    ref, _ = sv.classify(0.0, 0.0, rowptr, cols, vals, x, y_nan)  # alpha == 0 is not special: 0 * Inf
    assert same_class(ref, np.array([nan, nan, nan, nan, nan, 0.0, 0.0]))
    # the comparison: class against class, either zero, the bound on finite rows
    ref, scale = np.array([nan, inf, -inf, 0.0, 1.0]), np.array([0.0, 0.0, 0.0, 0.0, 2.0])
    assert sv.mismatches(np.array([nan, inf, -inf, -0.0, 1.0 + 1e-12]), ref, scale).size == 0
    assert sv.mismatches(np.array([inf, -inf, nan, 1e-300, 1.0 + 3e-12]), ref, scale).tolist() == [0, 1, 2, 3, 4]
    assert sv.mismatches(np.array([1.0, 1.0, 1.0, nan, inf]), ref, scale).tolist() == [0, 1, 2, 3, 4]
    # the transposed form: the roles of rows and columns swapped, columns outside [0, n) dropped
    rp = np.array([0, 2, 3], dtype=np.int32)
    ci = np.array([0, 2, 7], dtype=np.int32)
    ref, scale = sv.classify_t(-1.0, 1.0, rp, ci, np.array([1.0, 0.0, nan]), np.array([inf, 1.0]), np.array([1.0, 2.0, 3.0]), 3)
    assert same_class(ref, np.array([-inf, 2.0, nan]))


@pytest.fixture(scope="module")
def case_m():
    return sv.matrix_m()


def test_matrix_m_is_what_the_gpu_tests_need(case_m):
    c = case_m
    lens = np.diff(c.rowptr)
    assert c.nnz % 4 != 0 and lens[0] == 0 and lens[-1] == 0 and 11000 <= c.m <= 13000
    assert [int(lens[r]) for r in (100, 5000, 5001, 8000, 10000, 10400)] == [700, 3000, 1, 9000, 2500, 301] and lens[99] <= 8 and lens[101] <= 8
    assert not np.isin(c.cols, c.dead).any() and set(c.dead) >= {0, c.n - 1}
    assert np.all(lens[np.unique(sv.entry_rows(c.rowptr)[c.cols == c.big])] == 1)
    rows = sv.entry_rows(c.rowptr)
    assert np.all((np.diff(c.cols) >= 0) | (np.diff(rows) > 0)), "columns ascend inside rows"
    assert c.cols.min() >= 0 and c.cols.max() < c.n
    # the poisoned entries sit where the issue asks: mid-row of the rows longer than a tile, the first and last 4-group of the 700-row, the last non-zero
    e = set(c.entries)
    assert {int(c.rowptr[5000] + 1500), int(c.rowptr[8000] + 4500), int(c.rowptr[100]), int(c.rowptr[101] - 1), c.nnz - 1} <= e


@pytest.mark.parametrize("variant", ["x", "vals", "both"])
def test_matrix_m_meets_the_caps(case_m, variant):
    c = case_m
    vals, x, y0 = c.inputs(variant)
    p = sv.products(vals, x, c.cols)
    rows = sv.entry_rows(c.rowptr)
    multi = np.diff(c.rowptr)[rows] > 1
    assert np.all(np.abs(p[np.isfinite(p) & multi]) < 1e3)
    assert np.all(np.isfinite(p[multi]) | ~np.isfinite(vals[multi]) | ~np.isfinite(x[c.cols][multi])), "overflow outside a single-entry row"
    assert np.any(np.isinf(p) & np.isfinite(vals) & np.isfinite(x[c.cols])), "no overflowing product"
    if variant != "vals":
        assert np.any((vals == 0.0) & np.isinf(x[c.cols])), "no stored zero against an Inf"
        assert np.all(np.isnan(x[c.dead]))
    for alpha, beta in ABS:
        ref, _ = sv.classify(alpha, beta, c.rowptr, c.cols, vals, x, np.full(c.m, np.nan) if (alpha, beta) == (1.0, 0.0) else y0)
        sv.assert_caps(sv.caps(c.rowptr, p, ref), (variant, alpha, beta))
        assert np.all(np.isfinite(ref[[10000, 10400]])), "the long rows that are to stay clean"


@pytest.mark.parametrize("kind", sv.L_KINDS)
def test_matrix_l_meets_the_caps(kind):
    c = sv.matrix_l(kind)
    assert (c.nnz + 255) // 256 >= 64 and (c.nnz + 255) // 256 <= 90, "about 70 chunks: the smallest the encoding is built for, with a margin"
    assert not np.isin(c.cols, c.dead).any() and c.base in c.dead and sv.chunk_base(c.cols, c.base_chunk, c.half) == c.base
    vals, x, y0 = c.inputs("x")
    assert np.isnan(x[c.base])
    p = sv.products(vals, x, c.cols)
    near = sv.entry_rows(c.rowptr) * c.n // c.m if c.half == 32767 else sv.entry_rows(c.rowptr) * 92 // 100
    assert np.any(~np.isfinite(p) & (np.abs(c.cols - near) > 2 * c.half + 500)), "no poisoned escaped entry"
    for alpha, beta in ABS:
        ref, _ = sv.classify(alpha, beta, c.rowptr, c.cols, vals, x, np.full(c.m, np.nan) if (alpha, beta) == (1.0, 0.0) else y0)
        sv.assert_caps(sv.caps(c.rowptr, p, ref), (kind, alpha, beta))
    # the record sizes the GPU test pins: the 10 %-far matrix overflows 16-int records (12 escapes) in most chunks and 64-int ones (60) in none
    esc = sv.chunk_escapes(c.cols, c.half)
    if kind == "short rows, 10 % far":
        assert (esc > 12).mean() > 0.5 and esc.max() <= 60, (esc.max(), float((esc > 12).mean()))
    assert esc.max() > 0 and esc.max() <= 60, "escapes exist and 64-int records hold them all"


def test_subnormal_sums_are_exact(case_m):
    c = case_m
    iv, kx, ky = sv.subnormal_inputs(c)
    rows = sv.entry_rows(c.rowptr)
    for alpha, beta in ((1, 0), (2, 1)):
        k = sv.subnormal_reference(alpha, beta, rows, iv * kx[c.cols], c.m, ky)
        assert 0 <= k.min() and k.max() < 2 ** 52, "a sum of 2^52 units of 2^-1074 is 2^-1022: no longer subnormal"
        assert np.all(sv.tiny(k) < 2.0 ** -1022) and np.all(sv.tiny(k) / sv.TINY == k)
        # the transposed sums (columns own the terms) stay subnormal as well
        ivt, kxt, kyt = sv.subnormal_inputs_t(c)
        kt = sv.subnormal_reference(alpha, beta, c.cols, ivt * kxt[rows], c.n, kyt)
        assert 0 <= kt.min() and kt.max() < 2 ** 52
    # numpy's own fp64 arithmetic on these inputs is exact in any order: the float reference equals the integer one
    ref, _ = sv.classify(2.0, 1.0, c.rowptr, c.cols, iv.astype(np.float64), sv.tiny(kx), sv.tiny(ky))
    assert np.array_equal(ref, sv.tiny(sv.subnormal_reference(2, 1, rows, iv * kx[c.cols], c.m, ky)))
