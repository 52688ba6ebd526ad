"""GPU suite (-m gpu) of the aggregation coarsening (spmv_acc_csr_aggregate / csr_aggregate, spmv_acc_csr_tentative_values / csr_tentative,
csr_tentative_values): the aggregates exactly against the definition restated in numpy (tests/test_agg_host.py host_csr_aggregate), the
tentative prolongator's values bit for bit against their summation order restated there (host_tentative_values), the contract of the two
entries on the device, a captured and replayed values pass, grid striding, the Galerkin product through csr_spgemm on the returned arrays
against dense numpy, exactly, and a two-level cycle that beats the smoother alone.

No speed gate: the parent commit cannot do this job, so there is no figure to hold (tools/agg_bench.py measures)."""
import ctypes
import functools

import numpy as np
import pytest

import spmv_acc_amd
from test_agg_host import TAGS, aggregates, cases, grid5_matrix, host_csr_aggregate, host_tentative_values

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev(hiplib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def same(t, a):
    return np.array_equal(t.cpu().numpy(), a)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(t, a):
    """the same bits, NaNs by position (a NaN's payload and sign are not part of the contract)"""
    got, want = t.cpu().numpy(), np.asarray(a, dtype=np.float64)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


@pytest.mark.parametrize("tag", TAGS)
def test_aggregate_is_the_host_model(torch_dev, hiplib, tag):
    torch = torch_dev
    m, (rp, ci) = cases()[tag]
    w_agg, w_rows, w_ptr, w_naggs = aggregates(tag)
    d_rp, d_ci = dev(torch, rp), dev(torch, ci)
    plans = hiplib.spmv_acc_cached_plans()
    for _ in range(2):  # twice: the same arrays
        agg, agg_ptr, agg_rows, naggs = spmv_acc_amd.csr_aggregate(m, d_rp, d_ci)
        assert agg.numel() == agg_rows.numel() == m and agg_ptr.numel() == naggs + 1 and agg.dtype == agg_rows.dtype == agg_ptr.dtype == torch.int32
        assert naggs == w_naggs and same(agg, w_agg) and same(agg_rows, w_rows) and same(agg_ptr, w_ptr[:naggs + 1]), tag
    assert hiplib.spmv_acc_cached_plans() == plans and hiplib.spmv_acc_last_error() == 0
    # the C entry: agg_ptr holds m + 1 entries (m beyond the last aggregate), nothing beyond the arrays is written
    pad = 16
    o_agg = torch.full((m + pad,), -7, dtype=torch.int32, device="cuda")
    o_rows = torch.full((m + pad,), -7, dtype=torch.int32, device="cuda")
    o_ptr = torch.full((m + 1 + pad,), -7, dtype=torch.int32, device="cuda")
    h_n = ctypes.c_int(-5)
    hiplib.spmv_acc_set_stream(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    rc = hiplib.spmv_acc_csr_aggregate(m, ci.size, ptr(d_rp), ptr(d_ci), ptr(o_agg), ptr(o_rows), ptr(o_ptr), ctypes.byref(h_n))
    torch.cuda.synchronize()
    assert rc == 0 and h_n.value == w_naggs, (rc, hiplib.spmv_acc_last_error_string())
    if m:
        assert same(o_agg[:m], w_agg) and same(o_rows[:m], w_rows) and same(o_ptr[:m + 1], w_ptr)
        assert bool((o_agg[m:] == -7).all()) and bool((o_rows[m:] == -7).all()) and bool((o_ptr[m + 1:] == -7).all())
    else:  # no rows: nothing is touched
        assert bool((o_agg == -7).all()) and bool((o_rows == -7).all()) and bool((o_ptr == -7).all())


def test_aggregate_contract(torch_dev, hiplib):
    """Each defect of the input: SPMV_ACC_ERR_BAD_ARGUMENT with its count in the error string, outputs untouched; a capture is refused."""
    torch = torch_dev
    m, (rp, ci) = cases()["grid27"]
    nnz = ci.size
    pad = 64
    d_rp = dev(torch, rp)
    o_agg = torch.full((m + pad,), -7, dtype=torch.int32, device="cuda")
    o_rows = torch.full((m + pad,), -7, dtype=torch.int32, device="cuda")
    o_ptr = torch.full((m + 1 + pad,), -7, dtype=torch.int32, device="cuda")
    h_n = ctypes.c_int(-5)
    plans = hiplib.spmv_acc_cached_plans()

    def padded(a):  # (a wrong nnz never reaches past the array: the census reads clamped extents, and the array has room beyond them anyway)
        return dev(torch, np.concatenate([a, np.zeros(pad, a.dtype)]))

    def call(rowptr=d_rp, colindex=None, mm=m, nz=nnz):
        colindex = padded(ci) if colindex is None else colindex
        rc = hiplib.spmv_acc_csr_aggregate(mm, nz, ptr(rowptr), ptr(colindex), ptr(o_agg), ptr(o_rows), ptr(o_ptr), ctypes.byref(h_n))
        msg = hiplib.spmv_acc_last_error_string().decode()
        code = hiplib.spmv_acc_last_error()
        hiplib.spmv_acc_clear_error()
        return rc, code, msg

    def untouched():
        torch.cuda.synchronize()
        return bool((o_agg == -7).all()) and bool((o_rows == -7).all()) and bool((o_ptr == -7).all()) and h_n.value == -5

    clean = ("0 ends of rowptr that are not 0 and nnz, 0 rows with a descending or out-of-range rowptr extent, 0 columns outside [0, m), "
             "0 positions where a row does not strictly ascend, 0 off-diagonal entries without their mirror")

    def refused(result, *needles):
        rc, code, msg = result
        assert rc == 2 and code == 2 and "spmv_acc_csr_aggregate:" in msg and "nothing was written" in msg and all(s in msg for s in needles), (rc, msg)
        assert untouched(), msg

    hiplib.spmv_acc_set_stream(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    # an unsymmetric pattern: the last entry (i, j) of a row moved one column on, to a row that does not point back
    i = 200
    p = int(rp[i + 1]) - 1
    j = int(ci[p])
    assert i < j < m - 1 and (j + 1) not in ci[rp[i]:rp[i + 1]]
    bad = ci.copy()
    bad[p] = j + 1  # (i, j + 1) has no mirror, and (j, i) lost its own
    refused(call(colindex=padded(bad)), clean.replace("0 off-diagonal", "2 off-diagonal"), "A + A^T")
    # a descending row (two neighbours swapped), a repeated column
    q = int(rp[100]) + 1
    bad = ci.copy()
    bad[q], bad[q + 1] = ci[q + 1], ci[q]
    refused(call(colindex=padded(bad)), "1 positions where a row does not strictly ascend")
    bad = ci.copy()
    bad[q + 1] = ci[q]
    refused(call(colindex=padded(bad)), "1 positions where a row does not strictly ascend")
    # a column >= m, and a negative one
    for value in (m, 2 ** 31 - 1, -1):
        bad = ci.copy()
        bad[rp[300] + 2] = value
        refused(call(colindex=padded(bad)), "1 columns outside [0, m)")
    # rowptr[0] != 0, a descending extent, a wrong nnz
    bad = rp.copy()
    bad[0] = 1  # (row 0 loses its first entry, the diagonal: no other count moves)
    refused(call(rowptr=dev(torch, bad)), clean.replace("0 ends of rowptr", "1 ends of rowptr"))
    bad = rp.copy()
    bad[50] = rp[51] + 1
    refused(call(rowptr=dev(torch, bad)), "1 rows with a descending or out-of-range rowptr extent")
    for nz in (nnz - 1, nnz + 1):
        refused(call(nz=nz), "1 ends of rowptr")
    # host-side refusals leave the device alone as well
    big = 2 ** 31 - 2 ** 16
    assert call(mm=big)[0] == 4 and call(nz=big)[0] == 4 and call(mm=-1)[0] == 2 and untouched()
    # no rows: nothing is touched, no aggregate
    h_zero = ctypes.c_int(-5)
    assert hiplib.spmv_acc_csr_aggregate(0, 0, None, None, None, None, None, ctypes.byref(h_zero)) == 0 and h_zero.value == 0 and untouched()
    # the wrapper raises with the counts
    with pytest.raises(spmv_acc_amd.SpmvAccError, match="1 columns outside"):
        bad = ci.copy()
        bad[rp[300] + 2] = m
        spmv_acc_amd.csr_aggregate(m, d_rp, dev(torch, bad))
    torch.cuda.synchronize()  # (no device-side fault: the context is alive)
    # inside a capture: refused with "capture", nothing enqueued, the capture survives
    d_ci = padded(ci)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    filler = torch.zeros(8, device="cuda")
    with torch.cuda.stream(s):
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            filler += 1.0
            hiplib.spmv_acc_set_stream(ctypes.c_void_p(s.cuda_stream))
            rc = hiplib.spmv_acc_csr_aggregate(m, nnz, ptr(d_rp), ptr(d_ci), ptr(o_agg), ptr(o_rows), ptr(o_ptr), ctypes.byref(h_n))
            msg = hiplib.spmv_acc_last_error_string().decode()
            hiplib.spmv_acc_clear_error()
    assert rc == 2 and "capture" in msg, (rc, msg)
    g.replay()
    torch.cuda.synchronize()
    assert untouched() and float(filler[0]) == 1.0
    del g
    # and the clean input still passes, on the same arrays
    hiplib.spmv_acc_set_stream(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    rc, code, msg = call()
    w_agg, w_rows, w_ptr, w_naggs = aggregates("grid27")
    assert rc == 0 and h_n.value == w_naggs and same(o_agg[:m], w_agg) and same(o_rows[:m], w_rows) and same(o_ptr[:m + 1], w_ptr), (rc, msg)
    assert bool((o_agg[m:] == -7).all()) and hiplib.spmv_acc_cached_plans() == plans


@functools.lru_cache(maxsize=None)
def stride_case():
    """The 7-point stencil on 44 x 44 x 44 (85 184 rows) followed by 70 000 rows that hold only their diagonal -- every one of them a root, so
    there are more aggregates than 64 workgroups of the norms pass own: (m, rowptr, colindex)."""
    n, extra = 44, 70000
    idx = np.arange(n ** 3, dtype=np.int64).reshape(n, n, n)
    alone = np.arange(n ** 3, n ** 3 + extra, dtype=np.int64)
    pairs_i, pairs_j = [idx.reshape(-1), alone], [idx.reshape(-1), alone]
    for axis in range(3):
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, n - 1), slice(1, n)
        a, c = idx[tuple(lo)].reshape(-1), idx[tuple(hi)].reshape(-1)
        pairs_i += [a, c]
        pairs_j += [c, a]
    i, j = np.concatenate(pairs_i), np.concatenate(pairs_j)
    order = np.lexsort((j, i))
    i, j = i[order], j[order]
    m = n ** 3 + extra
    rp = np.zeros(m + 1, dtype=np.int32)
    np.cumsum(np.bincount(i, minlength=m), out=rp[1:])
    return m, rp, j.astype(np.int32)


def test_agg_grid_stride_at_test_size(torch_dev, hiplib):
    """max_grid_blocks lowered to 64, the smallest cap the library honours: the rounds, the assignment passes and the values pass stride over
    155 184 rows (607 workgroups of rows), the norms pass over more than 64 tiles of 256 aggregates; the same arrays and the same bits as
    with the default grid, and the host model's."""
    torch = torch_dev
    m, rp, ci = stride_case()
    rng = np.random.default_rng(78)
    b = rng.standard_normal(m)
    d_rp, d_ci, d_b = dev(torch, rp), dev(torch, ci), dev(torch, b)
    assert m > 64 * 256

    def run():
        agg, agg_ptr, agg_rows, naggs = spmv_acc_amd.csr_aggregate(m, d_rp, d_ci)
        (_, _, p_value), (_, _, r_value), bc = spmv_acc_amd.csr_tentative(m, agg, agg_ptr, agg_rows, d_b)
        torch.cuda.synchronize()
        return tuple(t.cpu().numpy() for t in (agg, agg_ptr, agg_rows)) + (naggs,) + tuple(t.cpu().numpy() for t in (p_value, r_value, bc))

    default = run()
    try:
        assert hiplib.spmv_acc_set_tunable(b"max_grid_blocks", 64) == 0
        strided = run()
    finally:
        hiplib.spmv_acc_reset_tunables()
    assert default[3] == strided[3] > 64 * 256  # the norms pass strides over its tiles
    for k in (0, 1, 2):
        assert np.array_equal(default[k], strided[k]), k
    for k in (4, 5, 6):
        assert np.array_equal(bits(default[k]), bits(strided[k])), k
    # the definition's (the sequential model on 155 184 rows takes a second or two)
    w_agg, w_rows, w_ptr, w_naggs = host_csr_aggregate(m, rp, ci)
    assert default[3] == w_naggs and np.array_equal(default[0], w_agg) and np.array_equal(default[2], w_rows)
    assert np.array_equal(default[1], w_ptr[:w_naggs + 1])
    w_p, w_r, w_bc = host_tentative_values(m, w_naggs, w_agg, w_ptr, w_rows, b)
    assert np.array_equal(bits(default[4]), bits(w_p)) and np.array_equal(bits(default[5]), bits(w_r)) and np.array_equal(bits(default[6]), bits(w_bc))
    assert hiplib.spmv_acc_last_error() == 0


@pytest.mark.parametrize("tag", TAGS)
def test_tentative_values_are_the_host_model(torch_dev, hiplib, tag):
    """Random b, b = None, an aggregate whose b is all zero (of either sign), inf and NaN in b: bit for bit the host model, bc included --
    the double square root is correctly rounded."""
    torch = torch_dev
    m, _ = cases()[tag]
    w_agg, w_rows, w_ptr, naggs = aggregates(tag)
    d_agg, d_ptr, d_rows = dev(torch, w_agg), dev(torch, w_ptr[:naggs + 1]), dev(torch, w_rows)
    rng = np.random.default_rng(300 + m)
    plain = rng.standard_normal(m) * 10.0 ** rng.integers(-3, 4, m)
    zeroed = plain.copy()
    if naggs:
        zeroed[w_agg == naggs - 1] = 0.0
        zeroed[w_agg == 0] = -0.0
    poisoned = plain.copy()
    if m:
        poisoned[rng.integers(0, m, 3)] = [np.inf, -np.inf, np.nan]
        poisoned[rng.integers(0, m, 2)] = [1e200, 5e-324]  # a square that overflows, one that vanishes
    plans = hiplib.spmv_acc_cached_plans()
    for b in (plain, None, zeroed, poisoned):
        want_p, want_r, want_bc = host_tentative_values(m, naggs, w_agg, w_ptr, w_rows, b)
        d_b = None if b is None else dev(torch, b)
        for _ in range(2):  # twice: the same bits
            (p_rp, p_ci, p_v), (r_rp, r_ci, r_v), bc = spmv_acc_amd.csr_tentative(m, d_agg, d_ptr, d_rows, d_b)
            assert same_bits(p_v, want_p) and same_bits(r_v, want_r) and same_bits(bc, want_bc), tag
        assert same(p_rp, np.arange(m + 1)) and p_rp.dtype == torch.int32 and p_ci is d_agg and r_rp is d_ptr and r_ci is d_rows
        # without R's values: P and bc are the same, and nothing else is written
        p2 = torch.full((m + 8,), 7.25, dtype=torch.float64, device="cuda")
        bc2 = torch.full((naggs + 8,), 7.25, dtype=torch.float64, device="cuda")
        spmv_acc_amd.csr_tentative_values(m, d_agg, d_ptr, d_rows, d_b, p2[:m], None, bc2[:naggs])
        assert same_bits(p2[:m], want_p) and same_bits(bc2[:naggs], want_bc) and bool((p2[m:] == 7.25).all()) and bool((bc2[naggs:] == 7.25).all())
    if naggs and m > 1:
        zp, _, zbc = host_tentative_values(m, naggs, w_agg, w_ptr, w_rows, zeroed)
        assert zbc[0] == 0.0 and np.all(zp[w_agg == 0] == 0.0) and not np.signbit(zp[w_agg == 0]).any()
    assert hiplib.spmv_acc_cached_plans() == plans and hiplib.spmv_acc_last_error() == 0


def test_tentative_captured_and_replayed(torch_dev, hiplib):
    """The values pass captured once (two launches, one stream) and replayed after b was edited in place."""
    torch = torch_dev
    m, _ = cases()["random3000"]
    w_agg, w_rows, w_ptr, naggs = aggregates("random3000")
    d_agg, d_ptr, d_rows = dev(torch, w_agg), dev(torch, w_ptr[:naggs + 1]), dev(torch, w_rows)
    rng = np.random.default_rng(6)
    d_b = dev(torch, rng.standard_normal(m))
    p, r, bc = (torch.full((n,), -3.0, dtype=torch.float64, device="cuda") for n in (m, m, naggs))
    spmv_acc_amd.csr_tentative_values(m, d_agg, d_ptr, d_rows, d_b, p, r, bc)  # (warm: the code object is loaded outside the capture)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            spmv_acc_amd.csr_tentative_values(m, d_agg, d_ptr, d_rows, d_b, p, r, bc)
    assert hiplib.spmv_acc_last_error() == 0
    for _ in range(2):
        new_b = rng.standard_normal(m) * 10.0 ** rng.integers(-2, 3, m)
        d_b.copy_(dev(torch, new_b))
        for t in (p, r, bc):
            t.fill_(-3.0)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want_p, want_r, want_bc = host_tentative_values(m, naggs, w_agg, w_ptr, w_rows, new_b)
        assert same_bits(p, want_p) and same_bits(r, want_r) and same_bits(bc, want_bc)
    del g


def test_tentative_contract(torch_dev, hiplib):
    """Crafted maps read nothing out of bounds and give the documented zeros; overlaps and bad sizes are refused before any launch."""
    torch = torch_dev
    m, _ = cases()["fem"]
    w_agg, w_rows, w_ptr, naggs = aggregates("fem")
    rng = np.random.default_rng(43)
    b = rng.standard_normal(m)
    d_b = dev(torch, b)
    pad = 64
    bufs = [torch.full((n + 2 * pad,), 7.25, dtype=torch.float64, device="cuda") for n in (m, m, naggs)]
    p, r, bc = (buf[pad:pad + n] for buf, n in zip(bufs, (m, m, naggs)))

    def guards():
        torch.cuda.synchronize()
        return all(bool((buf[:pad] == 7.25).all()) and bool((buf[pad + n:] == 7.25).all()) for buf, n in zip(bufs, (m, m, naggs)))

    def check(agg, agg_ptr, agg_rows):
        spmv_acc_amd.csr_tentative_values(m, dev(torch, agg), dev(torch, agg_ptr[:naggs + 1]), dev(torch, agg_rows), d_b, p, r, bc)
        want = host_tentative_values(m, naggs, agg, agg_ptr, agg_rows, b)
        assert same_bits(p, want[0]) and same_bits(r, want[1]) and same_bits(bc, want[2]) and guards()
        return want

    wild = np.array([-1, naggs, naggs + 7, 2 ** 31 - 1, -2 ** 31, -naggs] * 5, dtype=np.int64).astype(np.int32)
    # agg outside [0, naggs): +0.0 in P, the other rows as before
    clean = check(w_agg, w_ptr, w_rows)
    hit = rng.choice(m, 30, replace=False)
    bad = w_agg.copy()
    bad[hit] = wild
    got = check(bad, w_ptr, w_rows)
    assert np.all(got[0][hit] == 0.0) and np.array_equal(np.delete(got[0], hit), np.delete(clean[0], hit)) and np.array_equal(got[2], clean[2])
    # agg_rows outside [0, m): +0.0 to the norm and in R
    bad = w_rows.copy()
    rows_wild = np.array([-1, m, m + 7, 2 ** 31 - 1, -2 ** 31, -m] * 5, dtype=np.int64).astype(np.int32)
    bad[hit] = rows_wild
    got = check(w_agg, w_ptr, bad)
    assert np.all(got[1][hit] == 0.0) and np.all(np.isfinite(got[2]))
    # an agg_ptr that descends, leaves [0, m] or is constant: runs are clamped, empty runs give bc = +0.0 and zeros in P
    for craft in (w_ptr[::-1].copy(), np.where(np.arange(m + 1) % 2 == 0, -5, m + 1000).astype(np.int32), np.full(m + 1, 3, np.int32),
                  np.concatenate([[0], np.full(m, m, np.int32)]).astype(np.int32)):
        got = check(w_agg, craft, w_rows)
        assert np.all(np.isfinite(got[0])) and np.all(got[2] >= 0.0)
    got = check(w_agg, np.full(m + 1, 3, np.int32), w_rows)
    assert np.all(got[2] == 0.0) and np.all(got[0] == 0.0)
    # refusals on the host: nothing launched
    for t in (p, r, bc):
        t.fill_(-3.0)
    d_agg, d_ptr, d_rows = dev(torch, w_agg), dev(torch, w_ptr[:naggs + 1]), dev(torch, w_rows)
    hiplib.spmv_acc_set_stream(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    def call(mm=m, na=naggs, bb=d_b, pp=p, rr=r, cc=bc, agg=d_agg):
        rc = hiplib.spmv_acc_csr_tentative_values(mm, na, ptr(agg), ptr(d_ptr), ptr(d_rows), ptr(bb), ptr(pp), ptr(rr), ptr(cc))
        msg = hiplib.spmv_acc_last_error_string().decode()
        hiplib.spmv_acc_clear_error()
        return rc, msg

    assert "b overlaps an output" in call(bb=p)[1] and "b overlaps an output" in call(bb=r)[1] and "b overlaps an output" in call(bb=bufs[0][pad + m - 1:])[1]
    assert "b overlaps an output" in call(bb=bufs[2][pad - 3:])[1] and "overlap" in call(cc=p[5:])[1] and "overlap" in call(rr=p)[1]
    assert call(mm=-1)[0] == 2 and call(na=-1)[0] == 2 and call(agg=None)[0] == 2 and call(pp=None)[0] == 2 and call(cc=None)[0] == 2
    big = 2 ** 31 - 2 ** 16
    assert call(mm=big)[0] == 4 and call(na=big)[0] == 4
    torch.cuda.synchronize()
    assert all(bool((t == -3.0).all()) for t in (p, r, bc)) and guards()
    with pytest.raises(spmv_acc_amd.SpmvAccError, match="overlaps"):
        spmv_acc_amd.csr_tentative_values(m, d_agg, d_ptr, d_rows, p, p, r, bc)
    assert hiplib.spmv_acc_last_error() == 0
    # no rows: nothing to do
    assert hiplib.spmv_acc_csr_tentative_values(0, 0, None, None, None, None, None, None, None) == 0


def dense(m, n, rp, ci, v):
    D = np.zeros((m, n))
    np.add.at(D, (np.repeat(np.arange(m), np.diff(rp)), ci), v)
    return D


def test_galerkin_product_is_exact(torch_dev, hiplib):
    """The 24 x 24 five-point grid (values 4 and -1) with the unit-valued P: A_c = R (A P), formed only by csr_spgemm on the arrays the two
    entries returned, is dense numpy's P^T A P exactly -- every value is an integer."""
    torch = torch_dev
    m, (rp, ci, v) = grid5_matrix(24)
    d_rp, d_ci, d_v = dev(torch, rp), dev(torch, ci), dev(torch, v)
    agg, agg_ptr, agg_rows, naggs = spmv_acc_amd.csr_aggregate(m, d_rp, d_ci)
    (p_rp, p_ci, _), (r_rp, r_ci, _), _ = spmv_acc_amd.csr_tentative(m, agg, agg_ptr, agg_rows)
    ones = torch.ones(m, dtype=torch.float64, device="cuda")
    AP = spmv_acc_amd.csr_spgemm(m, m, naggs, d_rp, d_ci, d_v, p_rp, p_ci, ones)
    c_rp, c_ci, c_v = spmv_acc_amd.csr_spgemm(naggs, m, naggs, r_rp, r_ci, ones, *AP)
    torch.cuda.synchronize()
    P = np.zeros((m, naggs))
    P[np.arange(m), agg.cpu().numpy()] = 1.0
    want = P.T @ dense(m, m, rp, ci, v) @ P
    got = dense(naggs, naggs, c_rp.cpu().numpy(), c_ci.cpu().numpy(), c_v.cpu().numpy())
    assert naggs == 84 and np.array_equal(got, want) and np.array_equal(got, got.T)
    assert np.all(np.diff(c_rp.cpu().numpy()) > 0) and np.all(want.sum(axis=1) >= 0) and want.sum() == dense(m, m, rp, ci, v).sum()
    # R is P transposed: the same product with the structure of a transposed P from the host
    assert np.array_equal(dense(naggs, m, r_rp.cpu().numpy(), r_ci.cpu().numpy(), np.ones(m)), P.T)
    assert hiplib.spmv_acc_last_error() == 0


def test_it_coarsens(torch_dev, hiplib):
    """Ten two-level cycles on the 24 x 24 grid with the normalised P -- one symmetric csr_gs_sweep, the coarse correction with A_c = R A P
    (csr_spgemm) solved densely on the host, one symmetric sweep -- leave a smaller residual than twenty symmetric sweeps alone: the same
    smoothing work, so the coarse space is what makes the difference.  A condition, not a tuned number."""
    torch = torch_dev
    m, (rp, ci, v) = grid5_matrix(24)
    A = dense(m, m, rp, ci, v)
    d_rp, d_ci, d_v = dev(torch, rp), dev(torch, ci), dev(torch, v)
    agg, agg_ptr, agg_rows, naggs = spmv_acc_amd.csr_aggregate(m, d_rp, d_ci)
    P, R, bc = spmv_acc_amd.csr_tentative(m, agg, agg_ptr, agg_rows)
    AP = spmv_acc_amd.csr_spgemm(m, m, naggs, d_rp, d_ci, d_v, *P)
    c_rp, c_ci, c_v = spmv_acc_amd.csr_spgemm(naggs, m, naggs, *R, *AP)
    torch.cuda.synchronize()
    h_agg, h_p = agg.cpu().numpy(), P[2].cpu().numpy()
    Pd = np.zeros((m, naggs))
    Pd[np.arange(m), h_agg] = h_p
    Ac = dense(naggs, naggs, c_rp.cpu().numpy(), c_ci.cpu().numpy(), c_v.cpu().numpy())
    assert np.allclose(Ac, Pd.T @ A @ Pd, rtol=0, atol=1e-13) and np.allclose(Pd.T @ Pd, np.eye(naggs), rtol=0, atol=1e-15)
    _, color_rows, color_ptr, _ = spmv_acc_amd.csr_color(m, d_rp, d_ci)
    rng = np.random.default_rng(19)
    b = rng.standard_normal(m)
    d_b = dev(torch, b)

    def sweep(x):
        spmv_acc_amd.csr_gs_sweep(m, d_rp, d_ci, d_v, color_ptr, color_rows, d_b, x, omega=1.0, direction="symmetric")

    def residual(x):
        return float(np.linalg.norm(b - A @ x.cpu().numpy()))

    x = torch.zeros(m, dtype=torch.float64, device="cuda")
    for _ in range(10):
        sweep(x)
        xh = x.cpu().numpy()
        xh = xh + Pd @ np.linalg.solve(Ac, Pd.T @ (b - A @ xh))
        x.copy_(dev(torch, xh))
        sweep(x)
    cycles = residual(x)
    x = torch.zeros(m, dtype=torch.float64, device="cuda")
    for _ in range(20):
        sweep(x)
    alone = residual(x)
    print(f"residual norms (|b| = {np.linalg.norm(b):.3e}): ten two-level cycles {cycles:.3e}, twenty symmetric sweeps alone {alone:.3e}")
    assert cycles < alone
    assert hiplib.spmv_acc_last_error() == 0
