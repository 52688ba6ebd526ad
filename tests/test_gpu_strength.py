"""GPU suite (-m gpu) of the strength-of-connection filter and the prolongator smoother (spmv_acc_csr_strength / csr_strength,
spmv_acc_csr_strength_values / csr_strength_values, csr_smooth_prolongator): the kept pattern and the partition exactly against the definition
restated in numpy (tests/test_strength_host.py host_csr_strength), the lumped diagonal, the filtered matrix and the smoother bit for bit against
host_strength_values, the contract of the two entries on the device, a captured and replayed values pass, grid striding, the composition with
csr_aggregate at the tie, and two-level cycles on an anisotropic grid in which the filter and the smoothed prolongator each pay.

No speed gate: the parent commit cannot do this job, so there is no figure to hold (tools/strength_bench.py measures)."""
import ctypes

import numpy as np
import pytest

import spmv_acc_amd
from test_agg_host import grid5_matrix
from test_gpu_agg import stride_case
from test_strength_host import TAGS, cases, host_csr_strength, host_strength_values, strength

pytestmark = pytest.mark.gpu

OMEGAS = (0.0, 2.0 / 3.0, 1.0, -0.5)


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
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


@pytest.mark.parametrize("tag", TAGS)
def test_strength_is_the_host_model(torch_dev, hiplib, tag):
    torch = torch_dev
    m, (rp, ci, v), theta = cases()[tag]
    nnz = ci.size
    w_rp, w_ci, w_map, w_dp, w_nnz_s, w_no_diag, _ = strength(tag)
    w_val, w_diag = host_strength_values(m, w_nnz_s, w_rp, w_ci, w_map, w_dp, v)
    d_rp, d_ci, d_v = dev(torch, rp), dev(torch, ci), dev(torch, v)
    plans = hiplib.spmv_acc_cached_plans()
    for _ in range(2):  # twice: the same arrays
        (s_rp, s_ci, s_v), smap, drop_ptr, diag, no_diag = spmv_acc_amd.csr_strength(m, d_rp, d_ci, d_v, theta)
        assert s_rp.numel() == drop_ptr.numel() == m + 1 and smap.numel() == nnz and s_ci.numel() == s_v.numel() == w_nnz_s and diag.numel() == m
        assert s_rp.dtype == s_ci.dtype == smap.dtype == drop_ptr.dtype == torch.int32 and s_v.dtype == diag.dtype == torch.float64
        assert no_diag == w_no_diag and same(s_rp, w_rp) and same(s_ci, w_ci) and same(smap, w_map) and same(drop_ptr, w_dp), tag
        assert same_bits(s_v, w_val) and same_bits(diag, w_diag), tag
    assert hiplib.spmv_acc_cached_plans() == plans and hiplib.spmv_acc_last_error() == 0
    # the C entry: nothing beyond nnz_s, nnz or m + 1 entries is written
    pad = 16
    o_rp = torch.full((m + 1 + pad,), -7, dtype=torch.int32, device="cuda")
    o_dp = torch.full((m + 1 + pad,), -7, dtype=torch.int32, device="cuda")
    o_ci = torch.full((nnz + pad,), -7, dtype=torch.int32, device="cuda")
    o_map = torch.full((nnz + pad,), -7, dtype=torch.int32, device="cuda")
    h_s, h_d = ctypes.c_int(-5), ctypes.c_int(-6)
    hiplib.spmv_acc_set_stream(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    rc = hiplib.spmv_acc_csr_strength(m, nnz, ptr(d_rp), ptr(d_ci), ptr(d_v), theta, ptr(o_rp), ptr(o_ci), ptr(o_map), ptr(o_dp), ctypes.byref(h_s),
                                      ctypes.byref(h_d))
    torch.cuda.synchronize()
    assert rc == 0 and h_s.value == w_nnz_s and (h_d.value == w_no_diag or m == 0), (rc, hiplib.spmv_acc_last_error_string())
    if m:
        assert same(o_rp[:m + 1], w_rp) and same(o_dp[:m + 1], w_dp) and same(o_ci[:w_nnz_s], w_ci) and same(o_map[:nnz], w_map)
        assert bool((o_rp[m + 1:] == -7).all()) and bool((o_dp[m + 1:] == -7).all()) and bool((o_ci[w_nnz_s:] == -7).all()) and bool((o_map[nnz:] == -7).all())
    else:  # no rows: nothing is touched
        assert h_d.value == 0 and all(bool((t == -7).all()) for t in (o_rp, o_dp, o_ci, o_map))


@pytest.mark.parametrize("tag", TAGS)
def test_strength_values_are_the_host_model(torch_dev, hiplib, tag):
    """Both modes bit for bit, and a second call after the values of A changed in place refreshes them on the kept map."""
    torch = torch_dev
    m, (rp, ci, v), _ = cases()[tag]
    w_rp, w_ci, w_map, w_dp, nnz_s, _, _ = strength(tag)
    d_rp, d_ci, d_map, d_dp, d_v = dev(torch, w_rp), dev(torch, w_ci), dev(torch, w_map), dev(torch, w_dp), dev(torch, v)
    pad = 8
    s_buf = torch.full((nnz_s + pad,), 7.25, dtype=torch.float64, device="cuda")
    g_buf = torch.full((m + pad,), 7.25, dtype=torch.float64, device="cuda")
    rng = np.random.default_rng(500 + m)
    other = v * rng.uniform(0.5, 2.0, v.size)
    plans = hiplib.spmv_acc_cached_plans()
    for values in (v, other):
        d_v.copy_(dev(torch, values))  # in place: the same device array
        for omega in OMEGAS:
            want_s, want_d = host_strength_values(m, nnz_s, w_rp, w_ci, w_map, w_dp, values, omega)
            spmv_acc_amd.csr_strength_values(m, d_rp, d_ci, d_map, d_dp, d_v, s_buf[:nnz_s], g_buf[:m], omega)
            assert same_bits(s_buf[:nnz_s], want_s) and same_bits(g_buf[:m], want_d), (tag, omega)
            assert bool((s_buf[nnz_s:] == 7.25).all()) and bool((g_buf[m:] == 7.25).all())
    assert hiplib.spmv_acc_cached_plans() == plans and hiplib.spmv_acc_last_error() == 0


def test_strength_values_captured_and_replayed(torch_dev, hiplib):
    """The values pass captured once (two launches, one stream) and replayed after the values of A were edited in place."""
    torch = torch_dev
    tag = "random3000_uns"
    m, (rp, ci, v), _ = cases()[tag]
    w_rp, w_ci, w_map, w_dp, nnz_s, _, _ = strength(tag)
    d_rp, d_ci, d_map, d_dp, d_v = dev(torch, w_rp), dev(torch, w_ci), dev(torch, w_map), dev(torch, w_dp), dev(torch, v)
    s_v = torch.full((nnz_s,), -3.0, dtype=torch.float64, device="cuda")
    diag = torch.full((m,), -3.0, dtype=torch.float64, device="cuda")
    rng = np.random.default_rng(7)
    for omega in (0.0, 2.0 / 3.0):
        spmv_acc_amd.csr_strength_values(m, d_rp, d_ci, d_map, d_dp, d_v, s_v, diag, omega)  # (warm: the code object is loaded outside the capture)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=s):
                spmv_acc_amd.csr_strength_values(m, d_rp, d_ci, d_map, d_dp, d_v, s_v, diag, omega)
        assert hiplib.spmv_acc_last_error() == 0
        for _ in range(2):
            new_v = v * rng.uniform(0.5, 2.0, v.size)
            d_v.copy_(dev(torch, new_v))
            s_v.fill_(-3.0)
            diag.fill_(-3.0)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            want_s, want_d = host_strength_values(m, nnz_s, w_rp, w_ci, w_map, w_dp, new_v, omega)
            assert same_bits(s_v, want_s) and same_bits(diag, want_d), omega
        del g


def test_strength_contract(torch_dev, hiplib):
    """Each defect of the input: SPMV_ACC_ERR_BAD_ARGUMENT with its count in the error string, outputs untouched, h_nnz_s unchanged; a capture
    is refused."""
    torch = torch_dev
    tag = "grid27_sym"
    m, (rp, ci, v), theta = cases()[tag]
    nnz = ci.size
    pad = 64
    d_rp = dev(torch, rp)
    o_rp = torch.full((m + 1 + pad,), -7, dtype=torch.int32, device="cuda")
    o_dp = torch.full((m + 1 + pad,), -7, dtype=torch.int32, device="cuda")
    o_ci = torch.full((nnz + pad,), -7, dtype=torch.int32, device="cuda")
    o_map = torch.full((nnz + pad,), -7, dtype=torch.int32, device="cuda")
    h_s, h_d = ctypes.c_int(-5), ctypes.c_int(-6)
    plans = hiplib.spmv_acc_cached_plans()

    def padded(a):  # (a wrong nnz never reaches past the array: the census reads clamped extents, and the array has room beyond them anyway)
        return dev(torch, np.concatenate([a, np.zeros(pad, a.dtype)]))

    d_v = padded(v)

    def call(rowptr=d_rp, colindex=None, mm=m, nz=nnz, th=theta):
        colindex = padded(ci) if colindex is None else colindex
        rc = hiplib.spmv_acc_csr_strength(mm, nz, ptr(rowptr), ptr(colindex), ptr(d_v), th, ptr(o_rp), ptr(o_ci), ptr(o_map), ptr(o_dp),
                                          ctypes.byref(h_s), ctypes.byref(h_d))
        msg = hiplib.spmv_acc_last_error_string().decode()
        code = hiplib.spmv_acc_last_error()
        hiplib.spmv_acc_clear_error()
        return rc, code, msg

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == -7).all()) for t in (o_rp, o_dp, o_ci, o_map)) and h_s.value == -5 and h_d.value == -6

    clean = ("0 ends of rowptr that are not 0 and nnz, 0 rows with a descending or out-of-range rowptr extent, 0 columns outside [0, m), "
             "0 positions where a row does not strictly ascend, 0 off-diagonal entries without their mirror")

    def refused(result, *needles):
        rc, code, msg = result
        assert rc == 2 and code == 2 and "spmv_acc_csr_strength:" in msg and "nothing was written" in msg and all(s in msg for s in needles), (rc, msg)
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
    for th in (-1.0, float("nan"), float("inf")):
        rc, code, msg = call(th=th)
        assert rc == 2 and "theta" in msg and untouched()
    # no rows: nothing is touched
    h_zero, h_zd = ctypes.c_int(-5), ctypes.c_int(-5)
    assert hiplib.spmv_acc_csr_strength(0, 0, None, None, None, theta, None, None, None, None, ctypes.byref(h_zero), ctypes.byref(h_zd)) == 0
    assert h_zero.value == 0 and untouched()
    # the wrapper raises with the counts
    with pytest.raises(spmv_acc_amd.SpmvAccError, match="1 columns outside"):
        bad = ci.copy()
        bad[rp[300] + 2] = m
        spmv_acc_amd.csr_strength(m, d_rp, dev(torch, bad), dev(torch, v), theta)
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
            rc = hiplib.spmv_acc_csr_strength(m, nnz, ptr(d_rp), ptr(d_ci), ptr(d_v), theta, ptr(o_rp), ptr(o_ci), ptr(o_map), ptr(o_dp),
                                              ctypes.byref(h_s), ctypes.byref(h_d))
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
    w_rp, w_ci, w_map, w_dp, w_nnz_s, w_no_diag, _ = strength(tag)
    assert rc == 0 and h_s.value == w_nnz_s and h_d.value == w_no_diag, (rc, msg)
    assert same(o_rp[:m + 1], w_rp) and same(o_dp[:m + 1], w_dp) and same(o_ci[:w_nnz_s], w_ci) and same(o_map[:nnz], w_map)
    assert bool((o_ci[w_nnz_s:] == -7).all()) and bool((o_map[nnz:] == -7).all()) and hiplib.spmv_acc_cached_plans() == plans


def test_strength_values_contract(torch_dev, hiplib):
    """Crafted maps and pointers read nothing out of bounds, give the documented +0.0s and clamps and write nothing outside [0, nnz_s) and
    [0, m); overlaps and bad sizes are refused before any launch."""
    torch = torch_dev
    tag = "fem_uns"
    m, (rp, ci, v), _ = cases()[tag]
    nnz = ci.size
    w_rp, w_ci, w_map, w_dp, nnz_s, _, _ = strength(tag)
    d_v = dev(torch, v)
    pad = 64
    bufs = [torch.full((n + 2 * pad,), 7.25, dtype=torch.float64, device="cuda") for n in (nnz_s, m)]
    s_v, diag = (buf[pad:pad + n] for buf, n in zip(bufs, (nnz_s, m)))

    def guards():
        torch.cuda.synchronize()
        return all(bool((buf[:pad] == 7.25).all()) and bool((buf[pad + n:] == 7.25).all()) for buf, n in zip(bufs, (nnz_s, m)))

    def check(s_rowptr, s_colindex, smap, drop_ptr, omega):
        spmv_acc_amd.csr_strength_values(m, dev(torch, s_rowptr), dev(torch, s_colindex), dev(torch, smap), dev(torch, drop_ptr), d_v, s_v, diag, omega)
        want = host_strength_values(m, nnz_s, s_rowptr, s_colindex, smap, drop_ptr, v, omega)
        assert same_bits(s_v, want[0]) and same_bits(diag, want[1]) and guards()
        return want

    rng = np.random.default_rng(44)
    for omega in (0.0, 2.0 / 3.0):
        clean = check(w_rp, w_ci, w_map, w_dp, omega)
        # map indices outside [0, nnz), among the kept and among the dropped: +0.0 in the values and in the lumps
        wild = np.array([-1, nnz, nnz + 7, 2 ** 31 - 1, -2 ** 31, -nnz] * 5, dtype=np.int64).astype(np.int32)
        hit = np.concatenate([rng.choice(nnz_s, 20, replace=False), nnz_s + rng.choice(nnz - nnz_s, 10, replace=False)])
        bad = w_map.copy()
        bad[hit] = wild
        got = check(w_rp, w_ci, bad, w_dp, omega)
        if omega == 0.0:
            off = hit[:20][w_ci[hit[:20]] != np.searchsorted(w_rp, hit[:20], side="right") - 1]
            assert off.size and np.all(got[0][off] == 0.0)
        assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1]))
        # a drop_ptr that descends, leaves [0, nnz] or is constant: runs are clamped, an empty run leaves the diagonal's bits
        for craft in (w_dp[::-1].copy(), np.where(np.arange(m + 1) % 2 == 0, -5, nnz + 1000).astype(np.int32), np.full(m + 1, 3, np.int32),
                      np.concatenate([[0], np.full(m, nnz, np.int32)]).astype(np.int32)):
            got = check(w_rp, w_ci, w_map, craft, omega)
            assert np.all(np.isfinite(got[1]))
        got = check(w_rp, w_ci, w_map, np.full(m + 1, 3, np.int32), omega)
        on_diag = w_ci == (np.searchsorted(w_rp, np.arange(nnz_s), side="right") - 1)
        assert np.array_equal(bits(got[1]), bits(v[w_map[:nnz_s]][on_diag]))  # no lump anywhere: the stored diagonals, bit for bit
        # an s_rowptr that descends, leaves [0, nnz_s] or is constant: rows are searched inside [0, m) and clamped
        for craft in (w_rp[::-1].copy(), np.where(np.arange(m + 1) % 2 == 0, -5, nnz_s + 1000).astype(np.int32), np.full(m + 1, 3, np.int32),
                      np.concatenate([[0], np.full(m, nnz_s, np.int32)]).astype(np.int32)):
            got = check(craft, w_ci, w_map, w_dp, omega)
            assert got[0].size == nnz_s
        # an s_colindex out of range: never an address, only compared
        bad = w_ci.copy()
        bad[rng.choice(nnz_s, 30, replace=False)] = wild
        check(w_rp, bad, w_map, w_dp, omega)
        assert np.array_equal(bits(check(w_rp, w_ci, w_map, w_dp, omega)[0]), bits(clean[0]))
    # refusals on the host: nothing launched
    s_v.fill_(-3.0)
    diag.fill_(-3.0)
    d_rp, d_ci, d_map, d_dp = dev(torch, w_rp), dev(torch, w_ci), dev(torch, w_map), dev(torch, w_dp)
    hiplib.spmv_acc_set_stream(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    def call(mm=m, nz=nnz, ns=nnz_s, vv=d_v, ss=s_v, dd=diag, srp=d_rp, omega=0.5):
        rc = hiplib.spmv_acc_csr_strength_values(mm, nz, ns, ptr(srp), ptr(d_ci), ptr(d_map), ptr(d_dp), ptr(vv), omega, ptr(ss), ptr(dd))
        msg = hiplib.spmv_acc_last_error_string().decode()
        hiplib.spmv_acc_clear_error()
        return rc, msg

    assert "overlaps an output" in call(vv=bufs[0][pad + nnz_s - 1:])[1] and "overlaps an output" in call(dd=s_v[5:])[1]
    assert "overlaps an output" in call(ss=d_v[3:])[1] and "diag overlaps value" in call(dd=d_v[nnz - m:])[1]  # (diag's m doubles end where value ends)
    assert call(mm=-1)[0] == 2 and call(nz=-1)[0] == 2 and call(ns=-1)[0] == 2 and call(ns=nnz + 1)[0] == 2 and call(srp=None)[0] == 2
    assert call(ss=None)[0] == 2 and call(dd=None)[0] == 2 and call(vv=None)[0] == 2
    assert call(omega=float("nan"))[0] == 2 and call(omega=float("inf"))[0] == 2
    big = 2 ** 31 - 2 ** 16
    assert call(mm=big)[0] == 4 and call(nz=big)[0] == 4
    torch.cuda.synchronize()
    assert bool((s_v == -3.0).all()) and bool((diag == -3.0).all()) and guards()
    with pytest.raises(spmv_acc_amd.SpmvAccError, match="overlaps"):
        spmv_acc_amd.csr_strength_values(m, d_rp, d_ci, d_map, d_dp, d_v, d_v[:nnz_s], diag, 0.5)
    assert hiplib.spmv_acc_last_error() == 0
    # no rows: nothing to do
    assert hiplib.spmv_acc_csr_strength_values(0, 0, 0, None, None, None, None, None, 0.5, None, None) == 0


def test_strength_grid_stride_at_test_size(torch_dev, hiplib):
    """max_grid_blocks lowered to 64, the smallest cap the library honours: every pass strides over 155 184 rows and 666 400 entries with seeded
    anisotropic values; the same arrays and the same bits as with the default grid, and the host model's."""
    torch = torch_dev
    m, rp, ci = stride_case()
    nnz = ci.size
    rng = np.random.default_rng(79)
    row = np.repeat(np.arange(m), np.diff(rp))
    scale = np.where(np.abs(ci - row) == 1, 1.0, np.where(np.abs(ci - row) == 44, 0.3, 0.01))  # strong along a line, middling and weak across
    v = np.where(ci == row, rng.uniform(2.0, 3.0, nnz), -scale * rng.uniform(0.5, 1.5, nnz))
    theta, omega = 0.25, 2.0 / 3.0
    d_rp, d_ci, d_v = dev(torch, rp), dev(torch, ci), dev(torch, v)
    assert m > 64 * 256 and nnz > 64 * 1024

    def run():
        (s_rp, s_ci, s_v), smap, drop_ptr, diag, no_diag = spmv_acc_amd.csr_strength(m, d_rp, d_ci, d_v, theta)
        m_v = torch.empty_like(s_v)
        diag2 = torch.empty_like(diag)
        spmv_acc_amd.csr_strength_values(m, s_rp, s_ci, smap, drop_ptr, d_v, m_v, diag2, omega)
        torch.cuda.synchronize()
        return tuple(t.cpu().numpy() for t in (s_rp, s_ci, smap, drop_ptr)) + (no_diag,) + tuple(t.cpu().numpy() for t in (s_v, diag, m_v, diag2))

    default = run()
    try:
        assert hiplib.spmv_acc_set_tunable(b"max_grid_blocks", 64) == 0
        strided = run()
    finally:
        hiplib.spmv_acc_reset_tunables()
    for k in (0, 1, 2, 3):
        assert np.array_equal(default[k], strided[k]), k
    assert default[4] == strided[4] == 0
    for k in (5, 6, 7, 8):
        assert np.array_equal(bits(default[k]), bits(strided[k])), k
    w_rp, w_ci, w_map, w_dp, nnz_s, no_diag, _ = host_csr_strength(m, rp, ci, v, theta)
    assert nnz_s > 64 * 1024 and 0.3 * nnz < nnz - nnz_s < 0.7 * nnz  # the values pass strides over its tiles; a good part drops
    assert np.array_equal(default[0], w_rp) and np.array_equal(default[1], w_ci) and np.array_equal(default[2], w_map) and np.array_equal(default[3], w_dp)
    w_val, w_diag = host_strength_values(m, nnz_s, w_rp, w_ci, w_map, w_dp, v)
    w_m, _ = host_strength_values(m, nnz_s, w_rp, w_ci, w_map, w_dp, v, omega)
    assert np.array_equal(bits(default[5]), bits(w_val)) and np.array_equal(bits(default[6]), bits(w_diag)) and np.array_equal(bits(default[8]), bits(w_diag))
    assert np.array_equal(bits(default[7]), bits(w_m))
    assert hiplib.spmv_acc_last_error() == 0


def test_tie_composes_exactly(torch_dev, hiplib):
    """grid5_matrix(24) at the tie theta: S = A, so csr_aggregate on S is csr_aggregate on A (84 aggregates), and A_F's values are A's, bit for bit."""
    torch = torch_dev
    m, (rp, ci, v) = grid5_matrix(24)
    d_rp, d_ci, d_v = dev(torch, rp), dev(torch, ci), dev(torch, v)
    (s_rp, s_ci, s_v), smap, drop_ptr, diag, no_diag = spmv_acc_amd.csr_strength(m, d_rp, d_ci, d_v, 0.25)
    assert same(s_rp, rp) and same(s_ci, ci) and same_bits(s_v, v) and same(smap, np.arange(ci.size)) and bool((drop_ptr == ci.size).all()) and no_diag == 0
    assert bool((diag == 4.0).all())
    on_s = spmv_acc_amd.csr_aggregate(m, s_rp, s_ci)
    on_a = spmv_acc_amd.csr_aggregate(m, d_rp, d_ci)
    assert on_s[3] == on_a[3] == 84 and all(same(a, b.cpu().numpy()) for a, b in zip(on_s[:3], on_a[:3]))
    assert hiplib.spmv_acc_last_error() == 0


def dense(m, n, rp, ci, v):
    D = np.zeros((m, n))
    np.add.at(D, (np.repeat(np.arange(m), np.diff(rp)), ci), v)
    return D


def host(*ts):
    return tuple(t.cpu().numpy() for t in ts)


def test_it_is_worth_it(torch_dev, hiplib):
    """Ten two-level cycles on aniso24 (couplings -1 along a grid line, -0.01 across), built as test_gpu_agg.test_it_coarsens: colour once, one
    symmetric csr_gs_sweep before and after the coarse correction, the coarse matrix by csr_spgemm with R = csr_transpose(P), solved densely on the
    host.  (a) aggregates of A's own pattern with the tentative P, (b) aggregates of S with the tentative P, (c) aggregates of S with the
    smoothed P at omega = 2/3: each step must pay, res_c < res_b < res_a.  A condition, not a tuned number: with lexicographic Gauss-Seidel a
    numpy restatement gives 3.9e-2, 1.1e-3 and 1.8e-6, factors above 30 that the multicolour order cannot turn round (with it, on an MI355X:
    9.2e-2, 2.2e-3 and 1.3e-5)."""
    torch = torch_dev
    m, (rp, ci, v), theta = cases()["aniso24"]
    nnz = ci.size
    A = dense(m, m, rp, ci, v)
    d_rp, d_ci, d_v = dev(torch, rp), dev(torch, ci), dev(torch, v)
    S, smap, drop_ptr, diag, _ = spmv_acc_amd.csr_strength(m, d_rp, d_ci, d_v, theta)
    _, color_rows, color_ptr, _ = spmv_acc_amd.csr_color(m, d_rp, d_ci)
    rng = np.random.default_rng(19)
    b = rng.standard_normal(m)
    d_b = dev(torch, b)
    omega = 2.0 / 3.0

    def level(pattern, smoothed):
        agg, agg_ptr, agg_rows, naggs = spmv_acc_amd.csr_aggregate(m, *pattern)
        T, _, _ = spmv_acc_amd.csr_tentative(m, agg, agg_ptr, agg_rows)
        P = spmv_acc_amd.csr_smooth_prolongator(m, naggs, S[0], S[1], smap, drop_ptr, d_v, T, omega) if smoothed else T
        R = spmv_acc_amd.csr_transpose(m, naggs, int(P[1].numel()), *P)
        AP = spmv_acc_amd.csr_spgemm(m, m, naggs, d_rp, d_ci, d_v, *P)
        Ac = spmv_acc_amd.csr_spgemm(naggs, m, naggs, *R[:3], *AP)
        torch.cuda.synchronize()
        return naggs, dense(m, naggs, *host(*T)), dense(m, naggs, *host(*P)), dense(naggs, m, *host(*R[:3])), dense(naggs, naggs, *host(*Ac))

    def cycles(Pd, Rd, Ac):
        x = torch.zeros(m, dtype=torch.float64, device="cuda")
        for _ in range(10):
            spmv_acc_amd.csr_gs_sweep(m, d_rp, d_ci, d_v, color_ptr, color_rows, d_b, x, omega=1.0, direction="symmetric")
            xh = x.cpu().numpy()
            xh = xh + Pd @ np.linalg.solve(Ac, Rd @ (b - A @ xh))
            x.copy_(dev(torch, xh))
            spmv_acc_amd.csr_gs_sweep(m, d_rp, d_ci, d_v, color_ptr, color_rows, d_b, x, omega=1.0, direction="symmetric")
        return float(np.linalg.norm(b - A @ x.cpu().numpy()) / np.linalg.norm(b))

    n_a, _, P_a, R_a, Ac_a = level((d_rp, d_ci), False)
    n_b, T_b, P_b, R_b, Ac_b = level((S[0], S[1]), False)
    n_c, T_c, P_c, R_c, Ac_c = level((S[0], S[1]), True)
    assert n_b == n_c == 167 and np.array_equal(T_b, T_c) and np.array_equal(P_b, T_b)
    res_a, res_b, res_c = cycles(P_a, R_a, Ac_a), cycles(P_b, R_b, Ac_b), cycles(P_c, R_c, Ac_c)
    print(f"relative residuals after ten two-level cycles: (a) unfiltered aggregates ({n_a}), tentative P {res_a:.3e}; (b) aggregates of S "
          f"({n_b}), tentative P {res_b:.3e}; (c) aggregates of S, smoothed P {res_c:.3e}")
    assert res_c < res_b < res_a
    # the smoothed P is (I - omega D_F^-1 A_F) T, formed in numpy from the returned diag, A_F and T: within 4 ulp per entry
    A_F = dense(m, m, *host(*S))
    # (every term of an entry is positive here -- couplings are negative, T is positive --, so nothing cancels and an ulp of the entry is the scale)
    want = (np.eye(m) - omega * (A_F / diag.cpu().numpy()[:, None])) @ T_c
    assert np.all(np.abs(P_c - want) <= 4 * 2.0 ** -52 * np.abs(want)) and np.array_equal(P_c != 0.0, want != 0.0)
    assert np.array_equal(R_c, P_c.T) and np.allclose(Ac_c, Ac_c.T, rtol=0, atol=1e-13) and np.allclose(Ac_c, P_c.T @ A @ P_c, rtol=0, atol=1e-13)
    assert hiplib.spmv_acc_last_error() == 0
