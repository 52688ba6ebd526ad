"""GPU suite (-m gpu) of the dense coarse-level solve (spmv_acc_csr_dense_inverse / csr_dense_inverse, spmv_acc_dense_apply / dense_apply): the
inverse bit for bit against the definition restated in numpy (tests/test_dense_host.py host_dense_inverse), the apply bit for bit against
host_dense_apply -- -0.0 and +0.0 count as equal, NaNs by position --, info on singular inputs, the contract of the two entries on the
device, a captured and replayed apply, grid striding, no rows.

No speed gate: the parent commit cannot do this job, so there is no figure to hold (tools/amg_bench.py measures)."""
import ctypes

import numpy as np
import pytest

import spmv_acc_amd
from test_amg_host import hierarchy
from test_dense_host import TAGS, cases, host_dense_apply, host_dense_inverse, inverse, singular_cases

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


def bits(a):
    a = np.ascontiguousarray(a, dtype=np.float64) + 0.0  # a copy
    a[a == 0.0] = 0.0  # -0.0 and +0.0 count as equal
    return a.view(np.uint64)


def same_bits(t, a):
    """the same bits with -0.0 == +0.0, NaNs by position (a NaN's payload and sign are not part of the contract)"""
    got, want = t.cpu().numpy(), np.asarray(a, dtype=np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


def case(tag):
    """(m, (rowptr, colindex, value), inv, info) of the host model; galerkin84: the 84-row second level of grid24's hierarchy."""
    if tag == "galerkin84":
        levels, _ = hierarchy("grid24")
        m, A = levels[1]["m"], levels[1]["A"]
        return (m, A) + host_dense_inverse(m, *A)
    return cases()[tag] + inverse(tag)[:2]


ALL = TAGS + ("galerkin84",)


@pytest.mark.parametrize("tag", ALL)
def test_inverse_is_the_host_model(torch_dev, hiplib, tag):
    torch = torch_dev
    m, (rp, ci, v), want, want_info = case(tag)
    assert want_info == 0 and (tag != "galerkin84" or m == 84)
    d_rp, d_ci, d_v = dev(torch, rp), dev(torch, ci), dev(torch, v)
    plans = hiplib.spmv_acc_cached_plans()
    for _ in range(2):  # twice: the same bits
        inv, info = spmv_acc_amd.csr_dense_inverse(m, d_rp, d_ci, d_v)
        assert inv.shape == (m, m) and inv.dtype == torch.float64 and inv.is_contiguous() and info == 0, (tag, info)
        assert same_bits(inv, want), tag
    assert hiplib.spmv_acc_cached_plans() == plans and hiplib.spmv_acc_last_error() == 0
    # the C entry: nothing beyond m * m doubles is written
    pad = 16
    out = torch.full((m * m + pad,), 7.25, dtype=torch.float64, device="cuda")
    h_info = ctypes.c_int(-5)
    hiplib.spmv_acc_set_stream(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    rc = hiplib.spmv_acc_csr_dense_inverse(m, ci.size, ptr(d_rp), ptr(d_ci), ptr(d_v), ptr(out), ctypes.byref(h_info))
    torch.cuda.synchronize()
    assert rc == 0 and h_info.value == 0, (rc, hiplib.spmv_acc_last_error_string())
    assert same_bits(out[:m * m], want.reshape(-1)) and bool((out[m * m:] == 7.25).all())


@pytest.mark.parametrize("tag", ALL)
def test_apply_is_the_host_model(torch_dev, hiplib, tag):
    """The apply on the host model's inverse, bit for bit, for a normal b and for one with zeros, a -0.0, an inf and a NaN."""
    torch = torch_dev
    m, _, inv, _ = case(tag)
    rng = np.random.default_rng(900 + m)
    d_inv = dev(torch, inv)
    pad = 8
    buf = torch.full((m + 2 * pad,), 7.25, dtype=torch.float64, device="cuda")
    x = buf[pad:pad + m]
    special = rng.standard_normal(m)
    special[rng.integers(0, m, 4)] = [0.0, -0.0, np.inf, np.nan]
    plans = hiplib.spmv_acc_cached_plans()
    for b in (rng.standard_normal(m), special):
        spmv_acc_amd.dense_apply(m, d_inv, dev(torch, b), x)
        assert same_bits(x, host_dense_apply(m, inv, b)), tag
        assert bool((buf[:pad] == 7.25).all()) and bool((buf[pad + m:] == 7.25).all())
    assert hiplib.spmv_acc_cached_plans() == plans and hiplib.spmv_acc_last_error() == 0


def test_dense_grid_stride_at_test_size(torch_dev, hiplib):
    """max_grid_blocks lowered to 64, the smallest cap the library honours: grid18 (m = 324) is 972 tiles of E and 81 workgroups of rows of the
    apply; the same bits as with the default grid, and the host model's."""
    torch = torch_dev
    m, (rp, ci, v), want, _ = case("grid18")
    d_rp, d_ci, d_v = dev(torch, rp), dev(torch, ci), dev(torch, v)
    b = np.random.default_rng(81).standard_normal(m)
    d_b = dev(torch, b)
    assert m * ((2 * m + 255) // 256) > 64 and (m + 3) // 4 > 64

    def run():
        inv, info = spmv_acc_amd.csr_dense_inverse(m, d_rp, d_ci, d_v)
        x = torch.empty(m, dtype=torch.float64, device="cuda")
        spmv_acc_amd.dense_apply(m, inv, d_b, x)
        torch.cuda.synchronize()
        return inv, info, x

    default = run()
    try:
        assert hiplib.spmv_acc_set_tunable(b"max_grid_blocks", 64) == 0
        strided = run()
    finally:
        hiplib.spmv_acc_reset_tunables()
    for inv, info, x in (default, strided):
        assert info == 0 and same_bits(inv, want) and same_bits(x, host_dense_apply(m, inv.cpu().numpy(), b))
    assert hiplib.spmv_acc_last_error() == 0


def test_singular_inputs_give_info(torch_dev, hiplib):
    """A structurally zero column, a NaN entry, an empty row, no entries: info names the step the host model names (the contents are unspecified)."""
    torch = torch_dev
    for tag, (m, (rp, ci, v)) in singular_cases().items():
        want = host_dense_inverse(m, rp, ci, v)[1]
        inv, info = spmv_acc_amd.csr_dense_inverse(m, dev(torch, rp), dev(torch, ci), dev(torch, v))
        assert info == want and info != 0 and inv.shape == (m, m), (tag, info, want)
    assert hiplib.spmv_acc_last_error() == 0


def test_no_rows(torch_dev, hiplib):
    torch = torch_dev
    empty_i, empty_f = torch.zeros(0, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.float64, device="cuda")
    inv, info = spmv_acc_amd.csr_dense_inverse(0, torch.zeros(1, dtype=torch.int32, device="cuda"), empty_i, empty_f)
    assert inv.shape == (0, 0) and info == 0
    spmv_acc_amd.dense_apply(0, inv, empty_f, torch.zeros(0, dtype=torch.float64, device="cuda"))
    h_info = ctypes.c_int(-5)
    assert hiplib.spmv_acc_csr_dense_inverse(0, 0, None, None, None, None, ctypes.byref(h_info)) == 0 and h_info.value == 0
    assert hiplib.spmv_acc_dense_apply(0, None, None, None) == 0 and hiplib.spmv_acc_last_error() == 0


def test_apply_captured_and_replayed(torch_dev, hiplib):
    """The apply captured once (one launch) and replayed after b and the inverse were edited in place."""
    torch = torch_dev
    m, _, inv, _ = case("r130")
    d_inv, d_b = dev(torch, inv), torch.zeros(m, dtype=torch.float64, device="cuda")
    x = torch.full((m,), -3.0, dtype=torch.float64, device="cuda")
    spmv_acc_amd.dense_apply(m, d_inv, d_b, x)  # (warm: the code object is loaded outside the capture)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            spmv_acc_amd.dense_apply(m, d_inv, d_b, x)
    assert hiplib.spmv_acc_last_error() == 0
    rng = np.random.default_rng(7)
    for scale in (1.0, -0.5):
        b = rng.standard_normal(m)
        d_b.copy_(dev(torch, b))
        d_inv.copy_(dev(torch, inv * scale))
        x.fill_(-3.0)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(x, host_dense_apply(m, inv * scale, b)), scale
    del g


def test_inverse_contract(torch_dev, hiplib):
    """Each defect of the input: SPMV_ACC_ERR_BAD_ARGUMENT with its count in the error string, inv and h_info untouched; an unsymmetric pattern
    is taken; more than 4096 rows and a capture are refused."""
    torch = torch_dev
    m, (rp, ci, v), want, _ = case("grid18")
    nnz = ci.size
    pad = 64
    d_rp = dev(torch, rp)
    out = torch.full((m * m + pad,), 7.25, dtype=torch.float64, device="cuda")
    h_info = ctypes.c_int(-5)
    plans = hiplib.spmv_acc_cached_plans()

    def padded(a):  # (a wrong nnz never reaches past the array: the census reads clamped extents, and the array has room beyond them anyway)
        return dev(torch, np.concatenate([a, np.zeros(pad, a.dtype)]))

    d_v = padded(v)

    def call(rowptr=d_rp, colindex=None, mm=m, nz=nnz):
        colindex = padded(ci) if colindex is None else colindex
        rc = hiplib.spmv_acc_csr_dense_inverse(mm, nz, ptr(rowptr), ptr(colindex), ptr(d_v), ptr(out), ctypes.byref(h_info))
        msg = hiplib.spmv_acc_last_error_string().decode()
        code = hiplib.spmv_acc_last_error()
        hiplib.spmv_acc_clear_error()
        return rc, code, msg

    def untouched():
        torch.cuda.synchronize()
        return bool((out == 7.25).all()) and h_info.value == -5

    def refused(result, *needles):
        rc, code, msg = result
        assert rc == 2 and code == 2 and "spmv_acc_csr_dense_inverse:" in msg and "nothing was written" in msg and all(s in msg for s in needles), (rc, msg)
        assert untouched(), msg

    hiplib.spmv_acc_set_stream(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
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
    bad[0] = 1
    refused(call(rowptr=dev(torch, bad)), "1 ends of rowptr")
    bad = rp.copy()
    bad[50] = rp[51] + 1
    refused(call(rowptr=dev(torch, bad)), "1 rows with a descending or out-of-range rowptr extent")
    for nz in (nnz - 1, nnz + 1):
        refused(call(nz=nz), "1 ends of rowptr")
    # host-side refusals leave the device alone as well
    big = 2 ** 31 - 2 ** 16
    rc, code, msg = call(mm=4097)
    assert rc == 4 and "at most 4096" in msg and call(nz=big)[0] == 4 and call(mm=-1)[0] == 2 and untouched()
    with pytest.raises(spmv_acc_amd.SpmvAccError, match="at most 4096"):
        spmv_acc_amd.csr_dense_inverse(4097, torch.zeros(4098, dtype=torch.int32, device="cuda"), dev(torch, ci), dev(torch, v))
    with pytest.raises(spmv_acc_amd.SpmvAccError, match="1 columns outside"):
        bad = ci.copy()
        bad[rp[300] + 2] = m
        spmv_acc_amd.csr_dense_inverse(m, d_rp, dev(torch, bad), dev(torch, v))
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
            rc = hiplib.spmv_acc_csr_dense_inverse(m, nnz, ptr(d_rp), ptr(d_ci), ptr(d_v), ptr(out), ctypes.byref(h_info))
            msg = hiplib.spmv_acc_last_error_string().decode()
            hiplib.spmv_acc_clear_error()
    assert rc == 2 and "capture" in msg, (rc, msg)
    g.replay()
    torch.cuda.synchronize()
    assert untouched() and float(filler[0]) == 1.0
    del g
    hiplib.spmv_acc_set_stream(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    # an unsymmetric pattern is no defect: the entry (i, j) without its mirror
    keep = np.ones(nnz, dtype=bool)
    keep[int(rp[200 + 1]) - 1] = False  # the last entry of row 200 goes, its mirror stays
    u_rp = np.concatenate([[0], np.cumsum(np.bincount(np.repeat(np.arange(m), np.diff(rp))[keep], minlength=m))]).astype(np.int32)
    u_inv, u_info = spmv_acc_amd.csr_dense_inverse(m, dev(torch, u_rp), dev(torch, ci[keep]), dev(torch, v[keep]))
    w_inv, w_info = host_dense_inverse(m, u_rp, ci[keep], v[keep])
    assert u_info == w_info == 0 and same_bits(u_inv, w_inv)
    # and the clean input still passes, on the same arrays
    rc, code, msg = call()
    torch.cuda.synchronize()
    assert rc == 0 and h_info.value == 0 and same_bits(out[:m * m], want.reshape(-1)) and bool((out[m * m:] == 7.25).all()), (rc, msg)
    assert hiplib.spmv_acc_cached_plans() == plans


def test_apply_contract(torch_dev, hiplib):
    """Overlaps, bad sizes and null pointers are refused before any launch: x is untouched."""
    torch = torch_dev
    m, _, inv, _ = case("r65")
    store = torch.zeros(m * m + 2 * m, dtype=torch.float64, device="cuda")  # (m spare doubles on either side: a vector that starts on inv's last element ends here)
    d_inv = store[m:m + m * m]
    d_inv.copy_(dev(torch, inv).reshape(-1))
    room = torch.full((4 * m,), -3.0, dtype=torch.float64, device="cuda")
    d_b, x = room[:m], room[2 * m:3 * m]
    hiplib.spmv_acc_set_stream(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    def call(mm=m, ii=d_inv, bb=d_b, xx=x):
        rc = hiplib.spmv_acc_dense_apply(mm, ptr(ii), ptr(bb), ptr(xx))
        msg = hiplib.spmv_acc_last_error_string().decode()
        hiplib.spmv_acc_clear_error()
        return rc, msg

    assert call(bb=room[2 * m + 5:])[0] == 2 and "b overlaps x" in call(bb=room[2 * m - 1:])[1] and "b overlaps x" in call(xx=room[m - 1:])[1]
    flat = d_inv.reshape(-1)
    assert "overlaps inv" in call(xx=flat[m * m - 1:])[1] and "overlaps inv" in call(bb=flat[3:])[1] and "overlaps inv" in call(xx=flat)[1]
    assert call(mm=-1)[0] == 2 and call(ii=None)[0] == 2 and call(bb=None)[0] == 2 and call(xx=None)[0] == 2
    big = 2 ** 31 - 2 ** 16
    assert call(mm=big)[0] == 4 and call(mm=2 ** 31 - 1)[0] == 4
    torch.cuda.synchronize()
    assert bool((room == -3.0).all())
    with pytest.raises(spmv_acc_amd.SpmvAccError, match="overlaps"):
        spmv_acc_amd.dense_apply(m, d_inv, room[:m], room[m - 1:2 * m - 1])
    assert hiplib.spmv_acc_last_error() == 0
    # adjacent arrays do not overlap: b directly before x
    b = np.random.default_rng(65).standard_normal(m)
    room[m:2 * m].copy_(dev(torch, b))
    spmv_acc_amd.dense_apply(m, d_inv, room[m:2 * m], x)
    assert same_bits(x, host_dense_apply(m, inv, b)) and bool((room[:m] == -3.0).all()) and bool((room[3 * m:] == -3.0).all())
