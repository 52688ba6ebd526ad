"""GPU suite (-m gpu) of the multicolour Gauss-Seidel / SOR smoother (spmv_acc_csr_color / csr_color, spmv_acc_csr_gs_sweep / csr_gs_sweep):
the colouring exactly against the definition restated in numpy (tests/test_gs_host.py host_csr_color), the sweep bit for bit against its
summation order restated there (host_gs_sweep) in both forms -- through color_rows on the original matrix and on the colour-permuted matrix
-- forward, backward and symmetric, plain and relaxed; that it smooths an SPD system; a captured and replayed sweep; non-finite, subnormal and
zero-diagonal inputs; the contract of the two entries on the device; and grid striding.

No speed gate: the parent commit cannot do this job, so there is no figure to hold (tools/gs_bench.py measures)."""
import ctypes
import functools

import numpy as np
import pytest

import spmv_acc_amd
from spmv_acc_amd import synth
from special_values import BIG_VALUE, BIG_X, POISON, TINY
from test_extract_host import host_csr_permute
from test_gs_host import CHUNK_ROWS, TAGS, cases, coloring, host_csr_color, host_gs_sweep, is_proper

pytestmark = pytest.mark.gpu

DIRECTIONS = ("forward", "backward", "symmetric")
OMEGAS = (1.0, 0.8, 1.5)


@pytest.fixture(scope="module")
def torch_dev(hiplib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_csr(torch, csr):
    return tuple(dev(torch, a) for a in csr)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def same(t, a):
    return np.array_equal(t.cpu().numpy(), a)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(t, a):
    """the same bits, NaNs by position (a NaN's payload and sign are not part of the contract: the division and the adds may quiet or keep them)"""
    got, want = t.cpu().numpy(), np.asarray(a, dtype=np.float64)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


@functools.lru_cache(maxsize=None)
def vectors(tag):
    m = cases()[tag][0]
    rng = np.random.default_rng(100 + m)
    return rng.standard_normal(m), rng.standard_normal(m)


@functools.lru_cache(maxsize=None)
def permuted(tag):
    """the colour-permuted matrix of a case on the host: (rowptr, colindex, value)"""
    m, A = cases()[tag]
    rp, ci, _, v = host_csr_permute(m, A, coloring(tag)[1])
    return rp, ci, v


@pytest.mark.parametrize("tag", TAGS)
def test_color_is_the_host_model(torch_dev, hiplib, tag):
    torch = torch_dev
    m, (rp, ci, v) = cases()[tag]
    w_color, w_rows, w_ptr, w_no_diag = coloring(tag)
    if tag == "fem":  # assembled on the device, as a user would: the same pattern
        row, col, val = synth.fem_quads_coo(24, 17, seed=5)
        d_rp, d_ci, _ = spmv_acc_amd.coo_to_csr(m, m, dev(torch, row), dev(torch, col), dev(torch, val))
        assert same(d_rp, rp) and same(d_ci, ci)
    else:
        d_rp, d_ci = dev(torch, rp), dev(torch, ci)
    plans = hiplib.spmv_acc_cached_plans()
    for _ in range(2):  # twice: the same arrays
        color, color_rows, color_ptr, no_diag = spmv_acc_amd.csr_color(m, d_rp, d_ci)
        assert color.numel() == color_rows.numel() == m and color.dtype == color_rows.dtype == torch.int32
        assert same(color, w_color) and same(color_rows, w_rows) and color_ptr == w_ptr and no_diag == w_no_diag, tag
    assert is_proper(m, rp, ci, color.cpu().numpy())
    assert hiplib.spmv_acc_cached_plans() == plans and hiplib.spmv_acc_last_error() == 0
    # the C entry with an array of exactly ncolors: the outputs are exact-size, nothing beyond them is written
    ncolors = len(w_ptr) - 1
    pad = 16
    o_color = torch.full((m + pad,), -7, dtype=torch.int32, device="cuda")
    o_rows = torch.full((m + pad,), -7, dtype=torch.int32, device="cuda")
    h_ptr = (ctypes.c_int * (max(ncolors, 1) + 1 + pad))(*([-7] * (max(ncolors, 1) + 1 + pad)))
    h_n, h_d = ctypes.c_int(-5), ctypes.c_int(-5)
    hiplib.spmv_acc_set_stream(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    rc = hiplib.spmv_acc_csr_color(m, ci.size, ptr(d_rp), ptr(d_ci) if ci.size else None, ptr(o_color), ptr(o_rows), max(ncolors, 1), h_ptr,
                                   ctypes.byref(h_n), ctypes.byref(h_d))
    torch.cuda.synchronize()
    assert rc == 0 and h_n.value == ncolors and h_d.value == w_no_diag, (rc, hiplib.spmv_acc_last_error_string())
    assert list(h_ptr)[:ncolors + 1] == w_ptr and set(list(h_ptr)[ncolors + 1:]) == {-7}
    assert same(o_color[:m], w_color) and same(o_rows[:m], w_rows) and bool((o_color[m:] == -7).all()) and bool((o_rows[m:] == -7).all())


def test_color_cap_too_small(torch_dev, hiplib):
    """K_130 with room for 64 colours: SPMV_ACC_ERR_TOO_LARGE, the count and the colours are valid, the caller comes back with a larger array."""
    torch = torch_dev
    m, (rp, ci, v) = cases()["k130"]
    w_color, w_rows, w_ptr, _ = coloring("k130")
    d_rp, d_ci = dev(torch, rp), dev(torch, ci)
    color = torch.full((m,), -7, dtype=torch.int32, device="cuda")
    rows = torch.full((m,), -7, dtype=torch.int32, device="cuda")
    h_ptr = (ctypes.c_int * 65)(*([-7] * 65))
    h_n, h_d = ctypes.c_int(-5), ctypes.c_int(-5)
    hiplib.spmv_acc_set_stream(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    rc = hiplib.spmv_acc_csr_color(m, ci.size, ptr(d_rp), ptr(d_ci), ptr(color), ptr(rows), 64, h_ptr, ctypes.byref(h_n), ctypes.byref(h_d))
    msg = hiplib.spmv_acc_last_error_string().decode()
    assert rc == 4 and hiplib.spmv_acc_last_error() == 4 and "130 colours" in msg, (rc, msg)
    hiplib.spmv_acc_clear_error()
    assert h_n.value == 130 and same(color, w_color) and set(h_ptr) == {-7}
    h_big = (ctypes.c_int * (h_n.value + 1))()
    rc = hiplib.spmv_acc_csr_color(m, ci.size, ptr(d_rp), ptr(d_ci), ptr(color), ptr(rows), h_n.value, h_big, ctypes.byref(h_n), ctypes.byref(h_d))
    assert rc == 0 and list(h_big) == w_ptr and same(rows, w_rows)
    # the wrapper does the same from its first array
    old = spmv_acc_amd._GS_FIRST_CAP
    try:
        spmv_acc_amd._GS_FIRST_CAP = 64
        got = spmv_acc_amd.csr_color(m, d_rp, d_ci)
    finally:
        spmv_acc_amd._GS_FIRST_CAP = old
    assert same(got[0], w_color) and same(got[1], w_rows) and got[2] == w_ptr and got[3] == 0 and hiplib.spmv_acc_last_error() == 0


@pytest.mark.parametrize("tag", TAGS)
def test_sweep_is_the_host_model(torch_dev, hiplib, tag):
    """Both forms, each against its own model: color_rows on the original matrix, and NULL on the csr_permute-d matrix with b and x permuted."""
    torch = torch_dev
    m, (rp, ci, v) = cases()[tag]
    _, w_rows, w_ptr, _ = coloring(tag)
    b, x0 = vectors(tag)
    d_A = dev_csr(torch, (rp, ci, v))
    d_rows = dev(torch, w_rows)
    if m:
        p_A = spmv_acc_amd.csr_permute(m, *d_A, d_rows)
        w_p = permuted(tag)
        assert same(p_A[0], w_p[0]) and same(p_A[1], w_p[1]) and same_bits(p_A[2], w_p[2])
    else:
        p_A, w_p = d_A, (rp, ci, v)
    pb, px0 = b[w_rows], x0[w_rows]
    d_b, d_pb = dev(torch, b), dev(torch, pb)
    plans = hiplib.spmv_acc_cached_plans()
    for direction in DIRECTIONS:
        for omega in OMEGAS:
            want = host_gs_sweep(m, rp, ci, v, w_ptr, w_rows, b, x0, omega, direction)
            want_p = host_gs_sweep(m, *w_p, w_ptr, None, pb, px0, omega, direction)
            for _ in range(2):  # twice: the same bits
                x = dev(torch, x0)
                spmv_acc_amd.csr_gs_sweep(m, *d_A, w_ptr, d_rows, d_b, x, omega=omega, direction=direction)
                assert same_bits(x, want), (tag, direction, omega)
                px = dev(torch, px0)
                spmv_acc_amd.csr_gs_sweep(m, *p_A, w_ptr, None, d_pb, px, omega=omega, direction=direction)
                assert same_bits(px, want_p), (tag, direction, omega, "permuted")
    # two sweeps in one call are two calls
    want = host_gs_sweep(m, rp, ci, v, w_ptr, w_rows, b, host_gs_sweep(m, rp, ci, v, w_ptr, w_rows, b, x0, 1.5, "symmetric"), 1.5, "symmetric")
    x = dev(torch, x0)
    spmv_acc_amd.csr_gs_sweep(m, *d_A, w_ptr, d_rows, d_b, x, omega=1.5, sweeps=2)
    assert same_bits(x, want), tag
    assert hiplib.spmv_acc_cached_plans() == plans and hiplib.spmv_acc_last_error() == 0


def energy_norm(rp, ci, v, e):
    """sqrt(e^T A e) in extended precision"""
    row = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    e = e.astype(np.longdouble)
    return float(np.sqrt(np.sum(e[row] * v.astype(np.longdouble) * e[ci])))


def test_it_smooths(torch_dev, hiplib):
    """The SPD 7-point matrix (symmetric, strictly diagonally dominant, positive diagonal) with b = A x*: over five symmetric sweeps the energy
    norm of the error strictly decreases for omega = 1 and 1.5 -- the theorem for SPD A and 0 < omega < 2.  The engine's SpMV on the same arrays
    gives the residual the host computes."""
    torch = torch_dev
    m, (rp, ci, v) = cases()["grid7"]
    row = np.repeat(np.arange(m), np.diff(rp))
    D = np.zeros((m, m))
    D[row, ci] = v
    assert np.array_equal(D, D.T) and np.all(np.diag(D) > np.abs(D).sum(axis=1) - np.diag(D))  # SPD by Gershgorin
    _, w_rows, w_ptr, _ = coloring("grid7")
    rng = np.random.default_rng(17)
    star = rng.standard_normal(m)
    b = np.asarray((D.astype(np.longdouble) @ star.astype(np.longdouble)).astype(np.float64))
    d_A = dev_csr(torch, (rp, ci, v))
    d_rows, d_b = dev(torch, w_rows), dev(torch, b)
    for omega in (1.0, 1.5):
        x = torch.zeros(m, dtype=torch.float64, device="cuda")
        norms = [energy_norm(rp, ci, v, -star)]
        model = np.zeros(m)
        for _ in range(5):
            spmv_acc_amd.csr_gs_sweep(m, *d_A, w_ptr, d_rows, d_b, x, omega=omega, direction="symmetric")
            model = host_gs_sweep(m, rp, ci, v, w_ptr, w_rows, b, model, omega, "symmetric")
            assert same_bits(x, model), omega
            norms.append(energy_norm(rp, ci, v, x.cpu().numpy() - star))
        print(f"omega {omega}: energy norms of the error {['%.6e' % n for n in norms]}")
        assert all(later < earlier for earlier, later in zip(norms, norms[1:])), (omega, norms)
        # the residual b - A x through the engine (y = -1 * A x + 1 * b) against the host's
        r = d_b.clone()
        spmv_acc_amd.sparse_spmv(0, -1.0, 1.0, m, m, *d_A, x, r)
        torch.cuda.synchronize()
        xh = x.cpu().numpy()
        host_r = np.asarray((b.astype(np.longdouble) - D.astype(np.longdouble) @ xh.astype(np.longdouble)).astype(np.float64))
        scale = np.abs(b) + np.abs(D) @ np.abs(xh)
        assert np.all(np.abs(r.cpu().numpy() - host_r) <= 1e-12 * scale), omega  # the project's gate (rows of 7 terms sit orders below it)
    spmv_acc_amd.release_plans(d_A[0])


def test_captured_and_replayed(torch_dev, hiplib):
    """A symmetric sweep captured in one graph (one stream, no parallel branches) and replayed after value and b were edited in place; inside
    the capture csr_color refuses with "capture" and the capture survives."""
    torch = torch_dev
    m, (rp, ci, v) = cases()["grid27"]
    _, w_rows, w_ptr, _ = coloring("grid27")
    b, x0 = vectors("grid27")
    d_rp, d_ci, d_v = dev_csr(torch, (rp, ci, v))
    d_rows, d_b, x = dev(torch, w_rows), dev(torch, b), dev(torch, x0)
    spmv_acc_amd.csr_gs_sweep(m, d_rp, d_ci, d_v, w_ptr, d_rows, d_b, x, omega=0.8)  # (warm: the code object is loaded outside the capture)
    o_color = torch.full((m,), -7, dtype=torch.int32, device="cuda")
    o_rows = torch.full((m,), -7, dtype=torch.int32, device="cuda")
    h_ptr = (ctypes.c_int * 1025)(*([-7] * 1025))
    h_n, h_d = ctypes.c_int(-5), ctypes.c_int(-5)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            spmv_acc_amd.csr_gs_sweep(m, d_rp, d_ci, d_v, w_ptr, d_rows, d_b, x, omega=0.8)
            hiplib.spmv_acc_set_stream(ctypes.c_void_p(s.cuda_stream))
            rc = hiplib.spmv_acc_csr_color(m, ci.size, ptr(d_rp), ptr(d_ci), ptr(o_color), ptr(o_rows), 1024, h_ptr, ctypes.byref(h_n), ctypes.byref(h_d))
            msg = hiplib.spmv_acc_last_error_string().decode()
            hiplib.spmv_acc_clear_error()
    assert rc == 2 and "capture" in msg, (rc, msg)
    rng = np.random.default_rng(5)
    for _ in range(2):
        new_v, new_b = v * rng.uniform(0.5, 1.5, v.size), rng.standard_normal(m)
        d_v.copy_(dev(torch, new_v))
        d_b.copy_(dev(torch, new_b))
        x.copy_(dev(torch, x0))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(x, host_gs_sweep(m, rp, ci, new_v, w_ptr, w_rows, new_b, x0, 0.8, "symmetric"))
    assert bool((o_color == -7).all()) and bool((o_rows == -7).all()) and set(h_ptr) == {-7} and h_n.value == -5 and h_d.value == -5
    del g


def test_special_values(torch_dev):
    """NaN, +-Inf, overflowing products and subnormals in value, b and x, and a zero diagonal of either sign, come out as the host model says."""
    torch = torch_dev
    rng = np.random.default_rng(23)
    for tag in ("fem", "grid27", "star"):
        m, (rp, ci, v) = cases()[tag]
        _, w_rows, w_ptr, _ = coloring(tag)
        row = np.repeat(np.arange(m), np.diff(rp))
        b, x0 = (a.copy() for a in vectors(tag))
        v = v.copy()
        diag = np.flatnonzero(ci == row)
        off = np.flatnonzero(ci != row)
        specials = list(POISON) + [TINY, -TINY, 2.0 ** -1030, 0.0, -0.0]
        for k, s in enumerate(specials):
            v[off[(7 * k + 3) % off.size]] = s
            b[(11 * k + 1) % m] = s
            x0[(13 * k + 2) % m] = s
        v[off[5 % off.size]], x0[ci[off[5 % off.size]]] = BIG_VALUE, BIG_X  # a product that overflows
        v[diag[3]], v[diag[9]], v[diag[20]], v[diag[21]] = 0.0, -0.0, TINY, np.inf  # zero diagonals of either sign, a subnormal and an infinite one
        d_A = dev_csr(torch, (rp, ci, v))
        d_rows, d_b = dev(torch, w_rows), dev(torch, b)
        seen = np.zeros(m, dtype=bool)
        for direction, omega in (("forward", 1.0), ("symmetric", 0.8), ("backward", 1.5)):
            want = host_gs_sweep(m, rp, ci, v, w_ptr, w_rows, b, x0, omega, direction)
            x = dev(torch, x0)
            spmv_acc_amd.csr_gs_sweep(m, *d_A, w_ptr, d_rows, d_b, x, omega=omega, direction=direction)
            assert same_bits(x, want), (tag, direction, omega)
            seen |= ~np.isfinite(want)
        assert seen.any() and (tag == "star" or not seen.all()), tag  # the poison arrived and, but through the star's hub, did not take every row


def test_color_contract(torch_dev, hiplib):
    """Each defect of the input: SPMV_ACC_ERR_BAD_ARGUMENT with its count in the error string, outputs untouched."""
    torch = torch_dev
    m, (rp, ci, v) = cases()["grid27"]
    nnz = ci.size
    row = np.repeat(np.arange(m), np.diff(rp))
    pad = 64
    d_rp = dev(torch, rp)
    o_color = torch.full((m + pad,), -7, dtype=torch.int32, device="cuda")
    o_rows = torch.full((m + pad,), -7, dtype=torch.int32, device="cuda")
    h_ptr = (ctypes.c_int * 1025)(*([-7] * 1025))
    h_n, h_d = ctypes.c_int(-5), ctypes.c_int(-5)
    plans = hiplib.spmv_acc_cached_plans()

    def padded(a):  # (a wrong nnz never reaches past the array: the census reads clamped extents, and the array has room beyond them anyway)
        return dev(torch, np.concatenate([a, np.zeros(pad, a.dtype)]))

    def call(rowptr=d_rp, colindex=None, mm=m, nz=nnz, cap=1024):
        colindex = padded(ci) if colindex is None else colindex
        rc = hiplib.spmv_acc_csr_color(mm, nz, ptr(rowptr), ptr(colindex), ptr(o_color), ptr(o_rows), cap, h_ptr, ctypes.byref(h_n), ctypes.byref(h_d))
        msg = hiplib.spmv_acc_last_error_string().decode()
        code = hiplib.spmv_acc_last_error()
        hiplib.spmv_acc_clear_error()
        return rc, code, msg

    def untouched():
        torch.cuda.synchronize()
        return bool((o_color == -7).all()) and bool((o_rows == -7).all()) and set(h_ptr) == {-7} and h_n.value == -5 and h_d.value == -5

    clean = ("0 ends of rowptr that are not 0 and nnz, 0 rows with a descending or out-of-range rowptr extent, 0 columns outside [0, m), "
             "0 positions where a row does not strictly ascend, 0 off-diagonal entries without their mirror")

    def refused(result, *needles):
        rc, code, msg = result
        assert rc == 2 and code == 2 and "spmv_acc_csr_color:" in msg and "nothing was written" in msg and all(s in msg for s in needles), (rc, msg)
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
    # a descending row (two neighbours swapped: two positions that do not ascend would be one; the swap makes one descent)
    bad = ci.copy()
    q = int(rp[100]) + 1
    bad[q], bad[q + 1] = ci[q + 1], ci[q]
    refused(call(colindex=padded(bad)), "1 positions where a row does not strictly ascend")
    # a repeated column
    bad = ci.copy()
    bad[q + 1] = ci[q]
    rc, code, msg = call(colindex=padded(bad))
    refused((rc, code, msg), "1 positions where a row does not strictly ascend")
    # a column >= m, and a negative one
    for value in (m, 2 ** 31 - 1, -1):
        bad = ci.copy()
        bad[rp[300] + 2] = value
        rc, code, msg = call(colindex=padded(bad))
        refused((rc, code, msg), "1 columns outside [0, m)")
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
    assert call(mm=big)[0] == 4 and call(nz=big)[0] == 4 and call(cap=0)[0] == 2 and call(mm=-1)[0] == 2 and untouched()
    # the wrapper raises with the counts
    with pytest.raises(spmv_acc_amd.SpmvAccError, match="1 columns outside"):
        bad = ci.copy()
        bad[rp[300] + 2] = m
        spmv_acc_amd.csr_color(m, d_rp, dev(torch, bad))
    torch.cuda.synchronize()  # (no device-side fault: the context is alive)
    # and the clean input still passes, on the same arrays
    rc, code, msg = call()
    w_color, w_rows, w_ptr, _ = coloring("grid27")
    assert rc == 0 and h_n.value == len(w_ptr) - 1 and h_d.value == 0 and same(o_color[:m], w_color) and same(o_rows[:m], w_rows), (rc, msg)
    assert list(h_ptr)[:len(w_ptr)] == w_ptr and hiplib.spmv_acc_cached_plans() == plans


def test_sweep_contract(torch_dev, hiplib):
    """Crafted color_rows and colindex do not fault and change only valid rows; a bad h_color_ptr is refused; nothing outside x is written."""
    torch = torch_dev
    m, (rp, ci, v) = cases()["fem"]
    nnz = ci.size
    _, w_rows, w_ptr, _ = coloring("fem")
    b, x0 = vectors("fem")
    d_A = dev_csr(torch, (rp, ci, v))
    d_b = dev(torch, b)
    pad = 64
    buf = torch.full((m + 2 * pad,), 7.25, dtype=torch.float64, device="cuda")
    x = buf[pad:pad + m]
    rng = np.random.default_rng(41)
    # color_rows with entries outside [0, m): those positions are skipped, every other row gets the model's value
    crafted = w_rows.copy()
    out = rng.choice(m, 30, replace=False)
    crafted[out] = np.array([-1, m, m + 7, 2 ** 31 - 1, -2 ** 31, -m] * 5, dtype=np.int64).astype(np.int32)
    x.copy_(dev(torch, x0))
    spmv_acc_amd.csr_gs_sweep(m, *d_A, w_ptr, dev(torch, crafted), d_b, x, omega=1.5, direction="symmetric")
    torch.cuda.synchronize()
    want = host_gs_sweep(m, rp, ci, v, w_ptr, crafted, b, x0, 1.5, "symmetric")
    skipped = w_rows[out]
    assert same_bits(x, want) and np.array_equal(bits(want[skipped]), bits(x0[skipped])) and bool((buf[:pad] == 7.25).all()) and bool((buf[pad + m:] == 7.25).all())
    assert np.sum(bits(want) != bits(x0)) >= m - 30 - 5
    # colindex with entries outside [0, m): they contribute +0.0
    bad_ci = ci.copy()
    row = np.repeat(np.arange(m), np.diff(rp))
    off = np.flatnonzero(ci != row)
    hit = rng.choice(off, 40, replace=False)
    bad_ci[hit] = np.array([-1, m, m + 9, 2 ** 31 - 1, -2 ** 31] * 8, dtype=np.int64).astype(np.int32)
    x.copy_(dev(torch, x0))
    spmv_acc_amd.csr_gs_sweep(m, d_A[0], dev(torch, bad_ci), d_A[2], w_ptr, dev(torch, w_rows), d_b, x, omega=1.0, direction="forward")
    torch.cuda.synchronize()
    want = host_gs_sweep(m, rp, bad_ci, v, w_ptr, w_rows, b, x0, 1.0, "forward")
    assert same_bits(x, want) and np.all(np.isfinite(want)) and bool((buf[:pad] == 7.25).all()) and bool((buf[pad + m:] == 7.25).all())
    # a rowptr that leaves the arrays is clamped
    bad_rp = rp.copy()
    bad_rp[7], bad_rp[200] = -5, nnz + 1000
    x.copy_(dev(torch, x0))
    spmv_acc_amd.csr_gs_sweep(m, dev(torch, bad_rp), d_A[1], d_A[2], w_ptr, dev(torch, w_rows), d_b, x, omega=1.0, direction="forward")
    torch.cuda.synchronize()
    assert bool((buf[:pad] == 7.25).all()) and bool((buf[pad + m:] == 7.25).all())
    # a bad h_color_ptr, a bad direction, b overlapping x: refused on the host, nothing launched
    x.copy_(dev(torch, x0))
    hiplib.spmv_acc_set_stream(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    def call(hp=w_ptr, direction=2, bb=d_b, mm=m):
        h = (ctypes.c_int * len(hp))(*hp)
        rc = hiplib.spmv_acc_csr_gs_sweep(mm, nnz, ptr(d_A[0]), ptr(d_A[1]), ptr(d_A[2]), len(hp) - 1, h, None, 1.0, direction, ptr(bb), ptr(x))
        msg = hiplib.spmv_acc_last_error_string().decode()
        hiplib.spmv_acc_clear_error()
        return rc, msg

    for hp in ([1] + w_ptr[1:], w_ptr[:-1] + [m + 1], w_ptr[:-1] + [m - 1], [0, 300, 200, m], w_ptr[:-1]):
        rc, msg = call(hp=hp)
        assert rc == 2 and "h_color_ptr" in msg, (hp[:3], rc, msg)
    assert call(direction=3)[0] == 2 and "overlaps" in call(bb=x)[1] and call(bb=buf[pad + m - 1:])[0] == 2
    assert call(mm=2 ** 29 + 1, hp=[0, 2 ** 29 + 1])[0] == 4
    torch.cuda.synchronize()
    assert same_bits(x, x0)
    with pytest.raises(spmv_acc_amd.SpmvAccError, match="color_ptr"):
        spmv_acc_amd.csr_gs_sweep(m, *d_A, w_ptr[:-1], None, d_b, x)
    assert hiplib.spmv_acc_last_error() == 0


def test_gs_grid_stride_at_test_size(torch_dev, hiplib):
    """max_grid_blocks lowered to 64, the smallest cap the library honours (64 workgroups = 4 096 rows of a sweep launch): the 7-point stencil
    on 44 x 44 x 44 (85 184 rows: 333 workgroups of rows in the census and the rounds; its largest colours hold several times as many rows, so their
    launches stride) gives the same colours and the same bits as with the default grid."""
    torch = torch_dev
    rng = np.random.default_rng(77)
    n = 44
    idx = np.arange(n ** 3, dtype=np.int64).reshape(n, n, n)
    pairs_i, pairs_j = [idx.reshape(-1)], [idx.reshape(-1)]
    for axis in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, n - 1), slice(1, n)
        a, c = idx[tuple(lo)].reshape(-1), idx[tuple(hi)].reshape(-1)
        pairs_i += [a, c]
        pairs_j += [c, a]
    i, j = np.concatenate(pairs_i), np.concatenate(pairs_j)
    order = np.lexsort((j, i))
    i, j = i[order], j[order]
    m = n ** 3
    rp = np.zeros(m + 1, dtype=np.int32)
    np.cumsum(np.bincount(i, minlength=m), out=rp[1:])
    ci, v = j.astype(np.int32), rng.uniform(0.5, 2.0, j.size)
    b, x0 = rng.standard_normal(m), rng.standard_normal(m)
    d_A = dev_csr(torch, (rp, ci, v))
    d_b = dev(torch, b)
    assert m + 1 > 64 * 256

    def run():
        color, rows, color_ptr, no_diag = spmv_acc_amd.csr_color(m, d_A[0], d_A[1])
        x = dev(torch, x0)
        spmv_acc_amd.csr_gs_sweep(m, *d_A, color_ptr, rows, d_b, x, omega=1.5, direction="symmetric")
        p_A = spmv_acc_amd.csr_permute(m, *d_A, rows)
        px = x0[rows.cpu().numpy()]
        d_px = dev(torch, px)
        spmv_acc_amd.csr_gs_sweep(m, *p_A, color_ptr, None, dev(torch, b[rows.cpu().numpy()]), d_px, omega=1.5, direction="symmetric")
        torch.cuda.synchronize()
        return color.cpu().numpy(), rows.cpu().numpy(), color_ptr, no_diag, x.cpu().numpy(), d_px.cpu().numpy()

    default = run()
    try:
        assert hiplib.spmv_acc_set_tunable(b"max_grid_blocks", 64) == 0
        strided = run()
    finally:
        hiplib.spmv_acc_reset_tunables()
    color, rows, color_ptr, no_diag, x, px = default
    assert max(np.diff(color_ptr)) > 64 * 4 * CHUNK_ROWS and no_diag == 0 and is_proper(m, rp, ci, color)  # the largest colour strides in the sweep
    assert np.array_equal(color, strided[0]) and np.array_equal(rows, strided[1]) and color_ptr == strided[2]
    assert np.array_equal(bits(x), bits(strided[4])) and np.array_equal(bits(px), bits(strided[5]))
    # the colouring is the definition's (the sequential model on 85 184 rows takes a second or two)
    w_color, w_rows, w_ptr, _ = host_csr_color(m, rp, ci)
    assert np.array_equal(color, w_color) and np.array_equal(rows, w_rows) and color_ptr == w_ptr
