"""GPU suite (-m gpu) of the CSR SpMM entry (spmv_acc_csr_spmm / spmv_acc_amd.csr_spmm): every column of Y against the CPU oracle's SpMV of
the matching column of X, the entry's contract (beta = 0, padding, empty cases, bad arguments), its bitwise invariants, how it shares the SpMV
plan, streams and captures, 64-bit offsets and one speed gate against k SpMV calls."""
import ctypes

import numpy as np
import pytest

import spmv_acc_amd
from spmv_acc_amd import synth

pytestmark = pytest.mark.gpu

SCALED_TOL = 1e-12
REL_TOL = 1e-9
KS = (1, 2, 3, 7, 8, 16, 17, 33, 64)
ABS = ((1.0, 1.0), (0.5, -2.0), (1.0, 0.0))
# the parity suite's matrices (tests/test_gpu_parity.py KINDS, same synth.random_csr seeds)
KINDS = [("uniform", 3000, 3100, 5), ("short", 5000, 5000, 2), ("powerlaw", 2500, 4000, 6),
         ("spikes", 1500, 9000, 3), ("empty_rows", 4000, 2500, 4), ("dense_rows", 40, 5000, 400),
         ("single", 2049, 2049, 1), ("uniform", 700, 700, 33), ("uniform", 300, 900, 100)]


@pytest.fixture(scope="module")
def torch_dev(hiplib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def hub_csr(seed=5):
    """R-MAT-like: short rows around hub rows of 120 000 and 3 000 non-zeros (longer than any tile, many long-row pieces), nnz % 4 != 0."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 7, size=3000).astype(np.int64)
    lens[5], lens[777], lens[2999] = 120_001, 3_000, 257
    return synth.csr_from_row_lengths(lens, 4000, rng)


def matrices():
    for i, (kind, m, n, avg) in enumerate(KINDS):
        yield (kind, m), synth.random_csr(m, n, avg, seed=100 + i, kind=kind), n
    rp, ci, v = hub_csr()
    yield ("hubs", rp.size - 1), (rp, ci, v), 4000


def make_xy(torch, n, m, k, layout, rng, ldx_pad=0, ldy_pad=0):
    """X (n, k) and Y (m, k) host arrays and device views in `layout` with leading dimensions padded by ldx_pad / ldy_pad."""
    X = rng.standard_normal((n, k))
    Y0 = rng.standard_normal((m, k))
    if layout == "row":
        dXb = torch.zeros((n, k + ldx_pad), dtype=torch.float64, device="cuda")
        dYb = torch.full((m, k + ldy_pad), 7.25, dtype=torch.float64, device="cuda")
        dX, dY = dXb[:, :k], dYb[:, :k]
    else:
        dXb = torch.zeros((k, n + ldx_pad), dtype=torch.float64, device="cuda")
        dYb = torch.full((k, m + ldy_pad), 7.25, dtype=torch.float64, device="cuda")
        dX, dY = dXb[:, :n].t(), dYb[:, :m].t()
    dX.copy_(torch.from_numpy(X))
    dY.copy_(torch.from_numpy(Y0))
    return X, Y0, dX, dY, dYb


def check_cols(oracle, got, alpha, beta, rowptr, cols, vals, X, Y0, tag):
    import scipy.sparse as sp

    absA = sp.csr_matrix((np.abs(vals), cols, rowptr), shape=(rowptr.size - 1, X.shape[0]))
    for j in range(X.shape[1]):
        x, y0 = np.ascontiguousarray(X[:, j]), np.ascontiguousarray(Y0[:, j])
        ref = oracle.host_spmv(alpha, beta, rowptr, cols, vals, x, y0)
        g = np.ascontiguousarray(got[:, j])
        err = oracle.scaled_error(g, ref, alpha, beta, rowptr, cols, vals, x, y0)
        assert err <= SCALED_TOL, (tag, j, "scaled error", err)
        scale = abs(alpha) * (absA @ np.abs(x)) + np.abs(beta * y0)
        solid = np.abs(ref) >= 1e-6 * np.maximum(scale, 1e-300)
        if np.any(solid):
            assert np.max(np.abs(g[solid] - ref[solid]) / np.abs(ref[solid])) <= REL_TOL, (tag, j)
        assert oracle.verify_y(g, ref)[2] == 0, (tag, j)


@pytest.mark.parametrize("layout", ["row", "col"])
def test_spmm_parity(torch_dev, oracle, layout):
    torch = torch_dev
    for tag, (rp, ci, v), n in matrices():
        m, nnz = rp.size - 1, int(rp[-1])
        drp, dci, dv = dev(torch, rp), dev(torch, ci), dev(torch, v)
        rng = np.random.default_rng(len(tag[0]) + m)
        for k in KS:
            for alpha, beta in ABS:
                X, Y0, dX, dY, _ = make_xy(torch, n, m, k, layout, rng)
                spmv_acc_amd.csr_spmm(alpha, beta, m, n, nnz, drp, dci, dv, dX, dY, h_rowptr=rp if k % 2 else None)
                torch.cuda.synchronize()
                check_cols(oracle, dY.cpu().numpy(), alpha, beta, rp, ci, v, X, Y0, (tag, layout, k, alpha, beta))
        spmv_acc_amd.release_plans(drp)


def test_spmm_unrebased_row_range(torch_dev, oracle):
    """Rows [a, b) of a matrix as shard.cpp passes them: rowptr + a, the whole colindex / values, nnz = rowptr[b] (the END offset)."""
    torch = torch_dev
    rp, ci, v = hub_csr(seed=9)
    a, b = 3, 2500  # (holds the 120 001-non-zero row 5 and the 3 000-non-zero row 777)
    sub = rp[a:b + 1]
    drp, dci, dv = dev(torch, rp), dev(torch, ci), dev(torch, v)
    rb = (sub - sub[0]).astype(np.int32)
    cb, vb = ci[sub[0]:sub[-1]], v[sub[0]:sub[-1]]
    rng = np.random.default_rng(3)
    for layout in ("row", "col"):
        for k in (3, 8, 33):
            X, Y0, dX, dY, _ = make_xy(torch, 4000, b - a, k, layout, rng)
            spmv_acc_amd.csr_spmm(0.5, -2.0, b - a, 4000, int(sub[-1]), drp[a:b + 1], dci, dv, dX, dY)
            torch.cuda.synchronize()
            check_cols(oracle, dY.cpu().numpy(), 0.5, -2.0, rb, cb, vb, X, Y0, ("unrebased", layout, k))
    spmv_acc_amd.release_plans(drp[a:b + 1])


def test_spmm_contract(torch_dev, oracle, hiplib):
    torch = torch_dev
    rp, ci, v = synth.random_csr(3000, 3100, 5, seed=100, kind="uniform")
    m, n, nnz = 3000, 3100, int(rp[-1])
    drp, dci, dv = dev(torch, rp), dev(torch, ci), dev(torch, v)
    rng = np.random.default_rng(1)
    sentinel = torch.tensor([7.25], dtype=torch.float64).view(torch.int64).item()
    for layout in ("row", "col"):
        for k in (1, 5, 8, 40):
            # beta == 0: Y full of NaNs comes out finite and right; the padding keeps its sentinel bit for bit
            X, _, dX, dY, dYb = make_xy(torch, n, m, k, layout, rng, ldx_pad=3, ldy_pad=5)
            dY.fill_(float("nan"))
            spmv_acc_amd.csr_spmm(1.5, 0.0, m, n, nnz, drp, dci, dv, dX, dY)
            torch.cuda.synchronize()
            got = dY.cpu().numpy()
            assert np.all(np.isfinite(got)), (layout, k)
            check_cols(oracle, got, 1.5, 0.0, rp, ci, v, X, np.zeros((m, k)), ("beta0", layout, k))
            pad = dYb[:, k:] if layout == "row" else dYb[:, m:]
            assert bool((pad.contiguous().view(torch.int64) == sentinel).all()), (layout, k)
    # k == 0, m == 0: nothing happens; nnz == 0: Y = beta * Y
    X, Y0, dX, dY, _ = make_xy(torch, n, m, 4, "row", rng)
    before = dY.clone()
    spmv_acc_amd.csr_spmm(1.0, 2.0, m, n, nnz, drp, dci, dv, dX[:, :0], dY[:, :0])
    spmv_acc_amd.csr_spmm(1.0, 2.0, 0, n, 0, drp, dci, dv, dX, dY[:0])
    torch.cuda.synchronize()
    assert torch.equal(dY, before)
    zrp = torch.zeros(m + 1, dtype=torch.int32, device="cuda")
    for layout in ("row", "col"):
        X, Y0, dX, dY, _ = make_xy(torch, n, m, 6, layout, rng)
        spmv_acc_amd.csr_spmm(1.0, -3.0, m, n, 0, zrp, dci, dv, dX, dY)
        torch.cuda.synchronize()
        assert np.array_equal(dY.cpu().numpy(), -3.0 * Y0), layout
        dY.fill_(float("nan"))
        spmv_acc_amd.csr_spmm(1.0, 0.0, m, n, 0, zrp, dci, dv, dX, dY)
        torch.cuda.synchronize()
        assert bool((dY == 0).all()), layout
    # bad arguments: SPMV_ACC_ERR_BAD_ARGUMENT from the C entry, nothing launched, Y unchanged
    X, Y0, dX, dY, _ = make_xy(torch, n, m, 4, "row", rng)
    before = dY.clone()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    bad = [(2, 4, 4, 4), (0, -1, 4, 4), (0, 4, 3, 4), (0, 4, 4, 3), (1, 4, n - 1, m), (1, 4, n, m - 1)]
    for layout, k, ldx, ldy in bad:
        rc = hiplib.spmv_acc_csr_spmm(layout, k, 1.0, 1.0, m, n, nnz, None, p(drp), p(dci), p(dv), p(dX), ldx, p(dY), ldy)
        assert rc == 2 and hiplib.spmv_acc_last_error() == 2, (layout, k, ldx, ldy)
    assert hiplib.spmv_acc_csr_spmm(0, 4, 1.0, 1.0, m, n, nnz, None, p(drp), p(dci), p(dv), None, 4, p(dY), 4) == 2
    assert hiplib.spmv_acc_csr_spmm(0, 4, 1.0, 1.0, m, n, nnz, None, p(drp), None, p(dv), p(dX), 4, p(dY), 4) == 2
    assert hiplib.spmv_acc_csr_spmm(0, 4, 1.0, 1.0, m, n, nnz, None, None, p(dci), p(dv), p(dX), 4, p(dY), 4) == 2
    hiplib.spmv_acc_clear_error()
    torch.cuda.synchronize()
    assert torch.equal(dY, before)
    spmv_acc_amd.release_plans(drp)


def test_spmm_bitwise_invariants(torch_dev, hiplib):
    torch = torch_dev
    rp, ci, v = hub_csr(seed=21)
    m, n, nnz = rp.size - 1, 4000, int(rp[-1])
    drp, dci, dv = dev(torch, rp), dev(torch, ci), dev(torch, v)
    rng = np.random.default_rng(8)
    for layout in ("row", "col"):
        for k in (3, 8, 17):
            X, Y0, dX, dY, _ = make_xy(torch, n, m, k, layout, rng)
            outs = []
            for _ in range(3):  # identical calls (and, for SpMV, a zigzag pair): identical bits
                dY.copy_(torch.from_numpy(Y0))
                spmv_acc_amd.csr_spmm(0.5, -2.0, m, n, nnz, drp, dci, dv, dX, dY)
                outs.append(dY.clone())
            assert all(torch.equal(outs[0], o) for o in outs[1:]), (layout, k)
            # ldx = k + 3 and an 8-B offset view of X: the same bits
            _, _, dX2, dY2, _ = make_xy(torch, n, m, k, layout, rng, ldx_pad=3, ldy_pad=1)
            dX2.copy_(dX)
            dY2.copy_(torch.from_numpy(Y0))
            spmv_acc_amd.csr_spmm(0.5, -2.0, m, n, nnz, drp, dci, dv, dX2, dY2)
            assert torch.equal(dY2, outs[0]), (layout, k, "ldx + 3")
            if layout == "row":
                big = torch.zeros((n, k + 1), dtype=torch.float64, device="cuda")
                off = big[:, 1:]  # 8-B aligned only
                off.copy_(dX)
                dY.copy_(torch.from_numpy(Y0))
                spmv_acc_amd.csr_spmm(0.5, -2.0, m, n, nnz, drp, dci, dv, off, dY)
                assert torch.equal(dY, outs[0]), (k, "offset view")
            # column j does not depend on the other columns of X
            dX3 = dX.clone() if layout == "row" else dX.t().contiguous().t()
            dX3[:, 1:] = torch.from_numpy(rng.standard_normal((n, k - 1))).cuda()
            dY.copy_(torch.from_numpy(Y0))
            spmv_acc_amd.csr_spmm(0.5, -2.0, m, n, nnz, drp, dci, dv, dX3, dY)
            assert torch.equal(dY[:, 0], outs[0][:, 0]), (layout, k, "column independence")
    torch.cuda.synchronize()
    spmv_acc_amd.release_plans(drp)
    # k == 1 with contiguous vectors: bitwise csr_spmv with the active strategy after spmv_acc_prepare
    rp, ci, v = synth.random_csr(3000, 3100, 5, seed=100, kind="uniform")
    m, n, nnz = 3000, 3100, int(rp[-1])
    drp, dci, dv = dev(torch, rp), dev(torch, ci), dev(torch, v)
    x, y0 = rng.standard_normal(n), rng.standard_normal(m)
    dx = dev(torch, x)
    spmv_acc_amd.prepare(m, n, nnz, drp, dci, dv, dx)
    for layout in ("row", "col"):
        Y = dev(torch, y0).view(m, 1)
        spmv_acc_amd.csr_spmm(0.5, -2.0, m, n, nnz, drp, dci, dv, dx.view(n, 1), Y)
        y2 = dev(torch, y0)
        spmv_acc_amd.csr_spmv(0.5, -2.0, m, n, nnz, drp, dci, dv, dx, y2)
        torch.cuda.synchronize()
        assert torch.equal(Y.view(m), y2), layout
    spmv_acc_amd.release_plans(drp)


def test_spmm_leaves_the_spmv_plan_alone(torch_dev, oracle, hiplib):
    torch = torch_dev
    rp, ci, v = hub_csr(seed=31)
    m, n, nnz = rp.size - 1, 4000, int(rp[-1])
    drp, dci, dv = dev(torch, rp), dev(torch, ci), dev(torch, v)
    rng = np.random.default_rng(4)
    x, y0 = rng.standard_normal(n), rng.standard_normal(m)
    dx = dev(torch, x)
    spmv_acc_amd.prepare(m, n, nnz, drp, dci, dv, dx)

    def spmv():
        y = dev(torch, y0)
        spmv_acc_amd.csr_spmv(1.0, 1.0, m, n, nnz, drp, dci, dv, dx, y)
        torch.cuda.synchronize()
        return y.cpu().numpy()

    ya, yb = spmv(), spmv()  # a zigzag pair
    info = spmv_acc_amd.query_plan(drp, m)
    plans = hiplib.spmv_acc_cached_plans()
    for k, layout in ((8, "row"), (5, "col"), (40, "row")):
        X, Y0, dX, dY, _ = make_xy(torch, n, m, k, layout, rng)
        spmv_acc_amd.csr_spmm(1.0, 1.0, m, n, nnz, drp, dci, dv, dX, dY)
    torch.cuda.synchronize()
    assert spmv_acc_amd.query_plan(drp, m) == info and hiplib.spmv_acc_cached_plans() == plans
    yc, yd = spmv(), spmv()
    assert np.array_equal(ya.view(np.int64), yc.view(np.int64)) and np.array_equal(yb.view(np.int64), yd.view(np.int64))
    assert spmv_acc_amd.query_plan(drp, m) == info
    spmv_acc_amd.release_plans(drp)


def test_spmm_stale_plan_values_edit_and_release(torch_dev, oracle, hiplib):
    torch = torch_dev
    n = m = 30000
    rng = np.random.default_rng(11)
    lens = np.minimum((rng.pareto(1.3, size=m) * 6).astype(np.int64), 3000) + rng.integers(0, 4, size=m)
    lens[: m // 3] += 9
    rpA, ciA, vA = synth.csr_from_row_lengths(lens, n, rng)
    rpB, ciB, vB = synth.csr_from_row_lengths(lens[::-1].copy(), n, rng)
    nnz = int(rpA[-1])
    drp, dci, dv = dev(torch, rpA), dev(torch, ciA), dev(torch, vA)
    X, Y0, dX, dY, _ = make_xy(torch, n, m, 6, "row", rng)

    def spmm():
        dY.copy_(torch.from_numpy(Y0))
        spmv_acc_amd.csr_spmm(1.0, 1.0, m, n, nnz, drp, dci, dv, dX, dY)
        torch.cuda.synchronize()
        return dY.cpu().numpy()

    hiplib.spmv_acc_clear_error()
    check_cols(oracle, spmm(), 1.0, 1.0, rpA, ciA, vA, X, Y0, "A")
    plans = hiplib.spmv_acc_cached_plans()
    dv.copy_(dev(torch, vA * 1.5))  # values edited in place: picked up, no complaint
    got = spmm()
    assert hiplib.spmv_acc_last_error() == 0 and hiplib.spmv_acc_cached_plans() == plans
    check_cols(oracle, got, 1.0, 1.0, rpA, ciA, vA * 1.5, X, Y0, "A values")
    drp.copy_(dev(torch, rpB))
    dci.copy_(dev(torch, ciB))
    dv.copy_(dev(torch, vB))
    torch.cuda.synchronize()
    reported = False
    try:
        spmm()
    except spmv_acc_amd.SpmvAccError as ex:
        reported = "changed" in str(ex)
    if not reported:
        assert hiplib.spmv_acc_last_error() == 2 and b"changed" in hiplib.spmv_acc_last_error_string()
    hiplib.spmv_acc_clear_error()
    for _ in range(2):
        got = spmm()
        assert hiplib.spmv_acc_last_error() == 0
        check_cols(oracle, got, 1.0, 1.0, rpB, ciB, vB, X, Y0, "B")
    spmv_acc_amd.release_plans(drp)
    # create / use / release: the device memory comes back
    rp, ci, v = hub_csr(seed=41)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(20):
        drp, dci, dv = dev(torch, rp), dev(torch, ci), dev(torch, v)
        X, Y0, dX, dY, _ = make_xy(torch, 4000, rp.size - 1, 8, "row", rng)
        spmv_acc_amd.csr_spmm(1.0, 1.0, rp.size - 1, 4000, int(rp[-1]), drp, dci, dv, dX, dY)
        torch.cuda.synchronize()
        spmv_acc_amd.release_plans(drp)
        del drp, dci, dv, dX, dY
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    assert torch.cuda.mem_get_info()[0] >= free0 - (8 << 20)


def test_spmm_streams_and_capture(torch_dev, oracle, hiplib):
    torch = torch_dev
    rp, ci, v = hub_csr(seed=51)
    m, n, nnz = rp.size - 1, 4000, int(rp[-1])
    drp, dci, dv = dev(torch, rp), dev(torch, ci), dev(torch, v)
    rng = np.random.default_rng(6)
    X, Y0, dX, dY, _ = make_xy(torch, n, m, 8, "row", rng)
    ref = None
    for s in (torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.current_stream()):
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            dY.copy_(torch.from_numpy(Y0))
            spmv_acc_amd.csr_spmm(1.0, 1.0, m, n, nnz, drp, dci, dv, dX, dY)
            out = dY.clone()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        if ref is None:
            ref = out
            check_cols(oracle, out.cpu().numpy(), 1.0, 1.0, rp, ci, v, X, Y0, "streams")
        assert torch.equal(out, ref)
    # after that uncaptured call: a captured SpMM replays to the same bits
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        dY.copy_(torch.from_numpy(Y0))
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            spmv_acc_amd.csr_spmm(1.0, 1.0, m, n, nnz, drp, dci, dv, dX, dY)
    for _ in range(2):
        dY.copy_(torch.from_numpy(Y0))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(dY, ref)
    del g
    spmv_acc_amd.release_plans(drp)
    # a first call inside a capture is refused with a message and does not crash
    drp2 = dev(torch, rp)
    g2 = torch.cuda.CUDAGraph()
    refused = None
    s2 = torch.cuda.Stream()
    s2.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s2):
        torch.cuda.synchronize()
        with torch.cuda.graph(g2, stream=s2):
            try:
                spmv_acc_amd.csr_spmm(1.0, 1.0, m, n, nnz, drp2, dci, dv, dX, dY)
            except spmv_acc_amd.SpmvAccError as ex:
                refused = str(ex)
    assert refused is not None and "capture" in refused
    del g2
    torch.cuda.synchronize()
    spmv_acc_amd.release_plans(drp2)


def test_spmm_grid_stride_at_test_size(torch_dev, oracle, hiplib):
    """max_grid_blocks lowered so that both layouts' kernels, the pieces and the fix-up stride over the rows beyond the grid."""
    torch = torch_dev
    rp, ci, v = hub_csr(seed=61)
    m, n, nnz = rp.size - 1, 4000, int(rp[-1])
    drp, dci, dv = dev(torch, rp), dev(torch, ci), dev(torch, v)
    rng = np.random.default_rng(7)
    try:
        assert hiplib.spmv_acc_set_tunable(b"max_grid_blocks", 3) == 0
        for layout in ("row", "col"):
            for k in (2, 8, 33):
                X, Y0, dX, dY, _ = make_xy(torch, n, m, k, layout, rng)
                spmv_acc_amd.csr_spmm(0.5, -2.0, m, n, nnz, drp, dci, dv, dX, dY)
                torch.cuda.synchronize()
                check_cols(oracle, dY.cpu().numpy(), 0.5, -2.0, rp, ci, v, X, Y0, ("stride", layout, k))
                # nnz == 0 scale path strides too
                Z = torch.zeros(m + 1, dtype=torch.int32, device="cuda")
                spmv_acc_amd.csr_spmm(1.0, 2.0, m, n, 0, Z, dci, dv, dX, dY)
    finally:
        hiplib.spmv_acc_reset_tunables()
    spmv_acc_amd.release_plans(drp)


def test_spmm_offsets_beyond_int32(torch_dev):
    """Row-major X with n = 2^24 and ldx = 160 (21.5 GB): col * ldx reaches 2.7e9 > 2^31 elements; sampled rows against the host."""
    torch = torch_dev
    n, ldx, k, m = 1 << 24, 160, 8, 4096
    rng = np.random.default_rng(99)
    lens = rng.integers(1, 9, size=m)
    rp = np.zeros(m + 1, np.int32)
    np.cumsum(lens, out=rp[1:])
    ci = rng.integers(0, n, size=int(rp[-1])).astype(np.int32)
    ci[:8] = n - 1 - np.arange(8)  # the last columns
    v = rng.standard_normal(int(rp[-1]))
    Xb = torch.empty((n, ldx), dtype=torch.float64, device="cuda")
    X = Xb[:, :k]
    i = torch.arange(n, device="cuda", dtype=torch.float64).view(n, 1)
    j = torch.arange(k, device="cuda", dtype=torch.float64).view(1, k)
    X.copy_(torch.remainder(i, 1009.0) * 1e-3 + j)
    del i
    Y = torch.zeros((m, k), dtype=torch.float64, device="cuda")
    drp, dci, dv = (torch.from_numpy(a).cuda() for a in (rp, ci, v))
    spmv_acc_amd.csr_spmm(1.0, 0.0, m, n, int(rp[-1]), drp, dci, dv, X, Y)
    torch.cuda.synchronize()
    got = Y.cpu().numpy()
    for r in list(range(0, m, 97)) + [0, 1]:
        cols = ci[rp[r]:rp[r + 1]]
        xs = (np.remainder(cols, 1009).astype(np.float64) * 1e-3)[:, None] + np.arange(k)[None, :]
        want = v[rp[r]:rp[r + 1]] @ xs
        scale = np.abs(v[rp[r]:rp[r + 1]]) @ np.abs(xs)
        assert np.all(np.abs(got[r] - want) <= 1e-12 * scale), r
    spmv_acc_amd.release_plans(drp)
    del Xb, X
    torch.cuda.empty_cache()


def test_spmm_k8_is_under_half_of_eight_spmv_calls(torch_dev, hiplib):
    """boneS10 stand-in, row-major k = 8, beta = 1: one SpMM against 8 SpMV calls on the settled SpMV plan, medians of several regions."""
    torch = torch_dev
    m, n, nnz, rp, ci, v = synth.sweep_standin_torch("boneS10")
    k = 8
    X = torch.randn((n, k), dtype=torch.float64, device="cuda")
    Y = torch.randn((m, k), dtype=torch.float64, device="cuda")
    x = X[:, 0].contiguous()
    y = Y[:, 0].contiguous()
    spmv_acc_amd.prepare(m, n, nnz, rp, ci, v, x)
    spmv_region = spmv_acc_amd.time_spmv_region(spmv_acc_amd.get_strategy(), 8, 1.0, 1.0, m, n, nnz, rp, ci, v, x, y)
    spmv_acc_amd.csr_spmm(1.0, 1.0, m, n, nnz, rp, ci, v, X, Y)  # warm-up (builds the SpMM section)
    lib = hiplib
    args = (0, k, 1.0, 1.0, m, n, nnz, None, rp.data_ptr(), ci.data_ptr(), v.data_ptr(), X.data_ptr(), k, Y.data_ptr(), k)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    spmm_ms, spmv_ms = [], []
    for _ in range(7):
        spmv_ms.append(spmv_region())
        torch.cuda.synchronize()
        e0.record()
        for _ in range(4):
            lib.spmv_acc_csr_spmm(*args)
        e1.record()
        torch.cuda.synchronize()
        spmm_ms.append(e0.elapsed_time(e1) / 4)
    assert lib.spmv_acc_last_error() == 0
    a, b = float(np.median(spmm_ms)), float(np.median(spmv_ms))
    print(f"boneS10 k=8: SpMM {a:.4f} ms, 8 SpMV {b:.4f} ms, ratio {a / b:.3f}")
    assert a <= 0.5 * b, (a, b)
    spmv_acc_amd.release_plans(rp)
