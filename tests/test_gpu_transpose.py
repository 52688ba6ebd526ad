"""GPU suite (-m gpu) of the transposed product: the stable device transpose (spmv_acc_csr_transpose / csr_transpose) bit for bit against a host
stable argsort, its value refresh, every hot strategy on the device-made A^T against the CPU oracle, the stateless atomic product
(spmv_acc_csr_spmv_t / csr_spmv_t) against the same oracle results and the adjoint identity, and the contract of the three entries: beta = 0,
empty shapes, un-rebased row ranges, the deterministic switch, bad arguments, no plan, captures, the column guards and grid striding.

No speed gate: the parent commit cannot compute this product, so there is no figure to hold (tools/transpose_bench.py measures)."""
import ctypes

import numpy as np
import pytest

import spmv_acc_amd
from spmv_acc_amd import synth

pytestmark = pytest.mark.gpu

SCALED_TOL = 1e-12  # the project's gate, relative to |alpha| * sum |a| |x| + |beta y0|: it holds for any summation order (see
#                     tests/test_transpose_host.py::test_reversed_order_scatter_stays_within_the_gate, which checks that on the CPU)
ABS = ((1.0, 1.0), (0.5, -2.0), (1.0, 0.0), (0.0, 3.0))
# the parity suite's matrices (tests/test_gpu_parity.py KINDS, same synth.random_csr seeds)
KINDS = [("uniform", 3000, 3100, 5), ("short", 5000, 5000, 2), ("powerlaw", 2500, 4000, 6),
         ("spikes", 1500, 9000, 3), ("empty_rows", 4000, 2500, 4), ("dense_rows", 40, 5000, 400),
         ("single", 2049, 2049, 1), ("uniform", 700, 700, 33), ("uniform", 300, 900, 100)]


def hub_csr(seed=5):
    """tests/test_gpu_spmm.py hub_csr: short rows around hub rows of 120 001, 3 000 and 257 non-zeros, nnz % 4 != 0."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 7, size=3000).astype(np.int64)
    lens[5], lens[777], lens[2999] = 120_001, 3_000, 257
    return synth.csr_from_row_lengths(lens, 4000, rng)


def host_transpose(rp, ci, v, n):
    """(t_rowptr, t_colindex, t_value, perm) of the stable transpose: entries of a column in ascending source position."""
    m = rp.size - 1
    perm = np.argsort(ci, kind="stable").astype(np.int32)
    rows = np.repeat(np.arange(m, dtype=np.int32), np.diff(rp))
    t_rp = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(ci, minlength=n), out=t_rp[1:])
    return t_rp, rows[perm], (None if v is None else v[perm]), perm


def sorted_rows(rp, ci, v):
    """The same matrix with every row's entries in ascending column order (duplicates keep their order)."""
    rows = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    order = np.lexsort((ci, rows))
    return ci[order].copy(), v[order].copy()


def matrices():
    """(tag, (rowptr, colindex, value), n): the parity suite's KINDS, SpMM's hub rows, its transpose (hub COLUMNS of 120 001 and 3 000 entries),
    unsorted columns with duplicates inside rows, m >> n, n >> m, and empty columns."""
    for i, (kind, m, n, avg) in enumerate(KINDS):
        yield (kind, m), synth.random_csr(m, n, avg, seed=100 + i, kind=kind), n
    rp, ci, v = hub_csr()
    yield ("hub_rows", rp.size - 1), (rp, ci, v), 4000
    t_rp, t_ci, t_v, _ = host_transpose(rp, ci, v, 4000)
    yield ("hub_cols", 4000), (t_rp, t_ci, t_v), rp.size - 1
    rng = np.random.default_rng(77)
    lens = rng.integers(0, 40, size=900)
    rp = np.zeros(901, dtype=np.int32)
    np.cumsum(lens, out=rp[1:])
    ci = rng.integers(0, 12, size=int(rp[-1])).astype(np.int32) * 50  # twelve distinct columns: every row holds duplicates, in random order
    yield ("duplicates", 900), (rp, ci, rng.uniform(-1, 1, ci.size)), 600
    yield ("tall", 60000), synth.random_csr(60000, 37, 3, seed=201, kind="uniform"), 37
    yield ("wide", 37), synth.random_csr(37, 60000, 300, seed=202, kind="uniform"), 60000
    rp, ci, v = synth.random_csr(3000, 2000, 6, seed=203, kind="uniform")
    yield ("empty_cols", 3000), (rp, (ci // 7 * 7).astype(np.int32), v), 2000  # six of seven columns are empty


@pytest.fixture(scope="module")
def torch_dev(hiplib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def same(t, a):
    return np.array_equal(t.cpu().numpy(), a)


def test_transpose_is_the_host_stable_argsort(torch_dev):
    torch = torch_dev
    cases = list(matrices())
    cases.append((("large", 200_000), synth.random_csr(200_000, 150_000, 16, seed=204, kind="uniform"), 150_000))  # 3.2 M pairs: the sort's large path
    for tag, (rp, ci, v), n in cases:
        m, nnz = rp.size - 1, int(rp[-1])
        drp, dci, dv = dev(torch, rp), dev(torch, ci), dev(torch, v)
        w_rp, w_ci, w_v, w_perm = host_transpose(rp, ci, v, n)
        t_rp, t_ci, t_v, perm = spmv_acc_amd.csr_transpose(m, n, nnz, drp, dci, dv, want_perm=True)
        assert same(t_rp, w_rp) and same(t_ci, w_ci) and same(perm, w_perm), tag
        assert np.array_equal(t_v.cpu().numpy().view(np.int64), w_v.view(np.int64)), tag
        # structure only; no perm; nnz read from the device; called twice: the same arrays
        s_rp, s_ci, s_v = spmv_acc_amd.csr_transpose(m, n, -1, drp, dci)
        assert s_v is None and torch.equal(s_rp, t_rp) and torch.equal(s_ci, t_ci), tag
        a_rp, a_ci, a_v = spmv_acc_amd.csr_transpose(m, n, nnz, drp, dci, dv)
        assert torch.equal(a_rp, t_rp) and torch.equal(a_ci, t_ci) and torch.equal(a_v, t_v), tag
        # the values follow an in-place edit through perm
        dv.mul_(-1.5).add_(0.25)
        fresh = spmv_acc_amd.csr_transpose(m, n, nnz, drp, dci, dv)[2]
        spmv_acc_amd.csr_transpose_values(perm, dv, t_v)
        assert torch.equal(t_v, fresh), tag
        # column-sorted rows: the transpose of the transpose is the input
        sci, sv = sorted_rows(rp, ci, v)
        dsci, dsv = dev(torch, sci), dev(torch, sv)
        u_rp, u_ci, u_v = spmv_acc_amd.csr_transpose(m, n, nnz, drp, dsci, dsv)
        b_rp, b_ci, b_v = spmv_acc_amd.csr_transpose(n, m, nnz, u_rp, u_ci, u_v)
        assert torch.equal(b_rp, drp) and torch.equal(b_ci, dsci) and torch.equal(b_v, dsv), tag


def test_every_hot_strategy_on_the_device_made_transpose(torch_dev, oracle):
    torch = torch_dev
    for tag, (rp, ci, v), n in matrices():
        m, nnz = rp.size - 1, int(rp[-1])
        t_rp, t_ci, t_v = spmv_acc_amd.csr_transpose(m, n, nnz, dev(torch, rp), dev(torch, ci), dev(torch, v))
        w_rp, w_ci, w_v, _ = host_transpose(rp, ci, v, n)
        rng = np.random.default_rng(m + n)
        x, y0 = rng.standard_normal(m), rng.standard_normal(n)
        dx = dev(torch, x)
        for alpha, beta in ((1.0, 1.0), (0.5, -2.0)):
            ref = oracle.host_spmv(alpha, beta, w_rp, w_ci, w_v, x, y0)
            for strat in spmv_acc_amd.HOT_STRATEGIES:
                dy = dev(torch, y0)
                spmv_acc_amd.csr_spmv(alpha, beta, n, m, nnz, t_rp, t_ci, t_v, dx, dy, strategy=strat)
                torch.cuda.synchronize()
                got = dy.cpu().numpy()
                err = oracle.scaled_error(got, ref, alpha, beta, w_rp, w_ci, w_v, x, y0)
                print(f"{tag} {strat} alpha {alpha} beta {beta}: scaled error {err:.3e}")
                assert err <= SCALED_TOL, (tag, strat, alpha, beta, err)
                assert oracle.verify(got, ref) == -1, (tag, strat, alpha, beta)
        spmv_acc_amd.release_plans(t_rp)


def test_spmv_t_parity(torch_dev, oracle):
    torch = torch_dev
    for tag, (rp, ci, v), n in matrices():
        m, nnz = rp.size - 1, int(rp[-1])
        drp, dci, dv = dev(torch, rp), dev(torch, ci), dev(torch, v)
        w_rp, w_ci, w_v, _ = host_transpose(rp, ci, v, n)
        rng = np.random.default_rng(m + 3 * n)
        x, y0 = rng.standard_normal(m), rng.standard_normal(n)
        dx = dev(torch, x)
        for alpha, beta in ABS:
            ref = oracle.host_spmv(alpha, beta, w_rp, w_ci, w_v, x, y0)
            dy = dev(torch, y0)
            spmv_acc_amd.csr_spmv_t(alpha, beta, m, n, nnz if alpha != 0.5 else -1, drp, dci, dv, dx, dy)
            torch.cuda.synchronize()
            err = oracle.scaled_error(dy.cpu().numpy(), ref, alpha, beta, w_rp, w_ci, w_v, x, y0)
            print(f"{tag} alpha {alpha} beta {beta}: scaled error {err:.3e}")
            assert err <= SCALED_TOL, (tag, alpha, beta, err)


def test_adjoint_identity(torch_dev):
    """<A x, w> (the existing csr_spmv) against <x, A^T w> (csr_spmv_t), relative to the sum of the absolute products."""
    torch = torch_dev
    for tag, (rp, ci, v), n in matrices():
        m, nnz = rp.size - 1, int(rp[-1])
        drp, dci, dv = dev(torch, rp), dev(torch, ci), dev(torch, v)
        rng = np.random.default_rng(5 * m + n)
        x, w = rng.standard_normal(n), rng.standard_normal(m)
        dx, dw = dev(torch, x), dev(torch, w)
        ax = torch.zeros(m, dtype=torch.float64, device="cuda")
        atw = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
        spmv_acc_amd.csr_spmv(1.0, 0.0, m, n, nnz, drp, dci, dv, dx, ax)
        spmv_acc_amd.csr_spmv_t(1.0, 0.0, m, n, nnz, drp, dci, dv, dw, atw)
        torch.cuda.synchronize()
        left, right = float(np.dot(ax.cpu().numpy(), w)), float(np.dot(x, atw.cpu().numpy()))
        rows = np.repeat(np.arange(m), np.diff(rp))
        scale = float(np.sum(np.abs(v) * np.abs(x[ci]) * np.abs(w[rows])))
        print(f"{tag}: <Ax,w> {left:.17g} <x,A^T w> {right:.17g} scale {scale:.3e}")
        assert abs(left - right) <= SCALED_TOL * scale, (tag, left, right, scale)
        spmv_acc_amd.release_plans(drp)


def test_spmv_t_contract(torch_dev, oracle, hiplib):
    torch = torch_dev
    rp, ci, v = hub_csr(seed=9)
    m, n, nnz = rp.size - 1, 4000, int(rp[-1])
    drp, dci, dv = dev(torch, rp), dev(torch, ci), dev(torch, v)
    w_rp, w_ci, w_v, _ = host_transpose(rp, ci, v, n)
    rng = np.random.default_rng(2)
    x, y0 = rng.standard_normal(m), rng.standard_normal(n)
    dx = dev(torch, x)
    plans = hiplib.spmv_acc_cached_plans()
    # beta == 0 over a y full of NaNs
    dy = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    spmv_acc_amd.csr_spmv_t(1.5, 0.0, m, n, nnz, drp, dci, dv, dx, dy)
    torch.cuda.synchronize()
    got = dy.cpu().numpy()
    assert np.all(np.isfinite(got))
    ref = oracle.host_spmv(1.5, 0.0, w_rp, w_ci, w_v, x, np.zeros(n))
    assert oracle.scaled_error(got, ref, 1.5, 0.0, w_rp, w_ci, w_v, x, np.zeros(n)) <= SCALED_TOL
    # m == 0 and nnz == 0: y = beta * y; n == 0: nothing
    zrp = torch.zeros(m + 1, dtype=torch.int32, device="cuda")
    for args in ((0, n, 0, zrp), (m, n, 0, zrp)):
        dy = dev(torch, y0)
        spmv_acc_amd.csr_spmv_t(1.0, -3.0, args[0], args[1], args[2], args[3], dci, dv, dx, dy)
        torch.cuda.synchronize()
        assert np.array_equal(dy.cpu().numpy(), -3.0 * y0), args[:3]
    dy = dev(torch, y0)
    spmv_acc_amd.csr_spmv_t(1.0, -3.0, m, 0, 0, zrp, dci, dv, dx, dy[:0])
    torch.cuda.synchronize()
    assert np.array_equal(dy.cpu().numpy(), y0)
    # an un-rebased row sub-range per half (rowptr + r0, whole colindex / value, nnz = the END offset): the halves sum to the whole
    whole = dev(torch, y0)
    spmv_acc_amd.csr_spmv_t(0.5, -2.0, m, n, nnz, drp, dci, dv, dx, whole)
    halves = dev(torch, y0)
    cut = 1700
    spmv_acc_amd.csr_spmv_t(0.5, -2.0, cut, n, int(rp[cut]), drp[:cut + 1], dci, dv, dx[:cut], halves)
    spmv_acc_amd.csr_spmv_t(0.5, 1.0, m - cut, n, int(rp[m]), drp[cut:], dci, dv, dx[cut:], halves)
    torch.cuda.synchronize()
    ref = oracle.host_spmv(0.5, -2.0, w_rp, w_ci, w_v, x, y0)
    for name, t in (("whole", whole), ("halves", halves)):
        assert oracle.scaled_error(t.cpu().numpy(), ref, 0.5, -2.0, w_rp, w_ci, w_v, x, y0) <= SCALED_TOL, name
    # tunable deterministic = 1: refused with a message that names the transpose, nothing launched
    dy = dev(torch, y0)
    try:
        assert hiplib.spmv_acc_set_tunable(b"deterministic", 1) == 0
        with pytest.raises(spmv_acc_amd.SpmvAccError, match="spmv_acc_csr_transpose"):
            spmv_acc_amd.csr_spmv_t(1.0, 0.0, m, n, nnz, drp, dci, dv, dx, dy)
        assert hiplib.spmv_acc_csr_spmv_t(1.0, 0.0, m, n, nnz, ptr(drp), ptr(dci), ptr(dv), ptr(dx), ptr(dy)) == 2
        # ... while the transpose route runs under the switch
        t_rp, t_ci, t_v = spmv_acc_amd.csr_transpose(m, n, nnz, drp, dci, dv)
        assert same(t_rp, w_rp) and same(t_ci, w_ci)
    finally:
        hiplib.spmv_acc_reset_tunables()
        hiplib.spmv_acc_clear_error()
    torch.cuda.synchronize()
    assert np.array_equal(dy.cpu().numpy(), y0)
    # null / negative arguments: SPMV_ACC_ERR_BAD_ARGUMENT from the C entries, nothing launched
    t = hiplib.spmv_acc_csr_spmv_t
    bad = [(1.0, 1.0, -1, n, nnz, ptr(drp), ptr(dci), ptr(dv), ptr(dx), ptr(dy)), (1.0, 1.0, m, -1, nnz, ptr(drp), ptr(dci), ptr(dv), ptr(dx), ptr(dy)),
           (1.0, 1.0, m, n, nnz, None, ptr(dci), ptr(dv), ptr(dx), ptr(dy)), (1.0, 1.0, m, n, nnz, ptr(drp), None, ptr(dv), ptr(dx), ptr(dy)),
           (1.0, 1.0, m, n, nnz, ptr(drp), ptr(dci), None, ptr(dx), ptr(dy)), (1.0, 1.0, m, n, nnz, ptr(drp), ptr(dci), ptr(dv), None, ptr(dy)),
           (1.0, 1.0, m, n, nnz, ptr(drp), ptr(dci), ptr(dv), ptr(dx), None)]
    for args in bad:
        assert t(*args) == 2 and hiplib.spmv_acc_last_error() == 2, args[2:5]
    tr, tv = hiplib.spmv_acc_csr_transpose, hiplib.spmv_acc_csr_transpose_values
    o_rp = torch.full((n + 1,), -7, dtype=torch.int32, device="cuda")
    o_ci = torch.full((nnz,), -7, dtype=torch.int32, device="cuda")
    o_v = torch.full((nnz,), 7.25, dtype=torch.float64, device="cuda")
    bad = [(-1, n, nnz, ptr(drp), ptr(dci), ptr(dv), ptr(o_rp), ptr(o_ci), ptr(o_v), None), (m, -1, nnz, ptr(drp), ptr(dci), ptr(dv), ptr(o_rp), ptr(o_ci), ptr(o_v), None),
           (m, n, nnz, None, ptr(dci), ptr(dv), ptr(o_rp), ptr(o_ci), ptr(o_v), None), (m, n, nnz, ptr(drp), None, ptr(dv), ptr(o_rp), ptr(o_ci), ptr(o_v), None),
           (m, n, nnz, ptr(drp), ptr(dci), ptr(dv), None, ptr(o_ci), ptr(o_v), None), (m, n, nnz, ptr(drp), ptr(dci), ptr(dv), ptr(o_rp), None, ptr(o_v), None),
           (m, n, nnz, ptr(drp), ptr(dci), ptr(dv), ptr(o_rp), ptr(o_ci), None, None), (m, n, nnz, ptr(drp), ptr(dci), None, ptr(o_rp), ptr(o_ci), ptr(o_v), None),
           (m, n, nnz - 1, ptr(drp), ptr(dci), ptr(dv), ptr(o_rp), ptr(o_ci), ptr(o_v), None),        # nnz is not rowptr[m]
           (m - 6, n, -1, ptr(drp[6:]), ptr(dci), ptr(dv), ptr(o_rp), ptr(o_ci), ptr(o_v), None)]  # un-rebased: rowptr[0] != 0
    for args in bad:
        assert tr(*args) == 2 and hiplib.spmv_acc_last_error() == 2, args[:3]
    assert tv(-1, ptr(o_ci), ptr(dv), ptr(o_v)) == 2 and tv(nnz, None, ptr(dv), ptr(o_v)) == 2 and tv(nnz, ptr(o_ci), None, ptr(o_v)) == 2
    assert tv(nnz, ptr(o_ci), ptr(dv), None) == 2 and tv(0, None, None, None) == 0
    assert tr(2 ** 31 - 1, n, nnz, ptr(drp), ptr(dci), ptr(dv), ptr(o_rp), ptr(o_ci), ptr(o_v), None) == 4  # SPMV_ACC_ERR_TOO_LARGE
    assert t(1.0, 1.0, m, 2 ** 31 - 1, nnz, ptr(drp), ptr(dci), ptr(dv), ptr(dx), ptr(dy)) == 4
    hiplib.spmv_acc_clear_error()
    torch.cuda.synchronize()
    assert bool((o_rp == -7).all()) and bool((o_ci == -7).all()) and bool((o_v == 7.25).all()) and np.array_equal(dy.cpu().numpy(), y0)
    # empty matrices: t_rowptr is all zeros, nothing else is written
    for mm, nn, kk in ((0, n, 0), (m, n, 0)):
        o_rp.fill_(-7)
        assert tr(mm, nn, kk, ptr(zrp), ptr(dci), ptr(dv), ptr(o_rp), ptr(o_ci), ptr(o_v), None) == 0
        torch.cuda.synchronize()
        assert bool((o_rp == 0).all()) and bool((o_ci == -7).all()) and bool((o_v == 7.25).all())
    one = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    assert tr(m, 0, 0, ptr(zrp), ptr(dci), ptr(dv), ptr(one), ptr(o_ci), ptr(o_v), None) == 0
    torch.cuda.synchronize()
    assert one.tolist() == [0, -7, -7]
    # none of this made or touched a plan
    assert hiplib.spmv_acc_cached_plans() == plans
    spmv_acc_amd.release_plans(t_rp)


def test_transposed_calls_leave_the_plans_alone(torch_dev, hiplib):
    torch = torch_dev
    rp, ci, v = hub_csr(seed=31)
    m, n, nnz = rp.size - 1, 4000, int(rp[-1])
    drp, dci, dv = dev(torch, rp), dev(torch, ci), dev(torch, v)
    rng = np.random.default_rng(4)
    dx, dw = dev(torch, rng.standard_normal(n)), dev(torch, rng.standard_normal(m))
    y = torch.zeros(m, dtype=torch.float64, device="cuda")
    spmv_acc_amd.prepare(m, n, nnz, drp, dci, dv, dx)
    region = spmv_acc_amd.time_spmv_region(spmv_acc_amd.get_strategy(), 2, 1.0, 1.0, m, n, nnz, drp, dci, dv, dx, y)
    region()
    info, plans = spmv_acc_amd.query_plan(drp, m), hiplib.spmv_acc_cached_plans()
    z = torch.zeros(n, dtype=torch.float64, device="cuda")
    for _ in range(3):
        spmv_acc_amd.csr_spmv_t(1.0, 1.0, m, n, nnz, drp, dci, dv, dw, z)
        t_rp, t_ci, t_v, perm = spmv_acc_amd.csr_transpose(m, n, nnz, drp, dci, dv, want_perm=True)
        spmv_acc_amd.csr_transpose_values(perm, dv, t_v)
    torch.cuda.synchronize()
    assert hiplib.spmv_acc_cached_plans() == plans and spmv_acc_amd.query_plan(drp, m) == info
    region()  # (fails if plan work ran inside it: the matrix' plan is as settled as before)
    assert hiplib.spmv_acc_last_prepare_us() == 0.0
    spmv_acc_amd.release_plans(drp)


def test_first_spmv_t_inside_a_capture_and_transpose_refused_there(torch_dev, oracle, hiplib):
    torch = torch_dev
    rp, ci, v = hub_csr(seed=51)
    m, n, nnz = rp.size - 1, 4000, int(rp[-1])
    drp, dci, dv = dev(torch, rp), dev(torch, ci), dev(torch, v)  # a matrix the library has never seen
    w_rp, w_ci, w_v, _ = host_transpose(rp, ci, v, n)
    rng = np.random.default_rng(6)
    x, y0 = rng.standard_normal(m), rng.standard_normal(n)
    dx, dy, dy0 = dev(torch, x), dev(torch, y0), dev(torch, y0)
    o_rp = torch.full((n + 1,), -7, dtype=torch.int32, device="cuda")
    o_ci = torch.full((nnz,), -7, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    refused = None
    with torch.cuda.stream(s):
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            spmv_acc_amd.csr_spmv_t(0.5, -2.0, m, n, nnz, drp, dci, dv, dx, dy)
            hiplib.spmv_acc_set_stream(ctypes.c_void_p(s.cuda_stream))
            rc = hiplib.spmv_acc_csr_transpose(m, n, nnz, ptr(drp), ptr(dci), None, ptr(o_rp), ptr(o_ci), None, None)
            refused = (rc, hiplib.spmv_acc_last_error_string().decode())
            hiplib.spmv_acc_clear_error()
            try:  # nnz < 0 would read rowptr[m]: refused inside a capture as well
                spmv_acc_amd.csr_spmv_t(0.5, -2.0, m, n, -1, drp, dci, dv, dx, dy)
                unknown_nnz = None
            except spmv_acc_amd.SpmvAccError as ex:
                unknown_nnz = str(ex)
    assert refused[0] == 2 and "capture" in refused[1], refused
    assert unknown_nnz is not None and "capture" in unknown_nnz
    ref = oracle.host_spmv(0.5, -2.0, w_rp, w_ci, w_v, x, y0)
    for _ in range(2):
        dy.copy_(dy0)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert oracle.scaled_error(dy.cpu().numpy(), ref, 0.5, -2.0, w_rp, w_ci, w_v, x, y0) <= SCALED_TOL
    assert bool((o_rp == -7).all()) and bool((o_ci == -7).all())  # the refused transpose enqueued nothing
    del g


def test_column_guards_keep_writes_inside_the_outputs(torch_dev, oracle, hiplib):
    """Crafted columns in [n, n + pad), with y / the outputs the first part of larger owned buffers: a missing guard would write owned memory
    (and fail this test), never fault."""
    torch = torch_dev
    rp, ci, v = synth.random_csr(3000, 3100, 5, seed=100, kind="uniform")
    m, n, nnz, pad = 3000, 3100, int(rp[-1]), 64
    rng = np.random.default_rng(12)
    where = rng.choice(nnz, 200, replace=False)
    bad_ci = ci.copy()
    bad_ci[where] = n + rng.integers(0, pad, size=where.size)
    kept_v = v.copy()
    kept_v[where] = 0.0  # what the product must equal: the matrix without those entries
    kept_ci = ci.copy()
    drp, dci, dv = dev(torch, rp), dev(torch, bad_ci), dev(torch, v)
    x, y0 = rng.standard_normal(m), rng.standard_normal(n)
    dx = dev(torch, x)
    buf = torch.full((n + pad,), 7.25, dtype=torch.float64, device="cuda")
    buf[:n] = dev(torch, y0)
    spmv_acc_amd.csr_spmv_t(0.5, -2.0, m, n, nnz, drp, dci, dv, dx, buf[:n])
    torch.cuda.synchronize()
    assert bool((buf[n:] == 7.25).all())
    w_rp, w_ci, w_v, _ = host_transpose(rp, kept_ci, kept_v, n)
    ref = oracle.host_spmv(0.5, -2.0, w_rp, w_ci, w_v, x, y0)
    assert oracle.scaled_error(buf[:n].cpu().numpy(), ref, 0.5, -2.0, w_rp, w_ci, w_v, x, y0) <= SCALED_TOL
    # the transpose counts them, writes nothing and says so
    o_rp = torch.full((n + 1 + pad,), -7, dtype=torch.int32, device="cuda")
    o_ci = torch.full((nnz + pad,), -7, dtype=torch.int32, device="cuda")
    o_v = torch.full((nnz + pad,), 7.25, dtype=torch.float64, device="cuda")
    o_p = torch.full((nnz + pad,), -7, dtype=torch.int32, device="cuda")
    rc = hiplib.spmv_acc_csr_transpose(m, n, nnz, ptr(drp), ptr(dci), ptr(dv), ptr(o_rp), ptr(o_ci), ptr(o_v), ptr(o_p))
    msg = hiplib.spmv_acc_last_error_string().decode()
    hiplib.spmv_acc_clear_error()
    torch.cuda.synchronize()
    assert rc == 2 and "200 column indices outside" in msg, (rc, msg)
    assert bool((o_rp == -7).all()) and bool((o_ci == -7).all()) and bool((o_v == 7.25).all()) and bool((o_p == -7).all())
    # negative columns are out of range too
    neg = ci.copy()
    neg[where[:5]] = -1 - np.arange(5, dtype=np.int32)
    buf[:n] = dev(torch, y0)
    spmv_acc_amd.csr_spmv_t(0.5, -2.0, m, n, nnz, drp, dev(torch, neg), dv, dx, buf[:n])
    torch.cuda.synchronize()
    kept_v = v.copy()
    kept_v[where[:5]] = 0.0
    w_rp, w_ci, w_v, _ = host_transpose(rp, ci, kept_v, n)
    ref = oracle.host_spmv(0.5, -2.0, w_rp, w_ci, w_v, x, y0)
    assert oracle.scaled_error(buf[:n].cpu().numpy(), ref, 0.5, -2.0, w_rp, w_ci, w_v, x, y0) <= SCALED_TOL and bool((buf[n:] == 7.25).all())
    with pytest.raises(spmv_acc_amd.SpmvAccError, match="5 column indices outside"):
        spmv_acc_amd.csr_transpose(m, n, nnz, drp, dev(torch, neg), dv)


def test_transpose_grid_stride_at_test_size(torch_dev, oracle, hiplib):
    """max_grid_blocks lowered to 3: every kernel of the three entries strides over the work beyond its grid."""
    torch = torch_dev
    rp, ci, v = hub_csr(seed=61)
    m, n, nnz = rp.size - 1, 4000, int(rp[-1])
    drp, dci, dv = dev(torch, rp), dev(torch, ci), dev(torch, v)
    w_rp, w_ci, w_v, w_perm = host_transpose(rp, ci, v, n)
    rng = np.random.default_rng(7)
    x, y0 = rng.standard_normal(m), rng.standard_normal(n)
    dx = dev(torch, x)
    try:
        assert hiplib.spmv_acc_set_tunable(b"max_grid_blocks", 3) == 0
        t_rp, t_ci, t_v, perm = spmv_acc_amd.csr_transpose(m, n, nnz, drp, dci, dv, want_perm=True)
        assert same(t_rp, w_rp) and same(t_ci, w_ci) and same(perm, w_perm) and same(t_v, w_v)
        out = torch.zeros_like(t_v)
        spmv_acc_amd.csr_transpose_values(perm, dv, out)
        assert torch.equal(out, t_v)
        for alpha, beta in ((0.5, -2.0), (1.0, 0.0)):
            dy = dev(torch, y0)
            spmv_acc_amd.csr_spmv_t(alpha, beta, m, n, nnz, drp, dci, dv, dx, dy)
            torch.cuda.synchronize()
            ref = oracle.host_spmv(alpha, beta, w_rp, w_ci, w_v, x, y0)
            assert oracle.scaled_error(dy.cpu().numpy(), ref, alpha, beta, w_rp, w_ci, w_v, x, y0) <= SCALED_TOL, (alpha, beta)
    finally:
        hiplib.spmv_acc_reset_tunables()
