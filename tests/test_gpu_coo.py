"""GPU suite (-m gpu) of the device COO -> CSR assembly (spmv_acc_coo_to_csr / coo_to_csr, spmv_acc_coo_to_csr_values / coo_to_csr_values):
structure and map bit for bit against a host stable lexsort, the values bit for bit against the documented summation order
(tests/test_coo_host.py coo_sum_model), re-assembly through the kept map (plain and from a replayed graph, and with a crafted map between guard
words), the assembled matrix through the tuned engine against the CPU oracle, and the contract of the two entries: out-of-range indices,
empty input, captures, no plan, the deterministic switch, too-large sizes and grid striding.

No speed gate: the parent commit cannot do this job, so there is no figure to hold (tools/coo_bench.py measures, profiles/coo_bench.md records)."""
import ctypes
import functools

import numpy as np
import pytest

import spmv_acc_amd
from spmv_acc_amd import synth
from test_coo_host import LONG_RUN, coo_sum_model, host_assemble

pytestmark = pytest.mark.gpu

SCALED_TOL = 1e-12  # the project's gate, relative to |alpha| * sum |a| |x| + |beta y0| (tests/test_gpu_transpose.py SCALED_TOL)


def split_into_duplicates(rp, ci, seed):
    """Every entry of a CSR as 1 ... 4 triples with random values, shuffled."""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(rp.size - 1, dtype=np.int32), np.diff(rp))
    reps = rng.integers(1, 5, size=ci.size)
    row, col = np.repeat(rows, reps), np.repeat(ci, reps)
    return synth.shuffle_coo(row, col, rng.uniform(-1.0, 1.0, size=row.size), seed + 1)


def distinct_positions(m, n, count, rng):
    pos = rng.choice(m * n, size=count, replace=False)
    return (pos // n).astype(np.int32), (pos % n).astype(np.int32)


def _triple_lists():
    rng = np.random.default_rng(2024)
    row, col, val = synth.fem_quads_coo(60, 50, seed=1)
    yield ("quads_shuffled", 61 * 51, 61 * 51) + synth.shuffle_coo(row, col, val, seed=2)
    r, c = distinct_positions(300, 500, 8000, rng)
    o = np.lexsort((c, r))
    v = rng.standard_normal(8000)
    yield "sorted_no_duplicates", 300, 500, r[o].copy(), c[o].copy(), v
    yield "reversed_no_duplicates", 300, 500, r[o][::-1].copy(), c[o][::-1].copy(), v
    yield "one_position_1x1", 1, 1, np.zeros(5000, np.int32), np.zeros(5000, np.int32), rng.standard_normal(5000)
    r, c = distinct_positions(200, 200, 2997, rng)  # a long run inside short ones, runs of kCooLongRun and kCooLongRun + 1 beside it; 8 126 % 64 != 0
    r = np.concatenate([r, np.full(5000, 77, np.int32), np.full(LONG_RUN, 5, np.int32), np.full(LONG_RUN + 1, 6, np.int32)])
    c = np.concatenate([c, np.full(5000, 123, np.int32), np.full(LONG_RUN, 9, np.int32), np.full(LONG_RUN + 1, 9, np.int32)])
    yield ("long_run_among_short",) + (200, 200) + synth.shuffle_coo(r, c, rng.standard_normal(r.size) * 10.0 ** rng.integers(-3, 4, r.size), seed=3)
    yield "single_triple", 5, 7, np.array([3], np.int32), np.array([6], np.int32), np.array([-0.0])
    yield "one_row", 1, 9000, np.zeros(20000, np.int32), rng.integers(0, 9000, 20000).astype(np.int32), rng.standard_normal(20000)
    yield "one_column", 9000, 1, rng.integers(0, 9000, 20000).astype(np.int32), np.zeros(20000, np.int32), rng.standard_normal(20000)
    yield ("empty_first_and_last_rows", 1200, 900, rng.integers(100, 1100, 30000).astype(np.int32), rng.integers(0, 900, 30000).astype(np.int32),
           rng.standard_normal(30000))
    yield ("key_of_34_bits", 70_000, 70_000, rng.integers(0, 70_000, 200_000).astype(np.int32), rng.integers(0, 70_000, 200_000).astype(np.int32),
           rng.standard_normal(200_000))
    rp, ci, _ = synth.random_csr(200_000, 150_000, 8, seed=204, kind="uniform")  # 1.6 M entries as 3.2 M triples: the sort's large path
    rows = np.repeat(np.arange(200_000, dtype=np.int32), np.diff(rp))
    yield ("large", 200_000, 150_000) + synth.shuffle_coo(np.repeat(rows, 2), np.repeat(ci, 2), rng.standard_normal(2 * ci.size), seed=5)


@functools.lru_cache(maxsize=None)
def triple_lists():
    """(tag, m, n, row, col, val): the cases of the issue, made once and shared (nothing changes them)."""
    return tuple(_triple_lists())


@functools.lru_cache(maxsize=None)
def reference(tag):
    """(rowptr, colindex, order, start, value) of the host for a case of triple_lists(), computed once."""
    _, m, n, row, col, val = next(c for c in triple_lists() if c[0] == tag)
    w_rp, w_ci, w_order, w_start = host_assemble(m, n, row, col)
    return w_rp, w_ci, w_order, w_start, coo_sum_model(w_order, w_start, val)


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


def same_bits(t, a):
    return np.array_equal(t.cpu().numpy().view(np.int64), np.ascontiguousarray(a).view(np.int64))


def test_assembly_is_the_host_stable_sort(torch_dev):
    torch = torch_dev
    for tag, m, n, row, col, val in triple_lists():
        w_rp, w_ci, w_order, w_start, w_v = reference(tag)
        drow, dcol, dval = dev(torch, row), dev(torch, col), dev(torch, val)
        rp, ci, v, order, start = spmv_acc_amd.coo_to_csr(m, n, drow, dcol, dval, want_map=True)
        assert ci.numel() == w_ci.size and v.numel() == w_ci.size and start.numel() == w_ci.size + 1, (tag, ci.numel(), w_ci.size)  # *h_nnz
        assert same(rp, w_rp) and same(ci, w_ci) and same(order, w_order) and same(start, w_start), tag
        assert same_bits(v, w_v), tag
        # structure only; no map; called twice: the same arrays
        s_rp, s_ci, s_v = spmv_acc_amd.coo_to_csr(m, n, drow, dcol)
        assert s_v is None and torch.equal(s_rp, rp) and torch.equal(s_ci, ci), tag
        a_rp, a_ci, a_v = spmv_acc_amd.coo_to_csr(m, n, drow, dcol, dval)
        assert torch.equal(a_rp, rp) and torch.equal(a_ci, ci) and same_bits(a_v, w_v), tag
        b_rp, b_ci, b_v, b_order, b_start = spmv_acc_amd.coo_to_csr(m, n, drow, dcol, dval, want_map=True)
        assert torch.equal(b_rp, rp) and torch.equal(b_ci, ci) and same_bits(b_v, w_v) and torch.equal(b_order, order) and torch.equal(b_start, start), tag


def test_reassembly_follows_new_values(torch_dev, hiplib):
    torch = torch_dev
    cases = [c for c in triple_lists() if c[0] in ("quads_shuffled", "long_run_among_short", "one_position_1x1", "single_triple", "key_of_34_bits")]
    for tag, m, n, row, col, val in cases:
        drow, dcol, dval = dev(torch, row), dev(torch, col), dev(torch, val)
        rp, ci, v, order, start = spmv_acc_amd.coo_to_csr(m, n, drow, dcol, dval, want_map=True)
        nnz = ci.numel()
        new = np.random.default_rng(nnz).standard_normal(row.size)
        dnew = dev(torch, new)
        w_v = coo_sum_model(order.cpu().numpy(), start.cpu().numpy(), new)
        out = torch.full((nnz,), 7.25, dtype=torch.float64, device="cuda")
        spmv_acc_amd.coo_to_csr_values(order, start, dnew, out)
        fresh = spmv_acc_amd.coo_to_csr(m, n, drow, dcol, dnew)[2]
        assert same_bits(out, w_v) and same_bits(fresh, w_v), tag
        # captured into a graph (one stream, no parallel branches) and replayed twice, on values edited in place between the replays
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=s):
                spmv_acc_amd.coo_to_csr_values(order, start, dnew, out)
        for scale in (1.0, -3.0):
            dnew.copy_(dev(torch, new * scale))
            out.fill_(7.25)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert same_bits(out, coo_sum_model(order.cpu().numpy(), start.cpu().numpy(), new * scale)), (tag, scale)
        del g
    # a crafted map between guard words: order entries outside [0, nnz_coo) are skipped, runs that leave [0, nnz_coo] are clamped, and nothing
    # outside `out` is written (the reads stay inside order / val: a stray one would fault, not pass)
    tag, m, n, row, col, val = cases[1]
    drow, dcol, dval = dev(torch, row), dev(torch, col), dev(torch, val)
    rp, ci, v, order, start = spmv_acc_amd.coo_to_csr(m, n, drow, dcol, dval, want_map=True)
    nnz, k, pad = ci.numel(), row.size, 64
    h_order, h_start = order.cpu().numpy().copy(), start.cpu().numpy().copy()
    rng = np.random.default_rng(8)
    where = rng.choice(k, 300, replace=False)
    h_order[where] = np.concatenate([np.full(100, -1), np.full(100, k), rng.integers(k, 2 ** 31 - 1, 100)]).astype(np.int32)
    h_start[-1] = k + 1000          # the last run reaches past the triples
    h_start[-2] = k + 5
    h_start[0] = -4                 # the first starts before them
    h_start[nnz // 2] = 2 ** 31 - 1  # one in the middle is far outside: its run is empty, its predecessor's runs to the end
    buf = torch.full((nnz + 2 * pad,), 7.25, dtype=torch.float64, device="cuda")
    out = buf[pad:pad + nnz]
    spmv_acc_amd.coo_to_csr_values(dev(torch, h_order), dev(torch, h_start), dval, out)
    torch.cuda.synchronize()
    assert bool((buf[:pad] == 7.25).all()) and bool((buf[pad + nnz:] == 7.25).all())
    assert same_bits(out, coo_sum_model(h_order, h_start, val))
    assert hiplib.spmv_acc_last_error() == 0


def test_assembled_matrix_through_the_engine(torch_dev, oracle):
    torch = torch_dev
    row, col, val = synth.fem_quads_coo(60, 50, seed=21)
    quads = (61 * 51, 61 * 51) + synth.shuffle_coo(row, col, val, seed=22)
    rp, ci, _ = synth.random_csr(2500, 4000, 6, seed=102, kind="powerlaw")
    powerlaw = (2500, 4000) + split_into_duplicates(rp, ci, seed=23)
    for tag, (m, n, row, col, val) in (("quads", quads), ("powerlaw", powerlaw)):
        w_rp, w_ci, w_order, w_start = host_assemble(m, n, row, col)
        w_v = coo_sum_model(w_order, w_start, val)
        d_rp, d_ci, d_v = spmv_acc_amd.coo_to_csr(m, n, dev(torch, row), dev(torch, col), dev(torch, val))
        nnz = d_ci.numel()
        assert nnz == w_ci.size
        rng = np.random.default_rng(m + n)
        x, y0 = rng.standard_normal(n), rng.standard_normal(m)
        dx = dev(torch, x)
        for alpha, beta in ((1.0, 1.0), (0.5, -2.0)):
            ref = oracle.host_spmv(alpha, beta, w_rp, w_ci, w_v, x, y0)
            for strat in ("adaptive", "flat", "line_enhance"):
                dy = dev(torch, y0)
                spmv_acc_amd.csr_spmv(alpha, beta, m, n, nnz, d_rp, d_ci, d_v, dx, dy, strategy=strat)
                torch.cuda.synchronize()
                err = oracle.scaled_error(dy.cpu().numpy(), ref, alpha, beta, w_rp, w_ci, w_v, x, y0)
                print(f"{tag} {strat} alpha {alpha} beta {beta}: scaled error {err:.3e}")
                assert err <= SCALED_TOL, (tag, strat, alpha, beta, err)
        k = 5
        X, Y0 = rng.standard_normal((n, k)), rng.standard_normal((m, k))
        dX, dY = dev(torch, X), dev(torch, Y0)
        spmv_acc_amd.csr_spmm(0.5, -2.0, m, n, nnz, d_rp, d_ci, d_v, dX, dY)
        torch.cuda.synchronize()
        got = dY.cpu().numpy()
        for j in range(k):
            xj, yj = np.ascontiguousarray(X[:, j]), np.ascontiguousarray(Y0[:, j])
            ref = oracle.host_spmv(0.5, -2.0, w_rp, w_ci, w_v, xj, yj)
            err = oracle.scaled_error(np.ascontiguousarray(got[:, j]), ref, 0.5, -2.0, w_rp, w_ci, w_v, xj, yj)
            assert err <= SCALED_TOL, (tag, "spmm", j, err)
        spmv_acc_amd.release_plans(d_rp)


def test_coo_contract(torch_dev, hiplib):
    torch = torch_dev
    m, n = 900, 700
    row, col, val = split_into_duplicates(*synth.random_csr(m, n, 5, seed=100, kind="uniform")[:2], seed=31)
    k = row.size
    w_rp, w_ci, w_order, w_start = host_assemble(m, n, row, col)
    w_v = coo_sum_model(w_order, w_start, val)
    nnz = w_ci.size
    dval = dev(torch, val)
    plans = hiplib.spmv_acc_cached_plans()
    a, av = hiplib.spmv_acc_coo_to_csr, hiplib.spmv_acc_coo_to_csr_values
    pad = 64
    o_rp = torch.full((m + 1 + pad,), -7, dtype=torch.int32, device="cuda")
    o_ci = torch.full((k + pad,), -7, dtype=torch.int32, device="cuda")
    o_v = torch.full((k + pad,), 7.25, dtype=torch.float64, device="cuda")
    o_or = torch.full((k + pad,), -7, dtype=torch.int32, device="cuda")
    o_st = torch.full((k + 1 + pad,), -7, dtype=torch.int32, device="cuda")
    h = ctypes.c_int(-5)

    def untouched():
        torch.cuda.synchronize()
        return (bool((o_rp == -7).all()) and bool((o_ci == -7).all()) and bool((o_v == 7.25).all()) and bool((o_or == -7).all())
                and bool((o_st == -7).all()) and h.value == -5)

    def call(mm, nn, kk, drow, dcol):
        rc = a(mm, nn, kk, ptr(drow), ptr(dcol), ptr(dval), ptr(o_rp), ptr(o_ci), ptr(o_v), ptr(o_or), ptr(o_st), ctypes.byref(h))
        msg = hiplib.spmv_acc_last_error_string().decode()
        code = hiplib.spmv_acc_last_error()
        hiplib.spmv_acc_clear_error()
        return rc, code, msg

    hiplib.spmv_acc_set_stream(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    # out-of-range rows, columns, and both: counted, reported, nothing written
    rng = np.random.default_rng(5)
    where = rng.choice(k, 12, replace=False)
    bad_row, bad_col = row.copy(), col.copy()
    bad_row[where[:7]] = np.array([m, m + 1, -1, 2 ** 31 - 1, -2 ** 31, m + 50, -9], dtype=np.int64).astype(np.int32)
    bad_col[where[5:]] = np.array([n, -1, n + 3, 2 ** 31 - 1, -2 ** 31, n, -5], dtype=np.int64).astype(np.int32)  # (two triples have both)
    for r_, c_, count in ((bad_row, col, 7), (row, bad_col, 7), (bad_row, bad_col, 12)):
        rc, code, msg = call(m, n, k, dev(torch, r_), dev(torch, c_))
        assert rc == 2 and code == 2 and f"{count} triples with a row outside" in msg, (rc, msg)
        assert untouched()
    with pytest.raises(spmv_acc_amd.SpmvAccError, match="12 triples"):
        spmv_acc_amd.coo_to_csr(m, n, dev(torch, bad_row), dev(torch, bad_col), dval)
    drow, dcol = dev(torch, row), dev(torch, col)
    # triples in a matrix without rows / columns; sizes beyond int32 block arithmetic (the first refused size: nothing is allocated or read)
    assert call(0, n, k, drow, dcol)[0] == 2 and call(m, 0, k, drow, dcol)[0] == 2 and untouched()
    big = 2 ** 31 - 2 ** 16
    assert call(m, n, big, drow, dcol)[0] == 4 and call(big, n, k, drow, dcol)[0] == 4 and call(m, big, k, drow, dcol)[0] == 4 and untouched()
    assert av(big, nnz, ptr(o_or), ptr(o_st), ptr(dval), ptr(o_v)) == 4 and av(k, k + 1, ptr(o_or), ptr(o_st), ptr(dval), ptr(o_v)) == 2
    hiplib.spmv_acc_clear_error()
    assert untouched()
    # no triples: rowptr zeroed, *h_nnz = 0, nothing else touched
    rc, code, msg = call(m, n, 0, None, None)
    torch.cuda.synchronize()
    assert rc == 0 and h.value == 0 and bool((o_rp[:m + 1] == 0).all()) and bool((o_rp[m + 1:] == -7).all())
    assert bool((o_ci == -7).all()) and bool((o_v == 7.25).all()) and bool((o_or == -7).all()) and bool((o_st == -7).all())
    e_rp, e_ci, e_v, e_or, e_st = spmv_acc_amd.coo_to_csr(3, 4, drow[:0], dcol[:0], dval[:0], want_map=True)
    assert e_rp.tolist() == [0, 0, 0, 0] and e_ci.numel() == 0 and e_v.numel() == 0 and e_or.numel() == 0 and e_st.tolist() == [0]
    spmv_acc_amd.coo_to_csr_values(e_or, e_st, dval[:0], e_v)
    # only the used prefixes are written
    o_rp.fill_(-7)
    h.value = -5
    rc, code, msg = call(m, n, k, drow, dcol)
    torch.cuda.synchronize()
    assert rc == 0 and h.value == nnz, (rc, msg)
    assert same(o_rp[:m + 1], w_rp) and bool((o_rp[m + 1:] == -7).all()) and same(o_ci[:nnz], w_ci) and bool((o_ci[nnz:] == -7).all())
    assert same_bits(o_v[:nnz], w_v) and bool((o_v[nnz:] == 7.25).all()) and same(o_or[:k], w_order) and bool((o_or[k:] == -7).all())
    assert same(o_st[:nnz + 1], w_start) and bool((o_st[nnz + 1:] == -7).all())
    # tunable deterministic = 1 changes no bit of either entry
    try:
        assert hiplib.spmv_acc_set_tunable(b"deterministic", 1) == 0
        d_rp, d_ci, d_v, d_or, d_st = spmv_acc_amd.coo_to_csr(m, n, drow, dcol, dval, want_map=True)
        assert same(d_rp, w_rp) and same(d_ci, w_ci) and same_bits(d_v, w_v) and same(d_or, w_order) and same(d_st, w_start)
        again = torch.zeros_like(d_v)
        spmv_acc_amd.coo_to_csr_values(d_or, d_st, dval, again)
        assert same_bits(again, w_v)
    finally:
        hiplib.spmv_acc_reset_tunables()
        hiplib.spmv_acc_clear_error()
    # inside a capture: the first entry enqueues nothing and says why, the second is captured
    for t in (o_rp, o_ci, o_or, o_st):
        t.fill_(-7)
    o_v.fill_(7.25)
    h.value = -5
    out = torch.zeros(nnz, dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            spmv_acc_amd.coo_to_csr_values(d_or, d_st, dval, out)
            hiplib.spmv_acc_set_stream(ctypes.c_void_p(s.cuda_stream))
            refused = call(m, n, k, drow, dcol)
    assert refused[0] == 2 and "capture" in refused[2], refused
    g.replay()
    torch.cuda.synchronize()
    assert same_bits(out, w_v) and untouched()
    del g
    # none of this made or touched a plan
    assert hiplib.spmv_acc_cached_plans() == plans


def test_coo_grid_stride_at_test_size(torch_dev, hiplib):
    """max_grid_blocks lowered to 64, the smallest cap the library honours (config.cpp max_grid_blocks(): a smaller value leaves the default in
    place): every kernel of the two entries has more than 64 workgroups of work here -- 30 001 rowptr entries (118 blocks of 256), about 300 000
    triples (the census' 1 024-triple blocks: 290; keys, heads, entries: 1 170) and 120 000 CSR entries (79 tiles of 1 536) -- and strides."""
    torch = torch_dev
    rng = np.random.default_rng(17)
    m = n = 30_000
    r, c = distinct_positions(m, n, 120_000, rng)
    reps = rng.integers(1, 5, size=r.size)
    reps[1234] = 5000  # a long run as well
    row, col = np.repeat(r, reps), np.repeat(c, reps)
    row, col, val = synth.shuffle_coo(row, col, rng.standard_normal(row.size), seed=18)
    assert row.size > 64 * 1024 * 4 and 120_000 > 64 * 1536
    w_rp, w_ci, w_order, w_start = host_assemble(m, n, row, col)
    w_v = coo_sum_model(w_order, w_start, val)
    drow, dcol, dval = dev(torch, row), dev(torch, col), dev(torch, val)
    try:
        assert hiplib.spmv_acc_set_tunable(b"max_grid_blocks", 64) == 0
        rp, ci, v, order, start = spmv_acc_amd.coo_to_csr(m, n, drow, dcol, dval, want_map=True)
        assert same(rp, w_rp) and same(ci, w_ci) and same(order, w_order) and same(start, w_start) and same_bits(v, w_v)
        out = torch.zeros_like(v)
        spmv_acc_amd.coo_to_csr_values(order, start, dval, out)
        assert same_bits(out, w_v)
    finally:
        hiplib.spmv_acc_reset_tunables()
