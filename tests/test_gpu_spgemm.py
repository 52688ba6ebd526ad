"""GPU suite (-m gpu) of the device CSR SpGEMM C = A * B (spmv_acc_csr_spgemm_products / csr_spgemm_products, spmv_acc_csr_spgemm / csr_spgemm,
spmv_acc_csr_spgemm_values / csr_spgemm_values): structure, map and values bit for bit against the definition restated in numpy
(tests/test_spgemm_host.py host_spgemm), new factor values through the kept map (plain and from a replayed graph), the product through the tuned
engine against the CPU oracle, A^T A, and the contract of the three entries: out-of-range columns, un-rebased and inconsistent inputs, captures,
no plan, the deterministic switch, too-large counts and grid striding.

One case departs from the sizes it was first specified with: hub_row_of_B was to have 4 000 rows of A on a B row of 20 000 entries, which is
80 M products and an 80 M-entry C -- gigabytes of arrays and minutes of host sorting per run of the suite.  What the case crosses is a tile of
the expansion inside one row of B and product-parallel balance on it; B keeps its row of 20 000 entries (20 tiles per hit) and A keeps column 7
in every row, with 40 rows instead of 4 000: 800 k products, 782 tiles.

No speed gate: the parent commit cannot do this job, so there is no figure to hold (tools/spgemm_bench.py measures)."""
import ctypes
import functools

import numpy as np
import pytest

import spmv_acc_amd
from spmv_acc_amd import synth
from test_coo_host import LONG_RUN, coo_sum_model, host_assemble
from test_spgemm_host import host_spgemm, random_unsorted_csr

pytestmark = pytest.mark.gpu

SCALED_TOL = 1e-12  # the project's gate (tests/test_gpu_transpose.py SCALED_TOL), here relative to |A| |B| |x|


def fixed_rows_csr(m, n, per_row, rng):
    """An m x n CSR with per_row distinct random columns in every row, unsorted."""
    ci = np.argsort(rng.random((m, min(n, 4 * per_row + 8))), axis=1)[:, :per_row]  # distinct picks from a window of columns
    ci = (ci + rng.integers(0, n, size=(m, 1))) % n
    return np.arange(0, m * per_row + 1, per_row, dtype=np.int32), ci.reshape(-1).astype(np.int32), rng.standard_normal(m * per_row)


def csr_of_rows(rows, rng):
    """A CSR from a list of per-row column arrays, stored as given."""
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    ci = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows]) if rp[-1] else np.zeros(0, np.int32)
    return rp, ci, rng.standard_normal(ci.size) * 10.0 ** rng.integers(-3, 4, ci.size)


def _pairs():
    rng = np.random.default_rng(2025)
    row, col, val = synth.fem_quads_coo(60, 50, seed=1)
    nodes = 61 * 51
    rp, ci, order, start = host_assemble(nodes, nodes, row, col)
    quads = (rp, ci, coo_sum_model(order, start, val))
    yield "quads_squared", nodes, nodes, nodes, quads, quads
    yield ("rect_unsorted_dups", 300, 500, 200, random_unsorted_csr(300, 500, 3000, 0.05, rng), random_unsorted_csr(500, 200, 4000, 0.05, rng))
    # column 7 in every row of A, at a random place among two others; B's row 7 holds 20 000 entries, the other rows 3
    a_rows = [rng.permutation(np.concatenate([[7], rng.choice(np.delete(np.arange(50), 7), 2, replace=False)])) for _ in range(40)]
    b_rows = [rng.choice(30_000, 20_000 if r == 7 else 3, replace=False) for r in range(50)]
    yield "hub_row_of_B", 40, 50, 30_000, csr_of_rows(a_rows, rng), csr_of_rows(b_rows, rng)
    # every row of B holds column 9 (and one other): row 0 of A, 5 000 entries, gives a run of 5 000 at (0, 9); rows 1 and 2 give runs of exactly
    # kCooLongRun and kCooLongRun + 1; short rows beside them
    k = 5200
    b_rows = [rng.permutation([9, int(rng.integers(10, 60))]) for _ in range(k)]
    a_rows = [rng.permutation(k)[:5000], rng.permutation(k)[:LONG_RUN], rng.permutation(k)[:LONG_RUN + 1]] + [rng.permutation(k)[:int(c)] for c in rng.integers(0, 6, 9)]
    yield "long_runs", 12, k, 60, csr_of_rows(a_rows, rng), csr_of_rows(b_rows, rng)
    # A's first and last rows empty; rows 0 ... 9 of B empty, and A has entries in those columns
    a_rows = [[]] + [rng.choice(40, 5, replace=False) for _ in range(30)] + [[]]
    b_rows = [[] for _ in range(10)] + [rng.choice(25, 3, replace=False) for _ in range(30)]
    yield "empty_meets", 32, 40, 25, csr_of_rows(a_rows, rng), csr_of_rows(b_rows, rng)
    # ... and every entry of A meets an empty row: no product at all
    a_rows = [[]] + [rng.choice(10, 4, replace=False) for _ in range(30)] + [[]]
    yield "empty_meets_all", 32, 40, 25, csr_of_rows(a_rows, rng), csr_of_rows(b_rows, rng)
    one = np.array([0, 1], np.int32), np.array([0], np.int32)
    yield "one_by_one", 1, 1, 1, one + (np.array([-0.0]),), one + (np.array([3.0]),)
    yield "key_34_bits", 70_000, 70_000, 70_000, fixed_rows_csr(70_000, 70_000, 3, rng), fixed_rows_csr(70_000, 70_000, 3, rng)
    yield "large", 200_000, 150_000, 100_000, fixed_rows_csr(200_000, 150_000, 4, rng), fixed_rows_csr(150_000, 100_000, 4, rng)


@functools.lru_cache(maxsize=None)
def pairs():
    """(tag, m, k, n, A, B) with A = (rowptr, colindex, value) and B likewise: the cases of the issue, made once and shared (nothing changes them)."""
    return {c[0]: c for c in _pairs()}


TAGS = ("quads_squared", "rect_unsorted_dups", "hub_row_of_B", "long_runs", "empty_meets", "empty_meets_all", "one_by_one", "key_34_bits", "large")


@functools.lru_cache(maxsize=None)
def reference(tag):
    """(rowptr, colindex, pa, pb, start, value) of the host for a case of pairs(), computed once."""
    _, m, k, n, A, B = pairs()[tag]
    return host_spgemm(m, k, n, A, B)


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


def same_bits(t, a):
    return np.array_equal(t.cpu().numpy().view(np.int64), np.ascontiguousarray(a).view(np.int64))


def test_cases_are_what_they_claim():
    """(no GPU work: the shapes of the cases, so that a change of a generator cannot quietly stop crossing a branch)"""
    runs = {tag: np.diff(reference(tag)[4]) for tag in TAGS}
    assert set(runs["quads_squared"].tolist()) == {1, 2, 3, 4, 6, 9} and 200_000 < runs["quads_squared"].sum() < 300_000
    _, _, _, _, A, B = pairs()["rect_unsorted_dups"]
    assert any(np.any(np.diff(A[1][A[0][r]:A[0][r + 1]]) < 0) for r in range(300)) and A[1].size == 3150 and B[1].size == 4200
    _, _, _, _, A, B = pairs()["hub_row_of_B"]
    assert np.all(np.bincount(np.repeat(np.arange(40), 3)[A[1] == 7], minlength=40) == 1) and np.diff(B[0]).tolist() == [3] * 7 + [20_000] + [3] * 42
    lr = runs["long_runs"]
    assert LONG_RUN in lr.tolist() and LONG_RUN + 1 in lr.tolist() and 5000 in lr.tolist()
    rp = reference("empty_meets")[0]
    assert rp[1] == 0 and rp[-1] == rp[-2] and 0 < runs["empty_meets"].sum() < 150 * 3
    assert runs["empty_meets_all"].size == 0 and reference("empty_meets_all")[0].tolist() == [0] * 33
    assert runs["one_by_one"].tolist() == [1] and np.signbit(reference("one_by_one")[5][0])
    assert runs["key_34_bits"].sum() == 9 * 70_000 and runs["large"].sum() == 3_200_000


@pytest.mark.parametrize("tag", TAGS)
def test_product_is_the_host_model(torch_dev, tag):
    torch = torch_dev
    _, m, k, n, A, B = pairs()[tag]
    w_rp, w_ci, w_pa, w_pb, w_start, w_v = reference(tag)
    dA, dB = dev_csr(torch, A), dev_csr(torch, B)
    assert spmv_acc_amd.csr_spgemm_products(m, k, dA[0], dA[1], dB[0]) == w_pa.size
    rp, ci, v, pa, pb, start = spmv_acc_amd.csr_spgemm(m, k, n, *dA, *dB, want_map=True)
    assert ci.numel() == w_ci.size and v.numel() == w_ci.size and start.numel() == w_ci.size + 1 and pa.numel() == pb.numel() == w_pa.size  # *h_nnz
    assert same(rp, w_rp) and same(ci, w_ci) and same(pa, w_pa) and same(pb, w_pb) and same(start, w_start), tag
    assert same_bits(v, w_v), tag
    # structure only; no map; called twice: the same arrays
    s_rp, s_ci, s_v = spmv_acc_amd.csr_spgemm(m, k, n, dA[0], dA[1], None, dB[0], dB[1], None)
    assert s_v is None and torch.equal(s_rp, rp) and torch.equal(s_ci, ci), tag
    m_rp, m_ci, m_v, m_pa, m_pb, m_start = spmv_acc_amd.csr_spgemm(m, k, n, dA[0], dA[1], None, dB[0], dB[1], None, want_map=True)
    assert m_v is None and torch.equal(m_rp, rp) and torch.equal(m_ci, ci) and torch.equal(m_pa, pa) and torch.equal(m_pb, pb) and torch.equal(m_start, start)
    a_rp, a_ci, a_v = spmv_acc_amd.csr_spgemm(m, k, n, *dA, *dB)
    assert torch.equal(a_rp, rp) and torch.equal(a_ci, ci) and same_bits(a_v, w_v), tag
    b_rp, b_ci, b_v, b_pa, b_pb, b_start = spmv_acc_amd.csr_spgemm(m, k, n, *dA, *dB, want_map=True)
    assert torch.equal(b_rp, rp) and torch.equal(b_ci, ci) and same_bits(b_v, w_v) and torch.equal(b_pa, pa) and torch.equal(b_pb, pb)
    assert torch.equal(b_start, start), tag


def test_values_follow_new_factors(torch_dev, hiplib):
    torch = torch_dev
    for tag in ("quads_squared", "rect_unsorted_dups", "long_runs", "one_by_one"):
        _, m, k, n, A, B = pairs()[tag]
        w_start, w_v = reference(tag)[4:]
        dA, dB = dev_csr(torch, A), dev_csr(torch, B)
        rp, ci, v, pa, pb, start = spmv_acc_amd.csr_spgemm(m, k, n, *dA, *dB, want_map=True)
        nnz = ci.numel()
        h_pa, h_pb = pa.cpu().numpy(), pb.cpu().numpy()
        ident = np.arange(h_pa.size, dtype=np.int32)
        rng = np.random.default_rng(nnz)
        new_a, new_b = rng.standard_normal(A[2].size), rng.standard_normal(B[2].size)
        out = torch.full((nnz,), 7.25, dtype=torch.float64, device="cuda")
        spmv_acc_amd.csr_spgemm_values(pa, pb, start, dA[2], dB[2], out)  # the same values repeat the first call's bits
        assert same_bits(out, w_v) and torch.equal(out.view(torch.int64), v.view(torch.int64)), tag
        da, db = dA[2].clone(), dB[2].clone()
        # captured into a graph (one stream, no parallel branches) and replayed on factors edited in place between the replays
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=s):
                spmv_acc_amd.csr_spgemm_values(pa, pb, start, da, db, out)
        for va, vb in ((new_a, B[2]), (A[2], new_b), (new_a, new_b), (A[2], B[2])):
            want = coo_sum_model(ident, w_start, va[h_pa] * vb[h_pb])
            da.copy_(dev(torch, va))
            db.copy_(dev(torch, vb))
            out.fill_(7.25)
            spmv_acc_amd.csr_spgemm_values(pa, pb, start, da, db, out)
            assert same_bits(out, want), tag
            fresh = spmv_acc_amd.csr_spgemm(m, k, n, dA[0], dA[1], da, dB[0], dB[1], db)[2]
            assert same_bits(fresh, want), tag
            out.fill_(7.25)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert same_bits(out, want), tag
        del g
    # a crafted start between guard words: runs that leave [0, nprod] are clamped, and nothing outside `out` is written
    _, m, k, n, A, B = pairs()["long_runs"]
    dA, dB = dev_csr(torch, A), dev_csr(torch, B)
    rp, ci, v, pa, pb, start = spmv_acc_amd.csr_spgemm(m, k, n, *dA, *dB, want_map=True)
    nnz, nprod, pad = ci.numel(), pa.numel(), 64
    h_start = start.cpu().numpy().copy()
    h_start[-1] = nprod + 1000        # the last run reaches past the products
    h_start[0] = -4                   # the first starts before them
    h_start[nnz // 2] = 2 ** 31 - 1   # one in the middle is far outside: its run is empty, its predecessor's runs to the end
    buf = torch.full((nnz + 2 * pad,), 7.25, dtype=torch.float64, device="cuda")
    out = buf[pad:pad + nnz]
    spmv_acc_amd.csr_spgemm_values(pa, pb, dev(torch, h_start), dA[2], dB[2], out)
    torch.cuda.synchronize()
    assert bool((buf[:pad] == 7.25).all()) and bool((buf[pad + nnz:] == 7.25).all())
    assert same_bits(out, coo_sum_model(np.arange(nprod, dtype=np.int32), h_start, A[2][pa.cpu().numpy()] * B[2][pb.cpu().numpy()]))
    assert hiplib.spmv_acc_last_error() == 0


def scaled_product_error(oracle, got, ref, A, B, x):
    """max |got - ref| relative to |A| (|B| |x|), row by row"""
    inner = oracle.host_spmv(1.0, 0.0, B[0], B[1], np.abs(B[2]), np.abs(x), np.zeros(B[0].size - 1))
    scale = oracle.host_spmv(1.0, 0.0, A[0], A[1], np.abs(A[2]), inner, np.zeros(A[0].size - 1))
    live = scale > 0
    assert np.all(got[~live] == ref[~live])
    return float(np.max(np.abs(got[live] - ref[live]) / scale[live])) if live.any() else 0.0


def test_product_through_the_engine(torch_dev, oracle):
    torch = torch_dev
    for tag in ("quads_squared", "rect_unsorted_dups"):
        _, m, k, n, A, B = pairs()[tag]
        dA, dB = dev_csr(torch, A), dev_csr(torch, B)
        c_rp, c_ci, c_v = spmv_acc_amd.csr_spgemm(m, k, n, *dA, *dB)
        nnz = c_ci.numel()
        x = np.random.default_rng(m + n).standard_normal(n)
        ref = oracle.host_spmv(1.0, 0.0, A[0], A[1], A[2], oracle.host_spmv(1.0, 0.0, B[0], B[1], B[2], x, np.zeros(k)), np.zeros(m))
        dx = dev(torch, x)
        for strat in ("adaptive", "flat"):
            dy = torch.zeros(m, dtype=torch.float64, device="cuda")
            spmv_acc_amd.csr_spmv(1.0, 0.0, m, n, nnz, c_rp, c_ci, c_v, dx, dy, strategy=strat)
            torch.cuda.synchronize()
            err = scaled_product_error(oracle, dy.cpu().numpy(), ref, A, B, x)
            print(f"{tag} {strat}: C x against A (B x), scaled error {err:.3e}")
            # (the summation bound for these row lengths -- at most 81 terms of 2^-53 each -- is two orders below the gate)
            assert err <= SCALED_TOL, (tag, strat, err)
        spmv_acc_amd.release_plans(c_rp)
    # A^T A through csr_transpose + csr_spgemm: a symmetric pattern, and value[i, j] == value[j, i] within the gate relative to (|A^T| |A|)[i, j]
    _, m, k, _, A, _ = pairs()["rect_unsorted_dups"]
    dA = dev_csr(torch, A)
    nnz_a = A[1].size
    dT = spmv_acc_amd.csr_transpose(m, k, nnz_a, *dA)
    g_rp, g_ci, g_v = spmv_acc_amd.csr_spgemm(k, m, k, *dT, *dA)
    _, _, scale = spmv_acc_amd.csr_spgemm(k, m, k, dT[0], dT[1], dT[2].abs(), dA[0], dA[1], dA[2].abs())
    t_rp, t_ci, t_v, perm = spmv_acc_amd.csr_transpose(k, k, g_ci.numel(), g_rp, g_ci, g_v, want_perm=True)
    assert torch.equal(t_rp, g_rp) and torch.equal(t_ci, g_ci) and g_ci.numel() > k
    asym = float(((g_v - t_v).abs() / scale).max().item())
    print(f"A^T A: largest |value[i, j] - value[j, i]| relative to (|A^T| |A|)[i, j]: {asym:.3e}")
    assert asym <= SCALED_TOL


def test_spgemm_contract(torch_dev, hiplib):
    torch = torch_dev
    _, m, k, n, A, B = pairs()["rect_unsorted_dups"]
    w_rp, w_ci, w_pa, w_pb, w_start, w_v = reference("rect_unsorted_dups")
    nprod, nnz, nnz_a, nnz_b = w_pa.size, w_ci.size, A[1].size, B[1].size
    dA, dB = dev_csr(torch, A), dev_csr(torch, B)
    plans = hiplib.spmv_acc_cached_plans()
    product, count, values = hiplib.spmv_acc_csr_spgemm, hiplib.spmv_acc_csr_spgemm_products, hiplib.spmv_acc_csr_spgemm_values
    pad = 64
    o_rp = torch.full((m + 1 + pad,), -7, dtype=torch.int32, device="cuda")
    o_ci = torch.full((nprod + pad,), -7, dtype=torch.int32, device="cuda")
    o_v = torch.full((nprod + pad,), 7.25, dtype=torch.float64, device="cuda")
    o_pa = torch.full((nprod + pad,), -7, dtype=torch.int32, device="cuda")
    o_pb = torch.full((nprod + pad,), -7, dtype=torch.int32, device="cuda")
    o_st = torch.full((nprod + 1 + pad,), -7, dtype=torch.int32, device="cuda")
    h = ctypes.c_int(-5)
    hp = ctypes.c_longlong(-5)

    def untouched():
        torch.cuda.synchronize()
        return (bool((o_rp == -7).all()) and bool((o_ci == -7).all()) and bool((o_v == 7.25).all()) and bool((o_pa == -7).all())
                and bool((o_pb == -7).all()) and bool((o_st == -7).all()) and h.value == -5)

    def report(rc):
        msg = hiplib.spmv_acc_last_error_string().decode()
        code = hiplib.spmv_acc_last_error()
        hiplib.spmv_acc_clear_error()
        return rc, code, msg

    def call(a=dA, b=dB, mm=m, kk=k, nn=n, na=nnz_a, nb=nnz_b, np_=nprod):
        return report(product(mm, kk, nn, na, ptr(a[0]), ptr(a[1]), ptr(a[2]), nb, ptr(b[0]), ptr(b[1]), ptr(b[2]), np_, ptr(o_rp), ptr(o_ci),
                              ptr(o_v), ptr(o_pa), ptr(o_pb), ptr(o_st), ctypes.byref(h)))

    def call_count(a=dA, b=dB, mm=m, kk=k, na=nnz_a):
        return report(count(mm, kk, na, ptr(a[0]), ptr(a[1]), ptr(b[0]), ctypes.byref(hp)))

    hiplib.spmv_acc_set_stream(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    # out-of-range columns in A, in B, and in both: counted, reported, nothing written (the census runs before anything reads through them)
    rng = np.random.default_rng(5)
    bad_a, bad_b = A[1].copy(), B[1].copy()
    bad_a[rng.choice(nnz_a, 7, replace=False)] = np.array([k, k + 1, -1, 2 ** 31 - 1, -2 ** 31, k + 50, -9], dtype=np.int64).astype(np.int32)
    bad_b[rng.choice(nnz_b, 5, replace=False)] = np.array([n, -1, n + 3, 2 ** 31 - 1, -2 ** 31], dtype=np.int64).astype(np.int32)
    dbad_a, dbad_b = (dA[0], dev(torch, bad_a), dA[2]), (dB[0], dev(torch, bad_b), dB[2])
    for a_, b_, ca, cb in ((dbad_a, dB, 7, 0), (dA, dbad_b, 0, 5), (dbad_a, dbad_b, 7, 5)):
        rc, code, msg = call(a=a_, b=b_)
        assert rc == 2 and code == 2 and f"{ca} columns of A outside" in msg and f"{cb} columns of B outside" in msg, (rc, msg)
        assert untouched()
    rc, code, msg = call_count(a=dbad_a)
    assert rc == 2 and "7 columns of A outside" in msg and hp.value == -5
    with pytest.raises(spmv_acc_amd.SpmvAccError, match="7 columns of A"):
        spmv_acc_amd.csr_spgemm(m, k, n, *dbad_a, *dB)
    # an un-rebased rowptr, a wrong nnz, a wrong nprod
    shifted_a, shifted_b = (dA[0] + 1, dA[1], dA[2]), (dB[0] + 1, dB[1], dB[2])
    assert call(a=shifted_a)[0] == 2 and call(b=shifted_b)[0] == 2 and call_count(a=shifted_a)[0] == 2 and call_count(b=shifted_b)[0] == 2
    assert call(na=nnz_a - 1)[0] == 2 and call(nb=nnz_b + 1)[0] == 2 and call_count(na=nnz_a + 1)[0] == 2 and untouched()
    for wrong in (nprod - 1, nprod + 1, 0):
        rc, code, msg = call(np_=wrong)
        assert rc == 2 and f"which is {nprod}" in msg and untouched(), (rc, msg)
    # sizes beyond int32 block arithmetic: host-side, nothing is allocated or read
    big = 2 ** 31 - 2 ** 16
    assert call(mm=big)[0] == 4 and call(kk=big)[0] == 4 and call(nn=big)[0] == 4 and call(na=big)[0] == 4 and call(nb=big)[0] == 4
    assert call(np_=big)[0] == 4 and call_count(mm=big)[0] == 4 and untouched() and hp.value == -5
    # ... and a product count past it from tiny arrays: one row of 50 000 entries of A, all in column 0, on a row 0 of B with 50 000 entries
    wide = 50_000
    hub_a = (dev(torch, np.array([0, wide], np.int32)), torch.zeros(wide, dtype=torch.int32, device="cuda"), torch.ones(wide, dtype=torch.float64, device="cuda"))
    hub_b = (dev(torch, np.array([0, wide], np.int32)), torch.arange(wide, dtype=torch.int32, device="cuda"), torch.ones(wide, dtype=torch.float64, device="cuda"))
    rc, code, msg = call_count(a=hub_a, b=hub_b, mm=1, kk=1, na=wide)
    assert rc == 4 and hp.value == wide * wide and str(wide * wide) in msg and "row ranges of A" in msg, (rc, msg, hp.value)
    rc, code, msg = call(a=hub_a, b=hub_b, mm=1, kk=1, nn=wide, na=wide, nb=wide, np_=wide)
    assert rc == 4 and str(wide * wide) in msg and "row ranges of A" in msg and untouched(), (rc, msg)
    with pytest.raises(spmv_acc_amd.SpmvAccError, match=str(wide * wide)):
        spmv_acc_amd.csr_spgemm_products(1, 1, hub_a[0], hub_a[1], hub_b[0])
    # the counts: read from the device with nnz < 0
    hp.value = -5
    assert call_count(na=-1)[0] == 0 and hp.value == nprod
    # no products: rowptr zeroed, *h_nnz = 0, nothing else touched -- without non-zeros, and where A only meets empty rows of B
    _, em, ek, en, eA, eB = pairs()["empty_meets_all"]
    dEa, dEb = dev_csr(torch, eA), dev_csr(torch, eB)
    none_a = (torch.zeros(m + 1, dtype=torch.int32, device="cuda"), dA[1], dA[2])  # (nnz_a = 0: the arrays are not read)
    for kw in (dict(a=dEa, b=dEb, mm=em, kk=ek, nn=en, na=eA[1].size, nb=eB[1].size, np_=0), dict(a=none_a, na=0, np_=0), dict(mm=0, na=0, np_=0)):
        o_rp.fill_(-7)
        h.value = -5
        rc, code, msg = call(**kw)
        torch.cuda.synchronize()
        rows = kw.get("mm", m)
        assert rc == 0 and h.value == 0 and bool((o_rp[:rows + 1] == 0).all()) and bool((o_rp[rows + 1:] == -7).all()), (kw.keys(), rc, msg)
        assert bool((o_ci == -7).all()) and bool((o_v == 7.25).all()) and bool((o_pa == -7).all()) and bool((o_pb == -7).all()) and bool((o_st == -7).all())
    assert call(a=dEa, b=dEb, mm=em, kk=ek, nn=en, na=eA[1].size, nb=eB[1].size, np_=3)[0] == 2  # ... and an nprod that is not 0 is refused
    e_rp, e_ci, e_v, e_pa, e_pb, e_st = spmv_acc_amd.csr_spgemm(em, ek, en, *dEa, *dEb, want_map=True)
    assert e_rp.tolist() == [0] * (em + 1) and e_ci.numel() == 0 and e_v.numel() == 0 and e_pa.numel() == 0 and e_pb.numel() == 0 and e_st.tolist() == [0]
    spmv_acc_amd.csr_spgemm_values(e_pa, e_pb, e_st, dEa[2], dEb[2], e_v)
    assert values(nprod, nprod + 1, ptr(o_pa), ptr(o_pb), ptr(o_st), ptr(dA[2]), ptr(dB[2]), ptr(o_v)) == 2
    hiplib.spmv_acc_clear_error()
    # only the used prefixes are written
    o_rp.fill_(-7)
    h.value = -5
    assert untouched()
    rc, code, msg = call()
    torch.cuda.synchronize()
    assert rc == 0 and h.value == nnz, (rc, msg)
    assert same(o_rp[:m + 1], w_rp) and bool((o_rp[m + 1:] == -7).all()) and same(o_ci[:nnz], w_ci) and bool((o_ci[nnz:] == -7).all())
    assert same_bits(o_v[:nnz], w_v) and bool((o_v[nnz:] == 7.25).all()) and same(o_pa[:nprod], w_pa) and bool((o_pa[nprod:] == -7).all())
    assert same(o_pb[:nprod], w_pb) and bool((o_pb[nprod:] == -7).all()) and same(o_st[:nnz + 1], w_start) and bool((o_st[nnz + 1:] == -7).all())
    # tunable deterministic = 1 changes no bit of any entry
    try:
        assert hiplib.spmv_acc_set_tunable(b"deterministic", 1) == 0
        assert spmv_acc_amd.csr_spgemm_products(m, k, dA[0], dA[1], dB[0]) == nprod
        d_rp, d_ci, d_v, d_pa, d_pb, d_st = spmv_acc_amd.csr_spgemm(m, k, n, *dA, *dB, want_map=True)
        assert same(d_rp, w_rp) and same(d_ci, w_ci) and same_bits(d_v, w_v) and same(d_pa, w_pa) and same(d_pb, w_pb) and same(d_st, w_start)
        again = torch.zeros_like(d_v)
        spmv_acc_amd.csr_spgemm_values(d_pa, d_pb, d_st, dA[2], dB[2], again)
        assert same_bits(again, w_v)
    finally:
        hiplib.spmv_acc_reset_tunables()
        hiplib.spmv_acc_clear_error()
    # inside a capture: the main entry and the count entry enqueue nothing and say why, the values entry is captured; the capture survives
    for t in (o_rp, o_ci, o_pa, o_pb, o_st):
        t.fill_(-7)
    o_v.fill_(7.25)
    h.value = -5
    hp.value = -5
    out = torch.zeros(nnz, dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            spmv_acc_amd.csr_spgemm_values(d_pa, d_pb, d_st, dA[2], dB[2], out)
            hiplib.spmv_acc_set_stream(ctypes.c_void_p(s.cuda_stream))
            refused = call()
            refused_count = call_count()
    assert refused[0] == 2 and "capture" in refused[2], refused
    assert refused_count[0] == 2 and "capture" in refused_count[2] and hp.value == -5, refused_count
    g.replay()
    torch.cuda.synchronize()
    assert same_bits(out, w_v) and untouched()
    del g
    # none of this made or touched a plan
    assert hiplib.spmv_acc_cached_plans() == plans


def test_spgemm_grid_stride_at_test_size(torch_dev, hiplib):
    """max_grid_blocks lowered to 64, the smallest cap the library honours (config.cpp max_grid_blocks(): a smaller value leaves the default in
    place): quads_squared has about 250 000 products (245 tiles of the expansion, 980 blocks of the map pass) and 75 000 entries of C (73 tiles of
    the values pass); hub_row_of_B 800 000 products (782 tiles) and as many entries.  Only quads_squared's 27 000 non-zeros of A exceed 64
    blocks of the count pass (106)."""
    torch = torch_dev
    try:
        assert hiplib.spmv_acc_set_tunable(b"max_grid_blocks", 64) == 0
        for tag in ("quads_squared", "hub_row_of_B"):
            _, m, k, n, A, B = pairs()[tag]
            w_rp, w_ci, w_pa, w_pb, w_start, w_v = reference(tag)
            assert w_pa.size > 64 * 1024 and w_ci.size > 64 * 1024
            dA, dB = dev_csr(torch, A), dev_csr(torch, B)
            assert spmv_acc_amd.csr_spgemm_products(m, k, dA[0], dA[1], dB[0]) == w_pa.size
            rp, ci, v, pa, pb, start = spmv_acc_amd.csr_spgemm(m, k, n, *dA, *dB, want_map=True)
            assert same(rp, w_rp) and same(ci, w_ci) and same(pa, w_pa) and same(pb, w_pb) and same(start, w_start) and same_bits(v, w_v), tag
            out = torch.zeros_like(v)
            spmv_acc_amd.csr_spgemm_values(pa, pb, start, dA[2], dB[2], out)
            assert same_bits(out, w_v), tag
    finally:
        hiplib.spmv_acc_reset_tunables()
