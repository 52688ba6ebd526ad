"""GPU suite (-m gpu) of the device CSR sparse add C = alpha * A + beta * B (spmv_acc_csr_add / csr_add, spmv_acc_csr_add_values /
csr_add_values): structure, map and values bit for bit against the definition restated in numpy (tests/test_csr_add_host.py host_csr_add), new
values, alpha and beta through the kept map (plain and from a replayed graph), non-finite, huge, subnormal and signed-zero values, the sum through
the tuned engine against the CPU oracle, and the contract of the two entries: rows that are not strictly ascending, out-of-range columns,
descending row pointers, un-rebased and inconsistent inputs, captures, no plan, the deterministic switch, crafted maps and grid striding.

The cases of the issue's table, with the sub-cases of `empties` and `one_by_one` as tags of their own (empty_a, empty_b, empty_both, no_rows;
one_by_one_both), so that each is a parametrised case.

No speed gate: the parent commit cannot do this job, so there is no figure to hold (tools/csr_add_bench.py measures)."""
import ctypes
import functools

import numpy as np
import pytest

import spmv_acc_amd
from spmv_acc_amd import synth
from test_coo_host import coo_sum_model, host_assemble
from test_csr_add_host import host_csr_add, host_csr_add_values, random_sorted_csr

pytestmark = pytest.mark.gpu

SCALED_TOL = 1e-12  # the project's gate (tests/test_gpu_transpose.py SCALED_TOL), here relative to (|alpha| |A| + |beta| |B|) |x|
SCALARS = ((1.0, 1.0), (0.5, -2.0), (0.0, 1.0), (-1.0, 0.0))
RANK_TILE, VALUES_TILE = 256, 1024  # kCsrAddRankTile, kCsrAddTile (tests/test_csr_add_host.py CSR_ADD_SIZE_RULES holds them to the source)


def csr_of_rows(m, rows, rng):
    """An m-row CSR from {row: sorted column array}; rows not named are empty."""
    lens = np.array([len(rows.get(r, ())) for r in range(m)], dtype=np.int64)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = np.concatenate([np.asarray(rows[r], dtype=np.int64) for r in range(m) if r in rows] + [np.zeros(0, np.int64)]).astype(np.int32)
    return rp, ci, rng.standard_normal(ci.size) * 10.0 ** rng.integers(-3, 4, ci.size)


def host_transpose(m, n, csr):
    rp, ci, v = csr
    order = np.argsort(ci, kind="stable")
    t_rp = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(ci, minlength=n), out=t_rp[1:])
    return t_rp, np.repeat(np.arange(m, dtype=np.int32), np.diff(rp))[order], v[order]


def sorted_picks(m, n, per_row, rng):
    """An m x n CSR with per_row distinct random columns in every row, ascending."""
    window = 6 * per_row
    ci = np.sort(np.argsort(rng.random((m, window)), axis=1)[:, :per_row], axis=1) + rng.integers(0, n - window, size=(m, 1))
    return np.arange(0, m * per_row + 1, per_row, dtype=np.int32), ci.reshape(-1).astype(np.int32), rng.standard_normal(m * per_row)


SPECIALS = np.array([np.nan, np.inf, -np.inf, 2.0 ** 600, -2.0 ** 600, 2.0 ** -1074, -2.0 ** -1074, 0.0, -0.0, 1.0, -3.5, 2.0 ** 1000])


def special_pair():
    """A and B (12 x 40) with half of each row shared; every special value sits on matched and on unmatched entries of both."""
    rng = np.random.default_rng(77)
    rows_a, rows_b = {}, {}
    for r in range(12):
        cols = rng.permutation(40)[:30]
        rows_a[r], rows_b[r] = np.sort(cols[:20]), np.sort(cols[10:])  # 10 only in A, 10 shared, 10 only in B
    A, B = csr_of_rows(12, rows_a, rng), csr_of_rows(12, rows_b, rng)
    for M, other in ((A, B), (B, A)):
        row = np.repeat(np.arange(12), np.diff(M[0]))
        matched = np.array([M[1][q] in other[1][other[0][row[q]]:other[0][row[q] + 1]] for q in range(M[1].size)])
        for sel in (matched, ~matched):
            idx = np.flatnonzero(sel)
            M[2][idx] = SPECIALS[(np.arange(idx.size) + 5 * (M is B)) % SPECIALS.size]
    return A, B


def _cases():
    rng = np.random.default_rng(2026)
    row, col, val = synth.fem_quads_coo(60, 50, seed=1)
    nodes = 61 * 51
    rp, ci, order, start = host_assemble(nodes, nodes, row, col)
    stiff = (rp, ci, coo_sum_model(order, start, val))
    mass = (rp.copy(), ci.copy(), coo_sum_model(order, start, synth.fem_quads_coo(60, 50, seed=2)[2]))
    yield "same_pattern", nodes, nodes, stiff, mass
    A = random_sorted_csr(3000, 3000, 30_000, rng)
    yield "a_plus_at", 3000, 3000, A, host_transpose(3000, 3000, A)
    even, odd = random_sorted_csr(500, 500, 5000, rng), random_sorted_csr(500, 500, 6000, rng)
    yield "disjoint", 500, 1000, (even[0], even[1] * 2, even[2]), (odd[0], odd[1] * 2 + 1, odd[2])
    # A + sigma I: rows 0, 3, 6, ... hold their diagonal entry, rows 1, 4, 7, ... do not, the others as drawn
    m = 2000
    base = random_sorted_csr(m, m, 20_000, rng)
    r = np.repeat(np.arange(m, dtype=np.int64), np.diff(base[0]))
    pos = np.setdiff1d(np.union1d(r * m + base[1], np.arange(0, m, 3, dtype=np.int64) * (m + 1)), np.arange(1, m, 3, dtype=np.int64) * (m + 1))
    srp = np.zeros(m + 1, dtype=np.int32)
    np.cumsum(np.bincount(pos // m, minlength=m), out=srp[1:])
    yield ("shift", m, m, (srp, (pos % m).astype(np.int32), rng.standard_normal(pos.size)),
           (np.arange(m + 1, dtype=np.int32), np.arange(m, dtype=np.int32), np.ones(m)))
    # hub rows: 200 000 against 3, 3 against 200 000, 150 000 against 150 000 with half shared; short rows behind them
    n = 400_000
    mix = rng.permutation(n)[:225_000]
    rows_a = {0: np.sort(rng.permutation(n)[:200_000]), 1: np.array([5, 70_000, n - 1]), 2: np.sort(mix[:150_000])}
    rows_b = {0: np.array([0, 123_456, n - 2]), 1: np.sort(rng.permutation(n)[:200_000]), 2: np.sort(mix[75_000:])}
    for r in range(3, 20):
        rows_a[r], rows_b[r] = np.sort(rng.permutation(50)[:int(rng.integers(0, 7))]), np.sort(rng.permutation(50)[:int(rng.integers(0, 7))])
    yield "hub_rows", 20, n, csr_of_rows(20, rows_a, rng), csr_of_rows(20, rows_b, rng)
    # A's first and last rows empty; rows 10 ... 19 of B empty; rows 12 ... 14 empty in both
    rows_a = {r: np.sort(rng.permutation(30)[:5]) for r in range(1, 39) if not 12 <= r <= 14}
    rows_b = {r: np.sort(rng.permutation(30)[:4]) for r in range(40) if not 10 <= r <= 19}
    A, B = csr_of_rows(40, rows_a, rng), csr_of_rows(40, rows_b, rng)
    none = (np.zeros(41, np.int32), np.zeros(0, np.int32), np.zeros(0))
    yield "empties", 40, 30, A, B
    yield "empty_a", 40, 30, none, B
    yield "empty_b", 40, 30, A, none
    yield "empty_both", 40, 30, none, none
    yield "no_rows", 0, 30, (np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0)), (np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    one = np.array([0, 1], np.int32), np.array([0], np.int32)
    yield "one_by_one", 1, 1, one + (np.array([-0.0]),), (np.zeros(2, np.int32), np.zeros(0, np.int32), np.zeros(0))
    yield "one_by_one_both", 1, 1, one + (np.array([-0.0]),), one + (np.array([0.0]),)
    n = 2_147_000_000
    yield ("wide", 3, n, csr_of_rows(3, {0: [0, 1, 5, n - 3, n - 1], 2: [7, n - 2]}, rng),
           csr_of_rows(3, {0: [1, 2, n - 2, n - 1], 1: [0, n - 1], 2: [n - 2]}, rng))
    yield "large", 200_000, 150_000, sorted_picks(200_000, 150_000, 4, rng), sorted_picks(200_000, 150_000, 4, rng)
    A, B = special_pair()
    yield "specials", 12, 40, A, B


@functools.lru_cache(maxsize=None)
def cases():
    """(tag, m, n, A, B) with A = (rowptr, colindex, value) and B likewise: the cases of the issue, made once and shared (nothing changes them)."""
    return {c[0]: c for c in _cases()}


TAGS = ("same_pattern", "a_plus_at", "disjoint", "shift", "hub_rows", "empties", "empty_a", "empty_b", "empty_both", "no_rows", "one_by_one",
        "one_by_one_both", "wide", "large")


@functools.lru_cache(maxsize=None)
def reference(tag):
    """(rowptr, colindex, ia, ib) of the host for a case of cases(), computed once; the values follow from the map (host_csr_add_values)."""
    _, m, n, A, B = cases()[tag]
    return host_csr_add(m, n, (A[0], A[1], None), (B[0], B[1], None))[:4]


def want_values(tag, alpha, beta, a_v=None, b_v=None):
    _, _, _, A, B = cases()[tag]
    _, _, ia, ib = reference(tag)
    return host_csr_add_values(ia, ib, A[2] if a_v is None else a_v, B[2] if b_v is None else b_v, alpha, beta)


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


def same_bits_or_nan(t, a):
    """bit-equal, except that any NaN matches any NaN (the payload of a produced NaN is the hardware's); the sign of a zero counts"""
    g, w = t.cpu().numpy(), np.ascontiguousarray(a)
    nan = np.isnan(w)
    return np.array_equal(np.isnan(g), nan) and np.array_equal(g[~nan].view(np.int64), w[~nan].view(np.int64))


def test_cases_are_what_they_claim():
    """(no GPU work: the shapes of the cases, so that a change of a generator cannot quietly stop crossing a branch)"""
    for tag in TAGS + ("specials",):
        _, m, n, A, B = cases()[tag]
        for M in (A, B):  # what the entry demands: rebased, every row strictly ascending, columns in range
            assert M[0][0] == 0 and M[0][m] == M[1].size == M[2].size and np.all(np.diff(M[0]) >= 0), tag
            inner = np.ones(M[1].size, dtype=bool)
            inner[M[0][:-1][np.diff(M[0]) > 0]] = False  # the first entry of every row
            assert np.all(np.diff(M[1].astype(np.int64))[inner[1:]] > 0) and (M[1].size == 0 or (M[1].min() >= 0 and M[1].max() < n)), tag
    sizes = {tag: (cases()[tag][3][1].size, cases()[tag][4][1].size, reference(tag)[1].size) for tag in TAGS}
    _, _, ia, ib = reference("same_pattern")
    assert sizes["same_pattern"][0] == sizes["same_pattern"][1] == sizes["same_pattern"][2] > 64 * RANK_TILE and np.all(ia >= 0) and np.all(ib >= 0)
    assert not np.array_equal(cases()["same_pattern"][3][2], cases()["same_pattern"][4][2])
    na, nb, nc = sizes["a_plus_at"]
    assert na == nb == 30_000 and na < nc < na + nb  # partial overlap
    _, _, _, A, B = cases()["disjoint"]
    _, _, ia, ib = reference("disjoint")
    assert np.all(A[1] % 2 == 0) and np.all(B[1] % 2 == 1) and sizes["disjoint"][2] == 11_000 and np.all((ia < 0) != (ib < 0))
    _, m, _, A, B = cases()["shift"]
    _, _, ia, ib = reference("shift")
    diag = ib >= 0
    assert int(diag.sum()) == m and (ia[diag] >= 0).sum() >= m // 3 and (ia[diag] < 0).sum() >= m // 3  # A holds some diagonal entries, lacks others
    _, _, _, A, B = cases()["hub_rows"]
    assert np.diff(A[0])[:3].tolist() == [200_000, 3, 150_000] and np.diff(B[0])[:3].tolist() == [3, 200_000, 150_000]
    rp = reference("hub_rows")[0]
    assert rp[3] - rp[2] == 225_000 and np.diff(A[0])[3:].max() < 7 and sizes["hub_rows"][2] > 600 * VALUES_TILE
    _, _, _, A, B = cases()["empties"]
    la, lb = np.diff(A[0]), np.diff(B[0])
    assert la[0] == 0 and la[-1] == 0 and np.all(lb[10:20] == 0) and np.all((la[12:15] == 0) & (lb[12:15] == 0)) and la[10] > 0 and lb[0] > 0
    assert sizes["empty_a"][:2] == (0, B[1].size) and sizes["empty_b"][:2] == (A[1].size, 0) and sizes["empty_both"] == (0, 0, 0)
    assert cases()["no_rows"][1] == 0 and reference("no_rows")[0].tolist() == [0]
    assert np.signbit(want_values("one_by_one", 1.0, 1.0)[0]) and sizes["one_by_one"] == (1, 0, 1)
    both = want_values("one_by_one_both", 1.0, 1.0)
    assert both.tolist() == [0.0] and not np.signbit(both[0]) and sizes["one_by_one_both"] == (1, 1, 1)
    _, _, n, A, B = cases()["wide"]
    assert n == 2_147_000_000 and A[1].min() == 0 and A[1].max() == n - 1 and B[1].max() == n - 1 and 0 < sizes["wide"][2] < A[1].size + B[1].size
    assert sizes["large"][:2] == (800_000, 800_000) and cases()["large"][1] + 1 > 64 * 256 and sizes["large"][2] > 64 * VALUES_TILE
    _, _, _, A, B = cases()["specials"]
    _, _, ia, ib = reference("specials")
    for M, mine, other in ((A, ia, ib), (B, ib, ia)):
        for sel in ((mine >= 0) & (other >= 0), (mine >= 0) & (other < 0)):  # every special on matched and on unmatched entries
            v = M[2][mine[sel]]
            assert np.isnan(v).any() and np.isposinf(v).any() and np.isneginf(v).any() and (v == 2.0 ** -1074).any() and (np.abs(v) == 2.0 ** 600).any()
            assert ((v == 0) & np.signbit(v)).any() and ((v == 0) & ~np.signbit(v)).any()


@pytest.mark.parametrize("tag", TAGS)
def test_sum_is_the_host_model(torch_dev, tag):
    torch = torch_dev
    _, m, n, A, B = cases()[tag]
    w_rp, w_ci, w_ia, w_ib = reference(tag)
    dA, dB = dev_csr(torch, A), dev_csr(torch, B)
    for alpha, beta in SCALARS:
        w_v = want_values(tag, alpha, beta)
        rp, ci, v, ia, ib = spmv_acc_amd.csr_add(m, n, *dA, *dB, alpha=alpha, beta=beta, want_map=True)
        assert ci.numel() == v.numel() == ia.numel() == ib.numel() == w_ci.size and rp.numel() == m + 1, tag  # *h_nnz
        assert same(rp, w_rp) and same(ci, w_ci) and same(ia, w_ia) and same(ib, w_ib), tag
        assert same_bits(v, w_v), (tag, alpha, beta)
        a_rp, a_ci, a_v = spmv_acc_amd.csr_add(m, n, *dA, *dB, alpha=alpha, beta=beta)  # no map: it lives in the workspace
        assert torch.equal(a_rp, rp) and torch.equal(a_ci, ci) and same_bits(a_v, w_v), (tag, alpha, beta)
    # structure only, without and with the map
    s_rp, s_ci, s_v = spmv_acc_amd.csr_add(m, n, dA[0], dA[1], None, dB[0], dB[1], None)
    assert s_v is None and same(s_rp, w_rp) and same(s_ci, w_ci), tag
    m_rp, m_ci, m_v, m_ia, m_ib = spmv_acc_amd.csr_add(m, n, dA[0], dA[1], None, dB[0], dB[1], None, alpha=3.0, beta=0.0, want_map=True)
    assert m_v is None and same(m_rp, w_rp) and same(m_ci, w_ci) and same(m_ia, w_ia) and same(m_ib, w_ib), tag


def test_values_follow_new_inputs(torch_dev, hiplib):
    torch = torch_dev
    for tag in ("same_pattern", "a_plus_at", "hub_rows", "one_by_one"):
        _, m, n, A, B = cases()[tag]
        dA, dB = dev_csr(torch, A), dev_csr(torch, B)
        rp, ci, v, ia, ib = spmv_acc_amd.csr_add(m, n, *dA, *dB, alpha=0.5, beta=-2.0, want_map=True)
        nnz = ci.numel()
        rng = np.random.default_rng(nnz)
        new_a, new_b = rng.standard_normal(A[2].size), rng.standard_normal(B[2].size)
        out = torch.full((nnz,), 7.25, dtype=torch.float64, device="cuda")
        spmv_acc_amd.csr_add_values(ia, ib, dA[2], dB[2], out, alpha=0.5, beta=-2.0)  # the same values repeat the first call's bits
        assert same_bits(out, want_values(tag, 0.5, -2.0)) and torch.equal(out.view(torch.int64), v.view(torch.int64)), tag
        for alpha, beta in ((1.0, 1.0), (0.0, 3.0), (-1.0 / 3.0, 1e-3)):  # new alpha and beta on the kept map
            out.fill_(7.25)
            spmv_acc_amd.csr_add_values(ia, ib, dA[2], dB[2], out, alpha=alpha, beta=beta)
            assert same_bits(out, want_values(tag, alpha, beta)), (tag, alpha, beta)
        da, db = dA[2].clone(), dB[2].clone()
        # captured into a graph (one stream, no parallel branches) and replayed on values edited in place between the replays: alpha and beta
        # stay as captured
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=s):
                spmv_acc_amd.csr_add_values(ia, ib, da, db, out, alpha=0.25, beta=3.0)
        for va, vb in ((new_a, B[2]), (A[2], new_b), (new_a, new_b), (A[2], B[2])):
            da.copy_(dev(torch, va))
            db.copy_(dev(torch, vb))
            out.fill_(7.25)
            spmv_acc_amd.csr_add_values(ia, ib, da, db, out, alpha=-1.5, beta=0.125)
            assert same_bits(out, want_values(tag, -1.5, 0.125, va, vb)), tag
            fresh = spmv_acc_amd.csr_add(m, n, dA[0], dA[1], da, dB[0], dB[1], db, alpha=-1.5, beta=0.125)[2]
            assert same_bits(fresh, want_values(tag, -1.5, 0.125, va, vb)), tag
            out.fill_(7.25)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert same_bits(out, want_values(tag, 0.25, 3.0, va, vb)), tag
        del g
    assert hiplib.spmv_acc_last_error() == 0


def test_special_values(torch_dev):
    torch = torch_dev
    _, m, n, A, B = cases()["specials"]
    w_rp, w_ci, w_ia, w_ib = reference("specials")
    dA, dB = dev_csr(torch, A), dev_csr(torch, B)
    scalars = (0.0, -1.0, 2.0 ** 500, 1.0, -0.0, 2.0 ** -600)
    out = None
    for alpha in scalars:
        for beta in scalars:
            w_v = want_values("specials", alpha, beta)
            rp, ci, v, ia, ib = spmv_acc_amd.csr_add(m, n, *dA, *dB, alpha=alpha, beta=beta, want_map=True)
            assert same(rp, w_rp) and same(ci, w_ci) and same(ia, w_ia) and same(ib, w_ib)
            assert same_bits_or_nan(v, w_v), (alpha, beta)  # the sign of every zero included: the definition fixes it
            out = torch.full_like(v, 7.25) if out is None else out.fill_(7.25)
            spmv_acc_amd.csr_add_values(ia, ib, dA[2], dB[2], out, alpha=alpha, beta=beta)
            assert same_bits_or_nan(out, w_v) and torch.equal(out.view(torch.int64), v.view(torch.int64)), (alpha, beta)
    w = want_values("specials", 0.0, 1.0)
    assert np.isnan(w[(w_ia >= 0) & (w_ib < 0)]).any()  # alpha == 0 is not special-cased: 0 * Inf = NaN on an A-only entry
    w = want_values("specials", 1.0, 1.0)
    assert np.signbit(w[(w == 0) & (w_ib < 0)]).any()    # ... and an A-only -0.0 stays -0.0


def scaled_sum_error(oracle, got, ref, A, B, alpha, beta, x):
    """max |got - ref| relative to (|alpha| |A| + |beta| |B|) |x|, row by row"""
    m = A[0].size - 1
    scale = (abs(alpha) * oracle.host_spmv(1.0, 0.0, A[0], A[1], np.abs(A[2]), np.abs(x), np.zeros(m)) +
             abs(beta) * oracle.host_spmv(1.0, 0.0, B[0], B[1], np.abs(B[2]), np.abs(x), np.zeros(m)))
    live = scale > 0
    assert np.all(got[~live] == ref[~live])
    return float(np.max(np.abs(got[live] - ref[live]) / scale[live])) if live.any() else 0.0


def test_sum_through_the_engine(torch_dev, oracle):
    torch = torch_dev
    alpha, beta = 0.5, -2.0
    for tag in ("same_pattern", "a_plus_at"):
        _, m, n, A, B = cases()[tag]
        dA, dB = dev_csr(torch, A), dev_csr(torch, B)
        c_rp, c_ci, c_v, ia, ib = spmv_acc_amd.csr_add(m, n, *dA, *dB, alpha=alpha, beta=beta, want_map=True)
        nnz = c_ci.numel()
        rng = np.random.default_rng(m + nnz)
        x = rng.standard_normal(n)
        dx = dev(torch, x)

        def reference_y(a_v, b_v, al, be):
            return (al * oracle.host_spmv(1.0, 0.0, A[0], A[1], a_v, x, np.zeros(m)) + be * oracle.host_spmv(1.0, 0.0, B[0], B[1], b_v, x, np.zeros(m)))

        for strat in ("adaptive", "flat"):
            dy = torch.zeros(m, dtype=torch.float64, device="cuda")
            spmv_acc_amd.csr_spmv(1.0, 0.0, m, n, nnz, c_rp, c_ci, c_v, dx, dy, strategy=strat)
            torch.cuda.synchronize()
            err = scaled_sum_error(oracle, dy.cpu().numpy(), reference_y(A[2], B[2], alpha, beta), A, B, alpha, beta, x)
            print(f"{tag} {strat}: C x against alpha A x + beta B x, scaled error {err:.3e}")
            # (rows of at most 18 + 18 terms: the summation bound, 2^-53 per term and operation, is two orders below the gate)
            assert err <= SCALED_TOL, (tag, strat, err)
        # the time step: new values of A and B and a new dt into C's value array in place, the plans told, the same SpMV again
        new_a, new_b, dt = rng.standard_normal(A[2].size), rng.standard_normal(B[2].size), 0.03125
        spmv_acc_amd.csr_add_values(ia, ib, dev(torch, new_a), dev(torch, new_b), c_v, alpha=1.0, beta=dt)
        spmv_acc_amd.refresh_values(c_rp)
        for strat in ("adaptive", "flat"):
            dy = torch.zeros(m, dtype=torch.float64, device="cuda")
            spmv_acc_amd.csr_spmv(1.0, 0.0, m, n, nnz, c_rp, c_ci, c_v, dx, dy, strategy=strat)
            torch.cuda.synchronize()
            err = scaled_sum_error(oracle, dy.cpu().numpy(), reference_y(new_a, new_b, 1.0, dt), (A[0], A[1], new_a), (B[0], B[1], new_b), 1.0, dt, x)
            print(f"{tag} {strat}: after new values, scaled error {err:.3e}")
            assert err <= SCALED_TOL, (tag, strat, err)
        spmv_acc_amd.release_plans(c_rp)


def test_csr_add_contract(torch_dev, hiplib):
    torch = torch_dev
    _, m, n, A, B = cases()["a_plus_at"]
    w_rp, w_ci, w_ia, w_ib = reference("a_plus_at")
    alpha, beta = 0.5, -2.0
    w_v = want_values("a_plus_at", alpha, beta)
    nnz, nnz_a, nnz_b = w_ci.size, A[1].size, B[1].size
    cap = nnz_a + nnz_b
    dA, dB = dev_csr(torch, A), dev_csr(torch, B)
    plans = hiplib.spmv_acc_cached_plans()
    add, values = hiplib.spmv_acc_csr_add, hiplib.spmv_acc_csr_add_values
    pad = 64
    o_rp = torch.full((m + 1 + pad,), -7, dtype=torch.int32, device="cuda")
    o_ci = torch.full((cap + pad,), -7, dtype=torch.int32, device="cuda")
    o_v = torch.full((cap + pad,), 7.25, dtype=torch.float64, device="cuda")
    o_ia = torch.full((cap + pad,), -7, dtype=torch.int32, device="cuda")
    o_ib = torch.full((cap + pad,), -7, dtype=torch.int32, device="cuda")
    h = ctypes.c_int(-5)

    def untouched():
        torch.cuda.synchronize()
        return (bool((o_rp == -7).all()) and bool((o_ci == -7).all()) and bool((o_v == 7.25).all()) and bool((o_ia == -7).all())
                and bool((o_ib == -7).all()) and h.value == -5)

    def report(rc):
        msg = hiplib.spmv_acc_last_error_string().decode()
        code = hiplib.spmv_acc_last_error()
        hiplib.spmv_acc_clear_error()
        return rc, code, msg

    def call(a=dA, b=dB, mm=m, nn=n, na=nnz_a, nb=nnz_b):
        return report(add(mm, nn, na, ptr(a[0]), ptr(a[1]), nb, ptr(b[0]), ptr(b[1]), alpha, ptr(a[2]), beta, ptr(b[2]), ptr(o_rp), ptr(o_ci),
                          ptr(o_v), ptr(o_ia), ptr(o_ib), ctypes.byref(h)))

    hiplib.spmv_acc_set_stream(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    # rows that are not strictly ascending, columns outside the shape, a descending row pointer -- in A, and in B: each counted and reported,
    # nothing written (the census runs before anything reads through an index)
    for which, M in (("A", A), ("B", B)):
        lens = np.diff(M[0])
        r = int(np.flatnonzero(lens >= 3)[5])  # a row with three entries or more
        q = int(M[0][r])
        unsorted = M[1].copy()
        unsorted[q], unsorted[q + 1] = M[1][q + 1], M[1][q]
        dup = M[1].copy()
        dup[q + 1] = dup[q]
        high = M[1].copy()
        high[M[0][r + 1] - 1] = n  # (the row's last entry: still ascending)
        low = M[1].copy()
        low[q] = -1                # (the row's first entry: still ascending)
        two = unsorted.copy()
        two[M[0][r + 1] - 1] = n
        for cols, a_, b_ in ((unsorted, 0, 1), (dup, 0, 1), (high, 1, 0), (low, 1, 0), (two, 1, 1)):
            bad = (dev(torch, M[0]), dev(torch, cols), dev(torch, M[2]))
            rc, code, msg = call(a=bad) if which == "A" else call(b=bad)
            assert rc == 2 and code == 2 and "spmv_acc_csr_add:" in msg and "nothing was written" in msg and "spmv_acc_coo_to_csr" in msg, (rc, msg)
            assert f"{which}: {a_} columns outside [0, n), {b_} positions not ascending inside a row, 0 rows with" in msg, msg
            other = "B" if which == "A" else "A"
            assert f"{other}: 0 columns outside [0, n), 0 positions not ascending inside a row, 0 rows with" in msg, msg
            assert untouched()
        desc = M[0].copy()
        desc[r] = M[0][r + 1] + 1  # row r descends (row r - 1 grows, inside the arrays)
        bad = (dev(torch, desc), dev(torch, M[1]), dev(torch, M[2]))
        rc, code, msg = call(a=bad) if which == "A" else call(b=bad)
        assert rc == 2 and code == 2 and "1 rows with a descending or out-of-range rowptr extent" in msg.split("; B: ")[which == "B"], (rc, msg)
        assert "nothing was written" in msg and untouched()
        with pytest.raises(spmv_acc_amd.SpmvAccError, match="1 positions not ascending"):
            bad = (dev(torch, M[0]), dev(torch, dup), dev(torch, M[2]))
            spmv_acc_amd.csr_add(m, n, *(bad if which == "A" else dA), *(bad if which == "B" else dB))
    # an un-rebased rowptr, a wrong nnz
    shifted_a, shifted_b = (dA[0] + 1, dA[1], dA[2]), (dB[0] + 1, dB[1], dB[2])
    assert call(a=shifted_a)[0] == 2 and call(b=shifted_b)[0] == 2 and untouched()
    for kw in (dict(na=nnz_a - 1), dict(na=nnz_a + 1), dict(nb=nnz_b - 1), dict(nb=nnz_b + 1), dict(na=0), dict(nb=0)):
        rc, code, msg = call(**kw)
        assert rc == 2 and "rowptr[m]" in msg and untouched(), (kw, rc, msg)
    # sizes beyond int32 block arithmetic: host-side, nothing is allocated or read
    big = 2 ** 31 - 2 ** 16
    assert call(mm=big)[0] == 4 and call(nn=big)[0] == 4 and call(na=big)[0] == 4 and call(nb=big)[0] == 4 and call(na=big // 2, nb=big // 2)[0] == 4
    assert untouched()
    # nothing to add: rowptr zeroed, *h_nnz = 0, nothing else touched
    zero_rp = torch.zeros(m + 1, dtype=torch.int32, device="cuda")
    for kw in (dict(a=(zero_rp, dA[1], dA[2]), b=(zero_rp, dB[1], dB[2]), na=0, nb=0), dict(a=(zero_rp, dA[1], dA[2]), b=(zero_rp, dB[1], dB[2]), na=-1, nb=-1),
               dict(mm=0, na=0, nb=0)):
        o_rp.fill_(-7)
        h.value = -5
        rc, code, msg = call(**kw)
        torch.cuda.synchronize()
        rows = kw.get("mm", m)
        assert rc == 0 and h.value == 0 and bool((o_rp[:rows + 1] == 0).all()) and bool((o_rp[rows + 1:] == -7).all()), (kw.keys(), rc, msg)
        assert bool((o_ci == -7).all()) and bool((o_v == 7.25).all()) and bool((o_ia == -7).all()) and bool((o_ib == -7).all())
    assert call(mm=0)[0] == 2  # ... and non-zeros without rows are refused
    # only the used prefixes are written; the sizes are read from the device with nnz < 0
    for kw in (dict(), dict(na=-1, nb=-1)):
        for t in (o_rp, o_ci, o_ia, o_ib):
            t.fill_(-7)
        o_v.fill_(7.25)
        h.value = -5
        assert untouched()
        rc, code, msg = call(**kw)
        torch.cuda.synchronize()
        assert rc == 0 and h.value == nnz, (rc, msg)
        assert same(o_rp[:m + 1], w_rp) and bool((o_rp[m + 1:] == -7).all()) and same(o_ci[:nnz], w_ci) and bool((o_ci[nnz:] == -7).all())
        assert same_bits(o_v[:nnz], w_v) and bool((o_v[nnz:] == 7.25).all()) and same(o_ia[:nnz], w_ia) and bool((o_ia[nnz:] == -7).all())
        assert same(o_ib[:nnz], w_ib) and bool((o_ib[nnz:] == -7).all())
    # two calls on the same inputs give identical bits
    first = spmv_acc_amd.csr_add(m, n, *dA, *dB, alpha=alpha, beta=beta, want_map=True)
    second = spmv_acc_amd.csr_add(m, n, *dA, *dB, alpha=alpha, beta=beta, want_map=True)
    assert all(torch.equal(x if x.dtype != torch.float64 else x.view(torch.int64), y if y.dtype != torch.float64 else y.view(torch.int64))
               for x, y in zip(first, second))
    # a crafted map: -1 and indices at or past the arrays' ends count as absent, both absent gives +0.0; nothing outside `out` is written
    c_ia, c_ib = w_ia.copy(), w_ib.copy()
    rng = np.random.default_rng(9)
    for arr, size in ((c_ia, nnz_a), (c_ib, nnz_b)):
        arr[rng.choice(nnz, 200, replace=False)] = np.array([-1, size, size + 7, 2 ** 31 - 1, -2 ** 31] * 40, dtype=np.int64).astype(np.int32)
    assert (((c_ia < 0) | (c_ia >= nnz_a)) & ((c_ib < 0) | (c_ib >= nnz_b))).any()
    buf = torch.full((nnz + 2 * pad,), 7.25, dtype=torch.float64, device="cuda")
    out = buf[pad:pad + nnz]
    spmv_acc_amd.csr_add_values(dev(torch, c_ia), dev(torch, c_ib), dA[2], dB[2], out, alpha=alpha, beta=beta)
    torch.cuda.synchronize()
    assert bool((buf[:pad] == 7.25).all()) and bool((buf[pad + nnz:] == 7.25).all())
    assert same_bits(out, host_csr_add_values(c_ia, c_ib, A[2], B[2], alpha, beta))
    # tunable deterministic = 1 changes no bit of either entry
    try:
        assert hiplib.spmv_acc_set_tunable(b"deterministic", 1) == 0
        d_rp, d_ci, d_v, d_ia, d_ib = spmv_acc_amd.csr_add(m, n, *dA, *dB, alpha=alpha, beta=beta, want_map=True)
        assert same(d_rp, w_rp) and same(d_ci, w_ci) and same_bits(d_v, w_v) and same(d_ia, w_ia) and same(d_ib, w_ib)
        again = torch.zeros_like(d_v)
        spmv_acc_amd.csr_add_values(d_ia, d_ib, dA[2], dB[2], again, alpha=alpha, beta=beta)
        assert same_bits(again, w_v)
    finally:
        hiplib.spmv_acc_reset_tunables()
        hiplib.spmv_acc_clear_error()
    # inside a capture: the first entry enqueues nothing and says why, the values entry is captured; the capture survives
    for t in (o_rp, o_ci, o_ia, o_ib):
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
            spmv_acc_amd.csr_add_values(d_ia, d_ib, dA[2], dB[2], out, alpha=alpha, beta=beta)
            hiplib.spmv_acc_set_stream(ctypes.c_void_p(s.cuda_stream))
            refused = call()
    assert refused[0] == 2 and "capture" in refused[2], refused
    g.replay()
    torch.cuda.synchronize()
    assert same_bits(out, w_v) and untouched()
    del g
    # none of this made or touched a plan
    assert hiplib.spmv_acc_cached_plans() == plans


def test_csr_add_grid_stride_at_test_size(torch_dev, hiplib):
    """max_grid_blocks lowered to 64, the smallest cap the library honours (config.cpp max_grid_blocks(): a smaller value leaves the default in
    place).  hub_rows strides in every pass over non-zeros and entries (350 000 non-zeros a side: 1 370 tiles of 256; 625 000 entries: 611 tiles
    of 1 024); same_pattern (27 000 non-zeros a side: 106 tiles) in the census, the match and the two place passes, not in the values pass (27
    tiles); large (200 001 rows: 782 workgroups) adds the row pointer pass and the census' row loop."""
    torch = torch_dev
    try:
        assert hiplib.spmv_acc_set_tunable(b"max_grid_blocks", 64) == 0
        for tag, values_stride, rows_stride in (("hub_rows", True, False), ("same_pattern", False, False), ("large", True, True)):
            _, m, n, A, B = cases()[tag]
            w_rp, w_ci, w_ia, w_ib = reference(tag)
            assert A[1].size + 1 > 64 * RANK_TILE and B[1].size > 64 * RANK_TILE  # census, match, A's places, B's places
            assert (w_ci.size > 64 * VALUES_TILE) == values_stride and (m + 1 > 64 * 256) == rows_stride
            dA, dB = dev_csr(torch, A), dev_csr(torch, B)
            rp, ci, v, ia, ib = spmv_acc_amd.csr_add(m, n, *dA, *dB, alpha=0.5, beta=-2.0, want_map=True)
            w_v = want_values(tag, 0.5, -2.0)
            assert same(rp, w_rp) and same(ci, w_ci) and same(ia, w_ia) and same(ib, w_ib) and same_bits(v, w_v), tag
            out = torch.zeros_like(v)
            spmv_acc_amd.csr_add_values(ia, ib, dA[2], dB[2], out, alpha=0.5, beta=-2.0)
            assert same_bits(out, w_v), tag
    finally:
        hiplib.spmv_acc_reset_tunables()
