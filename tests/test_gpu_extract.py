"""GPU suite (-m gpu) of the device CSR extraction C = A[rows, colmap] with a diagonal band (spmv_acc_csr_extract / csr_extract, csr_permute,
spmv_acc_csr_extract_values / csr_extract_values): structure, map and values bit for bit against the definition restated in numpy
(tests/test_extract_host.py host_csr_extract), new values through the kept map (plain and from a replayed graph), non-finite, subnormal and
signed-zero values, a crafted map, the round trip L + D + U through csr_add, the permuted matrix through the tuned engine against the CPU oracle,
and the contract of the entries: rows and colmap values out of range or repeated, columns of candidates out of range, descending row extents,
un-rebased and inconsistent inputs, captures, and grid striding.

No speed gate: the parent commit cannot do this job, so there is no figure to hold (tools/extract_bench.py measures)."""
import ctypes
import functools

import numpy as np
import pytest

import spmv_acc_amd
from test_csr_add_host import dense_of, random_sorted_csr
from test_extract_host import INT_MAX, INT_MIN, host_csr_extract, host_csr_permute, shuffle_rows

pytestmark = pytest.mark.gpu

SCALED_TOL = 1e-12  # the project's gate (tests/test_gpu_transpose.py SCALED_TOL), here relative to |C| |x|, row by row
RANK_TILE, VALUES_TILE = 256, 2048  # kExtractRankTile, kExtractTile (tests/test_extract_host.py EXTRACT_SIZE_RULES holds them to the source)


def csr_of_rows(m, rows, rng):
    """An m-row CSR from {row: column array, in the order given}; rows not named are empty."""
    lens = np.array([len(rows.get(r, ())) for r in range(m)], dtype=np.int64)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = np.concatenate([np.asarray(rows[r], dtype=np.int64) for r in range(m) if r in rows] + [np.zeros(0, np.int64)]).astype(np.int32)
    return rp, ci, rng.standard_normal(ci.size) * 10.0 ** rng.integers(-3, 4, ci.size)


def grid_matrix(nx, ny, rng):
    """The 5-point stencil on an nx x ny grid: nx * ny rows, every row strictly ascending."""
    idx = np.arange(nx * ny).reshape(nx, ny)
    rows = {}
    for a in range(nx):
        for b in range(ny):
            nb = [idx[a, b]] + [idx[p, q] for p, q in ((a - 1, b), (a + 1, b), (a, b - 1), (a, b + 1)) if 0 <= p < nx and 0 <= q < ny]
            rows[int(idx[a, b])] = np.sort(nb)
    return csr_of_rows(nx * ny, rows, rng)


def sorted_picks(m, n, per_row, rng):
    """An m x n CSR with per_row distinct random columns in every row, ascending."""
    window = 6 * per_row
    ci = np.sort(np.argsort(rng.random((m, window)), axis=1)[:, :per_row], axis=1) + rng.integers(0, n - window, size=(m, 1))
    return np.arange(0, m * per_row + 1, per_row, dtype=np.int32), ci.reshape(-1).astype(np.int32), rng.standard_normal(m * per_row)


def inverse_of(perm, n):
    inv = np.full(n, -1, dtype=np.int32)
    inv[perm] = np.arange(perm.size, dtype=np.int32)
    return inv


def _cases():
    """(tag, m, n, A, keywords of csr_extract as numpy arrays / ints, perm or None: through csr_permute, mode: "full" | "structure_only" | "no_map")"""
    rng = np.random.default_rng(2027)
    A = random_sorted_csr(300, 400, 3000, rng)
    yield "identity", 300, 400, A, {}, None, "full"
    U = shuffle_rows(A, rng)
    yield "unsorted_in", 300, 400, U, {}, None, "full"
    rows = {r: rng.integers(0, 12, size=int(rng.integers(0, 30))) for r in range(50)}
    rows[7] = np.array([5, 3, 5, 5, 0, 3, 11, 0, 5])
    yield "repeats", 50, 12, csr_of_rows(50, rows, rng), {}, None, "full"
    sel_rows = np.sort(rng.permutation(300)[:120]).astype(np.int32)
    sel_cols = np.sort(rng.permutation(400)[:150])
    yield "sub_block", 300, 400, A, dict(rows=sel_rows, colmap=inverse_of(sel_cols, 400), nc=150), None, "full"
    yield "rows_shuffled", 300, 400, A, dict(rows=rng.permutation(300)[:200].astype(np.int32)), None, "full"
    G = grid_matrix(15, 20, rng)
    yield "permuted", 300, 300, G, {}, rng.permutation(300).astype(np.int32), "full"
    yield "embed", 300, 400, A, dict(colmap=(2 * np.arange(400) + 1).astype(np.int32), nc=805), None, "full"
    S = random_sorted_csr(250, 250, 4000, rng)
    yield "tril", 250, 250, S, dict(diag_hi=0), None, "full"
    yield "strict_triu", 250, 250, S, dict(diag_lo=1), None, "full"
    yield "diag", 250, 250, S, dict(diag_lo=0, diag_hi=0), None, "full"
    perm = rng.permutation(300).astype(np.int32)
    yield "band_after_map", 300, 300, G, dict(rows=perm, colmap=inverse_of(perm, 300), nc=300, diag_lo=-40, diag_hi=25), None, "full"
    yield "lo_above_hi", 250, 250, S, dict(diag_lo=3, diag_hi=2), None, "full"
    yield "all_dropped", 300, 400, A, dict(colmap=np.full(400, -1, np.int32), nc=7), None, "full"
    rows = {r: np.sort(rng.permutation(30)[:5]) for r in range(40) if r % 4 == 1}
    E = csr_of_rows(40, rows, rng)
    yield "empties", 40, 30, E, dict(rows=np.array([0, 2, 1, 3, 4, 9, 10, 11, 5, 39, 38], np.int32)), None, "full"
    yield "empties_only", 40, 30, E, dict(rows=np.array([0, 2, 3, 4, 38], np.int32)), None, "full"
    yield "no_rows", 300, 400, A, dict(rows=np.zeros(0, np.int32)), None, "full"
    yield "empty_a", 40, 30, (np.zeros(41, np.int32), np.zeros(0, np.int32), np.zeros(0)), dict(rows=np.array([3, 1], np.int32)), None, "full"
    yield "one_by_one", 1, 1, (np.array([0, 1], np.int32), np.array([0], np.int32), np.array([-0.0])), {}, None, "full"
    n = 40_000
    rows = {r: np.unique(rng.integers(0, n, size=int(rng.integers(0, 8)))) for r in range(n)}
    rows[7] = np.sort(rng.permutation(n)[:20_000])
    yield "hub_row", n, n, csr_of_rows(n, rows, rng), {}, rng.permutation(n).astype(np.int32), "full"
    yield "structure_only", 300, 400, U, dict(rows=rng.permutation(300)[:200].astype(np.int32)), None, "structure_only"
    yield "no_map", 300, 400, U, dict(rows=rng.permutation(300)[:200].astype(np.int32)), None, "no_map"
    yield "no_map_no_sort", 300, 400, A, dict(diag_lo=-50, diag_hi=60), None, "no_map"
    m = 200_000
    yield "large", m, m, sorted_picks(m, m, 4, rng), {}, rng.permutation(m).astype(np.int32), "full"
    Sp = random_sorted_csr(60, 60, 1200, rng)
    specials = np.array([np.nan, np.inf, -np.inf, 2.0 ** -1074, -2.0 ** -1074, 0.0, -0.0, 2.0 ** -1030, 1.0, -3.5])
    vals = specials[np.arange(1200) % specials.size].copy()
    vals.view(np.uint64)[::10] = 0x7FF8_0000_DEAD_BEEF  # a NaN with a payload
    yield "specials", 60, 60, (Sp[0], Sp[1], vals), {}, rng.permutation(60).astype(np.int32), "full"


@functools.lru_cache(maxsize=None)
def cases():
    """The cases of the issue, made once and shared (nothing changes them)."""
    return {c[0]: c for c in _cases()}


TAGS = ("identity", "unsorted_in", "repeats", "sub_block", "rows_shuffled", "permuted", "embed", "tril", "strict_triu", "diag", "band_after_map",
        "lo_above_hi", "all_dropped", "empties", "empties_only", "no_rows", "empty_a", "one_by_one", "hub_row", "structure_only", "no_map",
        "no_map_no_sort")


@functools.lru_cache(maxsize=None)
def reference(tag):
    """(rowptr, colindex, map) of the host for a case of cases(), computed once; the values follow from the map."""
    _, m, n, A, kw, perm, _ = cases()[tag]
    if perm is not None:
        return host_csr_permute(m, (A[0], A[1], None), perm)[:3]
    return host_csr_extract(m, n, (A[0], A[1], None), **kw)[:3]


def descents(tag):
    """the descents inside the rows of the COMPACTION of a case (A's order, before any sort): what selects the sort path"""
    _, m, n, A, kw, perm, _ = cases()[tag]
    if perm is not None:
        kw = dict(rows=perm, colmap=inverse_of(perm, m), nc=m)
    rp, _, cmap = reference(tag)
    colmap = kw.get("colmap")
    total = 0
    row = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    order = np.lexsort((cmap, row))  # ascending position of A inside every row of C
    col = A[1][cmap[order]] if colmap is None else colmap[A[1][cmap[order]]]
    inner = np.ones(col.size, dtype=bool)
    inner[rp[:-1][np.diff(rp) > 0]] = False
    if col.size > 1:
        total = int(np.sum((np.diff(col.astype(np.int64)) < 0) & inner[1:]))
    return total


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
    return np.array_equal(t.cpu().numpy().view(np.uint64), np.ascontiguousarray(a, dtype=np.float64).view(np.uint64))


def run_case(torch, tag, value="own", want_map=True):
    """csr_extract / csr_permute on a case; value: "own" (the case's), None (structure only) or a device tensor"""
    _, m, n, A, kw, perm, _ = cases()[tag]
    d_rp, d_ci, d_v = dev_csr(torch, A)
    v = d_v if isinstance(value, str) else value
    if perm is not None:
        return spmv_acc_amd.csr_permute(m, d_rp, d_ci, v, dev(torch, perm), want_map=want_map)
    args = {k: (dev(torch, a) if isinstance(a, np.ndarray) else a) for k, a in kw.items()}
    return spmv_acc_amd.csr_extract(m, n, d_rp, d_ci, v, want_map=want_map, **args)


def test_cases_are_what_they_claim():
    """(no GPU work: the shapes of the cases, so that a change of a generator cannot quietly stop crossing a branch)"""
    def strictly_ascending(rp, ci):
        inner = np.ones(ci.size, dtype=bool)
        inner[rp[:-1][np.diff(rp) > 0]] = False
        return ci.size < 2 or bool(np.all(np.diff(ci.astype(np.int64))[inner[1:]] > 0))

    for tag in TAGS + ("large", "specials"):
        _, m, n, A, kw, perm, mode = cases()[tag]
        assert A[0][0] == 0 and A[0][m] == A[1].size == A[2].size and np.all(np.diff(A[0]) >= 0), tag
        assert A[1].size == 0 or (A[1].min() >= 0 and A[1].max() < n), tag
        rp, ci, cmap = reference(tag)
        if tag != "repeats":
            assert strictly_ascending(rp, ci), tag  # C has strictly ascending rows exactly when the selected rows repeat no column
    sort_path = {tag for tag in TAGS + ("large", "specials") if descents(tag) > 0}
    assert sort_path == {"unsorted_in", "repeats", "permuted", "band_after_map", "hub_row", "structure_only", "no_map", "large", "specials"}, sort_path
    _, m, n, A, _, _, _ = cases()["identity"]
    rp, ci, cmap = reference("identity")
    assert np.array_equal(rp, A[0]) and np.array_equal(ci, A[1]) and np.array_equal(cmap, np.arange(A[1].size))
    _, _, _, U, _, _, _ = cases()["unsorted_in"]
    assert not strictly_ascending(U[0], U[1]) and np.array_equal(reference("unsorted_in")[1], A[1])  # the shuffled rows come back sorted
    _, _, _, R, _, _, _ = cases()["repeats"]
    rp, ci, cmap = reference("repeats")
    row7 = slice(rp[7], rp[8])
    assert ci[row7].tolist() == [0, 0, 3, 3, 5, 5, 5, 5, 11] and (cmap[row7] - R[0][7]).tolist() == [4, 7, 1, 5, 0, 2, 3, 8, 6]  # ties in A's order
    assert not strictly_ascending(rp, ci)
    _, _, _, _, kw, _, _ = cases()["sub_block"]
    kept = kw["colmap"][kw["colmap"] >= 0]
    assert np.all(np.diff(kw["rows"]) > 0) and np.all(np.diff(kept) > 0) and kw["rows"].size == 120 != kw["nc"] == 150 and 0 < reference("sub_block")[1].size
    _, _, _, _, kw, _, _ = cases()["rows_shuffled"]
    assert "colmap" not in kw and np.any(np.diff(kw["rows"]) < 0)
    _, m, _, G, _, perm, _ = cases()["permuted"]
    assert m == 300 and np.array_equal(np.sort(perm), np.arange(300)) and np.all(np.diff(G[0]) <= 5) and np.all(np.diff(G[0]) >= 3)
    rp, ci, cmap = reference("permuted")
    D = dense_of(300, 300, G)
    assert np.array_equal(dense_of(300, 300, (rp, ci, G[2][cmap])), D[perm][:, perm])
    _, _, n, _, kw, _, _ = cases()["embed"]
    assert kw["nc"] > 2 * n and reference("embed")[1].max() > n
    _, _, _, S, _, _, _ = cases()["tril"]
    srow = np.repeat(np.arange(250), np.diff(S[0]))
    for tag, sel in (("tril", S[1] <= srow), ("strict_triu", S[1] > srow), ("diag", S[1] == srow)):
        assert np.array_equal(reference(tag)[2], np.flatnonzero(sel)) and 0 < int(sel.sum()) < S[1].size, tag
    assert reference("diag")[1].size < 8 * 64  # fewer than one wavefront's chunk of the values pass
    _, _, _, G, kw, _, _ = cases()["band_after_map"]
    rp, ci, cmap = reference("band_after_map")
    crow = np.repeat(np.arange(300), np.diff(rp))
    arow = np.repeat(np.arange(300), np.diff(G[0]))
    assert np.all((ci - crow >= -40) & (ci - crow <= 25)) and 0 < ci.size < G[1].size
    d_in_a = G[1].astype(np.int64) - arow
    assert np.all((d_in_a >= -40) & (d_in_a <= 25))  # in A's own indices the band would keep every entry, and entries are dropped: the band is C's
    for tag in ("lo_above_hi", "all_dropped", "empties_only", "no_rows", "empty_a"):
        rp, ci, cmap = reference(tag)
        assert ci.size == 0 and not rp.any(), tag
    assert cases()["lo_above_hi"][4]["diag_lo"] > cases()["lo_above_hi"][4]["diag_hi"] and np.all(cases()["all_dropped"][4]["colmap"] < 0)
    _, _, _, E, kw, _, _ = cases()["empties"]
    lens = np.diff(E[0])[kw["rows"]]
    assert lens[0] == 0 and lens[-1] == 0 and np.any(lens[1:-1] == 0) and np.any(lens > 0) and np.all(np.diff(E[0])[cases()["empties_only"][4]["rows"]] == 0)
    assert cases()["no_rows"][4]["rows"].size == 0 and cases()["empty_a"][3][1].size == 0 and reference("no_rows")[0].tolist() == [0]
    assert reference("one_by_one")[1].tolist() == [0] and np.signbit(cases()["one_by_one"][3][2][0])
    _, _, _, H, _, perm, _ = cases()["hub_row"]
    rp, ci, cmap = reference("hub_row")
    assert np.diff(H[0])[7] == 20_000 and np.delete(np.diff(H[0]), 7).max() < 8 and np.diff(rp).max() == 20_000
    assert 20_000 > 64 * 64 and 20_000 > 2 * VALUES_TILE and ci.size > 50 * VALUES_TILE  # wavefronts and values tiles inside the one row; several tiles
    assert cases()["structure_only"][6] == "structure_only" and cases()["no_map"][6] == "no_map" and cases()["no_map_no_sort"][6] == "no_map"
    _, m, _, L, _, _, _ = cases()["large"]
    assert m == 200_000 and L[1].size == 800_000 and L[1].size % RANK_TILE == 0  # the closing element of the candidates opens a tile of its own
    v = cases()["specials"][3][2]
    assert np.isnan(v).any() and np.isposinf(v).any() and np.isneginf(v).any() and (np.abs(v) == 2.0 ** -1074).any()
    assert ((v == 0) & np.signbit(v)).any() and ((v == 0) & ~np.signbit(v)).any() and (v.view(np.uint64) == 0x7FF8_0000_DEAD_BEEF).any()


@pytest.mark.parametrize("tag", TAGS)
def test_extract_is_the_host_model(torch_dev, tag):
    torch = torch_dev
    _, m, n, A, kw, perm, mode = cases()[tag]
    w_rp, w_ci, w_map = reference(tag)
    w_v = A[2][w_map]
    mc = w_rp.size - 1
    if mode in ("full", "no_map"):
        rp, ci, v = run_case(torch, tag, want_map=False)  # no map: it lives in the workspace
        assert ci.numel() == v.numel() == w_ci.size and rp.numel() == mc + 1, tag  # *h_nnz
        assert same(rp, w_rp) and same(ci, w_ci) and same_bits(v, w_v), tag
    if mode == "full":
        rp, ci, v, cmap = run_case(torch, tag)
        assert ci.numel() == v.numel() == cmap.numel() == w_ci.size and rp.numel() == mc + 1, tag
        assert same(rp, w_rp) and same(ci, w_ci) and same(cmap, w_map) and same_bits(v, w_v), tag
    # structure only, without and with the map
    s_rp, s_ci, s_v = run_case(torch, tag, value=None, want_map=False)
    assert s_v is None and same(s_rp, w_rp) and same(s_ci, w_ci), tag
    m_rp, m_ci, m_v, m_map = run_case(torch, tag, value=None)
    assert m_v is None and same(m_rp, w_rp) and same(m_ci, w_ci) and same(m_map, w_map), tag


def test_values_follow_new_inputs(torch_dev, hiplib):
    torch = torch_dev
    for tag in ("permuted", "sub_block", "hub_row", "one_by_one"):
        _, m, n, A, kw, perm, _ = cases()[tag]
        w_rp, w_ci, w_map = reference(tag)
        rp, ci, v, cmap = run_case(torch, tag)
        nnz = ci.numel()
        rng = np.random.default_rng(nnz)
        out = torch.full((nnz,), 7.25, dtype=torch.float64, device="cuda")
        d_v = dev(torch, A[2])
        spmv_acc_amd.csr_extract_values(cmap, d_v, out)  # the same values repeat the first call's bits
        assert same_bits(out, A[2][w_map]) and torch.equal(out.view(torch.int64), v.view(torch.int64)), tag
        da = d_v.clone()
        # captured into a graph (one stream, no parallel branches) and replayed on values edited in place between the replays
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=s):
                spmv_acc_amd.csr_extract_values(cmap, da, out)
        for _ in range(2):
            new = rng.standard_normal(A[2].size)
            da.copy_(dev(torch, new))
            out.fill_(7.25)
            spmv_acc_amd.csr_extract_values(cmap, da, out)
            assert same_bits(out, new[w_map]), tag
            fresh = run_case(torch, tag, value=da, want_map=False)[2]
            assert same_bits(fresh, new[w_map]) and torch.equal(fresh.view(torch.int64), out.view(torch.int64)), tag
            out.fill_(7.25)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert same_bits(out, new[w_map]), tag
        del g
    assert hiplib.spmv_acc_last_error() == 0


def test_special_values(torch_dev):
    """NaN with a payload, +-Inf, +-0.0 and subnormals pass through untouched: the bits are copied."""
    torch = torch_dev
    _, m, n, A, kw, perm, _ = cases()["specials"]
    w_rp, w_ci, w_map = reference("specials")
    rp, ci, v, cmap = run_case(torch, "specials")
    assert same(rp, w_rp) and same(ci, w_ci) and same(cmap, w_map) and same_bits(v, A[2][w_map])
    out = torch.full_like(v, 7.25)
    spmv_acc_amd.csr_extract_values(cmap, dev(torch, A[2]), out)
    assert same_bits(out, A[2][w_map])
    got = out.cpu().numpy()
    assert (got.view(np.uint64) == 0x7FF8_0000_DEAD_BEEF).sum() == (A[2].view(np.uint64) == 0x7FF8_0000_DEAD_BEEF).sum() > 0
    # without a permutation, and a band
    d = dev_csr(torch, A)
    for kw in (dict(), dict(diag_hi=0), dict(diag_lo=1)):
        w = host_csr_extract(m, n, A, **kw)
        g = spmv_acc_amd.csr_extract(m, n, *d, want_map=True, **kw)
        assert same(g[0], w[0]) and same(g[1], w[1]) and same(g[3], w[2]) and same_bits(g[2], w[3])


def test_crafted_map(torch_dev):
    """A map entry of -1 or >= nnz_a gives +0.0 there; nothing outside `out` is written."""
    torch = torch_dev
    _, m, n, A, kw, perm, _ = cases()["hub_row"]
    w_map = reference("hub_row")[2]
    nnz, nnz_a = w_map.size, A[2].size
    crafted = w_map.copy()
    rng = np.random.default_rng(9)
    crafted[rng.choice(nnz, 200, replace=False)] = np.array([-1, nnz_a, nnz_a + 7, 2 ** 31 - 1, -2 ** 31] * 40, dtype=np.int64).astype(np.int32)
    pad = 64
    buf = torch.full((nnz + 2 * pad,), 7.25, dtype=torch.float64, device="cuda")
    out = buf[pad:pad + nnz]
    spmv_acc_amd.csr_extract_values(dev(torch, crafted), dev(torch, A[2]), out)
    torch.cuda.synchronize()
    assert bool((buf[:pad] == 7.25).all()) and bool((buf[pad + nnz:] == 7.25).all())
    inside = (crafted >= 0) & (crafted < nnz_a)
    want = np.where(inside, A[2][np.where(inside, crafted, 0)], 0.0)
    assert (~inside).sum() == 200 and same_bits(out, want) and not np.signbit(out.cpu().numpy()[~inside]).any()


def test_round_trip_through_csr_add(torch_dev):
    """Strict-lower, diagonal and strict-upper parts of a sorted A, added again: A's rowptr, colindex and value bits.  csr_add demands strictly
    ascending rows, so this also ties the output to that requirement."""
    torch = torch_dev
    _, m, n, A, _, _, _ = cases()["tril"]
    d = dev_csr(torch, A)
    L = spmv_acc_amd.csr_extract(m, n, *d, diag_hi=-1)
    D = spmv_acc_amd.csr_extract(m, n, *d, diag_lo=0, diag_hi=0)
    U = spmv_acc_amd.csr_extract(m, n, *d, diag_lo=1)
    assert L[1].numel() + D[1].numel() + U[1].numel() == A[1].size and min(L[1].numel(), D[1].numel(), U[1].numel()) > 0
    LD = spmv_acc_amd.csr_add(m, n, *L, *D)
    rp, ci, v = spmv_acc_amd.csr_add(m, n, *LD, *U)
    assert same(rp, A[0]) and same(ci, A[1]) and same_bits(v, A[2])
    # an unsorted A, sorted by an extraction, is accepted as well
    _, m, n, Un, _, _, _ = cases()["unsorted_in"]
    srt = spmv_acc_amd.csr_extract(m, n, *dev_csr(torch, Un))
    twice = spmv_acc_amd.csr_add(m, n, *srt, *srt, alpha=1.0, beta=1.0)
    w = host_csr_extract(m, n, Un)
    assert same(twice[0], w[0]) and same(twice[1], w[1]) and same_bits(twice[2], w[3] + w[3])


def test_permuted_through_the_engine(torch_dev, oracle):
    torch = torch_dev
    for tag in ("permuted",):
        _, m, n, A, _, perm, _ = cases()[tag]
        w_rp, w_ci, w_map = reference(tag)
        w_v = A[2][w_map]
        c_rp, c_ci, c_v = run_case(torch, tag, want_map=False)
        nnz = c_ci.numel()
        rng = np.random.default_rng(m + nnz)
        x = rng.standard_normal(n)
        xp = x[perm]  # (P A P^T) (P x) = P (A x)
        ref = oracle.host_spmv(1.0, 0.0, w_rp, w_ci, w_v, xp, np.zeros(m))
        scale = oracle.host_spmv(1.0, 0.0, w_rp, w_ci, np.abs(w_v), np.abs(xp), np.zeros(m))
        ax = oracle.host_spmv(1.0, 0.0, A[0], A[1], A[2], x, np.zeros(m))
        live = scale > 0
        assert np.all(np.abs(ref - ax[perm])[live] / scale[live] <= SCALED_TOL)  # the host model's C is the permuted A
        for strat in ("adaptive", "flat"):
            dy = torch.zeros(m, dtype=torch.float64, device="cuda")
            spmv_acc_amd.csr_spmv(1.0, 0.0, m, n, nnz, c_rp, c_ci, c_v, dev(torch, xp), dy, strategy=strat)
            torch.cuda.synchronize()
            got = dy.cpu().numpy()
            assert np.all(got[~live] == ref[~live])
            err = float(np.max(np.abs(got[live] - ref[live]) / scale[live]))
            print(f"{tag} {strat}: C x' against the oracle on the host model's C, scaled error {err:.3e}")
            # (rows of at most 5 terms: the summation bound, 2^-53 per term and operation, is three orders below the gate)
            assert err <= SCALED_TOL, (tag, strat, err)
        spmv_acc_amd.release_plans(c_rp)


def test_extract_contract(torch_dev, hiplib):
    torch = torch_dev
    rng = np.random.default_rng(31)
    m, n = 3000, 3000
    A = random_sorted_csr(m, n, 30_000, rng)
    rows = rng.permutation(m)[:2000].astype(np.int32)
    cols = rng.permutation(n)[:2500]
    nc = 2600
    colmap = np.full(n, -1, dtype=np.int32)
    colmap[cols] = rng.permutation(nc)[:2500].astype(np.int32)
    w_rp, w_ci, w_map, w_v = host_csr_extract(m, n, A, rows, colmap, nc, -2000, 1500)
    nnz, nnz_a, mc = w_ci.size, A[1].size, rows.size
    dA = dev_csr(torch, A)
    d_rows, d_colmap = dev(torch, rows), dev(torch, colmap)
    plans = hiplib.spmv_acc_cached_plans()
    extract = hiplib.spmv_acc_csr_extract
    pad = 64
    o_rp = torch.full((mc + 1 + pad,), -7, dtype=torch.int32, device="cuda")
    o_ci = torch.full((nnz_a + pad,), -7, dtype=torch.int32, device="cuda")
    o_v = torch.full((nnz_a + pad,), 7.25, dtype=torch.float64, device="cuda")
    o_map = torch.full((nnz_a + pad,), -7, dtype=torch.int32, device="cuda")
    h = ctypes.c_int(-5)

    def untouched():
        torch.cuda.synchronize()
        return bool((o_rp == -7).all()) and bool((o_ci == -7).all()) and bool((o_v == 7.25).all()) and bool((o_map == -7).all()) and h.value == -5

    def report(rc):
        msg = hiplib.spmv_acc_last_error_string().decode()
        code = hiplib.spmv_acc_last_error()
        hiplib.spmv_acc_clear_error()
        return rc, code, msg

    def call(a=dA, r=d_rows, cm=d_colmap, mm=m, nn=n, na=nnz_a, mcc=mc, ncc=nc):
        return report(extract(mm, nn, na, ptr(a[0]), ptr(a[1]), ptr(a[2]), mcc, ptr(r), ncc, ptr(cm), -2000, 1500, ptr(o_rp), ptr(o_ci), ptr(o_v),
                              ptr(o_map), ctypes.byref(h)))

    def refused(result, *needles):
        rc, code, msg = result
        assert rc == 2 and code == 2 and "spmv_acc_csr_extract:" in msg and all(s in msg for s in needles), (rc, msg)
        assert untouched(), msg

    hiplib.spmv_acc_set_stream(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    clean = "0 rows outside [0, m), 0 repeated rows, 0 selected rows with a descending or out-of-range rowptr extent, 0 colmap values >= nc, 0 repeated colmap values"
    # a row out of range (above and below), a repeated row
    for value in (m, -1, 2 ** 31 - 1):
        bad = rows.copy()
        bad[5] = value
        refused(call(r=dev(torch, bad)), clean.replace("0 rows outside", "1 rows outside"), "nothing was written")
    bad = rows.copy()
    bad[5] = bad[900]
    refused(call(r=dev(torch, bad)), clean.replace("0 repeated rows", "1 repeated rows"), "nothing was written")
    bad[6] = bad[900]
    refused(call(r=dev(torch, bad)), clean.replace("0 repeated rows", "2 repeated rows"))
    # a colmap value >= nc, a repeated one
    for value in (nc, 2 ** 31 - 1):
        bad = colmap.copy()
        bad[cols[3]] = value
        refused(call(cm=dev(torch, bad)), clean.replace("0 colmap values >= nc", "1 colmap values >= nc"), "nothing was written")
    bad = colmap.copy()
    bad[cols[3]] = bad[cols[700]]
    refused(call(cm=dev(torch, bad)), clean.replace("0 repeated colmap values", "1 repeated colmap values"), "nothing was written")
    # a candidate's column outside [0, n); the same in a row that is not selected is not an error
    lens = np.diff(A[0])
    selected = np.zeros(m, dtype=bool)
    selected[rows] = True
    r_in = int(np.flatnonzero(selected & (lens >= 2))[4])
    r_out = int(np.flatnonzero(~selected[1:] & ~selected[:-1] & (lens[1:] >= 2))[4]) + 1  # (its predecessor is not selected either)
    for value in (n, -1):
        bad = A[1].copy()
        bad[A[0][r_in] + 1] = value
        refused(call(a=(dA[0], dev(torch, bad), dA[2])), "1 candidates with a column outside [0, n)", "nothing was written")
    bad = A[1].copy()
    bad[A[0][r_out] + 1] = n
    h.value = -5
    rc, code, msg = call(a=(dA[0], dev(torch, bad), dA[2]))
    torch.cuda.synchronize()
    assert rc == 0 and h.value == nnz and same(o_rp[:mc + 1], w_rp) and same(o_ci[:nnz], w_ci) and same(o_map[:nnz], w_map) and same_bits(o_v[:nnz], w_v), msg

    def refill():
        for t in (o_rp, o_ci, o_map):
            t.fill_(-7)
        o_v.fill_(7.25)
        h.value = -5

    refill()
    # a descending extent of a selected row (row r_in - 1 grows, inside the arrays)
    desc = A[0].copy()
    desc[r_in] = A[0][r_in + 1] + 1
    refused(call(a=(dev(torch, desc), dA[1], dA[2])), clean.replace("0 selected rows with", "1 selected rows with"), "nothing was written")
    # ... of a row that is not selected: not read
    desc = A[0].copy()
    desc[r_out] = A[0][r_out + 1] + 1
    rc, code, msg = call(a=(dev(torch, desc), dA[1], dA[2]))
    torch.cuda.synchronize()
    assert rc == 0 and h.value == nnz and same(o_ci[:nnz], w_ci) and same(o_map[:nnz], w_map), msg
    refill()
    # an un-rebased rowptr, a wrong nnz_a
    refused(call(a=(dA[0] + 1, dA[1], dA[2])), "a_rowptr[0] != 0")
    for na in (nnz_a - 1, nnz_a + 1, 0):
        refused(call(na=na), "rowptr[m]")
    with pytest.raises(spmv_acc_amd.SpmvAccError, match="1 repeated rows"):
        bad = rows.copy()
        bad[5] = bad[900]
        spmv_acc_amd.csr_extract(m, n, *dA, rows=dev(torch, bad))
    # csr_permute: a perm out of range is refused by the wrapper before it is an index, a repeated one by the entry's distinct-rows check
    S = cases()["tril"][3]
    dS = dev_csr(torch, S)
    perm = rng.permutation(250).astype(np.int32)
    for value in (250, -1):
        bad = perm.copy()
        bad[17] = value
        with pytest.raises(spmv_acc_amd.SpmvAccError, match="perm: values in"):
            spmv_acc_amd.csr_permute(250, *dS, dev(torch, bad))
    bad = perm.copy()
    bad[17] = bad[100]
    with pytest.raises(spmv_acc_amd.SpmvAccError, match="1 repeated rows"):
        spmv_acc_amd.csr_permute(250, *dS, dev(torch, bad))
    torch.cuda.synchronize()  # (no device-side assertion was tripped: the context is alive)
    # sizes beyond int32 block arithmetic: host-side, nothing is allocated or read
    big = 2 ** 31 - 2 ** 16
    assert call(mm=big)[0] == 4 and call(nn=big)[0] == 4 and call(na=big)[0] == 4 and call(mcc=big)[0] == 4 and call(ncc=big)[0] == 4 and untouched()
    # nothing to extract: rowptr zeroed, *h_nnz = 0, nothing else touched
    zero_rp = torch.zeros(m + 1, dtype=torch.int32, device="cuda")
    none = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    for kw, rows_c in ((dict(a=(zero_rp, dA[1], dA[2]), na=0), mc), (dict(a=(zero_rp, dA[1], dA[2]), na=-1), mc), (dict(mcc=0), 0), (dict(mm=0, na=0), mc),
                       (dict(cm=none), mc)):
        refill()
        rc, code, msg = call(**kw)
        torch.cuda.synchronize()
        assert rc == 0 and h.value == 0 and bool((o_rp[:rows_c + 1] == 0).all()) and bool((o_rp[rows_c + 1:] == -7).all()), (kw.keys(), rc, msg)
        assert bool((o_ci == -7).all()) and bool((o_v == 7.25).all()) and bool((o_map == -7).all())
    refill()
    refused(call(mm=0), "without rows")  # non-zeros without rows
    # only the used prefixes are written; nnz_a is read from the device when negative
    for na in (nnz_a, -1):
        refill()
        rc, code, msg = call(na=na)
        torch.cuda.synchronize()
        assert rc == 0 and h.value == nnz, (rc, msg)
        assert same(o_rp[:mc + 1], w_rp) and bool((o_rp[mc + 1:] == -7).all()) and same(o_ci[:nnz], w_ci) and bool((o_ci[nnz:] == -7).all())
        assert same_bits(o_v[:nnz], w_v) and bool((o_v[nnz:] == 7.25).all()) and same(o_map[:nnz], w_map) and bool((o_map[nnz:] == -7).all())
    # two calls on the same inputs give identical bits; tunable deterministic = 1 changes no bit
    first = spmv_acc_amd.csr_extract(m, n, *dA, rows=d_rows, colmap=d_colmap, nc=nc, want_map=True)
    try:
        assert hiplib.spmv_acc_set_tunable(b"deterministic", 1) == 0
        second = spmv_acc_amd.csr_extract(m, n, *dA, rows=d_rows, colmap=d_colmap, nc=nc, want_map=True)
    finally:
        hiplib.spmv_acc_reset_tunables()
        hiplib.spmv_acc_clear_error()
    assert all(torch.equal(x if x.dtype != torch.float64 else x.view(torch.int64), y if y.dtype != torch.float64 else y.view(torch.int64))
               for x, y in zip(first, second))
    # inside a capture: the first entry enqueues nothing and says why, the values entry is captured; the capture survives
    refill()
    d_map = dev(torch, w_map)
    out = torch.zeros(nnz, dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            spmv_acc_amd.csr_extract_values(d_map, dA[2], out)
            hiplib.spmv_acc_set_stream(ctypes.c_void_p(s.cuda_stream))
            in_capture = call()
    assert in_capture[0] == 2 and "capture" in in_capture[2], in_capture
    g.replay()
    torch.cuda.synchronize()
    assert same_bits(out, w_v) and untouched()
    del g
    # none of this made or touched a plan
    assert hiplib.spmv_acc_cached_plans() == plans


def test_extract_grid_stride_at_test_size(torch_dev, hiplib):
    """max_grid_blocks lowered to 64, the smallest cap the library honours (config.cpp max_grid_blocks(): a smaller value leaves the default in
    place).  large (200 000 rows, 800 000 entries, a random symmetric permutation: the sort path) strides in every pass: 782 workgroups of rows,
    3 126 tiles of candidates -- 800 000 is a multiple of the rank tile, so the scan's closing element opens a tile of its own --, 3 125 of C
    entries, 390 of the values pass.  hub_row strides over candidates and entries with a row that spans many tiles; sub_block takes the path
    without a sort."""
    torch = torch_dev
    try:
        assert hiplib.spmv_acc_set_tunable(b"max_grid_blocks", 64) == 0
        for tag in ("large", "hub_row", "sub_block"):
            _, m, n, A, kw, perm, _ = cases()[tag]
            w_rp, w_ci, w_map = reference(tag)
            if tag != "sub_block":
                assert A[1].size + 1 > 64 * RANK_TILE and w_ci.size > 64 * VALUES_TILE and (tag != "large" or m + 1 > 64 * 256)
            rp, ci, v, cmap = run_case(torch, tag)
            assert same(rp, w_rp) and same(ci, w_ci) and same(cmap, w_map) and same_bits(v, A[2][w_map]), tag
            out = torch.zeros_like(v)
            spmv_acc_amd.csr_extract_values(cmap, dev(torch, A[2]), out)
            assert same_bits(out, A[2][w_map]), tag
    finally:
        hiplib.spmv_acc_reset_tunables()
