"""GPU suite (-m gpu): 8-bit codes of the column encoding (round 7; spmv_acc_amd/csrc/k_col16.hip encodes them, tile_stage.hpp Codes4<8> reads them,
tuner.cpp ensure_col16 picks the width by rule, tunable col16 = 8 / 2 pins 8- / 16-bit codes).

8-bit codes change how a column is stored, never which column a product uses: the same plan settings with either width must give bitwise the same
y, and both must match the oracle.  The window edges (base + 254 is a code, base + 255 and base - 1 escape), a base clamped at column 0, the last
column, a chunk of escapes that overflows its record, ragged ends, empty rows, row shards and the stale-colindex guard are exercised with 8-bit codes."""
import numpy as np
import pytest

import spmv_acc_amd
from spmv_acc_amd import synth

pytestmark = pytest.mark.gpu

SCALED_TOL = 1e-12
# the encoding pinned (8 = 8-bit codes, 2 = 16-bit codes) and every timed choice that could move a tile origin or a sum pinned with it
PINS = {"line_enhance": {"stream_plain": 1, "rowblock_target": 1800},
        "flat": {"stream_plain": 1, "flat_rowblock": 0, "flat_npt": 8, "flat_finish": 1, "flat_early": 0}}


@pytest.fixture(scope="module")
def torch_dev(hiplib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def headline_like(m, n, rng, far=0.10):
    """Hardesty3-shaped: 3..7 non-zeros per row, near columns drifting 0.92 per row within +-7, a fraction of uniformly random far columns."""
    lens = rng.integers(3, 8, size=m)
    rowptr = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(lens, out=rowptr[1:])
    rows = np.repeat(np.arange(m, dtype=np.int64), lens)
    near = (rows * 92) // 100 + rng.integers(-7, 8, size=rows.size)
    cols = np.where(rng.random(rows.size) < far, rng.integers(0, n, size=rows.size), np.clip(near, 0, n - 1)).astype(np.int32)
    return rowptr.astype(np.int32), cols, rng.uniform(-1.0, 1.0, size=rows.size)


def window_edges(rng, nchunks=400, n=300000):
    """Rows of 4 non-zeros: one chunk = 64 rows, lane l of a wavefront's step holds row l.  A plain chunk's row is {C, C+1, C+2, C+3}: every lane's
    second-smallest column is C + 1, so the 8-bit base is C - 126.  Rows of some chunks then put a column at base + 254 (code 254, the last code),
    base + 255 and base - 1 (escapes) without moving the median.  Chunk 0 has C = 0 (base clamped at 0: 254 is a code, 255 escapes), the last chunk
    ends at column n - 1, chunk 7 holds 256 columns 1000 apart (all but the median's escape: 16-int records overflow), chunks 9 and 11 hold 13 and
    61 escapes (just past 16- and 64-int records)."""
    m = nchunks * 64
    cols = np.zeros((m, 4), dtype=np.int64)
    for c in range(nchunks):
        C = 0 if c == 0 else (n - 4 if c == nchunks - 1 else int(rng.integers(200, n - 400)))
        rows = cols[64 * c:64 * (c + 1)]
        rows[:] = C + np.arange(4)
        b = max(C + 1 - 127, 0)
        if c % 3 == 1:
            rows[5, 3] = b + 254
            rows[6, 3] = b + 255
            rows[7, 0] = b - 1
        if c == 0:
            rows[5, 3], rows[6, 3] = 254, 255
    rows = cols[64 * 7:64 * 8]
    rows[:] = (np.arange(256) * 1000 + 500).reshape(64, 4)
    for c, k in ((9, 13), (11, 61)):
        rows = cols[64 * c:64 * (c + 1)]
        C = int(rows[0, 0])
        far = rng.choice(np.arange(0, n - 4), size=k + 32, replace=False)
        far = far[np.abs(far - C) > 300][:k]
        rows[np.arange(far.size), 3] = far  # (the largest entry of a lane: its second-smallest column stays C + 1)
    rowptr = np.arange(0, 4 * m + 1, 4, dtype=np.int32)
    return rowptr, cols.reshape(-1).astype(np.int32), rng.uniform(-1.0, 1.0, size=4 * m)


def _run(torch, hiplib, strategy, knobs, mat, n, x, y0, alpha, beta, rowptr_view=None):
    rowptr, cols, vals = mat
    hiplib.spmv_acc_reset_tunables()
    for k, v in knobs.items():
        assert hiplib.spmv_acc_set_tunable(k.encode(), v) == 0
    m = rowptr.size - 1
    drp, dci, dv, dx, dy = (dev(torch, a) for a in (rowptr, cols, vals, x, y0))
    spmv_acc_amd.csr_spmv(alpha, beta, m, n, int(rowptr[-1]), drp, dci, dv, dx, dy, strategy=strategy)
    torch.cuda.synchronize()
    info = spmv_acc_amd.query_plan(drp, m)
    spmv_acc_amd.release_plans(drp)
    return dy.cpu().numpy(), info


def _cases(rng):
    out = [("window edges", window_edges(rng), 300000), ("headline-shaped", headline_like(40000, 2_000_000, rng), 2_000_000)]
    for r in range(4):
        lens = rng.integers(3, 8, size=30000)
        lens[-1] += (r - int(lens.sum())) % 4  # nnz mod 4 == r
        out.append((f"nnz mod 4 = {r}", synth.csr_from_row_lengths(lens, 28000, rng, locality=7, far_fraction=0.05), 28000))
    lens = rng.integers(0, 12, size=40000)
    lens[rng.integers(0, 40000, 3000)] = 0
    lens[-50:] = 0  # an empty tail
    out.append(("empty rows and an empty tail", synth.csr_from_row_lengths(lens, 30000, rng, locality=20, far_fraction=0.02), 30000))
    return out


@pytest.mark.parametrize("strategy", ["line_enhance", "flat"])
def test_8_and_16_bit_codes_give_bitwise_the_same_y(torch_dev, oracle, hiplib, strategy):
    """Width pinned to 8 against width pinned to 16 under the same plan settings: the decoded columns are the same, so y is bitwise equal; both match
    the oracle at (alpha, beta) = (1, 1), (0.5, -2), (1, 0), and the plan reports the width and record size it read."""
    torch = torch_dev
    rng = np.random.default_rng(71)
    try:
        for tag, mat, n in _cases(rng):
            rowptr, cols, vals = mat
            x, y0 = rng.standard_normal(n), rng.standard_normal(rowptr.size - 1)
            for alpha, beta in ((1.0, 1.0), (0.5, -2.0), (1.0, 0.0)):
                ref = oracle.host_spmv(alpha, beta, rowptr, cols, vals, x, y0)
                got = {}
                for bits, mode in ((8, 8), (16, 2)):
                    y, info = _run(torch, hiplib, strategy, dict(PINS[strategy], col16=mode), mat, n, x, y0, alpha, beta)
                    assert info["last_kernel"] in ("rowblock", "flat_tile") and info["col_bits"] == bits and info["col16"] in (16, 32, 64), (tag, bits, info)
                    assert oracle.scaled_error(y, ref, alpha, beta, rowptr, cols, vals, x, y0) <= SCALED_TOL, (tag, strategy, bits, alpha, beta)
                    got[bits] = y
                assert np.array_equal(got[8], got[16]), (tag, strategy, alpha, beta)
    finally:
        hiplib.spmv_acc_reset_tunables()
        spmv_acc_amd.release_plans()


def test_window_edges_overflow_a_pinned_16_int_record(torch_dev, oracle, hiplib):
    """The edge matrix under 8-bit codes and 16-int records pinned by the rule: fewer than 1 % of its chunks hold more than 12 escapes, so its records
    are 16 ints and chunks 7, 9 and 11 go to the overflow list -- with the same y as the caller's colindex."""
    torch = torch_dev
    rng = np.random.default_rng(72)
    mat = window_edges(rng)
    rowptr, cols, vals = mat
    n = 300000
    x, y0 = rng.standard_normal(n), rng.standard_normal(rowptr.size - 1)
    ref = oracle.host_spmv(1.0, 1.0, rowptr, cols, vals, x, y0)
    try:
        for strategy in ("line_enhance", "flat"):
            y8, info = _run(torch, hiplib, strategy, dict(PINS[strategy], col16=8), mat, n, x, y0, 1.0, 1.0)
            assert info["col_bits"] == 8 and info["col16"] == 16, info
            y0b, info0 = _run(torch, hiplib, strategy, dict(PINS[strategy], col16=0), mat, n, x, y0, 1.0, 1.0)
            assert info0["col_bits"] == 0 and info0["col16"] == 0, info0
            assert oracle.scaled_error(y8, ref, 1.0, 1.0, rowptr, cols, vals, x, y0) <= SCALED_TOL, strategy
            if strategy == "flat":
                assert np.array_equal(y8, y0b)  # (same tile origins)
    finally:
        hiplib.spmv_acc_reset_tunables()
        spmv_acc_amd.release_plans()


def test_rule_picks_the_width(torch_dev, hiplib):
    """col16 = 1 (always, width by rule): 8-bit codes on a headline-shaped matrix (about 5 non-zeros per row, 10 % far columns: the far columns
    escape at either width), 16-bit on long rows whose chunks span thousands of columns (TSOPF-shaped) and where the locality is wider than 255."""
    torch = torch_dev
    rng = np.random.default_rng(73)
    cases = [
        ("headline-shaped", headline_like(150000, 4_000_000, rng), 4_000_000, (8,)),
        ("long rows", synth.csr_from_row_lengths(rng.integers(380, 470, size=600), 40000, rng, locality=2000, far_fraction=0.0), 40000, (16, 0)),
        ("locality 1000", synth.csr_from_row_lengths(rng.integers(20, 40, size=20000), 400000, rng, locality=1000, far_fraction=0.02), 400000, (16, 0)),
    ]
    try:
        for tag, mat, n, want in cases:
            rowptr = mat[0]
            x, y0 = rng.standard_normal(n), rng.standard_normal(rowptr.size - 1)
            _, info = _run(torch, hiplib, "line_enhance", {"col16": 1}, mat, n, x, y0, 1.0, 1.0)
            assert info["col_bits"] in want, (tag, info)
            if want == (8,):
                assert info["last_kernel"] == "rowblock" and info["col16"] == 64, (tag, info)
            assert (info["col16"] > 0) == (info["col_bits"] > 0), (tag, info)
    finally:
        hiplib.spmv_acc_reset_tunables()
        spmv_acc_amd.release_plans()


def test_settled_plan_repeats_bitwise(torch_dev, oracle, hiplib):
    """Default settings on a headline-shaped matrix: after spmv_acc_prepare the plan is settled, later calls repeat bitwise whichever stream and
    width it kept, and the width it reports goes with the record size."""
    torch = torch_dev
    rng = np.random.default_rng(74)
    n = 2_000_000
    rowptr, cols, vals = headline_like(200000, n, rng)
    m, nnz = rowptr.size - 1, int(rowptr[-1])
    x, y0 = rng.standard_normal(n), rng.standard_normal(m)
    ref = oracle.host_spmv(1.0, 1.0, rowptr, cols, vals, x, y0)
    drp, dci, dv, dx = (dev(torch, a) for a in (rowptr, cols, vals, x))
    try:
        for strategy in ("adaptive", "line_enhance"):
            hiplib.spmv_acc_reset_tunables()
            spmv_acc_amd.prepare(m, n, nnz, drp, dci, dv, dx, strategy=strategy)
            outs = []
            for _ in range(3):
                dy = dev(torch, y0)
                spmv_acc_amd.csr_spmv(1.0, 1.0, m, n, nnz, drp, dci, dv, dx, dy, strategy=strategy)
                torch.cuda.synchronize()
                outs.append(dy.cpu().numpy())
            info = spmv_acc_amd.query_plan(drp, m)
            assert info["settled"] and info["col_bits"] in (0, 8, 16) and (info["col16"] > 0) == (info["col_bits"] > 0), (strategy, info)
            assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[1], outs[2]), strategy
            assert oracle.scaled_error(outs[0], ref, 1.0, 1.0, rowptr, cols, vals, x, y0) <= SCALED_TOL, strategy
            spmv_acc_amd.release_plans(drp)
    finally:
        hiplib.spmv_acc_reset_tunables()
        spmv_acc_amd.release_plans()


@pytest.mark.parametrize("strategy", ["line_enhance", "flat"])
def test_row_shards_without_rebasing_8_bit(torch_dev, oracle, hiplib, strategy):
    """Un-rebased row sub-ranges read 8-bit codes by absolute non-zero index, as 16-bit ones (test_gpu_col16.py::test_row_shards_without_rebasing)."""
    torch = torch_dev
    rng = np.random.default_rng(75)
    n = 30000
    rowptr, cols, vals = synth.csr_from_row_lengths(rng.integers(3, 9, size=60000), n, rng, locality=5, far_fraction=0.03)
    x, y0 = rng.standard_normal(n), rng.standard_normal(60000)
    ref = oracle.host_spmv(1.0, 1.0, rowptr, cols, vals, x, y0)
    drp, dci, dv, dx = (dev(torch, a) for a in (rowptr, cols, vals, x))
    try:
        hiplib.spmv_acc_reset_tunables()
        for k, v in (("col16", 8), ("flat_rowblock", 0)):
            assert hiplib.spmv_acc_set_tunable(k.encode(), v) == 0
        for r0, r1 in ((12345, 57001), (1, 60000), (3001, 17777)):
            assert int(rowptr[r0]) % 2048 != 0
            dy = dev(torch, y0)
            spmv_acc_amd.csr_spmv(1.0, 1.0, r1 - r0, n, int(rowptr[r1]), drp[r0:], dci, dv, dx, dy[r0:], strategy=strategy)
            torch.cuda.synchronize()
            got = dy.cpu().numpy()
            assert np.array_equal(got[:r0], y0[:r0]) and np.array_equal(got[r1:], y0[r1:]), (r0, r1, "wrote outside the shard")
            assert np.max(np.abs(got[r0:r1] - ref[r0:r1])) <= 1e-11, (r0, r1)
            assert spmv_acc_amd.query_plan(drp[r0:], r1 - r0)["col_bits"] == 8, (r0, r1)
            spmv_acc_amd.release_plans(drp[r0:])
    finally:
        hiplib.spmv_acc_reset_tunables()
        spmv_acc_amd.release_plans()


def test_colindex_edited_in_place_is_noticed_8_bit(torch_dev, oracle, hiplib):
    """The stale-colindex guard covers 8-bit codes as it covers 16-bit ones: a wholesale in-place rewrite of colindex (same rowptr) raises the plan's
    stale flag, and the call after the report runs on a rebuilt plan."""
    torch = torch_dev
    rng = np.random.default_rng(76)
    n = 200000
    rowptr, cols, vals = headline_like(60000, n, rng, far=0.02)
    m, nnz = rowptr.size - 1, int(rowptr[-1])
    x, y0 = rng.standard_normal(n), rng.standard_normal(m)
    drp, dci, dv, dx = (dev(torch, a) for a in (rowptr, cols, vals, x))

    def spmv():
        dy = dev(torch, y0)
        spmv_acc_amd.csr_spmv(1.0, 1.0, m, n, nnz, drp, dci, dv, dx, dy, strategy="line_enhance")
        torch.cuda.synchronize()
        return dy.cpu().numpy()

    try:
        hiplib.spmv_acc_reset_tunables()
        assert hiplib.spmv_acc_set_tunable(b"col16", 8) == 0
        hiplib.spmv_acc_clear_error()
        got = spmv()
        assert spmv_acc_amd.query_plan(drp, m)["col_bits"] == 8
        assert oracle.scaled_error(got, oracle.host_spmv(1.0, 1.0, rowptr, cols, vals, x, y0), 1.0, 1.0, rowptr, cols, vals, x, y0) <= SCALED_TOL
        cols2 = (n - 1 - cols).astype(np.int32)  # every column mirrored: same rowptr, (almost) every colindex entry different
        dci.copy_(dev(torch, cols2))
        torch.cuda.synchronize()
        reported = False
        try:
            spmv()
        except spmv_acc_amd.SpmvAccError:
            reported = True
        reported = reported or hiplib.spmv_acc_last_error() != 0
        assert reported, "the colindex samples did not raise the stale flag"
        hiplib.spmv_acc_clear_error()
        try:
            got = spmv()
        except spmv_acc_amd.SpmvAccError:
            hiplib.spmv_acc_clear_error()
            got = spmv()
        assert oracle.scaled_error(got, oracle.host_spmv(1.0, 1.0, rowptr, cols2, vals, x, y0), 1.0, 1.0, rowptr, cols2, vals, x, y0) <= SCALED_TOL
    finally:
        hiplib.spmv_acc_clear_error()
        hiplib.spmv_acc_reset_tunables()
        spmv_acc_amd.release_plans()
