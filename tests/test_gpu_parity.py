"""GPU suite (-m gpu): the HIP path, called through the C ABI, against the CPU oracle on the same
seeded inputs, against the committed golden fixtures, and -- at BASELINE.json's full sizes -- through
size-independent properties.

Tolerances (fp64, north_star: 1e-9 relative vs the reference CPU verification path):
  * scaled error  |d-h| / (|alpha| sum_j |a_ij x_j| + |beta y0_i|)  <= 1e-12   (robust form)
  * plain relative error |d-h|/|h| <= 1e-9 on rows with |h| >= 1e-6 * scale (no cancellation)
  * the reference's own verdicts (cli/verification.cpp:43-54 and :15-38, rel 1e-7) must pass
  * integer preprocessing (break points, row blocks): bit-exact
"""
import os
import subprocess

import numpy as np
import pytest

import spmv_acc_amd
from spmv_acc_amd import synth
from special_values import MEASUREMENT_SWITCHES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SCALED_TOL = 1e-12
REL_TOL = 1e-9
ALL = spmv_acc_amd.STRATEGIES


@pytest.fixture(scope="module")
def torch_dev(hiplib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(torch, strat, alpha, beta, rowptr, cols, vals, x, y0, pass_host_rowptr=True):
    m, n, nnz = rowptr.size - 1, x.size, int(rowptr[-1])
    drp, dci, dv, dx, dy = dev(torch, rowptr), dev(torch, cols), dev(torch, vals), dev(torch, x), dev(torch, y0)
    spmv_acc_amd.csr_spmv(alpha, beta, m, n, nnz, drp, dci, dv, dx, dy, strategy=strat,
                          h_rowptr=rowptr if pass_host_rowptr else None)
    torch.cuda.synchronize()
    out = dy.cpu().numpy()
    spmv_acc_amd.release_plans(drp)
    return out


def check(oracle, got, alpha, beta, rowptr, cols, vals, x, y0, tag):
    ref = oracle.host_spmv(alpha, beta, rowptr, cols, vals, x, y0)
    err = oracle.scaled_error(got, ref, alpha, beta, rowptr, cols, vals, x, y0)
    assert err <= SCALED_TOL, (tag, "scaled error", err)
    import scipy.sparse as sp

    m = rowptr.size - 1
    scale = abs(alpha) * (sp.csr_matrix((np.abs(vals), cols, rowptr), shape=(m, x.size)) @ np.abs(x)) + np.abs(beta * y0)
    solid = np.abs(ref) >= 1e-6 * np.maximum(scale, 1e-300)
    if np.any(solid):
        rel = np.max(np.abs(got[solid] - ref[solid]) / np.abs(ref[solid]))
        assert rel <= REL_TOL, (tag, "relative error", rel)
    me, first, cnt = oracle.verify_y(got, ref)
    assert cnt == 0, (tag, "reference benchmark verdict", first, cnt, me)


KINDS = [("uniform", 3000, 3100, 5), ("short", 5000, 5000, 2), ("powerlaw", 2500, 4000, 6),
         ("spikes", 1500, 9000, 3), ("empty_rows", 4000, 2500, 4), ("dense_rows", 40, 5000, 400),
         ("single", 2049, 2049, 1), ("uniform", 700, 700, 33), ("uniform", 300, 900, 100)]


@pytest.mark.parametrize("strat", ALL)
def test_parity_all_strategies(torch_dev, oracle, strat):
    torch = torch_dev
    for i, (kind, m, n, avg) in enumerate(KINDS):
        rowptr, cols, vals = synth.random_csr(m, n, avg, seed=100 + i, kind=kind)
        rng = np.random.default_rng(200 + i)
        x, y0 = synth.reference_rand_grid(n, rng), synth.reference_rand_grid(m, rng)
        for alpha, beta in ((1.0, 1.0), (0.5, -2.0), (1.0, 0.0)):
            got = run(torch, strat, alpha, beta, rowptr, cols, vals, x, y0)
            check(oracle, got, alpha, beta, rowptr, cols, vals, x, y0, (strat, kind, m, alpha, beta))


@pytest.mark.parametrize("strat", spmv_acc_amd.HOT_STRATEGIES)
def test_golden_fixtures(torch_dev, oracle, strat):
    torch = torch_dev
    g = np.load(os.path.join(GOLD, "spmv_cases.npz"))
    for name in g["names"]:
        rowptr, cols, vals = g[f"{name}__rowptr"], g[f"{name}__cols"], g[f"{name}__vals"]
        x, y0 = g[f"{name}__x"], g[f"{name}__y0"]
        for k, (a, b) in enumerate(g["alpha_beta"]):
            got = run(torch, strat, float(a), float(b), rowptr, cols, vals, x, y0)
            want = g[f"{name}__out{k}"]
            err = oracle.scaled_error(got, want, float(a), float(b), rowptr, cols, vals, x, y0)
            assert err <= SCALED_TOL, (strat, name, a, b, err)


def test_rajat03_like_cli_protocol(torch_dev, oracle):
    """configs[0]'s protocol on the GPU path: alpha = beta = 1, 10 warm-ups with y reset, verify -> pass 7602."""
    torch = torch_dev
    rowptr, cols, vals = synth.rajat03_like()
    m = n = rowptr.size - 1
    rng = np.random.default_rng(1)
    x, y0 = synth.reference_rand_grid(n, rng), synth.reference_rand_grid(m, rng)
    drp, dci, dv, dx, dy0 = (dev(torch, a) for a in (rowptr, cols, vals, x, y0))
    dy = dy0.clone()
    for _ in range(11):
        dy.copy_(dy0)
        spmv_acc_amd.sparse_spmv(0, 1.0, 1.0, m, n, drp, dci, dv, dx, dy)  # ten-argument entry, device pointers only
    torch.cuda.synchronize()
    ref = oracle.host_spmv(1.0, 1.0, rowptr, cols, vals, x, y0)
    assert oracle.verify(dy.cpu().numpy(), ref) == -1  # "pass 7602 validation"
    info = spmv_acc_amd.query_plan(drp, m)
    assert info is not None and info["nnz"] == int(rowptr[-1])
    spmv_acc_amd.release_plans(drp)


@pytest.mark.parametrize("strat", spmv_acc_amd.HOT_STRATEGIES)
def test_edge_shapes(torch_dev, oracle, strat):
    torch = torch_dev
    rng = np.random.default_rng(42)
    cases = []
    # one row, one nnz; one long row; nnz not a multiple of 4; all rows empty; trailing/leading empties
    cases.append((np.array([0, 1], np.int32), np.array([0], np.int32), np.array([2.5]), 1))
    cases.append((np.array([0, 5001], np.int32), rng.integers(0, 64, 5001).astype(np.int32), rng.standard_normal(5001), 64))
    cases.append((np.array([0, 3, 3, 7], np.int32), np.array([0, 1, 2, 0, 1, 2, 3], np.int32), rng.standard_normal(7), 4))
    cases.append((np.zeros(100, np.int32), np.zeros(0, np.int32), np.zeros(0), 5))
    lens = np.zeros(9000, np.int64)
    lens[4000:4100] = 41
    rp = np.zeros(9001, np.int32)
    np.cumsum(lens, out=rp[1:])
    cases.append((rp, rng.integers(0, 300, int(rp[-1])).astype(np.int32), rng.standard_normal(int(rp[-1])), 300))
    # rows ending exactly on tile boundaries (2048 | 1024 | 4096)
    lens = np.full(40, 1024, np.int64)
    rp = np.zeros(41, np.int32)
    np.cumsum(lens, out=rp[1:])
    cases.append((rp, rng.integers(0, 500, int(rp[-1])).astype(np.int32), rng.standard_normal(int(rp[-1])), 500))
    # a long row preceded by empty rows inside one analysis block (the reference loses its first slice)
    lens = np.zeros(1500, np.int64)
    lens[700], lens[701], lens[1400:] = 9000, 4096, 5
    rp = np.zeros(1501, np.int32)
    np.cumsum(lens, out=rp[1:])
    cases.append((rp, rng.integers(0, 2000, int(rp[-1])).astype(np.int32), rng.standard_normal(int(rp[-1])), 2000))
    for ci_, (rowptr, cols, vals, n) in enumerate(cases):
        m = rowptr.size - 1
        x, y0 = rng.standard_normal(n), rng.standard_normal(m)
        for alpha, beta in ((1.0, 1.0), (-0.75, 0.0), (2.0, 0.5)):
            got = run(torch, strat, alpha, beta, rowptr, cols, vals, x, y0)
            check(oracle, got, alpha, beta, rowptr, cols, vals, x, y0, (strat, "edge", ci_, alpha, beta))


@pytest.mark.parametrize("strat", spmv_acc_amd.HOT_STRATEGIES)
def test_unaligned_views_and_device_only_rowptr(torch_dev, oracle, strat):
    """Sub-array views whose base is not 16-byte aligned take the element-wise load path; a NULL host
    rowptr makes the engine fetch its samples / rowptr from the device."""
    torch = torch_dev
    rowptr, cols, vals = synth.random_csr(3000, 3000, 9, seed=77, kind="uniform")
    m, n, nnz = 3000, 3000, int(rowptr[-1])
    rng = np.random.default_rng(5)
    x, y0 = rng.standard_normal(n), rng.standard_normal(m)
    pad_c = torch.zeros(nnz + 1, dtype=torch.int32, device="cuda")
    pad_v = torch.zeros(nnz + 1, dtype=torch.float64, device="cuda")
    pad_c[1:] = dev(torch, cols)
    pad_v[1:] = dev(torch, vals)
    dci, dv = pad_c[1:], pad_v[1:]
    assert dci.data_ptr() % 16 != 0
    drp, dx, dy = dev(torch, rowptr), dev(torch, x), dev(torch, y0)
    spmv_acc_amd.csr_spmv(1.0, 1.0, m, n, -1, drp, dci, dv, dx, dy, strategy=strat, h_rowptr=None)
    torch.cuda.synchronize()
    info = spmv_acc_amd.query_plan(drp, m)
    assert info["aligned16"] == 0 and info["nnz"] == nnz
    check(oracle, dy.cpu().numpy(), 1.0, 1.0, rowptr, cols, vals, x, y0, (strat, "unaligned"))
    spmv_acc_amd.release_plans(drp)


def test_bitwise_reproducible(torch_dev, hiplib):
    """No atomics anywhere: on one plan every call gives identical bits, for every strategy; with the timed per-matrix choices
    pinned (they may fall differently when candidates are within noise) a rebuilt plan does too."""
    torch = torch_dev
    rowptr, cols, vals = synth.random_csr(20000, 20000, 12, seed=9, kind="powerlaw")
    rng = np.random.default_rng(3)
    x, y0 = rng.standard_normal(20000), rng.standard_normal(20000)
    m = n = 20000
    nnz = int(rowptr[-1])
    drp, dci, dv, dx = (dev(torch, a) for a in (rowptr, cols, vals, x))
    for strat in ALL:
        outs = []
        # (a SETTLED plan: the first calls on a matrix may still be finishing the per-matrix timings -- tunable first_call_budget -- and a kernel
        # family that changes between two calls changes the order of the sums; spmv_acc_prepare settles everything up front)
        spmv_acc_amd.prepare(m, n, nnz, drp, dci, dv, dx, strategy=strat, beta=1.0)
        for _ in range(3):
            dy = dev(torch, y0)
            spmv_acc_amd.csr_spmv(1.0, 1.0, m, n, nnz, drp, dci, dv, dx, dy, strategy=strat)
            torch.cuda.synchronize()
            outs.append(dy.cpu().numpy())
        assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2]), strat
    spmv_acc_amd.release_plans(drp)
    try:
        # ONE switch pins every timed choice (round 3; rounds 1-2 pinned four tunables by hand, which no longer covers them all: flat's
        # small-grid choice between its tile kernel and the row blocks is timed too, and two fresh plans can fall differently)
        assert hiplib.spmv_acc_set_tunable(b"deterministic", 1) == 0
        for strat in ALL:
            a = run(torch, strat, 1.0, 1.0, rowptr, cols, vals, x, y0)  # run() releases the plan: b is computed on a new one
            b = run(torch, strat, 1.0, 1.0, rowptr, cols, vals, x, y0)
            assert np.array_equal(a, b), strat
    finally:
        hiplib.spmv_acc_reset_tunables()


def test_trans_is_reported_not_applied(torch_dev, oracle, hiplib):
    torch = torch_dev
    rowptr, cols, vals = synth.random_csr(500, 500, 5, seed=1)
    rng = np.random.default_rng(1)
    x, y0 = rng.standard_normal(500), rng.standard_normal(500)
    drp, dci, dv, dx, dy = (dev(torch, a) for a in (rowptr, cols, vals, x, y0))
    hiplib.spmv_acc_clear_error()
    spmv_acc_amd.sparse_spmv(1, 1.0, 1.0, 500, 500, drp, dci, dv, dx, dy)  # operation_transpose: unsupported
    torch.cuda.synchronize()
    assert hiplib.spmv_acc_last_error() == 1
    hiplib.spmv_acc_clear_error()
    # like the reference (which never reads trans) the non-transposed product is computed
    check(oracle, dy.cpu().numpy(), 1.0, 1.0, rowptr, cols, vals, x, y0, "trans")
    spmv_acc_amd.release_plans(drp)


# ---- row-block preprocessing pass ------------------------------------------------------------------------
def test_break_points_bit_exact(torch_dev, oracle):
    torch = torch_dev
    g = np.load(os.path.join(GOLD, "breakpoint_cases.npz"))
    cases = [(str(nm), g[f"{nm}__rowptr"]) for nm in g["names"]]
    for i, kind in enumerate(("uniform", "powerlaw", "spikes", "empty_rows", "dense_rows")):
        rp, _, _ = synth.random_csr(20000, 20000, 7, seed=300 + i, kind=kind)
        cases.append((kind, rp))
    for name, rp in cases:
        m, nnz = rp.size - 1, int(rp[-1])
        drp = dev(torch, rp)
        for stride in (256, 1024, 2048):
            n = spmv_acc_amd.break_points_len(nnz, stride)
            out = torch.full((n,), -7, dtype=torch.int32, device="cuda")  # no pre-zeroing needed
            spmv_acc_amd.break_points(drp, m, nnz, stride, out)
            torch.cuda.synchronize()
            want = oracle.break_points(rp, stride)
            assert np.array_equal(out.cpu().numpy(), want), (name, stride)
            key = f"{name}__{stride}"
            if key in g.files:
                assert np.array_equal(out.cpu().numpy(), g[key]), (name, stride, "golden")


def test_adaptive_branches_reached(torch_dev, oracle):
    """Each branch of the adaptive decision runs its kernel family and stays in parity."""
    torch = torch_dev
    rng = np.random.default_rng(8)
    specs = {
        1: np.concatenate([rng.integers(0, 3, 3000), rng.integers(20, 40, 3000)]),  # halves differ >= 4x
        2: rng.integers(0, 6, 6000),  # avg <= 4
        3: rng.integers(5, 12, 6000),  # small nnz, avg > 4
    }
    for want, lens in specs.items():
        rowptr, cols, vals = synth.csr_from_row_lengths(lens, 6000, rng)
        assert oracle.adaptive_pick(rowptr) == want
        x, y0 = rng.standard_normal(6000), rng.standard_normal(6000)
        got = run(torch, "adaptive", 1.0, 1.0, rowptr, cols, vals, x, y0)
        check(oracle, got, 1.0, 1.0, rowptr, cols, vals, x, y0, ("adaptive", want))
        got = run(torch, "adaptive", 1.0, 1.0, rowptr, cols, vals, x, y0, pass_host_rowptr=False)
        check(oracle, got, 1.0, 1.0, rowptr, cols, vals, x, y0, ("adaptive-device-samples", want))
    # branch 1 in the reference's own form (two lane widths, one per half) stays available behind a tunable
    lib = spmv_acc_amd.load_library()
    rowptr, cols, vals = synth.csr_from_row_lengths(specs[1], 6000, rng)
    x, y0 = rng.standard_normal(6000), rng.standard_normal(6000)
    assert lib.spmv_acc_set_tunable(b"adaptive_split", 1) == 0
    try:
        got = run(torch, "adaptive", 1.0, 1.0, rowptr, cols, vals, x, y0)
    finally:
        lib.spmv_acc_reset_tunables()
    check(oracle, got, 1.0, 1.0, rowptr, cols, vals, x, y0, ("adaptive-split", 1))


# ---- full-size checks (BASELINE.json configs[1]: Hardesty3-like, 8.2M rows / 40.5M nnz) --------------------------
@pytest.fixture(scope="module")
def hardesty(torch_dev):
    torch = torch_dev
    m, n, nnz, rp, ci, v = synth.hardesty3_like_torch(device="cuda")
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    x = torch.rand(n, generator=g, device="cuda", dtype=torch.float64) * 2 - 1
    y0 = torch.rand(m, generator=g, device="cuda", dtype=torch.float64) * 2 - 1
    return dict(m=m, n=n, nnz=nnz, rp=rp, ci=ci, v=v, x=x, y0=y0)


def _spmv(torch, H, strat, alpha, beta, x, y0):
    y = y0.clone()
    spmv_acc_amd.csr_spmv(alpha, beta, H["m"], H["n"], H["nnz"], H["rp"], H["ci"], H["v"], x, y, strategy=strat)
    torch.cuda.synchronize()
    return y


def test_full_size_adaptive_takes_line_branch(torch_dev, hardesty):
    H = hardesty
    assert (H["m"], H["n"], H["nnz"]) == synth.LARGE_SET["Hardesty3"]
    _spmv(torch_dev, H, "adaptive", 1.0, 1.0, H["x"], H["y0"])
    info = spmv_acc_amd.query_plan(H["rp"], H["m"])
    assert info["adaptive_branch"] == 2 and info["nnz"] == H["nnz"]  # 40451632 / 8217820 = 4 -> adaptive line


def test_full_size_row_sums_and_strategy_agreement(torch_dev, hardesty):
    """x = 1 makes y the row sums, which torch computes independently (index_add in fp64); all
    strategies must agree with it and with each other at full size."""
    torch = torch_dev
    H = hardesty
    m, nnz = H["m"], H["nnz"]
    rows = torch.repeat_interleave(torch.arange(m, device="cuda"), (H["rp"][1:] - H["rp"][:-1]).long(), output_size=nnz)
    want = torch.zeros(m, dtype=torch.float64, device="cuda").index_add_(0, rows, H["v"])
    scale = torch.zeros(m, dtype=torch.float64, device="cuda").index_add_(0, rows, H["v"].abs())
    ones = torch.ones(H["n"], dtype=torch.float64, device="cuda")
    zeros = torch.zeros(m, dtype=torch.float64, device="cuda")
    for strat in spmv_acc_amd.HOT_STRATEGIES:
        y = _spmv(torch, H, strat, 1.0, 0.0, ones, zeros)
        err = ((y - want).abs() / scale.clamp_min(1e-300)).max().item()
        assert err <= SCALED_TOL, (strat, err)


def test_full_size_linearity_and_beta(torch_dev, hardesty):
    """A(a*x1 + x2) = a*A x1 + A x2 and y = alpha*A*x + beta*y0 decomposes as alpha*(A x) + beta*y0."""
    torch = torch_dev
    H = hardesty
    g = torch.Generator(device="cuda")
    g.manual_seed(2)
    x2 = torch.rand(H["n"], generator=g, device="cuda", dtype=torch.float64) - 0.5
    zeros = torch.zeros(H["m"], dtype=torch.float64, device="cuda")
    for strat in ("adaptive", "flat", "line_enhance"):
        ax1 = _spmv(torch, H, strat, 1.0, 0.0, H["x"], zeros)
        ax2 = _spmv(torch, H, strat, 1.0, 0.0, x2, zeros)
        both = _spmv(torch, H, strat, 1.0, 0.0, 3.0 * H["x"] + x2, zeros)
        scale = (3.0 * ax1.abs() + ax2.abs()).clamp_min(1e-30)
        assert (((both - (3.0 * ax1 + ax2)).abs() / scale).max().item()) <= 1e-9, strat
        full = _spmv(torch, H, strat, 0.5, -2.0, H["x"], H["y0"])
        want = 0.5 * ax1 - 2.0 * H["y0"]
        scale = (0.5 * ax1.abs() + 2.0 * H["y0"].abs()).clamp_min(1e-30)
        assert (((full - want).abs() / scale).max().item()) <= 1e-12, strat


def test_full_size_sample_rows_vs_oracle(torch_dev, oracle, hardesty):
    """The first 200k rows of the full-size run against the CPU oracle (the oracle finishes in < 1 s)."""
    torch = torch_dev
    H = hardesty
    k = 200_000
    rp = H["rp"][: k + 1].cpu().numpy()
    e = int(rp[-1])
    ci, v = H["ci"][:e].cpu().numpy(), H["v"][:e].cpu().numpy()
    x, y0 = H["x"].cpu().numpy(), H["y0"][:k].cpu().numpy()
    ref = oracle.host_spmv(1.0, 1.0, rp, ci, v, x, y0)
    for strat in spmv_acc_amd.HOT_STRATEGIES:
        y = _spmv(torch, H, strat, 1.0, 1.0, H["x"], H["y0"])[:k].cpu().numpy()
        err = oracle.scaled_error(y, ref, 1.0, 1.0, rp, ci, v, x, y0)
        assert err <= SCALED_TOL, (strat, err)
        assert oracle.verify_y(y, ref)[2] == 0, strat


# ---- the C++ surface the reference's executables link against ----------------------------------------------------------
def test_cxx_api_driver(torch_dev, oracle, tmp_path):
    """Compiles a small C++ program against include/api/spmv.h + the per-strategy headers at the
    reference's include paths, links libspmv_acc.so and runs sparse_csr_spmv / the L1 wrappers."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "api_driver")
    libdir = os.path.dirname(spmv_acc_amd.LIB_PATH)
    subprocess.run([hipcc, "-O2", "-std=c++14", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cxx", "api_driver.cpp"), "-L", libdir, "-lspmv_acc",
                    f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    rowptr, cols, vals = synth.random_csr(4000, 4000, 9, seed=21, kind="powerlaw")
    rng = np.random.default_rng(6)
    x, y0 = rng.standard_normal(4000), rng.standard_normal(4000)
    inp = str(tmp_path / "in.bin")
    with open(inp, "wb") as f:
        np.array([4000, 4000, int(rowptr[-1])], dtype=np.int32).tofile(f)
        rowptr.tofile(f)
        cols.tofile(f)
        vals.tofile(f)
        x.tofile(f)
        y0.tofile(f)
    outp = str(tmp_path / "out.bin")
    subprocess.run([exe, inp, outp], check=True)
    ys = np.fromfile(outp, dtype=np.float64).reshape(-1, 4000)
    assert ys.shape[0] >= 13
    for k, y in enumerate(ys):
        check(oracle, y, 1.0, 1.0, rowptr, cols, vals, x, y0, ("cxx", k))


# ---- streams and graphs ---------------------------------------------------------------------------------------------------
def test_stream_and_hipgraph_capture(torch_dev, oracle, hiplib):
    """Steady-state calls are launches only: they run on a caller-chosen stream and capture into a hipGraph
    (plan built beforehand); replays reproduce the eager result bit for bit."""
    torch = torch_dev
    rowptr, cols, vals = synth.random_csr(50000, 50000, 11, seed=31, kind="powerlaw")
    m = n = 50000
    nnz = int(rowptr[-1])
    rng = np.random.default_rng(2)
    x, y0 = rng.standard_normal(n), rng.standard_normal(m)
    drp, dci, dv, dx, dy0 = (dev(torch, a) for a in (rowptr, cols, vals, x, y0))
    ref = oracle.host_spmv(1.0, 1.0, rowptr, cols, vals, x, y0)
    side = torch.cuda.Stream()
    try:
        hiplib.spmv_acc_set_stream(side.cuda_stream)
        for strat in ("adaptive", "flat", "line_enhance", "adaptive_plus"):
            dy = dy0.clone()
            # (steady state: the calls before a plan settles are served by its rule twin, the ones after by the timed choices -- round 6 -- so the
            # eager result the replays are compared with is taken once the plan has settled)
            for _ in range(60):
                dy = dy0.clone()
                with torch.cuda.stream(side):
                    spmv_acc_amd.csr_spmv(1.0, 1.0, m, n, nnz, drp, dci, dv, dx, dy, strategy=strat, h_rowptr=rowptr)  # builds the plan
                side.synchronize()
                if spmv_acc_amd.query_plan(drp, m)["settled"]:
                    break
            dy = dy0.clone()
            with torch.cuda.stream(side):
                spmv_acc_amd.csr_spmv(1.0, 1.0, m, n, nnz, drp, dci, dv, dx, dy, strategy=strat, h_rowptr=rowptr)
            side.synchronize()
            eager = dy.cpu().numpy()
            assert oracle.scaled_error(eager, ref, 1.0, 1.0, rowptr, cols, vals, x, y0) <= SCALED_TOL, strat
            static_y = dy0.clone()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                spmv_acc_amd.csr_spmv(1.0, 1.0, m, n, nnz, drp, dci, dv, dx, static_y, strategy=strat, h_rowptr=rowptr)
            for _ in range(3):
                static_y.copy_(dy0)
                g.replay()
                torch.cuda.synchronize()
                assert np.array_equal(static_y.cpu().numpy(), eager), strat
    finally:
        hiplib.spmv_acc_set_stream(None)
        spmv_acc_amd.release_plans(drp)


# ---- device form of the row-block analysis -----------------------------------------------------------------------------------
def test_device_analysis_matches_reference_goldens(torch_dev):
    """k_analyze.hip against tables produced by the REFERENCE's own csr_adaptive_plus_analyze.cpp (bit-exact)."""
    torch = torch_dev
    g = np.load(os.path.join(GOLD, "analysis_cases.npz"))
    for name in g["names"]:
        rp = g[f"{name}__rowptr"]
        m, nnz = rp.size - 1, int(rp[-1])
        drp = dev(torch, rp)
        for k, (threads, vec, min_nnz) in enumerate(g["params"]):
            blocks, bp, fbr = spmv_acc_amd.adaptive_plus_analyze_device(drp, m, nnz, int(min_nnz), int(threads), int(vec))
            assert np.array_equal(bp.cpu().numpy(), g[f"{name}__{k}__bp"]), (name, k)
            assert np.array_equal(fbr.cpu().numpy(), g[f"{name}__{k}__fbr"]), (name, k)
            assert blocks == g[f"{name}__{k}__bp"].size - 1


def test_device_analysis_matches_host_form_random(torch_dev, oracle):
    torch = torch_dev
    rng = np.random.default_rng(17)
    for trial in range(60):
        m = int(rng.integers(1, 60000))
        kind = trial % 5
        if kind == 0:
            lens = rng.integers(0, 12, m)
        elif kind == 1:
            lens = np.minimum((rng.pareto(1.2, m) * 3).astype(np.int64), 30000)
        elif kind == 2:
            lens = rng.integers(0, 3, m)
            lens[rng.integers(0, m, 5)] = rng.integers(2000, 40000, 5)
        elif kind == 3:
            lens = rng.integers(0, 700, min(m, 5000))
        else:
            lens = np.zeros(m, dtype=np.int64)
            lens[rng.integers(0, m, max(1, m // 50))] = rng.integers(1, 9000, max(1, m // 50))
        m = lens.size
        rp = np.zeros(m + 1, dtype=np.int32)
        np.cumsum(lens, out=rp[1:])
        drp = dev(torch, rp)
        for threads, vec, min_nnz in ((256, 1, 1024), (256, 4, 1024), (512, 16, 2048), (1024, 64, 4096)):
            want = oracle.adaptive_plus_analyze(rp, min_nnz, threads, vec)
            blocks, bp, fbr = spmv_acc_amd.adaptive_plus_analyze_device(drp, m, int(rp[-1]), min_nnz, threads, vec)
            assert blocks == want[0], (trial, threads, vec)
            assert np.array_equal(bp.cpu().numpy(), want[1]), (trial, threads, vec)
            assert np.array_equal(fbr.cpu().numpy(), want[2]), (trial, threads, vec)


def test_device_analysis_full_size(torch_dev, oracle, hardesty):
    """8.2 M rows: device tables against the host form."""
    H = hardesty
    rp = H["rp"].cpu().numpy()
    want = oracle.adaptive_plus_analyze(rp, 1024, 256, 1)
    blocks, bp, fbr = spmv_acc_amd.adaptive_plus_analyze_device(H["rp"], H["m"], H["nnz"], 1024, 256, 1)
    assert blocks == want[0]
    assert np.array_equal(bp.cpu().numpy(), want[1]) and np.array_equal(fbr.cpu().numpy(), want[2])


# ---- the other BASELINE workload families --------------------------------------------------------------------------------------
def test_rmat_power_law_parity(torch_dev, oracle):
    """configs[3] family at a size the oracle finishes in a second: R-MAT scale 18 (hub rows of tens of thousands of
    non-zeros, empty rows), every hot strategy against the oracle."""
    torch = torch_dev
    m, n, nnz, rp, ci, v = synth.rmat_torch(18, device="cuda", seed=0xC4)
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    x = torch.rand(n, generator=g, device="cuda", dtype=torch.float64) * 2 - 1
    y0 = torch.rand(m, generator=g, device="cuda", dtype=torch.float64) * 2 - 1
    hrp, hci, hv, hx, hy0 = (t.cpu().numpy() for t in (rp, ci, v, x, y0))
    assert np.diff(hrp).max() > 10_000 and np.diff(hrp).min() == 0
    ref = oracle.host_spmv(1.0, 1.0, hrp, hci, hv, hx, hy0)
    for strat in spmv_acc_amd.HOT_STRATEGIES:
        y = y0.clone()
        spmv_acc_amd.csr_spmv(1.0, 1.0, m, n, nnz, rp, ci, v, x, y, strategy=strat)
        torch.cuda.synchronize()
        err = oracle.scaled_error(y.cpu().numpy(), ref, 1.0, 1.0, hrp, hci, hv, hx, hy0)
        assert err <= SCALED_TOL, (strat, err)
        assert oracle.verify_y(y.cpu().numpy(), ref)[2] == 0, strat
    spmv_acc_amd.release_plans(rp)
    # the balance probe sends line_enhance / line to the row-block-plus kernel (until round 5 a tunable could send them to flat's nnz-cut tiles instead)
    # (adaptive times every family on the matrix and so builds both plans)
    for strat in ("line_enhance", "line"):
        y = y0.clone()
        spmv_acc_amd.csr_spmv(1.0, 1.0, m, n, nnz, rp, ci, v, x, y, strategy=strat)
        torch.cuda.synchronize()
        assert oracle.scaled_error(y.cpu().numpy(), ref, 1.0, 1.0, hrp, hci, hv, hx, hy0) <= SCALED_TOL, strat
    info = spmv_acc_amd.query_plan(rp, m)
    assert info["plus_blocks"] > 0 and info["flat_tiles"] <= 0, info
    spmv_acc_amd.release_plans(rp)


def test_banded_shard_closed_form(torch_dev):
    """configs[4] family: a 4 M-row shard of the banded matrix in the middle of a 32 M-row problem (global column
    ids).  With x = 1 every interior row sums to sum_off sign/(1+|off|), known in closed form."""
    torch = torch_dev
    rows, total, first = 4_000_000, 32_000_000, 12_000_000
    rp, ci, v = synth.banded_torch(rows, first_row=first, total_rows=total, device="cuda")
    nnz = int(rp[-1].item())
    assert nnz == 8 * rows and int(ci.max().item()) == first + rows - 1 + 3
    x = torch.ones(total, dtype=torch.float64, device="cuda")
    offs = np.arange(-4, 4)
    r = np.arange(first, first + 8)
    want8 = np.array([np.sum(np.where((ri + offs) % 2 == 0, 1.0, -1.0) / (1.0 + np.abs(offs))) for ri in r])
    for strat in ("adaptive", "flat", "line_enhance", "adaptive_plus"):
        y = torch.zeros(rows, dtype=torch.float64, device="cuda")
        spmv_acc_amd.csr_spmv(1.0, 0.0, rows, total, nnz, rp, ci, v, x, y, strategy=strat)
        torch.cuda.synchronize()
        got = y.cpu().numpy()
        assert np.allclose(got[:8], want8, rtol=0, atol=1e-14), strat
        # rows alternate between two values (row parity): check the whole shard against the period-2 pattern
        assert np.allclose(got[0::2], want8[0], rtol=0, atol=1e-14) and np.allclose(got[1::2], want8[1], rtol=0, atol=1e-14), strat
    spmv_acc_amd.release_plans(rp)


def test_bench_contract_small(torch_dev):
    """bench.py --full prints ONE JSON line with the driver's keys + roofline + cpu_baseline (reduced scale for speed)."""
    import json
    import sys

    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "5", "--warmup", "2", "--scale", "0.02", "--full",
                          "--cpu-seconds", "1"], capture_output=True, text=True, check=True).stdout.strip().splitlines()
    d = json.loads(out[-1])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 5 and d["dtype"] == "f64" and d["vs_baseline"] is None
    assert set(d["roofline"]) >= {"bound", "achieved", "peak", "unit", "frac", "traffic"} and d["roofline"]["bound"] == "hbm"
    assert set(d["cpu_baseline"]) >= {"value", "unit", "cores", "kind", "sample"} and d["cpu_baseline"]["kind"] == "port"
    assert "workload" in d["config"] and d["value"] > 0


# ---- error paths and plan cache ---------------------------------------------------------------------------------------------------
def test_error_codes_and_degenerate_shapes(torch_dev, hiplib, oracle):
    torch = torch_dev
    rowptr, cols, vals = synth.random_csr(100, 100, 4, seed=2)
    nnz = int(rowptr[-1])
    drp, dci, dv = dev(torch, rowptr), dev(torch, cols), dev(torch, vals)
    dx = torch.ones(100, dtype=torch.float64, device="cuda")
    dy = torch.ones(100, dtype=torch.float64, device="cuda")
    L = hiplib
    L.spmv_acc_clear_error()
    # m <= 0: nothing to do, no error (the reference would launch an empty grid)
    L.spmv_acc_csr_spmv_strategy(9, 0, 1.0, 1.0, 0, 100, 0, None, drp.data_ptr(), dci.data_ptr(), dv.data_ptr(), dx.data_ptr(), dy.data_ptr())
    assert L.spmv_acc_last_error() == 0
    # null y / unknown strategy / null colindex with nnz > 0 are reported, nothing is launched
    L.spmv_acc_csr_spmv_strategy(9, 0, 1.0, 1.0, 100, 100, nnz, None, drp.data_ptr(), dci.data_ptr(), dv.data_ptr(), dx.data_ptr(), None)
    assert L.spmv_acc_last_error() == 2
    L.spmv_acc_clear_error()
    L.spmv_acc_csr_spmv_strategy(99, 0, 1.0, 1.0, 100, 100, nnz, None, drp.data_ptr(), dci.data_ptr(), dv.data_ptr(), dx.data_ptr(), dy.data_ptr())
    assert L.spmv_acc_last_error() == 5
    L.spmv_acc_clear_error()
    L.spmv_acc_csr_spmv_strategy(9, 0, 1.0, 1.0, 100, 100, nnz, None, drp.data_ptr(), None, dv.data_ptr(), dx.data_ptr(), dy.data_ptr())
    assert L.spmv_acc_last_error() == 2
    L.spmv_acc_clear_error()
    assert L.spmv_acc_break_points(None, 10, 10, 1024, None, 2) == 2
    L.spmv_acc_clear_error()
    torch.cuda.synchronize()
    assert torch.all(dy == 1.0)  # untouched by the refused calls
    spmv_acc_amd.release_plans()
    # n == 0 columns with an all-empty matrix: y = beta * y
    rp0 = torch.zeros(51, dtype=torch.int32, device="cuda")
    y = torch.full((50,), 3.0, dtype=torch.float64, device="cuda")
    spmv_acc_amd.csr_spmv(2.0, 0.5, 50, 0, 0, rp0, None, None, None, y, strategy="adaptive")
    torch.cuda.synchronize()
    assert torch.all(y == 1.5)
    spmv_acc_amd.release_plans()


def test_plan_cache_lifecycle(torch_dev, hiplib, oracle):
    torch = torch_dev
    spmv_acc_amd.release_plans()
    assert hiplib.spmv_acc_cached_plans() == 0
    rowptr, cols, vals = synth.random_csr(5000, 5000, 6, seed=4)
    rng = np.random.default_rng(0)
    x, y0 = rng.standard_normal(5000), rng.standard_normal(5000)
    drp, dci, dv, dx = (dev(torch, a) for a in (rowptr, cols, vals, x))
    nnz = int(rowptr[-1])
    for strat in ("flat", "adaptive_plus", "adaptive"):
        dy = dev(torch, y0)
        spmv_acc_amd.csr_spmv(1.0, 1.0, 5000, 5000, nnz, drp, dci, dv, dx, dy, strategy=strat)
        spmv_acc_amd.prepare(5000, 5000, nnz, drp, dci, dv, dx, strategy=strat)  # (whatever the first call's tuning budget left open)
    torch.cuda.synchronize()
    assert hiplib.spmv_acc_cached_plans() == 1  # one matrix, one plan shared by the strategies
    info = spmv_acc_amd.query_plan(drp, 5000)
    # (small matrices time the 1024- and the 2048-non-zero tile and keep the faster)
    assert info["flat_tiles"] in (-(-nnz // 2048), -(-nnz // 1024)) and info["plus_blocks"] > 0 and info["adaptive_branch"] in (2, 3)
    assert info["stream_policy"] in (0, 1, 3)  # timed once when the plan was built
    # the values may change freely under a plan (only the structure is cached)
    dv.mul_(2.0)
    dy = dev(torch, y0)
    spmv_acc_amd.csr_spmv(1.0, 1.0, 5000, 5000, nnz, drp, dci, dv, dx, dy, strategy="flat")
    torch.cuda.synchronize()
    ref = oracle.host_spmv(1.0, 1.0, rowptr, cols, 2.0 * vals, x, y0)
    assert oracle.scaled_error(dy.cpu().numpy(), ref, 1.0, 1.0, rowptr, cols, 2.0 * vals, x, y0) <= SCALED_TOL
    spmv_acc_amd.release_plans(drp)
    assert hiplib.spmv_acc_cached_plans() == 0 and spmv_acc_amd.query_plan(drp, 5000) is None


def test_ragged_array_end_every_residue(torch_dev, oracle):
    """nnz mod 4 = 0..3 with the last row block / tile ending exactly at nnz: the wide-load fast path must hand the
    ragged end to the guarded path (tile_stage.hpp: round_up(hi, 4) <= nnz) and results stay in parity."""
    torch = torch_dev
    rng = np.random.default_rng(77)
    for extra in range(8):
        lens = np.full(700, 5, dtype=np.int64)
        lens[-1] = 5 + extra  # nnz = 3500 + extra
        rowptr, cols, vals = synth.csr_from_row_lengths(lens, 700, rng)
        nnz = int(rowptr[-1])
        x, y0 = rng.standard_normal(700), rng.standard_normal(700)
        drp, dci, dv, dx = dev(torch, rowptr), dev(torch, cols), dev(torch, vals), dev(torch, x)
        for strat in spmv_acc_amd.HOT_STRATEGIES:
            dy = dev(torch, y0)
            spmv_acc_amd.csr_spmv(1.0, 1.0, 700, 700, nnz, drp, dci, dv, dx, dy, strategy=strat)
            torch.cuda.synchronize()
            ref = oracle.host_spmv(1.0, 1.0, rowptr, cols, vals, x, y0)
            err = oracle.scaled_error(dy.cpu().numpy(), ref, 1.0, 1.0, rowptr, cols, vals, x, y0)
            assert err <= SCALED_TOL, (strat, extra, err)
        spmv_acc_amd.release_plans(drp)


def test_stream_policies_are_bitwise_equivalent(torch_dev, hiplib):
    """The cache policy of the stream loads (picked by timing at plan time) must never change a bit of the result."""
    torch = torch_dev
    rowptr, cols, vals = synth.random_csr(30000, 30000, 14, seed=55, kind="powerlaw")
    rng = np.random.default_rng(9)
    x, y0 = rng.standard_normal(30000), rng.standard_normal(30000)
    drp, dci, dv, dx = (dev(torch, a) for a in (rowptr, cols, vals, x))
    nnz = int(rowptr[-1])
    try:
        for strat in ("line_enhance", "flat", "adaptive_plus"):
            outs = []
            for policy in (0, 1, 2, 3):
                assert hiplib.spmv_acc_set_tunable(b"stream_plain", policy) == 0
                if policy == 0:  # every OTHER timed choice settled first (they may change the order of the sums; the cache policy may not)
                    spmv_acc_amd.prepare(30000, 30000, nnz, drp, dci, dv, dx, strategy=strat, beta=-1.5)
                dy = dev(torch, y0)
                spmv_acc_amd.csr_spmv(0.75, -1.5, 30000, 30000, nnz, drp, dci, dv, dx, dy, strategy=strat)
                torch.cuda.synchronize()
                outs.append(dy.cpu().numpy())
            for o in outs[1:]:
                assert np.array_equal(o, outs[0]), strat
    finally:
        hiplib.spmv_acc_reset_tunables()
        spmv_acc_amd.release_plans(drp)


def test_measurement_switches_keep_parity(torch_dev, oracle, hiplib):
    """Every A/B switch of the engine (tile sizes, block orders, staging forms, analysis forms) is a speed matter only."""
    torch = torch_dev
    rowptr, cols, vals = synth.random_csr(40000, 40000, 9, seed=91, kind="powerlaw")
    rng = np.random.default_rng(4)
    x, y0 = rng.standard_normal(40000), rng.standard_normal(40000)
    drp, dci, dv, dx = (dev(torch, a) for a in (rowptr, cols, vals, x))
    nnz = int(rowptr[-1])
    ref = oracle.host_spmv(1.0, 1.0, rowptr, cols, vals, x, y0)
    variants = MEASUREMENT_SWITCHES  # (tests/special_values.py: tests/test_gpu_special_values.py runs the same inventory on poisoned data)
    try:
        for strat, knobs in variants:
            hiplib.spmv_acc_reset_tunables()
            for k, v in knobs.items():
                assert hiplib.spmv_acc_set_tunable(k.encode(), v) == 0, k
            spmv_acc_amd.release_plans(drp)  # analysis-level switches take effect when the plan is (re)built
            dy = dev(torch, y0)
            spmv_acc_amd.csr_spmv(1.0, 1.0, 40000, 40000, nnz, drp, dci, dv, dx, dy, strategy=strat)
            torch.cuda.synchronize()
            err = oracle.scaled_error(dy.cpu().numpy(), ref, 1.0, 1.0, rowptr, cols, vals, x, y0)
            assert err <= SCALED_TOL, (strat, knobs, err)
        assert hiplib.spmv_acc_set_tunable(b"no_such_knob", 1) == -1
    finally:
        hiplib.spmv_acc_reset_tunables()
        spmv_acc_amd.release_plans(drp)


def test_randomised_shapes_all_strategies(torch_dev, oracle):
    """Fuzz: 160 random (valid) CSR matrices -- sizes, row-length laws, column laws, ragged nnz, unaligned views,
    alpha/beta -- through every hot strategy, against the oracle."""
    torch = torch_dev
    # soak runs: SPMV_ACC_FUZZ_CASES / SPMV_ACC_FUZZ_SEED / SPMV_ACC_FUZZ_ALL=1 (every strategy name, not only the hot ones)
    cases = int(os.environ.get("SPMV_ACC_FUZZ_CASES", "160"))
    rng = np.random.default_rng(int(os.environ.get("SPMV_ACC_FUZZ_SEED", "20261003")))
    strategies = ALL if os.environ.get("SPMV_ACC_FUZZ_ALL") == "1" else spmv_acc_amd.HOT_STRATEGIES
    for case in range(cases):
        m = int(rng.choice([1, 2, 3, 63, 64, 65, 255, 257, 1000, 4099, 20011]))
        n = int(rng.choice([1, 2, 64, 1000, 5000, 30000]))
        if cases > 160 and case % 7 == 3:  # soak only: arbitrary sizes
            m, n = int(rng.integers(1, 60000)), int(rng.integers(1, 80000))
        law = case % 8
        if law == 0:
            lens = rng.integers(0, 9, m)
        elif law == 1:
            lens = rng.integers(0, 3, m)
        elif law == 2:
            lens = np.minimum((rng.pareto(1.0, m) * 4).astype(np.int64), 60000)
        elif law == 3:
            lens = np.zeros(m, dtype=np.int64)
            lens[rng.integers(0, m, max(1, m // 40))] = rng.integers(1, 5000, max(1, m // 40))
        elif law == 4:
            lens = np.full(m, int(rng.integers(1, 70)))
        elif law == 5:
            lens = rng.integers(200, 900, m) if m <= 300 else rng.integers(0, 40, m)
        elif law == 6:
            lens = rng.integers(0, 6, m)
            lens[-1] = int(rng.integers(0, 9000))  # a long last row: the arrays end inside a wide-load group
        else:
            lens = rng.integers(0, 6, m)
            lens[0] = int(rng.integers(2048, 12000))  # a long first row
        rowptr = np.zeros(m + 1, dtype=np.int64)
        np.cumsum(lens, out=rowptr[1:])
        nnz = int(rowptr[-1])
        if nnz > 3_000_000:
            continue
        rowptr = rowptr.astype(np.int32)
        cols = rng.integers(0, n, nnz).astype(np.int32)
        if case % 3 == 0 and nnz:  # clustered columns
            cols = np.clip((np.repeat(np.arange(m), lens) * n // max(m, 1)) + rng.integers(-8, 9, nnz), 0, n - 1).astype(np.int32)
        vals = rng.standard_normal(nnz)
        x, y0 = rng.standard_normal(n), rng.standard_normal(m)
        alpha, beta = [(1.0, 1.0), (1.0, 0.0), (-0.5, 2.0), (0.0, 1.0)][case % 4]
        shift = case % 5 == 4  # unaligned views of colindex / values
        if shift:
            pc = torch.zeros(nnz + 1, dtype=torch.int32, device="cuda")
            pv = torch.zeros(nnz + 1, dtype=torch.float64, device="cuda")
            pc[1:] = dev(torch, cols)
            pv[1:] = dev(torch, vals)
            dci, dv = pc[1:], pv[1:]
        else:
            dci, dv = dev(torch, cols), dev(torch, vals)
        drp, dx = dev(torch, rowptr), dev(torch, x)
        ref = oracle.host_spmv(alpha, beta, rowptr, cols, vals, x, y0)
        for strat in strategies:
            dy = dev(torch, y0)
            spmv_acc_amd.csr_spmv(alpha, beta, m, n, nnz, drp, dci, dv, dx, dy, strategy=strat)
            torch.cuda.synchronize()
            err = oracle.scaled_error(dy.cpu().numpy(), ref, alpha, beta, rowptr, cols, vals, x, y0)
            assert err <= SCALED_TOL, (case, strat, m, n, nnz, alpha, beta, shift, err)
        spmv_acc_amd.release_plans(drp)


def test_flat_finish_and_carry_modes(torch_dev, oracle, hiplib):
    """flat folds rows cut by a tile boundary in one of two ways, chosen at plan time (kernels.hpp kFlatFinish): through
    head/tail carries and a fix-up kernel, or -- legal only when no row overhangs its tile by more than 128 non-zeros --
    by letting tiles finish short overhangs themselves (the engine times both per matrix; `flat_finish` pins one).  Both modes, and every flat_npt (tile size), against the oracle; the row
    lengths put cut rows at overhangs 1..127, exactly 128, and 129+ ."""
    torch = torch_dev
    rng = np.random.default_rng(77)
    n = 6000
    short = rng.integers(0, 96, size=9000)                       # overhangs < 128 everywhere -> finishing mode
    exact = np.concatenate([[2048 - 40, 40 + 128], short])       # a row ending exactly 128 past tile 0 -> still finishing
    over = np.concatenate([[2048 - 40, 40 + 129], short])        # 129 past -> carry mode
    long_ = np.concatenate([short[:3000], [7000], short[3000:]])  # a row spanning several tiles -> carry mode
    for name, lens, must_carry in (("short", short, 0), ("exact", exact, 0), ("over", over, 1), ("long", long_, 1)):
        rowptr = np.zeros(lens.size + 1, dtype=np.int32)
        np.cumsum(lens, out=rowptr[1:])
        nnz = int(rowptr[-1])
        cols = rng.integers(0, n, size=nnz).astype(np.int32)
        vals = rng.standard_normal(nnz)
        x, y0 = rng.standard_normal(n), rng.standard_normal(lens.size)
        m = lens.size
        for npt, finish in ((8, 1), (8, 0), (8, -1), (4, 1), (16, 1), (16, 0)):
            assert hiplib.spmv_acc_set_tunable(b"flat_npt", npt) == 0
            assert hiplib.spmv_acc_set_tunable(b"flat_finish", finish) == 0  # -1: the engine times both forms
            try:
                drp, dci, dv, dx, dy = (dev(torch, a) for a in (rowptr, cols, vals, x, y0))
                spmv_acc_amd.csr_spmv(0.75, -1.5, m, n, nnz, drp, dci, dv, dx, dy, strategy="flat", h_rowptr=rowptr)
                torch.cuda.synchronize()
                info = spmv_acc_amd.query_plan(drp, m)
                got = dy.cpu().numpy()
                spmv_acc_amd.release_plans(drp)
            finally:
                hiplib.spmv_acc_reset_tunables()
            if npt == 8 and finish >= 0:
                assert info["flat_fixup"] == (1 if (must_carry or finish == 0) else 0), (name, finish, info)
            if must_carry and (npt == 8 or name == "long"):  # 'over' is built around the 2048-non-zero tile
                assert info["flat_fixup"] == 1, (name, info)
            check(oracle, got, 0.75, -1.5, rowptr, cols, vals, x, y0, f"flat-{name}-npt{npt}-finish{finish}")


def test_largest_int32_nnz(torch_dev):
    """Maximum size (include/spmv_acc.h: nnz <= INT_MAX - 65536 per call): 268,427,263 interior rows of the configs[4]
    banded matrix = 2,147,418,104 non-zeros, one below-the-limit call per strategy.  x[j] = (j mod 7) - 3 makes every
    gather index matter; y is then a closed-form pattern of period 14 in the global row id.  One more non-zero's worth of
    rows must be refused (SPMV_ACC_ERR_TOO_LARGE) without touching y."""
    torch = torch_dev
    first, k = 8, 8
    m = (2**31 - 1 - 65536) // k
    n = first + m + 8
    rp, ci, v = synth.banded_interior_torch(m, first, device="cuda")
    nnz = m * k
    assert int(rp[-1].item()) == nnz and int(ci[-1].item()) == first + m - 1 + 3 and int(ci[0].item()) == first - 4
    x = ((torch.arange(n, device="cuda", dtype=torch.int64) % 7) - 3).to(torch.float64)
    offs = np.arange(-4, 4)
    pat = np.array([np.sum(np.where((g + offs) % 2 == 0, 1.0, -1.0) / (1.0 + np.abs(offs)) * (((g + offs) % 7) - 3.0))
                    for g in range(first, first + 14)])
    want = torch.from_numpy(pat).cuda()[torch.arange(m, device="cuda", dtype=torch.int64) % 14]
    for strat in ("adaptive", "flat", "line_enhance", "adaptive_plus", "default"):
        y = torch.full((m,), 7.0, dtype=torch.float64, device="cuda")
        spmv_acc_amd.csr_spmv(1.0, 0.0, m, n, nnz, rp, ci, v, x, y, strategy=strat)
        torch.cuda.synchronize()
        err = float((y - want).abs().max().item())
        assert err <= 1e-13, (strat, err)
        del y
    spmv_acc_amd.release_plans(rp)
    del want, ci, v
    # one row more than fits: rowptr alone decides (the arrays are never dereferenced)
    rp2 = (torch.arange(m + 10000 + 1, device="cuda", dtype=torch.int64) * k).clamp(max=2**31 - 1).to(torch.int32)
    y = torch.full((16,), 7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(spmv_acc_amd.SpmvAccError):
        spmv_acc_amd.csr_spmv(1.0, 0.0, m + 10000, n, -1, rp2, rp2, x, x, y, strategy="adaptive")
    torch.cuda.synchronize()
    assert float(y.min().item()) == 7.0


def test_opt_in_validation_refuses_corrupt_matrices(torch_dev, oracle, hiplib):
    """Tunable `validate` (or SPMV_ACC_TUNABLES=validate=1): rowptr / colindex of a new matrix are checked on the device
    before the first launch.  A consistent matrix computes as usual; a column index outside [0, n), a decreasing rowptr or
    an nnz that disagrees with rowptr[m] is refused with SPMV_ACC_ERR_BAD_ARGUMENT and y is left untouched -- no kernel
    reads through the bad index."""
    torch = torch_dev
    rowptr, cols, vals = synth.random_csr(3000, 2500, 7, seed=5, kind="uniform")
    rng = np.random.default_rng(6)
    x, y0 = rng.standard_normal(2500), rng.standard_normal(3000)
    m, n, nnz = 3000, 2500, int(rowptr[-1])
    assert hiplib.spmv_acc_set_tunable(b"validate", 1) == 0
    try:
        for strat in ("adaptive", "flat", "adaptive_plus", "default"):
            got = run(torch, strat, 1.0, 1.0, rowptr, cols, vals, x, y0)
            check(oracle, got, 1.0, 1.0, rowptr, cols, vals, x, y0, f"validate-ok-{strat}")
        bad_col = cols.copy(); bad_col[nnz // 2] = n          # one past the last column
        neg_col = cols.copy(); neg_col[7] = -1
        bad_rp = rowptr.copy(); bad_rp[100], bad_rp[101] = rowptr[101], rowptr[100] - 1 if rowptr[100] > 0 else 0
        bad_rp = rowptr.copy(); bad_rp[1500] = rowptr[1501] + 3  # rowptr[1500] > rowptr[1501]
        cases = {"col == n": (rowptr, bad_col, nnz), "col < 0": (rowptr, neg_col, nnz), "rowptr decreases": (bad_rp, cols, nnz),
                 "nnz mismatch": (rowptr, cols, nnz - 1)}
        for tag, (rp_, ci_, nnz_) in cases.items():
            for strat in ("adaptive", "flat"):
                drp, dci, dv, dx, dy = dev(torch, rp_), dev(torch, ci_), dev(torch, vals), dev(torch, x), dev(torch, y0)
                with pytest.raises(spmv_acc_amd.SpmvAccError, match="validation"):
                    spmv_acc_amd.csr_spmv(1.0, 1.0, m, n, nnz_, drp, dci, dv, dx, dy, strategy=strat)
                with pytest.raises(spmv_acc_amd.SpmvAccError, match="validation"):  # the verdict is kept with the plan
                    spmv_acc_amd.csr_spmv(1.0, 1.0, m, n, nnz_, drp, dci, dv, dx, dy, strategy=strat)
                torch.cuda.synchronize()
                assert np.array_equal(dy.cpu().numpy(), y0), (tag, strat)
                spmv_acc_amd.release_plans(drp)
    finally:
        hiplib.spmv_acc_reset_tunables()


def test_host_staging_then_spmv(torch_dev, oracle, hiplib):
    """spmv_acc_stage_csr (north_star: 'host-side C++ stages CSR arrays with pinned hipMemcpyAsync'): host arrays -- writable
    numpy memory that can be pinned in place, and a read-only buffer that cannot and takes the bounce-buffer route -- arrive
    intact: an SpMV on the staged device pointers matches the oracle; NULL host pointers skip their array."""
    import ctypes

    torch = torch_dev
    rowptr, cols, vals = synth.random_csr(20011, 9000, 9, seed=17, kind="powerlaw")
    rng = np.random.default_rng(18)
    x, y0 = rng.standard_normal(9000), rng.standard_normal(20011)
    m, n, nnz = 20011, 9000, int(rowptr[-1])
    ref = oracle.host_spmv(1.0, 1.0, rowptr, cols, vals, x, y0)
    ro_vals = np.frombuffer(vals.tobytes(), dtype=np.float64)  # read-only memory
    assert not ro_vals.flags.writeable
    for hv in (vals, ro_vals):
        outs = [ctypes.c_void_p() for _ in range(5)]
        rc = hiplib.spmv_acc_stage_csr(m, n, nnz, rowptr.ctypes.data, cols.ctypes.data, hv.ctypes.data, x.ctypes.data, None,
                                       *[ctypes.byref(o) for o in outs])
        assert rc == 0, spmv_acc_amd.load_library().spmv_acc_last_error_string()
        d_rp, d_ci, d_v, d_x, d_y = (o.value for o in outs)
        assert d_rp and d_ci and d_v and d_x and d_y is None  # h_y was NULL: no buffer made for it
        dy = dev(torch, y0)
        hiplib.spmv_acc_csr_spmv_strategy(spmv_acc_amd.strategy_id("adaptive"), 0, 1.0, 1.0, m, n, nnz, None, d_rp, d_ci, d_v, d_x,
                                          dy.data_ptr())
        torch.cuda.synchronize()
        assert hiplib.spmv_acc_last_error() == 0
        got = dy.cpu().numpy()
        assert oracle.scaled_error(got, ref, 1.0, 1.0, rowptr, cols, vals, x, y0) <= SCALED_TOL
        hiplib.spmv_acc_release_plans(d_rp)
        for p in (d_rp, d_ci, d_v, d_x):
            assert hiplib.spmv_acc_free_device(p) == 0


def test_prepare_then_first_call_is_capturable(torch_dev, oracle, hiplib):
    """spmv_acc_prepare builds the plan (structural passes + per-matrix timings) without any y; the very first SpMV call
    afterwards is launches only: it is captured into a hipGraph here, and the replay matches the oracle."""
    torch = torch_dev
    rowptr, cols, vals = synth.random_csr(30000, 30000, 13, seed=41, kind="powerlaw")
    m = n = 30000
    nnz = int(rowptr[-1])
    rng = np.random.default_rng(42)
    x, y0 = rng.standard_normal(n), rng.standard_normal(m)
    ref = oracle.host_spmv(1.0, 1.0, rowptr, cols, vals, x, y0)
    side = torch.cuda.Stream()
    try:
        hiplib.spmv_acc_set_stream(side.cuda_stream)
        for strat in ("adaptive", "flat", "line_enhance", "adaptive_plus", "default", "vector_row"):
            drp, dci, dv, dx = (dev(torch, a) for a in (rowptr, cols, vals, x))  # fresh buffers: no plan yet
            assert spmv_acc_amd.query_plan(drp, m) is None
            ms = spmv_acc_amd.prepare(m, n, nnz, drp, dci, dv, dx, strategy=strat)
            assert ms > 0.0 and spmv_acc_amd.query_plan(drp, m) is not None
            static_y = dev(torch, y0)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):  # the FIRST spmv call on this matrix, under capture
                spmv_acc_amd.csr_spmv(1.0, 1.0, m, n, nnz, drp, dci, dv, dx, static_y, strategy=strat)
            g.replay()
            torch.cuda.synchronize()
            err = oracle.scaled_error(static_y.cpu().numpy(), ref, 1.0, 1.0, rowptr, cols, vals, x, y0)
            assert err <= SCALED_TOL, (strat, err)
            # the other beta class (y = A x) captured straight after a preparation made at beta = 1: the cache policy of that class
            # has not been timed -- the captured call must not try to (it would synchronise inside the capture)
            y_b0 = dev(torch, y0)
            g0 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g0, stream=side):
                spmv_acc_amd.csr_spmv(1.0, 0.0, m, n, nnz, drp, dci, dv, dx, y_b0, strategy=strat)
            g0.replay()
            torch.cuda.synchronize()
            ref0 = oracle.host_spmv(1.0, 0.0, rowptr, cols, vals, x, y0)
            assert oracle.scaled_error(y_b0.cpu().numpy(), ref0, 1.0, 0.0, rowptr, cols, vals, x, y0) <= SCALED_TOL, (strat, "beta = 0 captured")
            spmv_acc_amd.release_plans(drp)
    finally:
        hiplib.spmv_acc_set_stream(None)


def test_adaptive_times_the_kernel_families(torch_dev, oracle, hiplib):
    """adaptive keeps the fastest of fixed row blocks / row-block-plus / flat, timed on the matrix (query_plan reports the family);
    `adaptive_timed` 0 decides from the rowptr samples and the balance probe alone.  Both forms, three row-length laws, parity."""
    torch = torch_dev
    rng = np.random.default_rng(55)
    m = 60000
    laws = {"even": rng.integers(20, 31, m), "halves": np.concatenate([rng.integers(30, 50, m // 2), rng.integers(3, 7, m - m // 2)]),
            "lognormal": np.minimum(np.exp(rng.normal(np.log(20.0), 1.2, m)).astype(np.int64), 20000)}
    for name, lens in laws.items():
        rowptr, cols, vals = synth.csr_from_row_lengths(lens, m, rng)
        nnz = int(rowptr[-1])
        x, y0 = rng.standard_normal(m), rng.standard_normal(m)
        ref = oracle.host_spmv(1.0, 1.0, rowptr, cols, vals, x, y0)
        for timed in (1, 0):
            assert hiplib.spmv_acc_set_tunable(b"adaptive_timed", timed) == 0
            try:
                drp, dci, dv, dx, dy = (dev(torch, a) for a in (rowptr, cols, vals, x, y0))
                spmv_acc_amd.prepare(m, m, nnz, drp, dci, dv, dx, strategy="adaptive")  # the whole comparison, up front
                spmv_acc_amd.csr_spmv(1.0, 1.0, m, m, nnz, drp, dci, dv, dx, dy, strategy="adaptive")
                torch.cuda.synchronize()
                info = spmv_acc_amd.query_plan(drp, m)
                got = dy.cpu().numpy()
                dy2 = dev(torch, y0)  # steady state: the kept family only
                spmv_acc_amd.csr_spmv(1.0, 1.0, m, m, nnz, drp, dci, dv, dx, dy2, strategy="adaptive")
                torch.cuda.synchronize()
                assert np.array_equal(dy2.cpu().numpy(), got), (name, timed)
                spmv_acc_amd.release_plans(drp)
            finally:
                hiplib.spmv_acc_reset_tunables()
            assert info["adaptive_family"] == (-1 if timed == 0 else info["adaptive_family"]) and (timed == 0 or info["adaptive_family"] in (0, 1, 2))
            if timed:
                assert info["flat_tiles"] > 0 and info["plus_blocks"] > 0, (name, info)  # every family was built and timed
            assert oracle.scaled_error(got, ref, 1.0, 1.0, rowptr, cols, vals, x, y0) <= SCALED_TOL, (name, timed)


def test_long_spans_among_short_rows(torch_dev, oracle, hiplib):
    """Rows of hundreds of non-zeros among rows of 5 (circuit-like): inside a tile such a row's span is summed by whole waves
    instead of its own 1..16 lanes (tile_stage.hpp tile_row_sum).  Span lengths around every threshold (63/64/65 products, 16 w),
    spans cut by tile boundaries, several posted spans per tile, all tile kernels and every flat tile size, against the oracle."""
    torch = torch_dev
    rng = np.random.default_rng(91)
    m = 30000
    lens = rng.integers(3, 8, m)
    special = [63, 64, 65, 100, 127, 128, 129, 255, 256, 600, 1023, 1024, 1025, 2047, 2048, 2049, 3000, 4096, 5000]
    where = rng.choice(m, size=8 * len(special), replace=False)
    lens[where] = np.tile(special, 8)
    lens[1000:1012] = 70          # twelve posted spans in one tile
    lens[5000:5003] = [2000, 2100, 64]
    rowptr, cols, vals = synth.csr_from_row_lengths(lens, m, rng)
    nnz = int(rowptr[-1])
    x, y0 = rng.standard_normal(m), rng.standard_normal(m)
    ref = oracle.host_spmv(-0.5, 2.0, rowptr, cols, vals, x, y0)
    variants = [("adaptive", {}), ("line_enhance", {}), ("adaptive_plus", {}), ("adaptive_plus", {"plus_min_nnz": 1024}),
                ("adaptive_plus", {"plus_min_nnz": 1920}), ("flat", {}), ("flat", {"flat_npt": 4}), ("flat", {"flat_npt": 16}),
                ("flat", {"flat_finish": 0}), ("line_enhance", {"rowblock_guard": 0}), ("line_enhance", {"rowblock_vec": 4}),
                ("line_enhance", {"rowblock_vec": 16}), ("line_enhance", {"rowlen": 1}), ("line_enhance", {"rowlen": 1, "rowblock_vec": 8}),
                ("vector_row", {}), ("vector_row", {"vector_tile": 0}), ("flat", {"flat_early": 1}), ("flat", {"col16": 1})]
    for strat, knobs in variants:
        try:
            for k, val in knobs.items():
                assert hiplib.spmv_acc_set_tunable(k.encode(), val) == 0, k
            got = run(torch, strat, -0.5, 2.0, rowptr, cols, vals, x, y0)
        finally:
            hiplib.spmv_acc_reset_tunables()
        err = oracle.scaled_error(got, ref, -0.5, 2.0, rowptr, cols, vals, x, y0)
        assert err <= SCALED_TOL, (strat, knobs, err)
        if not knobs:  # two FRESH plans with every timed choice pinned (the timed ones may fall differently: same result to rounding only)
            try:
                hiplib.spmv_acc_set_tunable(b"deterministic", 1)
                a = run(torch, strat, -0.5, 2.0, rowptr, cols, vals, x, y0)
                b = run(torch, strat, -0.5, 2.0, rowptr, cols, vals, x, y0)
            finally:
                hiplib.spmv_acc_reset_tunables()
            assert np.array_equal(a, b), (strat, "not reproducible")


def test_plan_cache_is_lru_bounded(torch_dev, hiplib):
    """More live matrices than the plan cache holds (1024): the least recently used plans go, the cache never grows past its
    bound, recently used matrices keep their plans, and results stay right throughout."""
    torch = torch_dev
    spmv_acc_amd.release_plans()
    rng = np.random.default_rng(12)
    m = 64
    mats = []
    for i in range(1040):
        rowptr = torch.arange(0, 2 * m + 1, 2, dtype=torch.int32, device="cuda")           # 2 non-zeros per row
        cols = torch.stack([torch.arange(m, device="cuda"), (torch.arange(m, device="cuda") + 1 + i) % m], 1).reshape(-1).to(torch.int32)
        vals = torch.full((2 * m,), float(i + 1), dtype=torch.float64, device="cuda")
        mats.append((rowptr, cols, vals))
    x = torch.ones(m, dtype=torch.float64, device="cuda")
    y = torch.zeros(m, dtype=torch.float64, device="cuda")
    for i, (rp, ci, v) in enumerate(mats):
        spmv_acc_amd.csr_spmv(1.0, 0.0, m, m, 2 * m, rp, ci, v, x, y, strategy="line_enhance")
        if i % 97 == 0:
            torch.cuda.synchronize()
            assert float(y.min().item()) == float(y.max().item()) == 2.0 * (i + 1)
        if i == 1000:  # touch matrix 0 again: it becomes the most recently used and must survive the evictions that follow
            spmv_acc_amd.csr_spmv(1.0, 0.0, m, m, 2 * m, *mats[0], x, y, strategy="line_enhance")
    torch.cuda.synchronize()
    assert hiplib.spmv_acc_cached_plans() == 1024
    assert spmv_acc_amd.query_plan(mats[0][0], m) is not None      # re-used late: kept
    assert spmv_acc_amd.query_plan(mats[1][0], m) is None          # oldest: evicted
    assert spmv_acc_amd.query_plan(mats[1039][0], m) is not None
    spmv_acc_amd.release_plans()
    assert hiplib.spmv_acc_cached_plans() == 0


def test_row_shard_without_rebasing(torch_dev, oracle):
    """A row shard handed over as views of the whole matrix -- rowptr + r0 (so rowptr[0] > 0), the complete colindex / value
    arrays, y + r0 -- as a caller slicing a larger CSR in place would: every strategy computes exactly the shard's rows and
    touches nothing outside them."""
    torch = torch_dev
    rowptr, cols, vals = synth.random_csr(30000, 30000, 11, seed=4, kind="powerlaw")
    rng = np.random.default_rng(1)
    x, y0 = rng.standard_normal(30000), rng.standard_normal(30000)
    ref = oracle.host_spmv(1.0, 1.0, rowptr, cols, vals, x, y0)
    drp, dci, dv, dx = (dev(torch, a) for a in (rowptr, cols, vals, x))
    for r0, r1 in ((12345, 27001), (1, 30000), (29990, 30000), (7, 8)):
        for strat in ALL:
            dy = dev(torch, y0)
            spmv_acc_amd.csr_spmv(1.0, 1.0, r1 - r0, 30000, int(rowptr[r1]), drp[r0:], dci, dv, dx, dy[r0:], strategy=strat)
            torch.cuda.synchronize()
            got = dy.cpu().numpy()
            assert np.array_equal(got[:r0], y0[:r0]) and np.array_equal(got[r1:], y0[r1:]), (strat, r0, r1, "wrote outside the shard")
            sl = slice(r0, r1)
            err = oracle.scaled_error(got[sl], ref[sl], 1.0, 1.0, (rowptr[r0:r1 + 1] - rowptr[r0]).astype(np.int32),
                                      cols[rowptr[r0]:rowptr[r1]], vals[rowptr[r0]:rowptr[r1]], x, y0[sl])
            assert err <= SCALED_TOL, (strat, r0, r1, err)
            spmv_acc_amd.release_plans(drp[r0:])


def test_billion_rows(torch_dev):
    """Row-count extreme: 1,000,000,000 rows with one non-zero each (plus two long rows), columns a fixed stride walk; y has a
    closed form.  Exercises the int32 row arithmetic of every kernel family a long way past 2^29."""
    torch = torch_dev
    m = 1_000_000_000
    n = 1 << 20
    rp = torch.arange(m + 1, dtype=torch.int32, device="cuda")           # one non-zero per row ...
    extra = 5000
    rp[m // 2 + 1:] += extra                                             # ... except row m/2: 5001 non-zeros
    nnz = m + extra
    idx = torch.arange(nnz, dtype=torch.int64, device="cuda")
    ci = ((idx * 7919) % n).to(torch.int32)
    v = torch.ones(nnz, dtype=torch.float64, device="cuda")
    del idx
    x = torch.arange(n, dtype=torch.float64, device="cuda") % 13.0 - 6.0
    def expected(rows):  # rows: int64 tensor of row ids (not m/2)
        j = torch.where(rows > m // 2, rows + extra, rows)
        return 2.0 * x[(j * 7919) % n] + 1.0
    probe = torch.tensor([0, 1, 12345, m // 2 - 1, m // 2 + 1, m - 2, m - 1], dtype=torch.int64, device="cuda")
    big = torch.arange(m // 2, m // 2 + extra + 1, dtype=torch.int64, device="cuda")
    want_big = 2.0 * float(x[(big * 7919) % n].sum().item()) + 1.0
    # (wf_row: one wavefront per row -- far more wavefronts than one launch holds, see the test below)
    for strat in ("adaptive", "line_enhance", "flat", "adaptive_plus", "vector_row", "wf_row", "thread_row"):
        y = torch.ones(m, dtype=torch.float64, device="cuda")
        spmv_acc_amd.csr_spmv(2.0, 1.0, m, n, nnz, rp, ci, v, x, y, strategy=strat)
        torch.cuda.synchronize()
        assert torch.equal(y[probe], expected(probe)), strat
        assert abs(float(y[m // 2].item()) - want_big) <= 1e-9 * abs(want_big) + 1e-9, strat
        # whole-vector check in chunks (exact: one product per row)
        for a in range(0, m, 1 << 28):
            b = min(m, a + (1 << 28))
            rows = torch.arange(a, b, dtype=torch.int64, device="cuda")
            ok = y[a:b] == expected(rows)
            if a <= m // 2 < b:
                ok[m // 2 - a] = True
            assert bool(ok.all().item()), (strat, a)
            del rows, ok
        del y
    spmv_acc_amd.release_plans(rp)


def test_more_rows_than_a_launch_holds_wavefronts(torch_dev, hiplib):
    """70 M rows: at one wavefront per row a grid would be 17.5 M workgroups = 2^32.06 work-items, and a HIP launch of 2^32 or more
    work-items WRAPS on this stack (the first 2.9 M rows were computed, nothing was reported: KERNEL_STRATEGY WF_ROW returned a wrong y
    from round 1 on, found in round 3 by profiles/probes/many_rows_probe.py).  Every kernel whose grid grows with m alone now strides over a capped
    number of workgroups: wf_row, the direct vector-row form under a forced width, LIGHT, and the plan-time builds of both column-slab
    forms, against an independent device evaluation on every row."""
    torch = torch_dev
    m = n = 70_000_000
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    lens = (torch.rand(m, generator=g, device="cuda") < 0.05).long() * torch.randint(1, 6, (m,), generator=g, device="cuda")
    lens[12345] = 3000  # (longer rows only slow the checker down: its index_add serialises on one address)
    lens[m - 3] = 70
    rp = torch.zeros(m + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(lens, 0, out=rp[1:])
    nnz = int(rp[-1].item())
    rows = torch.repeat_interleave(torch.arange(m, device="cuda"), lens, output_size=nnz)
    ci = torch.randint(0, n, (nnz,), generator=g, device="cuda")
    ci = (torch.sort(rows * n + ci).values % n).to(torch.int32)  # ascending inside the rows: the run lists apply
    rp = rp.to(torch.int32)
    v = torch.rand(nnz, generator=g, device="cuda", dtype=torch.float64) * 2 - 1
    x = torch.rand(n, generator=g, device="cuda", dtype=torch.float64) * 2 - 1
    y0 = torch.rand(m, generator=g, device="cuda", dtype=torch.float64)
    prod = v * x[ci.long()]
    ref = y0.clone().index_add_(0, rows, prod)
    scale = y0.abs().index_add_(0, rows, prod.abs()) + 1e-300
    del prod, rows, lens
    try:
        for strat, knobs in (("wf_row", {}), ("light", {}), ("vector_row", {"vector_tile": 0, "vector_width": 64}),
                             ("line_enhance", {"slab_segments": 4}), ("adaptive", {"col_slabs": 2})):
            hiplib.spmv_acc_reset_tunables()
            for k, val in knobs.items():
                assert hiplib.spmv_acc_set_tunable(k.encode(), val) == 0
            y = y0.clone()
            spmv_acc_amd.csr_spmv(1.0, 1.0, m, n, nnz, rp, ci, v, x, y, strategy=strat)
            torch.cuda.synchronize()
            assert float(((y - ref).abs() / scale).max().item()) <= SCALED_TOL, (strat, knobs)
            if "slab_segments" in knobs:
                assert spmv_acc_amd.query_plan(rp, m)["slab_passes"] == 4
            spmv_acc_amd.release_plans(rp)
            del y
    finally:
        hiplib.spmv_acc_reset_tunables()
        spmv_acc_amd.release_plans()


def test_against_rocsparse_as_second_opinion(torch_dev):
    """The reference's optional device-side verifier compares against rocSPARSE instead of the CPU loop (cli/verification.cpp:81-112,
    DEVICE_SIDE_VERIFY).  Same here, as a second, independent implementation: rocsparse_dcsrmv (the librocsparse bundled with torch)
    on a 400 K-row power-law matrix against every hot strategy.  Comparison only -- the product never links rocSPARSE."""
    import sys

    torch = torch_dev
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from rocsparse_row import RocsparseCsrmv
        roc = RocsparseCsrmv()
    except (OSError, AssertionError) as ex:
        pytest.skip(f"librocsparse not loadable: {ex}")
    import ctypes

    m, n, nnz, rp, ci, v = synth.rmat_torch(17, device="cuda", seed=0xC4)
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    x = torch.rand(n, generator=g, device="cuda", dtype=torch.float64) * 2 - 1
    y0 = torch.rand(m, generator=g, device="cuda", dtype=torch.float64) * 2 - 1
    alpha, beta = ctypes.c_double(0.75), ctypes.c_double(-1.5)
    y_roc = y0.clone()
    rc = roc.lib.rocsparse_dcsrmv(roc.handle, 111, m, n, nnz, ctypes.addressof(alpha), roc.descr, v.data_ptr(), rp.data_ptr(),
                                  ci.data_ptr(), None, x.data_ptr(), ctypes.addressof(beta), y_roc.data_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    rows = torch.repeat_interleave(torch.arange(m, device="cuda"), (rp[1:] - rp[:-1]).long(), output_size=nnz)
    scale = (1.5 * y0.abs()).index_add_(0, rows, 0.75 * (v * x[ci.long()]).abs()) + 1e-300
    for strat in spmv_acc_amd.HOT_STRATEGIES:
        y = y0.clone()
        spmv_acc_amd.csr_spmv(0.75, -1.5, m, n, nnz, rp, ci, v, x, y, strategy=strat)
        torch.cuda.synchronize()
        err = float(((y - y_roc).abs() / scale).max().item())
        assert err <= SCALED_TOL, (strat, err)
    spmv_acc_amd.release_plans(rp)


def test_benchmark_flat_copy_surface(torch_dev, oracle, tmp_path):
    """The reference benchmark keeps a private copy of flat (benchmark/flat/spmv_acc_flat.cpp) that launches the break-point
    kernels itself and expands the FLAT_KERNEL*_WRAPPER macros.  tests/cxx/bench_flat_driver.cpp does the same against
    include/hip-flat/ + include/common/macros.h: both break-point tables must equal the oracle's restatements bit for bit (with
    empty rows, where v1 and v2 differ) and every wrapper's y must match the oracle."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "bench_flat_driver")
    libdir = os.path.dirname(spmv_acc_amd.LIB_PATH)
    subprocess.run([hipcc, "-O2", "-std=c++14", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cxx", "bench_flat_driver.cpp"), "-L", libdir, "-lspmv_acc",
                    f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    for kind, m, avg, seed in (("powerlaw", 6000, 9, 5), ("empty_rows", 5000, 6, 6), ("dense_rows", 60, 700, 7)):
        rowptr, cols, vals = synth.random_csr(m, m, avg, seed=seed, kind=kind)
        nnz = int(rowptr[-1])
        rng = np.random.default_rng(seed)
        x, y0 = rng.standard_normal(m), rng.standard_normal(m)
        inp, outp = str(tmp_path / f"in_{kind}.bin"), str(tmp_path / f"out_{kind}.bin")
        with open(inp, "wb") as f:
            np.array([m, m, nnz], dtype=np.int32).tofile(f)
            for a in (rowptr, cols, vals, x, y0):
                a.tofile(f)
        subprocess.run([exe, inp, outp], check=True)
        raw = open(outp, "rb").read()
        blen = int(np.frombuffer(raw, dtype=np.int32, count=1)[0])
        assert blen == -(-nnz // 1024) + 1
        t1 = np.frombuffer(raw, dtype=np.int32, count=blen, offset=4)
        t2 = np.frombuffer(raw, dtype=np.int32, count=blen, offset=4 + 4 * blen)
        ys = np.frombuffer(raw, dtype=np.float64, offset=4 + 8 * blen).reshape(3, m)
        want1, want2 = oracle.break_points(rowptr, 1024), oracle.break_points(rowptr, 1024, v2=True)
        assert want1.size == blen and np.array_equal(t1, want1), kind
        assert np.array_equal(t2, want2), kind
        for k, y in enumerate(ys):
            check(oracle, y, 1.0, 1.0, rowptr, cols, vals, x, y0, ("bench-flat", kind, k))


def test_nan_stays_in_its_row(torch_dev, oracle):
    """A NaN (or Inf) in one matrix value must reach exactly the rows that hold it: the kernels load whole 16-byte groups and
    staged tiles that contain neighbouring rows' elements, and mask or ignore the foreign ones rather than multiply them by zero.
    Also beta = 0 must not read y (BLAS convention): a y full of NaN comes back finite.
    (Non-finite x, every pinned kernel form, the newer entries and subnormals: tests/test_gpu_special_values.py.)"""
    torch = torch_dev
    rng = np.random.default_rng(77)
    lens = rng.integers(1, 9, 20000)
    lens[[100, 5000, 5001, 19999]] = [700, 3000, 1, 2500]       # long rows next to short ones (slices, cooperative sums)
    rowptr, cols, vals = synth.csr_from_row_lengths(lens, 20000, rng)
    nnz = int(rowptr[-1])
    x = rng.standard_normal(20000)
    poisoned = {99: np.nan, 100: np.inf, 101: np.nan, 5000: np.nan, 5001: -np.inf, 12345: np.nan, 19999: np.nan, 0: np.nan}
    vals = vals.copy()
    for r, bad in poisoned.items():
        j = rowptr[r] + (rowptr[r + 1] - rowptr[r]) // 2   # some element inside the row
        vals[j] = bad
        x[cols[j]] = 1.0                                    # keep inf * x from turning into NaN by accident of sign only
    y_nan = np.full(20000, np.nan)
    clean = np.ones(20000, dtype=bool)
    clean[list(poisoned)] = False
    for strat in ALL:
        got = run(torch, strat, 1.0, 0.0, rowptr, cols, vals, x, y_nan)
        assert np.all(np.isfinite(got[clean])), (strat, np.nonzero(~np.isfinite(got) & clean)[0][:5])
        assert not np.any(np.isfinite(got[~clean])), strat
    ref = oracle.host_spmv(1.0, 0.0, rowptr, cols, np.where(np.isfinite(vals), vals, 0.0), x, np.zeros(20000))
    got = run(torch, "adaptive", 1.0, 0.0, rowptr, cols, vals, x, y_nan)
    assert np.allclose(got[clean], ref[clean], rtol=1e-12, atol=1e-12)


def test_host_threads_on_different_matrices(torch_dev, oracle):
    """host threads may call concurrently on DIFFERENT matrices (first calls included: plans are built and timed
    under the cache's lock discipline, kernels share the library stream).  Six threads, six matrices, every hot strategy, 40 calls
    each, all against the oracle."""
    import threading

    torch = torch_dev
    problems = []
    for t in range(6):
        rowptr, cols, vals = synth.random_csr(6000 + 700 * t, 5000, 5 + 2 * t, seed=300 + t, kind=("powerlaw", "uniform", "short")[t % 3])
        rng = np.random.default_rng(400 + t)
        x, y0 = rng.standard_normal(5000), rng.standard_normal(rowptr.size - 1)
        ref = oracle.host_spmv(1.0, 1.0, rowptr, cols, vals, x, y0)
        problems.append((rowptr, cols, vals, x, y0, ref, [dev(torch, a) for a in (rowptr, cols, vals, x, y0)]))
    torch.cuda.synchronize()
    errors = []

    def work(t):
        rowptr, cols, vals, x, y0, ref, (drp, dci, dv, dx, dy0) = problems[t]
        m, nnz = rowptr.size - 1, int(rowptr[-1])
        try:
            for it in range(40):
                strat = spmv_acc_amd.HOT_STRATEGIES[(it + t) % len(spmv_acc_amd.HOT_STRATEGIES)]
                dy = dy0.clone()
                spmv_acc_amd.csr_spmv(1.0, 1.0, m, 5000, nnz, drp, dci, dv, dx, dy, strategy=strat)
                torch.cuda.synchronize()
                err = oracle.scaled_error(dy.cpu().numpy(), ref, 1.0, 1.0, rowptr, cols, vals, x, y0)
                if not err <= SCALED_TOL:
                    errors.append((t, it, strat, err))
        except Exception as ex:  # noqa: BLE001
            errors.append((t, repr(ex)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(6)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    for p in problems:
        spmv_acc_amd.release_plans(p[6][0])
    assert not errors, errors[:5]


def test_giant_rows(torch_dev):
    """Rows of millions of non-zeros: flat cuts them into thousands of tiles, row-block-plus into thousands of slices, and the
    fix-up kernels add those carries with the whole wave instead of one lane walking them (device_utils.hpp wave_range_sum).
    Three rows of 3 M / 5 M / 70 non-zeros between ordinary rows; y against an fp64 index_add evaluation on the device."""
    torch = torch_dev
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    m, n = 5000, 200000
    lens = torch.randint(3, 12, (m,), generator=g, device="cuda")
    lens[7], lens[2500], lens[2501], lens[4999] = 3_000_000, 5_000_000, 70, 2_200_000
    rp = torch.zeros(m + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(lens, 0, out=rp[1:])
    nnz = int(rp[-1].item())
    ci = torch.randint(0, n, (nnz,), generator=g, device="cuda").to(torch.int32)
    v = torch.rand(nnz, generator=g, device="cuda", dtype=torch.float64) * 2 - 1
    x = torch.rand(n, generator=g, device="cuda", dtype=torch.float64) * 2 - 1
    y0 = torch.rand(m, generator=g, device="cuda", dtype=torch.float64) * 2 - 1
    # reference on the host with numpy's pairwise row sums (a device index_add would serialise millions of fp64 atomics on
    # three addresses); every row here has at least 3 non-zeros, so reduceat needs no empty-row handling
    prod = (v * x[ci.long()]).cpu().numpy()
    starts = rp[:-1].cpu().numpy()
    ref = torch.from_numpy(-0.5 * y0.cpu().numpy() + 1.5 * np.add.reduceat(prod, starts)).cuda()
    scale = torch.from_numpy(0.5 * np.abs(y0.cpu().numpy()) + 1.5 * np.add.reduceat(np.abs(prod), starts)).cuda()
    rp32 = rp.to(torch.int32)
    lib = spmv_acc_amd.load_library()
    for strat, knobs in (("flat", {"flat_finish": 0}), ("flat", {}), ("adaptive_plus", {}), ("adaptive_plus", {"plus_min_nnz": 1024}),
                         ("line_enhance", {}), ("adaptive", {}), ("default", {})):
        try:
            for k, val in knobs.items():
                assert lib.spmv_acc_set_tunable(k.encode(), val) == 0
            outs = []
            spmv_acc_amd.prepare(m, n, nnz, rp32, ci, v, x, strategy=strat, beta=-0.5)  # a settled plan (see test_bitwise_reproducible)
            for _ in range(2):
                y = y0.clone()
                spmv_acc_amd.csr_spmv(1.5, -0.5, m, n, nnz, rp32, ci, v, x, y, strategy=strat)
                torch.cuda.synchronize()
                outs.append(y)
        finally:
            lib.spmv_acc_reset_tunables()
            spmv_acc_amd.release_plans(rp32)
        err = float(((outs[0] - ref).abs() / scale).max().item())
        assert err <= SCALED_TOL, (strat, knobs, err)
        assert torch.equal(outs[0], outs[1]), (strat, "not reproducible on one plan")


def test_hypersparse_rows(torch_dev, hiplib):
    """Five million rows, 3000 non-zeros: every non-zero falls into one or two flat tiles, which would own millions of (empty)
    rows each -- flat hands such matrices to the fixed row blocks (dispatch.cpp kFlatMaxTileRows).  All strategies against a
    device-side evaluation; beta != 0 so every empty row must still be scaled."""
    import time

    torch = torch_dev
    g = torch.Generator(device="cuda")
    g.manual_seed(8)
    m, n = 5_000_000, 1000
    lens = torch.zeros(m, dtype=torch.int64, device="cuda")
    lens[torch.randint(0, m, (150,), generator=g, device="cuda")] = 20
    rp = torch.zeros(m + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(lens, 0, out=rp[1:])
    nnz = int(rp[-1].item())
    rows = torch.repeat_interleave(torch.arange(m, device="cuda"), lens, output_size=nnz)
    ci = torch.randint(0, n, (nnz,), generator=g, device="cuda").to(torch.int32)
    v = torch.rand(nnz, generator=g, device="cuda", dtype=torch.float64) * 2 - 1
    x = torch.rand(n, generator=g, device="cuda", dtype=torch.float64) * 2 - 1
    y0 = torch.rand(m, generator=g, device="cuda", dtype=torch.float64) * 2 - 1
    ref = (0.25 * y0).index_add_(0, rows, 2.0 * (v * x[ci.long()]))
    rp32 = rp.to(torch.int32)
    for strat in ("flat", "adaptive", "line_enhance", "adaptive_plus", "default", "vector_row"):
        y = y0.clone()
        spmv_acc_amd.csr_spmv(2.0, 0.25, m, n, nnz, rp32, ci, v, x, y, strategy=strat)
        torch.cuda.synchronize()
        assert float((y - ref).abs().max().item()) <= 1e-13, strat
        t0 = time.perf_counter()
        for _ in range(5):
            spmv_acc_amd.csr_spmv(2.0, 0.25, m, n, nnz, rp32, ci, v, x, y, strategy=strat)
        torch.cuda.synchronize()
        assert (time.perf_counter() - t0) / 5 < 5e-3, (strat, "steady-state call slower than 5 ms on a 100 MB problem")
    spmv_acc_amd.release_plans(rp32)
