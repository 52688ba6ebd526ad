"""GPU suite (-m gpu) of the AMG hierarchy and the V-cycle (spmv_acc_amd.amg: amg_setup, amg_cycle) on the four hierarchies of
tests/test_amg_host.py: the level sizes and every index array exactly as the host restatement has them, the values of P, R and A_c and the
iterate after each of ten cycles within a tolerance that comes from the host restatement's own spread, the residual after ten cycles below the
host file's bound, a one-level hierarchy as a direct solve, the two refusals of the coarsest level, and the plans released.

TOLERANCES, each 100 times a spread measured on the CPU between two host restatements that differ only in summation order (the figures are in
the docstring of tests/test_amg_host.py, whose test_the_spreads measures them again):
  the products (P, R, A_c): the host_spgemm chain against scipy.sparse differs by 0.0 on all four hierarchies, so the tolerance is 0: the
    device's values are the host chain's, bit for bit (-0.0 == +0.0) -- what the entries' own contracts promise;
  the iterates: forward against reversed SpMV row sums differ by at most 2.4e-15 of the iterate's largest magnitude over ten cycles, so the
    device's iterate (whose SpMVs add in the engine's order) is held to 2.4e-13 of it.

No speed gate: the parent commit cannot do this job (tools/amg_bench.py measures)."""
import numpy as np
import pytest

import spmv_acc_amd
from test_agg_host import grid5_matrix
from test_amg_host import (CYCLES, HIERARCHIES, ITERATE_SPREAD, OMEGA, PRODUCT_SPREAD, RESIDUAL_BOUND, TAGS, hierarchy, iterates,
                           relative_residuals, rhs)
from test_dense_host import host_dense_apply, host_dense_inverse, to_dense
from test_gpu_dense import dev, same_bits

pytestmark = pytest.mark.gpu

PRODUCT_TOL, ITERATE_TOL = 100 * PRODUCT_SPREAD, 100 * ITERATE_SPREAD


@pytest.fixture(scope="module")
def torch_dev(hiplib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def same(t, a):
    return np.array_equal(t.cpu().numpy(), np.asarray(a))


def close_values(t, want, tol):
    """Within tol of the matrix' largest magnitude; tol == 0: the same bits."""
    got, want = t.cpu().numpy(), np.asarray(want, dtype=np.float64)
    if tol == 0.0:
        return same_bits(t, want)
    return got.shape == want.shape and float(np.max(np.abs(got - want))) <= tol * float(np.max(np.abs(want)))


def device_setup(torch, tag):
    make, theta, coarse_rows, sizes, rule = HIERARCHIES[tag]
    m, (rp, ci, v) = make()
    return spmv_acc_amd.amg_setup(m, dev(torch, rp), dev(torch, ci), dev(torch, v), theta=theta, omega=OMEGA, coarse_rows=coarse_rows)


@pytest.mark.parametrize("tag", TAGS)
def test_hierarchy_and_cycles_are_the_host_model(torch_dev, hiplib, tag):
    torch = torch_dev
    _, _, _, sizes, rule = HIERARCHIES[tag]
    levels, coarsest = hierarchy(tag)
    plans = hiplib.spmv_acc_cached_plans()
    h = device_setup(torch, tag)
    assert hiplib.spmv_acc_cached_plans() == plans  # the setup makes no plan
    # the level sizes and every index array, exactly; the values within the products' tolerance
    assert h.sizes == sizes and h.coarsest.rule == rule and len(h.levels) == len(levels), (tag, h.sizes, h.coarsest.rule)
    for got, want in zip(h.levels, levels):
        assert got.m == want["m"] and got.mc == want["mc"]
        for name in ("A", "P", "R"):
            g, w = getattr(got, name), want[name]
            assert same(g[0], w[0]) and same(g[1], w[1]), (tag, got.m, name)
            assert close_values(g[2], w[2], PRODUCT_TOL), (tag, got.m, name)
        assert got.color_ptr == list(want["color_ptr"]) and same(got.color_rows, want["color_rows"])
        assert all(t.dtype == torch.float64 and t.numel() == n and not bool(t.any()) for t, n in ((got.r, got.m), (got.bc, got.mc), (got.xc, got.mc)))
    g, w = h.coarsest.A, coarsest["A"]
    assert same(g[0], w[0]) and same(g[1], w[1]) and close_values(g[2], w[2], PRODUCT_TOL)
    if PRODUCT_TOL == 0.0:  # the same coarsest matrix: the same inverse, bit for bit
        assert same_bits(h.coarsest.inv, coarsest["inv"])
    # ten cycles: every iterate within the iterates' tolerance, the residual below the host file's bound
    m = sizes[0]
    b = rhs(m)
    d_b, x = dev(torch, b), torch.zeros(m, dtype=torch.float64, device="cuda")
    want_x = iterates(tag)
    for k in range(CYCLES):
        spmv_acc_amd.amg_cycle(h, d_b, x)
        got = x.cpu().numpy()
        err = float(np.max(np.abs(got - want_x[k])) / np.max(np.abs(want_x[k])))
        assert err <= ITERATE_TOL, (tag, k, err)
    assert hiplib.spmv_acc_last_error() == 0
    res = relative_residuals(tag, [x.cpu().numpy()])[0]
    print(f"{tag}: relative residual after {CYCLES} cycles on the device {res:.3e} (host model {relative_residuals(tag, [want_x[-1]])[0]:.3e})")
    assert res <= RESIDUAL_BOUND, (tag, res)
    # the plans of the cycle's SpMVs are keyed by the hierarchy's rowptrs: release() drops them, and none of them was stale
    assert hiplib.spmv_acc_cached_plans() > plans
    torch.cuda.synchronize()
    assert spmv_acc_amd.check_plans() == 0
    h.release()
    assert hiplib.spmv_acc_cached_plans() == plans and spmv_acc_amd.check_plans() == 0 and hiplib.spmv_acc_last_error() == 0


def test_one_level_is_a_direct_solve(torch_dev, hiplib):
    """The 84-row second level of grid24 under coarse_rows = 256: no level above the coarsest, a cycle is x = inv b -- the host model's bits, and
    A x = b to the dense tolerance: |A X - I| <= m cond_2(A) 2^-52 entry by entry gives |A x - b| <= that times |b|_1, doubled for the apply's own
    rounding (m / 64 + 8 roundings of |A| |X| |b|, far below it)."""
    torch = torch_dev
    levels, _ = hierarchy("grid24")
    m, (rp, ci, v) = levels[1]["m"], levels[1]["A"]
    assert m == 84
    plans = hiplib.spmv_acc_cached_plans()
    h = spmv_acc_amd.amg_setup(m, dev(torch, rp), dev(torch, ci), dev(torch, v))
    assert h.sizes == [84] and h.levels == [] and h.coarsest.rule == "coarse_rows"
    b = rhs(m)
    x = torch.full((m,), 5.0, dtype=torch.float64, device="cuda")
    spmv_acc_amd.amg_cycle(h, dev(torch, b), x)
    inv, info = host_dense_inverse(m, rp, ci, v)
    assert info == 0 and same_bits(h.coarsest.inv, inv) and same_bits(x, host_dense_apply(m, inv, b))
    A = to_dense(m, m, rp, ci, v)
    tol = m * np.linalg.cond(A, 2) * 2.0 ** -52
    assert float(np.max(np.abs(A @ x.cpu().numpy() - b))) <= 2.0 * tol * float(np.sum(np.abs(b)))
    h.release()
    assert hiplib.spmv_acc_cached_plans() == plans and spmv_acc_amd.check_plans() == 0 and hiplib.spmv_acc_last_error() == 0


def neumann_with_an_emptied_row(n, gone):
    """The pure-Neumann five-point grid (diagonal = the number of neighbours, couplings -1: singular, constants in its kernel) with row and column
    `gone` emptied, the pattern still symmetric: structurally singular."""
    m, (rp, ci, v) = grid5_matrix(n)
    row = np.repeat(np.arange(m), np.diff(rp))
    v = np.where(ci == row, (np.diff(rp) - 1)[row].astype(np.float64), -1.0)
    keep = (row != gone) & (ci != gone)
    k_rp = np.concatenate([[0], np.cumsum(np.bincount(row[keep], minlength=m))]).astype(np.int32)
    return m, (k_rp, ci[keep], v[keep])


def test_a_singular_coarsest_level_is_refused_with_its_step(torch_dev, hiplib):
    torch = torch_dev
    m, (rp, ci, v) = neumann_with_an_emptied_row(8, 27)
    info = host_dense_inverse(m, rp, ci, v)[1]
    assert info == 27 + 1  # the emptied column: the first pivot that is zero
    with pytest.raises(spmv_acc_amd.SpmvAccError, match=r"singular: the pivot of step 27 .*info = 28"):
        spmv_acc_amd.amg_setup(m, dev(torch, rp), dev(torch, ci), dev(torch, v))
    # the same through a level: the emptied row is an aggregate of its own, and the coarse matrix keeps an empty row
    m, (rp, ci, v) = neumann_with_an_emptied_row(24, 300)
    with pytest.raises(spmv_acc_amd.SpmvAccError, match=r"singular: the pivot of step \d+ "):
        spmv_acc_amd.amg_setup(m, dev(torch, rp), dev(torch, ci), dev(torch, v), coarse_rows=128)
    assert hiplib.spmv_acc_last_error() == 0 and spmv_acc_amd.check_plans() == 0


def test_a_coarsest_level_over_the_cap_is_refused(torch_dev, hiplib):
    """65 x 65 grid points are 4225 rows: with max_levels = 1 they are the coarsest level, 129 more than the dense inverse takes; the message names
    the rule.  The stall rule likewise: a diagonal matrix has as many aggregates as rows."""
    torch = torch_dev
    m, (rp, ci, v) = grid5_matrix(65)
    with pytest.raises(spmv_acc_amd.SpmvAccError, match=r"4225 rows, the dense inverse takes at most 4096.*it is level max_levels"):
        spmv_acc_amd.amg_setup(m, dev(torch, rp), dev(torch, ci), dev(torch, v), max_levels=1)
    m = 5000
    with pytest.raises(spmv_acc_amd.SpmvAccError, match=r"5000 rows.*the aggregation stalled"):
        spmv_acc_amd.amg_setup(m, dev(torch, np.arange(m + 1, dtype=np.int32)), dev(torch, np.arange(m, dtype=np.int32)), dev(torch, np.full(m, 2.0)))
    assert hiplib.spmv_acc_last_error() == 0 and spmv_acc_amd.check_plans() == 0
