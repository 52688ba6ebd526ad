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

THE IRREGULAR CASES of tests/test_amg_host.py (fem_weak, fem_mixed, fem_scaled, graph608, graph608_two) run the same chain on levels that are no
stencils, with dropped entries, a near-nullspace vector and max_levels:
  the values of A, P, R and inv: bit for bit against the host chain, and no tolerance at all -- not because a spread against scipy is 0 (on
    graph608 it is 4.9e-16) but because every entry of the chain documents its summation order and its own GPU suite holds it to the bit;
  the iterates, in each (pre, post, direction) of VARIANTS: the same 2.4e-13, the host model's spread on these cases being at most 2.26e-15;
  the residual after ten cycles, per case and variant: below ten times the host model's, rounded up to a power of ten (residual_bound).
Also: what a cycle may write (x alone), two hierarchies alive at once, m = 0 and m = 1, and the refusal of an unknown direction.
Nobody has measured the device's spreads on these cases: every tolerance comes from the host model alone.

No speed gate: the parent commit cannot do this job (tools/amg_bench.py measures)."""
import numpy as np
import pytest

import spmv_acc_amd
from test_agg_host import grid5_matrix
from test_amg_host import (CYCLES, HIERARCHIES, IRREGULAR, IRREGULAR_TAGS, ITERATE_SPREAD, OMEGA, PRODUCT_SPREAD, RESIDUAL_BOUND, TAGS, VARIANTS,
                           hierarchy, host_amg_cycle, host_amg_setup, iterates, problem, relative_residuals, residual_bound, rhs, rhs_of,
                           variant_iterates)
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
    """amg_setup on a case of either table of tests/test_amg_host.py, with the case's max_levels and near-nullspace vector."""
    m, (rp, ci, v), theta, coarse_rows, max_levels, near = problem(tag)
    return spmv_acc_amd.amg_setup(m, dev(torch, rp), dev(torch, ci), dev(torch, v), theta=theta, omega=OMEGA, coarse_rows=coarse_rows,
                                  max_levels=max_levels, b=None if near is None else dev(torch, near))


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


# ---- the irregular cases of tests/test_amg_host.py, every cycle option, what a cycle may write, two hierarchies, edge shapes ------------------------------
PAD, FILL = 8, 7.25


def guarded(torch, a):
    """(buffer, view): a on the device inside a buffer with PAD entries of 7.25 on either side."""
    a = np.asarray(a, dtype=np.float64)
    buf = torch.full((a.size + 2 * PAD,), FILL, dtype=torch.float64, device="cuda")
    view = buf[PAD:PAD + a.size]
    if a.size:
        view.copy_(dev(torch, a))
    return buf, view


def guards_intact(buf):
    return bool((buf[:PAD] == FILL).all()) and bool((buf[-PAD:] == FILL).all())


def held_arrays(h):
    """name -> every array the hierarchy holds and a cycle reads: A, P, R and color_rows of each level, the coarsest A and inv."""
    out = {}
    for k, lv in enumerate(h.levels):
        for name in ("A", "P", "R"):
            for part, t in zip(("rowptr", "colindex", "value"), getattr(lv, name)):
                out[f"{k}.{name}.{part}"] = t
        out[f"{k}.color_rows"] = lv.color_rows
    for part, t in zip(("rowptr", "colindex", "value"), h.coarsest.A):
        out[f"coarsest.A.{part}"] = t
    out["coarsest.inv"] = h.coarsest.inv
    return out


def words(torch, t):
    """The array's bits: the doubles as int64 words (a NaN or a -0.0 compares by its bits), the int32 index arrays as they are."""
    return (t.view(torch.int64) if t.dtype == torch.float64 else t).clone()


def changed(torch, h, snap):
    torch.cuda.synchronize()
    return [name for name, t in held_arrays(h).items() if not torch.equal(words(torch, t), snap[name])]


def hierarchy_is_the_host_chain(torch, h, tag):
    """Sizes, rule and every index array exactly; the values of A, P, R on every level, of the coarsest A and of inv bit for bit (-0.0 == +0.0):
    no tolerance.  Each entry of the chain -- csr_strength, csr_aggregate, csr_tentative, csr_smooth_prolongator, csr_transpose, csr_spgemm,
    csr_color, csr_dense_inverse -- documents its summation order, and its own GPU suite holds it to the host model's bits; a value that
    differs here breaks the contract of the entry that made it (P: csr_tentative or csr_smooth_prolongator; R: csr_transpose; A_c:
    csr_spgemm; inv: csr_dense_inverse)."""
    levels, coarsest = hierarchy(tag)
    assert h.sizes == [lv["m"] for lv in levels] + [coarsest["m"]] and h.coarsest.rule == coarsest["rule"] and len(h.levels) == len(levels), (tag, h.sizes)
    for got, want in zip(h.levels, levels):
        assert got.m == want["m"] and got.mc == want["mc"]
        for name in ("A", "P", "R"):
            g, w = getattr(got, name), want[name]
            assert same(g[0], w[0]) and same(g[1], w[1]), (tag, got.m, name)
            assert same_bits(g[2], w[2]), (tag, got.m, name)
        assert got.color_ptr == list(want["color_ptr"]) and same(got.color_rows, want["color_rows"]), (tag, got.m)
        assert all(t.dtype == torch.float64 and t.numel() == n and not bool(t.any()) for t, n in ((got.r, got.m), (got.bc, got.mc), (got.xc, got.mc)))
    g, w = h.coarsest.A, coarsest["A"]
    assert same(g[0], w[0]) and same(g[1], w[1]) and same_bits(g[2], w[2]), tag
    assert same_bits(h.coarsest.inv, coarsest["inv"]), tag


def iterate_error(x, want):
    return float(np.max(np.abs(x.cpu().numpy() - want)) / np.max(np.abs(want)))


@pytest.mark.parametrize("tag", IRREGULAR_TAGS)
def test_irregular_hierarchy_and_cycles_are_the_host_model(torch_dev, hiplib, tag):
    """The hierarchy is the host chain's to the bit; ten cycles in each (pre, post, direction) of VARIANTS stay within ITERATE_TOL of the host
    model's iterates (the tolerance comes from the host model's spread alone: nobody measured the device's), the residual of the device's x,
    computed in numpy, below residual_bound() of the host model's; a cycle writes x and nothing else -- not the guards around b and x, no bit of
    b, no array the hierarchy holds --; the setup caches no plan and release() drops every plan of the cycles."""
    torch = torch_dev
    assert IRREGULAR[tag][3] == [lv["m"] for lv in hierarchy(tag)[0]] + [hierarchy(tag)[1]["m"]]
    plans = hiplib.spmv_acc_cached_plans()
    h = device_setup(torch, tag)
    assert hiplib.spmv_acc_cached_plans() == plans  # the setup makes no plan
    hierarchy_is_the_host_chain(torch, h, tag)
    torch.cuda.synchronize()
    snap = {name: words(torch, t) for name, t in held_arrays(h).items()}
    m, b = h.sizes[0], rhs_of(tag)
    b_buf, d_b = guarded(torch, b)
    b_bits = words(torch, b_buf)
    for variant in VARIANTS:
        pre, post, direction = variant
        x_buf, x = guarded(torch, np.zeros(m))
        want_x = variant_iterates(tag, variant)
        worst = 0.0
        for k in range(CYCLES):
            spmv_acc_amd.amg_cycle(h, d_b, x, pre=pre, post=post, direction=direction)
            err = iterate_error(x, want_x[k])
            worst = max(worst, err)
            assert err <= ITERATE_TOL, (tag, variant, k, err)
        assert hiplib.spmv_acc_last_error() == 0
        res, host_res = relative_residuals(tag, [x.cpu().numpy()])[0], relative_residuals(tag, [want_x[-1]])[0]
        print(f"{tag} {variant}: iterates within {worst:.2e}; relative residual after {CYCLES} cycles on the device {res:.3e} (host model {host_res:.3e})")
        assert res <= residual_bound(host_res), (tag, variant, res, host_res)
        assert guards_intact(x_buf) and guards_intact(b_buf) and torch.equal(words(torch, b_buf), b_bits), (tag, variant)
    assert changed(torch, h, snap) == [], tag
    assert hiplib.spmv_acc_cached_plans() > plans
    assert spmv_acc_amd.check_plans() == 0
    h.release()
    assert hiplib.spmv_acc_cached_plans() == plans and spmv_acc_amd.check_plans() == 0 and hiplib.spmv_acc_last_error() == 0


def test_two_hierarchies_alive_at_once(torch_dev, hiplib):
    """fem_weak and grid24, five cycles on each in turn: each keeps to its own host model; releasing the first drops exactly its plans and leaves
    the second cycling on, with no stale plan."""
    torch = torch_dev
    plans = hiplib.spmv_acc_cached_plans()
    tags = ("fem_weak", "grid24")
    hs = [device_setup(torch, t) for t in tags]
    bs = [dev(torch, rhs_of(t)) for t in tags]
    xs = [torch.zeros(h.sizes[0], dtype=torch.float64, device="cuda") for h in hs]
    counts = []
    for k in range(5):
        for n, tag in enumerate(tags):
            before = hiplib.spmv_acc_cached_plans()
            spmv_acc_amd.amg_cycle(hs[n], bs[n], xs[n])
            if k == 0:
                counts.append(hiplib.spmv_acc_cached_plans() - before)  # the plans this hierarchy's first cycle made
            else:
                assert hiplib.spmv_acc_cached_plans() == before  # ... and no later one made another
            err = iterate_error(xs[n], iterates(tag)[k])
            assert err <= ITERATE_TOL, (tag, k, err)
    assert counts == [3 * len(h.levels) for h in hs] and hiplib.spmv_acc_cached_plans() == plans + sum(counts)  # one plan each for A, P and R of a level
    torch.cuda.synchronize()
    assert spmv_acc_amd.check_plans() == 0
    hs[0].release()
    assert hiplib.spmv_acc_cached_plans() == plans + counts[1]  # reduced by exactly the first hierarchy's plans
    for n, h in enumerate(hs):  # ... which are gone, every one, while the second hierarchy's are all there
        for lv in h.levels:
            found = [spmv_acc_amd.query_plan(mat[0], rows) is not None for mat, rows in ((lv.A, lv.m), (lv.P, lv.m), (lv.R, lv.mc))]
            assert found == [n == 1] * 3, (tags[n], lv.m, found)
    for k in range(5, 8):
        before = hiplib.spmv_acc_cached_plans()
        spmv_acc_amd.amg_cycle(hs[1], bs[1], xs[1])
        err = iterate_error(xs[1], iterates("grid24")[k])
        assert err <= ITERATE_TOL and hiplib.spmv_acc_cached_plans() == before, (k, err)
    torch.cuda.synchronize()
    assert spmv_acc_amd.check_plans() == 0
    hs[1].release()
    assert hiplib.spmv_acc_cached_plans() == plans and spmv_acc_amd.check_plans() == 0 and hiplib.spmv_acc_last_error() == 0


@pytest.mark.parametrize("m", (0, 1))
def test_edge_shapes(torch_dev, hiplib, m):
    """No rows, and the 1 x 1 matrix [2.0] with b = [1.0]: amg_setup, one amg_cycle and pcg with the hierarchy give the host model's answers --
    [] with status 1 after 0 iterations, [0.5] with status 1 after 1 iteration -- without an error and without a plan left behind."""
    from test_cg_host import host_pcg

    torch = torch_dev
    A = (np.arange(m + 1, dtype=np.int32), np.arange(m, dtype=np.int32), np.full(m, 2.0))
    b = np.ones(m)
    host = host_amg_setup(m, A)
    assert host[0] == [] and host[1]["info"] == 0 and host[1]["rule"] == "coarse_rows"
    want = host_pcg(A, b, np.zeros(m), host, rtol=1e-10)
    assert (want["status"], want["iterations"], want["x"].tolist()) == (1, m, [0.5] * m)
    plans = hiplib.spmv_acc_cached_plans()
    d_A = tuple(dev(torch, a) for a in A)
    h = spmv_acc_amd.amg_setup(m, *d_A)
    assert h.sizes == [m] and h.levels == [] and h.coarsest.rule == "coarse_rows" and tuple(h.coarsest.inv.shape) == (m, m)
    assert same_bits(h.coarsest.inv, host[1]["inv"])
    b_buf, d_b = guarded(torch, b)
    x_buf, x = guarded(torch, np.full(m, 3.0))
    spmv_acc_amd.amg_cycle(h, d_b, x)
    assert same_bits(x, host_amg_cycle(host, b, np.zeros(m))) and x.cpu().tolist() == [0.5] * m
    x.zero_()
    res = spmv_acc_amd.pcg(m, *d_A, d_b, x, precond=h, rtol=1e-10, history=True)
    assert (res.status, res.iterations) == (1, m) and same_bits(x, want["x"]) and res.history == want["history"].tolist(), res
    assert guards_intact(b_buf) and guards_intact(x_buf) and same_bits(d_b, b)
    h.release()
    spmv_acc_amd.release_plans(d_A[0])
    assert hiplib.spmv_acc_cached_plans() == plans and spmv_acc_amd.check_plans() == 0 and hiplib.spmv_acc_last_error() == 0


def test_an_unknown_direction_is_refused(torch_dev, hiplib):
    """amg_cycle checks `direction` itself: on a hierarchy of one level (which never sweeps) and on grid24 alike, SpmvAccError names amg_cycle and
    the three directions, and x keeps its bits."""
    torch = torch_dev
    levels, _ = hierarchy("grid24")
    m1, (rp, ci, v) = levels[1]["m"], levels[1]["A"]
    plans = hiplib.spmv_acc_cached_plans()
    one = spmv_acc_amd.amg_setup(m1, dev(torch, rp), dev(torch, ci), dev(torch, v))
    assert one.levels == []
    for h in (one, device_setup(torch, "grid24")):
        m = h.sizes[0]
        x_buf, x = guarded(torch, rhs(m) + 2.0)
        before = words(torch, x_buf)
        for bad in ("sideways", "Symmetric", 2, None):
            with pytest.raises(spmv_acc_amd.SpmvAccError, match=r"amg_cycle: direction .*one of \('forward', 'backward', 'symmetric'\)"):
                spmv_acc_amd.amg_cycle(h, dev(torch, rhs(m)), x, direction=bad)
        torch.cuda.synchronize()
        assert torch.equal(words(torch, x_buf), before)
        h.release()
    assert hiplib.spmv_acc_cached_plans() == plans and spmv_acc_amd.check_plans() == 0 and hiplib.spmv_acc_last_error() == 0
