"""GPU suite (-m gpu) of the AMG cycle on the one-launch Jacobi / l1-Jacobi smoother (amg_setup(smoother=...), amg_cycle, pcg): the nine
hierarchies of tests/test_amg_host.py under "l1_jacobi" and two of them under "jacobi".  The smoother does not touch the setup, so A, P and R of
every level are the host chain's to the bit, no colouring is made, and each level's dinv is the host model's to the bit; ten cycles stay within
100 times the host model's pinned spread of its iterates (tests/test_amg_jacobi_host.py: the tolerance comes from the host model alone) and end
below residual_bound() of its residual; zero_start=True gives the bits of zero_start=False from x = 0; AMG-PCG converges in the host model's
iteration count, with the same bits of x for every check_every; a Gauss-Seidel and a Jacobi hierarchy of one matrix live side by side; no
rows and one row work.

No speed gate: the parent commit cannot do this job (tools/jacobi_bench.py measures)."""
import numpy as np
import pytest

import spmv_acc_amd
from test_amg_host import CYCLES, OMEGA, hierarchy, host_amg_setup, iterates, problem, relative_residuals, residual_bound, rhs_of
from test_amg_jacobi_host import (ALL_TAGS, GS_OMEGA, JACOBI_ITERATE_SPREAD, PCG_JACOBI_COUNTS, PCG_JACOBI_ITERATE_SPREAD, PCG_JACOBI_RESIDUAL_BOUND, SMOOTHERS,
                                  gs_omega_iterates, host_amg_cycle_jacobi, host_pcg_jacobi, inverses, jacobi_history_tolerances, jacobi_iterates, jacobi_solve)
from test_cg_host import PCG_RTOL, true_residual
from test_gpu_amg import ITERATE_TOL, guarded, guards_intact, iterate_error, same, words
from test_gpu_dense import dev, same_bits

pytestmark = pytest.mark.gpu

JACOBI_ITERATE_TOL, PCG_JACOBI_ITERATE_TOL = 100 * JACOBI_ITERATE_SPREAD, 100 * PCG_JACOBI_ITERATE_SPREAD  # the factor test_gpu_amg.py uses
CASES = [(tag, "l1_jacobi") for tag in ALL_TAGS] + [("grid24", "jacobi"), ("fem_scaled", "jacobi")]


@pytest.fixture(scope="module")
def torch_dev(hiplib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def device_setup(torch, tag, smoother="gs", **options):
    m, (rp, ci, v), theta, coarse_rows, max_levels, near = problem(tag)
    return spmv_acc_amd.amg_setup(m, dev(torch, rp), dev(torch, ci), dev(torch, v), theta=theta, omega=OMEGA, coarse_rows=coarse_rows,
                                  max_levels=max_levels, b=None if near is None else dev(torch, near), smoother=smoother, **options)


@pytest.mark.parametrize("tag,smoother", CASES)
def test_hierarchy_and_cycles_are_the_host_model(torch_dev, hiplib, tag, smoother):
    torch = torch_dev
    levels, coarsest = hierarchy(tag)
    kind, omega = SMOOTHERS[smoother]
    plans = hiplib.spmv_acc_cached_plans()
    h = device_setup(torch, tag, smoother)
    assert hiplib.spmv_acc_cached_plans() == plans  # the setup makes no plan
    assert h.smoother == smoother and h.smoother_omega == omega
    # the host chain's arrays to the bit, no colouring, the host model's dinv to the bit
    assert h.sizes == [lv["m"] for lv in levels] + [coarsest["m"]] and h.coarsest.rule == coarsest["rule"], (tag, h.sizes)
    for got, want, dinv in zip(h.levels, levels, inverses(tag, smoother)):
        assert got.m == want["m"] and got.mc == want["mc"]
        for name in ("A", "P", "R"):
            g, w = getattr(got, name), want[name]
            assert same(g[0], w[0]) and same(g[1], w[1]) and same_bits(g[2], w[2]), (tag, got.m, name)
        assert got.color_ptr is None and got.color_rows is None
        assert same_bits(got.dinv, dinv), (tag, got.m)
        assert all(t.dtype == torch.float64 and t.numel() == n and not bool(t.any())
                   for t, n in ((got.r, got.m), (got.bc, got.mc), (got.xc, got.mc), (got.xw, got.m)))
    g, w = h.coarsest.A, coarsest["A"]
    assert same(g[0], w[0]) and same(g[1], w[1]) and same_bits(g[2], w[2]) and same_bits(h.coarsest.inv, coarsest["inv"]), tag
    # ten cycles: every iterate within the tolerance, the residual below the bound; a cycle writes x and nothing around it, and leaves b alone
    m, b = h.sizes[0], rhs_of(tag)
    b_buf, d_b = guarded(torch, b)
    b_bits = words(torch, b_buf)
    x_buf, x = guarded(torch, np.zeros(m))
    want_x = jacobi_iterates(tag, smoother)
    worst = 0.0
    for k in range(CYCLES):
        spmv_acc_amd.amg_cycle(h, d_b, x)
        err = iterate_error(x, want_x[k])
        worst = max(worst, err)
        assert err <= JACOBI_ITERATE_TOL, (tag, smoother, k, err)
    assert hiplib.spmv_acc_last_error() == 0
    res, host_res = relative_residuals(tag, [x.cpu().numpy()])[0], relative_residuals(tag, [want_x[-1]])[0]
    print(f"{tag} {smoother}: iterates within {worst:.2e}; relative residual after {CYCLES} cycles on the device {res:.3e} (host model {host_res:.3e})")
    assert res <= residual_bound(host_res), (tag, smoother, res, host_res)
    assert guards_intact(x_buf) and guards_intact(b_buf) and torch.equal(words(torch, b_buf), b_bits)
    # the passes over a level's A are plan-free: a cycle plans R and P of each level and nothing else
    assert hiplib.spmv_acc_cached_plans() == plans + 2 * len(h.levels)
    # zero_start=True from x = 0 -- and from anything else: x is not read -- gives the bits of zero_start=False from x = 0
    for pre, post in ((1, 1), (2, 1), (0, 1)):
        plain = torch.zeros(m, dtype=torch.float64, device="cuda")
        spmv_acc_amd.amg_cycle(h, d_b, plain, pre=pre, post=post)
        for start in (0.0, 3.5):
            z_buf, z = guarded(torch, np.full(m, start))
            spmv_acc_amd.amg_cycle(h, d_b, z, pre=pre, post=post, direction="forward", zero_start=True)
            assert torch.equal(words(torch, z), words(torch, plain)) and guards_intact(z_buf), (tag, smoother, pre, post, start)
        if (pre, post) == (1, 1):
            assert iterate_error(plain, want_x[0]) <= JACOBI_ITERATE_TOL
    torch.cuda.synchronize()
    assert spmv_acc_amd.check_plans() == 0
    h.release()
    assert hiplib.spmv_acc_cached_plans() == plans and spmv_acc_amd.check_plans() == 0 and hiplib.spmv_acc_last_error() == 0


def settle_plans(h, x):
    """spmv_acc_amd.prepare, in both beta classes as tests/test_gpu_cg.py test_check_every_independence prepares its matrix, on every matrix
    whose SpMV a solve with the Jacobi hierarchy plans: the finest A (q = A p and r = b - A x of pcg itself), R and P of every level."""
    top = h.levels[0]
    planned = [(top.m, top.m, top.A, x)] + [(lv.mc, lv.m, lv.R, lv.r) for lv in h.levels] + [(lv.m, lv.mc, lv.P, lv.xc) for lv in h.levels]
    for rows, cols, mat, vec in planned:
        for beta in (0.0, 1.0):
            spmv_acc_amd.prepare(rows, cols, int(mat[1].numel()), *mat, vec, beta=beta)
        assert spmv_acc_amd.query_plan(mat[0], rows)["settled"], (rows, cols)


@pytest.mark.parametrize("tag,smoother", CASES)
def test_amg_pcg_is_the_host_model(torch_dev, hiplib, tag, smoother):
    """pcg with the Jacobi hierarchy as M at rtol 1e-10: status 1, the host's iteration count exactly, every history entry within that entry's
    own tolerance, the final iterate within 100 times the host model's spread, the true residual below its bound; the same bits of x for
    check_every 1 and 8 once the plans of the solve's SpMVs have settled; no plan left behind."""
    torch = torch_dev
    want = jacobi_solve(tag, smoother)
    count = PCG_JACOBI_COUNTS[smoother][tag]
    plans = hiplib.spmv_acc_cached_plans()
    h = device_setup(torch, tag, smoother)
    m, A = h.sizes[0], h.levels[0].A
    d_b = dev(torch, rhs_of(tag))
    x = torch.zeros(m, dtype=torch.float64, device="cuda")
    res = spmv_acc_amd.pcg(m, *A, d_b, x, precond=h, rtol=PCG_RTOL, history=True, check_every=1)
    assert res.status == 1 and res.iterations == count == want["iterations"], (tag, smoother, res.status, res.iterations)
    assert len(res.history) == count + 1 and res.rr == res.history[-1] and res.bb == float(want["state"]["bb"])
    err = np.abs(np.array(res.history) - want["history"]) / want["history"]
    tols = jacobi_history_tolerances(tag, smoother)
    true = true_residual(tag, x.cpu().numpy())
    its = iterate_error(x, want["x"])
    print(f"{tag} {smoother}: {res.iterations} iterations, true relative residual on the device {true:.3e} (host model {true_residual(tag, want['x']):.3e}), "
          f"history within {err.max():.2e}, at most {np.max(err / tols):.2g} of an entry's tolerance, the solution within {its:.2e}")
    assert np.all(err <= tols), (tag, smoother, err, tols)
    assert true <= PCG_JACOBI_RESIDUAL_BOUND and its <= PCG_JACOBI_ITERATE_TOL, (tag, smoother, true, its)
    # on settled plans (the engine may change the last bits of an SpMV once before its plan settles -- the finest A of pcg's own products, R
    # and P of every level; the sweeps and the cycle's residuals have no plan to settle) check_every = 1 and 8 give the same bits of x
    settle_plans(h, x)
    runs = []
    for check_every in (1, 8):
        x.fill_(0.0)
        runs.append((spmv_acc_amd.pcg(m, *A, d_b, x, precond=h, rtol=PCG_RTOL, history=True, check_every=check_every), words(torch, x)))
    (one, x_one), (eight, x_eight) = runs
    assert one.status == 1 and one.iterations == count and one == eight and torch.equal(x_one, x_eight), (tag, smoother, one, eight)
    x.fill_(0.0)
    part = spmv_acc_amd.pcg(m, *A, d_b, x, precond=h, rtol=PCG_RTOL, maxiter=5, check_every=3)
    assert part.status == 0 and part.iterations == 5 and iterate_error(x, want["iterates"][4]) <= PCG_JACOBI_ITERATE_TOL, (tag, smoother, part)
    assert hiplib.spmv_acc_last_error() == 0
    torch.cuda.synchronize()
    assert spmv_acc_amd.check_plans() == 0
    h.release()
    spmv_acc_amd.release_plans(A[0])  # (pcg's own SpMVs plan the finest A, which the Jacobi cycle never does)
    assert hiplib.spmv_acc_cached_plans() == plans and spmv_acc_amd.check_plans() == 0 and hiplib.spmv_acc_last_error() == 0


def test_pre_post_two(torch_dev, hiplib):
    """pre = post = 2 on fem_scaled: the host model's count, fewer than with one sweep each; an odd and an even number of out-of-place sweeps
    both end in x."""
    torch = torch_dev
    tag, smoother = "fem_scaled", "l1_jacobi"
    want = jacobi_solve(tag, smoother, False, 2, 2)
    h = device_setup(torch, tag, smoother)
    m, A = h.sizes[0], h.levels[0].A
    d_b = dev(torch, rhs_of(tag))
    x = torch.zeros(m, dtype=torch.float64, device="cuda")
    res = spmv_acc_amd.pcg(m, *A, d_b, x, precond=h, rtol=PCG_RTOL, pre=2, post=2)
    assert res.status == 1 and res.iterations == want["iterations"] < PCG_JACOBI_COUNTS[smoother][tag], (res, want["iterations"])
    assert iterate_error(x, want["x"]) <= PCG_JACOBI_ITERATE_TOL
    b = rhs_of(tag)
    for pre, post in ((0, 0), (0, 1), (1, 0), (2, 1), (1, 2), (3, 3)):
        x = dev(torch, np.linspace(-1.0, 1.0, m))
        spmv_acc_amd.amg_cycle(h, d_b, x, pre=pre, post=post)
        ref = host_amg_cycle_jacobi(hierarchy(tag), inverses(tag, smoother), 1.0, b, np.linspace(-1.0, 1.0, m), pre, post)
        assert iterate_error(x, ref) <= JACOBI_ITERATE_TOL, (pre, post)
    h.release()
    spmv_acc_amd.release_plans(A[0])


def test_a_gauss_seidel_and_a_jacobi_hierarchy_alive_at_once(torch_dev, hiplib):
    """grid24 under both smoothers: the Gauss-Seidel hierarchy's cycles have the same bits with a Jacobi hierarchy of the same matrix cycling
    in between as alone, and keep to their host model; the Jacobi one keeps to its own; smoother_omega is honoured by both smoothers."""
    torch = torch_dev
    tag = "grid24"
    plans = hiplib.spmv_acc_cached_plans()
    d_b = dev(torch, rhs_of(tag))
    alone = device_setup(torch, tag)
    m = alone.sizes[0]
    x = torch.zeros(m, dtype=torch.float64, device="cuda")
    alone_bits = []
    for k in range(4):
        spmv_acc_amd.amg_cycle(alone, d_b, x)
        alone_bits.append(words(torch, x))
    alone.release()
    gs, jac = device_setup(torch, tag), device_setup(torch, tag, "l1_jacobi")
    assert gs.smoother == "gs" and gs.levels[0].dinv is None and gs.levels[0].xw is None and gs.levels[0].color_ptr is not None
    xg, xj = torch.zeros(m, dtype=torch.float64, device="cuda"), torch.zeros(m, dtype=torch.float64, device="cuda")
    for k in range(4):
        spmv_acc_amd.amg_cycle(gs, d_b, xg, zero_start=(k == 0))  # (ignored under Gauss-Seidel)
        spmv_acc_amd.amg_cycle(jac, d_b, xj)
        assert torch.equal(words(torch, xg), alone_bits[k]), k
        assert iterate_error(xg, iterates(tag)[k]) <= ITERATE_TOL and iterate_error(xj, jacobi_iterates(tag, "l1_jacobi")[k]) <= JACOBI_ITERATE_TOL, k
    assert hiplib.spmv_acc_cached_plans() == plans + 3 * len(gs.levels) + 2 * len(jac.levels)
    gs.release()
    jac.release()
    # another omega is another cycle, the host model's at that omega
    damped = device_setup(torch, tag, "l1_jacobi", smoother_omega=0.8)
    assert damped.smoother_omega == 0.8
    xd = torch.zeros(m, dtype=torch.float64, device="cuda")
    spmv_acc_amd.amg_cycle(damped, d_b, xd)
    ref = host_amg_cycle_jacobi(hierarchy(tag), inverses(tag, "l1_jacobi"), 0.8, rhs_of(tag), np.zeros(m))
    assert iterate_error(xd, ref) <= JACOBI_ITERATE_TOL and iterate_error(xd, jacobi_iterates(tag, "l1_jacobi")[0]) > 1e-3
    damped.release()
    # ... under Gauss-Seidel too: smoother_omega is the sweeps' omega (SOR), the host model's cycle at that omega and not the cycle at 1.0
    sor = device_setup(torch, tag, "gs", smoother_omega=GS_OMEGA)
    assert sor.smoother == "gs" and sor.smoother_omega == GS_OMEGA
    xs = torch.zeros(m, dtype=torch.float64, device="cuda")
    for k, ref in enumerate(gs_omega_iterates(tag)):
        spmv_acc_amd.amg_cycle(sor, d_b, xs)
        assert iterate_error(xs, ref) <= ITERATE_TOL, k
        assert iterate_error(xs, iterates(tag)[k]) > 1e-3, k
    sor.release()
    torch.cuda.synchronize()
    assert hiplib.spmv_acc_cached_plans() == plans and spmv_acc_amd.check_plans() == 0 and hiplib.spmv_acc_last_error() == 0


@pytest.mark.parametrize("m", (0, 1))
@pytest.mark.parametrize("smoother", tuple(SMOOTHERS))
def test_edge_shapes(torch_dev, hiplib, m, smoother):
    """No rows, and the 1 x 1 matrix [2.0] with b = [1.0]: a hierarchy of the coarsest level alone, which never sweeps; a cycle and pcg give []
    and [0.5]."""
    torch = torch_dev
    A = (np.arange(m + 1, dtype=np.int32), np.arange(m, dtype=np.int32), np.full(m, 2.0))
    b = np.ones(m)
    host = host_amg_setup(m, A)
    want = host_pcg_jacobi(A, b, np.zeros(m), host, (), SMOOTHERS[smoother][1], rtol=1e-10)
    assert (want["status"], want["iterations"], want["x"].tolist()) == (1, m, [0.5] * m)
    plans = hiplib.spmv_acc_cached_plans()
    d_A = tuple(dev(torch, a) for a in A)
    h = spmv_acc_amd.amg_setup(m, *d_A, smoother=smoother)
    assert h.sizes == [m] and h.levels == [] and h.smoother == smoother and same_bits(h.coarsest.inv, host[1]["inv"])
    b_buf, d_b = guarded(torch, b)
    x_buf, x = guarded(torch, np.full(m, 3.0))
    spmv_acc_amd.amg_cycle(h, d_b, x, zero_start=True)
    assert x.cpu().tolist() == [0.5] * m
    x.zero_()
    res = spmv_acc_amd.pcg(m, *d_A, d_b, x, precond=h, rtol=1e-10, history=True)
    assert (res.status, res.iterations) == (1, m) and same_bits(x, want["x"]) and res.history == want["history"].tolist(), res
    assert guards_intact(b_buf) and guards_intact(x_buf) and same_bits(d_b, b)
    # the entries themselves on these shapes
    for kind in ("jacobi", "l1"):
        dinv = spmv_acc_amd.csr_jacobi_diagonal(m, *d_A, kind=kind)
        assert dinv.cpu().tolist() == [0.5] * m
        out = torch.full((m,), 7.25, dtype=torch.float64, device="cuda")
        spmv_acc_amd.csr_jacobi_sweep(m, *d_A, dinv, d_b, None, x_out=out)
        assert out.cpu().tolist() == [0.5] * m
    h.release()
    spmv_acc_amd.release_plans(d_A[0])
    assert hiplib.spmv_acc_cached_plans() == plans and spmv_acc_amd.check_plans() == 0 and hiplib.spmv_acc_last_error() == 0
