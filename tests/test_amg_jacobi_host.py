"""CPU side of the AMG cycle on the one-launch Jacobi / l1-Jacobi smoother (spmv_acc_amd/amg.py amg_setup(smoother=...); no GPU): the cycle
and AMG-PCG on it restated from the pieces -- host_jacobi_diagonal and host_jacobi_sweep (tests/test_jacobi_host.py), the host hierarchies,
host_spmv and host_dense_apply of tests/test_amg_host.py, the conjugate-gradient entries of tests/test_cg_host.py -- and exported to the GPU
suite as its reference.  The smoother does not touch the setup: the hierarchies are those of tests/test_amg_host.py, colours unused.

The cycle, per level, as amg_cycle runs it: `pre` sweeps, the first in the zero-start form (x = omega dinv b, the matrix not read) where the
level's x is known to be zero -- every coarse level, and the finest under zero_start --; r = b - A x in the sweep's own summation order;
b_c = R r and x += P x_c by SpMV; `post` sweeps.  "l1_jacobi" sweeps with the scaled l1 diagonal at omega = 1, "jacobi" with 1 / a_ii at 2/3.

MEASURED with this file's model (pre = post = 1, b = rhs_of(tag), x0 = 0) on the nine hierarchies: the relative residual |b - A x| / |b| after
ten cycles and the worst per-cycle factor (every cycle of every case reduces the residual), then AMG-PCG at rtol 1e-10: iterations (the same
in both summation orders of the SpMVs) and the true relative residual -- beside the iterations of the Gauss-Seidel hierarchy and of
unpreconditioned CG:
                      l1_jacobi                          jacobi (omega 2/3)                   GS    none
    grid24        9.9e-03  0.73   23  8.2e-11        3.4e-03  0.67   20  5.5e-11          12      87
    grid48        1.5e-02  0.77   28  5.1e-11        6.5e-03  0.73   24  5.4e-11          14     171
    aniso48       1.7e-02  0.75   25  7.4e-11        6.9e-03  0.70   22  3.7e-11          13     342
    aniso24       1.6e-02  0.74   23  5.8e-11        6.0e-03  0.68   20  4.5e-11          12     172
    fem_weak      2.3e-02  0.81   25  8.9e-11        1.1e-02  0.77   22  4.5e-11          12     113
    fem_mixed     3.1e-03  0.65   20  3.0e-11        6.6e-04  0.58   17  3.1e-11           9      42
    fem_scaled    4.6e-03  0.68   21  2.3e-11        1.1e-03  0.60   18  1.9e-11           9   >1000
    graph608      9.9e-02  0.94   24  4.6e-11        6.8e-02  0.92   20  7.6e-11          11      66
    graph608_two  6.9e-03  0.70   21  5.7e-11        1.9e-03  0.63   18  4.2e-11           9      66
(unpreconditioned CG on fem_scaled is stopped unconverged at its cap of 1000 iterations.)  The cycle needs about twice the iterations of
Gauss-Seidel, at two matrix passes per level where a symmetric Gauss-Seidel sweep is two launches per colour.  The last history entry above
the threshold tol2 and the first one below it lie at least 0.12 of themselves from it on all eighteen solves, their tolerances
(jacobi_history_tolerances) are at most 5.9e-07: the device's count must be the host's.  PCG_JACOBI_RESIDUAL_BOUND is ten times the largest
true residual, 8.9e-10, rounded up to a power of ten: 1e-9.

The spread the GPU suite's tolerance comes from (two host restatements that differ only in the summation order of the restriction's and the
prolongation's SpMVs, forward against reversed row sums; the sweeps and the residual have ONE documented order, the device's): the iterates of
ten cycles, relative to the iterate's largest magnitude, the largest over the nine cases: 5.6e-15 under l1_jacobi and 5.7e-15 under jacobi
(both on aniso48) -- ABOVE the Gauss-Seidel cycle's ITERATE_SPREAD of 2.4e-15, so the Jacobi cycle has its own constant,
JACOBI_ITERATE_SPREAD 6e-15.  The AMG-PCG iterates over all iterations: 2.6e-15 and 3.8e-15 (both on fem_weak): PCG_JACOBI_ITERATE_SPREAD
4e-15.  Nobody has measured the device's spreads: the tolerances come from this model alone."""
import functools

import numpy as np
import pytest

from test_amg_host import CYCLES, IRREGULAR_TAGS, ITERATE_SPREAD, TAGS, hierarchy, host_spmv, problem, relative_residuals, rhs_of
from test_cg_host import (PCG_COUNTS, PCG_IRREGULAR_COUNTS, PCG_RTOL, host_cg_direction, host_cg_start, host_cg_update, host_pcg, true_residual)
from test_dense_host import host_dense_apply
from test_gs_host import host_gs_sweep
from test_jacobi_host import host_jacobi_diagonal, host_jacobi_sweep

ALL_TAGS = TAGS + IRREGULAR_TAGS
# smoother -> (the kind of the diagonal, the omega that smoother_omega=None stands for)
SMOOTHERS = {"l1_jacobi": ("l1", 1.0), "jacobi": ("jacobi", 2.0 / 3.0)}
# (the docstring; the tests below hold every figure to this file's model)
TEN_CYCLES = {
    "l1_jacobi": dict(grid24=9.9e-03, grid48=1.5e-02, aniso48=1.7e-02, aniso24=1.6e-02, fem_weak=2.3e-02, fem_mixed=3.1e-03, fem_scaled=4.6e-03,
                      graph608=9.9e-02, graph608_two=6.9e-03),
    "jacobi": dict(grid24=3.4e-03, grid48=6.5e-03, aniso48=6.9e-03, aniso24=6.0e-03, fem_weak=1.1e-02, fem_mixed=6.6e-04, fem_scaled=1.1e-03,
                   graph608=6.8e-02, graph608_two=1.9e-03),
}
WORST_FACTOR = 0.95  # every per-cycle factor of the table lies below it (graph608 under l1_jacobi: 0.94)
PCG_JACOBI_COUNTS = {
    "l1_jacobi": dict(grid24=23, grid48=28, aniso48=25, aniso24=23, fem_weak=25, fem_mixed=20, fem_scaled=21, graph608=24, graph608_two=21),
    "jacobi": dict(grid24=20, grid48=24, aniso48=22, aniso24=20, fem_weak=22, fem_mixed=17, fem_scaled=18, graph608=20, graph608_two=18),
}
NONE_COUNTS = dict(grid24=87, grid48=171, aniso48=342, aniso24=172, fem_weak=113, fem_mixed=42, fem_scaled=1000, graph608=66, graph608_two=66)
JACOBI_ITERATE_SPREAD = 6e-15  # (above test_amg_host.ITERATE_SPREAD, so not shared)
PCG_JACOBI_ITERATE_SPREAD = 4e-15
PCG_JACOBI_RESIDUAL_BOUND = 1e-9


@functools.lru_cache(maxsize=None)
def inverses(tag, smoother):
    """dinv of every non-coarsest level of a hierarchy, finest first."""
    kind = SMOOTHERS[smoother][0]
    return tuple(host_jacobi_diagonal(lv["m"], *lv["A"], kind) for lv in hierarchy(tag)[0])


def host_amg_cycle_jacobi(h, dinvs, omega, b, x, pre=1, post=1, reverse=False, zero=False, depth=0):
    """One V-cycle on a Jacobi hierarchy; returns the new x.  zero: x counts as zero whatever it holds.  reverse: the SpMVs of R and P add
    their rows from the last entry (the other summation order of the spread)."""
    levels, coarsest = h
    if depth == len(levels):
        return host_dense_apply(coarsest["m"], coarsest["inv"], b)
    lv = levels[depth]
    m, (rp, ci, v), dinv = lv["m"], lv["A"], dinvs[depth]
    for _ in range(pre):
        x = host_jacobi_sweep(m, rp, ci, v, dinv, b, None if zero else x, omega)[0]
        zero = False
    if zero:  # (pre == 0)
        x = np.zeros(m)
    r = host_jacobi_sweep(m, rp, ci, v, dinv, b, x, omega)[1]
    bc = host_spmv(lv["R"], r, reverse)
    xc = host_amg_cycle_jacobi(h, dinvs, omega, bc, None, pre, post, reverse, True, depth + 1)
    x = x + host_spmv(lv["P"], xc, reverse)
    for _ in range(post):
        x = host_jacobi_sweep(m, rp, ci, v, dinv, b, x, omega)[0]
    return x


def host_pcg_jacobi(A, b, x0, h, dinvs, omega, rtol=1e-8, maxiter=1000, reverse=False, pre=1, post=1):
    """pcg with a Jacobi hierarchy, restated from the entries' models as tests/test_cg_host.py host_pcg restates it for Gauss-Seidel: z = one
    cycle from a zero start (zero_start=True: what z holds is not read).  Returns host_pcg's dict."""
    hist = np.zeros(maxiter + 1)
    x = np.array(x0, dtype=np.float64)
    r = b - host_spmv(A, x, reverse)

    def M(r):
        return host_amg_cycle_jacobi(h, dinvs, omega, r, None, pre, post, reverse, zero=True)

    z = M(r)
    p, state = host_cg_start(rtol, b, r, z, hist)
    iterates = []
    while state["status"] == 0 and state["iterations"] < maxiter:
        q = host_spmv(A, p, reverse)
        x, r, state = host_cg_update(p, q, x, r, state, hist)
        if state["status"] != 2:
            iterates.append(x)
        if state["status"] == 0:
            z = M(r)
        z, p, state = host_cg_direction(r, z, p, state, None)
    return dict(status=state["status"], iterations=state["iterations"], history=hist[:state["iterations"] + 1].copy(), iterates=tuple(iterates), x=x, state=state)


@functools.lru_cache(maxsize=None)
def jacobi_iterates(tag, smoother, reverse=False, pre=1, post=1):
    """The iterate after each of the ten cycles (x0 = 0, zero_start False), as a tuple of arrays."""
    m = problem(tag)[0]
    b, x, out = rhs_of(tag), np.zeros(m), []
    for _ in range(CYCLES):
        x = host_amg_cycle_jacobi(hierarchy(tag), inverses(tag, smoother), SMOOTHERS[smoother][1], b, x, pre, post, reverse)
        out.append(x)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def jacobi_solve(tag, smoother, reverse=False, pre=1, post=1):
    """The host AMG-PCG solve of the GPU suite: rtol 1e-10, b = rhs_of(tag), x0 = 0."""
    m, A = problem(tag)[:2]
    return host_pcg_jacobi(A, rhs_of(tag), np.zeros(m), hierarchy(tag), inverses(tag, smoother), SMOOTHERS[smoother][1], rtol=PCG_RTOL, reverse=reverse,
                           pre=pre, post=post)


@functools.lru_cache(maxsize=None)
def plain_count(tag):
    m, A = problem(tag)[:2]
    s = host_pcg(A, rhs_of(tag), np.zeros(m), None, rtol=PCG_RTOL)
    return s["status"], s["iterations"]


def jacobi_history_tolerances(tag, smoother):
    """As tests/test_cg_host.py history_tolerances: entry by entry 100 times the forward-against-reversed spread, at least 100 * 2^-52."""
    fwd, rev = jacobi_solve(tag, smoother)["history"], jacobi_solve(tag, smoother, True)["history"]
    assert fwd.size == rev.size
    return np.maximum(100.0 * np.abs(fwd - rev) / fwd, 100.0 * 2.0 ** -52)


CASES = [(tag, s) for s in SMOOTHERS for tag in ALL_TAGS]


@pytest.mark.parametrize("tag,smoother", CASES)
def test_ten_cycles_reduce_the_residual(tag, smoother):
    """Every one of ten cycles reduces the residual; the figure after ten is the docstring's, to its two digits."""
    res = relative_residuals(tag, jacobi_iterates(tag, smoother))
    factors = [b / a for a, b in zip([1.0] + res[:-1], res)]
    print(f"{tag} {smoother}: relative residual after {CYCLES} cycles {res[-1]:.3e}, worst per-cycle factor {max(factors):.3f}")
    assert max(factors) < WORST_FACTOR < 1.0, (tag, smoother, factors)
    assert abs(res[-1] - TEN_CYCLES[smoother][tag]) <= 0.05 * TEN_CYCLES[smoother][tag], (tag, smoother, res[-1])


def test_the_zero_start_is_the_same_cycle():
    """From an x of zeros, zero=True gives the same numbers as zero=False: the zero-start sweep is the general sweep on x = 0."""
    for tag, smoother in (("grid24", "l1_jacobi"), ("fem_scaled", "jacobi"), ("graph608", "l1_jacobi")):
        m = problem(tag)[0]
        for pre, post in ((1, 1), (0, 2), (2, 1)):
            args = (hierarchy(tag), inverses(tag, smoother), SMOOTHERS[smoother][1], rhs_of(tag))
            a = host_amg_cycle_jacobi(*args, np.zeros(m), pre, post)
            b = host_amg_cycle_jacobi(*args, np.full(m, np.nan), pre, post, zero=True)  # what x holds is never read
            assert np.array_equal(a, b), (tag, smoother, pre, post)


@pytest.mark.parametrize("tag,smoother", CASES)
def test_host_amg_pcg_on_jacobi(tag, smoother):
    """AMG-PCG at rtol 1e-10 converges with the pinned count, in both summation orders, in fewer iterations than unpreconditioned CG and more
    than the Gauss-Seidel hierarchy; the two history entries on either side of the threshold lie farther from it than their tolerance, so the
    device's count must be the host's; the true residual a tenth of the bound."""
    tols = jacobi_history_tolerances(tag, smoother)
    for reverse in (False, True):
        s = jacobi_solve(tag, smoother, reverse)
        n = s["iterations"]
        assert s["status"] == 1 and n == PCG_JACOBI_COUNTS[smoother][tag] and len(s["iterates"]) == n, (tag, smoother, reverse, n)
        tol2, h = s["state"]["tol2"], s["history"]
        assert np.all(h[:-1] > tol2) and h[-1] <= tol2
        for k in (n - 1, n):
            assert abs(h[k] - tol2) > tols[k] * h[k], (tag, smoother, reverse, k, h[k], tol2, tols[k])
    s = jacobi_solve(tag, smoother)
    status, plain = plain_count(tag)
    gs = {**PCG_COUNTS, **PCG_IRREGULAR_COUNTS}[tag]
    res = true_residual(tag, s["x"])
    print(f"{tag} {smoother}: {s['iterations']} iterations (Gauss-Seidel {gs}, none {plain} with status {status}), true relative residual {res:.2e}, "
          f"threshold margins {abs(h[-2] - tol2) / h[-2]:.2g} above and {abs(h[-1] - tol2) / h[-1]:.2g} below")
    assert plain == NONE_COUNTS[tag] and status == (0 if plain == 1000 else 1)
    assert gs < s["iterations"] < plain, (tag, smoother)
    assert res <= PCG_JACOBI_RESIDUAL_BOUND / 10, (tag, smoother, res)


@pytest.mark.parametrize("tag,smoother", CASES)
def test_the_spreads(tag, smoother):
    """The spreads of the module docstring, measured again: the GPU suite's tolerances are 100 times these constants."""
    fwd, rev = jacobi_iterates(tag, smoother), jacobi_iterates(tag, smoother, True)
    cycles = max(float(np.max(np.abs(a - b)) / np.max(np.abs(a))) for a, b in zip(fwd, rev))
    a, b = jacobi_solve(tag, smoother), jacobi_solve(tag, smoother, True)
    assert a["iterations"] == b["iterations"]
    solves = max(float(np.max(np.abs(u - v)) / np.max(np.abs(u))) for u, v in zip(a["iterates"], b["iterates"]))
    print(f"{tag} {smoother}: forward against reversed: the cycles' iterates {cycles:.3g}, the solve's iterates {solves:.3g}")
    assert cycles <= JACOBI_ITERATE_SPREAD and solves <= PCG_JACOBI_ITERATE_SPREAD, (tag, smoother, cycles, solves)
    assert ITERATE_SPREAD < JACOBI_ITERATE_SPREAD  # (were it under the Gauss-Seidel cycle's constant, the two would share it)


def test_pre_post_two_needs_fewer_iterations():
    """pre = post = 2 on the l1 hierarchy: fewer iterations than pre = post = 1 on every case."""
    for tag in ("grid24", "fem_scaled", "graph608"):
        two, one = jacobi_solve(tag, "l1_jacobi", False, 2, 2), jacobi_solve(tag, "l1_jacobi")
        print(f"{tag}: pre = post = 2: {two['iterations']} iterations, pre = post = 1: {one['iterations']}")
        assert two["status"] == 1 and two["iterations"] < one["iterations"], tag


def host_amg_cycle_gs(h, omega, b, x, pre=1, post=1, direction="symmetric", reverse=False, depth=0):
    """tests/test_amg_host.py host_amg_cycle with the sweeps' relaxation: what amg_cycle does on a "gs" hierarchy of smoother_omega = omega."""
    levels, coarsest = h
    if depth == len(levels):
        return host_dense_apply(coarsest["m"], coarsest["inv"], b)
    lv = levels[depth]
    m, (rp, ci, v) = lv["m"], lv["A"]
    for _ in range(pre):
        x = host_gs_sweep(m, rp, ci, v, lv["color_ptr"], lv["color_rows"], b, x, omega, direction)
    r = b - host_spmv(lv["A"], x, reverse)
    bc = host_spmv(lv["R"], r, reverse)
    xc = host_amg_cycle_gs(h, omega, bc, np.zeros(lv["mc"]), pre, post, direction, reverse, depth + 1)
    x = x + host_spmv(lv["P"], xc, reverse)
    for _ in range(post):
        x = host_gs_sweep(m, rp, ci, v, lv["color_ptr"], lv["color_rows"], b, x, omega, direction)
    return x


GS_OMEGA = 0.8  # the relaxed Gauss-Seidel hierarchy of the GPU suite


@functools.lru_cache(maxsize=None)
def gs_omega_iterates(tag, omega=GS_OMEGA, reverse=False, cycles=4):
    m = problem(tag)[0]
    b, x, out = rhs_of(tag), np.zeros(m), []
    for _ in range(cycles):
        x = host_amg_cycle_gs(hierarchy(tag), omega, b, x, reverse=reverse)
        out.append(x)
    return tuple(out)


def test_the_gauss_seidel_cycle_takes_its_omega():
    """smoother_omega reaches the Gauss-Seidel sweeps: at 1.0 the cycle is host_amg_cycle's to the bit, at 0.8 it is another cycle, which
    still reduces the residual every time and whose forward-against-reversed spread stays under ITERATE_SPREAD (the GPU suite's tolerance)."""
    from test_amg_host import iterates

    for tag in ("grid24", "fem_weak"):
        one = gs_omega_iterates(tag, 1.0)
        assert all(np.array_equal(a, b) for a, b in zip(one, iterates(tag)[:4])), tag
        fwd, rev = gs_omega_iterates(tag), gs_omega_iterates(tag, GS_OMEGA, True)
        assert not np.array_equal(fwd[0], one[0])
        res = relative_residuals(tag, fwd)
        assert all(later < earlier for earlier, later in zip([1.0] + res, res)), (tag, res)
        spread = max(float(np.max(np.abs(a - b)) / np.max(np.abs(a))) for a, b in zip(fwd, rev))
        print(f"{tag}: Gauss-Seidel at omega {GS_OMEGA}: residuals {['%.2e' % r for r in res]}, spread {spread:.3g}")
        assert spread <= ITERATE_SPREAD, (tag, spread)


def test_amg_wrappers_refuse_a_bad_smoother(monkeypatch):
    """Bad values raise SpmvAccError before the library is loaded; the hierarchy still constructs with two arguments and the level keeps its
    field order."""
    import spmv_acc_amd
    from spmv_acc_amd import amg
    from test_coo_host import _f, _i

    def no_library(*a, **k):
        raise AssertionError("the library must not be loaded")

    monkeypatch.setattr(spmv_acc_amd, "load_library", no_library)
    E = spmv_acc_amd.SpmvAccError
    args = (10, _i(11), _i(30), _f(30))
    for bad in ("sgs", "l1", "Jacobi", None, 1):
        with pytest.raises(E, match="smoother"):
            spmv_acc_amd.amg_setup(*args, smoother=bad)
    for smoother in ("gs", "jacobi", "l1_jacobi"):
        for bad in (float("nan"), float("inf"), 0.0, "1"):
            with pytest.raises(E, match="smoother_omega"):
                spmv_acc_amd.amg_setup(*args, smoother=smoother, smoother_omega=bad)
    h = spmv_acc_amd.AmgHierarchy([], amg.AmgCoarsest(0, None, None, "coarse_rows"))
    assert h.smoother == "gs" and h.smoother_omega == 1.0 and h.sizes == [0]
    assert amg.AmgLevel._fields[:11] == ("m", "mc", "A", "P", "R", "color_ptr", "color_rows", "r", "bc", "xc", "keep")
    assert amg.AmgLevel._fields[11:] == ("dinv", "xw") and amg.AmgLevel._field_defaults == dict(dinv=None, xw=None)
    lv = amg.AmgLevel(1, 1, None, None, None, [0, 1], None, None, None, None, keep=())
    assert lv.dinv is None and lv.xw is None
    assert amg._SMOOTHERS == {"gs": (None, 1.0), "jacobi": ("jacobi", 2.0 / 3.0), "l1_jacobi": ("l1", 1.0)}
    with pytest.raises(E, match="direction"):
        spmv_acc_amd.amg_cycle(spmv_acc_amd.AmgHierarchy([], None, smoother="l1_jacobi"), _f(1), _f(1), direction="sideways", zero_start=True)
    for word in ("DAMPING PLAIN JACOBI IS THE CALLER'S RESPONSIBILITY", "l1_jacobi", "smoother_omega"):
        assert word in spmv_acc_amd.amg_setup.__doc__, word
    assert "zero_start" in spmv_acc_amd.amg_cycle.__doc__ and "csr_jacobi_sweep" in amg.__doc__
