"""CPU side of the AMG hierarchy and the V-cycle (spmv_acc_amd/amg.py; no GPU): amg_setup and amg_cycle restated from the host models of the
entries they compose -- host_csr_strength, host_csr_aggregate, host_tentative_values, host_strength_values, host_spgemm, host_csr_color,
host_gs_sweep, host_dense_inverse and host_dense_apply -- and exported to the GPU suite as its reference.  Pinned here: the level sizes of four
hierarchies and the rule that ends each, and the convergence of ten V-cycles.

MEASURED with this file's model (multicolour Gauss-Seidel, pre = post = 1, symmetric sweeps, b standard normal from seed 5, x0 = 0), the
relative residual |b - A x| / |b| after ten cycles and the worst per-cycle factor:
    grid24   [576, 84, 6]      8.6e-06   0.45
    grid48   [2304, 341, 24]   9.7e-05   0.52
    aniso48  [2304, 648, 197]  5.1e-05   0.44   (ended by the stall rule: 197 rows give 194 aggregates)
    aniso24  [576, 167, 56]    2.8e-05   0.39   (ended by the stall rule)
RESIDUAL_BOUND is ten times the largest of them, 9.7e-4, rounded up to a power of ten: 1e-3.

The spreads the GPU suite's tolerances come from (two host restatements that differ only in summation order), largest over the four
hierarchies: the products P and A_c of the host_spgemm chain against scipy.sparse, entry by entry relative to the matrix' largest magnitude:
0.0 on all four (PRODUCT_SPREAD: the two add the few products of an entry in the same order); the iterates of ten cycles with forward against
reversed SpMV row sums, relative to the iterate's largest magnitude: 3.2e-16, 7.5e-16, 2.3e-15 and 1.1e-15 (ITERATE_SPREAD: 2.4e-15)."""
import functools

import numpy as np
import pytest

from test_agg_host import grid5_matrix, host_csr_aggregate, host_tentative_values
from test_dense_host import host_dense_apply, host_dense_inverse, to_dense
from test_gs_host import host_csr_color, host_gs_sweep
from test_spgemm_host import host_spgemm
from test_strength_host import EPS, aniso_matrix, host_csr_strength, host_strength_values

OMEGA = 2.0 / 3.0
CYCLES = 10
RESIDUAL_BOUND = 1e-3  # (the docstring: ten times the largest measured value, rounded up to a power of ten)
PRODUCT_SPREAD, ITERATE_SPREAD = 0.0, 2.4e-15  # (the docstring; test_the_spreads holds them to this file's model)
# tag -> (the matrix, theta, coarse_rows, the level sizes, the rule that ends the hierarchy)
HIERARCHIES = {
    "grid24": (lambda: grid5_matrix(24), 0.0, 16, [576, 84, 6], "coarse_rows"),
    "grid48": (lambda: grid5_matrix(48), 0.0, 64, [2304, 341, 24], "coarse_rows"),
    "aniso48": (lambda: aniso_matrix(48, EPS), 0.25, 64, [2304, 648, 197], "stall"),
    "aniso24": (lambda: aniso_matrix(24, EPS), 0.25, 16, [576, 167, 56], "stall"),
}
TAGS = tuple(HIERARCHIES)


# ---- the pieces the entries' host models do not already give -------------------------------------------------------------------------------------
def host_transpose(m, n, A):
    """The stable transpose (csr_transpose): the entries of a column in ascending source position."""
    rp, ci, v = A
    order = np.argsort(ci, kind="stable")
    t_rp = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(ci, minlength=n), out=t_rp[1:])
    return t_rp, np.repeat(np.arange(m, dtype=np.int32), np.diff(rp))[order], v[order]


def host_spmv(A, x, reverse=False):
    """A x with every row's products added one after the other from the row's first entry (reverse: from its last)."""
    rp, ci, v = A
    rp = rp.astype(np.int64)
    lens = np.diff(rp)
    acc = np.zeros(lens.size)
    for t in range(int(lens.max()) if lens.size else 0):
        live = t < lens
        p = np.where(live, rp[1:] - 1 - t if reverse else rp[:-1] + t, 0)
        term = v[p] * x[ci[p]]
        acc = np.where(live, term if t == 0 else acc + term, acc)
    return acc


# ---- amg_setup, restated ---------------------------------------------------------------------------------------------------------------------------
def host_amg_setup(m, A, theta=0.0, omega=OMEGA, coarse_rows=256, max_levels=16, b=None):
    """(levels, coarsest): levels = dicts of m, mc, A, P, R (CSR triples), color_ptr, color_rows; coarsest = dict of m, A, inv, info, rule."""
    levels, level = [], 1
    while True:
        rp, ci, v = A
        rule = "coarse_rows" if m <= coarse_rows else ("max_levels" if level == max_levels else None)
        if rule is None:
            s_rp, s_ci, smap, drop_ptr, nnz_s, _, _ = host_csr_strength(m, rp, ci, v, theta)
            agg, agg_rows, agg_ptr, naggs = host_csr_aggregate(m, s_rp, s_ci)
            if 2 * naggs > m:
                rule = "stall"
        if rule is not None:
            inv, info = host_dense_inverse(m, rp, ci, v)
            return levels, dict(m=m, A=A, inv=inv, info=info, rule=rule)
        p_value, _, bc = host_tentative_values(m, naggs, agg, agg_ptr[:naggs + 1], agg_rows, b)
        T = (np.arange(m + 1, dtype=np.int32), agg, p_value)
        m_value, _ = host_strength_values(m, nnz_s, s_rp, s_ci, smap, drop_ptr, v, omega)
        c = host_spgemm(m, m, naggs, (s_rp, s_ci, m_value), T)
        P = (c[0], c[1], c[5])
        R = host_transpose(m, naggs, P)
        c = host_spgemm(m, m, naggs, A, P)
        AP = (c[0], c[1], c[5])
        c = host_spgemm(naggs, m, naggs, R, AP)
        _, color_rows, color_ptr, _ = host_csr_color(m, rp, ci)
        levels.append(dict(m=m, mc=naggs, A=A, P=P, R=R, color_ptr=color_ptr, color_rows=color_rows, M=(s_rp, s_ci, m_value), T=T))
        A, m, b = (c[0], c[1], c[5]), naggs, bc
        level += 1


def host_amg_cycle(h, b, x, pre=1, post=1, direction="symmetric", reverse=False, depth=0):
    """One V-cycle; returns the new x.  reverse: the SpMVs add their rows from the last entry (the other summation order of the spread)."""
    levels, coarsest = h
    if depth == len(levels):
        return host_dense_apply(coarsest["m"], coarsest["inv"], b)
    lv = levels[depth]
    m, (rp, ci, v) = lv["m"], lv["A"]
    for _ in range(pre):
        x = host_gs_sweep(m, rp, ci, v, lv["color_ptr"], lv["color_rows"], b, x, 1.0, direction)
    r = b - host_spmv(lv["A"], x, reverse)
    bc = host_spmv(lv["R"], r, reverse)
    xc = host_amg_cycle(h, bc, np.zeros(lv["mc"]), pre, post, direction, reverse, depth + 1)
    x = x + host_spmv(lv["P"], xc, reverse)
    for _ in range(post):
        x = host_gs_sweep(m, rp, ci, v, lv["color_ptr"], lv["color_rows"], b, x, 1.0, direction)
    return x


# ---- the four hierarchies and their ten cycles, made once and shared with the GPU suite --------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hierarchy(tag):
    make, theta, coarse_rows, _, _ = HIERARCHIES[tag]
    m, A = make()
    return host_amg_setup(m, A, theta=theta, omega=OMEGA, coarse_rows=coarse_rows)


def rhs(m):
    return np.random.default_rng(5).standard_normal(m)


@functools.lru_cache(maxsize=None)
def iterates(tag, reverse=False):
    """The iterate after each of the ten cycles (x0 = 0), as a tuple of arrays."""
    h = hierarchy(tag)
    m = h[0][0]["m"] if h[0] else h[1]["m"]
    b, x, out = rhs(m), np.zeros(m), []
    for _ in range(CYCLES):
        x = host_amg_cycle(h, b, x, reverse=reverse)
        out.append(x)
    return tuple(out)


def relative_residuals(tag, xs):
    levels, _ = hierarchy(tag)
    A = levels[0]["A"]
    b = rhs(levels[0]["m"])
    return [float(np.linalg.norm(b - host_spmv(A, x)) / np.linalg.norm(b)) for x in xs]


@pytest.mark.parametrize("tag", TAGS)
def test_level_sizes_and_the_rule_that_ends_them(tag):
    _, theta, coarse_rows, sizes, rule = HIERARCHIES[tag]
    levels, coarsest = hierarchy(tag)
    assert [lv["m"] for lv in levels] + [coarsest["m"]] == sizes and coarsest["rule"] == rule and coarsest["info"] == 0, tag
    assert all(lv["mc"] == nxt for lv, nxt in zip(levels, sizes[1:]))
    if rule == "stall":  # the integer rule 2 * naggs > m on the level that became the coarsest, which is above coarse_rows
        m, (rp, ci, v) = coarsest["m"], coarsest["A"]
        s_rp, s_ci = host_csr_strength(m, rp, ci, v, theta)[:2]
        naggs = host_csr_aggregate(m, s_rp, s_ci)[3]
        assert m > coarse_rows and 2 * naggs > m, (tag, m, naggs)
        if tag == "aniso48":
            assert (m, naggs) == (197, 194)
    else:
        assert coarsest["m"] <= coarse_rows < levels[-1]["m"]
    for lv in levels:  # every level is a Galerkin level: R = P^T, the coarse matrix symmetric to rounding
        P, R = to_dense(lv["m"], lv["mc"], *lv["P"]), to_dense(lv["mc"], lv["m"], *lv["R"])
        assert np.array_equal(R, P.T)


@pytest.mark.parametrize("tag", TAGS)
def test_ten_cycles_converge(tag):
    """The relative residual after ten cycles is below RESIDUAL_BOUND, and every cycle reduces it (the module docstring holds the figures)."""
    res = relative_residuals(tag, iterates(tag))
    factors = [b / a for a, b in zip([1.0] + res[:-1], res)]
    print(f"{tag}: sizes {HIERARCHIES[tag][3]}, relative residual after {CYCLES} cycles {res[-1]:.3e}, worst per-cycle factor {max(factors):.3f}")
    assert res[-1] <= RESIDUAL_BOUND and max(factors) < 1.0, (tag, res)


def test_one_level_is_a_direct_solve():
    """coarse_rows at or above m: no level above the coarsest, and a cycle is inv b."""
    levels, coarsest = hierarchy("grid24")
    m, A = coarsest["m"], coarsest["A"]  # (the 6-row matrix)
    h = host_amg_setup(m, A, coarse_rows=m)
    assert h[0] == [] and h[1]["rule"] == "coarse_rows" and h[1]["info"] == 0
    b = rhs(m)
    x = host_amg_cycle(h, b, np.zeros(m))
    assert np.allclose(to_dense(m, m, *A) @ x, b, rtol=0, atol=1e-13 * np.abs(b).max() * np.linalg.cond(to_dense(m, m, *A)))
    one = host_amg_setup(levels[0]["m"], levels[0]["A"], coarse_rows=16, max_levels=1)  # max_levels ends it as well
    assert one[0] == [] and one[1]["rule"] == "max_levels" and one[1]["m"] == 576


def spreads(tag):
    """(products, iterates): the spreads of the module docstring for one hierarchy."""
    import scipy.sparse as sp

    levels, _ = hierarchy(tag)
    worst = 0.0
    for k, lv in enumerate(levels):
        m, mc = lv["m"], lv["mc"]
        A = sp.csr_matrix((lv["A"][2], lv["A"][1], lv["A"][0]), shape=(m, m))
        P = sp.csr_matrix((lv["P"][2], lv["P"][1], lv["P"][0]), shape=(m, mc))
        M = sp.csr_matrix((lv["M"][2], lv["M"][1], lv["M"][0]), shape=(m, m))
        T = sp.csr_matrix((lv["T"][2], lv["T"][1], lv["T"][0]), shape=(m, mc))
        Ps = (M @ T).toarray()
        worst = max(worst, float(np.max(np.abs(Ps - P.toarray())) / np.max(np.abs(Ps))))
        Ac = (P.T @ (A @ P)).toarray()
        nxt = levels[k + 1]["A"] if k + 1 < len(levels) else hierarchy(tag)[1]["A"]
        worst = max(worst, float(np.max(np.abs(Ac - to_dense(mc, mc, *nxt))) / np.max(np.abs(Ac))))
    fwd, rev = iterates(tag), iterates(tag, True)
    return worst, max(float(np.max(np.abs(a - b)) / np.max(np.abs(a))) for a, b in zip(fwd, rev))


@pytest.mark.parametrize("tag", TAGS)
def test_the_spreads(tag):
    """The two spreads of the module docstring, measured again: the GPU suite's tolerances are 100 times these constants."""
    products, its = spreads(tag)
    print(f"{tag}: products against scipy.sparse {products:.3g}, iterates forward against reversed {its:.3g}")
    assert products <= PRODUCT_SPREAD and its <= ITERATE_SPREAD, (tag, products, its)


if __name__ == "__main__":
    for t in TAGS:
        lv, co = hierarchy(t)
        r = relative_residuals(t, iterates(t))
        f = [b / a for a, b in zip([1.0] + r[:-1], r)]
        print(t, [x["m"] for x in lv] + [co["m"]], co["rule"], f"{r[-1]:.3e}", f"{max(f):.3f}", spreads(t))
