"""CPU side of the AMG hierarchy and the V-cycle (spmv_acc_amd/amg.py; no GPU): amg_setup and amg_cycle restated from the host models of the
entries they compose -- host_csr_strength, host_csr_aggregate, host_tentative_values, host_strength_values, host_spgemm, host_csr_color,
host_gs_sweep, host_dense_inverse and host_dense_apply -- and exported to the GPU suite as its reference.  Pinned here: the level sizes of four
hierarchies and the rule that ends each, and the convergence of ten V-cycles; the same for five irregular cases under every cycle option (below);
the wrappers' refusals.

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
reversed SpMV row sums, relative to the iterate's largest magnitude: 3.2e-16, 7.5e-16, 2.3e-15 and 1.1e-15 (ITERATE_SPREAD: 2.4e-15).

THE IRREGULAR CASES (IRREGULAR, beside the four grids): unstructured patterns whose coarse levels are no stencils, off-diagonals of mixed sign
that a theta > 0 drops and lumps, a matrix scaled over six decades, a near-nullspace vector handed to the setup, and max_levels ending a
working hierarchy.  The values are weak_spd's: a pure function of the unordered pair and a seed, magnitudes 0.25 .. 4.25, the diagonal the
row's absolute sum plus a small shift.  Nothing in the recipe is unseeded, and nothing in it was tuned: the seeds 11, 13, 608, 609 and 77, the
shifts and the thetas are the first ones tried, and every condition the cases must meet held with them (fem_scaled ends by the stall rule at
19 rows, which is pinned as it comes out; three of the five cases have three levels).
MEASURED with this file's model (b = rhs_of(tag), x0 = 0): the level sizes, the rule, the longest row of each level, the share of the finest
level's entries that theta drops, and the relative residual after ten cycles under (pre, post, direction) = (1, 1, symmetric), (0, 2, forward),
(2, 0, backward), (1, 0, symmetric) -- every cycle of every variant reduces the residual, the worst per-cycle factor is the last figure:
    fem_weak      [450, 41, 5]   coarse_rows  rows of 9, 14, 5    dropped 0       5.2e-05  2.0e-04  8.7e-04  2.8e-03   0.63
    fem_mixed     [450, 43]      stall        rows of 9, 14       dropped 10.5 %  1.3e-08  5.9e-08  8.2e-08  1.4e-05   0.41
    fem_scaled    [450, 43, 19]  stall        rows of 9, 14, 13   dropped 10.5 %  8.5e-08  1.8e-07  2.8e-07  3.5e-05   0.44
    graph608      [608, 58, 9]   stall        rows of 14, 50, 1   dropped 0.9 %   1.9e-02  1.7e-02  8.8e-02  9.8e-02   0.90
    graph608_two  [608, 58]      max_levels   rows of 14, 50      dropped 0       3.2e-07  5.8e-07  4.1e-07  1.5e-04   0.51
(graph608: the 8 rows that hold only their diagonal stay aggregates of one row on every level; its third level is diagonal.)  The GPU suite
holds the device's residual of each case and variant below residual_bound() of the host's: ten times it, rounded up to a power of ten.
The iterates' spread, forward against reversed SpMV row sums, the largest over the four variants and ten cycles: 2.26e-15, 2.9e-16, 3.7e-16,
2.5e-17 and 8.4e-17 -- all under ITERATE_SPREAD, which the irregular cases therefore share.  The products of the host chain against
scipy.sparse differ by 0, 0, 0, 4.9e-16 and 3.3e-16: scipy adds the up to 50 products of an entry in another order, so that comparison
supports no tolerance here, and the GPU suite needs none: it compares the device's values with the host chain to the bit, on the documented
summation order of each entry.  Nobody has measured the device's spreads on these cases: the tolerances come from this model alone."""
import functools

import numpy as np
import pytest

from test_agg_host import grid5_matrix, host_csr_aggregate, host_tentative_values
from test_dense_host import host_dense_apply, host_dense_inverse, to_dense
from test_gs_host import cases as gs_cases
from test_gs_host import host_csr_color, host_gs_sweep, mix32
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
# the cycle variants of the irregular cases: (pre, post, direction)
VARIANTS = ((1, 1, "symmetric"), (0, 2, "forward"), (2, 0, "backward"), (1, 0, "symmetric"))


# ---- the irregular cases: unstructured patterns, mixed signs, a bad scaling, a near-nullspace vector, max_levels ------------------------------------------
def pair_hash(i, j, seed):
    """32 bits that depend on the unordered pair (min(i, j), max(i, j)) and the seed alone."""
    lo, hi = np.minimum(i, j).astype(np.uint64), np.maximum(i, j).astype(np.uint64)
    return mix32(mix32(lo + np.uint64(seed) * np.uint64(0x9E3779B1)) + hi * np.uint64(0x85EBCA6B))


def weak_spd(m, pairs, seed, shift, positive_in=0):
    """(m, A): the CSR of the set of (i, j) with the full diagonal added.  An off-diagonal is a function of its unordered pair and the seed
    (symmetric): magnitude 0.25 + 4 k / 4096 for a hashed k < 4096, negative -- or, for one hashed pair in `positive_in` (0: none), positive.
    The diagonal is its row's sum of |a_ij| plus shift: SPD by a weak dominance."""
    i, j = np.array(sorted(set(pairs) | {(k, k) for k in range(m)}), dtype=np.int64).reshape(-1, 2).T
    rp = np.zeros(m + 1, dtype=np.int32)
    np.cumsum(np.bincount(i, minlength=m), out=rp[1:])
    h = pair_hash(i, j, seed)
    v = -(0.25 + 4.0 * (h % np.uint64(4096)).astype(np.float64) / 4096.0)
    if positive_in:
        v = np.where(mix32(h + np.uint64(1)) % np.uint64(positive_in) == 0, -v, v)
    off = np.bincount(i[i != j], weights=np.abs(v[i != j]), minlength=m)
    return m, (rp, j.astype(np.int32), np.where(i == j, off[i] + shift, v))


def fem_pairs():
    m, (rp, ci, _) = gs_cases()["fem"]
    assert m == 450
    return list(zip(np.repeat(np.arange(m), np.diff(rp)).tolist(), ci.tolist()))


def scaling():
    """d of fem_scaled: 10^u, u uniform in [-3, 3] (six decades)."""
    return 10.0 ** np.random.default_rng(77).uniform(-3.0, 3.0, 450)


def fem_scaled():
    m, (rp, ci, v) = weak_spd(450, fem_pairs(), 13, 0.05, positive_in=5)
    d = scaling()
    return m, (rp, ci, v * (d[np.repeat(np.arange(m), np.diff(rp))] * d[ci]))  # (d_i d_j is commutative: the values stay symmetric to the bit)


def graph608():
    """600 rows on a ring with 1300 seeded random symmetric pairs, then 8 rows that hold only their diagonal (the shift)."""
    rng = np.random.default_rng(608)
    a, b = rng.integers(0, 600, 1300), rng.integers(0, 600, 1300)
    pairs = [(i, (i + 1) % 600) for i in range(600)] + [(int(p), int(q)) for p, q in zip(a, b) if p != q]
    return weak_spd(608, pairs + [(q, p) for p, q in pairs], 608, 0.02)


# tag -> (the matrix, theta, coarse_rows, the level sizes, the rule that ends the hierarchy, max_levels, the near-nullspace vector or None)
IRREGULAR = {
    "fem_weak": (lambda: weak_spd(450, fem_pairs(), 11, 0.05), 0.0, 16, [450, 41, 5], "coarse_rows", 16, lambda: None),
    "fem_mixed": (lambda: weak_spd(450, fem_pairs(), 13, 0.05, positive_in=5), 0.05, 16, [450, 43], "stall", 16, lambda: None),
    "fem_scaled": (fem_scaled, 0.05, 16, [450, 43, 19], "stall", 16, lambda: 1.0 / scaling()),
    "graph608": (graph608, 0.02, 8, [608, 58, 9], "stall", 16, lambda: np.random.default_rng(609).uniform(0.5, 2.0, 608)),
    "graph608_two": (graph608, 0.0, 8, [608, 58], "max_levels", 2, lambda: None),
}
IRREGULAR_TAGS = tuple(IRREGULAR)
DROPPED = ("fem_mixed", "fem_scaled")  # the cases whose theta must drop between 5 % and 50 % of the finest level's entries


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


# ---- the hierarchies and their ten cycles, made once and shared with the GPU suite ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def problem(tag):
    """(m, A, theta, coarse_rows, max_levels, the near-nullspace vector or None) of a case of either table."""
    if tag in HIERARCHIES:
        make, theta, coarse_rows, _, _ = HIERARCHIES[tag]
        max_levels, near = 16, None
    else:
        make, theta, coarse_rows, _, _, max_levels, near = IRREGULAR[tag]
        near = near()
    m, A = make()
    return m, A, theta, coarse_rows, max_levels, near


@functools.lru_cache(maxsize=None)
def hierarchy(tag):
    m, A, theta, coarse_rows, max_levels, near = problem(tag)
    return host_amg_setup(m, A, theta=theta, omega=OMEGA, coarse_rows=coarse_rows, max_levels=max_levels, b=near)


def rhs(m):
    return np.random.default_rng(5).standard_normal(m)


def rhs_of(tag):
    """The right-hand side of a case: rhs(m), scaled by d on fem_scaled (the right-hand side of D A D y = D b)."""
    m = problem(tag)[0]
    return rhs(m) * scaling() if tag == "fem_scaled" else rhs(m)


@functools.lru_cache(maxsize=None)
def variant_iterates(tag, variant=VARIANTS[0], reverse=False):
    """The iterate after each of the ten cycles (x0 = 0) of one (pre, post, direction), as a tuple of arrays."""
    h = hierarchy(tag)
    m = problem(tag)[0]
    pre, post, direction = variant
    b, x, out = rhs_of(tag), np.zeros(m), []
    for _ in range(CYCLES):
        x = host_amg_cycle(h, b, x, pre, post, direction, reverse=reverse)
        out.append(x)
    return tuple(out)


def iterates(tag, reverse=False):
    """The same under pre = post = 1 and symmetric sweeps."""
    return variant_iterates(tag, VARIANTS[0], reverse)


def relative_residuals(tag, xs):
    A, b = problem(tag)[1], rhs_of(tag)
    return [float(np.linalg.norm(b - host_spmv(A, x)) / np.linalg.norm(b)) for x in xs]


def residual_bound(host_residual):
    """Ten times the host model's figure, rounded up to a power of ten: what the device's residual is held below."""
    return 10.0 ** int(np.ceil(np.log10(10.0 * host_residual)))


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



# ---- the irregular cases ---------------------------------------------------------------------------------------------------------------------------------
def strength_of(tag, m, A):
    """(nnz_s, naggs) of a level's strength filter and aggregation under the case's theta."""
    s_rp, s_ci = host_csr_strength(m, *A, problem(tag)[2])[:2]
    return int(s_ci.size), host_csr_aggregate(m, s_rp, s_ci)[3]


def dropped_share(tag):
    """The share of the finest level's entries that the strength filter drops (and lumps into the diagonal)."""
    lv = hierarchy(tag)[0][0]
    return 1.0 - lv["M"][1].size / lv["A"][1].size


@pytest.mark.parametrize("tag", IRREGULAR_TAGS)
def test_irregular_level_sizes_and_the_rule_that_ends_them(tag):
    """The pinned sizes and rule of each irregular case, and what makes the case worth having: a level above the coarsest, a symmetric matrix,
    Galerkin levels, the share theta drops, the near-nullspace vector reproduced by the tentative prolongator, graph608's singletons."""
    _, theta, coarse_rows, sizes, rule, max_levels, _ = IRREGULAR[tag]
    m, A, _, _, _, near = problem(tag)
    levels, coarsest = hierarchy(tag)
    longest = [int(np.diff(lv["A"][0]).max()) for lv in levels] + [int(np.diff(coarsest["A"][0]).max())]
    print(f"{tag}: sizes {[lv['m'] for lv in levels] + [coarsest['m']]}, rule {coarsest['rule']}, longest rows {longest}, "
          f"dropped at the finest level {dropped_share(tag):.3f} of {A[1].size}")
    assert [lv["m"] for lv in levels] + [coarsest["m"]] == sizes and coarsest["rule"] == rule and coarsest["info"] == 0, tag
    assert len(levels) >= 1 and all(lv["mc"] == nxt for lv, nxt in zip(levels, sizes[1:]))
    dense = to_dense(m, m, *A)
    assert np.array_equal(dense, dense.T) and np.all(np.linalg.eigvalsh(dense) > 0.0)  # symmetric to the bit, positive definite
    cm, cA = coarsest["m"], coarsest["A"]
    if rule == "stall":
        assert cm > coarse_rows and len(levels) + 1 < max_levels and 2 * strength_of(tag, cm, cA)[1] > cm
    elif rule == "max_levels":  # neither other rule would have ended it there
        assert len(levels) + 1 == max_levels and cm > coarse_rows and 2 * strength_of(tag, cm, cA)[1] <= cm
    else:
        assert cm <= coarse_rows < levels[-1]["m"] and len(levels) + 1 <= max_levels
    for lv in levels:
        P, R = to_dense(lv["m"], lv["mc"], *lv["P"]), to_dense(lv["mc"], lv["m"], *lv["R"])
        assert np.array_equal(R, P.T)
    if tag in DROPPED:
        assert 0.05 <= dropped_share(tag) <= 0.5, (tag, dropped_share(tag))
        kept = levels[0]["M"][1].size
        assert kept == strength_of(tag, m, A)[0] < A[1].size
        off = A[2][A[1] != np.repeat(np.arange(m), np.diff(A[0]))]
        assert 0.1 < np.mean(off > 0.0) < 0.3  # (about one off-diagonal in five is positive: the dropped ones are of both signs)
    # the tentative prolongator of the finest level is the near-nullspace vector, normalised aggregate by aggregate (the one-vector QR)
    T = levels[0]["T"]
    want = np.ones(m) if near is None else near
    norms = np.sqrt(np.bincount(T[1], weights=want * want, minlength=levels[0]["mc"]))
    assert np.allclose(T[2], want / norms[T[1]], rtol=1e-14, atol=0.0), tag
    if tag == "graph608":  # the 8 rows that hold only their diagonal stay aggregates of one row, and rows of one entry, on every level
        rows = np.arange(600, 608)
        for k, lv in enumerate(levels):
            assert np.all(np.diff(lv["A"][0])[rows] == 1)
            agg = lv["T"][1]
            assert np.all(np.bincount(agg, minlength=lv["mc"])[agg[rows]] == 1), k
            rows = agg[rows]
        assert np.unique(rows).size == 8 and np.all(np.diff(cA[0])[rows] == 1)
        assert longest[1] >= 40 and longest[2] == 1  # long rows out of the SpGEMM, then a diagonal third level


def test_three_irregular_hierarchies_have_three_levels():
    assert sum(len(IRREGULAR[t][3]) >= 3 for t in IRREGULAR_TAGS) >= 3
    assert {IRREGULAR[t][4] for t in IRREGULAR_TAGS} == {"coarse_rows", "stall", "max_levels"}


def variant_residuals(tag):
    """variant -> the relative residual after each of the ten cycles of the host model."""
    return {v: relative_residuals(tag, variant_iterates(tag, v)) for v in VARIANTS}


@pytest.mark.parametrize("tag", IRREGULAR_TAGS)
def test_irregular_cycles_converge(tag):
    """Ten stationary cycles reduce the residual in every cycle, in each (pre, post, direction) of VARIANTS; the variants differ (the model takes
    its options).  The module docstring holds the figures; the GPU suite's residual bounds are residual_bound() of them."""
    res = variant_residuals(tag)
    for v, r in res.items():
        factors = [b / a for a, b in zip([1.0] + r[:-1], r)]
        print(f"{tag} {v}: relative residual after {CYCLES} cycles {r[-1]:.3e} (bound {residual_bound(r[-1]):g}), worst per-cycle factor {max(factors):.3f}")
        assert max(factors) < 1.0, (tag, v, r)
    firsts = [variant_iterates(tag, v)[0] for v in VARIANTS]
    assert all(not np.array_equal(a, b) for k, a in enumerate(firsts) for b in firsts[k + 1:])


def variant_spread(tag):
    """The largest forward-against-reversed spread of the iterates over the four variants and the ten cycles."""
    return max(float(np.max(np.abs(a - b)) / np.max(np.abs(a))) for v in VARIANTS
               for a, b in zip(variant_iterates(tag, v), variant_iterates(tag, v, True)))


@pytest.mark.parametrize("tag", IRREGULAR_TAGS)
def test_the_irregular_spreads(tag):
    """The iterates' spread of the irregular cases fits under ITERATE_SPREAD (the docstring holds each figure).  The products' spread against
    scipy.sparse is printed, not held: the GPU suite compares the products with the host chain to the bit, on the entries' own contracts."""
    its = variant_spread(tag)
    print(f"{tag}: iterates forward against reversed, four variants {its:.3g}; products against scipy.sparse {spreads(tag)[0]:.3g}")
    assert its <= ITERATE_SPREAD, (tag, its)


def test_amg_wrappers_refuse_bad_arguments(monkeypatch):
    """Every argument check of amg_setup and amg_cycle raises SpmvAccError with its text before the library is loaded or a pointer taken."""
    import spmv_acc_amd
    from spmv_acc_amd.amg import AmgCoarsest
    from test_coo_host import _f, _i

    def no_library():
        raise AssertionError("the wrapper must refuse before it calls the library")

    monkeypatch.setattr(spmv_acc_amd, "load_library", no_library)
    E = spmv_acc_amd.SpmvAccError
    m, nnz = 10, 30
    A = (_i(m + 1), _i(nnz), _f(nnz))

    def setup(match, mm=m, A=A, **kw):
        with pytest.raises(E, match=match):
            spmv_acc_amd.amg_setup(mm, *A, **kw)

    setup(r"negative shape \(-1, -1\)", mm=-1)
    setup("coarse_rows = 0, max_levels = 16: both must be at least 1", coarse_rows=0)
    setup("coarse_rows = 256, max_levels = 0: both must be at least 1", max_levels=0)
    for theta in (-0.25, float("nan"), float("inf")):
        setup("theta = .*a finite threshold >= 0 is required", theta=theta)
    for omega in (0.0, float("nan"), float("inf"), -float("inf")):
        setup("omega = .*a finite, non-zero relaxation factor is required", omega=omega)
    for k, name in enumerate(("rowptr", "colindex", "value")):
        for bad in (None, [0] * 4):
            setup(name + ": a torch tensor on the GPU is required", A=A[:k] + (bad,) + A[k + 1:])

    h = spmv_acc_amd.AmgHierarchy([], AmgCoarsest(m, A, None, "coarse_rows"))

    def cycle(match, h=h, b=_f(m), x=_f(m), **kw):
        with pytest.raises(E, match=match):
            spmv_acc_amd.amg_cycle(h, b, x, **kw)

    for bad in (None, ([], None), "hierarchy"):
        cycle("h: the AmgHierarchy of amg_setup is required", h=bad)
    cycle(r"negative sweeps \(-1, 1\)", pre=-1)
    cycle(r"negative sweeps \(1, -1\)", post=-1)
    for bad in ("sideways", 2, None):
        cycle(r"amg_cycle: direction .*: one of \('forward', 'backward', 'symmetric'\)", direction=bad)
    cycle("b: a torch tensor on the GPU is required", b=None)
    cycle("b: a torch tensor on the GPU is required", b=[0.0] * m)
    cycle("x: a torch tensor on the GPU is required", x=None)
    cycle("x: a torch tensor on the GPU is required", x=np.zeros(m))
    # the text and the tuple are csr_gs_sweep's own
    monkeypatch.undo()
    with pytest.raises(E, match=r"^direction 'sideways': one of \('forward', 'backward', 'symmetric'\)$"):
        spmv_acc_amd.csr_gs_sweep(m, *A, [0, m], _i(m), _f(m), _f(m), direction="sideways")


if __name__ == "__main__":
    for t in TAGS:
        lv, co = hierarchy(t)
        r = relative_residuals(t, iterates(t))
        f = [b / a for a, b in zip([1.0] + r[:-1], r)]
        print(t, [x["m"] for x in lv] + [co["m"]], co["rule"], f"{r[-1]:.3e}", f"{max(f):.3f}", spreads(t))
    for t in IRREGULAR_TAGS:
        lv, co = hierarchy(t)
        print(t, [x["m"] for x in lv] + [co["m"]], co["rule"], f"dropped {dropped_share(t):.3f}", {v: f"{r[-1]:.3e}" for v, r in variant_residuals(t).items()},
              f"{variant_spread(t):.3g}", f"{spreads(t)[0]:.3g}")
