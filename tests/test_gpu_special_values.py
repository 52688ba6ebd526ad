"""GPU suite (-m gpu): NaN, +-Inf, overflowing products and subnormals through every kernel form and entry.

The kernels load more than they need -- 16-byte groups that straddle row ends, a tile's first group re-read by lanes past its end, the chunk's
base column gathered by lanes that own nothing, dead lanes given 0.0 or column 0 -- which is right only while a foreign product never reaches
a sum.  Finite data cannot show such a leak (a leaked 0 * x[c] is zero); a NaN or an Inf shows it at once.  The reference
(tests/special_values.py, checked on the CPU by tests/test_special_values_host.py) classifies every row from its own products, independent of
any summation order: non-finite rows must match in class exactly, finite rows within the project's scaled bound 1e-12.  The sign of a zero
result is not asserted.  Subnormal inputs are chosen so that every product and partial sum is exact: the results must be equal bit for bit,
which a flush to zero anywhere (a code path, a compiler flag, the atomic-add instruction) would break."""
import numpy as np
import pytest

import special_values as sv
import spmv_acc_amd

pytestmark = pytest.mark.gpu

ABS = ((1.0, 0.0), (-0.75, 0.0), (2.0, 0.5))  # (1, 0) runs over a y full of NaN
SENTINEL = 7.25


@pytest.fixture(scope="module")
def torch_dev(hiplib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def y_before(alpha, beta, y0):
    return np.full(y0.size, np.nan) if (alpha, beta) == (1.0, 0.0) else y0


class Refs:
    """One case's inputs per variant and their classification per (alpha, beta): computed once, shared, never written."""

    def __init__(self, case):
        self.case, self._inputs, self._refs = case, {}, {}

    def inputs(self, variant):
        if variant not in self._inputs:
            self._inputs[variant] = self.case.inputs(variant)
        return self._inputs[variant]

    def ref(self, variant, alpha, beta, xvariant=None):
        key = (variant, xvariant, alpha, beta)
        if key not in self._refs:
            c = self.case
            vals, x, y0 = self.inputs(variant)
            if xvariant is not None:
                x = self.inputs(xvariant)[1]
            self._refs[key] = sv.classify(alpha, beta, c.rowptr, c.cols, vals, x, y_before(alpha, beta, y0))
            for a in self._refs[key]:
                a.setflags(write=False)
        return self._refs[key]


@pytest.fixture(scope="module")
def refs_m():
    return Refs(sv.matrix_m())


def spmv(torch, strat, alpha, beta, c, drp, dci, dv, dx, y_start):
    dy = dev(torch, y_start)
    spmv_acc_amd.csr_spmv(alpha, beta, c.m, c.n, c.nnz, drp, dci, dv, dx, dy, strategy=strat)
    torch.cuda.synchronize()
    return dy.cpu().numpy()


def set_tunables(hiplib, knobs):
    hiplib.spmv_acc_reset_tunables()
    for k, v in knobs.items():
        assert hiplib.spmv_acc_set_tunable(k.encode(), v) == 0, k


# ---- a. every strategy under default tunables -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strat", spmv_acc_amd.STRATEGIES)
def test_every_strategy_classifies_every_row(torch_dev, refs_m, strat):
    """Matrix M with poison in x, in the values and in both: every row's class and every finite row's value, beta == 0 over a NaN y included."""
    torch = torch_dev
    c = refs_m.case
    drp, dci = dev(torch, c.rowptr), dev(torch, c.cols)
    try:
        for variant in ("x", "vals", "both"):
            vals, x, y0 = refs_m.inputs(variant)
            dv, dx = dev(torch, vals), dev(torch, x)
            for alpha, beta in ABS:
                ref, scale = refs_m.ref(variant, alpha, beta)
                got = spmv(torch, strat, alpha, beta, c, drp, dci, dv, dx, y_before(alpha, beta, y0))
                sv.check(got, ref, scale, (strat, variant, alpha, beta))
    finally:
        spmv_acc_amd.release_plans(drp)


@pytest.mark.parametrize("strat", spmv_acc_amd.STRATEGIES)
def test_alpha_zero_is_not_special_cased(torch_dev, refs_m, strat):
    """alpha == 0 still multiplies: 0 * Inf and 0 * NaN are NaN in the rows that hold them, every other row is a zero; beta == 0 over a NaN y."""
    torch = torch_dev
    c = refs_m.case
    vals, x, y0 = refs_m.inputs("x")
    drp, dci, dv, dx = (dev(torch, a) for a in (c.rowptr, c.cols, vals, x))
    dirty = ~np.isfinite(refs_m.ref("x", 1.0, 0.0)[0])  # the rows that hold a non-finite product: 0 * Inf and 0 * NaN make each of them a NaN
    assert dirty.sum() >= 0.005 * c.m
    try:
        for beta, ys in ((0.0, np.full(c.m, np.nan)), (0.5, y0)):
            ref, scale = sv.classify(0.0, beta, c.rowptr, c.cols, vals, x, ys)
            assert np.isnan(ref[dirty]).all() and (beta != 0 or np.array_equal(np.isnan(ref), dirty))
            sv.check(spmv(torch, strat, 0.0, beta, c, drp, dci, dv, dx, ys), ref, scale, (strat, "alpha 0", beta))
    finally:
        spmv_acc_amd.release_plans(drp)


# ---- b. pinned kernel forms -------------------------------------------------------------------------------------------------------------
FORMS = sv.MEASUREMENT_SWITCHES + sv.SLAB_FORMS


@pytest.mark.parametrize("part", range(4))
def test_pinned_forms_classify_every_row(torch_dev, hiplib, refs_m, part):
    """The engine's inventory of forms (tile sizes, staging orders, digests, segmented scan, carries, gather hints, the column codes where they
    can be built) plus column slabs, slab segments and the deterministic switch, on matrix M with poisoned x."""
    torch = torch_dev
    c = refs_m.case
    vals, x, y0 = refs_m.inputs("x")
    drp, dci, dv, dx = (dev(torch, a) for a in (c.rowptr, c.cols, vals, x))
    try:
        for strat, knobs in FORMS[part::4]:
            set_tunables(hiplib, knobs)
            spmv_acc_amd.release_plans(drp)  # analysis-level switches take effect when the plan is (re)built
            for alpha, beta in ((1.0, 0.0), (2.0, 0.5)):
                ref, scale = refs_m.ref("x", alpha, beta)
                got = spmv(torch, strat, alpha, beta, c, drp, dci, dv, dx, y_before(alpha, beta, y0))
                sv.check(got, ref, scale, (strat, knobs, alpha, beta))
            info = spmv_acc_amd.query_plan(drp, c.m)
            if "slab_segments" in knobs:
                assert info["slab_passes"] == knobs["slab_segments"], (strat, knobs, info)
            if "col_slabs" in knobs:
                assert hiplib.spmv_acc_cached_plans() > 1, (strat, knobs, info)  # the parent + its slabs
    finally:
        hiplib.spmv_acc_reset_tunables()
        spmv_acc_amd.release_plans()


# per L kind: (tunable col16, record sizes the plan may report, code width it must report).  col16 = 16 / 64 pin the record size (the width
# follows the rule: 16 bits where a chunk spans thousands of columns, 8 on the headline shape), 2 / 8 pin the width (the record size follows
# the escape statistics)
COL_CODE_TABLE = {
    "short rows, 10 % far": [(16, (16,), 16), (64, (64,), 16), (2, (16, 32, 64), 16)],
    "fem-like, 2 % far": [(16, (16,), 16), (64, (64,), 16), (2, (16, 32, 64), 16)],
    "headline-shaped": [(8, (16, 32, 64), 8), (16, (16,), 8), (64, (64,), 8)],
}


@pytest.mark.parametrize("kind", sv.L_KINDS)
def test_column_codes_classify_every_row(torch_dev, hiplib, kind):
    """Matrix L under the pinned column encoding: NaN in the base column that a chunk's non-owning lanes gather (no row references it), in
    column 0 (the clamped base of the first chunks), +-Inf in the column of an escaped entry -- through 16-int records (the 10 %-far matrix
    overflows them) and 64-int ones, 16- and 8-bit codes.  A plan that fell back to colindex fails the test: it would prove nothing."""
    torch = torch_dev
    c = sv.matrix_l(kind)
    vals, x, y0 = c.inputs("x")
    drp, dci, dv, dx = (dev(torch, a) for a in (c.rowptr, c.cols, vals, x))
    refs = {ab: sv.classify(ab[0], ab[1], c.rowptr, c.cols, vals, x, y_before(ab[0], ab[1], y0)) for ab in ABS}
    pins = COL_CODE_TABLE[kind]
    families = (("line_enhance", {"stream_plain": 1}, ("rowblock",)),
                ("flat", {"stream_plain": 1, "flat_rowblock": 0, "flat_npt": 8, "flat_finish": 1, "flat_early": 0}, ("flat_tile",)),
                ("flat", {"stream_plain": 1, "flat_rowblock": 0, "flat_npt": 8, "flat_finish": 0, "flat_early": 1}, ("flat_tile",)))
    try:
        for pin, want_rec, want_bits in pins:
            for strat, knobs, kernel in families:
                set_tunables(hiplib, dict(knobs, col16=pin))
                spmv_acc_amd.release_plans(drp)
                for alpha, beta in ABS:
                    ref, scale = refs[(alpha, beta)]
                    got = spmv(torch, strat, alpha, beta, c, drp, dci, dv, dx, y_before(alpha, beta, y0))
                    info = spmv_acc_amd.query_plan(drp, c.m)
                    assert info["last_kernel"] in kernel, (kind, pin, strat, info)
                    assert info["col16"] in want_rec and info["col_bits"] == want_bits, (kind, pin, strat, info)
                    sv.check(got, ref, scale, (kind, pin, strat, alpha, beta))
    finally:
        hiplib.spmv_acc_reset_tunables()
        spmv_acc_amd.release_plans()


# ---- c. plan reuse ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strat", ["line_enhance", "flat", "adaptive"])
def test_a_plan_serves_clean_and_poisoned_calls_alike(torch_dev, hiplib, refs_m, strat):
    """A plan built and timed on clean data classifies a later poisoned call, and a plan whose first call -- timing trials included -- ran on
    poisoned data keeps its verdict, leaves no NaN behind in y where beta == 0, and serves a later clean call."""
    torch = torch_dev
    c = refs_m.case
    vals, x_bad, y0 = refs_m.inputs("x")
    x_clean = refs_m.inputs("vals")[1]
    try:
        for first in ("clean", "poisoned"):
            drp, dci, dv = dev(torch, c.rowptr), dev(torch, c.cols), dev(torch, vals)  # (a fresh rowptr: a fresh plan)
            dx = dev(torch, x_clean if first == "clean" else x_bad)
            if first == "clean":
                spmv_acc_amd.prepare(c.m, c.n, c.nnz, drp, dci, dv, dx, strategy=strat, beta=0.0)
                order = ("vals", None, "vals")
            else:
                ref, scale = refs_m.ref("x", 1.0, 0.0)
                sv.check(spmv(torch, strat, 1.0, 0.0, c, drp, dci, dv, dx, np.full(c.m, np.nan)), ref, scale, (strat, "first call on poison"))
                spmv_acc_amd.prepare(c.m, c.n, c.nnz, drp, dci, dv, dx, strategy=strat, beta=0.0)  # (the rest of the timings, on poisoned data)
                order = (None, "vals", None)
            assert spmv_acc_amd.query_plan(drp, c.m)["settled"], (strat, first)
            for xvariant in order:
                dx.copy_(dev(torch, x_clean if xvariant else x_bad))
                for alpha, beta in ((1.0, 0.0), (2.0, 0.5)):
                    ref, scale = refs_m.ref("x", alpha, beta, xvariant)
                    got = spmv(torch, strat, alpha, beta, c, drp, dci, dv, dx, y_before(alpha, beta, y0))
                    sv.check(got, ref, scale, (strat, first, xvariant, alpha, beta))
            spmv_acc_amd.release_plans(drp)
    finally:
        hiplib.spmv_acc_reset_tunables()
        spmv_acc_amd.release_plans()


# ---- d. SpMM ----------------------------------------------------------------------------------------------------------------------------
def xy_views(torch, X, Y0, layout, ldx_pad=3, ldy_pad=5):
    (n, k), m = X.shape, Y0.shape[0]
    if layout == "row":
        dXb = torch.zeros((n, k + ldx_pad), dtype=torch.float64, device="cuda")
        dYb = torch.full((m, k + ldy_pad), SENTINEL, dtype=torch.float64, device="cuda")
        dX, dY, pad = dXb[:, :k], dYb[:, :k], dYb[:, k:]
    else:
        dXb = torch.zeros((k, n + ldx_pad), dtype=torch.float64, device="cuda")
        dYb = torch.full((k, m + ldy_pad), SENTINEL, dtype=torch.float64, device="cuda")
        dX, dY, pad = dXb[:, :n].t(), dYb[:, :m].t(), dYb[:, m:]
    dX.copy_(torch.from_numpy(X))
    dY.copy_(torch.from_numpy(Y0))
    return dX, dY, pad


POISONED_COLUMNS = {1: (0,), 2: (1,), 3: (1,), 8: (0, 5)}


@pytest.mark.parametrize("layout", ["row", "col"])
def test_spmm_keeps_poison_in_its_column(torch_dev, refs_m, layout):
    """Column c of Y is classified from column c of X alone: a NaN in X[:, c] must not reach Y[:, c' != c], although one 16-byte load fetches
    both.  Poisoned values under a clean X, an un-rebased row range and the padding beyond k (kept bit for bit) as well."""
    torch = torch_dev
    c = refs_m.case
    sentinel = torch.tensor([SENTINEL], dtype=torch.float64).view(torch.int64).item()
    x_bad, x_clean = refs_m.inputs("x")[1], refs_m.inputs("vals")[1]
    y0 = refs_m.inputs("x")[2]
    drp, dci = dev(torch, c.rowptr), dev(torch, c.cols)
    a, b = 3, 9000  # the un-rebased row range: rowptr + a, the whole colindex / values, nnz = rowptr[b]
    sub_rp = (c.rowptr[a:b + 1] - c.rowptr[a]).astype(np.int32)
    sl = slice(int(c.rowptr[a]), int(c.rowptr[b]))
    try:
        for variant, ks in (("x", (1, 2, 3, 8)), ("vals", (3,))):
            vals = refs_m.inputs(variant)[0]
            dv = dev(torch, vals)
            for k in ks:
                bad = POISONED_COLUMNS[k] if variant == "x" else ()
                # clean columns differ from each other, so a column read in another's place shows as well
                X = np.stack([x_bad if j in bad else x_clean * (1.0 + 0.125 * j) for j in range(k)], axis=1)
                Y0 = np.stack([y0 * (1.0 + j) for j in range(k)], axis=1)
                for alpha, beta in ((1.0, 0.0), (2.0, 0.5)):
                    Ys = np.full_like(Y0, np.nan) if beta == 0 else Y0
                    dX, dY, pad = xy_views(torch, X, Ys, layout)
                    spmv_acc_amd.csr_spmm(alpha, beta, c.m, c.n, c.nnz, drp, dci, dv, dX, dY)
                    torch.cuda.synchronize()
                    got = dY.cpu().numpy()
                    assert bool((pad.contiguous().view(torch.int64) == sentinel).all()), (layout, variant, k, "padding")
                    for j in range(k):
                        ref, scale = sv.classify(alpha, beta, c.rowptr, c.cols, vals, X[:, j], Ys[:, j])
                        sv.check(got[:, j], ref, scale, (layout, variant, k, j, alpha, beta))
                if k in (3, 8):
                    dX, dY, pad = xy_views(torch, X, Y0[a:b], layout)
                    spmv_acc_amd.csr_spmm(2.0, 0.5, b - a, c.n, int(c.rowptr[b]), drp[a:b + 1], dci, dv, dX, dY)
                    torch.cuda.synchronize()
                    got = dY.cpu().numpy()
                    assert bool((pad.contiguous().view(torch.int64) == sentinel).all()), (layout, variant, k, "padding, row range")
                    for j in range(k):
                        ref, scale = sv.classify(2.0, 0.5, sub_rp, c.cols[sl], vals[sl], X[:, j], Y0[a:b, j])
                        sv.check(got[:, j], ref, scale, (layout, variant, k, j, "row range"))
    finally:
        spmv_acc_amd.release_plans()


# ---- e. the transposed product ----------------------------------------------------------------------------------------------------------
def transposed_inputs(c, seed=6):
    """x over the ROWS of matrix M with a few non-finite entries (short rows, the 700- and the 3000-row, an empty row, a row next to the
    single-entry ones whose 2^600 meet 2^500), y0 over its columns, and colindex with out-of-range columns beside poisoned entries."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.5, 2.0, c.m) * rng.choice([-1.0, 1.0], c.m)
    y0 = rng.standard_normal(c.n)
    y0[[5, c.n // 2, c.n - 3]] = sv.POISON
    poisoned = {0: np.nan, 99: np.inf, 100: -np.inf, 101: np.nan, 4000: np.inf, 5000: np.nan, 6001: -np.inf, 9500: np.inf, c.m - 2: -np.inf}
    for r, v in poisoned.items():
        x[r] = v
    x[c.singles] = sv.BIG_X
    cols = c.cols.copy()
    for r, k in ((99, 0), (101, 1), (5000, 7), (9500, 63)):  # dropped, whatever their product would have been
        cols[c.rowptr[r]] = c.n + k
    cols[c.rowptr[5000] + 1] = -1 - 3
    return x, y0, cols


def test_spmv_t_poison_reaches_its_pattern_only(torch_dev, refs_m):
    """A non-finite x[row] reaches exactly the columns of that row's pattern; every other column stays finite and within the bound of
    tests/test_gpu_transpose.py, columns no row references keep beta * y bit for bit, out-of-range columns beside poisoned entries are
    dropped and nothing is written past y."""
    torch = torch_dev
    c = refs_m.case
    x, y0, cols = transposed_inputs(c)
    vals = refs_m.inputs("x")[0]  # (a stored zero and the +-2^600 of the single-entry rows)
    drp, dci, dv, dx = (dev(torch, a) for a in (c.rowptr, cols, vals, x))
    pad = 64
    for alpha, beta in ABS:
        ys = y_before(alpha, beta, y0)
        buf = torch.full((c.n + pad,), SENTINEL, dtype=torch.float64, device="cuda")
        buf[:c.n] = dev(torch, ys)
        spmv_acc_amd.csr_spmv_t(alpha, beta, c.m, c.n, c.nnz, drp, dci, dv, dx, buf[:c.n])
        torch.cuda.synchronize()
        got = buf[:c.n].cpu().numpy()
        assert bool((buf[c.n:] == SENTINEL).all()), (alpha, beta, "wrote past y")
        ref, scale = sv.classify_t(alpha, beta, c.rowptr, cols, vals, x, ys, c.n)
        sv.check(got, ref, scale, ("spmv_t", alpha, beta))
        assert 0.005 <= float((~np.isfinite(ref)).mean()) <= 0.25 and np.isnan(ref).sum() >= 3 and np.isinf(ref).sum() >= 3
        with np.errstate(all="ignore"):
            untouched = np.zeros(c.dead.size) if beta == 0 else beta * ys[c.dead]
        assert np.array_equal(got[c.dead], untouched, equal_nan=True), (alpha, beta, "a column no row references")
    # alpha == 0: this entry skips the product pass, so y = beta * y whatever x holds
    dy = dev(torch, y0)
    spmv_acc_amd.csr_spmv_t(0.0, 0.5, c.m, c.n, c.nnz, drp, dci, dv, dx, dy)
    torch.cuda.synchronize()
    with np.errstate(all="ignore"):
        assert np.array_equal(dy.cpu().numpy(), 0.5 * y0, equal_nan=True)


# ---- f. the transpose moves bits ---------------------------------------------------------------------------------------------------------
def test_transpose_moves_special_values_bit_for_bit(torch_dev, refs_m):
    """NaNs with distinct payloads (quiet and signalling), both Infs, -0.0 and subnormals arrive as they left: int64 views against the host
    stable argsort, for the transpose and for its value refresh."""
    torch = torch_dev
    c = refs_m.case
    rng = np.random.default_rng(8)
    bits = rng.standard_normal(c.nnz).view(np.int64).copy()
    where = rng.choice(c.nnz, 600, replace=False)
    special = np.concatenate([0x7FF8000000000000 + np.arange(1, 201), 0x7FF0000000000000 + np.arange(1, 101), -0x0008000000000000 + np.arange(100),
                              np.full(50, 0x7FF0000000000000), np.full(50, -0x0010000000000000), np.full(50, -0x8000000000000000), np.arange(1, 51)])
    bits[where] = special.astype(np.int64)
    vals = bits.view(np.float64)
    assert np.isnan(vals).sum() == 400 and np.isinf(vals).sum() == 100
    drp, dci, dv = dev(torch, c.rowptr), dev(torch, c.cols), dev(torch, vals)
    perm = np.argsort(c.cols, kind="stable")
    t_rp, t_ci, t_v, d_perm = spmv_acc_amd.csr_transpose(c.m, c.n, c.nnz, drp, dci, dv, want_perm=True)
    assert np.array_equal(d_perm.cpu().numpy(), perm)
    assert np.array_equal(t_v.cpu().numpy().view(np.int64), bits[perm])
    bits2 = np.roll(bits, 17)
    dv2 = dev(torch, bits2.view(np.float64))
    out = torch.zeros_like(t_v)
    spmv_acc_amd.csr_transpose_values(d_perm, dv2, out)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.int64), bits2[perm])


# ---- g. COO assembly ----------------------------------------------------------------------------------------------------------------------
RUN_LENGTHS = (1, 2, 64, 65, 300)  # up to 64 triples one lane adds, more a wavefront
RUN_KINDS = ("clean", "nan first", "nan middle", "nan last", "both infs", "plus inf", "clean")


def coo_runs(seed=12, subnormal=False):
    """Triples of duplicate runs of every length and kind, shuffled; returns (row, col, val, run of each triple, kind of each run, n)."""
    rng = np.random.default_rng(seed)
    n = 16
    row, col, val, run, kinds = [], [], [], [], []
    for length in RUN_LENGTHS:
        for kind in RUN_KINDS:
            if length == 1 and kind == "both infs":
                continue
            r = len(kinds)
            v = sv.tiny(rng.integers(1, 9, length)) if subnormal else rng.uniform(-1.0, 1.0, length)
            if not subnormal:
                if kind.startswith("nan"):
                    v[{"nan first": 0, "nan middle": length // 2, "nan last": length - 1}[kind]] = np.nan
                elif kind == "both infs":
                    v[length // 3], v[length - 1] = np.inf, -np.inf
                elif kind == "plus inf":
                    v[rng.integers(0, length, min(length, 3))] = np.inf
            row += [r // n] * length
            col += [r % n] * length
            val += list(v)
            run += [r] * length
            kinds.append(kind)
    order = rng.permutation(len(row))
    f = lambda a, t: np.asarray(a, dtype=t)[order]
    return f(row, np.int32), f(col, np.int32), f(val, np.float64), f(run, np.int64), kinds, n


def test_coo_assembly_keeps_poison_in_its_run(torch_dev):
    """Duplicate runs summed by one lane (1, 2, 64 triples) and by a wavefront (65, 300) with `ok ? v : 0.0` masks: a NaN in the first, a middle
    or the last triple of a run, +Inf with -Inf, only +Inf.  Each entry's class follows its own run; clean entries are bitwise what the same
    triples give with the poisoned runs removed (the summation order is documented and data-independent); the values-only refresh repeats
    the first assembly's bits."""
    torch = torch_dev
    row, col, val, run, kinds, n = coo_runs()
    m = (len(kinds) + n - 1) // n
    rp, ci, v, order, start = spmv_acc_amd.coo_to_csr(m, n, dev(torch, row), dev(torch, col), dev(torch, val), want_map=True)
    got = v.cpu().numpy()
    assert got.size == len(kinds) and np.array_equal(ci.cpu().numpy(), np.arange(len(kinds)) % n)  # (run r is entry r: one (row, col) each, in key order)
    assert np.array_equal(rp.cpu().numpy(), np.minimum(np.arange(m + 1) * n, len(kinds)))
    ref, scale = sv.classify_products(1.0, 0.0, run, val, len(kinds), None)
    sv.check(got, ref, scale, "coo")
    clean = np.array([k == "clean" for k in kinds])
    assert np.array_equal(np.isfinite(ref), clean) and set(np.unique(ref[~clean][~np.isnan(ref[~clean])])) == {np.inf}
    keep = clean[run]
    rp2, ci2, v2 = spmv_acc_amd.coo_to_csr(m, n, dev(torch, row[keep]), dev(torch, col[keep]), dev(torch, val[keep]))
    assert np.array_equal(v2.cpu().numpy().view(np.int64), got[clean].view(np.int64)), "a clean run's bits depend on its neighbours"
    out = torch.full_like(v, SENTINEL)
    spmv_acc_amd.coo_to_csr_values(order, start, dev(torch, val), out)
    torch.cuda.synchronize()
    again = out.cpu().numpy()
    assert np.array_equal(np.isnan(again), np.isnan(got)) and np.array_equal(again[~np.isnan(got)].view(np.int64), got[~np.isnan(got)].view(np.int64))


# ---- h. subnormals are never flushed ------------------------------------------------------------------------------------------------------
SUBNORMAL_ABS = ((1, 0), (2, 1))


@pytest.fixture(scope="module")
def tiny_m(refs_m):
    c = refs_m.case
    iv, kx, ky = sv.subnormal_inputs(c)
    rows = sv.entry_rows(c.rowptr)
    want = {ab: sv.tiny(sv.subnormal_reference(ab[0], ab[1], rows, iv * kx[c.cols], c.m, ky)) for ab in SUBNORMAL_ABS}
    assert all(0 < w.max() < 2.0 ** -1022 for w in want.values())
    return iv.astype(np.float64), sv.tiny(kx), sv.tiny(ky), want


def exact(got, want, tag):
    bad = np.nonzero(got != want)[0]  # (equal values of subnormals are equal bits; either zero)
    assert bad.size == 0, (tag, "rows", bad[:8].tolist(), "got / 2^-1074", (got[bad[:8]] / sv.TINY).tolist(), "want", (want[bad[:8]] / sv.TINY).tolist())


@pytest.mark.parametrize("strat", spmv_acc_amd.STRATEGIES)
def test_subnormals_every_strategy(torch_dev, refs_m, tiny_m, strat):
    torch = torch_dev
    c = refs_m.case
    vals, x, y0, want = tiny_m
    drp, dci, dv, dx = (dev(torch, a) for a in (c.rowptr, c.cols, vals, x))
    try:
        for alpha, beta in SUBNORMAL_ABS:
            exact(spmv(torch, strat, float(alpha), float(beta), c, drp, dci, dv, dx, y0), want[(alpha, beta)], (strat, alpha, beta))
    finally:
        spmv_acc_amd.release_plans(drp)


def test_subnormals_arithmetic_forms(torch_dev, hiplib, refs_m, tiny_m):
    """The forms that move the additions: flat's segmented scan, column slabs and their merge y[r] += ys[i], slab segments."""
    torch = torch_dev
    c = refs_m.case
    vals, x, y0, want = tiny_m
    drp, dci, dv, dx = (dev(torch, a) for a in (c.rowptr, c.cols, vals, x))
    try:
        for strat, knobs in sv.ARITHMETIC_FORMS:
            set_tunables(hiplib, knobs)
            spmv_acc_amd.release_plans(drp)
            for alpha, beta in SUBNORMAL_ABS:
                exact(spmv(torch, strat, float(alpha), float(beta), c, drp, dci, dv, dx, y0), want[(alpha, beta)], (strat, knobs, alpha, beta))
    finally:
        hiplib.spmv_acc_reset_tunables()
        spmv_acc_amd.release_plans()


@pytest.mark.parametrize("layout", ["row", "col"])
def test_subnormals_spmm(torch_dev, refs_m, tiny_m, layout):
    torch = torch_dev
    c = refs_m.case
    vals, x, y0, want = tiny_m
    drp, dci, dv = dev(torch, c.rowptr), dev(torch, c.cols), dev(torch, vals)
    try:
        for k in (3, 8):
            X, Y0 = np.stack([x] * k, axis=1), np.stack([y0] * k, axis=1)
            for alpha, beta in SUBNORMAL_ABS:
                dX, dY, _ = xy_views(torch, X, Y0, layout)
                spmv_acc_amd.csr_spmm(float(alpha), float(beta), c.m, c.n, c.nnz, drp, dci, dv, dX, dY)
                torch.cuda.synchronize()
                got = dY.cpu().numpy()
                for j in range(k):
                    exact(got[:, j], want[(alpha, beta)], (layout, k, j, alpha, beta))
    finally:
        spmv_acc_amd.release_plans()


def test_subnormals_coo_duplicate_sums(torch_dev):
    torch = torch_dev
    row, col, val, run, kinds, n = coo_runs(seed=13, subnormal=True)
    m = (len(kinds) + n - 1) // n
    _, _, v = spmv_acc_amd.coo_to_csr(m, n, dev(torch, row), dev(torch, col), dev(torch, val))
    want = sv.tiny(np.bincount(run, val / sv.TINY, len(kinds)).astype(np.int64))
    exact(v.cpu().numpy(), want, "coo")


def test_subnormals_spmv_t(torch_dev, refs_m):
    """The stateless transposed product adds with the hardware's fp64 atomic: integer multiples of 2^-1074 must come back exact."""
    torch = torch_dev
    c = refs_m.case
    iv, kx, ky = sv.subnormal_inputs_t(c)
    rows = sv.entry_rows(c.rowptr)
    drp, dci, dv, dx = (dev(torch, a) for a in (c.rowptr, c.cols, iv.astype(np.float64), sv.tiny(kx)))
    for alpha, beta in SUBNORMAL_ABS:
        want = sv.tiny(sv.subnormal_reference(alpha, beta, c.cols, iv * kx[rows], c.n, ky))
        assert 0 < want.max() < 2.0 ** -1022
        dy = dev(torch, sv.tiny(ky))
        spmv_acc_amd.csr_spmv_t(float(alpha), float(beta), c.m, c.n, c.nnz, drp, dci, dv, dx, dy)
        torch.cuda.synchronize()
        exact(dy.cpu().numpy(), want, ("spmv_t", alpha, beta))
