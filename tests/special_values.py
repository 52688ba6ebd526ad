"""Shared helpers of tests/test_special_values_host.py (CPU) and tests/test_gpu_special_values.py (GPU): a reference for
y = alpha*A*x + beta*y on inputs that hold NaN, +-Inf, overflowing products and subnormals, and the small matrices that carry them through
every staging form of the kernels.

The reference is order-independent by construction.  One fp64 multiply does not depend on any summation order, so a row is CLASSIFIED from
its products p_j = value[j] * x[col[j]] (a product that overflows counts as its Inf):
    any NaN product                -> NaN          only +Inf products -> +Inf
    +Inf and -Inf products         -> NaN          only -Inf products -> -Inf
    otherwise finite: the exact sum (math.fsum) of the products.
alpha and beta are then applied to that sum by IEEE rules: a negative alpha flips an Inf, beta == 0 never reads y, beta != 0 with a non-finite
y0[i] makes row i non-finite.  Finite products stay below 1e3 in rows of more than one entry, so no finite partial sum can overflow in any
order; product overflow (2^600 * 2^500) sits in single-entry rows only.

Non-finite rows must match in class exactly (NaN against NaN, the sign of an Inf); finite rows are held to the project's bound, scaled error
|d - h| / (|alpha| sum |p_j| + |beta y0_i|) <= 1e-12 over the row's own finite products.  The SIGN OF A ZERO RESULT IS NOT ASSERTED: -0.0 and
+0.0 compare equal here, as nothing in the library's contract fixes it.

PLAIN MODULE, not a conftest: imported by name."""
import math

import numpy as np

from spmv_acc_amd import synth

SCALED_TOL = 1e-12
TINY = 2.0 ** -1074  # the smallest subnormal
BIG_VALUE, BIG_X = 2.0 ** 600, 2.0 ** 500  # their product overflows; each alone is finite
POISON = (np.inf, -np.inf, np.nan)

# ---------------------------------------------------------------------------------------------------------------------------------------
# the engine's A/B switches (strategy, tunables): the inventory tests/test_gpu_parity.py::test_measurement_switches_keep_parity runs on finite
# data and tests/test_gpu_special_values.py on poisoned data
# ---------------------------------------------------------------------------------------------------------------------------------------
MEASUREMENT_SWITCHES = [
    ("flat", {"flat_npt": 4}), ("flat", {"flat_npt": 16}), ("flat", {"xcd_chunk": 0}), ("flat", {"xcd_chunk": 5}),
    ("line_enhance", {"xcd_chunk": 0}),
    ("line_enhance", {"xcd_chunk": 64}), ("line_enhance", {"rowblock_guard": 0}),
    ("line_enhance", {"rowblock_vec": 8}), ("line_enhance", {"rowblock_target": 600}),
    ("adaptive_plus", {"plus_host_analysis": 1}), ("adaptive_plus", {"xcd_chunk": 0}), ("adaptive_plus", {"xcd_chunk": 3}),
    # round 2: row digest on / off, vector-row forms, flat's stream-first staging and tile sizes, 16-bit columns
    ("line_enhance", {"rowlen": 1, "rowblock_guard": 0}), ("line_enhance", {"rowlen": 0, "rowblock_guard": 0}),
    ("line_enhance", {"rowlen": 1, "rowblock_vec": 4, "rowblock_guard": 0}), ("line_enhance", {"rowlen": 1, "rowblock_vec": 64, "rowblock_guard": 0}),
    ("line", {"rowlen": 1, "rowblock_target": 700, "rowblock_guard": 0}),
    ("vector_row", {"vector_tile": 0}), ("vector_row", {"vector_tile": 1, "rowblock_guard": 0}), ("light", {"vector_tile": 1, "rowblock_guard": 0}),
    ("adaptive", {"adaptive_timed": 0, "adaptive_split": 1, "vector_tile": 1}), ("adaptive", {"adaptive_timed": 0, "adaptive_split": 1, "vector_tile": 0}),
    ("flat", {"flat_early": 1, "flat_npt": 8}), ("flat", {"flat_early": 1, "flat_npt": 4}), ("flat", {"flat_early": 0, "flat_npt": 4}),
    ("flat", {"flat_early": 1, "flat_npt": 16, "flat_finish": 0}), ("flat", {"col16": 1}), ("flat", {"col16": 1, "flat_finish": 0}),
    # walking direction and cacheable grid ends (speed only)
    ("flat", {"zigzag": 0}), ("line_enhance", {"zigzag": 0}), ("adaptive_plus", {"zigzag": 0}), ("vector_row", {"zigzag": 0}),
    ("line_enhance", {"cache_ends_mb": 0, "stream_plain": 0}), ("line_enhance", {"cache_ends_mb": 1, "stream_plain": 0}),
    ("flat", {"cache_ends_mb": 1, "stream_plain": 0}), ("flat", {"cache_ends_mb": 4000, "stream_plain": 0}),
    # the segmented-scan reduction of a flat tile (the reference's FLAT_SEGMENT_SUM_REDUCE)
    ("flat", {"flat_reduce": 1}), ("flat", {"flat_reduce": 1, "flat_finish": 0}), ("flat", {"flat_reduce": 1, "flat_finish": 1, "stream_plain": 1}),
    ("flat", {"flat_reduce": 1, "flat_npt": 4}),
    # gather hints (cold gathers non-temporal): forced on, tiny and huge hot sets
    ("adaptive_plus", {"gather_hint": 1}), ("adaptive_plus", {"gather_hint": 1, "hint_budget_kb": 1}),
    ("adaptive_plus", {"gather_hint": 1, "hint_budget_kb": 100000}), ("flat", {"gather_hint": 1, "flat_npt": 8, "flat_early": 0}),
    ("flat", {"gather_hint": 1, "hint_budget_kb": 8, "flat_npt": 8, "flat_early": 0, "flat_finish": 0}),
    ("adaptive", {"gather_hint": 1, "hint_budget_kb": 16}), ("line_enhance", {"gather_hint": 1, "hint_budget_kb": 16}),
    ("line_enhance", {"gather_hint": 1, "rowblock_guard": 0, "rowlen": 1}), ("default", {"gather_hint": 1, "hint_budget_kb": 1})]

# forms the list above does not pin: column slabs (a re-ordered copy, merged by y[r] += ys[i]), slab segments (run lists; the rows' columns
# ascend), the deterministic switch.  ARITHMETIC_FORMS are those that change the order or the place of the additions.
SLAB_FORMS = [("adaptive", {"col_slabs": 3}), ("line_enhance", {"col_slabs": 8}), ("flat", {"col_slabs": 3}),
              ("line_enhance", {"slab_segments": 4}), ("flat", {"slab_segments": 4}), ("line_enhance", {"slab_segments": 4, "gather_hint": 1}),
              ("line_enhance", {"deterministic": 1}), ("flat", {"deterministic": 1}), ("adaptive", {"deterministic": 1})]
ARITHMETIC_FORMS = [(s, k) for s, k in MEASUREMENT_SWITCHES if "flat_reduce" in k] + [(s, k) for s, k in SLAB_FORMS if "deterministic" not in k]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------------------------
def entry_rows(rowptr):
    return np.repeat(np.arange(rowptr.size - 1, dtype=np.int64), np.diff(rowptr))


def products(vals, x, cols):
    with np.errstate(all="ignore"):
        return np.asarray(vals, dtype=np.float64) * np.asarray(x, dtype=np.float64)[cols]


def classify_products(alpha, beta, owner, p, m, y0):
    """(ref, scale) of the m sums: entry j adds p[j] to sum owner[j].  ref[i] = alpha * S_i + beta * y0[i] with S_i the class of sum i (see the
    module docstring); scale[i] = |alpha| sum |finite p| + |beta y0[i]|."""
    owner, p = np.asarray(owner, dtype=np.int64), np.asarray(p, dtype=np.float64)
    order = np.argsort(owner, kind="stable")
    owner, p = owner[order], p[order]
    nan = np.bincount(owner, np.isnan(p), m) > 0
    pos = np.bincount(owner, p == np.inf, m) > 0
    neg = np.bincount(owner, p == -np.inf, m) > 0
    fin = np.isfinite(p)
    absum = np.bincount(owner, np.where(fin, np.abs(p), 0.0), m)
    start = np.searchsorted(owner, np.arange(m + 1))
    s = np.zeros(m)
    for i in np.nonzero(~(nan | pos | neg) & (start[1:] > start[:-1]))[0]:
        s[i] = math.fsum(p[start[i]:start[i + 1]])
    s[pos] = np.inf
    s[neg] = -np.inf
    s[nan | (pos & neg)] = np.nan
    with np.errstate(all="ignore"):
        ref = alpha * s if beta == 0 else alpha * s + beta * np.asarray(y0, dtype=np.float64)
        scale = abs(alpha) * absum + (0.0 if beta == 0 else np.abs(beta * np.asarray(y0, dtype=np.float64)))
    return ref, scale


def classify(alpha, beta, rowptr, cols, vals, x, y0):
    """(ref, scale) of y = alpha*A*x + beta*y0, row by row."""
    return classify_products(alpha, beta, entry_rows(rowptr), products(vals, x, cols), rowptr.size - 1, y0)


def classify_t(alpha, beta, rowptr, cols, vals, x, y0, n):
    """(ref, scale) of y = alpha*A^T*x + beta*y0 as spmv_acc_csr_spmv_t evaluates it: it adds the terms (alpha * a) * x[row] to beta * y0[col], so
    the terms are the products and the roles of rows and columns are swapped.  Columns outside [0, n) are dropped."""
    rows = entry_rows(rowptr)
    keep = (cols >= 0) & (cols < n)
    with np.errstate(all="ignore"):
        p = (alpha * np.asarray(vals, dtype=np.float64)) * np.asarray(x, dtype=np.float64)[rows]
    return classify_products(1.0, beta, cols[keep], p[keep], n, y0)


def mismatches(got, ref, scale, tol=SCALED_TOL):
    """Indices where `got` misses `ref`: the class of a non-finite entry, the scaled bound of a finite one (scale 0: equal, either zero)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    nf = ~np.isfinite(ref)
    with np.errstate(all="ignore"):
        bad = np.where(nf, ~((np.isnan(ref) & np.isnan(got)) | (got == ref)), ~np.isfinite(got) | ~(np.abs(got - ref) <= tol * scale))
    return np.nonzero(bad)[0]


def check(got, ref, scale, tag, tol=SCALED_TOL):
    bad = mismatches(got, ref, scale, tol)
    assert bad.size == 0, (tag, "rows", bad[:8].tolist(), "got", np.asarray(got)[bad[:8]].tolist(), "want", ref[bad[:8]].tolist())


def caps(rowptr, p, ref):
    """The conditions of the inputs, from the reference's classification alone: the share of non-finite rows, how often each class occurs,
    whether a clean row lies between two poisoned ones, and whether a clean row shares a 16-byte 4-group / a 2048-product tile of the
    non-zero stream with a poisoned entry of another row."""
    m = rowptr.size - 1
    dirty = ~np.isfinite(ref)
    rows = entry_rows(rowptr)
    badj = np.nonzero(~np.isfinite(p))[0]
    j = np.arange(p.size)
    clean_entry = ~dirty[rows]
    return {"share": float(dirty.mean()), "nan": int(np.isnan(ref).sum()), "pos": int((ref == np.inf).sum()), "neg": int((ref == -np.inf).sum()),
            "between": bool(np.any(~dirty[1:m - 1] & dirty[:m - 2] & dirty[2:])),
            "group": bool(np.any(clean_entry & np.isin(j // 4, badj // 4))), "tile": bool(np.any(clean_entry & np.isin(j // 2048, badj // 2048)))}


def assert_caps(c, tag):
    assert 0.005 <= c["share"] <= 0.05, (tag, c)
    assert min(c["nan"], c["pos"], c["neg"]) >= 3, (tag, c)
    assert c["between"] and c["group"] and c["tile"], (tag, c)


# ---------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------------
def sort_rows(rowptr, cols, vals):
    order = np.lexsort((cols, entry_rows(rowptr)))
    return cols[order].copy(), vals[order].copy()


def reserve_columns(cols, which, n):
    """No entry references the columns `which` afterwards: their entries move to the next column that is not reserved."""
    which = set(int(c) for c in which)
    for c in sorted(which):
        t = c + 1
        while t in which:
            t += 1
        if t >= n:
            t = c - 1
            while t in which:
                t -= 1
        cols[cols == c] = t
    assert not np.isin(cols, sorted(which)).any()


class Case:
    """One matrix with the places its poison goes: `dead` columns no entry references, `big` a column only single-entry rows reference,
    `entries` the non-zeros whose value (or whose column of x) is poisoned, in the order (+Inf, -Inf, NaN, ...)."""

    def __init__(self, rowptr, cols, vals, n, dead, big, singles, entries, zero_entry):
        self.rowptr, self.cols, self.vals, self.n = rowptr, cols, vals, n
        self.m, self.nnz = rowptr.size - 1, int(rowptr[-1])
        self.dead, self.big, self.singles, self.entries, self.zero_entry = dead, big, singles, entries, zero_entry

    def inputs(self, variant, seed=5):
        """(vals, x, y0) of variant 'x' (poison in x), 'vals' (poison in the values, x finite) or 'both'.  y0 holds three non-finite entries
        (they count only where beta != 0).  In every variant the single-entry rows overflow: +-2^600 * 2^500."""
        rng = np.random.default_rng(seed)
        x, y0 = rng.uniform(0.5, 2.0, self.n) * rng.choice([-1.0, 1.0], self.n), rng.standard_normal(self.m)
        vals = self.vals.copy()
        for k, r in enumerate(self.singles):
            vals[self.rowptr[r]] = BIG_VALUE if k % 2 == 0 else -BIG_VALUE
        x[self.big] = BIG_X
        for k, i in enumerate((self.m // 3, self.m // 3 + 1, self.m - 2)):
            y0[i] = POISON[k]
        if variant in ("x", "both"):
            x[self.dead] = np.nan
            for k, j in enumerate(self.entries if variant == "x" else self.entries[::2]):
                x[self.cols[j]] = POISON[k % 3]
            vals[self.zero_entry] = 0.0  # a stored zero against an Inf of x: a NaN product
            x[self.cols[self.zero_entry]] = np.inf
        if variant in ("vals", "both"):
            for k, j in enumerate(self.entries if variant == "vals" else self.entries[1::2]):
                vals[j] = POISON[(k + 1) % 3]
        return vals, x, y0


def _finish(rowptr, cols, vals, n, dead, big, singles, between, rng, long_rows, clean_long):
    """Reserve the special columns, point the single-entry rows at `big` and the two neighbours of row `between` at one column of their own,
    sort the rows, then choose the poisoned entries."""
    m = rowptr.size - 1
    sand = between + n // 3 if between + n // 3 < n - 2 else n // 2
    reserve_columns(cols, list(dead) + [big, sand], n)
    for r in singles:
        assert rowptr[r + 1] - rowptr[r] == 1
        cols[rowptr[r]] = big
    for r in (between - 1, between + 1):
        assert rowptr[r + 1] > rowptr[r]
        cols[rowptr[r]] = sand
    cols, vals = sort_rows(rowptr, cols, vals)
    lens = np.diff(rowptr)
    entries = []
    for r in (between - 1, between + 1):  # the sandwich: both through the same column
        entries.append(int(rowptr[r] + np.nonzero(cols[rowptr[r]:rowptr[r + 1]] == sand)[0][0]))
    for r in long_rows:
        if lens[r] >= 2000:
            entries.append(int(rowptr[r] + lens[r] // 2))           # the middle of a row longer than a tile
        elif lens[r] > 8:
            entries += [int(rowptr[r]), int(rowptr[r + 1] - 1)]     # the first and the last 4-group of a row
    entries.append(int(rowptr[-1] - 1))                              # the last non-zero of the arrays
    short = np.nonzero((lens >= 1) & (lens <= 64))[0]  # (not the long rows: those are poisoned by place)
    taken = {big, sand} | set(int(c) for c in dead)
    for r in rng.choice(short, size=4 * m // 1000 + 6, replace=False):
        j = int(rowptr[r] + rng.integers(0, lens[r]))
        if int(cols[j]) not in taken and r not in singles:
            entries.append(j)
    entries = [j for j in entries if int(cols[j]) != big and j not in [int(rowptr[r]) for r in singles]]
    r = next(int(r) for r in short[short.size // 2:] if lens[r] >= 2 and abs(r - between) > 1 and int(cols[rowptr[r]]) not in taken)
    zero_entry = int(rowptr[r])
    assert int(cols[zero_entry]) not in taken
    # the long rows that stay CLEAN (a leak into the tail of a long row's last piece or span shows only there): their entries step off every
    # column that will hold poison
    hot = {int(cols[j]) for j in entries} | {int(cols[zero_entry])} | taken
    for r in clean_long:
        a, b = int(rowptr[r]), int(rowptr[r + 1])
        cc = cols[a:b].copy()
        for i in range(cc.size):
            step = 1 if int(cc[i]) < n // 2 else -1
            while int(cc[i]) in hot:
                cc[i] += step
        order = np.argsort(cc, kind="stable")
        cols[a:b], vals[a:b] = cc[order], vals[a:b][order]
    return Case(rowptr, cols, vals, n, np.array(sorted(dead)), big, list(singles), entries, zero_entry)


def matrix_m(seed=20261):
    """Matrix M (mixed): 12 000 rows of 0 .. 8 non-zeros, rows of 700, 3000, 1 and 9000 next to short ones (the 9000-row makes flat carry across
    more than two tiles), rows of 2500 and 301 that stay clean, empty rows -- the first and the last among them --, single-entry rows for the overflowing products, nnz % 4 != 0,
    columns ascending inside every row (slab segments need that)."""
    rng = np.random.default_rng(seed)
    m = n = 12000
    lens = rng.integers(0, 9, m)
    lens[[100, 5000, 5001, 8000]] = [700, 3000, 1, 9000]
    lens[[10000, 10400]] = [2500, 301]  # long rows that stay clean: pieces and spans with dead lanes at their ends
    lens[[0, m - 1, 2500, 2501, 7999]] = 0
    singles = [5001, 7001, 7003, 7005, 7007, 7009]
    lens[singles] = 1
    lens[[2999, 3000, 3001]] = [3, 2, 3]
    if int(lens.sum()) % 4 == 0:
        lens[6000] += 1
    rowptr, cols, vals = synth.csr_from_row_lengths(lens, n, rng)
    assert int(rowptr[-1]) % 4 != 0
    return _finish(rowptr, cols, vals, n, (0, n - 1, 3001, 9001), 6500, singles, 3000, rng, (100, 5000, 8000), (10000, 10400))


def chunk_base(cols, chunk, half):
    """The base column of 256-non-zero chunk `chunk` as k_col16.hip computes it: the median over the 64 lanes of each lane's second-smallest
    column (its smallest where it holds one), minus `half` (32767 for 16-bit codes, 127 for 8-bit ones), clamped at 0.  A HOST COPY of the
    kernel's rule for a whole matrix (first chunk 0); nothing on the GPU side confirms that the column it names is the one the lanes gather.
    Should the kernel's rule change, the NaN put there lands in an ordinary unreferenced column and the test still passes -- keep the two
    in step (column 0, the clamped base of every early chunk, does not depend on this copy)."""
    c = np.full(256, np.iinfo(np.int32).max, dtype=np.int64)
    part = cols[256 * chunk:256 * (chunk + 1)]
    c[:part.size] = part
    lanes = np.sort(c.reshape(64, 4), axis=1)
    rep = np.where(lanes[:, 1] != np.iinfo(np.int32).max, lanes[:, 1], lanes[:, 0])
    valid = int((rep != np.iinfo(np.int32).max).sum())
    return max(int(np.sort(rep)[(valid - 1) // 2]) - half, 0) if valid else 0


def headline_like(m, n, rng, far=0.10):
    """The 8-bit cases' shape (tests/test_gpu_col8.py): 3..7 non-zeros per row, near columns drifting 0.92 per row within +-7, `far` random."""
    lens = rng.integers(3, 8, size=m)
    rowptr = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(lens, out=rowptr[1:])
    rows = np.repeat(np.arange(m, dtype=np.int64), lens)
    near = (rows * 92) // 100 + rng.integers(-7, 8, size=rows.size)
    cols = np.where(rng.random(rows.size) < far, rng.integers(0, n, size=rows.size), np.clip(near, 0, n - 1)).astype(np.int32)
    return rowptr.astype(np.int32), cols, rng.uniform(-1.0, 1.0, size=rows.size)


L_KINDS = ("short rows, 10 % far", "fem-like, 2 % far", "headline-shaped")


def matrix_l(kind, seed=20262):
    """Matrix L (local columns): the recipes of tests/test_gpu_col16.py::_cases and the 8-bit shape of tests/test_gpu_col8.py cut to about 70 chunks
    of 256 non-zeros (the encoding needs 64).  Returns (case, half, base chunk): besides the places of _finish the poison goes into the base
    column of a middle chunk -- the column the chunk's non-owning lanes gather, reserved so that no row references it -- and into the column
    of an escaped far entry."""
    rng = np.random.default_rng(seed)
    if kind == "short rows, 10 % far":
        lens, n, half = rng.integers(3, 8, size=3600), 500000, 32767
        lens[[1500, 1502, 1504]] = 1
        rowptr, cols, vals = synth.csr_from_row_lengths(lens, n, rng, locality=64, far_fraction=0.10)
    elif kind == "fem-like, 2 % far":
        lens, n, half = rng.integers(20, 40, size=600), 400000, 32767
        lens[[300, 302, 304]] = 1
        rowptr, cols, vals = synth.csr_from_row_lengths(lens, n, rng, locality=300, far_fraction=0.02)
    else:
        n, half = 2_000_000, 127
        rowptr, cols, vals = headline_like(3600, n, rng)
    m, nnz = rowptr.size - 1, int(rowptr[-1])
    assert nnz >= 66 * 256
    lens = np.diff(rowptr)
    singles = [int(r) for r in np.nonzero(lens == 1)[0][:3]]
    chunk = nnz // 256 // 2
    rows = entry_rows(rowptr)
    mid = int(np.median(cols[256 * chunk:256 * (chunk + 1)]))
    near = rows * n // m if half == 32767 else rows * 92 // 100
    far = [int(j) for j in np.nonzero(np.abs(cols.astype(np.int64) - near) > 2 * half + 1000)[0][:2]]  # (outside either window: escapes)
    assert far, "no escaped entry"
    far_cols = cols[far].copy()
    between = m // 2 + 7
    case = _finish(rowptr, cols, vals, n, (0, n - 1, mid + 3), int(cols[rowptr[m // 4]]) + 1, singles, between, rng, (), ())
    # the base of the finished structure (sorting the rows regroups the lanes' four columns), then reserved: its entries move one column up,
    # far below the median, so the base stands
    base = chunk_base(case.cols, chunk, half)
    assert 0 < base < n - 1 and base not in case.dead and base + 1 not in case.dead and base != case.big
    reserve_columns(case.cols, [base], n)
    assert chunk_base(case.cols, chunk, half) == base, "the reserved base column moved the chunk's median"
    case.dead = np.array(sorted(list(case.dead) + [base]))
    case.entries += [int(np.nonzero(case.cols == c)[0][0]) for c in far_cols]
    case.half, case.base_chunk, case.base = half, chunk, base
    return case


def subnormal_inputs(case, seed=9):
    """(ivals, kx, ky): integer values 1 .. 8 and the integer multiples of 2^-1074 that x and y0 hold (1 .. 7 and 0 .. 7): every product, partial
    sum and result -- alpha in {1, 2}, beta in {0, 1} -- is an integer multiple of 2^-1074 below 2^-1022, exact in any order and under any fused
    multiply-add."""
    rng = np.random.default_rng(seed)
    return rng.integers(1, 9, case.nnz), rng.integers(1, 8, case.n), rng.integers(0, 8, case.m)


def subnormal_inputs_t(case, seed=10):
    """(ivals, kx, ky) of the transposed product: kx over the ROWS (1 .. 7), ky over the columns (0 .. 7), the same integer values."""
    rng = np.random.default_rng(seed)
    return subnormal_inputs(case)[0], rng.integers(1, 8, case.m), rng.integers(0, 8, case.n)


def chunk_escapes(cols, half):
    """Escapes per 256-non-zero chunk under the code width of `half`: entries outside [base, base + 2 * half]."""
    out = []
    for c in range((cols.size + 255) // 256):
        d = cols[256 * c:256 * (c + 1)].astype(np.int64) - chunk_base(cols, c, half)
        out.append(int(((d < 0) | (d > 2 * half)).sum()))
    return np.array(out)


def subnormal_reference(alpha, beta, owner, iterms, m, ky):
    """The integer-arithmetic result, as integers (multiples of 2^-1074)."""
    s = np.bincount(owner, iterms.astype(np.float64), m).astype(np.int64)  # (sums far below 2^53: exact)
    return int(alpha) * s + int(beta) * ky.astype(np.int64)


def tiny(k):
    return np.ldexp(np.asarray(k, dtype=np.float64), -1074)
