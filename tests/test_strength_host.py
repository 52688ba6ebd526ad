"""CPU side of the strength-of-connection filter and the prolongator smoother (no GPU): the C ABI declares and exports the two entries, they
and the Python wrappers refuse bad arguments before any launch, the compiled kernels use no scratch and no AGPR and fit 64 VGPRs, every
size-selected branch of the new code names the GPU tests that cross it, the engine file stays stateless, and the definitions are restated here
in numpy and exported to the GPU suite as its references: the kept pattern and the partition (host_csr_strength) and the lumped diagonal, the
filtered matrix and the smoother in their documented order (host_strength_values, bit for bit), checked against independent statements: the
symmetry of the kept pattern, the partition's invariants, the two ends of theta, the tie, the mirror, row sums, and M 1 = 1 - omega A_F 1 / f."""
import ctypes
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import spmv_acc_amd
from test_agg_host import cases as agg_cases
from test_agg_host import TAGS as AGG_TAGS
from test_agg_host import grid5_matrix, grid5_pairs, host_csr_aggregate
from test_coo_host import LONG_RUN, SHARED, _FakeTensor, _f, _i, coo_sum_model
from test_gs_host import HELPERS, csr_from_pattern, row_sum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "spmv_acc_amd/csrc/"
NEW_SOURCES = ("strength.hpp", "k_strength.hip", "strength.cpp")
MODEL = "test_strength_is_the_host_model"
VALUES = "test_strength_values_are_the_host_model"
CAPTURE = "test_strength_values_captured_and_replayed"
CONTRACT = "test_strength_contract"
VALUES_CONTRACT = "test_strength_values_contract"
STRIDE = "test_strength_grid_stride_at_test_size"
RANK_TILE, LUMP_PER_LANE, PER_LANE = 256, 1, 4  # kStrengthRankTile, kStrengthLumpPerLane, kStrengthPerLane (STRENGTH_SIZE_RULES holds them to the source)
WAVE_CHUNK = 64 * PER_LANE  # kStrengthWaveChunk: the S entries whose rows one wavefront searches between its two end rows

# (rule, file, regex that must match the source, GPU tests of tests/test_gpu_strength.py that cross it at test size, what it selects)
STRENGTH_SIZE_RULES = [
    ("kStrengthRankTile", CSRC + "strength.hpp", r"constexpr int kStrengthRankTile = 256;",
     [MODEL, STRIDE], "flags and scatter: 256 positions of A per workgroup, one per lane; cases of fewer (one, the special values) leave lanes empty, "
                      "aniso24 (2 784) is 11 tiles with a short last one, the stride case more tiles than 64 workgroups"),
    ("the scan's closing element", CSRC + "k_strength.hip", r"if \(p == nnz\) \{",
     [MODEL], "flag[nnz] = 0: in a wavefront of its own where nnz is a multiple of 64 (one_empty: nnz = 0), else behind the last entries"),
    ("a stored diagonal is always kept", CSRC + "k_strength.hip", r"if \(j != i\) \{",
     [MODEL], "every case with a stored diagonal; the special values hold NaN, inf, 0.0 and -0.0 diagonals"),
    ("the mirror", CSRC + "k_strength.hip", r"if \(q < chi && colindex\[q\] == i\) strong = strong \|\| fabs\(value\[q\]\) >= rhs;",
     [MODEL], "the unsymmetric cases keep entries only their mirror makes strong"),
    ("tile loops of the entry passes", CSRC + "k_strength.hip", r"for \(long long tile = blockIdx\.x; tile < ntiles; tile \+= gridDim\.x\) \{ // \(block-uniform\)",
     [STRIDE], "flags, scatter, diagonal and values stride over their tiles beyond the grid"),
    ("row loops", CSRC + "k_strength.hip", r"r < m; r \+= stride\) \{",
     [STRIDE], "the roots stride over rows (the stride test: 155 184 rows over 64 workgroups); the row pointers likewise over m + 1"),
    ("kMaxGridBlocks (grid striding)", CSRC + SHARED, r"const long long cap = max_grid_blocks\(\);",
     [STRIDE], "every kernel of the two entries strides over the work beyond max_grid_blocks() workgroups"),
    ("census grid", CSRC + SHARED, r"return grid > static_cast<unsigned>\(kCooCheckBlocks\) \? static_cast<unsigned>\(kCooCheckBlocks\) : grid;",
     [STRIDE, CONTRACT], "one count slot per wavefront of at most 1 024 workgroups (the colouring's census)"),
    ("kStrengthLumpPerLane", CSRC + "strength.hpp", r"constexpr int kStrengthLumpPerLane = 1;",
     [VALUES, STRIDE], "rows per lane of the diagonal pass"),
    ("kStrengthLumpWaveChunk", CSRC + "strength.hpp", r"constexpr int kStrengthLumpWaveChunk = 64 \* kStrengthLumpPerLane;",
     [VALUES], "64 rows per wavefront: the special values (16 rows) leave lanes empty, k130 (130) fills two wavefronts and starts a third"),
    ("kStrengthLumpTile", CSRC + "strength.hpp", r"constexpr int kStrengthLumpTile = 4 \* kStrengthLumpWaveChunk;",
     [VALUES, STRIDE], "256 rows per workgroup: aniso24 (576) is three tiles with a short last one; the stride case 607 tiles over 64 workgroups"),
    ("kCooLongRun", CSRC + "coo.hpp", r"constexpr int kCooLongRun = 64;",
     [MODEL, VALUES], "a row that drops more than 64 entries is lumped by a wavefront (star's hub: 299, k130's rows: about 90), the others by one lane"),
    ("an empty run copies the diagonal's bits", CSRC + "k_strength.hip", r"return dhi > dlo \? a \+ lump : a;",
     [VALUES], "rows that drop nothing (the tie, the -0.0 diagonal of the special values) against rows that drop"),
    ("no diagonal in S's row", CSRC + "k_strength.hip", r"if \(q >= hi \|\| s_colindex\[q\] != i\) return 0\.0;",
     [VALUES, VALUES_CONTRACT], "+0.0 and the lump discarded (fem_holes, grid7_holes, empties; a crafted s_rowptr)"),
    ("a map index outside [0, nnz)", CSRC + "k_strength.hip", r"if \(static_cast<unsigned>\(u\[k\]\) < static_cast<unsigned>\(nnz\)\) v\[k\] = value\[u\[k\]\];",
     [VALUES_CONTRACT], "+0.0 for a crafted map, in the values and in the lump"),
    ("kStrengthPerLane", CSRC + "strength.hpp", r"constexpr int kStrengthPerLane = 4;",
     [VALUES, STRIDE], "S entries per lane of the values pass (kept patterns of fewer than 256 entries leave lanes and steps empty: one, the special values)"),
    ("kStrengthWaveChunk", CSRC + "strength.hpp", r"constexpr int kStrengthWaveChunk = 64 \* kStrengthPerLane;",
     [VALUES, VALUES_CONTRACT], "256 entries per wavefront, whose rows are searched between the wavefront's two end rows"),
    ("kStrengthTile", CSRC + "strength.hpp", r"constexpr int kStrengthTile = 4 \* kStrengthWaveChunk;",
     [VALUES, STRIDE], "1 024 entries per workgroup: aniso24 (1 680 kept) is two tiles; the stride case more tiles than 64 workgroups"),
    ("omega == 0", CSRC + "k_strength.hip", r"if \(omega == 0\.0\) return on_diag \? d : v;",
     [VALUES, CAPTURE], "the filtered matrix (bits copied) against the smoother (omega = 2/3, 1.0, -0.5)"),
    ("a zero diag", CSRC + "k_strength.hip", r"if \(d == 0\.0\) return on_diag \? 1\.0 : 0\.0;",
     [VALUES], "identity rows: the 0.0 and -0.0 diagonals of the special values, the rows without a diagonal"),
    ("kEntryAlign", CSRC + HELPERS, r"constexpr size_t kEntryAlign = 256;",
     [MODEL], "workspace parts are padded to 256 B (row and entry counts that are no multiple of 64: most cases)"),
    ("no rows", CSRC + "strength.cpp", r"if \(m == 0\) \{",
     [MODEL], "m == 0: nothing is read, written or allocated"),
    ("no rows: the values", CSRC + "strength.cpp", r"if \(m == 0\) return kOk;",
     [VALUES], "nothing to launch"),
    ("no entries", CSRC + "k_strength.hip", r"if \(nnz <= 0\) return;",
     [MODEL, VALUES], "one_empty: a row without entries: the scatter and the values pass are not launched, diag is +0.0"),
    ("int32 block arithmetic", CSRC + HELPERS, r"inline bool too_large\(long long v\) \{ return v > INT_MAX - \(1 << 16\); \}",
     [CONTRACT, VALUES_CONTRACT], "m or nnz beyond this: SPMV_ACC_ERR_TOO_LARGE, as the other entries"),
    ("the census is shared", CSRC + "strength.cpp", r"pattern_census\(st, kEntry, ",
     [CONTRACT, MODEL], "the refusals and their text are entry_helpers.hpp's, the same for the four entries; the count of rows without a diagonal comes back from it"),
]


def test_strength_size_rules_name_their_tests():
    gpu_tests = open(os.path.join(ROOT, "tests", "test_gpu_strength.py")).read()
    defined = set(re.findall(r"^def (test_\w+)\(", gpu_tests, flags=re.M))
    for name, path, pattern, tests, what in STRENGTH_SIZE_RULES:
        assert re.search(pattern, open(os.path.join(ROOT, path)).read()), f"{name}: no longer matches {path}: {pattern}"
        assert tests and what
        for t in tests:
            assert t in defined, f"{name}: names {t}, which is not a test of tests/test_gpu_strength.py"
    # every named constant of the new files is registered above (tests/size_thresholds.py does not scan them)
    registered = " ".join(r[0] + " " + r[2] for r in STRENGTH_SIZE_RULES)
    found = 0
    for f in NEW_SOURCES:
        for k in re.findall(r"constexpr\s+[\w:<> ]+?\s+(k[A-Z]\w*)\s*=", open(os.path.join(ROOT, CSRC, f)).read()):
            found += 1
            assert k in registered, f"{f}: constant {k} is not in STRENGTH_SIZE_RULES"
    assert found == 7
    header = open(os.path.join(ROOT, CSRC, "strength.hpp")).read()
    assert f"constexpr int kStrengthRankTile = {RANK_TILE};" in header and f"constexpr int kStrengthLumpPerLane = {LUMP_PER_LANE};" in header
    assert f"constexpr int kStrengthPerLane = {PER_LANE};" in header and LONG_RUN == 64
    kernels = open(os.path.join(ROOT, CSRC, "k_strength.hip")).read()
    assert kernels.count("tile += gridDim.x") == 4 and kernels.count("+= stride)") == 2  # every loop over work is one of the registered forms


PROTOTYPES = (
    r"int spmv_acc_csr_strength\(int m, int nnz, const int \*d_rowptr, const int \*d_colindex, const double \*d_value, double theta,\s*"
    r"int \*d_s_rowptr, int \*d_s_colindex, int \*d_map, int \*d_drop_ptr, int \*h_nnz_s, int \*h_no_diag\);",
    r"int spmv_acc_csr_strength_values\(int m, int nnz, int nnz_s, const int \*d_s_rowptr, const int \*d_s_colindex, const int \*d_map,\s*"
    r"const int \*d_drop_ptr, const double \*d_value, double omega, double \*d_s_value, double \*d_diag\);",
)


def test_strength_entries_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "spmv_acc.h")).read()
    for proto in PROTOTYPES:
        assert re.search(proto, header), proto
    for entry in ("1", "2"):
        block = re.search(r"/\* ---- strength of connection, " + entry + r".*?\*/", header, flags=re.S)
        assert block, entry
        for word in ("replaces: nothing in the reference", "COST", "CHECKS", "CANNOT CHECK"):
            assert word in block.group(0), (entry, word)
    # the callers are no longer told to filter for themselves: the four places point at the new entry
    assert "value threshold is out of scope of this entry: spmv_acc_csr_strength does it" in " ".join(header.replace(" * ", " ").split())
    assert "spmv_acc_csr_strength" in open(os.path.join(ROOT, CSRC, "agg.hpp")).read()
    assert "spmv_acc_csr_strength" in open(os.path.join(ROOT, "INTEGRATION.md")).read() and "the caller filters" not in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "csr_strength" in spmv_acc_amd.csr_aggregate.__doc__
    # the header declares exactly what the package lists
    declared = set(re.findall(r"\b(sparse_spmv|spmv_acc_[a-z_0-9]+)\s*\(", header))
    assert declared == set(spmv_acc_amd.C_ABI_SYMBOLS), declared ^ set(spmv_acc_amd.C_ABI_SYMBOLS)
    lib = spmv_acc_amd.load_library()
    for s in ("spmv_acc_csr_strength", "spmv_acc_csr_strength_values"):
        assert s in spmv_acc_amd.C_ABI_SYMBOLS and hasattr(lib, s), s
    assert lib.spmv_acc_csr_strength.restype is ctypes.c_int and lib.spmv_acc_csr_strength_values.restype is ctypes.c_int
    assert len(lib.spmv_acc_csr_strength.argtypes) == 12 and len(lib.spmv_acc_csr_strength_values.argtypes) == 11
    for f in ("csr_strength", "csr_strength_values", "csr_smooth_prolongator"):
        assert callable(getattr(spmv_acc_amd, f))
    doc = spmv_acc_amd.csr_smooth_prolongator.__doc__
    recipe = doc.split("One level of an aggregation AMG setup on the device:")[1]
    steps = [recipe.index(s) for s in ("csr_strength(", "csr_aggregate(", "csr_tentative(", "csr_smooth_prolongator(", "csr_transpose(", "csr_spgemm(")]
    assert steps == sorted(steps) and recipe.count("csr_spgemm(") == 2 and "4 / (3 rho" in recipe  # the level recipe, in order; two products for R A P
    for f in ("k_strength.hip", "strength.cpp"):  # both builds compile the new files
        assert f in open(os.path.join(ROOT, CSRC, "Makefile")).read() and f in open(os.path.join(ROOT, "CMakeLists.txt")).read(), f
    assert "strength.hpp" in open(os.path.join(ROOT, CSRC, "Makefile")).read()
    assert " k_strength " in open(os.path.join(ROOT, "tools", "resource_usage.sh")).read()
    assert "spmv_acc_csr_strength" in open(os.path.join(ROOT, "README.md")).read()
    assert "spmv_acc_csr_strength" in open(os.path.join(ROOT, "DESIGN.md")).read()


BAD, TOO_LARGE = 2, 4  # SPMV_ACC_ERR_BAD_ARGUMENT, SPMV_ACC_ERR_TOO_LARGE


def test_bad_arguments_are_refused_without_a_gpu():
    """The C entries check their arguments before they touch the device: the error codes come back on a machine without one."""
    lib = spmv_acc_amd.load_library()
    one = 8  # (never dereferenced: a non-null pointer value)
    h_s, h_d = ctypes.c_int(-5), ctypes.c_int(-6)

    def strength(m=4, nnz=8, rp=one, ci=one, v=one, theta=0.25, srp=one, sci=one, mp=one, dp=one, hs=ctypes.byref(h_s), hd=ctypes.byref(h_d)):
        return lib.spmv_acc_csr_strength(m, nnz, rp, ci, v, theta, srp, sci, mp, dp, hs, hd)

    for neg in ("m", "nnz"):
        assert strength(**{neg: -1}) == BAD, neg
        assert b"spmv_acc_csr_strength: negative" in lib.spmv_acc_last_error_string()
    for null in ("rp", "ci", "v", "srp", "sci", "mp", "dp", "hs", "hd"):
        assert strength(**{null: None}) == BAD, null
        assert b"spmv_acc_csr_strength: null" in lib.spmv_acc_last_error_string(), null
    for theta in (-1.0, float("nan"), float("inf"), -float("inf"), -1e-300):
        assert strength(theta=theta) == BAD, theta
        assert b"spmv_acc_csr_strength: theta" in lib.spmv_acc_last_error_string()
    for big in (2 ** 31 - 1, 2 ** 31 - 2 ** 16):
        for which in ("m", "nnz"):
            assert strength(**{which: big}) == TOO_LARGE, which
            assert b"spmv_acc_csr_strength:" in lib.spmv_acc_last_error_string()
    assert strength(m=0, nnz=3) == BAD and b"without rows" in lib.spmv_acc_last_error_string()
    assert h_s.value == -5 and h_d.value == -6
    assert strength(m=0, nnz=0, rp=None, ci=None, v=None, srp=None, sci=None, mp=None, dp=None) == 0  # no rows: the device is not touched
    assert h_s.value == 0 and h_d.value == 0 and lib.spmv_acc_last_error() == 0

    # the values pass: value of nnz = 8 doubles (64 B), s_value of nnz_s = 6 (48 B) and diag of m = 4 (32 B) at distinct places
    v_at, s_at, d_at = 1 << 20, 2 << 20, 3 << 20

    def values(m=4, nnz=8, nnz_s=6, srp=one, sci=one, mp=one, dp=one, v=v_at, omega=2.0 / 3.0, sv=s_at, d=d_at):
        return lib.spmv_acc_csr_strength_values(m, nnz, nnz_s, srp, sci, mp, dp, v, omega, sv, d)

    for neg in ("m", "nnz", "nnz_s"):
        assert values(**{neg: -1}) == BAD, neg
        assert b"spmv_acc_csr_strength_values: negative" in lib.spmv_acc_last_error_string()
    assert values(nnz_s=9) == BAD and b"nnz_s exceeds nnz" in lib.spmv_acc_last_error_string()
    for null in ("srp", "sci", "mp", "dp", "v", "sv", "d"):
        assert values(**{null: None}) == BAD, null
        assert b"spmv_acc_csr_strength_values: null" in lib.spmv_acc_last_error_string(), null
    for omega in (float("nan"), float("inf"), -float("inf")):
        assert values(omega=omega) == BAD and b"omega must be finite" in lib.spmv_acc_last_error_string(), omega
    for big in (2 ** 31 - 1, 2 ** 31 - 2 ** 16):
        for which in ("m", "nnz"):
            assert values(**{which: big}) == TOO_LARGE, which
            assert b"spmv_acc_csr_strength_values:" in lib.spmv_acc_last_error_string()
    for bad in (dict(v=s_at), dict(v=s_at + 40), dict(v=s_at - 56), dict(d=s_at), dict(d=s_at + 40), dict(d=s_at - 24), dict(sv=v_at + 56), dict(sv=d_at - 40)):
        assert values(**bad) == BAD and b"overlaps an output" in lib.spmv_acc_last_error_string(), bad
    for bad in (dict(d=v_at), dict(d=v_at + 56), dict(d=v_at - 24), dict(v=d_at + 24)):
        assert values(**bad) == BAD and b"diag overlaps value" in lib.spmv_acc_last_error_string(), bad
    # nothing to do: no rows
    assert values(m=0, nnz=0, nnz_s=0, srp=None, sci=None, mp=None, dp=None, v=None, sv=None, d=None) == 0
    assert lib.spmv_acc_last_error() == 0
    lib.spmv_acc_clear_error()


def test_wrappers_refuse_bad_arguments():
    E = spmv_acc_amd.SpmvAccError
    m, nnz, nnz_s = 10, 30, 22

    def strength(match, mm=m, rp=_i(m + 1), ci=_i(nnz), v=_f(nnz), theta=0.25):
        with pytest.raises(E, match=match):
            spmv_acc_amd.csr_strength(mm, rp, ci, v, theta)

    strength("not on the GPU", ci=_i(nnz, cuda=False))
    strength("not on the GPU", v=_f(nnz, cuda=False))
    strength("dtype", rp=_FakeTensor(m + 1, dtype="torch.int64"))
    strength("dtype", ci=_f(nnz))
    strength("dtype", v=_i(nnz))
    strength("dtype", v=_FakeTensor(nnz, dtype="torch.float32"))
    strength("not contiguous", ci=_i(nnz, contiguous=False))
    strength("not contiguous", v=_f(nnz, contiguous=False))
    strength("elements", rp=_i(m))
    strength("as many", v=_f(nnz - 1))
    strength("as many", v=_f(nnz + 1))
    strength("on cuda:1", v=_f(nnz, device="cuda:1"))
    strength("torch tensor", rp=None)
    strength("torch tensor", ci=[0] * nnz)
    strength("torch tensor", v=3.0)
    strength("negative", mm=-1)
    for theta in (-1.0, float("nan"), float("inf")):
        strength("theta", theta=theta)

    good = dict(srp=_i(m + 1), sci=_i(nnz_s), mp=_i(nnz), dp=_i(m + 1), v=_f(nnz), sv=_f(nnz_s), d=_f(m))

    def values(match, mm=m, omega=0.0, **bad):
        a = dict(good, **bad)
        with pytest.raises(E, match=match):
            spmv_acc_amd.csr_strength_values(mm, a["srp"], a["sci"], a["mp"], a["dp"], a["v"], a["sv"], a["d"], omega)

    values("not on the GPU", srp=_i(m + 1, cuda=False))
    values("not on the GPU", v=_f(nnz, cuda=False))
    values("not on the GPU", d=_f(m, cuda=False))
    values("dtype", sci=_f(nnz_s))
    values("dtype", mp=_FakeTensor(nnz, dtype="torch.int64"))
    values("dtype", v=_i(nnz))
    values("dtype", sv=_i(nnz_s))
    values("dtype", d=_FakeTensor(m, dtype="torch.float32"))
    values("not contiguous", sv=_f(nnz_s, contiguous=False))
    values("not contiguous", mp=_i(nnz, contiguous=False))
    values("elements", srp=_i(m))
    values("elements", dp=_i(0))
    values("as many", v=_f(nnz - 1))
    values("as many", v=_f(nnz + 1))
    values("as many", sv=_f(nnz_s + 1))
    values("as many", sv=_f(nnz_s - 1))
    values("as many", d=_f(m + 1))
    values("at most as many", sci=_i(nnz + 1), sv=_f(nnz + 1))
    values("on cuda:1", d=_f(m, device="cuda:1"))
    values("torch tensor", srp=None)
    values("torch tensor", sv=None)
    values("torch tensor", d=[0.0] * m)
    values("torch tensor", v=3.0)
    values("negative", mm=-1)
    values("omega", omega=float("nan"))
    values("omega", omega=float("inf"))
    P = (_i(m + 1), _i(m), _f(m))
    with pytest.raises(E, match="torch tensor"):
        spmv_acc_amd.csr_smooth_prolongator(m, 3, _i(m + 1), None, _i(nnz), _i(m + 1), _f(nnz), P, 2.0 / 3.0)
    with pytest.raises(E, match="negative"):
        spmv_acc_amd.csr_smooth_prolongator(m, -1, _i(m + 1), _i(nnz_s), _i(nnz), _i(m + 1), _f(nnz), P, 2.0 / 3.0)
    with pytest.raises(E, match="p_rowptr, p_colindex, p_value"):
        spmv_acc_amd.csr_smooth_prolongator(m, 3, _i(m + 1), _i(nnz_s), _i(nnz), _i(m + 1), _f(nnz), _f(m), 2.0 / 3.0)


def test_strength_entries_keep_no_state():
    """As test_agg_entries_keep_no_state: the engine file neither finds nor makes a plan, counts no plan work, reads no tunable and keeps nothing
    static; the filter's one allocation is freed on every way out; the values pass is launch-only."""
    src = open(os.path.join(ROOT, CSRC, "strength.cpp")).read()
    code = re.sub(r"//[^\n]*", "", src)
    for word in ("get_plan", "g_plans", "t_plan_work", "t_last_plan", "tune_", "TimingPhase", "TuneTimer", "static std::", "thread_local", "g_tunables"):
        assert word not in code, word
    assert not re.search(r"\bstatic\b(?! const char \*const kEntry)", code), "a static other than the entries' names"
    assert code.count("hipMalloc(") == 1 and code.count("hipFree(") == 1 and "const auto leave = " in code
    leave = code.split("const auto leave = ")[1].split("};", 1)[0]
    assert leave.count("hipFree(") == 1 and "hipStreamSynchronize(" in leave.split("hipFree(")[0]  # the stream has run before the workspace goes
    assert "plan_work_allowed(" in code.split("const auto leave = ")[0]  # (a capture is refused before anything is enqueued or allocated)
    assert "hipMalloc(" not in code.split("const auto leave = ")[0]
    after = code.split("const auto leave = ")[1].split("};", 1)[1].split("\n}\n")[0]  # (to the end of the routine that allocates)
    launches = ("pattern_census", "launch_strength_sd", "launch_strength_flags", "launch_coo_scan", "launch_strength_ptrs", "launch_strength_scatter")
    for launch in launches:
        assert launch in after, launch
    body = after.split("hipMalloc(")[1]
    assert [body.index(s + "(st, ") for s in launches] == sorted(body.index(s + "(st, ") for s in launches)  # the passes in the documented order
    assert body.index("pattern_census(") < body.index("launch_strength_sd(")  # the census is judged before anything is written
    assert 'pattern_census(st, kEntry, m, nnz, d_rowptr, d_colindex, d_slots, "filter A + A^T instead", ' in body
    bare = [ln.strip() for ln in after.splitlines() if re.search(r"\breturn\b(?! leave\()", ln)]
    # (the one way out that may skip leave(): the scratch query before the allocation)
    assert bare == ['return entry_error(kEntry, kErrHip, "scan workspace query failed");'], bare
    tail = after.split("launch_strength_scatter")[1]
    assert tail.index("*h_nnz_s = nnz_s;") < tail.index("*h_no_diag = ") < tail.index("return leave(kOk);")  # (written last, once everything else has run)
    assert "while (" not in code and "for (;;)" not in code  # no host loop that waits on the device
    values = code.split("int run_csr_strength_values")[1]
    assert "hipMalloc" not in values and "Synchronize" not in values and "hipMemcpy" not in values and "hipMemset" not in values  # launch-only
    assert "plan_work_allowed" not in values and values.count("launch_strength_diag(") == 1 and values.count("launch_strength_values(") == 1
    assert re.findall(r"\blaunch_\w+\(", values) == ["launch_strength_diag(", "launch_strength_values(", "launch_error("]  # two kernels, then the check
    assert values.index("overlaps an output") < values.index("diag overlaps value") < values.index("launch_strength_diag(")  # refused before any launch
    assert values.index("omega must be finite") < values.index("launch_strength_diag(")
    kernels = open(os.path.join(ROOT, CSRC, "k_strength.hip")).read()
    assert "atomic" not in re.sub(r"//[^\n]*", "", kernels).lower() and "__syncthreads" not in kernels and "while (" not in re.sub(r"//[^\n]*", "", kernels)
    assert kernels.count("#pragma clang fp contract(off)") == 3  # the edge's rhs, the lumped diagonal, the entry of M


KERNELS = ("strength_sd_kernel", "strength_flags_kernel", "strength_ptrs_kernel", "strength_scatter_kernel", "strength_diag_kernel",
           "strength_values_kernel")
# as recorded in k_strength.hip's header comment
RECORDED_VGPRS = dict(strength_sd_kernel=14, strength_flags_kernel=24, strength_ptrs_kernel=22, strength_scatter_kernel=13, strength_diag_kernel=34,
                      strength_values_kernel=54)


def test_strength_kernels_fit_their_register_budget(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_table

    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-DKERNEL_STRATEGY_ADAPTIVE",
                        "-I" + os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
                        os.path.join(ROOT, CSRC, "k_strength.hip"), "-o", str(tmp_path / "k_strength.o")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    header = open(os.path.join(ROOT, CSRC, "k_strength.hip")).read().split("#include")[0]
    rows = [k for k in resource_table.parse(r.stderr) if "rocprim" not in k["name"]]
    for k in rows:
        k["name"] = re.sub(r"<.*", "", k["name"])
    assert sorted(k["name"] for k in rows) == sorted(KERNELS), sorted(k["name"] for k in rows)
    for k in rows:
        assert k["scratch"] == 0 and k["agprs"] == 0 and k["vgprs"] <= 64 and k["occupancy"] >= 8, k
        want = RECORDED_VGPRS[k["name"]]
        assert re.search(k["name"] + r", " + str(want) + r"\b", header), (k["name"], "the count recorded in the header comment")
        assert k["vgprs"] <= want + 4, (k, "grew past the count recorded in k_strength.hip (a few registers of compiler drift are allowed)")


# ---- the kept pattern (strength.hpp), in numpy: the GPU suite's reference ------------------------------------------------------------------------
def mirror_positions(m, rp, ci):
    """(q, found): the position of (j, i) for every entry (i, j) of a CSR with strictly ascending rows (any q where it is not stored)."""
    row = np.repeat(np.arange(m, dtype=np.int64), np.diff(rp))
    key = row * max(m, 1) + ci  # ascending: the rows strictly ascend
    q = np.searchsorted(key, ci.astype(np.int64) * max(m, 1) + row)
    found = q < ci.size
    found[found] = key[q[found]] == (ci.astype(np.int64) * max(m, 1) + row)[found]
    return np.where(found, q, 0), found


def host_csr_strength(m, rp, ci, v, theta):
    """(s_rowptr, s_colindex, map, drop_ptr, nnz_s, no_diag, keep) by the definition of strength.hpp; keep: the flag of every position of A."""
    rp, ci, v = np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64), np.asarray(v, dtype=np.float64)
    nnz = ci.size
    row = np.repeat(np.arange(m, dtype=np.int64), np.diff(rp))
    on_diag = ci == row
    theta = np.float64(theta)
    with np.errstate(all="ignore"):
        sd = np.zeros(m)
        sd[row[on_diag]] = np.sqrt(np.abs(v[on_diag]))
        q, found = mirror_positions(m, rp, ci)
        rhs = (sd[row] * sd[ci]) * theta  # the two roots first, then theta: each product rounded on its own
        keep = on_diag | (np.abs(v) >= rhs) | (found & (np.abs(v[q]) >= rhs))  # IEEE: a NaN on either side is false
    pos = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
    nnz_s = int(pos[nnz])
    smap = np.concatenate([np.flatnonzero(keep), np.flatnonzero(~keep)]).astype(np.int32)
    s_rowptr = pos[rp].astype(np.int32)
    drop_ptr = (nnz_s + rp - pos[rp]).astype(np.int32)
    no_diag = m - int(np.unique(row[on_diag]).size)
    return s_rowptr, ci[keep].astype(np.int32), smap, drop_ptr, nnz_s, no_diag, keep


# ---- the values (strength.hpp), in numpy, bit for bit: the GPU suite's reference ---------------------------------------------------------------
def last_at_most(ptr, lo, hi, q):
    """structure_passes.hpp last_at_most, step for step: what it returns on ANY array."""
    while lo < hi:
        mid = lo + (hi - lo + 1) // 2
        if ptr[mid] <= q:
            lo = mid
        else:
            hi = mid - 1
    return lo


def first_at_least(key, lo, hi, c):
    """structure_passes.hpp first_at_least, step for step."""
    while lo < hi:
        mid = lo + (hi - lo) // 2
        if key[mid] < c:
            lo = mid + 1
        else:
            hi = mid
    return lo


def rows_of_entries(m, nnz_s, s_rowptr):
    """The row the values pass gives every entry of S.  A pointer as the analysis left it: the last row that begins at or before the entry.
    Any other array: the device's searches, a wavefront's kStrengthWaveChunk entries between the rows of its two ends."""
    ptr = np.asarray(s_rowptr, dtype=np.int64)
    j = np.arange(nnz_s, dtype=np.int64)
    if ptr[0] == 0 and ptr[m] == nnz_s and np.all(np.diff(ptr[:m + 1]) >= 0):
        return np.searchsorted(ptr[:m], j, side="right") - 1
    rows = np.zeros(nnz_s, dtype=np.int64)
    for base in range(0, nnz_s, WAVE_CHUNK):
        last = min(base + WAVE_CHUNK, nnz_s) - 1
        r_first = last_at_most(ptr, 0, m - 1, base)
        r_last = last_at_most(ptr, r_first, m - 1, last)
        for e in range(base, last + 1):
            rows[e] = last_at_most(ptr, r_first, r_last, e)
    return rows


def host_strength_values(m, nnz_s, s_rowptr, s_colindex, smap, drop_ptr, value, omega=0.0):
    """(s_value, diag).  The maps are taken as they are: runs clamped to [0, nnz], S's rows to [0, nnz_s], a map index outside [0, nnz) gives +0.0."""
    s_rowptr, s_colindex, smap, drop_ptr = (np.asarray(a, dtype=np.int64) for a in (s_rowptr, s_colindex, smap, drop_ptr))
    value = np.asarray(value, dtype=np.float64)
    nnz = smap.size
    omega = np.float64(omega)
    inside = (smap >= 0) & (smap < nnz)
    through = np.where(inside, value[np.where(inside, smap, 0)], 0.0) if nnz else np.zeros(0)  # A's values in map's order
    with np.errstate(all="ignore"):
        lump = coo_sum_model(smap, drop_ptr[:m + 1], value) if m else np.zeros(0)  # coo.hpp's order; an empty run gives +0.0
        dlo = np.clip(drop_ptr[:m], 0, nnz)
        empty = np.maximum(np.clip(drop_ptr[1:m + 1], 0, nnz), dlo) == dlo
        diag = np.zeros(m)
        for i in range(m):
            lo = min(max(int(s_rowptr[i]), 0), nnz_s)
            hi = min(max(int(s_rowptr[i + 1]), lo), nnz_s)
            q = first_at_least(s_colindex, lo, hi, i)
            if q < hi and s_colindex[q] == i:
                diag[i] = through[q] if empty[i] else through[q] + lump[i]
        rows = rows_of_entries(m, nnz_s, s_rowptr) if m and nnz_s else np.zeros(0, dtype=np.int64)
        vals, d, on = through[:nnz_s], diag[rows], s_colindex[:nnz_s] == rows
        if omega == 0.0:
            s_value = np.where(on, d, vals)
        else:
            safe = np.where(d == 0.0, 1.0, d)
            s_value = np.where(d == 0.0, np.where(on, 1.0, 0.0), np.where(on, 1.0 - omega, (-omega * vals) / safe))
    return s_value, diag


# ---- the cases of the GPU suite, made once ----------------------------------------------------------------------------------------------------
EPS = 0.01


def aniso_matrix(n, eps):
    """The five-point grid with couplings -1 along a grid line (consecutive rows) and -eps across, diagonal 2 + 2 eps: (m, (rowptr, colindex, value))."""
    rp, ci, _ = csr_from_pattern(n * n, grid5_pairs(n, n), np.random.default_rng(0))
    row = np.repeat(np.arange(n * n), np.diff(rp))
    v = np.where(ci == row, 2.0 + 2.0 * eps, np.where(np.abs(ci - row) == 1, -1.0, -eps))
    return n * n, (rp, ci, v)


def lognormal_values(m, rp, ci, rng, symmetric):
    """Negative log-normal couplings and a positive diagonal of their size: symmetric (a function of the unordered pair) or each drawn alone."""
    row = np.repeat(np.arange(m), np.diff(rp))
    w = -rng.lognormal(0.0, 1.5, ci.size)
    if symmetric:
        q, found = mirror_positions(m, rp, ci)
        assert found.all()
        w = np.where(row <= ci, w, w[q])
    return np.where(ci == row, rng.lognormal(1.0, 1.0, ci.size), w)


def special_matrix():
    """A chain of 16 rows, diagonal 2 and couplings -1, with: a weak pair (0, 1); a NaN at (2, 3) whose mirror is weak; an inf diagonal in row
    6; a 0.0 diagonal in row 9 and a -0.0 one in row 12; a NaN diagonal in row 14."""
    m = 16
    rp, ci, _ = csr_from_pattern(m, [(i, j) for i in range(m) for j in (i - 1, i, i + 1) if 0 <= j < m], np.random.default_rng(0))
    row = np.repeat(np.arange(m), np.diff(rp))
    v = np.where(ci == row, 2.0, -1.0)

    def at(i, j):
        return int(np.flatnonzero((row == i) & (ci == j))[0])

    v[at(0, 1)] = v[at(1, 0)] = -0.01
    v[at(2, 3)], v[at(3, 2)] = np.nan, -0.01
    v[at(6, 6)] = np.inf
    v[at(9, 9)] = 0.0
    v[at(12, 12)] = -0.0
    v[at(14, 14)] = np.nan
    return m, (rp, ci, v), at


def _cases():
    yield "aniso24", *aniso_matrix(24, EPS), 0.25
    m, A = grid5_matrix(24)
    yield "tie", m, A, 0.25
    yield "above_tie", m, A, float(np.nextafter(0.25, 1.0))
    rng = np.random.default_rng(2032)
    for tag in AGG_TAGS:
        m, (rp, ci) = agg_cases()[tag]
        yield tag + "_sym", m, (rp, ci, lognormal_values(m, rp, ci, rng, True)), 0.25
        yield tag + "_uns", m, (rp, ci, lognormal_values(m, rp, ci, rng, False)), 0.25
    m, (rp, ci) = agg_cases()["star"]
    row = np.repeat(np.arange(m), np.diff(rp))
    yield "star_hub", m, (rp, ci, np.where(ci == row, np.where(row == 0, 1e6, 1.0), -1.0)), 0.25  # the hub's rhs is 250: its 299 couplings drop
    m, (rp, ci) = agg_cases()["k130"]
    row = np.repeat(np.arange(m), np.diff(rp))
    yield "k130_weak", m, (rp, ci, np.where(ci == row, 100.0, -25.0 * rng.lognormal(-1.0, 1.0, ci.size))), 0.25  # about 90 of a row's 129 drop
    m, A, _ = special_matrix()
    yield "special", m, A, 0.25


@functools.lru_cache(maxsize=None)
def cases():
    """tag -> (m, (rowptr, colindex, value), theta); made once and shared, nothing changes them."""
    return {tag: (m, A, theta) for tag, m, A, theta in _cases()}


TAGS = ("aniso24", "tie", "above_tie") + tuple(t + s for t in AGG_TAGS for s in ("_sym", "_uns")) + ("star_hub", "k130_weak", "special")


@functools.lru_cache(maxsize=None)
def strength(tag):
    """host_csr_strength of a case, computed once."""
    m, (rp, ci, v), theta = cases()[tag]
    return host_csr_strength(m, rp, ci, v, theta)


def check_partition(m, rp, ci, s_rowptr, s_colindex, smap, drop_ptr, nnz_s, keep):
    """What any stable partition by a symmetric keep flag is, from the flags alone."""
    nnz = ci.size
    row = np.repeat(np.arange(m), np.diff(rp))
    kept = set(zip(row[keep].tolist(), ci[keep].tolist()))
    assert all((j, i) in kept for i, j in kept)  # the kept pattern is symmetric
    assert np.all(keep[ci == row])  # a stored diagonal is always kept
    assert np.array_equal(np.sort(smap), np.arange(nnz)) and np.all(np.diff(smap[:nnz_s]) > 0) and np.all(np.diff(smap[nnz_s:]) > 0)
    assert np.array_equal(s_colindex, ci[smap[:nnz_s]]) and np.all(keep[smap[:nnz_s]]) and not np.any(keep[smap[nnz_s:]])
    assert s_rowptr.size == drop_ptr.size == m + 1 and s_rowptr[0] == 0 and s_rowptr[m] == nnz_s and drop_ptr[0] == nnz_s and drop_ptr[m] == nnz
    for i in range(m):
        mine = np.arange(rp[i], rp[i + 1])
        assert np.array_equal(smap[s_rowptr[i]:s_rowptr[i + 1]], mine[keep[mine]]), i
        assert np.array_equal(smap[drop_ptr[i]:drop_ptr[i + 1]], mine[~keep[mine]]), i
        assert np.all(np.diff(s_colindex[s_rowptr[i]:s_rowptr[i + 1]]) > 0), i  # S's rows strictly ascend


def test_the_cases_and_their_kept_patterns():
    assert set(TAGS) == set(cases()) and len(TAGS) == len(set(TAGS))
    dropped_runs = []
    for tag in TAGS:
        m, (rp, ci, v), theta = cases()[tag]
        assert rp.size == m + 1 and rp[0] == 0 and rp[m] == ci.size == v.size, tag
        s_rowptr, s_colindex, smap, drop_ptr, nnz_s, no_diag, keep = strength(tag)
        check_partition(m, rp, ci, s_rowptr, s_colindex, smap, drop_ptr, nnz_s, keep)
        row = np.repeat(np.arange(m), np.diff(rp))
        assert no_diag == m - np.count_nonzero(ci == row), tag
        dropped_runs.append(np.diff(drop_ptr))
        # each case with couplings holds kept entries, and dropped ones unless it is there to keep everything or has too few to choose from
        if np.any(ci != row):
            assert nnz_s > 0, tag
            keeps_all = tag in ("tie",) or tag.startswith(("one", "none"))
            assert (nnz_s == ci.size) == keeps_all, (tag, nnz_s, ci.size)
    runs = np.concatenate(dropped_runs)
    assert np.any(runs > LONG_RUN) and np.any((runs > 0) & (runs <= LONG_RUN)) and np.any(runs == 0)  # both sides of kCooLongRun, and empty runs
    assert np.diff(strength("star_hub")[3])[0] == 299 and np.median(np.diff(strength("k130_weak")[3])) > LONG_RUN
    assert strength("fem_holes_sym")[5] == 40 and strength("grid7_holes_uns")[5] == 101 and strength("empties_sym")[5] == 50
    assert strength("none_sym")[4] == 0 and strength("one_sym")[4] == 1 and strength("one_empty_uns")[4] == 0


def test_the_two_ends_of_theta():
    for tag in ("fem_sym", "grid27_uns", "random3000_uns", "k130_weak", "empties_sym"):
        m, (rp, ci, v), _ = cases()[tag]
        row = np.repeat(np.arange(m), np.diff(rp))
        everything = host_csr_strength(m, rp, ci, v, 0.0)
        assert everything[4] == ci.size and np.array_equal(everything[2], np.arange(ci.size)) and np.array_equal(everything[0], rp), tag
        assert np.all(everything[3] == ci.size)
        with_diag = np.zeros(m, dtype=bool)
        with_diag[row[ci == row]] = True
        both = with_diag[row] & with_diag[ci]  # (an edge with an end without a diagonal has rhs 0 and is always kept)
        nothing = host_csr_strength(m, rp, ci, v, 1e12)
        assert np.array_equal(nothing[6][both], (ci == row)[both]) and np.all(nothing[6][~both]), tag
    m, (rp, ci, v), _ = cases()["k130_weak"]
    assert host_csr_strength(m, rp, ci, v, 1e12)[4] == m  # a theta above every ratio keeps exactly the stored diagonals


def test_the_tie():
    """grid5_matrix(24), values 4 and -1: at theta = 0.25 rhs is exactly 1.0 and >= keeps every entry; one ulp above, every off-diagonal drops and
    the lumped diagonal is 4 - (the number of neighbours), exactly."""
    m, (rp, ci, v), theta = cases()["tie"]
    s_rowptr, s_colindex, smap, drop_ptr, nnz_s, no_diag, keep = strength("tie")
    assert theta == 0.25 and nnz_s == ci.size and keep.all() and np.array_equal(s_rowptr, rp) and np.array_equal(s_colindex, ci) and no_diag == 0
    s_value, diag = host_strength_values(m, nnz_s, s_rowptr, s_colindex, smap, drop_ptr, v)
    assert np.array_equal(s_value.view(np.uint64), v.view(np.uint64)) and np.all(diag == 4.0)
    m, (rp, ci, v), theta = cases()["above_tie"]
    s_rowptr, s_colindex, smap, drop_ptr, nnz_s, no_diag, keep = strength("above_tie")
    assert 0.25 < theta < 0.25 + 1e-15 and nnz_s == m and np.array_equal(s_colindex, np.arange(m)) and np.array_equal(s_rowptr, np.arange(m + 1))
    s_value, diag = host_strength_values(m, nnz_s, s_rowptr, s_colindex, smap, drop_ptr, v)
    assert np.array_equal(diag, 4.0 - (np.diff(rp) - 1)) and np.array_equal(s_value, diag) and set(diag.tolist()) == {0.0, 1.0, 2.0}


def test_the_mirror():
    """Values of (i, j) and (j, i) drawn independently: entries are kept only because their mirror is strong, and edges drop in both directions."""
    for tag in ("fem_uns", "random3000_uns", "grid27_uns"):
        m, (rp, ci, v), theta = cases()[tag]
        keep = strength(tag)[6]
        row = np.repeat(np.arange(m), np.diff(rp))
        q, found = mirror_positions(m, rp, ci)
        assert found.all() and np.array_equal(q[q], np.arange(ci.size)) and np.array_equal(keep, keep[q])
        sd = np.zeros(m)
        sd[row[ci == row]] = np.sqrt(np.abs(v[ci == row]))
        own = np.abs(v) >= sd[row] * sd[ci] * theta
        off = ci != row
        assert np.count_nonzero(off & keep & ~own & own[q]) > 10, tag  # kept only because the mirror is strong
        assert np.count_nonzero(off & ~keep) > 10 and not np.any(off & ~keep & (own | own[q])), tag  # dropped in both directions, weak in both


def test_aniso24():
    m, (rp, ci, v), theta = cases()["aniso24"]
    s_rowptr, s_colindex, smap, drop_ptr, nnz_s, no_diag, keep = strength("aniso24")
    assert ci.size == 2784 and nnz_s == 1680 and no_diag == 0
    row = np.repeat(np.arange(m), np.diff(rp))
    assert np.array_equal(keep, np.abs(ci - row) <= 1)  # the diagonal and the couplings along the line
    agg, agg_rows, agg_ptr, naggs = host_csr_aggregate(m, s_rowptr, s_colindex)
    assert naggs == 167 and np.all(agg_rows[agg_ptr[:naggs + 1][:-1]] // 24 == agg_rows[agg_ptr[1:naggs + 1] - 1] // 24)  # each inside one grid line
    s_value, diag = host_strength_values(m, nnz_s, s_rowptr, s_colindex, smap, drop_ptr, v)
    for i in range(m):
        want = np.float64(2.0 + 2.0 * EPS)
        dropped = int(drop_ptr[i + 1] - drop_ptr[i])
        if dropped:
            lump = np.float64(-EPS)
            for _ in range(dropped - 1):
                lump = lump + np.float64(-EPS)
            want = want + lump
        assert diag[i] == want and dropped in (1, 2), i
    assert np.array_equal(s_value[s_colindex == rows_of_entries(m, nnz_s, s_rowptr)], diag) and np.all(s_value[s_colindex != rows_of_entries(m, nnz_s, s_rowptr)] == -1.0)


def test_special_values():
    m, (rp, ci, v), at = special_matrix()
    s_rowptr, s_colindex, smap, drop_ptr, nnz_s, no_diag, keep = strength("special")
    assert not keep[at(0, 1)] and not keep[at(1, 0)]  # weak in both directions
    assert not keep[at(2, 3)] and not keep[at(3, 2)]  # a NaN fails its comparison, its mirror is weak
    assert not keep[at(6, 5)] and not keep[at(5, 6)] and not keep[at(6, 7)] and not keep[at(7, 6)]  # an inf diagonal: rhs is inf
    assert keep[at(9, 8)] and keep[at(8, 9)] and keep[at(9, 10)] and keep[at(12, 11)] and keep[at(12, 13)]  # a zero diagonal of either sign: rhs is 0
    assert not keep[at(14, 13)] and not keep[at(13, 14)] and not keep[at(14, 15)]  # a NaN diagonal: rhs is NaN
    assert keep[ci == np.repeat(np.arange(m), np.diff(rp))].all()
    a_f, diag = host_strength_values(m, nnz_s, s_rowptr, s_colindex, smap, drop_ptr, v)
    assert np.isnan(diag[2]) and diag[3] == 2.0 - 0.01 and diag[6] == np.inf and diag[5] == 1.0 and diag[7] == 1.0 and np.isnan(diag[14])
    assert diag[9] == 0.0 and not np.signbit(diag[9]) and diag[12] == 0.0 and np.signbit(diag[12]) and diag[13] == 1.0  # (the bits of -0.0 copied)
    for omega in (2.0 / 3.0, 1.0, -0.5):
        mv, _ = host_strength_values(m, nnz_s, s_rowptr, s_colindex, smap, drop_ptr, v, omega)
        rows = rows_of_entries(m, nnz_s, s_rowptr)
        for i in (9, 12):  # identity rows
            mine = rows == i
            assert np.array_equal(mv[mine], (s_colindex[mine] == i).astype(np.float64)) and not np.signbit(mv[mine]).any(), (omega, i)
        assert np.isnan(mv[(rows == 2) & (s_colindex != 2)]).all() and mv[(rows == 2) & (s_colindex == 2)][0] == 1.0 - omega
        assert np.all(mv[(rows == 6) & (s_colindex == 6)] == 1.0 - omega)  # (row 6 kept only its diagonal)


def test_row_sums_and_the_smoother():
    """Row sums of A_F are those of A within (row length + 1) ulp of the row's absolute sum (rows with a stored diagonal), the bits of the
    lumps are row_sum's, and M 1 = 1 - omega rowsum(A_F) / f to rounding."""
    for tag in ("aniso24", "fem_sym", "fem_holes_uns", "random3000_uns", "grid27_sym", "star_hub", "k130_weak", "lonely_uns"):
        m, (rp, ci, v), _ = cases()[tag]
        s_rowptr, s_colindex, smap, drop_ptr, nnz_s, no_diag, keep = strength(tag)
        a_f, diag = host_strength_values(m, nnz_s, s_rowptr, s_colindex, smap, drop_ptr, v)
        rows = rows_of_entries(m, nnz_s, s_rowptr)
        row = np.repeat(np.arange(m), np.diff(rp))
        assert np.array_equal(rows, row[keep]), tag
        stored = np.zeros(m, dtype=bool)
        stored[row[ci == row]] = True
        for i in range(m):  # the lump's bits, from the definition alone
            d = v[rp[i]:rp[i + 1]][~keep[rp[i]:rp[i + 1]]]
            if stored[i]:
                a_ii = v[rp[i]:rp[i + 1]][ci[rp[i]:rp[i + 1]] == i][0]
                want = a_ii if d.size == 0 else a_ii + row_sum(d, 1 if d.size <= LONG_RUN else 64)
                assert diag[i] == want, (tag, i)
            else:
                assert diag[i] == 0.0 and not np.signbit(diag[i]), (tag, i)
        exact_a = np.array([np.sum(v[rp[i]:rp[i + 1]].astype(np.longdouble)) for i in range(m)])
        exact_f = np.array([np.sum(a_f[s_rowptr[i]:s_rowptr[i + 1]].astype(np.longdouble)) for i in range(m)])
        scale = np.array([np.sum(np.abs(v[rp[i]:rp[i + 1]])) for i in range(m)])
        bound = (np.diff(rp) + 1) * 2.0 ** -52 * scale
        assert np.all(np.abs(exact_a - exact_f)[stored] <= bound[stored]), tag
        omega = 2.0 / 3.0
        mv, _ = host_strength_values(m, nnz_s, s_rowptr, s_colindex, smap, drop_ptr, v, omega)
        m_one = np.array([np.sum(mv[s_rowptr[i]:s_rowptr[i + 1]].astype(np.longdouble)) for i in range(m)])
        live = stored & (diag != 0.0)
        want = 1.0 - omega * exact_f[live] / diag[live].astype(np.longdouble)
        kept_scale = np.array([np.sum(np.abs(a_f[s_rowptr[i]:s_rowptr[i + 1]])) for i in range(m)])
        # (each entry of M carries two roundings of a term of size omega |a| / |f|, the diagonal one of size 1)
        slack = (np.diff(s_rowptr)[live] + 2) * 2.0 ** -52 * (1.0 + omega * kept_scale[live] / np.abs(diag[live]))
        assert np.all(np.abs(m_one[live] - want) <= slack), tag
        assert np.all(m_one[~live] == np.where(np.diff(s_rowptr)[~live] > 0, stored[~live] * 1.0, 0.0)), tag  # identity rows; rows without a diagonal: zeros


def test_crafted_maps_in_the_model():
    """The model takes any arrays, as the device does: a descending s_rowptr, indices out of range."""
    m, (rp, ci, v), _ = cases()["fem_sym"]
    s_rowptr, s_colindex, smap, drop_ptr, nnz_s, no_diag, keep = strength("fem_sym")
    clean = host_strength_values(m, nnz_s, s_rowptr, s_colindex, smap, drop_ptr, v, 0.5)
    wild = smap.copy()
    wild[[3, nnz_s + 2]] = [-1, 2 ** 31 - 1]
    got = host_strength_values(m, nnz_s, s_rowptr, s_colindex, wild, drop_ptr, v, 0.5)
    assert np.all(np.isfinite(got[0])) and np.count_nonzero(got[0] != clean[0]) >= 1
    got = host_strength_values(m, nnz_s, s_rowptr[::-1].copy(), s_colindex, smap, drop_ptr, v, 0.5)
    assert got[0].size == nnz_s and np.all(np.isfinite(got[0])) and np.all(got[1] == 0.0)  # every clamped row of S is empty: no diagonal is found
    rows = rows_of_entries(m, nnz_s, s_rowptr[::-1].copy())
    assert rows.min() >= 0 and rows.max() < m
