"""CPU side of the aggregation coarsening (no GPU): the C ABI declares and exports the two entries, they and the Python wrappers refuse bad
arguments before any launch, the compiled kernels use no scratch and no AGPR and fit 64 VGPRs, every size-selected branch of the new code names
the GPU tests that cross it, the engine file stays stateless, and the definitions are restated here in numpy and exported to the GPU suite as
its references: the aggregates (host_csr_aggregate, the sequential greedy and the two assignment passes; host_csr_aggregate_rounds, the key /
T1 / T2 form, which must give the same arrays) and the tentative prolongator's values in their documented summation order
(host_tentative_values, bit for bit), checked against independent statements: the invariants of a distance-2 maximal independent set and its
aggregates, and P^T P = I."""
import ctypes
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import spmv_acc_amd
from test_coo_host import LONG_RUN, SHARED, _FakeTensor, _f, _i, coo_sum_model
from test_gs_host import TAGS as GS_TAGS
from test_gs_host import cases as gs_cases
from test_gs_host import HELPERS, csr_from_pattern, priorities, row_sum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "spmv_acc_amd/csrc/"
NEW_SOURCES = ("agg.hpp", "k_agg.hip", "agg.cpp")
MODEL = "test_aggregate_is_the_host_model"
CONTRACT = "test_aggregate_contract"
STRIDE = "test_agg_grid_stride_at_test_size"
VALUES = "test_tentative_values_are_the_host_model"
VALUES_CONTRACT = "test_tentative_contract"
ROUNDS_PER_READ, LANE_GROUP, PER_LANE = 4, 1, 1  # kAggRoundsPerRead, kAggLaneGroup, kAggPerLane (AGG_SIZE_RULES holds them to the source)
KEY_ROOT, KEY_OUT = np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(0)

# (rule, file, regex that must match the source, GPU tests of tests/test_gpu_agg.py that cross it at test size, what it selects)
AGG_SIZE_RULES = [
    ("kAggRoot", CSRC + "agg.hpp", r"constexpr unsigned long long kAggRoot = ~0ull;",
     [MODEL], "the key of a root, above every priority (every case has a root)"),
    ("kAggOut", CSRC + "agg.hpp", r"constexpr unsigned long long kAggOut = 0ull;",
     [MODEL], "the key of a row with a root within distance 2, below every priority: row 0's undecided key is gs_priority(0) + 1 = 1, not 0"),
    ("kAggRoundsPerRead", CSRC + "agg.hpp", r"constexpr int kAggRoundsPerRead = 4;",
     [MODEL], "rounds between two reads: star and k130 end inside the first group (2 rounds), band25 and empties at its end (4), grid24 needs 3 groups (9), random3000 3 (11)"),
    ("no progress", CSRC + "agg.cpp", r"if \(now >= remaining\)",
     [MODEL], "the host loop ends: the count falls after every group of rounds on every case (the error branch needs a pattern the census refuses)"),
    ("a row without an aggregate", CSRC + "agg.cpp", r"if \(unassigned != 0 \|\| naggs < 1 \|\| naggs > m\)",
     [MODEL], "never taken: every row of every case is assigned after B (the branch reports and does not loop)"),
    ("kAggLaneGroup", CSRC + "agg.hpp", r"constexpr int kAggLaneGroup = 1;",
     [MODEL, STRIDE], "lanes per row of the neighbourhood pass; max is exact, so every case gives the model's arrays whatever the group"),
    ("four entries a step", CSRC + "k_agg.hip", r"for \(int p = lo \+ l; p < hi; p \+= 4 \* G\) \{",
     [MODEL], "rows of 0 entries (empties), 1 (lonely), 2 and 3 (path), 4 and 5 (grid24), 9 (fem), 27 (grid27), 130 and 300 (k130, star): a "
              "last step of one to four entries"),
    ("a root's row is not read", CSRC + "k_agg.hip", r"if \(best != kAggRoot\) best = neighbourhood_max<G>",
     [MODEL], "from the second round on (every case of two rounds or more)"),
    ("decided rows skip the second pass", CSRC + "k_agg.hip", r"if \(mine == kAggRoot \|\| mine == kAggOut\) continue;",
     [MODEL], "from the second round on"),
    ("census grid", CSRC + SHARED, r"return grid > static_cast<unsigned>\(kCooCheckBlocks\) \? static_cast<unsigned>\(kCooCheckBlocks\) : grid;",
     [STRIDE, CONTRACT], "one count slot per wavefront of at most 1 024 workgroups"),
    ("census grid: the rounds' calls", CSRC + "k_agg.hip", r"dim3\(census_grid_for\(m, kThreads / kAggLaneGroup\)\)",
     [STRIDE, MODEL], "both passes of a round take the shared census grid"),
    ("row loops of the rounds", CSRC + "k_agg.hip", r"r < m; r \+= stride\) \{",
     [STRIDE], "grid-striding rows (the stride test: 155 184 rows over 64 workgroups)"),
    ("kMaxGridBlocks (grid striding)", CSRC + SHARED, r"const long long cap = max_grid_blocks\(\);",
     [STRIDE], "every kernel of the two entries strides over the work beyond max_grid_blocks() workgroups"),
    ("kAggPerLane", CSRC + "agg.hpp", r"constexpr int kAggPerLane = 1;",
     [VALUES, STRIDE], "aggregates per lane of the norms pass"),
    ("kAggWaveChunk", CSRC + "agg.hpp", r"constexpr int kAggWaveChunk = 64 \* kAggPerLane;",
     [VALUES, STRIDE], "64 aggregates per wavefront: cases of fewer (star, k130, the bands, grid27) leave wavefronts without work, grid24 (84) fills one and starts another"),
    ("kAggTile", CSRC + "agg.hpp", r"constexpr int kAggTile = 4 \* kAggWaveChunk;",
     [STRIDE], "256 aggregates per workgroup: path (543) and random3000 (455) are several tiles with a short last one; the stride test has more than 70 000 aggregates, more tiles than the 64 workgroups it is given"),
    ("tile loop of the norms", CSRC + "k_agg.hip", r"for \(long long tile = blockIdx\.x; tile < ntiles; tile \+= gridDim\.x\) \{ // \(block-uniform\)",
     [STRIDE], "the square roots walk sum_runs' own tiles"),
    ("kCooLongRun", CSRC + "coo.hpp", r"constexpr int kCooLongRun = 64;",
     [VALUES], "aggregates of more than 64 rows are summed by a wavefront (star: 300, k130: 130), the others by one lane"),
    ("a zero norm", CSRC + "k_agg.hip", r"return d == 0\.0 \? 0\.0 :",
     [VALUES], "+0.0 in P where the aggregate's b is all zero"),
    ("an aggregate outside [0, naggs)", CSRC + "k_agg.hip", r"if \(static_cast<unsigned>\(a\) >= static_cast<unsigned>\(naggs\)\) return 0\.0;",
     [VALUES_CONTRACT], "+0.0 for a crafted agg"),
    ("b == NULL", CSRC + "k_agg.hip", r"b != nullptr \? b\[i\] : 1\.0",
     [VALUES], "all ones"),
    ("r_value == NULL", CSRC + "k_agg.hip", r"if \(r_value != nullptr\) \{",
     [VALUES], "R's values are optional"),
    ("kEntryAlign", CSRC + HELPERS, r"constexpr size_t kEntryAlign = 256;",
     [MODEL], "workspace parts are padded to 256 B (row counts that are no multiple of 64: most cases)"),
    ("no rows", CSRC + "agg.cpp", r"if \(m == 0\) \{",
     [MODEL], "m == 0: no aggregate, nothing is read or allocated"),
    ("no rows: the values", CSRC + "agg.cpp", r"if \(m == 0\) return kOk;",
     [VALUES], "nothing to launch"),
    ("int32 block arithmetic", CSRC + HELPERS, r"inline bool too_large\(long long v\) \{ return v > INT_MAX - \(1 << 16\); \}",
     [CONTRACT, VALUES_CONTRACT], "m, nnz or naggs beyond this: SPMV_ACC_ERR_TOO_LARGE, as the other entries"),
    ("the census is shared", CSRC + "agg.cpp", r"pattern_census\(st, kEntry, ",
     [CONTRACT, MODEL], "the refusals and their text are entry_helpers.hpp's, the same for the four entries"),
]


def test_agg_size_rules_name_their_tests():
    gpu_tests = open(os.path.join(ROOT, "tests", "test_gpu_agg.py")).read()
    defined = set(re.findall(r"^def (test_\w+)\(", gpu_tests, flags=re.M))
    for name, path, pattern, tests, what in AGG_SIZE_RULES:
        assert re.search(pattern, open(os.path.join(ROOT, path)).read()), f"{name}: no longer matches {path}: {pattern}"
        assert tests and what
        for t in tests:
            assert t in defined, f"{name}: names {t}, which is not a test of tests/test_gpu_agg.py"
    # every named constant of the new files is registered above (tests/size_thresholds.py does not scan them)
    registered = " ".join(r[0] + " " + r[2] for r in AGG_SIZE_RULES)
    found = 0
    for f in NEW_SOURCES:
        for k in re.findall(r"constexpr\s+[\w:<> ]+?\s+(k[A-Z]\w*)\s*=", open(os.path.join(ROOT, CSRC, f)).read()):
            found += 1
            assert k in registered, f"{f}: constant {k} is not in AGG_SIZE_RULES"
    assert found == 7
    header = open(os.path.join(ROOT, CSRC, "agg.hpp")).read()
    assert f"constexpr int kAggRoundsPerRead = {ROUNDS_PER_READ};" in header and f"constexpr int kAggLaneGroup = {LANE_GROUP};" in header
    assert f"constexpr int kAggPerLane = {PER_LANE};" in header and LONG_RUN == 64
    kernels = open(os.path.join(ROOT, CSRC, "k_agg.hip")).read()
    assert kernels.count("tile += gridDim.x") == 1 and kernels.count("+= stride)") == 7  # every loop over work is one of the registered forms


PROTOTYPES = (
    r"int spmv_acc_csr_aggregate\(int m, int nnz, const int \*d_rowptr, const int \*d_colindex,\s*"
    r"int \*d_agg, int \*d_agg_rows, int \*d_agg_ptr, int \*h_naggs\);",
    r"int spmv_acc_csr_tentative_values\(int m, int naggs, const int \*d_agg, const int \*d_agg_ptr, const int \*d_agg_rows,\s*"
    r"const double \*d_b, double \*d_p_value, double \*d_r_value, double \*d_bc\);",
)


def test_agg_entries_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "spmv_acc.h")).read()
    for proto in PROTOTYPES:
        assert re.search(proto, header), proto
    for entry in ("1", "2"):
        block = re.search(r"/\* ---- aggregation coarsening, " + entry + r".*?\*/", header, flags=re.S)
        assert block, entry
        for word in ("replaces: nothing in the reference", "COST", "CHECKS", "CANNOT CHECK"):
            assert word in block.group(0), (entry, word)
    assert "value threshold is out of scope" in header
    # the header declares exactly what the package lists
    declared = set(re.findall(r"\b(sparse_spmv|spmv_acc_[a-z_0-9]+)\s*\(", header))
    assert declared == set(spmv_acc_amd.C_ABI_SYMBOLS), declared ^ set(spmv_acc_amd.C_ABI_SYMBOLS)
    lib = spmv_acc_amd.load_library()
    for s in ("spmv_acc_csr_aggregate", "spmv_acc_csr_tentative_values"):
        assert s in spmv_acc_amd.C_ABI_SYMBOLS and hasattr(lib, s), s
    assert lib.spmv_acc_csr_aggregate.restype is ctypes.c_int and lib.spmv_acc_csr_tentative_values.restype is ctypes.c_int
    assert len(lib.spmv_acc_csr_aggregate.argtypes) == 8 and len(lib.spmv_acc_csr_tentative_values.argtypes) == 9
    for f in ("csr_aggregate", "csr_tentative", "csr_tentative_values"):
        assert callable(getattr(spmv_acc_amd, f))
    assert "csr_spgemm(" in spmv_acc_amd.csr_aggregate.__doc__ and "csr_tentative(" in spmv_acc_amd.csr_aggregate.__doc__
    for f in ("k_agg.hip", "agg.cpp"):  # both builds compile the new files
        assert f in open(os.path.join(ROOT, CSRC, "Makefile")).read() and f in open(os.path.join(ROOT, "CMakeLists.txt")).read(), f
    assert "agg.hpp" in open(os.path.join(ROOT, CSRC, "Makefile")).read()
    assert " k_agg " in open(os.path.join(ROOT, "tools", "resource_usage.sh")).read()  # (test_gs_host holds k_gs to the last place)
    assert "spmv_acc_csr_aggregate" in open(os.path.join(ROOT, "README.md")).read()


BAD, TOO_LARGE = 2, 4  # SPMV_ACC_ERR_BAD_ARGUMENT, SPMV_ACC_ERR_TOO_LARGE


def test_bad_arguments_are_refused_without_a_gpu():
    """The C entries check their arguments before they touch the device: the error codes come back on a machine without one."""
    lib = spmv_acc_amd.load_library()
    one = 8  # (never dereferenced: a non-null pointer value)
    h_n = ctypes.c_int(-5)

    def aggregate(m=4, nnz=8, rp=one, ci=one, agg=one, rows=one, ptr=one, hn=ctypes.byref(h_n)):
        return lib.spmv_acc_csr_aggregate(m, nnz, rp, ci, agg, rows, ptr, hn)

    for neg in ("m", "nnz"):
        assert aggregate(**{neg: -1}) == BAD, neg
        assert b"spmv_acc_csr_aggregate: negative" in lib.spmv_acc_last_error_string()
    for null in ("rp", "ci", "agg", "rows", "ptr", "hn"):
        assert aggregate(**{null: None}) == BAD, null
        assert b"spmv_acc_csr_aggregate: null" in lib.spmv_acc_last_error_string(), null
    for big in (2 ** 31 - 1, 2 ** 31 - 2 ** 16):
        for which in ("m", "nnz"):
            assert aggregate(**{which: big}) == TOO_LARGE, which
            assert b"spmv_acc_csr_aggregate:" in lib.spmv_acc_last_error_string()
    assert aggregate(m=0, nnz=3) == BAD and b"without rows" in lib.spmv_acc_last_error_string()
    assert h_n.value == -5
    assert aggregate(m=0, nnz=0, rp=None, ci=None, agg=None, rows=None, ptr=None) == 0  # no rows: no aggregate, the device is not touched
    assert h_n.value == 0 and lib.spmv_acc_last_error() == 0

    # the values pass: b, p_value, r_value of m = 4 doubles (32 B) and bc of naggs = 2 (16 B) at distinct places
    b_at, p_at, r_at, bc_at = 1 << 20, 2 << 20, 3 << 20, 4 << 20

    def values(m=4, naggs=2, agg=one, ptr=one, rows=one, b=b_at, p=p_at, r=r_at, bc=bc_at):
        return lib.spmv_acc_csr_tentative_values(m, naggs, agg, ptr, rows, b, p, r, bc)

    for neg in ("m", "naggs"):
        assert values(**{neg: -1}) == BAD, neg
        assert b"spmv_acc_csr_tentative_values: negative" in lib.spmv_acc_last_error_string()
    for null in ("agg", "ptr", "rows", "p", "bc"):
        assert values(**{null: None}) == BAD, null
        assert b"spmv_acc_csr_tentative_values: null" in lib.spmv_acc_last_error_string(), null
    for big in (2 ** 31 - 1, 2 ** 31 - 2 ** 16):
        for which in ("m", "naggs"):
            assert values(**{which: big}) == TOO_LARGE, which
            assert b"spmv_acc_csr_tentative_values:" in lib.spmv_acc_last_error_string()
    for bad in (dict(b=p_at), dict(b=p_at + 24), dict(b=p_at - 24), dict(b=r_at + 8), dict(b=bc_at + 8), dict(b=bc_at - 24)):
        assert values(**bad) == BAD and b"b overlaps an output" in lib.spmv_acc_last_error_string(), bad
    for bad in (dict(bc=p_at), dict(bc=p_at + 24), dict(bc=p_at - 8), dict(bc=r_at + 16), dict(r=p_at), dict(r=p_at + 24), dict(p=r_at - 24)):
        assert values(**bad) == BAD and b"overlap" in lib.spmv_acc_last_error_string(), bad
    # nothing to do: no rows
    assert values(m=0, naggs=0, agg=None, ptr=None, rows=None, b=None, p=None, r=None, bc=None) == 0
    assert lib.spmv_acc_last_error() == 0
    lib.spmv_acc_clear_error()


def test_wrappers_refuse_bad_arguments():
    E = spmv_acc_amd.SpmvAccError
    m, nnz, naggs = 10, 30, 3

    def aggregate(match, mm=m, rp=_i(m + 1), ci=_i(nnz)):
        with pytest.raises(E, match=match):
            spmv_acc_amd.csr_aggregate(mm, rp, ci)

    aggregate("not on the GPU", ci=_i(nnz, cuda=False))
    aggregate("dtype", rp=_FakeTensor(m + 1, dtype="torch.int64"))
    aggregate("dtype", ci=_f(nnz))
    aggregate("not contiguous", ci=_i(nnz, contiguous=False))
    aggregate("elements", rp=_i(m))
    aggregate("on cuda:1", ci=_i(nnz, device="cuda:1"))
    aggregate("torch tensor", rp=None)
    aggregate("torch tensor", ci=[0] * nnz)
    aggregate("negative", mm=-1)

    good = dict(agg=_i(m), ptr=_i(naggs + 1), rows=_i(m), b=_f(m), p=_f(m), r=_f(m), bc=_f(naggs))

    def values(match, mm=m, **bad):
        a = dict(good, **bad)
        with pytest.raises(E, match=match):
            spmv_acc_amd.csr_tentative_values(mm, a["agg"], a["ptr"], a["rows"], a["b"], a["p"], a["r"], a["bc"])

    values("not on the GPU", agg=_i(m, cuda=False))
    values("not on the GPU", b=_f(m, cuda=False))
    values("not on the GPU", r=_f(m, cuda=False))
    values("dtype", agg=_f(m))
    values("dtype", ptr=_FakeTensor(naggs + 1, dtype="torch.int64"))
    values("dtype", b=_i(m))
    values("dtype", p=_i(m))
    values("dtype", bc=_FakeTensor(naggs, dtype="torch.float32"))
    values("not contiguous", p=_f(m, contiguous=False))
    values("not contiguous", rows=_i(m, contiguous=False))
    values("elements", b=_f(m - 1))
    values("elements", p=_f(m - 1))
    values("elements", r=_f(m - 1))
    values("elements", ptr=_i(0))
    values("as many", agg=_i(m - 1))
    values("as many", agg=_i(m + 1))
    values("as many", rows=_i(m + 1))
    values("as many", bc=_f(naggs + 1))
    values("as many", bc=_f(naggs - 1))
    values("on cuda:1", bc=_f(naggs, device="cuda:1"))
    values("torch tensor", agg=None)
    values("torch tensor", p=None)
    values("torch tensor", bc=[0.0] * naggs)
    values("torch tensor", b=[1.0] * m)
    values("torch tensor", r=3.0)
    values("negative", mm=-1)
    with pytest.raises(E, match="torch tensor"):
        spmv_acc_amd.csr_tentative(m, None, _i(naggs + 1), _i(m))
    with pytest.raises(E, match="negative"):
        spmv_acc_amd.csr_tentative(-1, _i(m), _i(naggs + 1), _i(m))


def test_agg_entries_keep_no_state():
    """As test_gs_entries_keep_no_state: the engine file neither finds nor makes a plan, counts no plan work, reads no tunable and keeps nothing
    static; the aggregation's one allocation is freed on every way out; the values pass is launch-only."""
    src = open(os.path.join(ROOT, CSRC, "agg.cpp")).read()
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
    for launch in ("pattern_census", "launch_agg_init", "launch_agg_max", "launch_agg_decide", "launch_agg_flags", "launch_coo_scan",
                   "launch_agg_assign_roots", "launch_agg_assign_rest", "launch_gs_keys", "launch_coo_sort", "launch_gs_color_ptr"):
        assert launch in after, launch
    bare = [ln.strip() for ln in after.splitlines() if re.search(r"\breturn\b(?! leave\()", ln)]
    # (the one way out that may skip leave(): the scratch query before the allocation)
    assert bare == ['return entry_error(kEntry, kErrHip, "scan / radix sort workspace query failed");'], bare
    # the host loop can end: one comparison guards every further group of rounds
    loop = after.split("while (remaining != 0) {")[1].split("\n  }\n")[0]
    assert "if (now >= remaining)" in loop and "return leave(entry_error(kEntry, kErrHip" in loop and "remaining = now;" in loop
    assert after.index("pattern_census(") < after.index("launch_agg_init(")  # the census is judged before anything is written
    assert 'pattern_census(st, kEntry, m, nnz, d_rowptr, d_colindex, d_slots, "aggregate the pattern of A + A^T instead", ' in after
    assert "*h_naggs = naggs;" in after.split("launch_gs_color_ptr")[1]  # (written last, once everything else has run)
    values = code.split("int run_csr_tentative_values")[1]
    assert "hipMalloc" not in values and "Synchronize" not in values and "hipMemcpy" not in values and "hipMemset" not in values  # launch-only
    assert "plan_work_allowed" not in values and values.count("launch_agg_norms(") == 1 and values.count("launch_agg_values(") == 1
    assert values.index("launch_agg_norms(") < values.index("launch_agg_values(") and values.count("launch_agg_") == 2
    assert values.index("overlaps an output") < values.index("launch_agg_norms(")  # refused before any launch
    kernels = open(os.path.join(ROOT, CSRC, "k_agg.hip")).read()
    assert "atomic" not in re.sub(r"//[^\n]*", "", kernels).lower() and "__syncthreads" not in kernels and "while (" not in re.sub(r"//[^\n]*", "", kernels)


KERNELS = ("agg_max_kernel", "agg_decide_kernel", "agg_init_kernel", "agg_flags_kernel", "agg_assign_roots_kernel", "agg_assign_rest_kernel",
           "agg_norms_kernel", "agg_values_kernel")
# as recorded in k_agg.hip's header comment
RECORDED_VGPRS = dict(agg_max_kernel=26, agg_decide_kernel=36, agg_init_kernel=7, agg_flags_kernel=8, agg_assign_roots_kernel=12,
                      agg_assign_rest_kernel=11, agg_norms_kernel=32, agg_values_kernel=18)


def test_agg_kernels_fit_their_register_budget(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_table

    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-DKERNEL_STRATEGY_ADAPTIVE",
                        "-I" + os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
                        os.path.join(ROOT, CSRC, "k_agg.hip"), "-o", str(tmp_path / "k_agg.o")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    header = open(os.path.join(ROOT, CSRC, "k_agg.hip")).read().split("#include")[0]
    rows = [k for k in resource_table.parse(r.stderr) if "rocprim" not in k["name"]]
    for k in rows:
        k["name"] = re.sub(r"<.*", "", k["name"])  # (the two passes of a round are instances of their lane group)
    assert sorted(k["name"] for k in rows) == sorted(KERNELS), sorted(k["name"] for k in rows)
    for k in rows:
        assert k["scratch"] == 0 and k["agprs"] == 0 and k["vgprs"] <= 64 and k["occupancy"] >= 8, k
        want = RECORDED_VGPRS[k["name"]]
        assert re.search(k["name"] + r", " + str(want) + r"\b", header), (k["name"], "the count recorded in the header comment")
        assert k["vgprs"] <= want + 4, (k, "grew past the count recorded in k_agg.hip (a few registers of compiler drift are allowed)")


# ---- the aggregates (agg.hpp), in numpy: the GPU suite's reference ---------------------------------------------------------------------------
def agg_outputs(m, agg):
    """(agg, agg_rows, agg_ptr of m + 1 entries, naggs) as the entry returns them, from the aggregate of every row."""
    agg = np.asarray(agg, dtype=np.int32)
    naggs = int(agg.max()) + 1 if m else 0
    agg_rows = np.argsort(agg, kind="stable").astype(np.int32)
    agg_ptr = np.searchsorted(agg[agg_rows], np.arange(m + 1), side="left").astype(np.int32)  # (m beyond the last aggregate)
    return agg, agg_rows, agg_ptr, naggs


def assign(m, rp, ci, root):
    """Ids and the two assignment passes, from the roots."""
    row = np.repeat(np.arange(m), np.diff(rp))
    ids = np.cumsum(root) - 1  # ascending row order
    first = np.where(root, ids, -1)
    near = root[ci] & ~root[row] & (ci != row)
    assert np.unique(row[near]).size == np.count_nonzero(near)  # at most one root neighbour
    first[row[near]] = ids[ci[near]]
    agg = first.copy()
    rest = (first[row] < 0) & (first[ci] >= 0)
    best = np.full(m, np.iinfo(np.int64).max)
    np.minimum.at(best, row[rest], first[ci[rest]])  # B reads only A's results
    agg[first < 0] = best[first < 0]
    assert m == 0 or agg.max() < m, "a row without an aggregate"
    return agg


def host_roots(m, rp, ci):
    """The roots by the definition: the rows in descending priority, a root where no root already chosen lies within distance 2."""
    root, blocked = np.zeros(m, dtype=bool), np.zeros(m, dtype=bool)
    for v in np.argsort(priorities(m))[::-1]:
        if blocked[v]:
            continue
        root[v] = blocked[v] = True
        nb = ci[rp[v]:rp[v + 1]]
        blocked[nb] = True
        for u in nb:
            blocked[ci[rp[u]:rp[u + 1]]] = True
    return root


def host_csr_aggregate(m, rp, ci):
    """The definition: the sequential greedy roots, then the ids and the assignment passes A and B."""
    return agg_outputs(m, assign(m, rp, ci, host_roots(m, rp, ci)))


def host_csr_aggregate_rounds(m, rp, ci):
    """The round form: (outputs, rounds).  key: ROOT, OUT, or priority + 1 while undecided; T1 = max key over the closed neighbourhood, T2 = max T1."""
    row = np.repeat(np.arange(m), np.diff(rp))
    key = priorities(m) + np.uint64(1)
    rounds = 0
    while True:
        undecided = (key != KEY_ROOT) & (key != KEY_OUT)
        if not undecided.any():
            break
        t1 = key.copy()
        np.maximum.at(t1, row, key[ci])
        t2 = t1.copy()
        np.maximum.at(t2, row, t1[ci])
        new = key.copy()
        new[undecided & (t2 == KEY_ROOT)] = KEY_OUT
        new[undecided & (t2 == key)] = KEY_ROOT
        assert np.count_nonzero((new != KEY_ROOT) & (new != KEY_OUT)) < np.count_nonzero(undecided)
        key = new
        rounds += 1
    return agg_outputs(m, assign(m, rp, ci, key == KEY_ROOT)), rounds


# ---- the tentative values (agg.hpp), in numpy, bit for bit: the GPU suite's reference -------------------------------------------------------------
def host_tentative_values(m, naggs, agg, agg_ptr, agg_rows, b=None):
    """(p_value, r_value, bc).  The maps are taken as they are: runs clamped to [0, m], rows and aggregates out of range give +0.0."""
    agg, agg_ptr, agg_rows = (np.asarray(a, dtype=np.int64) for a in (agg, agg_ptr, agg_rows))
    bb = np.ones(m) if b is None else np.asarray(b, dtype=np.float64)
    with np.errstate(all="ignore"):
        s = coo_sum_model(agg_rows, agg_ptr[:naggs + 1], bb * bb)  # every square rounded on its own; coo.hpp's order
        bc = np.sqrt(s)
        ok = (agg >= 0) & (agg < naggs)
        d = bc[np.where(ok, agg, 0)] if naggs else np.zeros(m)
        p = np.where(ok & (d != 0.0), bb / np.where(ok & (d != 0.0), d, 1.0), 0.0)
        inside = (agg_rows >= 0) & (agg_rows < m)
        r = np.where(inside, p[np.where(inside, agg_rows, 0)], 0.0)
    return p, r, bc


# ---- the cases of the GPU suite, made once ----------------------------------------------------------------------------------------------------
def grid5_pairs(nx, ny):
    idx = np.arange(nx * ny).reshape(nx, ny)
    pairs = [(int(v), int(v)) for v in idx.reshape(-1)]
    for a, c in ((idx[:-1, :], idx[1:, :]), (idx[:, :-1], idx[:, 1:])):
        for p, q in zip(a.reshape(-1).tolist(), c.reshape(-1).tolist()):
            pairs += [(p, q), (q, p)]
    return pairs


def grid5_matrix(n):
    """The five-point Laplacian on an n x n grid, values 4 and -1: (m, (rowptr, colindex, value))."""
    rp, ci, _ = csr_from_pattern(n * n, grid5_pairs(n, n), np.random.default_rng(0))
    row = np.repeat(np.arange(n * n), np.diff(rp))
    return n * n, (rp, ci, np.where(ci == row, 4.0, -1.0))


# (tag, rows, aggregates, rounds): from a CPU run of the two host models (test_the_cases_and_their_aggregates holds the cases to it)
TABLE = (("grid24", 576, 84, 9), ("star", 300, 1, 2), ("k130", 130, 1, 2), ("fem", 450, 41, 9), ("grid7", 504, 55, 8), ("grid27", 504, 16, 6),
         ("path", 2000, 543, 8), ("band25", 200, 4, 4), ("lonely", 150, 113, 5), ("empties", 100, 64, 4), ("isolated", 120, 71, 5),
         ("random3000", 3000, 455, 11))
TAGS = tuple(GS_TAGS) + ("grid24", "isolated", "random3000")


def _cases():
    for tag in GS_TAGS:
        m, (rp, ci, _) = gs_cases()[tag]
        yield tag, m, (rp, ci)
    m, (rp, ci, _) = grid5_matrix(24)
    yield "grid24", m, (rp, ci)
    rng = np.random.default_rng(2031)
    # isolated rows: every third row holds only its diagonal, every seventh nothing at all; the others form a chain
    chain = [v for v in range(120) if v % 3 and v % 7]
    pairs = [(v, v) for v in range(120) if v % 7] + [(p, q) for p, q in zip(chain, chain[1:])] + [(q, p) for p, q in zip(chain, chain[1:])]
    rp, ci, _ = csr_from_pattern(120, pairs, rng)
    yield "isolated", 120, (rp, ci)
    i, j = rng.integers(0, 3000, 7000), rng.integers(0, 3000, 7000)
    pairs = list(zip(i.tolist(), j.tolist())) + list(zip(j.tolist(), i.tolist())) + [(v, v) for v in range(0, 3000, 2)]
    rp, ci, _ = csr_from_pattern(3000, pairs, rng)
    yield "random3000", 3000, (rp, ci)


@functools.lru_cache(maxsize=None)
def cases():
    """tag -> (m, (rowptr, colindex)); made once and shared, nothing changes them."""
    return {tag: (m, A) for tag, m, A in _cases()}


@functools.lru_cache(maxsize=None)
def aggregates(tag):
    """(agg, agg_rows, agg_ptr, naggs) of the host for a case, computed once."""
    m, (rp, ci) = cases()[tag]
    return host_csr_aggregate(m, rp, ci)


def adjacency(m, rp, ci):
    adj = np.zeros((m, m), dtype=bool)
    row = np.repeat(np.arange(m), np.diff(rp))
    adj[row, ci] = True
    adj[np.arange(m), np.arange(m)] = False
    return adj


def check_invariants(m, rp, ci, roots, agg, agg_rows, agg_ptr, naggs):
    """What a distance-2 maximal independent set (`roots`: its rows, ascending) and its aggregates are, from the dense adjacency alone: no
    model's choice is compared, only the properties any valid answer has."""
    adj = adjacency(m, rp, ci).astype(np.float32)
    member = np.zeros((naggs, m), dtype=np.float32)
    member[agg, np.arange(m)] = 1.0
    assert roots.size == naggs and np.all(np.diff(roots) > 0) and np.array_equal(agg[roots], np.arange(naggs))  # ids in ascending row order
    ball1 = adj[roots] > 0
    ball1[np.arange(naggs), roots] = True
    ball2 = (ball1.astype(np.float32) @ adj > 0) | ball1
    assert np.array_equal(ball2[:, roots], np.eye(naggs, dtype=bool))  # roots are pairwise at distance >= 3
    assert ball2.any(axis=0).all()  # no row could be added as a root: every row has a root within distance 2
    # every row reaches its aggregate's root in at most two steps through members of that aggregate
    near = ball1 & (member > 0)  # [a, u]: u is the root of a or a member next to it
    via = near.astype(np.float32) @ adj > 0
    assert np.all(near[agg, np.arange(m)] | via[agg, np.arange(m)])
    # the stable sort
    assert np.array_equal(np.sort(agg_rows), np.arange(m)) and np.all(np.diff(agg[agg_rows]) >= 0)
    assert agg_ptr.size == m + 1 and agg_ptr[0] == 0 and np.all(agg_ptr[naggs:] == m) and np.all(np.diff(agg_ptr[:naggs + 1]) > 0)
    for a in range(naggs):
        rows = agg_rows[agg_ptr[a]:agg_ptr[a + 1]]
        assert np.all(agg[rows] == a) and np.all(np.diff(rows) > 0), a  # ascending rows inside an aggregate


def test_the_cases_and_their_aggregates():
    """Every case is what the entry demands; the sequential model and the round model give the same arrays; the invariants hold; rows,
    aggregates and rounds are the table's."""
    assert set(TAGS) == set(cases()) and len(TAGS) == len(set(TAGS))
    counted = {}
    for tag in TAGS:
        m, (rp, ci) = cases()[tag]
        assert rp.size == m + 1 and rp[0] == 0 and rp[m] == ci.size and np.all(np.diff(rp) >= 0), tag
        row = np.repeat(np.arange(m), np.diff(rp))
        pattern = set(zip(row.tolist(), ci.tolist()))
        assert all((j, i) in pattern for i, j in pattern) and len(pattern) == ci.size, tag
        inner = np.ones(ci.size, dtype=bool)
        inner[rp[:-1][np.diff(rp) > 0]] = False
        assert ci.size < 2 or np.all(np.diff(ci.astype(np.int64))[inner[1:]] > 0), tag
        agg, agg_rows, agg_ptr, naggs = aggregates(tag)
        (r_agg, r_rows, r_ptr, r_naggs), rounds = host_csr_aggregate_rounds(m, rp, ci)
        assert np.array_equal(agg, r_agg) and np.array_equal(agg_rows, r_rows) and np.array_equal(agg_ptr, r_ptr) and naggs == r_naggs, tag
        if m:
            check_invariants(m, rp, ci, np.flatnonzero(host_roots(m, rp, ci)), agg, agg_rows, agg_ptr, naggs)
        counted[tag] = (m, naggs, rounds)
    for tag, rows, naggs, rounds in TABLE:
        assert counted[tag] == (rows, naggs, rounds), (tag, counted[tag])
    assert counted["none"] == (0, 0, 0) and counted["one"] == (1, 1, 1) and counted["one_empty"] == (1, 1, 1)
    # the groups of rounds the GPU cases cross (AGG_SIZE_RULES kAggRoundsPerRead): inside the first, and more than one
    groups = {tag: -(-c[2] // ROUNDS_PER_READ) for tag, c in counted.items()}
    assert groups["star"] == 1 and counted["star"][2] < ROUNDS_PER_READ and groups["grid24"] == 3 and max(groups.values()) >= 3
    # isolated rows are roots, aggregates of one row
    m, (rp, ci) = cases()["isolated"]
    alone = np.flatnonzero(np.array([np.all(ci[rp[v]:rp[v + 1]] == v) for v in range(m)]))
    agg, agg_rows, agg_ptr, naggs = aggregates("isolated")
    assert alone.size >= 40 and np.all(np.bincount(agg, minlength=naggs)[agg[alone]] == 1) and np.any(np.diff(rp) == 0)
    # aggregates on both sides of kCooLongRun
    sizes = np.concatenate([np.bincount(aggregates(t)[0]) for t in TAGS if cases()[t][0]])
    assert sizes.min() == 1 and np.any(sizes > LONG_RUN) and np.any((sizes > 1) & (sizes <= LONG_RUN))


def test_the_round_form_on_further_patterns():
    """Random symmetric patterns of several densities: the two models agree (the statement the device form rests on)."""
    rng = np.random.default_rng(9)
    for m, edges in ((50, 30), (200, 150), (200, 600), (500, 3000), (64, 2000)):
        i, j = rng.integers(0, m, edges), rng.integers(0, m, edges)
        rp, ci, _ = csr_from_pattern(m, list(zip(i.tolist(), j.tolist())) + list(zip(j.tolist(), i.tolist())), rng)
        want = host_csr_aggregate(m, rp, ci)
        got, rounds = host_csr_aggregate_rounds(m, rp, ci)
        assert all(np.array_equal(a, b) for a, b in zip(want[:3], got[:3])) and want[3] == got[3] and rounds >= 1, (m, edges)
        check_invariants(m, rp, ci, np.flatnonzero(host_roots(m, rp, ci)), *want)


def test_host_tentative_values():
    """Bit for bit the documented order (test_gs_host row_sum: one lane from the first term up to kCooLongRun rows, 64 lanes and the balanced
    tree beyond), and the independent statement: the columns of P are orthonormal, P^T P = I to rounding, and P bc = b."""
    rng = np.random.default_rng(21)
    for tag in ("grid24", "star", "k130", "fem", "random3000", "isolated"):
        m, (rp, ci) = cases()[tag]
        agg, agg_rows, agg_ptr, naggs = aggregates(tag)
        b = rng.standard_normal(m) * 10.0 ** rng.integers(-3, 4, m)
        p, r, bc = host_tentative_values(m, naggs, agg, agg_ptr, agg_rows, b)
        for a in range(naggs):
            rows = agg_rows[agg_ptr[a]:agg_ptr[a + 1]]
            squares = b[rows] * b[rows]
            s = row_sum(squares, 1 if rows.size <= LONG_RUN else 64)
            assert bc[a] == np.sqrt(s), (tag, a)
            assert np.array_equal(p[rows], b[rows] / np.sqrt(s)), (tag, a)
        assert np.array_equal(r, p[agg_rows])
        P = np.zeros((m, naggs), dtype=np.longdouble)
        P[np.arange(m), agg] = p
        gram = P.T @ P
        sizes = np.bincount(agg, minlength=naggs)
        assert np.all(np.abs(gram - np.eye(naggs)) <= (sizes[:, None] + 4) * 2.0 ** -52), tag  # a norm of n squares and a division per entry
        back = np.asarray(P @ bc.astype(np.longdouble), dtype=np.float64)
        assert np.all(np.abs(back - b) <= 4 * 2.0 ** -53 * np.abs(b)), tag
        ones = host_tentative_values(m, naggs, agg, agg_ptr, agg_rows, None)
        assert np.array_equal(ones[0], 1.0 / np.sqrt(sizes.astype(np.float64))[agg]) and np.array_equal(ones[2], np.sqrt(sizes.astype(np.float64)))
    # an aggregate whose b is all zero: +0.0, no division by zero; crafted maps give the documented zeros
    m, (rp, ci) = cases()["grid24"]
    agg, agg_rows, agg_ptr, naggs = aggregates("grid24")
    b = rng.standard_normal(m)
    b[agg == 5] = 0.0
    b[agg == 6] = -0.0
    p, r, bc = host_tentative_values(m, naggs, agg, agg_ptr, agg_rows, b)
    for a in (5, 6):
        assert bc[a] == 0.0 and np.all(p[agg == a] == 0.0) and not np.signbit(p[agg == a]).any()
    bad = agg.copy()
    bad[[3, 4, 5]] = [-1, naggs, 2 ** 31 - 1]
    p2, _, _ = host_tentative_values(m, naggs, bad, agg_ptr, agg_rows, b)
    assert np.all(p2[[3, 4, 5]] == 0.0) and np.array_equal(np.delete(p2, [3, 4, 5]), np.delete(p, [3, 4, 5]))
