"""CPU side of the device CSR sparse add C = alpha * A + beta * B (no GPU): the C ABI declares and exports the two entries, they and the Python
wrappers refuse bad arguments before any launch, the compiled kernels use no scratch, no AGPR, no atomic and no fused multiply-add and fit 64
VGPRs, every size-selected branch of the new code names the GPU tests that cross it, the engine file stays stateless, and the definition of the
sum -- the sorted union, the (ia, ib) map, each product rounded, an absent side left out -- is restated here in numpy (host_csr_add, exported to
the GPU suite as its reference) and checked bit for bit against a dense sum and, where it is installed, against scipy.sparse."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import spmv_acc_amd
from test_coo_host import HELPERS, SHARED, _FakeTensor, _f, _i

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "spmv_acc_amd/csrc/"
NEW_SOURCES = ("csr_add.hpp", "k_csr_add.hip", "csr_add.cpp")
GPU = "test_sum_is_the_host_model"
STRIDE = "test_csr_add_grid_stride_at_test_size"

# (rule, file, regex that must match the source, GPU tests of tests/test_gpu_csr_add.py that cross it at test size, what it selects)
CSR_ADD_SIZE_RULES = [
    ("kCsrAddPerLane", CSRC + "csr_add.hpp", r"constexpr int kCsrAddPerLane = 4;",
     [GPU, "test_special_values"], "values pass: C entries per lane (sums of fewer than 4 * 64 entries leave lanes and steps empty: one_by_one, wide)"),
    ("kCsrAddWaveChunk", CSRC + "csr_add.hpp", r"constexpr int kCsrAddWaveChunk = 64 \* kCsrAddPerLane;",
     [GPU], "entries per wavefront: 256; the last wavefront of a sum is partly empty"),
    ("kCsrAddTile", CSRC + "csr_add.hpp", r"constexpr int kCsrAddTile = 4 \* kCsrAddWaveChunk;",
     [GPU, STRIDE], "entries per workgroup of the values pass: 1 024 (hub_rows: over 600 tiles; same_pattern: 27)"),
    ("kCsrAddRankTile", CSRC + "csr_add.hpp", r"constexpr int kCsrAddRankTile = 256;",
     [GPU, STRIDE], "non-zeros per workgroup of the census, the match and the two places: 256, a wavefront 64 consecutive ones -- inside one row "
                    "(hub_rows: no row between the ends), across rows, across empty rows (empties)"),
    ("tile loop of the census", CSRC + "k_csr_add.hip",
     r"for \(long long tile = blockIdx\.x; tile < ntiles; tile \+= gridDim\.x\) \{ // \(block-uniform\)\n    const long long base = tile \* kCsrAddRankTile \+ static_cast<long long>\(wave\) \* kWave;\n    if \(base >= nnz\) continue;",
     [STRIDE], "blocks stride over the tiles of non-zeros beyond the grid, at most kCooCheckBlocks of them (large: 800 000 non-zeros, 3 125 tiles)"),
    ("row loop of the census", CSRC + "k_csr_add.hip", r"r < m; r \+= stride\)",
     [STRIDE, "test_csr_add_contract"], "rowptr extents, one row per lane, striding (large: 200 000 rows)"),
    ("census grid", CSRC + SHARED, r"return grid > static_cast<unsigned>\(kCooCheckBlocks\) \? static_cast<unsigned>\(kCooCheckBlocks\) : grid;",
     [GPU, "test_csr_add_contract"], "one count slot per wavefront of at most 1 024 workgroups (hub_rows and large exceed them)"),
    ("census grid: the add's call", CSRC + "k_csr_add.hip", r"dim3\(census_grid_for\(items, kCsrAddRankTile\), 2\)",
     [GPU, "test_csr_add_contract"], "the census of both matrices takes the shared census grid"),
    ("tile loop of the match", CSRC + "k_csr_add.hip", r"if \(base >= items\) continue; // \(wave-uniform\)",
     [STRIDE], "nnz_a + 1 items: the closing element may open a tile of its own (nnz_a a multiple of 256)"),
    ("tile loop of A's places", CSRC + "k_csr_add.hip", r"const long long q = tile \* kCsrAddRankTile \+ threadIdx\.x;",
     [STRIDE], "blocks stride over the tiles of A's non-zeros beyond the grid"),
    ("tile loop of B's places", CSRC + "k_csr_add.hip", r"if \(base >= nnz_b\) continue; // \(wave-uniform\)",
     [STRIDE], "blocks stride over the tiles of B's non-zeros beyond the grid"),
    ("tile loop of the values pass", CSRC + "k_csr_add.hip",
     r"for \(long long tile = blockIdx\.x; tile < ntiles; tile \+= gridDim\.x\) \{ // \(block-uniform\)\n    const long long base = tile \* kCsrAddTile",
     [STRIDE], "blocks stride over the tiles of C entries beyond the grid"),
    ("row pointer pass", CSRC + "k_csr_add.hip", r"r <= m; r \+= stride\)",
     [STRIDE], "one lane per row, striding (large: 200 001 rows, 782 workgroups)"),
    ("kMaxGridBlocks (grid striding)", CSRC + SHARED, r"const long long cap = max_grid_blocks\(\);",
     [STRIDE], "every kernel of the two entries strides over the work beyond max_grid_blocks() workgroups"),
    ("kMaxGridBlocks (grid striding): the add's call", CSRC + "k_csr_add.hip", r"dim3\(grid_for\(nnz_c, kCsrAddTile\)\)",
     [STRIDE], "the launchers of the two entries take the shared grid"),
    ("absent side of an entry", CSRC + "k_csr_add.hip", r"value\[j\] = has_a \? \(has_b \? both : ta\) : \(has_b \? tb : 0\.0\);",
     [GPU, "test_special_values", "test_csr_add_contract"], "both / only A / only B / neither (a crafted map): a select, never + 0.0"),
    ("scan sizes", CSRC + "k_csr_add.hip", r"ms, 0, static_cast<size_t>\(nnz_a\) \+ 1,",
     [GPU], "the library scan over 1 (A empty) ... 800 001 match flags"),
    ("nothing to add", CSRC + "csr_add.cpp", r"if \(nnz_a == 0 && nnz_b == 0\) return nothing_to_add\(\);",
     [GPU, "test_csr_add_contract"], "both matrices empty: c_rowptr zeroed, nothing allocated"),
    ("no rows", CSRC + "csr_add.cpp", r"if \(m == 0\) \{",
     [GPU], "m == 0: c_rowptr[0] = 0, nothing is read"),
    ("one side empty", CSRC + "k_csr_add.hip", r"if \(m <= 0 \|\| nnz_b <= 0\) return;",
     [GPU], "an empty B (or A: if (nnz_a <= 0) return;) skips its place pass; the other matrix is copied, scaled"),
    ("workspace with / without the map", CSRC + "csr_add.cpp", r"const bool own_map = d_ia == nullptr && d_c_value != nullptr;",
     [GPU], "values without a caller's map: ia and ib live in the workspace (8 B per possible entry more); structure only without a map: none is written"),
    ("kEntryAlign", CSRC + HELPERS, r"constexpr size_t kEntryAlign = 256;",
     [GPU], "workspace parts are padded to 256 B (counts that are no multiple of 64: most cases)"),
    ("int32 block arithmetic", CSRC + HELPERS, r"inline bool too_large\(long long v\) \{ return v > INT_MAX - \(1 << 16\); \}",
     ["test_csr_add_contract"], "m, n, nnz_a, nnz_b or nnz_a + nnz_b beyond this: SPMV_ACC_ERR_TOO_LARGE, as the other entries"),
]


def test_csr_add_size_rules_name_their_tests():
    gpu_tests = open(os.path.join(ROOT, "tests", "test_gpu_csr_add.py")).read()
    defined = set(re.findall(r"^def (test_\w+)\(", gpu_tests, flags=re.M))
    for name, path, pattern, tests, what in CSR_ADD_SIZE_RULES:
        assert re.search(pattern, open(os.path.join(ROOT, path)).read()), f"{name}: no longer matches {path}: {pattern}"
        assert tests and what
        for t in tests:
            assert t in defined, f"{name}: names {t}, which is not a test of tests/test_gpu_csr_add.py"
    # every named constant of the new files is registered above (tests/size_thresholds.py does not scan them)
    registered = " ".join(r[0] + " " + r[2] for r in CSR_ADD_SIZE_RULES)
    found = 0
    for f in NEW_SOURCES + (HELPERS,):  # (csr_add.cpp holds none since its alignment is the shared header's)
        for k in re.findall(r"constexpr\s+[\w:<> ]+?\s+(k[A-Z]\w*)\s*=", open(os.path.join(ROOT, CSRC, f)).read()):
            found += 1
            assert k in registered, f"{f}: constant {k} is not in CSR_ADD_SIZE_RULES"
    assert found == 5


PROTOTYPES = (
    r"int spmv_acc_csr_add\(int m, int n,\s*"
    r"int nnz_a, const int \*d_a_rowptr, const int \*d_a_colindex,\s*"
    r"int nnz_b, const int \*d_b_rowptr, const int \*d_b_colindex,\s*"
    r"double alpha, const double \*d_a_value, double beta, const double \*d_b_value,\s*"
    r"int \*d_c_rowptr, int \*d_c_colindex, double \*d_c_value,\s*"
    r"int \*d_ia, int \*d_ib, int \*h_nnz\);",
    r"int spmv_acc_csr_add_values\(int nnz_c, int nnz_a, int nnz_b, const int \*d_ia, const int \*d_ib,\s*"
    r"double alpha, const double \*d_a_value, double beta, const double \*d_b_value,\s*"
    r"double \*d_c_value\);",
)


def test_csr_add_entries_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "spmv_acc.h")).read()
    for proto in PROTOTYPES:
        assert re.search(proto, header), proto
    assert header.count("replaces: nothing in the reference") >= 5  # the product's three and these two
    for entry in ("C = alpha \\* A \\+ beta \\* B, 1", "C = alpha \\* A \\+ beta \\* B, 2"):
        block = re.search(r"/\* ---- sparse add " + entry + r".*?\*/", header, flags=re.S)
        assert block and "replaces: nothing in the reference" in block.group(0) and "COST" in block.group(0), entry
    assert re.sub(r"\s*\n \* ", " ", header).lower().count("d_c_value must not overlap d_a_value or d_b_value") == 2  # said for both entries
    lib = spmv_acc_amd.load_library()
    for s in ("spmv_acc_csr_add", "spmv_acc_csr_add_values"):
        assert s in spmv_acc_amd.C_ABI_SYMBOLS and hasattr(lib, s), s
    assert lib.spmv_acc_csr_add.restype is ctypes.c_int and lib.spmv_acc_csr_add_values.restype is ctypes.c_int
    assert lib.spmv_acc_csr_add.argtypes[8] is ctypes.c_double and lib.spmv_acc_csr_add.argtypes[10] is ctypes.c_double
    assert lib.spmv_acc_csr_add_values.argtypes[5] is ctypes.c_double and lib.spmv_acc_csr_add_values.argtypes[7] is ctypes.c_double
    for f in ("csr_add", "csr_add_values"):
        assert callable(getattr(spmv_acc_amd, f))
    for f in ("k_csr_add.hip", "csr_add.cpp"):  # both builds compile the new files
        assert f in open(os.path.join(ROOT, CSRC, "Makefile")).read() and f in open(os.path.join(ROOT, "CMakeLists.txt")).read(), f
    assert "csr_add.hpp" in open(os.path.join(ROOT, CSRC, "Makefile")).read()


BAD, TOO_LARGE = 2, 4  # SPMV_ACC_ERR_BAD_ARGUMENT, SPMV_ACC_ERR_TOO_LARGE


def test_bad_arguments_are_refused_without_a_gpu():
    """The C entries check their arguments before they touch the device: the error codes come back on a machine without one."""
    lib = spmv_acc_amd.load_library()
    one = 8  # (never dereferenced: a non-null pointer value)
    h = ctypes.c_int(-5)
    add, values = lib.spmv_acc_csr_add, lib.spmv_acc_csr_add_values

    def call(m=4, n=4, nnz_a=4, arp=one, aci=one, nnz_b=4, brp=one, bci=one, alpha=1.0, av=one, beta=1.0, bv=one, crp=one, cci=one, cv=one,
             ia=one, ib=one, hn=ctypes.byref(h)):
        return add(m, n, nnz_a, arp, aci, nnz_b, brp, bci, alpha, av, beta, bv, crp, cci, cv, ia, ib, hn)

    for neg in ("m", "n"):
        assert call(**{neg: -1}) == BAD, neg
    assert b"spmv_acc_csr_add:" in lib.spmv_acc_last_error_string()
    assert call(crp=None) == BAD and call(hn=None) == BAD
    for mix in (dict(av=None), dict(bv=None), dict(cv=None), dict(av=None, bv=None), dict(av=None, cv=None), dict(bv=None, cv=None)):
        assert call(**mix) == BAD, mix  # values: all three or none
        assert b"all be given or all be NULL" in lib.spmv_acc_last_error_string()
    for mix in (dict(ia=None), dict(ib=None)):
        assert call(**mix) == BAD, mix  # the map: both or none
        assert b"both be given or both be NULL" in lib.spmv_acc_last_error_string()
    for null in ("arp", "aci", "brp", "bci", "cci"):
        for groups in (dict(), dict(av=None, bv=None, cv=None), dict(ia=None, ib=None)):
            assert call(**{null: None}, **groups) == BAD, null
            assert call(**{null: None}, nnz_a=-1, nnz_b=-1, **groups) == BAD, null  # (sizes to be read from the device: not before the pointers are checked)
        assert b"spmv_acc_csr_add: null" in lib.spmv_acc_last_error_string(), null
    in_range = 2 ** 31 - 2 ** 16 - 1  # the largest size the entries take
    for big in (2 ** 31 - 1, 2 ** 31 - 2 ** 16):
        for which in ("m", "n", "nnz_a", "nnz_b"):
            assert call(**{which: big}) == TOO_LARGE, which
            assert b"row ranges" in lib.spmv_acc_last_error_string() and b"spmv_acc_csr_add:" in lib.spmv_acc_last_error_string()
        assert values(big, 4, 4, one, one, 1.0, one, 1.0, one, one) == TOO_LARGE and values(4, big, 4, one, one, 1.0, one, 1.0, one, one) == TOO_LARGE
        assert values(4, 4, big, one, one, 1.0, one, 1.0, one, one) == TOO_LARGE
        assert b"spmv_acc_csr_add_values:" in lib.spmv_acc_last_error_string()
    # nnz_a + nnz_b, each alone in range
    for na, nb in ((in_range, 1), (1, in_range), (in_range, in_range), (2 ** 30, 2 ** 30)):
        assert call(nnz_a=na, nnz_b=nb) == TOO_LARGE, (na, nb)
        assert b"nnz_a + nnz_b" in lib.spmv_acc_last_error_string() and b"row ranges" in lib.spmv_acc_last_error_string()
    assert h.value == -5
    for neg in range(3):
        assert values(*[-1 if i == neg else 4 for i in range(3)], one, one, 1.0, one, 1.0, one, one) == BAD, neg
    for null in range(5):
        p = [None if i == null else one for i in range(5)]
        assert values(4, 4, 4, p[0], p[1], 1.0, p[2], 1.0, p[3], p[4]) == BAD, null
    assert b"spmv_acc_csr_add_values: null" in lib.spmv_acc_last_error_string()
    assert values(0, 0, 0, None, None, 1.0, None, 1.0, None, None) == 0 and values(0, 4, 4, None, None, 0.5, None, -2.0, None, None) == 0
    assert lib.spmv_acc_last_error() == 0
    try:  # the deterministic switch refuses nothing here
        assert lib.spmv_acc_set_tunable(b"deterministic", 1) == 0
        assert values(0, 0, 0, None, None, 1.0, None, 1.0, None, None) == 0
    finally:
        lib.spmv_acc_reset_tunables()
        lib.spmv_acc_clear_error()


def test_wrappers_refuse_bad_arguments():
    E = spmv_acc_amd.SpmvAccError
    m, n, nnz_a, nnz_b, nnz_c = 10, 12, 30, 40, 55
    good = dict(arp=_i(m + 1), aci=_i(nnz_a), av=_f(nnz_a), brp=_i(m + 1), bci=_i(nnz_b), bv=_f(nnz_b))

    def add(match, mm=m, nn=n, **bad):
        a = dict(good, **bad)
        with pytest.raises(E, match=match):
            spmv_acc_amd.csr_add(mm, nn, a["arp"], a["aci"], a["av"], a["brp"], a["bci"], a["bv"], alpha=0.5, beta=2.0, want_map=True)

    add("not on the GPU", bci=_i(nnz_b, cuda=False))
    add("dtype", arp=_FakeTensor(m + 1, dtype="torch.int64"))
    add("dtype", aci=_f(nnz_a))
    add("dtype", brp=_f(m + 1))
    add("dtype", bci=_f(nnz_b))
    add("dtype", av=_i(nnz_a))
    add("dtype", bv=_i(nnz_b))
    add("not contiguous", bv=_f(nnz_b, contiguous=False))
    add("not contiguous", aci=_i(nnz_a, contiguous=False))
    add("elements", arp=_i(m))
    add("elements", brp=_i(m))
    add("elements", av=_f(nnz_a - 1))
    add("elements", bv=_f(nnz_b - 1))
    add("as many", av=_f(nnz_a + 1))
    add("as many", bv=_f(nnz_b + 1))
    add("both", av=None)
    add("both", bv=None)
    add("on cuda:1", bv=_f(nnz_b, device="cuda:1"))
    add("torch tensor", arp=None)
    add("torch tensor", aci=[0] * nnz_a)
    add("torch tensor", brp=None)
    add("torch tensor", bci=None)
    add("torch tensor", av=3.0)
    add("negative", mm=-1)
    add("negative", nn=-3)

    def values(match, ia=_i(nnz_c), ib=_i(nnz_c), av=_f(nnz_a), bv=_f(nnz_b), out=_f(nnz_c)):
        with pytest.raises(E, match=match):
            spmv_acc_amd.csr_add_values(ia, ib, av, bv, out, alpha=0.5, beta=2.0)

    values("dtype", ia=_f(nnz_c))
    values("dtype", ib=_f(nnz_c))
    values("dtype", av=_i(nnz_a))
    values("dtype", bv=_i(nnz_b))
    values("dtype", out=_i(nnz_c))
    values("elements", ib=_i(nnz_c - 1))
    values("elements", out=_f(nnz_c - 1))
    values("as many", ib=_i(nnz_c + 1))
    values("as many", out=_f(nnz_c + 1))
    values("not on the GPU", av=_f(nnz_a, cuda=False))
    values("not contiguous", ia=_i(nnz_c, contiguous=False))
    values("on cuda:1", out=_f(nnz_c, device="cuda:1"))
    values("torch tensor", ia=None)
    values("torch tensor", ib=[0])
    values("torch tensor", av=None)
    values("torch tensor", bv=None)
    values("torch tensor", out=None)


def test_csr_add_entries_keep_no_state():
    """As test_spgemm_entries_keep_no_state: the engine file neither finds nor makes a plan, counts no plan work, reads no tunable and keeps nothing
    static; the one allocation is freed on every way out; the values entry is launch-only."""
    src = open(os.path.join(ROOT, CSRC, "csr_add.cpp")).read()
    code = re.sub(r"//[^\n]*", "", src)
    for word in ("get_plan", "g_plans", "t_plan_work", "t_last_plan", "tune_", "TimingPhase", "TuneTimer", "static std::", "thread_local", "g_tunables"):
        assert word not in code, word
    assert not re.search(r"\bstatic\b(?! const char \*const kEntry)", code), "a static other than the entries' names"
    assert code.count("hipMalloc(") == 1 and code.count("hipFree(") == 1 and "const auto leave = " in code
    assert "plan_work_allowed(" in code.split("hipMalloc(")[0]  # (a capture is refused before anything is enqueued or allocated)
    after = code.split("hipMalloc(")[1].split("\n}\n")[0]  # (to the end of the routine that allocates)
    for launch in ("launch_csr_add_census", "launch_csr_add_match", "launch_csr_add_scan", "launch_csr_add_rowptr", "launch_csr_add_place_a",
                   "launch_csr_add_place_b", "launch_csr_add_values"):
        assert launch in after, launch
    assert not re.search(r"return (?!leave\()", after.split("const auto leave = ")[1].split("};", 1)[1]), "a way out of the sum that skips leave()"
    values = code.split("int run_csr_add_values")[1]
    assert "hipMalloc" not in values and "Synchronize" not in values and "hipMemcpy" not in values and "hipMemset" not in values  # launch-only: capturable
    assert values.count("launch_csr_add_values(") == 1 and "launch_csr_add_" not in values.replace("launch_csr_add_values(", "")  # one kernel


KERNELS = ("csr_add_census_kernel", "csr_add_match_kernel", "csr_add_rowptr_kernel", "csr_add_place_a_kernel", "csr_add_place_b_kernel",
           "csr_add_values_kernel")


def test_csr_add_kernels_fit_their_register_budget(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_table

    asm = tmp_path / "k_csr_add.s"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-DKERNEL_STRATEGY_ADAPTIVE",
                        "-I" + os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-S",
                        os.path.join(ROOT, CSRC, "k_csr_add.hip"), "-o", str(asm)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    text = asm.read_text()
    assert set(re.findall(r"\.wavefront_size:\s*(\d+)", text)) == {"64"}  # wave64, every kernel of the file
    bodies = {}
    for mt in re.finditer(r"^(_ZN8spmv_acc\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, flags=re.M | re.S):
        bodies[mt.group(1)] = mt.group(2)
    assert len(bodies) == len(KERNELS), sorted(bodies)
    for k, b in bodies.items():
        assert "atomic" not in b, k  # no atomics anywhere: every output is written once, at a place computed from the inputs alone
        # every product is rounded before it is added: a fused multiply-add would round once where the definition rounds twice
        assert "v_fma_f64" not in b and "v_fmac_f64" not in b and "v_pk_fma" not in b, k
    values_body = next(b for k, b in bodies.items() if "csr_add_values_kernel" in k)
    assert "v_mul_f64" in values_body and "v_add_f64" in values_body
    rows = [k for k in resource_table.parse(r.stderr) if "rocprim" not in k["name"]]
    assert sorted(k["name"] for k in rows) == sorted(KERNELS), sorted(k["name"] for k in rows)
    for k in rows:
        # as found when the kernels were written: VGPRs -- census 20, match 18, row pointer 20, A's places 13, B's places 16, values 26 (four
        # pairs of map loads, then up to eight gathers in flight); no scratch, no AGPR, 8 waves per SIMD everywhere
        assert k["scratch"] == 0 and k["agprs"] == 0 and k["vgprs"] <= 64 and k["occupancy"] >= 8, k
    # (rocPRIM's scan kernels are instantiated in the same file and are not held to this)


# ---- the definition of the sum (include/spmv_acc.h, csr_add.hpp), in numpy: the GPU suite's reference ---------------------------------------
def host_csr_add_values(ia, ib, a_v, b_v, alpha, beta):
    """value[j] of the values entry for the map (ia, ib): ta = alpha * a_v[ia[j]], tb = beta * b_v[ib[j]], each rounded (numpy rounds every
    product and the sum to fp64: no fused multiply-add); both present: ta + tb; one present: that one alone (no + 0.0); an index outside the
    value array counts as absent; both absent: +0.0."""
    has_a, has_b = (ia >= 0) & (ia < a_v.size), (ib >= 0) & (ib < b_v.size)
    with np.errstate(all="ignore"):
        ta = np.float64(alpha) * (a_v[np.where(has_a, ia, 0)] if a_v.size else np.zeros(ia.size))
        tb = np.float64(beta) * (b_v[np.where(has_b, ib, 0)] if b_v.size else np.zeros(ib.size))
        both = ta + tb
    return np.where(has_a & has_b, both, np.where(has_a, ta, np.where(has_b, tb, 0.0)))


def host_csr_add(m, n, A, B, alpha=1.0, beta=1.0):
    """(rowptr, colindex, ia, ib, value | None) of C = alpha * A + beta * B for A = (rowptr, colindex, value | None) and B likewise, both m x n with
    strictly ascending rows: a stable sort of the concatenated (row, col) keys, A's before B's; a run of equal keys (one or two long) is one entry
    of C; ia / ib = the position of its member from A / B, or -1; the values by host_csr_add_values."""
    a_rp, a_ci, a_v = A
    b_rp, b_ci, b_v = B
    nnz_a, nnz_b = a_ci.size, b_ci.size
    assert a_rp.size == m + 1 and b_rp.size == m + 1 and a_rp[0] == 0 and b_rp[0] == 0 and a_rp[m] == nnz_a and b_rp[m] == nnz_b
    row = np.concatenate([np.repeat(np.arange(m, dtype=np.int64), np.diff(a_rp)), np.repeat(np.arange(m, dtype=np.int64), np.diff(b_rp))])
    key = row * max(n, 1) + np.concatenate([a_ci, b_ci]).astype(np.int64)
    src = np.concatenate([np.arange(nnz_a, dtype=np.int64), -1 - np.arange(nnz_b, dtype=np.int64)])  # A's positions q, B's as -1 - t
    order = np.argsort(key, kind="stable")
    sk, ss = key[order], src[order]
    head = np.ones(sk.size, dtype=bool)
    head[1:] = sk[1:] != sk[:-1]
    entry = np.cumsum(head) - 1
    nnz_c = int(head.sum())
    ia, ib = np.full(nnz_c, -1, dtype=np.int32), np.full(nnz_c, -1, dtype=np.int32)
    ia[entry[ss >= 0]] = ss[ss >= 0]
    ib[entry[ss < 0]] = -1 - ss[ss < 0]
    rowptr = np.zeros(m + 1, dtype=np.int32)
    np.cumsum(np.bincount(sk[head] // max(n, 1), minlength=m)[:m], out=rowptr[1:])
    colindex = (sk[head] % max(n, 1)).astype(np.int32)
    value = None if a_v is None else host_csr_add_values(ia, ib, a_v, b_v, alpha, beta)
    return rowptr, colindex, ia, ib, value


def random_sorted_csr(m, n, count, rng, scale=True):
    """An m x n CSR of `count` distinct positions, every row strictly ascending in column."""
    pos = np.sort(rng.choice(m * n, size=count, replace=False))
    row, col = pos // n, (pos % n).astype(np.int32)
    rowptr = np.zeros(m + 1, dtype=np.int32)
    np.cumsum(np.bincount(row, minlength=m), out=rowptr[1:])
    v = rng.standard_normal(count)
    return rowptr, col, v * 10.0 ** rng.integers(-3, 4, count) if scale else v


def dense_of(m, n, csr):
    rp, ci, v = csr
    d = np.zeros((m, n))
    d[np.repeat(np.arange(m), np.diff(rp)), ci] = v
    return d


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.int64), np.ascontiguousarray(b, dtype=np.float64).view(np.int64))


def test_host_model_against_a_dense_sum():
    """Bit for bit: a dense fp64 alpha * A + beta * B holds at most two terms per entry, each product rounded, one addition -- the same arithmetic
    wherever both are present; where one is absent the dense form adds alpha * a + beta * 0.0, which differs from the definition only in the sign of
    a zero result, so there the comparison is on the present term."""
    rng = np.random.default_rng(11)
    for m, n, ca, cb in ((40, 50, 300, 400), (7, 90, 200, 20), (1, 1, 1, 1), (30, 20, 0, 100), (30, 20, 100, 0), (5, 5, 25, 25), (6, 7, 0, 0)):
        A, B = random_sorted_csr(m, n, ca, rng), random_sorted_csr(m, n, cb, rng)
        for alpha, beta in ((1.0, 1.0), (0.5, -2.0), (0.0, 1.0), (-1.0, 0.0), (1.0 / 3.0, 1e-3)):
            rp, ci, ia, ib, v = host_csr_add(m, n, A, B, alpha, beta)
            pa, pb = dense_of(m, n, (A[0], A[1], np.ones(ca))) > 0, dense_of(m, n, (B[0], B[1], np.ones(cb))) > 0
            rows = np.repeat(np.arange(m), np.diff(rp))
            got = np.zeros((m, n), dtype=bool)
            got[rows, ci] = True
            assert np.array_equal(got, pa | pb) and ci.size == int((pa | pb).sum()) == ia.size == ib.size  # the union, nothing pruned
            assert all(np.all(np.diff(ci[rp[r]:rp[r + 1]]) > 0) for r in range(m))
            assert np.array_equal(ia >= 0, pa[rows, ci]) and np.array_equal(ib >= 0, pb[rows, ci]) and np.all((ia >= 0) | (ib >= 0))
            a_row, b_row = np.repeat(np.arange(m), np.diff(A[0])), np.repeat(np.arange(m), np.diff(B[0]))
            assert np.array_equal(a_row[ia[ia >= 0]], rows[ia >= 0]) and np.array_equal(A[1][ia[ia >= 0]], ci[ia >= 0])
            assert np.array_equal(b_row[ib[ib >= 0]], rows[ib >= 0]) and np.array_equal(B[1][ib[ib >= 0]], ci[ib >= 0])
            assert np.array_equal(np.sort(ia[ia >= 0]), np.arange(ca)) and np.array_equal(np.sort(ib[ib >= 0]), np.arange(cb))
            da, db = dense_of(m, n, A), dense_of(m, n, B)
            dense = (alpha * da + beta * db)[rows, ci]
            both = (ia >= 0) & (ib >= 0)
            assert same_bits(v[both], dense[both])
            assert same_bits(v[~both & (ia >= 0)], (alpha * da)[rows, ci][~both & (ia >= 0)])
            assert same_bits(v[~both & (ib >= 0)], (beta * db)[rows, ci][~both & (ib >= 0)])
            assert np.array_equal(v, dense)  # (as numbers everywhere: -0.0 == +0.0)
            s = host_csr_add(m, n, (A[0], A[1], None), (B[0], B[1], None))
            assert s[4] is None and all(np.array_equal(x, y) for x, y in zip(s[:4], (rp, ci, ia, ib)))
    # by hand: A = [[a0 . a1], [. . .], [a2 . .]], B = [[. b0 b1], [b2 . .], [. . .]]
    A = (np.array([0, 2, 2, 3], np.int32), np.array([0, 2, 0], np.int32), np.array([2.0, 3.0, 5.0]))
    B = (np.array([0, 2, 3, 3], np.int32), np.array([1, 2, 0], np.int32), np.array([7.0, 11.0, 13.0]))
    rp, ci, ia, ib, v = host_csr_add(3, 3, A, B, 0.5, -2.0)
    assert rp.tolist() == [0, 3, 4, 5] and ci.tolist() == [0, 1, 2, 0, 0]
    assert ia.tolist() == [0, -1, 1, -1, 2] and ib.tolist() == [-1, 0, 1, 2, -1]
    assert v.tolist() == [1.0, -14.0, 1.5 - 22.0, -26.0, 2.5]
    # the sign of zero: an absent side is left out, not added as +0.0; a cancelled entry stays, as +0.0
    one = np.array([0, 1], np.int32), np.array([0], np.int32)
    none = np.array([0, 0], np.int32), np.zeros(0, np.int32), np.zeros(0)
    assert np.signbit(host_csr_add(1, 1, one + (np.array([-0.0]),), none)[4][0])
    z = host_csr_add(1, 1, one + (np.array([-0.0]),), one + (np.array([0.0]),))[4]
    assert z.tolist() == [0.0] and not np.signbit(z[0])
    c = host_csr_add(1, 1, one + (np.array([3.0]),), one + (np.array([3.0]),), 1.0, -1.0)
    assert c[1].tolist() == [0] and c[4].tolist() == [0.0]
    # alpha == 0 is not special: 0 * Inf = NaN, and the pattern is the union
    nan = host_csr_add(1, 1, one + (np.array([np.inf]),), none, 0.0, 1.0)
    assert nan[1].tolist() == [0] and np.isnan(nan[4][0])
    # the values entry's crafted maps: an index outside the value array is absent, both absent is +0.0
    crafted = host_csr_add_values(np.array([0, -1, 5, -7], np.int32), np.array([-1, 9, 0, 1], np.int32), np.array([2.0]), np.array([3.0]), -1.0, 1.0)
    assert crafted.tolist() == [-2.0, 0.0, 3.0, 0.0] and not np.signbit(crafted[1]) and not np.signbit(crafted[3])


def test_host_model_against_scipy():
    sp = pytest.importorskip("scipy.sparse")
    rng = np.random.default_rng(12)
    for m, n, ca, cb in ((60, 70, 500, 600), (300, 200, 3000, 2500), (50, 50, 0, 300)):
        A, B = random_sorted_csr(m, n, ca, rng), random_sorted_csr(m, n, cb, rng)
        for alpha, beta in ((1.0, 1.0), (0.5, -2.0)):
            rp, ci, ia, ib, v = host_csr_add(m, n, A, B, alpha, beta)
            # the pattern from all-ones values (no cancellation, so scipy prunes nothing), the values from the scaled sum
            P = sp.csr_matrix((np.ones(ca), A[1], A[0]), shape=(m, n)) + sp.csr_matrix((np.ones(cb), B[1], B[0]), shape=(m, n))
            P.sort_indices()
            assert np.array_equal(P.indptr, rp) and np.array_equal(P.indices, ci)
            C = (alpha * sp.csr_matrix((A[2], A[1], A[0]), shape=(m, n)) + beta * sp.csr_matrix((B[2], B[1], B[0]), shape=(m, n))).toarray()
            assert np.array_equal(C[np.repeat(np.arange(m), np.diff(rp)), ci], v)  # the same two roundings and one addition: equal as numbers
