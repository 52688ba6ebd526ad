"""CPU side of the device CSR extraction C = A[rows, colmap] with a diagonal band (no GPU): the C ABI declares and exports the two entries, they
and the Python wrappers refuse bad arguments before any launch, the compiled kernels use no scratch, no AGPR and no atomic and fit 64 VGPRs,
every size-selected branch of the new code names the GPU tests that cross it, the engine file stays stateless, and the definition -- selected
rows, mapped and dropped columns, the band in C's own indices, every row in ascending new column with ties in A's order, the map -- is restated
here in numpy (host_csr_extract, exported to the GPU suite as its reference) and checked bit for bit against dense indexing and, where it is
installed, against scipy.sparse."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import spmv_acc_amd
from test_coo_host import HELPERS, SHARED, _FakeTensor, _f, _i
from test_csr_add_host import dense_of, random_sorted_csr, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "spmv_acc_amd/csrc/"
NEW_SOURCES = ("extract.hpp", "k_extract.hip", "extract.cpp")
GPU = "test_extract_is_the_host_model"
STRIDE = "test_extract_grid_stride_at_test_size"
CONTRACT = "test_extract_contract"
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1

# (rule, file, regex that must match the source, GPU tests of tests/test_gpu_extract.py that cross it at test size, what it selects)
EXTRACT_SIZE_RULES = [
    ("kExtractPerLane", CSRC + "extract.hpp", r"constexpr int kExtractPerLane = 8;",
     [GPU, "test_special_values"], "values pass: C entries per lane (results of fewer than 8 * 64 entries leave lanes and steps empty: one_by_one, diag)"),
    ("kExtractWaveChunk", CSRC + "extract.hpp", r"constexpr int kExtractWaveChunk = 64 \* kExtractPerLane;",
     [GPU], "entries per wavefront: 512; the last wavefront of a result is partly empty"),
    ("kExtractTile", CSRC + "extract.hpp", r"constexpr int kExtractTile = 4 \* kExtractWaveChunk;",
     [GPU, STRIDE], "entries per workgroup of the values pass: 2 048 (hub_row: 60 tiles and more, several inside the hub row; large: 390)"),
    ("kExtractRankTile", CSRC + "extract.hpp", r"constexpr int kExtractRankTile = 256;",
     [GPU, STRIDE], "items per workgroup of the candidates, the scatter, the descents and the keys: 256, a wavefront 64 consecutive ones -- inside "
                    "one row (hub_row), across rows, across empty rows (empties)"),
    ("kEntryAlign", CSRC + HELPERS, r"constexpr size_t kEntryAlign = 256;",
     [GPU], "workspace parts are padded to 256 B (counts that are no multiple of 64: most cases)"),
    ("kExtractCounts", CSRC + "extract.cpp", r"constexpr int kExtractCounts = 7;",
     [GPU, CONTRACT], "seven groups of per-wavefront counts: the census' five, the candidates' columns, the descents"),
    ("census grid", CSRC + SHARED, r"return grid > static_cast<unsigned>\(kCooCheckBlocks\) \? static_cast<unsigned>\(kCooCheckBlocks\) : grid;",
     [STRIDE, CONTRACT], "one count slot per wavefront of at most 1 024 workgroups (large: 3 126 tiles of candidates exceed them)"),
    ("census grid: the extraction's call", CSRC + "k_extract.hip", r"dim3\(census_grid_for\(static_cast<long long>\(S\) \+ 1, kExtractRankTile\)\)",
     [STRIDE, CONTRACT], "the census, the candidates and the descents take the shared census grid"),
    ("row loop of the marks", CSRC + "k_extract.hip", r"for \(long long i = first; i < mc; i \+= stride\) \{",
     [STRIDE], "one selected row per lane, striding (large: 200 000 rows, 782 workgroups); likewise the columns: c < n; c += stride"),
    ("row loop of the census", CSRC + "k_extract.hip", r"for \(long long i = first; i <= mc; i \+= stride\) \{",
     [STRIDE, CONTRACT], "mc + 1 lengths, one per lane, striding"),
    ("tile loop of the candidates", CSRC + "k_extract.hip", r"if \(base >= items\) continue; // \(wave-uniform\)",
     [STRIDE], "S + 1 items: the closing element may open a tile of its own (large: S = 800 000, a multiple of 256)"),
    ("tile loop of the scatter", CSRC + "k_extract.hip", r"if \(base >= S\) continue; // \(wave-uniform\)",
     [STRIDE], "blocks stride over the tiles of candidates beyond the grid"),
    ("tile loops of the descents and the keys", CSRC + "k_extract.hip", r"if \(base >= nnz_c\) continue; // \(wave-uniform\)",
     [STRIDE], "blocks stride over the tiles of C entries beyond the grid"),
    ("tile loop of the values pass", CSRC + "k_extract.hip",
     r"for \(long long tile = blockIdx\.x; tile < ntiles; tile \+= gridDim\.x\) \{ // \(block-uniform\)\n    const long long base = tile \* kExtractTile",
     [STRIDE], "blocks stride over the tiles of C entries beyond the grid"),
    ("row pointer pass", CSRC + "k_extract.hip", r"i <= mc; i \+= stride\) c_rowptr\[i\] = pos\[src_ptr\[i\]\];",
     [STRIDE], "one lane per row, striding (large: 200 001 rows)"),
    ("sorted pass", CSRC + "k_extract.hip", r"j < nnz_c; j \+= stride\) \{",
     [STRIDE], "one sorted entry per lane, striding (large: 3 125 workgroups)"),
    ("kMaxGridBlocks (grid striding)", CSRC + SHARED, r"const long long cap = max_grid_blocks\(\);",
     [STRIDE], "every kernel of the two entries strides over the work beyond max_grid_blocks() workgroups"),
    ("kMaxGridBlocks (grid striding): the extraction's call", CSRC + "k_extract.hip", r"dim3\(grid_for\(nnz_c, kExtractTile\)\)",
     [STRIDE], "the launchers of the two entries take the shared grid"),
    ("sort or not", CSRC + "extract.cpp", r"if \(descents != 0\) \{ // some row is not ascending: one stable sort by \(row, column\)",
     [GPU, STRIDE], "no descent inside a row (identity, sub_block, rows_shuffled, embed, tril, strict_triu, diag): the compaction is the answer; "
                    "otherwise (unsorted_in, repeats, permuted, band_after_map, hub_row, large) one radix sort"),
    ("a map index outside the value array", CSRC + "k_extract.hip", r"if \(static_cast<unsigned>\(u\[k\]\) < static_cast<unsigned>\(nnz_a\)\) v\[k\] = a_value\[u\[k\]\];",
     ["test_crafted_map"], "-1 or >= nnz_a gives +0.0 and is never turned into an address"),
    ("scan sizes", CSRC + "k_extract.hip", r"rocprim::make_transform_iterator\(newcol, ExtractKept\(\)\), pos, 0, count,",
     [GPU, STRIDE], "the library scans over 2 (one_by_one) ... 800 001 items"),
    ("no rows, no matrix", CSRC + "extract.cpp", r"if \(mc == 0\) return nothing_to_extract\(\);",
     [GPU], "mc == 0 (no_rows), and before it m == 0: c_rowptr zeroed, nothing is read or allocated"),
    ("no entries", CSRC + "extract.cpp", r"if \(nnz_a == 0\) return nothing_to_extract\(\);",
     [GPU], "A has no entries (empty_a): c_rowptr zeroed, nothing allocated"),
    ("no candidates", CSRC + "extract.cpp", r"if \(S == 0\) return nothing_kept\(\);",
     [GPU], "only empty rows selected (empties_only): c_rowptr zeroed after the census"),
    ("nothing kept", CSRC + "extract.cpp", r"if \(nnz_c == 0\) return nothing_kept\(\);",
     [GPU], "every candidate dropped (all_dropped, lo_above_hi): c_rowptr zeroed, nothing else written"),
    ("workspace with / without the map", CSRC + "extract.cpp", r"const bool own_map = d_map == nullptr && d_c_value != nullptr;",
     [GPU], "values without a caller's map (no_map): it lives in the workspace, 4 B per candidate more; structure only without a map: none is written"),
    ("int32 block arithmetic", CSRC + HELPERS, r"inline bool too_large\(long long v\) \{ return v > INT_MAX - \(1 << 16\); \}",
     [CONTRACT], "m, n, mc, nc or nnz_a beyond this: SPMV_ACC_ERR_TOO_LARGE, as the other entries"),
]


def test_extract_size_rules_name_their_tests():
    gpu_tests = open(os.path.join(ROOT, "tests", "test_gpu_extract.py")).read()
    defined = set(re.findall(r"^def (test_\w+)\(", gpu_tests, flags=re.M))
    for name, path, pattern, tests, what in EXTRACT_SIZE_RULES:
        assert re.search(pattern, open(os.path.join(ROOT, path)).read()), f"{name}: no longer matches {path}: {pattern}"
        assert tests and what
        for t in tests:
            assert t in defined, f"{name}: names {t}, which is not a test of tests/test_gpu_extract.py"
    # every named constant of the new files is registered above (tests/size_thresholds.py does not scan them)
    registered = " ".join(r[0] + " " + r[2] for r in EXTRACT_SIZE_RULES)
    found = 0
    for f in NEW_SOURCES + (HELPERS,):  # (the alignment is the shared header's)
        for k in re.findall(r"constexpr\s+[\w:<> ]+?\s+(k[A-Z]\w*)\s*=", open(os.path.join(ROOT, CSRC, f)).read()):
            found += 1
            assert k in registered, f"{f}: constant {k} is not in EXTRACT_SIZE_RULES"
    assert found == 6
    # every tile loop of the kernels file is one of the registered forms
    kernels = open(os.path.join(ROOT, CSRC, "k_extract.hip")).read()
    assert kernels.count("tile += gridDim.x") == 5 and kernels.count("if (base >= ") == 5


PROTOTYPES = (
    r"int spmv_acc_csr_extract\(int m, int n, int nnz_a, const int \*d_a_rowptr, const int \*d_a_colindex, const double \*d_a_value,\s*"
    r"int mc, const int \*d_rows, int nc, const int \*d_colmap, int diag_lo, int diag_hi,\s*"
    r"int \*d_c_rowptr, int \*d_c_colindex, double \*d_c_value, int \*d_map, int \*h_nnz\);",
    r"int spmv_acc_csr_extract_values\(int nnz_c, int nnz_a, const int \*d_map, const double \*d_a_value, double \*d_c_value\);",
)


def test_extract_entries_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "spmv_acc.h")).read()
    for proto in PROTOTYPES:
        assert re.search(proto, header), proto
    for entry in ("1", "2"):
        block = re.search(r"/\* ---- extraction C = A\[rows, colmap\] with a diagonal band, " + entry + r".*?\*/", header, flags=re.S)
        assert block and "replaces: nothing in the reference" in block.group(0) and "COST" in block.group(0), entry
        assert "d_c_value must not overlap d_a_value" in re.sub(r"\s*\n \* ", " ", block.group(0)).lower(), entry  # said for both entries
    lib = spmv_acc_amd.load_library()
    for s in ("spmv_acc_csr_extract", "spmv_acc_csr_extract_values"):
        assert s in spmv_acc_amd.C_ABI_SYMBOLS and hasattr(lib, s), s
    assert lib.spmv_acc_csr_extract.restype is ctypes.c_int and lib.spmv_acc_csr_extract_values.restype is ctypes.c_int
    assert len(lib.spmv_acc_csr_extract.argtypes) == 17 and len(lib.spmv_acc_csr_extract_values.argtypes) == 5
    for i in (0, 1, 2, 6, 8, 10, 11):
        assert lib.spmv_acc_csr_extract.argtypes[i] is ctypes.c_int, i
    for i in (3, 4, 5, 7, 9, 12, 13, 14, 15):
        assert lib.spmv_acc_csr_extract.argtypes[i] is ctypes.c_void_p, i
    for f in ("csr_extract", "csr_extract_values", "csr_permute"):
        assert callable(getattr(spmv_acc_amd, f))
    for f in ("k_extract.hip", "extract.cpp"):  # both builds compile the new files
        assert f in open(os.path.join(ROOT, CSRC, "Makefile")).read() and f in open(os.path.join(ROOT, "CMakeLists.txt")).read(), f
    assert "extract.hpp" in open(os.path.join(ROOT, CSRC, "Makefile")).read()


BAD, TOO_LARGE = 2, 4  # SPMV_ACC_ERR_BAD_ARGUMENT, SPMV_ACC_ERR_TOO_LARGE


def test_bad_arguments_are_refused_without_a_gpu():
    """The C entries check their arguments before they touch the device: the error codes come back on a machine without one."""
    lib = spmv_acc_amd.load_library()
    one = 8  # (never dereferenced: a non-null pointer value)
    h = ctypes.c_int(-5)
    extract, values = lib.spmv_acc_csr_extract, lib.spmv_acc_csr_extract_values

    def call(m=4, n=4, nnz_a=4, arp=one, aci=one, av=one, mc=3, rows=one, nc=5, colmap=one, lo=INT_MIN, hi=INT_MAX, crp=one, cci=one, cv=one,
             cmap=one, hn=ctypes.byref(h)):
        return extract(m, n, nnz_a, arp, aci, av, mc, rows, nc, colmap, lo, hi, crp, cci, cv, cmap, hn)

    for neg in ("m", "n", "mc", "nc"):
        assert call(**{neg: -1}) == BAD, neg
        assert b"spmv_acc_csr_extract: negative" in lib.spmv_acc_last_error_string()
    assert call(crp=None) == BAD and call(hn=None) == BAD
    for mix in (dict(av=None), dict(cv=None)):
        assert call(**mix) == BAD, mix  # values: both or none
        assert b"both be given or both be NULL" in lib.spmv_acc_last_error_string()
    for mc in (3, 5, 0):
        assert call(rows=None, mc=mc) == BAD, mc  # every row: mc must be m
        assert b"mc must equal m" in lib.spmv_acc_last_error_string()
    for nc in (3, 5, 0):
        assert call(colmap=None, nc=nc) == BAD, nc  # the identity: nc must be n
        assert b"nc must equal n" in lib.spmv_acc_last_error_string()
    for null in ("arp", "aci", "cci"):
        for groups in (dict(), dict(av=None, cv=None), dict(cmap=None), dict(rows=None, mc=4), dict(colmap=None, nc=4)):
            assert call(**{null: None}, **groups) == BAD, null
            assert call(**{null: None}, nnz_a=-1, **groups) == BAD, null  # (the size to be read from the device: not before the pointers are checked)
        assert b"spmv_acc_csr_extract: null" in lib.spmv_acc_last_error_string(), null
    for big in (2 ** 31 - 1, 2 ** 31 - 2 ** 16):
        for which in ("m", "n", "mc", "nc", "nnz_a"):
            assert call(**{which: big}) == TOO_LARGE, which
            assert b"row ranges" in lib.spmv_acc_last_error_string() and b"spmv_acc_csr_extract:" in lib.spmv_acc_last_error_string()
        assert call(rows=None, m=big, mc=big) == TOO_LARGE and call(colmap=None, n=big, nc=big) == TOO_LARGE
        assert values(big, 4, one, one, one) == TOO_LARGE and values(4, big, one, one, one) == TOO_LARGE
        assert b"spmv_acc_csr_extract_values:" in lib.spmv_acc_last_error_string()
    assert h.value == -5
    for neg in range(2):
        assert values(*[-1 if i == neg else 4 for i in range(2)], one, one, one) == BAD, neg
    for null in range(3):
        p = [None if i == null else one for i in range(3)]
        assert values(4, 4, *p) == BAD, null
    assert b"spmv_acc_csr_extract_values: null" in lib.spmv_acc_last_error_string()
    assert values(0, 0, None, None, None) == 0 and values(0, 4, None, None, None) == 0
    assert lib.spmv_acc_last_error() == 0
    try:  # the deterministic switch refuses nothing here
        assert lib.spmv_acc_set_tunable(b"deterministic", 1) == 0
        assert values(0, 0, None, None, None) == 0
    finally:
        lib.spmv_acc_reset_tunables()
        lib.spmv_acc_clear_error()


def test_wrappers_refuse_bad_arguments():
    E = spmv_acc_amd.SpmvAccError
    m, n, nnz_a, mc, nnz_c = 10, 12, 30, 7, 20
    good = dict(rp=_i(m + 1), ci=_i(nnz_a), v=_f(nnz_a), rows=_i(mc), colmap=_i(n))

    def extract(match, mm=m, nn=n, nc=9, **bad):
        a = dict(good, **bad)
        with pytest.raises(E, match=match):
            spmv_acc_amd.csr_extract(mm, nn, a["rp"], a["ci"], a["v"], rows=a["rows"], colmap=a["colmap"], nc=nc, diag_lo=-1, diag_hi=1, want_map=True)

    extract("not on the GPU", ci=_i(nnz_a, cuda=False))
    extract("not on the GPU", rows=_i(mc, cuda=False))
    extract("dtype", rp=_FakeTensor(m + 1, dtype="torch.int64"))
    extract("dtype", ci=_f(nnz_a))
    extract("dtype", v=_i(nnz_a))
    extract("dtype", rows=_FakeTensor(mc, dtype="torch.int64"))
    extract("dtype", colmap=_f(n))
    extract("not contiguous", v=_f(nnz_a, contiguous=False))
    extract("not contiguous", colmap=_i(n, contiguous=False))
    extract("elements", rp=_i(m))
    extract("elements", v=_f(nnz_a - 1))
    extract("elements", colmap=_i(n - 1))
    extract("as many", v=_f(nnz_a + 1))
    extract("as many", colmap=_i(n + 1))
    extract("on cuda:1", v=_f(nnz_a, device="cuda:1"))
    extract("on cuda:1", colmap=_i(n, device="cuda:1"))
    extract("torch tensor", rp=None)
    extract("torch tensor", ci=[0] * nnz_a)
    extract("torch tensor", v=3.0)
    extract("torch tensor", rows=[0, 1])
    extract("torch tensor", colmap=[0] * n)
    extract("negative", mm=-1)
    extract("negative", nn=-3)
    extract("negative", nc=-1)
    extract("must be n", colmap=None, nc=n + 1)
    with pytest.raises(E, match="outside int32"):
        spmv_acc_amd.csr_extract(m, n, good["rp"], good["ci"], good["v"], diag_lo=-2 ** 31 - 1)
    with pytest.raises(E, match="outside int32"):
        spmv_acc_amd.csr_extract(m, n, good["rp"], good["ci"], good["v"], diag_hi=2 ** 31)

    def values(match, cmap=_i(nnz_c), av=_f(nnz_a), out=_f(nnz_c)):
        with pytest.raises(E, match=match):
            spmv_acc_amd.csr_extract_values(cmap, av, out)

    values("dtype", cmap=_f(nnz_c))
    values("dtype", av=_i(nnz_a))
    values("dtype", out=_i(nnz_c))
    values("elements", out=_f(nnz_c - 1))
    values("as many", out=_f(nnz_c + 1))
    values("not on the GPU", av=_f(nnz_a, cuda=False))
    values("not contiguous", cmap=_i(nnz_c, contiguous=False))
    values("on cuda:1", out=_f(nnz_c, device="cuda:1"))
    values("torch tensor", cmap=None)
    values("torch tensor", av=None)
    values("torch tensor", out=[0.0])

    def permute(match, mm=m, perm=_i(m)):
        with pytest.raises(E, match=match):
            spmv_acc_amd.csr_permute(mm, _i(m + 1), _i(nnz_a), _f(nnz_a), perm, want_map=True)

    permute("as many", perm=_i(m - 1))  # a perm of the wrong length, before it is used as an index
    permute("as many", perm=_i(m + 1))
    permute("as many", perm=_i(0))
    permute("dtype", perm=_FakeTensor(m, dtype="torch.int64"))
    permute("not on the GPU", perm=_i(m, cuda=False))
    permute("not contiguous", perm=_i(m, contiguous=False))
    permute("torch tensor", perm=None)
    permute("torch tensor", perm=list(range(m)))
    permute("negative", mm=-1)


def test_extract_entries_keep_no_state():
    """As test_csr_add_entries_keep_no_state: the engine file neither finds nor makes a plan, counts no plan work, reads no tunable and keeps
    nothing static; its three allocations are freed on every way out; the values entry is launch-only."""
    src = open(os.path.join(ROOT, CSRC, "extract.cpp")).read()
    code = re.sub(r"//[^\n]*", "", src)
    for word in ("get_plan", "g_plans", "t_plan_work", "t_last_plan", "tune_", "TimingPhase", "TuneTimer", "static std::", "thread_local", "g_tunables"):
        assert word not in code, word
    assert not re.search(r"\bstatic\b(?! const char \*const kEntry)", code), "a static other than the entries' names"
    assert code.count("hipMalloc(") == 3 and code.count("hipFree(") == 3 and "const auto leave = " in code
    leave = code.split("const auto leave = ")[1].split("};", 1)[0]
    assert leave.count("hipFree(") == 3 and "hipStreamSynchronize(" in leave.split("hipFree(")[0]  # the stream has run before the workspace goes
    assert "plan_work_allowed(" in code.split("const auto leave = ")[0]  # (a capture is refused before anything is enqueued or allocated)
    assert "hipMalloc(" not in code.split("const auto leave = ")[0]
    after = code.split("const auto leave = ")[1].split("};", 1)[1].split("\n}\n")[0]  # (to the end of the routine that allocates)
    for launch in ("launch_extract_mark", "launch_extract_census", "launch_extract_scan(", "launch_extract_candidates", "launch_extract_scan_kept",
                   "launch_extract_rowptr", "launch_extract_scatter", "launch_extract_descents", "launch_extract_keys", "launch_coo_sort",
                   "launch_extract_sorted", "launch_extract_values"):
        assert launch in after, launch
    no_lambdas = re.sub(r"const auto nothing_kept = .*?\n  \};", "", after, flags=re.S)
    bare = [ln.strip() for ln in no_lambdas.splitlines() if re.search(r"\breturn\b(?! leave\()(?! nothing_kept\(\))", ln)]
    # (the one way out that may skip leave(): the scratch query before the first allocation)
    assert bare == ['return entry_error(kEntry, kErrHip, "scan workspace query failed");'], bare
    values = code.split("int run_csr_extract_values")[1]
    assert "hipMalloc" not in values and "Synchronize" not in values and "hipMemcpy" not in values and "hipMemset" not in values  # launch-only: capturable
    assert values.count("launch_extract_values(") == 1 and "launch_extract_" not in values.replace("launch_extract_values(", "")  # one kernel


KERNELS = ("extract_mark_kernel", "extract_census_kernel", "extract_candidates_kernel", "extract_rowptr_kernel", "extract_scatter_kernel",
           "extract_descents_kernel", "extract_keys_kernel", "extract_sorted_kernel", "extract_values_kernel")
# as recorded in k_extract.hip's header comment
RECORDED_VGPRS = dict(extract_mark_kernel=18, extract_census_kernel=16, extract_candidates_kernel=20, extract_rowptr_kernel=18,
                      extract_scatter_kernel=20, extract_descents_kernel=20, extract_keys_kernel=18, extract_sorted_kernel=9, extract_values_kernel=26)


def test_extract_kernels_fit_their_register_budget(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_table

    asm = tmp_path / "k_extract.s"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-DKERNEL_STRATEGY_ADAPTIVE",
                        "-I" + os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-S",
                        os.path.join(ROOT, CSRC, "k_extract.hip"), "-o", str(asm)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    text = asm.read_text()
    assert set(re.findall(r"\.wavefront_size:\s*(\d+)", text)) == {"64"}  # wave64, every kernel of the file
    bodies = {}
    for mt in re.finditer(r"^(_ZN8spmv_acc\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, flags=re.M | re.S):
        bodies[mt.group(1)] = mt.group(2)
    assert len(bodies) == len(KERNELS), sorted(bodies)
    for k, b in bodies.items():
        assert "atomic" not in b, k  # no atomics anywhere
    values_body = next(b for k, b in bodies.items() if "extract_values_kernel" in k)
    for op in ("v_mul_f64", "v_add_f64", "v_fma_f64", "v_max_f64", "v_min_f64"):  # the bits are copied: no arithmetic touches a value
        assert op not in values_body, op
    header = open(os.path.join(ROOT, CSRC, "k_extract.hip")).read().split("#include")[0]
    rows = [k for k in resource_table.parse(r.stderr) if "rocprim" not in k["name"]]
    assert sorted(k["name"] for k in rows) == sorted(KERNELS), sorted(k["name"] for k in rows)
    for k in rows:
        assert k["scratch"] == 0 and k["agprs"] == 0 and k["vgprs"] <= 64 and k["occupancy"] >= 8, k
        want = RECORDED_VGPRS[k["name"]]
        assert re.search(k["name"] + r", " + str(want) + r"\b", header), (k["name"], "the count recorded in the header comment")
        assert k["vgprs"] <= want + 4, (k, "grew past the count recorded in k_extract.hip (a few registers of compiler drift are allowed)")
    # (rocPRIM's scan kernels are instantiated in the same file and are not held to this)


# ---- the definition of the extraction (include/spmv_acc.h, extract.hpp), in numpy: the GPU suite's reference ----------------------------------
def host_csr_extract(m, n, A, rows=None, colmap=None, nc=None, diag_lo=None, diag_hi=None):
    """(rowptr, colindex, map, value | None) of C = A[rows, colmap] with the band [diag_lo, diag_hi] for A = (rowptr, colindex, value | None),
    m x n, rows in any column order: the candidates are the entries of the selected rows, in the order of rows and inside a row in A's order;
    kept are those whose new column colmap[c] is >= 0 and whose diagonal new column - i lies in the band; per row a STABLE argsort of the new
    columns of the kept entries (here: one stable sort of row * width + new column, the same thing).  map = the position in A's arrays."""
    rp, ci, v = A
    rows = np.arange(m, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    colmap = np.arange(n, dtype=np.int64) if colmap is None else np.asarray(colmap, dtype=np.int64)
    nc = n if nc is None else nc
    lo = INT_MIN if diag_lo is None else diag_lo
    hi = INT_MAX if diag_hi is None else diag_hi
    mc = rows.size
    assert rp.size == m + 1 and rp[0] == 0 and rp[m] == ci.size and colmap.size == n and np.unique(rows).size == mc
    assert mc == 0 or (rows.min() >= 0 and rows.max() < m)
    kept_cols = colmap[colmap >= 0]
    assert np.unique(kept_cols).size == kept_cols.size and (kept_cols.size == 0 or kept_cols.max() < nc)
    lens = (rp[rows + 1] - rp[rows]).astype(np.int64) if mc else np.zeros(0, np.int64)
    src_ptr = np.concatenate([[0], np.cumsum(lens)])
    i = np.repeat(np.arange(mc, dtype=np.int64), lens)
    q = rp[rows].astype(np.int64)[i] + np.arange(src_ptr[-1], dtype=np.int64) - src_ptr[:-1][i]  # the position in A of every candidate
    j = colmap[ci[q]] if q.size else np.zeros(0, np.int64)
    keep = (j >= 0) & (j - i >= lo) & (j - i <= hi)
    i, q, j = i[keep], q[keep], j[keep]
    order = np.argsort(i * max(nc, 1) + j, kind="stable")
    rowptr = np.zeros(mc + 1, dtype=np.int32)
    np.cumsum(np.bincount(i, minlength=mc)[:mc], out=rowptr[1:])
    cmap = q[order].astype(np.int32)
    return rowptr, j[order].astype(np.int32), cmap, None if v is None else v[cmap]


def host_csr_permute(m, A, perm):
    """C[i, j] = A[perm[i], perm[j]]: rows = perm, colmap = the inverse of perm."""
    perm = np.asarray(perm, dtype=np.int64)
    inverse = np.full(m, -1, dtype=np.int64)
    inverse[perm] = np.arange(m)
    return host_csr_extract(m, m, A, rows=perm, colmap=inverse, nc=m)


def band_mask(mc, nc, lo, hi):
    d = np.arange(nc, dtype=np.int64)[None, :] - np.arange(mc, dtype=np.int64)[:, None]
    return (d >= (INT_MIN if lo is None else lo)) & (d <= (INT_MAX if hi is None else hi))


BANDS = ((None, None), (0, 0), (None, 0), (1, None), (-2, 3), (3, 2), (None, -1))


def selections(m, n, rng):
    """(rows, cols, nc): C = A[rows][:, cols] embedded in nc columns -- None for all, subsets in ascending and in random order."""
    yield None, None, n
    yield np.sort(rng.permutation(m)[:max(1, m // 2)]), np.sort(rng.permutation(n)[:max(1, n // 3)]), max(1, n // 3)
    yield rng.permutation(m)[:max(1, 2 * m // 3)], rng.permutation(n)[:max(1, n // 2)], max(1, n // 2) + 3
    yield rng.permutation(m), rng.permutation(n), n
    yield np.zeros(0, np.int64), rng.permutation(n)[:1], 1


def colmap_of(n, cols):
    if cols is None:
        return None
    colmap = np.full(n, -1, dtype=np.int64)
    colmap[cols] = np.arange(cols.size)
    return colmap


def test_host_model_against_dense_indexing():
    """Bit for bit on matrices that repeat no column (values are drawn non-zero, so the dense form shows the pattern): the model against
    dense[rows][:, cols] under the band mask, and the permutation's model against D[perm][:, perm]."""
    rng = np.random.default_rng(21)
    for m, n, count in ((40, 50, 300), (7, 90, 200), (1, 1, 1), (30, 20, 0), (5, 5, 25), (60, 60, 500)):
        A = random_sorted_csr(m, n, count, rng)
        shuffled = shuffle_rows(A, rng)
        D = dense_of(m, n, A)
        assert same_bits(D, dense_of(m, n, shuffled)) and int((D != 0).sum()) == count
        for rows, cols, nc in selections(m, n, rng):
            for lo, hi in BANDS:
                mc = m if rows is None else rows.size
                want = D[np.arange(m) if rows is None else rows][:, np.arange(n) if cols is None else cols]
                want = np.where(band_mask(mc, nc, lo, hi), np.pad(want, ((0, 0), (0, nc - want.shape[1]))), 0.0)
                for M in (A, shuffled):  # whatever the order inside A's rows
                    rp, ci, cmap, v = host_csr_extract(m, n, M, rows, colmap_of(n, cols), nc, lo, hi)
                    assert rp[0] == 0 and rp[mc] == ci.size == cmap.size == v.size == int((want != 0).sum())  # nothing pruned, nothing invented
                    assert all(np.all(np.diff(ci[rp[r]:rp[r + 1]]) > 0) for r in range(mc))  # strictly ascending: A repeats no column
                    assert same_bits(dense_of(mc, nc, (rp, ci, v)), want)
                    assert same_bits(v, M[2][cmap])
                    s = host_csr_extract(m, n, (M[0], M[1], None), rows, colmap_of(n, cols), nc, lo, hi)
                    assert s[3] is None and all(np.array_equal(x, y) for x, y in zip(s[:3], (rp, ci, cmap)))
        if m == n:
            perm = rng.permutation(m)
            rp, ci, cmap, v = host_csr_permute(m, shuffled, perm)
            assert same_bits(dense_of(m, m, (rp, ci, v)), D[perm][:, perm]) and ci.size == count
            assert np.array_equal(np.sort(cmap), np.arange(count))  # every entry of A exactly once
    # by hand: A = [[a0 . a1 a2], [. . . .], [a3 a4 . .]] with row 0 stored as columns (3, 0, 2)
    A = (np.array([0, 3, 3, 5], np.int32), np.array([3, 0, 2, 1, 0], np.int32), np.array([2.0, 3.0, 5.0, 7.0, 11.0]))
    rp, ci, cmap, v = host_csr_extract(3, 4, A)
    assert rp.tolist() == [0, 3, 3, 5] and ci.tolist() == [0, 2, 3, 0, 1] and cmap.tolist() == [1, 2, 0, 4, 3] and v.tolist() == [3.0, 5.0, 2.0, 11.0, 7.0]
    rp, ci, cmap, v = host_csr_extract(3, 4, A, rows=[2, 0], colmap=[1, -1, 5, 0], nc=6)
    assert rp.tolist() == [0, 1, 4] and ci.tolist() == [1, 0, 1, 5] and cmap.tolist() == [4, 0, 1, 2]
    rp, ci, cmap, v = host_csr_extract(3, 4, A, rows=[2, 0], colmap=[1, -1, 5, 0], nc=6, diag_lo=0, diag_hi=0)  # the band in C's own indices
    assert rp.tolist() == [0, 0, 1] and ci.tolist() == [1] and cmap.tolist() == [1] and v.tolist() == [3.0]
    # a row that repeats a column: the ties stay in ascending position of A
    R = (np.array([0, 5], np.int32), np.array([2, 0, 2, 0, 2], np.int32), np.array([1.0, 2.0, 3.0, 4.0, 5.0]))
    rp, ci, cmap, v = host_csr_extract(1, 3, R)
    assert ci.tolist() == [0, 0, 2, 2, 2] and cmap.tolist() == [1, 3, 0, 2, 4]
    # the bits are copied
    Z = (np.array([0, 2], np.int32), np.array([1, 0], np.int32), np.array([-0.0, np.nan]))
    v = host_csr_extract(1, 2, Z)[3]
    assert np.isnan(v[0]) and v[1] == 0 and np.signbit(v[1])


def shuffle_rows(A, rng):
    """The same matrix with the entries of every row in a random order."""
    rp, ci, v = A
    row = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    order = np.lexsort((rng.random(ci.size), row))
    return rp, ci[order], v[order]


def test_host_model_against_scipy():
    sp = pytest.importorskip("scipy.sparse")
    rng = np.random.default_rng(22)
    for m, n, count in ((60, 70, 500), (300, 200, 3000), (50, 50, 300)):
        A = random_sorted_csr(m, n, count, rng)
        S = sp.csr_matrix((A[2], A[1], A[0]), shape=(m, n))
        for rows, cols, nc in selections(m, n, rng):
            if rows is not None and rows.size == 0:
                continue
            rp, ci, cmap, v = host_csr_extract(m, n, shuffle_rows(A, rng), rows, colmap_of(n, cols), None if cols is None else cols.size)
            want = S[np.arange(m) if rows is None else rows][:, np.arange(n) if cols is None else cols].tocsr()
            want.sort_indices()
            assert np.array_equal(want.indptr, rp) and np.array_equal(want.indices, ci) and same_bits(want.data, v)
        for lo, hi, ref in ((None, 0, sp.tril(S, 0)), (None, -1, sp.tril(S, -1)), (1, None, sp.triu(S, 1)), (0, 0, sp.tril(sp.triu(S, 0), 0)),
                            (-2, 3, sp.tril(sp.triu(S, -2), 3))):
            want = ref.tocsr()
            want.sort_indices()
            rp, ci, cmap, v = host_csr_extract(m, n, A, diag_lo=lo, diag_hi=hi)
            assert np.array_equal(want.indptr, rp) and np.array_equal(want.indices, ci) and same_bits(want.data, v), (lo, hi)
