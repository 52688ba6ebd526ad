"""CPU side of the device CSR SpGEMM C = A * B (no GPU): the C ABI declares and exports the three entries, they and the Python wrappers refuse
bad arguments before any launch, the compiled kernels use no scratch, no atomic and no fused multiply-add and the values kernel fits 64 VGPRs,
every size-selected branch of the new code names the GPU tests that cross it, the engine file stays stateless, and the definition of the product
-- expansion order, one stable sort, the assembly's summation order on rounded products -- is restated here in numpy (host_spgemm, exported to the
GPU suite as its reference) and checked against a dense product and, where it is installed, scipy.sparse."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import spmv_acc_amd
from test_coo_host import HELPERS, LONG_RUN, SHARED, _FakeTensor, _f, _i, coo_sum_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "spmv_acc_amd/csrc/"
NEW_SOURCES = ("spgemm.hpp", "k_spgemm.hip", "spgemm.cpp")
GPU = "test_product_is_the_host_model"

# (rule, file, regex that must match the source, GPU tests of tests/test_gpu_spgemm.py that cross it at test size, what it selects)
SPGEMM_SIZE_RULES = [
    ("kSpgemmPerLane", CSRC + "spgemm.hpp", r"constexpr int kSpgemmPerLane = 4;",
     [GPU], "values pass: C entries per lane (products of fewer than 4 * 64 entries leave lanes and steps empty: one_by_one, long_runs)"),
    ("kSpgemmWaveChunk", CSRC + "spgemm.hpp", r"constexpr int kSpgemmWaveChunk = 64 \* kSpgemmPerLane;",
     [GPU], "entries per wavefront: 256; the last wavefront of a product is partly empty"),
    ("kSpgemmTile", CSRC + "spgemm.hpp", r"constexpr int kSpgemmTile = 4 \* kSpgemmWaveChunk;",
     [GPU, "test_spgemm_grid_stride_at_test_size"], "entries per workgroup: 1 024; blocks stride over the tiles beyond the grid"),
    ("kSpgemmExpandPerLane", CSRC + "spgemm.hpp", r"constexpr int kSpgemmExpandPerLane = 4;",
     [GPU], "expansion: products per lane (one_by_one: one lane, one product)"),
    ("kSpgemmExpandChunk", CSRC + "spgemm.hpp", r"constexpr int kSpgemmExpandChunk = 64 \* kSpgemmExpandPerLane;",
     [GPU], "products per wavefront: 256 -- inside one row of B (hub_row_of_B: no search below the wavefront's), across about 28 non-zeros of A "
            "(quads_squared), across non-zeros without products (empty_meets)"),
    ("kSpgemmExpandTile", CSRC + "spgemm.hpp", r"constexpr int kSpgemmExpandTile = 4 \* kSpgemmExpandChunk;",
     [GPU, "test_spgemm_grid_stride_at_test_size"], "products per workgroup: 1 024; a B row of 20 000 entries is 20 tiles"),
    ("tile loop of the expansion", CSRC + "k_spgemm.hip", r"for \(long long tile = blockIdx\.x; tile < ntiles; tile \+= gridDim\.x\) \{ // \(block-uniform\)\n    const long long base = tile \* kSpgemmExpandTile",
     ["test_spgemm_grid_stride_at_test_size"], "blocks stride over the tiles of products beyond the grid"),
    ("tile loop of the values pass", CSRC + SHARED, r"for \(long long tile = blockIdx\.x; tile < ntiles; tile \+= gridDim\.x\) \{ // \(block-uniform\)\n    const long long base = tile \* tile_items",
     ["test_spgemm_grid_stride_at_test_size"], "blocks stride over the tiles of C entries beyond the grid"),
    ("tile loop of the values pass: the product's tile", CSRC + "k_spgemm.hip", r"kSpgemmTile == \(kThreads / kWave\) \* kSpgemmWaveChunk,\n +\"sum_runs derives",
     ["test_spgemm_grid_stride_at_test_size"], "the shared loop's tile is the launcher's kSpgemmTile"),
    ("kMaxGridBlocks (grid striding)", CSRC + SHARED, r"const long long cap = max_grid_blocks\(\);",
     ["test_spgemm_grid_stride_at_test_size"], "every kernel of the three entries strides over the work beyond max_grid_blocks() workgroups"),
    ("kMaxGridBlocks (grid striding): the product's call", CSRC + "k_spgemm.hip", r"dim3\(grid_for\(nnz_c, kSpgemmTile\)\)",
     ["test_spgemm_grid_stride_at_test_size"], "the launchers of the three entries take the shared grid"),
    ("long runs leave the lane pass", CSRC + SHARED, r"len\[k\] = l > kCooLongRun \? -l : l;",
     [GPU, "test_values_follow_new_factors"], "a run of 65 or more products is summed by the wavefront, one run at a time (long_runs: 64, 65, 5 000)"),
    ("long runs leave the lane pass: the product's call", CSRC + "k_spgemm.hip", r"sum_runs<kSpgemmPerLane>\(nprod, nnz_c, start, SpgemmTerms\{pa, pb, a_value, b_value\}, value\);",
     [GPU, "test_values_follow_new_factors"], "the values pass is the shared body on the product's terms"),
    ("four products per step of a long run", CSRC + SHARED, r"for \(; p \+ 3 \* kWave < end; p \+= 4 \* kWave\)",
     [GPU], "long runs: steps of four products per lane, then single ones (65: neither, 5 000: both)"),
    ("four products per step of a long run: the product's fetch", CSRC + "k_spgemm.hip", r"__device__ __forceinline__ double fetch\(int p\) const \{",
     [GPU], "what a lane of the long-run path fetches per position: two index loads, two gathers, one rounded product"),
    ("count sizes", CSRC + "k_spgemm.hip", r"rocprim::reduce\(tmp, \*tmp_bytes, count, total, 0LL, static_cast<size_t>\(nnz_a\),",
     [GPU, "test_spgemm_contract"], "the library reduction over 1 ... 800 000 counts, 64-bit: a total of 2.5e9 is a number"),
    ("scan sizes", CSRC + "k_spgemm.hip", r"rocprim::exclusive_scan\(tmp, \*tmp_bytes, count, off, 0LL, static_cast<size_t>\(nnz_a\) \+ 1,",
     [GPU], "the library scan over 2 ... 800 001 counts, 64-bit"),
    ("no products", CSRC + "spgemm.cpp", r"if \(nprod == 0\) return leave\(no_products\(\)\);",
     [GPU, "test_spgemm_contract"], "A only meets empty rows of B (empty_meets, second pair): c_rowptr zeroed, nothing else written"),
    ("no non-zeros", CSRC + "spgemm.cpp", r"if \(!has_a \|\| nnz_a <= 0 \|\| nnz_b <= 0\) return no_products\(\);",
     ["test_spgemm_contract"], "an empty A or B: nothing is allocated"),
    ("workspace with / without the map", CSRC + "spgemm.cpp", r"off_pb = off_pa \+ \(d_pa \? 0 : ints\)",
     [GPU], "pa == pb == start == NULL: the map lives in the workspace (28 B instead of 16 B per product)"),
    ("map pass only when something reads it", CSRC + "spgemm.cpp", r"if \(d_pa \|\| d_c_value\) launch_spgemm_map\(",
     [GPU], "structure only and no map: the sorted order is dropped unread"),
    ("kEntryAlign", CSRC + HELPERS, r"constexpr size_t kEntryAlign = 256;",
     [GPU], "workspace parts are padded to 256 B (counts that are no multiple of 64: most cases)"),
    ("int32 block arithmetic", CSRC + HELPERS, r"inline bool too_large\(long long v\) \{ return v > INT_MAX - \(1 << 16\); \}",
     ["test_spgemm_contract"], "m, k, n, nnz_a, nnz_b or the product count beyond this: SPMV_ACC_ERR_TOO_LARGE, as the other entries"),
    ("key bits from m and n", CSRC + "spgemm.cpp", r"key_bits = coo_index_bits\(m\) \+ col_bits;",
     [GPU], "radix-sort passes follow the shape of C: 1 x 1 sorts 2 bits, 70 000 x 70 000 sorts 34 (more than 32), 200 000 x 100 000 sorts 35"),
]


def test_spgemm_size_rules_name_their_tests():
    gpu_tests = open(os.path.join(ROOT, "tests", "test_gpu_spgemm.py")).read()
    defined = set(re.findall(r"^def (test_\w+)\(", gpu_tests, flags=re.M))
    for name, path, pattern, tests, what in SPGEMM_SIZE_RULES:
        assert re.search(pattern, open(os.path.join(ROOT, path)).read()), f"{name}: no longer matches {path}: {pattern}"
        assert tests and what
        for t in tests:
            assert t in defined, f"{name}: names {t}, which is not a test of tests/test_gpu_spgemm.py"
    # every named constant of the new files is registered above (tests/size_thresholds.py does not scan them)
    registered = " ".join(r[0] + " " + r[2] for r in SPGEMM_SIZE_RULES)
    for f in NEW_SOURCES:
        for k in re.findall(r"constexpr\s+[\w:<> ]+?\s+(k[A-Z]\w*)\s*=", open(os.path.join(ROOT, CSRC, f)).read()):
            assert k in registered, f"{f}: constant {k} is not in SPGEMM_SIZE_RULES"
    assert f"constexpr int kCooLongRun = {LONG_RUN};" in open(os.path.join(ROOT, CSRC, "coo.hpp")).read()  # the switch is the assembly's


def test_spgemm_entries_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "spmv_acc.h")).read()
    assert re.search(r"int spmv_acc_csr_spgemm_products\(int m, int k, int nnz_a, const int \*d_a_rowptr, const int \*d_a_colindex,\s*"
                     r"const int \*d_b_rowptr, long long \*h_nprod\);", header)
    assert re.search(r"int spmv_acc_csr_spgemm\(int m, int k, int n,\s*"
                     r"int nnz_a, const int \*d_a_rowptr, const int \*d_a_colindex, const double \*d_a_value,\s*"
                     r"int nnz_b, const int \*d_b_rowptr, const int \*d_b_colindex, const double \*d_b_value,\s*"
                     r"int nprod, int \*d_c_rowptr, int \*d_c_colindex, double \*d_c_value,\s*"
                     r"int \*d_pa, int \*d_pb, int \*d_start, int \*h_nnz\);", header)
    assert re.search(r"int spmv_acc_csr_spgemm_values\(int nprod, int nnz_c, const int \*d_pa, const int \*d_pb, const int \*d_start,\s*"
                     r"const double \*d_a_value, const double \*d_b_value, double \*d_c_value\);", header)
    assert header.count("replaces: nothing in the reference") >= 3
    lib = spmv_acc_amd.load_library()
    for s in ("spmv_acc_csr_spgemm_products", "spmv_acc_csr_spgemm", "spmv_acc_csr_spgemm_values"):
        assert s in spmv_acc_amd.C_ABI_SYMBOLS and hasattr(lib, s), s
    for f in ("csr_spgemm_products", "csr_spgemm", "csr_spgemm_values"):
        assert callable(getattr(spmv_acc_amd, f))
    for f in ("k_spgemm.hip", "spgemm.cpp"):  # both builds compile the new files
        assert f in open(os.path.join(ROOT, CSRC, "Makefile")).read() and f in open(os.path.join(ROOT, "CMakeLists.txt")).read(), f
    assert "spgemm.hpp" in open(os.path.join(ROOT, CSRC, "Makefile")).read()


BAD, TOO_LARGE = 2, 4  # SPMV_ACC_ERR_BAD_ARGUMENT, SPMV_ACC_ERR_TOO_LARGE


def test_bad_arguments_are_refused_without_a_gpu():
    """The C entries check their arguments before they touch the device: the error codes come back on a machine without one."""
    lib = spmv_acc_amd.load_library()
    one = 8  # (never dereferenced: a non-null pointer value)
    h = ctypes.byref(ctypes.c_int(-5))
    hp = ctypes.c_longlong(-5)
    count, product, values = lib.spmv_acc_csr_spgemm_products, lib.spmv_acc_csr_spgemm, lib.spmv_acc_csr_spgemm_values

    def prod(m=4, k=4, n=4, nnz_a=4, arp=one, aci=one, av=one, nnz_b=4, brp=one, bci=one, bv=one, nprod=4, crp=one, cci=one, cv=one, pa=one,
             pb=one, st=one, hn=h):
        return product(m, k, n, nnz_a, arp, aci, av, nnz_b, brp, bci, bv, nprod, crp, cci, cv, pa, pb, st, hn)

    for neg in ("m", "k", "n", "nprod"):
        assert prod(**{neg: -1}) == BAD, neg
    assert prod(crp=None) == BAD and prod(hn=None) == BAD
    for mix in (dict(av=None), dict(bv=None), dict(cv=None), dict(av=None, bv=None), dict(av=None, cv=None), dict(bv=None, cv=None)):
        assert prod(**mix) == BAD, mix  # values: all three or none
    for mix in (dict(pa=None), dict(pb=None), dict(st=None), dict(pa=None, pb=None), dict(pa=None, st=None), dict(pb=None, st=None)):
        assert prod(**mix) == BAD, mix  # the map: all three or none
    for null in ("arp", "aci", "brp", "bci", "cci"):
        assert prod(**{null: None}) == BAD, null
        assert prod(**{null: None}, nnz_a=-1, nnz_b=-1) == BAD, null  # (sizes to be read from the device: not before the pointers are checked)
    assert b"spmv_acc_csr_spgemm:" in lib.spmv_acc_last_error_string()
    for big in (2 ** 31 - 1, 2 ** 31 - 2 ** 16):
        for which in ("m", "k", "n", "nnz_a", "nnz_b", "nprod"):
            assert prod(**{which: big}) == TOO_LARGE, which
        assert b"row ranges of A" in lib.spmv_acc_last_error_string()
        assert count(big, 4, 4, one, one, one, ctypes.byref(hp)) == TOO_LARGE and count(4, big, 4, one, one, one, ctypes.byref(hp)) == TOO_LARGE
        assert count(4, 4, big, one, one, one, ctypes.byref(hp)) == TOO_LARGE
        assert values(big, 4, one, one, one, one, one, one) == TOO_LARGE
    assert count(-1, 4, 4, one, one, one, ctypes.byref(hp)) == BAD and count(4, -1, 4, one, one, one, ctypes.byref(hp)) == BAD
    assert count(4, 4, 4, None, one, one, ctypes.byref(hp)) == BAD and count(4, 4, 4, one, None, one, ctypes.byref(hp)) == BAD
    assert count(4, 4, 4, one, one, None, ctypes.byref(hp)) == BAD and count(4, 4, 4, one, one, one, None) == BAD
    assert b"spmv_acc_csr_spgemm_products" in lib.spmv_acc_last_error_string() and hp.value == -5
    assert values(-1, 0, one, one, one, one, one, one) == BAD and values(4, -1, one, one, one, one, one, one) == BAD
    assert values(4, 5, one, one, one, one, one, one) == BAD  # more entries than products
    for null in range(6):
        assert values(4, 4, *[None if i == null else one for i in range(6)]) == BAD, null
    assert b"spmv_acc_csr_spgemm_values" in lib.spmv_acc_last_error_string()
    assert values(0, 0, None, None, None, None, None, None) == 0 and values(4, 0, None, None, None, None, None, None) == 0
    assert lib.spmv_acc_last_error() == 0
    try:  # the deterministic switch refuses nothing here
        assert lib.spmv_acc_set_tunable(b"deterministic", 1) == 0
        assert values(0, 0, None, None, None, None, None, None) == 0
    finally:
        lib.spmv_acc_reset_tunables()
        lib.spmv_acc_clear_error()


def test_wrappers_refuse_bad_arguments():
    E = spmv_acc_amd.SpmvAccError
    m, k, n, nnz_a, nnz_b, nprod, nnz_c = 10, 12, 9, 30, 40, 100, 70
    good = dict(arp=_i(m + 1), aci=_i(nnz_a), av=_f(nnz_a), brp=_i(k + 1), bci=_i(nnz_b), bv=_f(nnz_b))

    def product(match, mm=m, kk=k, nn=n, **bad):
        a = dict(good, **bad)
        with pytest.raises(E, match=match):
            spmv_acc_amd.csr_spgemm(mm, kk, nn, a["arp"], a["aci"], a["av"], a["brp"], a["bci"], a["bv"], want_map=True)

    product("not on the GPU", bci=_i(nnz_b, cuda=False))
    product("dtype", arp=_FakeTensor(m + 1, dtype="torch.int64"))
    product("dtype", aci=_f(nnz_a))
    product("dtype", brp=_f(k + 1))
    product("dtype", bci=_f(nnz_b))
    product("dtype", av=_i(nnz_a))
    product("dtype", bv=_i(nnz_b))
    product("not contiguous", bv=_f(nnz_b, contiguous=False))
    product("elements", arp=_i(m))
    product("elements", brp=_i(k))
    product("elements", av=_f(nnz_a - 1))
    product("elements", bv=_f(nnz_b - 1))
    product("as many", av=_f(nnz_a + 1))
    product("as many", bv=_f(nnz_b + 1))
    product("both", av=None)
    product("both", bv=None)
    product("on cuda:1", bv=_f(nnz_b, device="cuda:1"))
    product("torch tensor", arp=None)
    product("torch tensor", aci=[0] * nnz_a)
    product("torch tensor", brp=None)
    product("torch tensor", bci=None)
    product("torch tensor", av=3.0)
    product("negative", mm=-1)
    product("negative", kk=-2)
    product("negative", nn=-3)

    def count(match, mm=m, kk=k, arp=_i(m + 1), aci=_i(nnz_a), brp=_i(k + 1)):
        with pytest.raises(E, match=match):
            spmv_acc_amd.csr_spgemm_products(mm, kk, arp, aci, brp)

    count("dtype", aci=_f(nnz_a))
    count("elements", brp=_i(k))
    count("not on the GPU", arp=_i(m + 1, cuda=False))
    count("torch tensor", brp=None)
    count("negative", mm=-1)

    def values(match, pa=_i(nprod), pb=_i(nprod), start=_i(nnz_c + 1), av=_f(nnz_a), bv=_f(nnz_b), out=_f(nnz_c)):
        with pytest.raises(E, match=match):
            spmv_acc_amd.csr_spgemm_values(pa, pb, start, av, bv, out)

    values("dtype", pa=_f(nprod))
    values("dtype", pb=_f(nprod))
    values("dtype", start=_f(nnz_c + 1))
    values("dtype", av=_i(nnz_a))
    values("dtype", out=_i(nnz_c))
    values("elements", pb=_i(nprod - 1))
    values("elements", out=_f(nnz_c - 1))
    values("elements", start=_i(0))
    values("elements", bv=_f(0))
    values("not on the GPU", av=_f(nnz_a, cuda=False))
    values("not contiguous", pa=_i(nprod, contiguous=False))
    values("on cuda:1", out=_f(nnz_c, device="cuda:1"))
    values("torch tensor", pa=None)
    values("torch tensor", bv=None)
    values("torch tensor", out=None)


def test_spgemm_entries_keep_no_state():
    """As test_coo_entries_keep_no_state: the engine file neither finds nor makes a plan, counts no plan work and keeps nothing static; the one
    allocation (the count entry and the main entry are one routine) is freed on every way out; the values entry is launch-only."""
    src = open(os.path.join(ROOT, CSRC, "spgemm.cpp")).read()
    code = re.sub(r"//[^\n]*", "", src)
    for word in ("get_plan", "g_plans", "t_plan_work", "t_last_plan", "tune_", "TimingPhase", "TuneTimer", "static std::", "thread_local"):
        assert word not in code, word
    assert not re.search(r"\bstatic\b(?! const char \*const kEntry)", code), "a static other than the entries' names"
    assert code.count("hipMalloc(") == 1 and code.count("hipFree(") == 1 and "const auto leave = " in code
    after = code.split("hipMalloc(")[1].split("\n}\n")[0]  # (to the end of the routine that allocates)
    assert "launch_spgemm_expand" in after and "launch_spgemm_values" in after
    assert not re.search(r"return (?!leave\()", after.split("const auto leave = ")[1].split("};", 1)[1]), "a way out of the product that skips leave()"
    values = code.split("int run_csr_spgemm_values")[1]
    assert "hipMalloc" not in values and "Synchronize" not in values and "hipMemcpy" not in values  # launch-only: capturable
    assert "g_tunables" not in code  # (no tunable is read: `deterministic` changes nothing)


def test_spgemm_kernels_fit_their_register_budget(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_table

    asm = tmp_path / "k_spgemm.s"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-DKERNEL_STRATEGY_ADAPTIVE",
                        "-I" + os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-S",
                        os.path.join(ROOT, CSRC, "k_spgemm.hip"), "-o", str(asm)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    text = asm.read_text()
    bodies = {}
    for mt in re.finditer(r"^(_ZN8spmv_acc\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, flags=re.M | re.S):
        bodies[mt.group(1)] = mt.group(2)
    assert len(bodies) == 4, sorted(bodies)
    for k, b in bodies.items():
        assert "atomic" not in b, k  # no atomics anywhere: the sums and the counts are pure functions of the input
        # every product is rounded before it is added: a fused multiply-add would round once where the definition rounds twice
        assert "v_fma_f64" not in b and "v_fmac_f64" not in b and "v_pk_fma" not in b, k
    values_body = next(b for k, b in bodies.items() if "spgemm_values_kernel" in k)
    assert "v_mul_f64" in values_body and "v_add_f64" in values_body
    rows = [k for k in resource_table.parse(r.stderr) if "rocprim" not in k["name"]]
    names = sorted(k["name"] for k in rows)
    assert names == sorted(["spgemm_counts_kernel", "spgemm_expand_kernel", "spgemm_map_kernel", "spgemm_values_kernel"]), names
    for k in rows:
        assert k["scratch"] == 0 and k["agprs"] == 0, k
        # as found when the kernels were written: 54 VGPRs for the values pass (four runs with two indices and two gathers each in flight), counts
        # 11, map 16, expansion 26
        assert k["vgprs"] <= (64 if k["name"] == "spgemm_values_kernel" else 32) and k["occupancy"] >= 8, k
    # (rocPRIM's reduction and scan kernels are instantiated in the same file and are not held to this)


# ---- the definition of the product (include/spmv_acc.h, spgemm.hpp), in numpy: the GPU suite's reference ------------------------------------
def host_spgemm(m, k, n, A, B):
    """(rowptr, colindex, pa, pb, start, value) of C = A * B for A = (rowptr, colindex, value | None), m x k, and B likewise, k x n.  Product e
    enumerates A's non-zeros q in storage order and for each the entries t of B's row a_colindex[q] in storage order; one stable sort by
    (row of q, b_colindex[t], e); a run of equal (i, j) is one entry; its value is coo_sum_model's sum of the rounded products a[pa] * b[pb]."""
    a_rp, a_ci, a_v = A
    b_rp, b_ci, b_v = B
    a_rp, b_rp = a_rp.astype(np.int64), b_rp.astype(np.int64)
    nnz_a = a_ci.size
    assert a_rp.size == m + 1 and b_rp.size == k + 1 and a_rp[0] == 0 and b_rp[0] == 0 and a_rp[m] == nnz_a and b_rp[k] == b_ci.size
    a_row = np.repeat(np.arange(m, dtype=np.int64), np.diff(a_rp))
    count = np.diff(b_rp)[a_ci] if nnz_a else np.zeros(0, np.int64)
    off = np.concatenate([[0], np.cumsum(count)])
    nprod = int(off[-1])
    ua = np.repeat(np.arange(nnz_a, dtype=np.int64), count)               # the non-zero of A of product e
    ub = b_rp[a_ci[ua]] + (np.arange(nprod, dtype=np.int64) - off[ua])     # ... and of B
    i, j = a_row[ua], b_ci[ub].astype(np.int64)
    order = np.lexsort((np.arange(nprod), j, i))
    pa, pb = ua[order].astype(np.int32), ub[order].astype(np.int32)
    si, sj = i[order], j[order]
    head = np.ones(nprod, dtype=bool)
    head[1:] = (si[1:] != si[:-1]) | (sj[1:] != sj[:-1])
    start = np.concatenate([np.flatnonzero(head), [nprod]]).astype(np.int32)
    rowptr = np.zeros(m + 1, dtype=np.int32)
    np.cumsum(np.bincount(si[head], minlength=m), out=rowptr[1:])
    value = None
    if a_v is not None:
        products = a_v[pa] * b_v[pb]  # (numpy rounds every product to fp64: no fused multiply-add)
        value = coo_sum_model(np.arange(nprod, dtype=np.int32), start, products)
    return rowptr, sj[head].astype(np.int32), pa, pb, start, value


def random_unsorted_csr(m, n, count, dup_fraction, rng):
    """An m x n CSR of `count` distinct positions plus dup_fraction * count repeated ones (separate entries), every row in shuffled order."""
    pos = rng.choice(m * n, size=count, replace=False)
    pos = np.concatenate([pos, rng.choice(pos, size=int(dup_fraction * count), replace=True)])
    row, col = (pos // n).astype(np.int32), (pos % n).astype(np.int32)
    o = np.lexsort((rng.random(row.size), row))  # rows ascend, the order inside a row is random
    rowptr = np.zeros(m + 1, dtype=np.int32)
    np.cumsum(np.bincount(row, minlength=m), out=rowptr[1:])
    return rowptr, col[o].copy(), rng.standard_normal(row.size) * 10.0 ** rng.integers(-2, 3, row.size)


def dense_of(m, n, csr, dtype, absolute=False):
    rp, ci, v = csr
    d = np.zeros((m, n), dtype=dtype)
    np.add.at(d, (np.repeat(np.arange(m), np.diff(rp)), ci), np.abs(v) if absolute else v.astype(dtype))
    return d


def test_host_model_against_a_dense_product():
    rng = np.random.default_rng(5)
    for m, k, n, ca, cb, dup in ((40, 30, 50, 300, 400, 0.05), (7, 90, 5, 400, 300, 0.2), (1, 1, 1, 1, 1, 0.0), (30, 20, 25, 0, 100, 0.0)):
        A, B = random_unsorted_csr(m, k, ca, dup, rng), random_unsorted_csr(k, n, cb, dup, rng)
        rp, ci, pa, pb, start, v = host_spgemm(m, k, n, A, B)
        # structure, exact: the pattern is the set of positions with at least one product; rows strictly ascending
        pattern = (dense_of(m, k, (A[0], A[1], np.ones(A[1].size)), np.float64) @ dense_of(k, n, (B[0], B[1], np.ones(B[1].size)), np.float64)) > 0
        got = np.zeros((m, n), dtype=bool)
        rows = np.repeat(np.arange(m), np.diff(rp))
        got[rows, ci] = True
        assert np.array_equal(got, pattern) and ci.size == int(pattern.sum()) == start.size - 1
        assert all(np.all(np.diff(ci[rp[r]:rp[r + 1]]) > 0) for r in range(m))
        assert start[0] == 0 if ci.size else start.tolist() == [0]
        assert int(start[-1]) == pa.size == pb.size == int(np.diff(B[0].astype(np.int64))[A[1]].sum())
        # every product once, at its entry
        a_row = np.repeat(np.arange(m), np.diff(A[0]))
        entry = np.repeat(np.arange(ci.size), np.diff(start))
        assert np.array_equal(a_row[pa], rows[entry]) and np.array_equal(B[1][pb], ci[entry])
        b_row = np.repeat(np.arange(k), np.diff(B[0]))
        assert np.array_equal(A[1][pa], b_row[pb])
        assert np.unique(pa.astype(np.int64) * max(B[1].size, 1) + pb).size == pa.size
        # values, entrywise within the summation bound of their terms.  The dense product is formed in extended precision (its own error is
        # 2^-11 of fp64's and is not counted); a sum of t rounded products errs by at most gamma_t * sum |a| |b|, gamma_t = t u / (1 - t u),
        # u = 2^-53 (t - 1 additions and one rounding per product)
        exact = dense_of(m, k, A, np.longdouble) @ dense_of(k, n, B, np.longdouble)
        scale = dense_of(m, k, A, np.float64, absolute=True) @ dense_of(k, n, B, np.float64, absolute=True)
        t = np.diff(start).astype(np.float64)
        gamma = t * 2.0 ** -53 / (1.0 - t * 2.0 ** -53)
        err = np.abs(v.astype(np.longdouble) - exact[rows, ci]).astype(np.float64)
        assert np.all(err <= gamma * scale[rows, ci]), float((err / (gamma * scale[rows, ci])).max())
        # structure only
        s = host_spgemm(m, k, n, (A[0], A[1], None), (B[0], B[1], None))
        assert s[5] is None and all(np.array_equal(x, y) for x, y in zip(s[:5], (rp, ci, pa, pb, start)))
    # by hand: A = [[a0 a1], [0 a2]] stored with row 0 as columns (1, 0); B = [[b0 0], [b1 b2]] with row 1 as columns (1, 0)
    A = (np.array([0, 2, 3], np.int32), np.array([1, 0, 1], np.int32), np.array([2.0, 3.0, 5.0]))
    B = (np.array([0, 1, 3], np.int32), np.array([0, 1, 0], np.int32), np.array([7.0, 11.0, 13.0]))
    rp, ci, pa, pb, start, v = host_spgemm(2, 2, 2, A, B)
    # products in expansion order: e0 = A[0]*B[1] -> (0,1); e1 = A[0]*B[2] -> (0,0); e2 = A[1]*B[0] -> (0,0); e3 = A[2]*B[1] -> (1,1); e4 = A[2]*B[2] -> (1,0)
    assert rp.tolist() == [0, 2, 4] and ci.tolist() == [0, 1, 0, 1] and start.tolist() == [0, 2, 3, 4, 5]
    assert pa.tolist() == [0, 1, 0, 2, 2] and pb.tolist() == [2, 0, 1, 2, 1]
    assert v.tolist() == [2.0 * 13.0 + 3.0 * 7.0, 2.0 * 11.0, 5.0 * 13.0, 5.0 * 11.0]
    # the sign of zero is kept: the sum starts from the first product, not from +0.0
    one = np.array([0, 1], np.int32), np.array([0], np.int32)
    assert np.signbit(host_spgemm(1, 1, 1, one + (np.array([-0.0]),), one + (np.array([3.0]),))[5][0])


def test_host_model_against_scipy():
    sp = pytest.importorskip("scipy.sparse")
    rng = np.random.default_rng(6)
    for m, k, n, ca, cb in ((60, 45, 70, 500, 600), (300, 500, 200, 3000, 2500)):
        A, B = random_unsorted_csr(m, k, ca, 0.05, rng), random_unsorted_csr(k, n, cb, 0.05, rng)
        rp, ci, pa, pb, start, v = host_spgemm(m, k, n, A, B)
        C = sp.csr_matrix((A[2], A[1], A[0]), shape=(m, k)) @ sp.csr_matrix((B[2], B[1], B[0]), shape=(k, n))
        C.sort_indices()
        assert np.array_equal(C.indptr, rp) and np.array_equal(C.indices, ci)
        S = sp.csr_matrix((np.abs(A[2]), A[1], A[0]), shape=(m, k)) @ sp.csr_matrix((np.abs(B[2]), B[1], B[0]), shape=(k, n))
        S.sort_indices()
        t = np.diff(start).astype(np.float64)  # both sides sum the same t rounded products, in their own order: twice the bound of one
        assert np.all(np.abs(C.data - v) <= 2.0 * t * 2.0 ** -53 / (1.0 - t * 2.0 ** -53) * S.data)
