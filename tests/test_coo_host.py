"""CPU side of the device COO -> CSR assembly (no GPU): the C ABI declares and exports the two entries, they and the Python wrappers refuse bad
arguments before any launch, the compiled kernels fit their register budget, every size-selected branch of the new code names the GPU tests that
cross it, the engine file stays stateless, and the documented summation order -- restated here in numpy and exported to the GPU suite as its
reference -- is a sequential loop for short runs and within the standard error bound of a k-term sum for all of them."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import spmv_acc_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "spmv_acc_amd/csrc/"
NEW_SOURCES = ("coo.hpp", "k_coo.hip", "coo.cpp")
SHARED = "structure_passes.hpp"  # what the structure-pass kernel files share: the other features' tables name it too
HELPERS = "entry_helpers.hpp"  # what the entry files share on the host: the other features' tables name it too (test_gs_host.py holds it to its list)
LONG_RUN = 64  # kCooLongRun (test_coo_size_rules_name_their_tests holds the two together)

# (rule, file, regex that must match the source, GPU tests of tests/test_gpu_coo.py that cross it at test size, what it selects)
COO_SIZE_RULES = [
    ("kCooLongRun", CSRC + "coo.hpp", r"constexpr int kCooLongRun = 64;",
     ["test_assembly_is_the_host_stable_sort", "test_reassembly_follows_new_values"],
     "runs of up to 64 triples are summed by one lane, longer ones by a wavefront (runs of 1, 2, 4, 64, 65 and 5 000 in the suite)"),
    ("kCooPerLane", CSRC + "coo.hpp", r"constexpr int kCooPerLane = 6;",
     ["test_assembly_is_the_host_stable_sort", "test_coo_contract"],
     "summing pass: CSR entries per lane (matrices of fewer than 6 * 64 entries leave lanes and steps empty: the single triple, the 1 x 1 matrix)"),
    ("kCooWaveChunk", CSRC + "coo.hpp", r"constexpr int kCooWaveChunk = 64 \* kCooPerLane;",
     ["test_assembly_is_the_host_stable_sort"], "entries per wavefront: 384; the last wavefront of a matrix is partly empty"),
    ("kCooTile", CSRC + "coo.hpp", r"constexpr int kCooTile = 4 \* kCooWaveChunk;",
     ["test_assembly_is_the_host_stable_sort", "test_coo_grid_stride_at_test_size"], "entries per workgroup: 1 536; blocks stride over the tiles beyond the grid"),
    ("kCooCheckBlocks", CSRC + "coo.hpp", r"constexpr int kCooCheckBlocks = 1024;",
     ["test_assembly_is_the_host_stable_sort", "test_coo_contract"],
     "range census: at most 1 024 workgroups (more than 1 Mi triples stride: the 3.2 M case), one count slot per wavefront"),
    ("kCooCheckSlots", CSRC + "coo.hpp", r"constexpr int kCooCheckSlots = 4 \* kCooCheckBlocks;",
     ["test_coo_contract"], "the host adds up every slot, written or not (small inputs leave most at zero)"),
    ("kMaxGridBlocks (grid striding)", CSRC + SHARED, r"const long long cap = max_grid_blocks\(\);",
     ["test_coo_grid_stride_at_test_size"], "every kernel of the two entries strides over the work beyond max_grid_blocks() workgroups"),
    ("kMaxGridBlocks (grid striding): the assembly's call", CSRC + "k_coo.hip", r"dim3\(grid_for\(nnz, kCooTile\)\)",
     ["test_coo_grid_stride_at_test_size"], "the launchers of the two entries take the shared grid"),
    ("tile loop of the summing pass", CSRC + SHARED, r"for \(long long tile = blockIdx\.x; tile < ntiles; tile \+= gridDim\.x\)",
     ["test_coo_grid_stride_at_test_size"], "blocks stride over the tiles of CSR entries beyond the grid"),
    ("tile loop of the summing pass: the assembly's tile", CSRC + "k_coo.hip", r"kCooTile == \(kThreads / kWave\) \* kCooWaveChunk, \"sum_runs derives",
     ["test_coo_grid_stride_at_test_size"], "the shared loop's tile is the launcher's kCooTile"),
    ("long runs leave the lane pass", CSRC + SHARED, r"len\[k\] = l > kCooLongRun \? -l : l;",
     ["test_assembly_is_the_host_stable_sort", "test_reassembly_follows_new_values"], "a run of 65 or more is summed by the wavefront, one run at a time"),
    ("long runs leave the lane pass: the assembly's call", CSRC + "k_coo.hip", r"sum_runs<kCooPerLane>\(nnz_coo, nnz, start, CooTerms\{order, val, nnz_coo\}, value\);",
     ["test_assembly_is_the_host_stable_sort", "test_reassembly_follows_new_values"], "the summing pass is the shared body on the assembly's terms"),
    ("four gathers per step of a long run", CSRC + SHARED, r"for \(; p \+ 3 \* kWave < end; p \+= 4 \* kWave\)",
     ["test_assembly_is_the_host_stable_sort"], "long runs: steps of four values per lane, then single ones (65: neither, 5 000: both)"),
    ("four gathers per step of a long run: the assembly's gather", CSRC + "k_coo.hip", r"__device__ __forceinline__ double fetch\(int p\) const \{",
     ["test_assembly_is_the_host_stable_sort"], "what a lane of the long-run path fetches per position: one checked gather"),
    ("key bits from m and n", CSRC + "coo.hpp", r"while \(bits < 31 && \(1LL << bits\) < n\) \+\+bits;",
     ["test_assembly_is_the_host_stable_sort"], "radix-sort passes follow the shape: 1 x 1 sorts 2 bits, 70 000 x 70 000 sorts 34 (more than 32), 200 000 x 150 000 sorts 36"),
    ("sort size paths", CSRC + "k_coo.hip", r"rocprim::radix_sort_pairs\(tmp, \*tmp_bytes, keys, keys_out, rocprim::counting_iterator<int>\(0\), order,",
     ["test_assembly_is_the_host_stable_sort"], "the library sort picks its algorithm by size: lists of 1 ... 3.2 M triples cross its single-block, merge and multi-pass forms"),
    ("scan size paths", CSRC + "k_coo.hip", r"rocprim::exclusive_scan\(tmp, \*tmp_bytes, head, index, 0, static_cast<size_t>\(nnz_coo\) \+ 1,",
     ["test_assembly_is_the_host_stable_sort"], "the library scan: 2 ... 3.2 M + 1 flags"),
    ("int32 block arithmetic", CSRC + HELPERS, r"inline bool too_large\(long long v\) \{ return v > INT_MAX - \(1 << 16\); \}",
     ["test_coo_contract"], "m, n, nnz_coo or nnz beyond this: SPMV_ACC_ERR_TOO_LARGE, as the other entries"),
    ("workspace with / without the map", CSRC + "coo.cpp", r"off_start = off_order \+ \(d_order \? 0 : ints\)",
     ["test_assembly_is_the_host_stable_sort"], "order == start == NULL: the map lives in the workspace (24 B instead of 16 B per triple)"),
    ("kEntryAlign", CSRC + HELPERS, r"constexpr size_t kEntryAlign = 256;",
     ["test_assembly_is_the_host_stable_sort"], "workspace parts are padded to 256 B (nnz_coo not a multiple of 64: the 8 000-triple case)"),
    ("no triples", CSRC + "coo.cpp", r"if \(nnz_coo == 0\) \{",
     ["test_coo_contract"], "an empty list: rowptr zeroed, nothing allocated"),
]


def test_coo_size_rules_name_their_tests():
    gpu_tests = open(os.path.join(ROOT, "tests", "test_gpu_coo.py")).read()
    defined = set(re.findall(r"^def (test_\w+)\(", gpu_tests, flags=re.M))
    for name, path, pattern, tests, what in COO_SIZE_RULES:
        assert re.search(pattern, open(os.path.join(ROOT, path)).read()), f"{name}: no longer matches {path}: {pattern}"
        assert tests and what
        for t in tests:
            assert t in defined, f"{name}: names {t}, which is not a test of tests/test_gpu_coo.py"
    # every named constant of the new files is registered above (tests/size_thresholds.py does not scan them)
    registered = " ".join(r[0] + " " + r[2] for r in COO_SIZE_RULES)
    for f in NEW_SOURCES + (SHARED,):  # (the shared header holds none today)
        for k in re.findall(r"constexpr\s+[\w:<> ]+?\s+(k[A-Z]\w*)\s*=", open(os.path.join(ROOT, CSRC, f)).read()):
            assert k in registered, f"{f}: constant {k} is not in COO_SIZE_RULES"
    assert f"constexpr int kCooLongRun = {LONG_RUN};" in open(os.path.join(ROOT, CSRC, "coo.hpp")).read()


def test_coo_entries_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "spmv_acc.h")).read()
    assert re.search(r"int spmv_acc_coo_to_csr\(int m, int n, int nnz_coo,\s*const int \*d_row, const int \*d_col, const double \*d_val,\s*"
                     r"int \*d_rowptr, int \*d_colindex, double \*d_value,\s*int \*d_order, int \*d_start, int \*h_nnz\);", header)
    assert re.search(r"int spmv_acc_coo_to_csr_values\(int nnz_coo, int nnz, const int \*d_order, const int \*d_start,\s*"
                     r"const double \*d_val, double \*d_value\);", header)
    lib = spmv_acc_amd.load_library()
    for s in ("spmv_acc_coo_to_csr", "spmv_acc_coo_to_csr_values"):
        assert s in spmv_acc_amd.C_ABI_SYMBOLS and hasattr(lib, s), s
    for f in ("coo_to_csr", "coo_to_csr_values"):
        assert callable(getattr(spmv_acc_amd, f))
    for f in ("k_coo.hip", "coo.cpp"):  # both builds compile the new files
        assert f in open(os.path.join(ROOT, CSRC, "Makefile")).read() and f in open(os.path.join(ROOT, "CMakeLists.txt")).read(), f
    assert "coo.hpp" in open(os.path.join(ROOT, CSRC, "Makefile")).read()


def test_bad_arguments_are_refused_without_a_gpu():
    """The C entries check their arguments before they touch the device: the error codes come back on a machine without one."""
    lib = spmv_acc_amd.load_library()
    one = 8  # (never dereferenced: a non-null pointer value)
    h = ctypes.byref(ctypes.c_int(-5))
    a, v = lib.spmv_acc_coo_to_csr, lib.spmv_acc_coo_to_csr_values
    assert a(-1, 4, 4, one, one, one, one, one, one, one, one, h) == 2
    assert a(4, -1, 4, one, one, one, one, one, one, one, one, h) == 2
    assert a(4, 4, -1, one, one, one, one, one, one, one, one, h) == 2
    assert a(4, 4, 4, one, one, one, None, one, one, one, one, h) == 2   # no rowptr
    assert a(4, 4, 4, one, one, one, one, one, one, one, one, None) == 2  # no h_nnz
    assert a(4, 4, 4, one, one, one, one, one, None, one, one, h) == 2   # val without value
    assert a(4, 4, 4, one, one, None, one, one, one, one, one, h) == 2   # value without val
    assert a(4, 4, 4, one, one, one, one, one, one, one, None, h) == 2   # order without start
    assert a(4, 4, 4, one, one, one, one, one, one, None, one, h) == 2   # start without order
    assert a(4, 4, 4, None, one, one, one, one, one, one, one, h) == 2   # no row
    assert a(4, 4, 4, one, None, one, one, one, one, one, one, h) == 2   # no col
    assert a(4, 4, 4, one, one, one, one, None, one, one, one, h) == 2   # no colindex
    assert a(0, 4, 4, one, one, one, one, one, one, one, one, h) == 2    # triples in a matrix without rows
    assert a(4, 0, 4, one, one, one, one, one, one, one, one, h) == 2
    for big in (2 ** 31 - 1, 2 ** 31 - 2 ** 16):
        assert a(big, 4, 4, one, one, one, one, one, one, one, one, h) == 4
        assert a(4, big, 4, one, one, one, one, one, one, one, one, h) == 4
        assert a(4, 4, big, one, one, one, one, one, one, one, one, h) == 4
        assert v(big, 4, one, one, one, one) == 4
    assert b"spmv_acc_coo_to_csr_values" in lib.spmv_acc_last_error_string()
    assert v(-1, 0, one, one, one, one) == 2 and v(4, -1, one, one, one, one) == 2
    assert v(4, 5, one, one, one, one) == 2  # more distinct positions than triples
    assert v(4, 4, None, one, one, one) == 2 and v(4, 4, one, None, one, one) == 2 and v(4, 4, one, one, None, one) == 2
    assert v(4, 4, one, one, one, None) == 2
    assert v(0, 0, None, None, None, None) == 0 and v(4, 0, None, None, None, None) == 0
    assert lib.spmv_acc_last_error() == 0
    try:  # the deterministic switch refuses nothing here
        assert lib.spmv_acc_set_tunable(b"deterministic", 1) == 0
        assert v(0, 0, None, None, None, None) == 0
    finally:
        lib.spmv_acc_reset_tunables()
        lib.spmv_acc_clear_error()


class _FakeTensor:
    """Enough of a torch tensor for the wrappers' checks to run without a GPU (they never reach the C entries)."""

    def __init__(self, numel, dtype="torch.float64", cuda=True, device="cuda:0", contiguous=True):
        self._numel, self.dtype, self.is_cuda, self.device, self._contiguous = numel, dtype, cuda, device, contiguous

    def numel(self):
        return self._numel

    def is_contiguous(self):
        return self._contiguous

    def data_ptr(self):
        raise AssertionError("the wrapper must refuse before it takes a pointer")


def _i(numel, **kw):
    return _FakeTensor(numel, dtype="torch.int32", **kw)


def _f(numel, **kw):
    return _FakeTensor(numel, **kw)


def test_wrappers_refuse_bad_arguments():
    E = spmv_acc_amd.SpmvAccError
    m, n, k, nnz = 10, 12, 30, 17
    good = dict(row=_i(k), col=_i(k), val=_f(k))

    def assemble(match, mm=m, nn=n, **bad):
        a = dict(good, **bad)
        with pytest.raises(E, match=match):
            spmv_acc_amd.coo_to_csr(mm, nn, a["row"], a["col"], a["val"], want_map=True)

    assemble("not on the GPU", col=_i(k, cuda=False))
    assemble("dtype", row=_FakeTensor(k, dtype="torch.int64"))
    assemble("dtype", col=_f(k))
    assemble("dtype", val=_i(k))
    assemble("not contiguous", val=_f(k, contiguous=False))
    assemble("elements", col=_i(k - 1))
    assemble("elements", val=_f(k - 1))
    assemble("as many", col=_i(k + 1))
    assemble("on cuda:1", val=_f(k, device="cuda:1"))
    assemble("torch tensor", row=None)
    assemble("torch tensor", col=[0] * k)
    assemble("torch tensor", val=3.0)
    assemble("negative", mm=-1)
    assemble("negative", nn=-2)

    def values(match, order=_i(k), start=_i(nnz + 1), val=_f(k), out=_f(nnz)):
        with pytest.raises(E, match=match):
            spmv_acc_amd.coo_to_csr_values(order, start, val, out)

    values("dtype", order=_f(k))
    values("dtype", start=_f(nnz + 1))
    values("dtype", out=_i(nnz))
    values("elements", val=_f(k - 1))
    values("elements", out=_f(nnz - 1))
    values("elements", start=_i(0))
    values("not on the GPU", val=_f(k, cuda=False))
    values("not contiguous", order=_i(k, contiguous=False))
    values("on cuda:1", out=_f(nnz, device="cuda:1"))
    values("torch tensor", order=None)
    values("torch tensor", out=None)


def test_coo_entries_keep_no_state():
    """ADVICE.md's high-severity finding is a plan that silently holds a copy of the caller's values: the engine file of these entries neither
    finds nor makes a plan, counts no plan work and keeps nothing static; the one allocation is freed on every way out."""
    src = open(os.path.join(ROOT, CSRC, "coo.cpp")).read()
    code = re.sub(r"//[^\n]*", "", src)
    for word in ("get_plan", "g_plans", "t_plan_work", "t_last_plan", "tune_", "TimingPhase", "TuneTimer", "static std::", "thread_local"):
        assert word not in code, word
    assert not re.search(r"\bstatic\b(?! const char \*const kEntry)", code), "a static other than the entries' names"
    assert code.count("hipMalloc(") == 1 and code.count("hipFree(") == 1 and "const auto leave = " in code
    after = code.split("hipMalloc(")[1].split("int run_coo_to_csr_values")[0]
    assert not re.search(r"return (?!leave\()", after.split("const auto leave = ")[1].split("};", 1)[1]), "a way out of the assembly that skips leave()"
    values = code.split("int run_coo_to_csr_values")[1]
    assert "hipMalloc" not in values and "Synchronize" not in values and "hipMemcpy" not in values  # launch-only: capturable


def test_coo_kernels_fit_their_register_budget(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_table

    asm = tmp_path / "k_coo.s"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-DKERNEL_STRATEGY_ADAPTIVE",
                        "-I" + os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-S",
                        os.path.join(ROOT, CSRC, "k_coo.hip"), "-o", str(asm)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    text = asm.read_text()
    bodies = {}
    for mt in re.finditer(r"^(_ZN8spmv_acc\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, flags=re.M | re.S):
        bodies[mt.group(1)] = mt.group(2)
    assert len(bodies) == 6, sorted(bodies)
    for k, b in bodies.items():
        assert "atomic" not in b, k  # no atomics anywhere: the sums and the census are pure functions of the input
    rows = [k for k in resource_table.parse(r.stderr) if "rocprim" not in k["name"]]
    names = sorted(k["name"] for k in rows)
    assert names == sorted(["coo_check_kernel", "coo_keys_kernel", "coo_heads_kernel", "coo_entries_kernel", "coo_rowptr_kernel",
                            "coo_values_kernel"]), names
    for k in rows:
        assert k["scratch"] == 0 and k["agprs"] == 0, k
        # as found when the kernels were written: 60 VGPRs for the summing pass (six runs, their order entries and values in flight; eight runs took
        # 80 VGPRs and 6 waves per SIMD), 8 ... 13 elsewhere (check 8, heads 10, rowptr 11, keys and entries 13)
        assert k["vgprs"] <= (64 if k["name"] == "coo_values_kernel" else 16) and k["occupancy"] >= 8, k
    # (rocPRIM's sort and scan kernels are instantiated in the same file and are not held to this)


# ---- the documented summation order (coo.hpp), in numpy: the GPU suite's reference for the values ----------------------------------------
def host_assemble(m, n, row, col):
    """(rowptr, colindex, order, start) of the stable assembly: triples by (row, col, input position), one CSR entry per distinct position."""
    k = row.size
    order = np.lexsort((np.arange(k), col, row)).astype(np.int32)
    r, c = row[order], col[order]
    head = np.ones(k, dtype=bool)
    head[1:] = (r[1:] != r[:-1]) | (c[1:] != c[:-1])
    start = np.concatenate([np.flatnonzero(head), [k]]).astype(np.int32)
    rowptr = np.zeros(m + 1, dtype=np.int32)
    np.cumsum(np.bincount(r[head], minlength=m), out=rowptr[1:])
    return rowptr, c[head].astype(np.int32), order, start


def coo_sum_model(order, start, val):
    """value[j] of the two entries for the map (order, start): runs of up to kCooLongRun values are added one after the other, starting from the
    first; a longer run is dealt to 64 lanes (lane l: values l, l + 64, ... in order, starting from its first), and the 64 partial sums are
    combined as a balanced tree over neighbours.  A run is clamped to [0, len(order)]; an order entry outside [0, len(val)) counts as +0.0."""
    k = order.size
    lo = np.clip(start[:-1].astype(np.int64), 0, k)
    hi = np.maximum(np.clip(start[1:].astype(np.int64), 0, k), lo)
    ok = (order >= 0) & (order < val.size)
    seq = np.where(ok, val[np.where(ok, order, 0)], 0.0)  # the values in sorted order
    length = hi - lo
    out = np.zeros(length.size)
    short = np.flatnonzero((length > 0) & (length <= LONG_RUN))
    out[short] = seq[lo[short]]
    for t in range(1, int(length[short].max()) if short.size else 0):  # round t adds every short run's t-th value: sequential per run
        live = short[length[short] > t]
        out[live] = out[live] + seq[lo[live] + t]
    for j in np.flatnonzero(length > LONG_RUN):
        v = seq[lo[j]:hi[j]]
        part = v[:64].copy()
        for i in range(64, v.size, 64):
            chunk = v[i:i + 64]
            part[:chunk.size] = part[:chunk.size] + chunk
        while part.size > 1:
            part = part[0::2] + part[1::2]
        out[j] = part[0]
    return out


RUN_LENGTHS = (1, 2, 4, LONG_RUN, LONG_RUN + 1, 5000)


def test_summation_order_model():
    rng = np.random.default_rng(11)
    # one matrix of runs of every length, values of mixed magnitude and sign, in shuffled input order
    lens = np.array(RUN_LENGTHS * 3)
    start = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    k = int(start[-1])
    order = np.empty(k, dtype=np.int32)
    pool = rng.permutation(k)
    for j in range(lens.size):  # inside a run the input positions ascend, as the stable sort leaves them
        order[start[j]:start[j + 1]] = np.sort(pool[start[j]:start[j + 1]])
    val = rng.standard_normal(k) * 10.0 ** rng.integers(-6, 7, size=k)
    got = coo_sum_model(order, start, val)
    for j, n in enumerate(lens):
        v = val[order[start[j]:start[j + 1]]]
        if n <= LONG_RUN:  # the sequential part: bitwise a plain loop that starts from the first value
            s = float(v[0])
            for x in v[1:]:
                s += float(x)
            assert got[j] == s and np.float64(got[j]).view(np.int64) == np.float64(s).view(np.int64), (j, n)
        # any order of a k-term sum errs by at most (k - 1) * 2^-53 * sum |v|
        err, bound = abs(got[j] - math.fsum(v)), (n - 1) * 2.0 ** -53 * float(np.sum(np.abs(v)))
        assert err <= bound, (j, n, err, bound)
    # a first value of -0.0 stays -0.0 (the sum starts from it, not from +0.0)
    z = coo_sum_model(np.array([0], dtype=np.int32), np.array([0, 1], dtype=np.int32), np.array([-0.0]))
    assert np.signbit(z[0])
    # the host structure on a small case by hand: duplicates keep their input order
    row, col = np.array([2, 0, 2, 0, 2], dtype=np.int32), np.array([1, 3, 1, 0, 0], dtype=np.int32)
    rp, ci, order, start = host_assemble(3, 4, row, col)
    assert rp.tolist() == [0, 2, 2, 4] and ci.tolist() == [0, 3, 0, 1] and order.tolist() == [3, 1, 4, 0, 2] and start.tolist() == [0, 1, 2, 3, 5]
    # a crafted map: clamped runs, skipped order entries
    bad = coo_sum_model(np.array([0, 7, -1, 1], dtype=np.int32), np.array([-3, 2, 9], dtype=np.int32), np.array([1.5, 2.5]))
    assert bad.tolist() == [1.5, 2.5]


def test_synthetic_quad_assembly():
    from spmv_acc_amd import synth

    nx, ny = 7, 5
    row, col, val = synth.fem_quads_coo(nx, ny, seed=3)
    nodes = (nx + 1) * (ny + 1)
    assert row.size == col.size == val.size == 16 * nx * ny and row.dtype == col.dtype == np.int32 and val.dtype == np.float64
    assert row.min() == 0 and row.max() == nodes - 1 and col.min() == 0 and col.max() == nodes - 1
    rp, ci, order, start = host_assemble(nodes, nodes, row, col)
    hits = np.diff(start)
    assert set(hits.tolist()) == {1, 2, 4}
    assert np.array_equal(np.sort(np.diff(rp))[[0, -1]], [4, 9])  # a corner node couples to 4 nodes, an interior one to 9
    r2, c2, v2 = synth.shuffle_coo(row, col, val, seed=4)
    assert not np.array_equal(r2, row) and np.array_equal(np.sort(v2), np.sort(val))
    a, b = host_assemble(nodes, nodes, r2, c2), (rp, ci)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    r3, c3, v3 = synth.shuffle_coo(row, col, None, seed=4)
    assert v3 is None and np.array_equal(r3, r2) and np.array_equal(c3, c2)
