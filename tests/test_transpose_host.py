"""CPU side of the transposed product (no GPU): the C ABI declares and exports the three entries, the Python wrappers refuse bad arguments before
any launch, the compiled kernels add with one hardware fp64 atomic and fit their register budget, every size-selected branch of the new code
names the GPU tests that cross it, the engine file stays stateless, and the GPU suite's tolerance cannot fail on summation order alone."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import spmv_acc_amd
from test_coo_host import HELPERS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "spmv_acc_amd/csrc/"
NEW_SOURCES = ("transpose.hpp", "k_transpose.hip", "transpose.cpp")

# (rule, file, regex that must match the source, GPU tests of tests/test_gpu_transpose.py that cross it at test size, what it selects)
TRANSPOSE_SIZE_RULES = [
    ("kTransPerLane", CSRC + "transpose.hpp", r"constexpr int kTransPerLane = 8;",
     ["test_spmv_t_parity", "test_spmv_t_contract"], "scatter pass: non-zeros per lane (matrices of fewer than 8 * 64 non-zeros leave lanes and steps empty)"),
    ("kTransWaveChunk", CSRC + "transpose.hpp", r"constexpr int kTransWaveChunk = 64 \* kTransPerLane;",
     ["test_spmv_t_parity", "test_adjoint_identity"],
     "non-zeros per wavefront: a wavefront inside the 120 001-non-zero hub row searches no row, one over 3-per-row rows searches 170"),
    ("kTransTile", CSRC + "transpose.hpp", r"constexpr int kTransTile = 4 \* kTransWaveChunk;",
     ["test_spmv_t_parity", "test_spmv_t_contract"],
     "fixed tiles of the non-zero stream whatever the row lengths; an un-rebased row range starts at the tile that holds rowptr[0]"),
    ("first tile of a view", CSRC + "k_transpose.hip", r"for \(long long tile = lo / kTransTile \+ blockIdx\.x; tile < ntiles; tile \+= gridDim\.x\)",
     ["test_spmv_t_contract", "test_transpose_grid_stride_at_test_size"], "un-rebased sub-range: tiles from rowptr[0] on; blocks stride over the tiles beyond the grid"),
    ("kMaxGridBlocks (grid striding)", CSRC + "structure_passes.hpp", r"const long long cap = max_grid_blocks\(\);",
     ["test_transpose_grid_stride_at_test_size"], "every kernel of the three entries strides over the work beyond max_grid_blocks() workgroups"),
    ("kMaxGridBlocks (grid striding): the transpose's call", CSRC + "k_transpose.hip", r"dim3\(grid_for\(nnz_end, kTransTile\)\)",
     ["test_transpose_grid_stride_at_test_size"], "the launchers of the three entries take the shared grid"),
    ("sort bits from n", CSRC + "transpose.hpp", r"while \(bits < 31 && \(1LL << bits\) < n\) \+\+bits;",
     ["test_transpose_is_the_host_stable_argsort"], "radix-sort passes follow the column count: n = 37 sorts 6 bits, n = 150 000 sorts 18"),
    ("sort size paths", CSRC + "k_transpose.hip", r"rocprim::radix_sort_pairs\(tmp, \*tmp_bytes, ci, keys_out, rocprim::counting_iterator<int>\(0\), perm,",
     ["test_transpose_is_the_host_stable_argsort"],
     "the library sort picks its algorithm by size: matrices of 2 049 ... 3.2 M non-zeros cross its single-block, merge and multi-pass forms"),
    ("int32 block arithmetic", CSRC + HELPERS, r"inline bool too_large\(long long v\) \{ return v > INT_MAX - \(1 << 16\); \}",
     ["test_spmv_t_contract"], "m, n or nnz beyond this: SPMV_ACC_ERR_TOO_LARGE, as the other entries"),
    ("workspace with / without perm", CSRC + "transpose.cpp", r"off_bad = off_perm \+ \(d_perm \? 0 : ints\)",
     ["test_transpose_is_the_host_stable_argsort"], "perm == NULL: the permutation lives in the workspace (12 B instead of 8 B per non-zero)"),
    ("kEntryAlign", CSRC + HELPERS, r"constexpr size_t kEntryAlign = 256;",
     ["test_transpose_is_the_host_stable_argsort"], "workspace parts are padded to 256 B (nnz not a multiple of 64 ints: the hub matrices)"),
]


def test_transpose_size_rules_name_their_tests():
    gpu_tests = open(os.path.join(ROOT, "tests", "test_gpu_transpose.py")).read()
    defined = set(re.findall(r"^def (test_\w+)\(", gpu_tests, flags=re.M))
    for name, path, pattern, tests, what in TRANSPOSE_SIZE_RULES:
        assert re.search(pattern, open(os.path.join(ROOT, path)).read()), f"{name}: no longer matches {path}: {pattern}"
        assert tests and what
        for t in tests:
            assert t in defined, f"{name}: names {t}, which is not a test of tests/test_gpu_transpose.py"
    # every named constant of the new files is registered above (tests/size_thresholds.py does not scan them)
    registered = " ".join(r[0] + " " + r[2] for r in TRANSPOSE_SIZE_RULES)
    for f in NEW_SOURCES:
        for k in re.findall(r"constexpr\s+[\w:<> ]+?\s+(k[A-Z]\w*)\s*=", open(os.path.join(ROOT, CSRC, f)).read()):
            assert k in registered, f"{f}: constant {k} is not in TRANSPOSE_SIZE_RULES"


def test_transposed_entries_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "spmv_acc.h")).read()
    assert re.search(r"int spmv_acc_csr_transpose\(int m, int n, int nnz, const int \*d_rowptr, const int \*d_colindex, const double \*d_value,\s*"
                     r"int \*d_t_rowptr, int \*d_t_colindex, double \*d_t_value, int \*d_perm\);", header)
    assert re.search(r"int spmv_acc_csr_transpose_values\(int nnz, const int \*d_perm, const double \*d_value, double \*d_t_value\);", header)
    assert re.search(r"int spmv_acc_csr_spmv_t\(double alpha, double beta, int m, int n, int nnz, const int \*d_rowptr, const int \*d_colindex,\s*"
                     r"const double \*d_value, const double \*dx, double \*dy\);", header)
    assert "the one\n *     exception, spmv_acc_csr_spmv_t" in header  # "the kernels never use atomics" names its exception
    lib = spmv_acc_amd.load_library()
    for s in ("spmv_acc_csr_transpose", "spmv_acc_csr_transpose_values", "spmv_acc_csr_spmv_t"):
        assert s in spmv_acc_amd.C_ABI_SYMBOLS and hasattr(lib, s), s
    for f in ("csr_transpose", "csr_transpose_values", "csr_spmv_t"):
        assert callable(getattr(spmv_acc_amd, f))
    for f in ("k_transpose.hip", "transpose.cpp"):  # both builds compile the new files
        assert f in open(os.path.join(ROOT, CSRC, "Makefile")).read() and f in open(os.path.join(ROOT, "CMakeLists.txt")).read(), f


def test_bad_arguments_are_refused_without_a_gpu():
    """The C entries check their arguments before they touch the device: the error codes come back on a machine without one."""
    lib = spmv_acc_amd.load_library()
    one = 8  # (never dereferenced: a non-null pointer value)
    assert lib.spmv_acc_csr_spmv_t(1.0, 1.0, -1, 4, 4, one, one, one, one, one) == 2
    assert lib.spmv_acc_csr_spmv_t(1.0, 1.0, 4, 2 ** 31 - 1, 4, one, one, one, one, one) == 4
    assert lib.spmv_acc_csr_spmv_t(1.0, 1.0, 4, 4, 4, one, one, one, one, None) == 2
    assert lib.spmv_acc_csr_spmv_t(1.0, 1.0, 4, 4, 4, None, one, one, one, one) == 2
    assert lib.spmv_acc_csr_transpose(4, -1, 4, one, one, one, one, one, one, None) == 2
    assert lib.spmv_acc_csr_transpose(4, 4, 4, one, one, one, None, one, one, None) == 2
    assert lib.spmv_acc_csr_transpose(4, 4, 4, one, one, None, one, one, one, None) == 2
    assert lib.spmv_acc_csr_transpose(4, 4, 4, None, one, one, one, one, one, None) == 2
    assert lib.spmv_acc_csr_transpose(2 ** 31 - 1, 4, 4, one, one, one, one, one, one, None) == 4
    assert lib.spmv_acc_csr_transpose_values(-1, one, one, one) == 2
    assert lib.spmv_acc_csr_transpose_values(4, None, one, one) == 2
    assert lib.spmv_acc_csr_transpose_values(0, None, None, None) == 0
    assert lib.spmv_acc_last_error() == 0
    try:
        assert lib.spmv_acc_set_tunable(b"deterministic", 1) == 0
        assert lib.spmv_acc_csr_spmv_t(1.0, 1.0, 4, 4, 4, one, one, one, one, one) == 2
        assert b"spmv_acc_csr_transpose" in lib.spmv_acc_last_error_string()
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
    m, n, nnz = 10, 12, 30
    good = dict(rowptr=_i(m + 1), colindex=_i(nnz), value=_f(nnz), x=_f(m), y=_f(n))

    def spmv_t(match, mm=m, nn=n, **bad):
        a = dict(good, **bad)
        with pytest.raises(E, match=match):
            spmv_acc_amd.csr_spmv_t(1.0, 1.0, mm, nn, nnz, a["rowptr"], a["colindex"], a["value"], a["x"], a["y"])

    spmv_t("not on the GPU", y=_f(n, cuda=False))
    spmv_t("dtype", value=_f(nnz, dtype="torch.float32"))
    spmv_t("dtype", rowptr=_FakeTensor(m + 1, dtype="torch.int64"))
    spmv_t("not contiguous", x=_f(m, contiguous=False))
    spmv_t("elements", x=_f(n - 3))        # x holds m entries, y holds n: the roles of the plain product swapped
    spmv_t("elements", y=_f(n - 1))
    spmv_t("elements", colindex=_i(nnz - 1))
    spmv_t("elements", rowptr=_i(m))
    spmv_t("on cuda:1", x=_f(m, device="cuda:1"))
    spmv_t("torch tensor", y=[0.0] * n)
    spmv_t("torch tensor", x=None)
    spmv_t("negative", mm=-1)

    def transpose(match, mm=m, nn=n, **bad):
        a = dict(good, **bad)
        with pytest.raises(E, match=match):
            spmv_acc_amd.csr_transpose(mm, nn, nnz, a["rowptr"], a["colindex"], a["value"], want_perm=True)

    transpose("not on the GPU", colindex=_i(nnz, cuda=False))
    transpose("dtype", colindex=_f(nnz))
    transpose("dtype", value=_i(nnz))
    transpose("not contiguous", value=_f(nnz, contiguous=False))
    transpose("elements", value=_f(nnz - 1))
    transpose("elements", rowptr=_i(m))
    transpose("torch tensor", rowptr=None)
    transpose("torch tensor", value=3.0)
    transpose("negative", nn=-2)

    def values(match, perm=_i(nnz), value=_f(nnz), out=_f(nnz)):
        with pytest.raises(E, match=match):
            spmv_acc_amd.csr_transpose_values(perm, value, out)

    values("dtype", perm=_f(nnz))
    values("dtype", out=_i(nnz))
    values("elements", value=_f(nnz - 1))
    values("elements", out=_f(nnz - 1))
    values("not on the GPU", value=_f(nnz, cuda=False))
    values("torch tensor", perm=None)


def test_transposed_entries_keep_no_state():
    """ADVICE.md's high-severity finding is a plan that silently holds a copy of the caller's values: the engine file of these entries neither
    finds nor makes a plan, counts no plan work and keeps nothing static; the one allocation is freed on every way out."""
    src = open(os.path.join(ROOT, CSRC, "transpose.cpp")).read()
    code = re.sub(r"//[^\n]*", "", src)
    for word in ("get_plan", "g_plans", "t_plan_work", "t_last_plan", "tune_", "TimingPhase", "TuneTimer", "static std::", "thread_local"):
        assert word not in code, word
    assert code.count("hipMalloc(") == 1 and code.count("hipFree(") == 1 and "const auto leave = " in code
    after = code.split("hipMalloc(")[1].split("int run_csr_transpose_values")[0]
    assert not re.search(r"return (?!leave\()", after.split("const auto leave = ")[1].split("};", 1)[1]), "a way out of the transpose that skips leave()"


def test_scatter_kernel_adds_with_one_hardware_fp64_atomic(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_table

    asm = tmp_path / "k_transpose.s"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-DKERNEL_STRATEGY_ADAPTIVE",
                        "-I" + os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-S",
                        os.path.join(ROOT, CSRC, "k_transpose.hip"), "-o", str(asm)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    text = asm.read_text()
    assert "cmpswap" not in text  # no compare-and-swap loop anywhere in the file
    bodies = {}
    for mt in re.finditer(r"^(_ZN8spmv_acc\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, flags=re.M | re.S):
        bodies[mt.group(1)] = mt.group(2)
    scatter = [b for k, b in bodies.items() if "spmv_t_scatter_kernel" in k]
    assert len(scatter) == 1 and scatter[0].count("global_atomic_add_f64") == 8, len(scatter)  # one per non-zero of a lane, none returning
    assert not re.search(r"global_atomic_add_f64 v\[\d+:\d+\], v\[\d+:\d+\], v\[\d+:\d+\]", scatter[0])  # (the returning form has a destination)
    for k, b in bodies.items():
        if "spmv_t_scatter_kernel" not in k:
            assert "global_atomic_add_f64" not in b, k  # the transpose itself never adds a float
    rows = [k for k in resource_table.parse(r.stderr) if "rocprim" not in k["name"]]
    names = sorted(k["name"] for k in rows)
    assert names == sorted(["transpose_check_kernel", "transpose_rowptr_kernel", "transpose_rows_kernel", "transpose_gather_kernel",
                            "transpose_values_kernel", "spmv_t_scale_kernel", "spmv_t_scatter_kernel"]), names
    for k in rows:
        assert k["scratch"] == 0 and k["agprs"] == 0, k
        # as found when the kernels were written: 62 VGPRs for the scatter pass (8 columns, 8 values and 8 row searches in flight), 6 ... 16 elsewhere
        assert k["vgprs"] <= (64 if k["name"] == "spmv_t_scatter_kernel" else 16) and k["occupancy"] >= 8, k
    # (rocPRIM's sort kernels are instantiated in the same file and are not held to this: its multi-pass kernel keeps 80 B of scratch per lane)


def test_no_new_source_names_a_forbidden_instruction():
    words = ("s_" + "store", "s_buffer_" + "store", "s_scratch_" + "store", "s_" + "atomic", "s_buffer_" + "atomic", "s_dcache_" + "wb",
             "s_dcache_" + "discard")
    files = [os.path.join(ROOT, CSRC, f) for f in NEW_SOURCES] + [os.path.join(ROOT, "tools", "transpose_bench.py"),
                                                                 os.path.join(ROOT, "tests", "test_gpu_transpose.py"), __file__]
    for f in files:
        text = open(f).read().lower()
        for w in words:
            assert w not in text, (f, w)


def test_reversed_order_scatter_stays_within_the_gate(oracle):
    """The GPU suite holds csr_spmv_t to scaled_error <= 1e-12 although its sums depend on arrival order.  That gate is relative to
    |alpha| * sum |a| |x| + |beta y0|, and a sum of k terms in ANY order errs by at most about k * 2^-53 of it (k <= 120 001 here: 1.3e-11 in
    the worst case, a few 1e-15 in practice).  Checked here on every matrix of the GPU suite with the opposite order to the oracle's: a numpy
    scatter over the non-zeros from last to first."""
    import test_gpu_transpose as g

    worst = 0.0
    for tag, (rp, ci, v), n in g.matrices():
        m = rp.size - 1
        w_rp, w_ci, w_v, _ = g.host_transpose(rp, ci, v, n)
        rng = np.random.default_rng(m + 3 * n)
        x, y0 = rng.standard_normal(m), rng.standard_normal(n)
        rows = np.repeat(np.arange(m), np.diff(rp))
        for alpha, beta in g.ABS:
            ref = oracle.host_spmv(alpha, beta, w_rp, w_ci, w_v, x, y0)
            y = beta * y0 if beta != 0.0 else np.zeros(n)
            np.add.at(y, ci[::-1], (alpha * v * x[rows])[::-1])
            err = oracle.scaled_error(y, ref, alpha, beta, w_rp, w_ci, w_v, x, y0)
            worst = max(worst, err)
            assert err <= g.SCALED_TOL, (tag, alpha, beta, err)
    print(f"worst scaled error of the reversed-order scatter: {worst:.3e}")
