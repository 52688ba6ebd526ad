"""CPU side of the dense coarse-level solve (no GPU): the C ABI declares and exports the two entries, they and the Python wrappers refuse bad
arguments before any launch, the compiled kernels use no scratch and no AGPR and fit 64 VGPRs, every size-selected branch of the new code names
the GPU tests that cross it, the engine file stays stateless, and the definitions are restated here in numpy and exported to the GPU suite as
its references: the inverse in its unblocked order (host_dense_inverse, bit for bit) and the apply in its summation order (host_dense_apply),
checked against independent statements: the residual of the inverse, a permutation's transpose, a zero column's info, the tie's pivot."""
import ctypes
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import spmv_acc_amd
from test_agg_host import grid5_matrix
from test_coo_host import SHARED, _FakeTensor, _f, _i
from test_gs_host import HELPERS, row_sum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "spmv_acc_amd/csrc/"
NEW_SOURCES = ("dense.hpp", "k_dense.hip", "dense.cpp")
INVERSE = "test_inverse_is_the_host_model"
APPLY = "test_apply_is_the_host_model"
STRIDE = "test_dense_grid_stride_at_test_size"
INFO = "test_singular_inputs_give_info"
EMPTY = "test_no_rows"
CAPTURE = "test_apply_captured_and_replayed"
INVERSE_CONTRACT = "test_inverse_contract"
APPLY_CONTRACT = "test_apply_contract"
MAX_ROWS, PIVOT_THREADS, TILE, ROWS_PER_BLOCK = 4096, 256, 256, 4  # kDenseMaxRows, kDensePivotThreads, kDenseTile, kDenseRowsPerBlock

# (rule, file, regex that must match the source, GPU tests of tests/test_gpu_dense.py that cross it at test size, what it selects)
DENSE_SIZE_RULES = [
    ("kDenseMaxRows", CSRC + "dense.hpp", r"constexpr int kDenseMaxRows = 4096;",
     [INVERSE_CONTRACT], "m = 4097 is refused on the host with SPMV_ACC_ERR_TOO_LARGE, by the entry and by the wrapper"),
    ("the cap", CSRC + "dense.cpp", r"if \(m > kDenseMaxRows\)",
     [INVERSE_CONTRACT], "refused before the device is touched"),
    ("kDensePivotThreads", CSRC + "dense.hpp", r"constexpr int kDensePivotThreads = 256;",
     [INVERSE], "one workgroup searches the column: m = 1 .. 130 leave lanes without a row, m = 257 gives lane 0 a second row at step 0"),
    ("the pivot's strided rows", CSRC + "k_dense.hip", r"for \(int i = k \+ t; i < m; i \+= kDensePivotThreads\) \{",
     [INVERSE, STRIDE], "r257 and grid18 (324): more rows than lanes in the first steps, fewer in the last"),
    ("the larger magnitude, the smaller row", CSRC + "k_dense.hip", r"if \(om > s_mag\[t\] \|\| \(om == s_mag\[t\] && orow < s_row\[t\]\)\) \{",
     [INVERSE], "the tie between -3 and +3 in rows 1 and 2 (tie4): the smaller row wins whichever lane holds it; a NaN never wins (nan_entry)"),
    ("all NaN", CSRC + "k_dense.hip", r"const int p = s_row\[0\] == INT_MAX \? k : s_row\[0\];",
     [INFO], "a column of NaNs only: p = k (the NaN entry has spread over its row and column by then)"),
    ("the first flagged step", CSRC + "k_dense.hip", r"if \(bad && state\[2\] == 0\) state\[2\] = static_cast<u64>\(k \+ 1\);",
     [INFO, INVERSE], "info stays 0 on the regular cases; the zero column, the NaN and the empty row flag one step and keep it"),
    ("the swap", CSRC + "k_dense.hip", r"if \(p != k\) \{",
     [INVERSE], "swap2 and perm6 force swaps, the random cases swap in most steps, grid18 (diagonally dominant) in none"),
    ("the multipliers of the other rows", CSRC + "k_dense.hip", r"if \(i != k && i != p\) f\[i\] = ",
     [INVERSE], "every case of more than two rows; one and swap2 have no such row"),
    ("the pivot row is not updated", CSRC + "k_dense.hip", r"if \(i == k\) continue;",
     [INVERSE], "every case"),
    ("kDenseTile", CSRC + "dense.hpp", r"constexpr int kDenseTile = 256;",
     [INVERSE, STRIDE], "columns per workgroup: E's rows of 2 m columns are one ragged tile up to m = 128, two from r130 on, three at r257 and grid18"),
    ("tile loops", CSRC + "k_dense.hip", r"for \(long long tile = blockIdx\.x; tile < ntiles; tile \+= gridDim\.x\) \{ // \(block-uniform\)",
     [STRIDE], "fill, update and copy stride over their tiles beyond the grid (grid18: 972 and 648 tiles over 64 workgroups)"),
    ("row loops", CSRC + "k_dense.hip", r"r < m; r \+= stride\) \{",
     [STRIDE], "the apply strides over its rows (grid18: 81 workgroups' worth over 64); the scatter's 324 rows are two workgroups and never stride "
               "below the cap of 4096 rows, nor do the row pass's 3 m items: their loops are the shared form, crossed once"),
    ("the row pass's items", CSRC + "k_dense.hip", r"t < items; t \+= stride\) \{",
     [INVERSE], "3 m lanes: 2 m columns and m multipliers (at most 48 workgroups at the cap)"),
    ("kMaxGridBlocks (grid striding)", CSRC + SHARED, r"const long long cap = max_grid_blocks\(\);",
     [STRIDE], "every launcher clamps its grid with passes::grid_for"),
    ("census grid", CSRC + SHARED, r"return grid > static_cast<unsigned>\(kCooCheckBlocks\) \? static_cast<unsigned>\(kCooCheckBlocks\) : grid;",
     [INVERSE_CONTRACT], "one count slot per wavefront (the colouring's census, whose mirror count is not judged)"),
    ("kDenseRowsPerBlock", CSRC + "dense.hpp", r"constexpr int kDenseRowsPerBlock = 4;",
     [APPLY], "one wavefront per row: m = 1 and swap2 leave wavefronts without a row, r65 is 17 workgroups with one row in the last"),
    ("a lane without a term", CSRC + "k_dense.hip", r"if \(j < m\) \{",
     [APPLY], "m = 1 .. 63: lanes hold +0.0; r64 fills the wavefront exactly, r65 gives lane 0 a second term"),
    ("four lines in flight", CSRC + "k_dense.hip", r"for \(; j \+ 3 \* kWave < m; j \+= 4 \* kWave\) \{",
     [APPLY, STRIDE], "taken from m = 257 on (lane 0 of r257; grid18: lanes 0 .. 3), never below"),
    ("the ragged tail", CSRC + "k_dense.hip", r"for \(; j < m; j \+= kWave\) \{",
     [APPLY], "r130: three 64-strides, the third of two lanes; r65; the tail behind the four-line step at grid18"),
    ("kDenseState", CSRC + "dense.hpp", r"constexpr int kDenseState = 3;",
     [INVERSE, INFO], "p, piv and info, zeroed before the first step"),
    ("kEntryAlign", CSRC + HELPERS, r"constexpr size_t kEntryAlign = 256;",
     [INVERSE], "workspace parts are padded to 256 B (row counts that are no multiple of 16: most cases)"),
    ("no rows", CSRC + "dense.cpp", r"if \(m == 0\) \{",
     [EMPTY], "m == 0: nothing is read, written or allocated, info = 0"),
    ("no rows: the apply", CSRC + "dense.cpp", r"if \(m == 0\) return kOk;",
     [EMPTY], "nothing to launch"),
    ("no entries", CSRC + "k_dense.hip", r"nnz <= 0\) return;",
     [INFO], "a matrix without entries: the scatter is not launched, E = [0 | I], info = 1"),
    ("int32 block arithmetic", CSRC + HELPERS, r"inline bool too_large\(long long v\) \{ return v > INT_MAX - \(1 << 16\); \}",
     [INVERSE_CONTRACT, APPLY_CONTRACT], "nnz (the inverse) or m (the apply) beyond this: SPMV_ACC_ERR_TOO_LARGE, as the other entries"),
    ("the census is shared", CSRC + "dense.cpp", r"pattern_census\(st, kEntry, ",
     [INVERSE_CONTRACT, INVERSE], "the refusals and their text are entry_helpers.hpp's, the same for the four entries; without an advice the mirrors are not judged"),
]


def test_dense_size_rules_name_their_tests():
    gpu_tests = open(os.path.join(ROOT, "tests", "test_gpu_dense.py")).read()
    defined = set(re.findall(r"^def (test_\w+)\(", gpu_tests, flags=re.M))
    for name, path, pattern, tests, what in DENSE_SIZE_RULES:
        assert re.search(pattern, open(os.path.join(ROOT, path)).read()), f"{name}: no longer matches {path}: {pattern}"
        assert tests and what
        for t in tests:
            assert t in defined, f"{name}: names {t}, which is not a test of tests/test_gpu_dense.py"
    # every named constant of the new files is registered above (tests/size_thresholds.py does not scan them)
    registered = " ".join(r[0] + " " + r[2] for r in DENSE_SIZE_RULES)
    found = 0
    for f in NEW_SOURCES:
        for k in re.findall(r"constexpr\s+[\w:<> ]+?\s+(k[A-Z]\w*)\s*=", open(os.path.join(ROOT, CSRC, f)).read()):
            found += 1
            assert k in registered, f"{f}: constant {k} is not in DENSE_SIZE_RULES"
    assert found == 5
    header = open(os.path.join(ROOT, CSRC, "dense.hpp")).read()
    assert f"constexpr int kDenseMaxRows = {MAX_ROWS};" in header and f"constexpr int kDensePivotThreads = {PIVOT_THREADS};" in header
    assert f"constexpr int kDenseTile = {TILE};" in header and f"constexpr int kDenseRowsPerBlock = {ROWS_PER_BLOCK};" in header
    assert spmv_acc_amd.DENSE_MAX_ROWS == MAX_ROWS
    kernels = open(os.path.join(ROOT, CSRC, "k_dense.hip")).read()
    assert kernels.count("tile += gridDim.x") == 3 and kernels.count("+= stride)") == 3  # every loop over work is one of the registered forms


PROTOTYPES = (
    r"int spmv_acc_csr_dense_inverse\(int m, int nnz, const int \*d_rowptr, const int \*d_colindex, const double \*d_value, double \*d_inv, int \*h_info\);",
    r"int spmv_acc_dense_apply\(int m, const double \*d_inv, const double \*d_b, double \*d_x\);",
)


def test_dense_entries_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "spmv_acc.h")).read()
    for proto in PROTOTYPES:
        assert re.search(proto, header), proto
    for entry in ("1", "2"):
        block = re.search(r"/\* ---- dense coarse-level solve, " + entry + r".*?\*/", header, flags=re.S)
        assert block, entry
        for word in ("replaces: nothing in the reference", "COST", "CHECKS", "CANNOT CHECK"):
            assert word in block.group(0), (entry, word)
    # the header declares exactly what the package lists
    declared = set(re.findall(r"\b(sparse_spmv|spmv_acc_[a-z_0-9]+)\s*\(", header))
    assert declared == set(spmv_acc_amd.C_ABI_SYMBOLS), declared ^ set(spmv_acc_amd.C_ABI_SYMBOLS)
    lib = spmv_acc_amd.load_library()
    for s in ("spmv_acc_csr_dense_inverse", "spmv_acc_dense_apply"):
        assert s in spmv_acc_amd.C_ABI_SYMBOLS and hasattr(lib, s), s
    assert lib.spmv_acc_csr_dense_inverse.restype is ctypes.c_int and lib.spmv_acc_dense_apply.restype is ctypes.c_int
    assert len(lib.spmv_acc_csr_dense_inverse.argtypes) == 7 and len(lib.spmv_acc_dense_apply.argtypes) == 4
    for f in ("csr_dense_inverse", "dense_apply", "amg_setup", "amg_cycle"):
        assert callable(getattr(spmv_acc_amd, f))
    assert "amg_setup" in spmv_acc_amd.csr_smooth_prolongator.__doc__  # the recipe's docstring points at the function that runs it
    for f in ("k_dense.hip", "dense.cpp"):  # both builds compile the new files
        assert f in open(os.path.join(ROOT, CSRC, "Makefile")).read() and f in open(os.path.join(ROOT, "CMakeLists.txt")).read(), f
    assert "dense.hpp" in open(os.path.join(ROOT, CSRC, "Makefile")).read()
    assert " k_dense " in open(os.path.join(ROOT, "tools", "resource_usage.sh")).read()
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "spmv_acc_csr_dense_inverse" in text and "amg_setup" in text, doc


BAD, TOO_LARGE = 2, 4  # SPMV_ACC_ERR_BAD_ARGUMENT, SPMV_ACC_ERR_TOO_LARGE


def test_bad_arguments_are_refused_without_a_gpu():
    """The C entries check their arguments before they touch the device: the error codes come back on a machine without one."""
    lib = spmv_acc_amd.load_library()
    one = 8  # (never dereferenced: a non-null pointer value)
    h_info = ctypes.c_int(-5)

    def inverse(m=4, nnz=8, rp=one, ci=one, v=one, inv=one, hi=ctypes.byref(h_info)):
        return lib.spmv_acc_csr_dense_inverse(m, nnz, rp, ci, v, inv, hi)

    for neg in ("m", "nnz"):
        assert inverse(**{neg: -1}) == BAD, neg
        assert b"spmv_acc_csr_dense_inverse: negative" in lib.spmv_acc_last_error_string()
    for null in ("rp", "ci", "v", "inv", "hi"):
        assert inverse(**{null: None}) == BAD, null
        assert b"spmv_acc_csr_dense_inverse: null" in lib.spmv_acc_last_error_string(), null
    for big in (MAX_ROWS + 1, 2 ** 20, 2 ** 31 - 1):
        assert inverse(m=big) == TOO_LARGE, big
        assert b"at most 4096" in lib.spmv_acc_last_error_string()
    for big in (2 ** 31 - 1, 2 ** 31 - 2 ** 16):
        assert inverse(nnz=big) == TOO_LARGE and b"spmv_acc_csr_dense_inverse:" in lib.spmv_acc_last_error_string()
    assert inverse(m=0, nnz=3) == BAD and b"without rows" in lib.spmv_acc_last_error_string()
    assert h_info.value == -5
    assert inverse(m=0, nnz=0, rp=None, ci=None, v=None, inv=None) == 0  # no rows: the device is not touched
    assert h_info.value == 0 and lib.spmv_acc_last_error() == 0

    # the apply: inv of m * m = 16 doubles (128 B), b and x of m = 4 (32 B) at distinct places
    inv_at, b_at, x_at = 1 << 20, 2 << 20, 3 << 20

    def apply(m=4, inv=inv_at, b=b_at, x=x_at):
        return lib.spmv_acc_dense_apply(m, inv, b, x)

    assert apply(m=-1) == BAD and b"spmv_acc_dense_apply: negative" in lib.spmv_acc_last_error_string()
    for null in ("inv", "b", "x"):
        assert apply(**{null: None}) == BAD, null
        assert b"spmv_acc_dense_apply: null" in lib.spmv_acc_last_error_string(), null
    for big in (2 ** 31 - 1, 2 ** 31 - 2 ** 16):
        assert apply(m=big) == TOO_LARGE and b"spmv_acc_dense_apply:" in lib.spmv_acc_last_error_string()
    for bad in (dict(b=x_at), dict(b=x_at + 24), dict(b=x_at - 24), dict(x=b_at + 8)):
        assert apply(**bad) == BAD and b"b overlaps x" in lib.spmv_acc_last_error_string(), bad
    for bad in (dict(x=inv_at), dict(x=inv_at + 120), dict(x=inv_at - 24), dict(b=inv_at + 64), dict(b=inv_at - 8), dict(inv=b_at - 120), dict(inv=x_at + 24)):
        assert apply(**bad) == BAD and b"overlaps inv" in lib.spmv_acc_last_error_string(), bad
    assert apply(m=0, inv=None, b=None, x=None) == 0 and lib.spmv_acc_last_error() == 0  # nothing to do: no rows
    lib.spmv_acc_clear_error()


def test_wrappers_refuse_bad_arguments():
    E = spmv_acc_amd.SpmvAccError
    m, nnz = 10, 30

    def inverse(match, mm=m, rp=_i(m + 1), ci=_i(nnz), v=_f(nnz)):
        with pytest.raises(E, match=match):
            spmv_acc_amd.csr_dense_inverse(mm, rp, ci, v)

    inverse("not on the GPU", ci=_i(nnz, cuda=False))
    inverse("not on the GPU", v=_f(nnz, cuda=False))
    inverse("dtype", rp=_FakeTensor(m + 1, dtype="torch.int64"))
    inverse("dtype", ci=_f(nnz))
    inverse("dtype", v=_i(nnz))
    inverse("dtype", v=_FakeTensor(nnz, dtype="torch.float32"))
    inverse("not contiguous", ci=_i(nnz, contiguous=False))
    inverse("not contiguous", v=_f(nnz, contiguous=False))
    inverse("elements", rp=_i(m))
    inverse("as many", v=_f(nnz - 1))
    inverse("as many", v=_f(nnz + 1))
    inverse("on cuda:1", v=_f(nnz, device="cuda:1"))
    inverse("torch tensor", rp=None)
    inverse("torch tensor", ci=[0] * nnz)
    inverse("torch tensor", v=3.0)
    inverse("negative", mm=-1)
    inverse("at most 4096", mm=MAX_ROWS + 1, rp=_i(MAX_ROWS + 2))

    def apply(match, mm=m, inv=_f(m * m), b=_f(m), x=_f(m)):
        with pytest.raises(E, match=match):
            spmv_acc_amd.dense_apply(mm, inv, b, x)

    apply("not on the GPU", inv=_f(m * m, cuda=False))
    apply("not on the GPU", b=_f(m, cuda=False))
    apply("dtype", inv=_i(m * m))
    apply("dtype", x=_FakeTensor(m, dtype="torch.float32"))
    apply("not contiguous", inv=_f(m * m, contiguous=False))
    apply("not contiguous", x=_f(m, contiguous=False))
    apply("must hold 100", inv=_f(m * m - 1))
    apply("must hold 100", inv=_f(m * m + 1))
    apply("as many", b=_f(m - 1))
    apply("as many", x=_f(m + 1))
    apply("on cuda:1", b=_f(m, device="cuda:1"))
    apply("torch tensor", inv=None)
    apply("torch tensor", b=[0.0] * m)
    apply("torch tensor", x=3.0)
    apply("negative", mm=-1)
    # the hierarchy's own arguments, before any entry is called
    good = (_i(m + 1), _i(nnz), _f(nnz))
    for kw, match in ((dict(coarse_rows=0), "at least 1"), (dict(max_levels=0), "at least 1"), (dict(theta=-1.0), "theta"), (dict(theta=float("nan")), "theta"),
                      (dict(omega=float("inf")), "omega"), (dict(omega=0.0), "omega")):
        with pytest.raises(E, match=match):
            spmv_acc_amd.amg_setup(m, *good, **kw)
    with pytest.raises(E, match="negative"):
        spmv_acc_amd.amg_setup(-1, *good)
    with pytest.raises(E, match="torch tensor"):
        spmv_acc_amd.amg_setup(m, None, good[1], good[2])
    with pytest.raises(E, match="AmgHierarchy"):
        spmv_acc_amd.amg_cycle(None, _f(m), _f(m))


def test_dense_entries_keep_no_state():
    """As test_strength_entries_keep_no_state: the engine file neither finds nor makes a plan, counts no plan work, reads no tunable and keeps
    nothing static; the inverse's one allocation is freed on every way out; info is read once, after the last step; the apply is launch-only."""
    src = open(os.path.join(ROOT, CSRC, "dense.cpp")).read()
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
    launches = ("pattern_census", "launch_dense_fill", "launch_dense_scatter", "launch_dense_pivot", "launch_dense_row", "launch_dense_update",
                "launch_dense_copy")
    body = after.split("hipMalloc(")[1]
    assert [body.index(s + "(st, ") for s in launches] == sorted(body.index(s + "(st, ") for s in launches)  # the passes in the documented order
    assert all(body.count(s + "(st, ") == 1 for s in launches)
    assert body.index("pattern_census(") < body.index("launch_dense_fill(")  # the census is judged before anything is written
    # ... without an advice: the mirrors are neither judged nor reported, the pattern need not be symmetric (nor is the count of diagonals asked for)
    assert "pattern_census(st, kEntry, m, nnz, d_rowptr, d_colindex, d_slots, nullptr, nullptr)" in body
    assert not [ln for ln in after.splitlines() if re.search(r"\breturn\b(?! leave\()", ln)]  # every way out passes leave()
    loop = body.split("for (int k = 0; k < m; ++k) {")[1].split("\n  }\n")[0]
    assert "Synchronize" not in loop and "hipMemcpy" not in loop and len(re.findall(r"\blaunch_\w+\(", loop)) == 3  # a step is three launches, no read
    tail = body.split("launch_dense_copy")[1]
    assert tail.count("hipMemcpyAsync(") == 1 and tail.index("hipMemcpyAsync(&info") < tail.index("*h_info = ") < tail.index("return leave(kOk);")
    assert body.count("hipMemcpyAsync(") == 1 and "while (" not in code  # info (the census' one copy is the helper's, pinned in test_gs_host): the host reads the elimination's state once
    apply = code.split("int run_dense_apply")[1]
    assert "hipMalloc" not in apply and "Synchronize" not in apply and "hipMemcpy" not in apply and "hipMemset" not in apply  # launch-only
    assert "plan_work_allowed" not in apply and re.findall(r"\blaunch_\w+\(", apply) == ["launch_dense_apply(", "launch_error("]
    assert apply.index("b overlaps x") < apply.index("overlaps inv") < apply.index("launch_dense_apply(")  # refused before any launch
    kernels = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, CSRC, "k_dense.hip")).read())
    assert "atomic" not in kernels.lower() and "while (" not in kernels
    assert kernels.count("__shared__") == 2 and kernels.split("__shared__")[0].count("__global__") == 3  # LDS in the pivot search alone
    assert kernels.count("#pragma clang fp contract(off)") == 3  # the scaled pivot row, the update, the apply


KERNELS = ("dense_fill_kernel", "dense_scatter_kernel", "dense_pivot_kernel", "dense_row_kernel", "dense_update_kernel", "dense_copy_kernel",
           "dense_apply_kernel")
# as recorded in k_dense.hip's header comment
RECORDED_VGPRS = dict(dense_fill_kernel=9, dense_scatter_kernel=16, dense_pivot_kernel=10, dense_row_kernel=28, dense_update_kernel=10,
                      dense_copy_kernel=8, dense_apply_kernel=40)


def test_dense_kernels_fit_their_register_budget(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_table

    asm = tmp_path / "k_dense.s"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-DKERNEL_STRATEGY_ADAPTIVE",
                        "-I" + os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-S",
                        os.path.join(ROOT, CSRC, "k_dense.hip"), "-o", str(asm)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    text = asm.read_text()
    assert set(re.findall(r"\.wavefront_size:\s*(\d+)", text)) == {"64"}  # wave64, every kernel of the file
    bodies = {}
    for mt in re.finditer(r"^(_ZN8spmv_acc\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, flags=re.M | re.S):
        bodies[mt.group(1)] = mt.group(2)
    assert len(bodies) == len(KERNELS), sorted(bodies)
    for k, b in bodies.items():
        assert "atomic" not in b, k  # no atomics anywhere
        assert "s_sleep" not in b, k  # ... and nothing waits
        if "dense_row_kernel" not in k:  # contraction is off: no fused operation outside the division's own expansion
            assert "v_fma_f64" not in b and "v_fmac_f64" not in b, k
    for name in ("dense_update_kernel", "dense_apply_kernel"):
        body = next(b for k, b in bodies.items() if name in k)
        assert "v_mul_f64" in body and "v_add_f64" in body, name  # products and sums are instructions of their own
    row_body = next(b for k, b in bodies.items() if "dense_row_kernel" in k)
    # the IEEE division (the compiler keeps one copy per arm of p != k): its expansion refines a reciprocal with fused operations of its own
    divisions = re.findall(r"v_div_scale_f64.*?v_div_fixup_f64", row_body, flags=re.S)
    assert 1 <= len(divisions) <= 2 and all("v_rcp_f64" in d and "v_fma" in d for d in divisions)
    outside = re.sub(r"v_div_scale_f64.*?v_div_fixup_f64", "", row_body, flags=re.S)
    assert "v_fma_f64" not in outside and "v_fmac_f64" not in outside and "v_mul_f64" not in outside  # the quotient is not a reciprocal multiply
    header = open(os.path.join(ROOT, CSRC, "k_dense.hip")).read().split("#include")[0]
    rows = [k for k in resource_table.parse(r.stderr) if "rocprim" not in k["name"]]
    for k in rows:
        k["name"] = re.sub(r"<.*", "", k["name"])
    assert sorted(k["name"] for k in rows) == sorted(KERNELS), sorted(k["name"] for k in rows)
    for k in rows:
        assert k["scratch"] == 0 and k["agprs"] == 0 and k["vgprs"] <= 64 and k["occupancy"] >= 8, k
        want = RECORDED_VGPRS[k["name"]]
        assert re.search(k["name"] + r", " + str(want) + r"\b", header), (k["name"], "the count recorded in the header comment")
        assert k["vgprs"] <= want + 4, (k, "grew past the count recorded in k_dense.hip (a few registers of compiler drift are allowed)")


# ---- the inverse (dense.hpp THE DEFINITION), in numpy, bit for bit: the GPU suite's reference ---------------------------------------------------
def to_dense(m, n, rp, ci, v):
    D = np.zeros((m, n))
    D[np.repeat(np.arange(m), np.diff(rp)), ci] = v
    return D


def host_dense_inverse(m, rp, ci, v, pivots=None):
    """(inv, info) by the definition of dense.hpp, step for step: numpy rounds every product, difference and quotient on its own.  pivots: a
    list that receives the pivot row of every step."""
    rp, ci, v = np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64), np.asarray(v, dtype=np.float64)
    E = np.zeros((m, 2 * m))
    E[np.repeat(np.arange(m), np.diff(rp)), ci] = v  # positions not stored are +0.0
    E[np.arange(m), m + np.arange(m)] = 1.0
    info = 0
    with np.errstate(all="ignore"):
        for k in range(m):
            mag = np.abs(E[k:, k])
            real = ~np.isnan(mag)
            p = k + int(np.flatnonzero(real & (mag == mag[real].max()))[0]) if real.any() else k  # the smallest row that holds the maximum
            if pivots is not None:
                pivots.append(p)
            if p != k:
                E[[k, p]] = E[[p, k]]
            piv = E[k, k]
            if info == 0 and (piv == 0.0 or not np.isfinite(piv)):
                info = k + 1
            E[k] = E[k] / piv
            f = E[:, k].copy()  # taken before the rows change
            new = E - f[:, None] * E[k][None, :]  # the product, then the subtraction
            new[k] = E[k]
            E = new
    return E[:, m:].copy(), info


def host_dense_apply(m, inv, b):
    """x = inv b in the apply's order: the products rounded on their own, row_sum with a lane group of 64."""
    inv, b = np.asarray(inv, dtype=np.float64).reshape(m, m), np.asarray(b, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.array([row_sum(inv[i] * b, 64) for i in range(m)], dtype=np.float64)


# ---- the cases of the GPU suite, made once ----------------------------------------------------------------------------------------------------
def csr_of(D, keep=None):
    """The CSR of a dense array: the entries of `keep` (default: the non-zeros), rows ascending."""
    keep = D != 0.0 if keep is None else keep
    rp = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int32)
    i, j = np.nonzero(keep)
    return rp, j.astype(np.int32), D[i, j].astype(np.float64)


def random_matrix(m, rng, density=1.0):
    """Uniform entries in (-1, 1), none of them dominant: most steps swap.  density < 1: that share of the off-diagonals, and the diagonal."""
    D = rng.uniform(-1.0, 1.0, (m, m))
    keep = np.ones((m, m), dtype=bool) if density >= 1.0 else (rng.random((m, m)) < density) | np.eye(m, dtype=bool)
    return m, csr_of(D, keep)


def perm_matrix(perm):
    m = len(perm)
    return m, (np.arange(m + 1, dtype=np.int32), np.asarray(perm, dtype=np.int32), np.ones(m))


TIE = np.array([[1.0, 2.0, 0.5, -1.0], [-3.0, 1.0, 2.0, 0.25], [3.0, -1.0, 1.0, 2.0], [0.5, 0.75, -2.0, 1.0]])  # column 0: rows 1 and 2 tie at 3


def _cases():
    yield "one", 1, (np.array([0, 1], np.int32), np.array([0], np.int32), np.array([2.5]))
    yield "swap2", *perm_matrix([1, 0])
    yield "perm6", *perm_matrix([3, 0, 5, 1, 2, 4])
    yield "tie4", 4, csr_of(TIE)
    rng = np.random.default_rng(2033)
    for m in (63, 64, 65, 130):
        yield f"r{m}", *random_matrix(m, rng)
    yield "r257", *random_matrix(257, rng, density=0.08)
    yield "grid18", *grid5_matrix(18)


@functools.lru_cache(maxsize=None)
def cases():
    """tag -> (m, (rowptr, colindex, value)); made once and shared, nothing changes them."""
    return {tag: (m, A) for tag, m, A in _cases()}


TAGS = ("one", "swap2", "perm6", "tie4", "r63", "r64", "r65", "r130", "r257", "grid18")


@functools.lru_cache(maxsize=None)
def inverse(tag):
    """(inv, info, pivots) of a case by host_dense_inverse, computed once."""
    m, (rp, ci, v) = cases()[tag]
    pivots = []
    inv, info = host_dense_inverse(m, rp, ci, v, pivots)
    return inv, info, tuple(pivots)


def singular_cases():
    """tag -> (m, (rowptr, colindex, value)): a structurally zero column, a NaN entry, an empty row, no entries at all."""
    rng = np.random.default_rng(2034)
    m = 40
    D = rng.uniform(-1.0, 1.0, (m, m))
    keep = np.ones((m, m), dtype=bool)
    keep[:, 17] = False
    out = {"zero_column": (m, csr_of(D, keep))}
    N = D.copy()
    N[22, 9] = np.nan
    out["nan_entry"] = (m, csr_of(N, np.ones((m, m), dtype=bool)))
    keep = np.ones((m, m), dtype=bool)
    keep[31, :] = False
    out["empty_row"] = (m, csr_of(D, keep))
    out["no_entries"] = (5, (np.zeros(6, np.int32), np.zeros(0, np.int32), np.zeros(0)))
    return out


def test_the_cases():
    assert set(TAGS) == set(cases()) and len(TAGS) == len(set(TAGS))
    swaps = {}
    for tag in TAGS:
        m, (rp, ci, v) = cases()[tag]
        assert rp.size == m + 1 and rp[0] == 0 and rp[m] == ci.size == v.size, tag
        assert all(np.all(np.diff(ci[rp[i]:rp[i + 1]]) > 0) for i in range(m)), tag  # rows strictly ascend
        inv, info, pivots = inverse(tag)
        assert info == 0 and inv.shape == (m, m) and np.all(np.isfinite(inv)), tag
        swaps[tag] = sum(p != k for k, p in enumerate(pivots))
    assert swaps["one"] == 0 and swaps["swap2"] == 1 and swaps["perm6"] >= 3 and swaps["grid18"] == 0
    assert all(swaps[t] > cases()[t][0] // 2 for t in ("r63", "r64", "r65", "r130", "r257"))  # the random cases swap in most steps
    m, (rp, ci, v) = cases()["r257"]
    assert ci.size < 0.12 * m * m  # sparse: most of E's left half starts as +0.0


def test_inverse_residual():
    """max |A X - I| <= m cond_2(A) 2^-52 on the well-conditioned cases (measured: 4.7e-15 against 1.05e-11 on grid18, cond 146; the random
    130 x 130 case of this file is printed by the test)."""
    for tag in ("grid18", "r130", "r65", "tie4"):
        m, (rp, ci, v) = cases()[tag]
        A = to_dense(m, m, rp, ci, v)
        inv, info, _ = inverse(tag)
        err = float(np.max(np.abs(A @ inv - np.eye(m))))
        bound = m * np.linalg.cond(A, 2) * 2.0 ** -52
        print(f"{tag}: m = {m}, cond = {np.linalg.cond(A, 2):.3g}, max|A X - I| = {err:.3g}, bound {bound:.3g}")
        assert info == 0 and err <= bound, (tag, err, bound)
        assert np.allclose(inv, np.linalg.inv(A), rtol=0, atol=bound * np.max(np.abs(inv)))


def test_permutations_invert_exactly():
    for tag in ("swap2", "perm6"):
        m, (rp, ci, v) = cases()[tag]
        inv, info, pivots = inverse(tag)
        assert info == 0 and np.array_equal(inv, to_dense(m, m, rp, ci, v).T), tag  # exactly the transpose (-0.0 == +0.0)
    assert inverse("swap2")[2] == (1, 1) and np.array_equal(inverse("one")[0], [[0.4]])


def test_the_tie_takes_the_smaller_row():
    inv, info, pivots = inverse("tie4")
    assert pivots[0] == 1 and info == 0  # |-3| in row 1 and |+3| in row 2: the smaller row
    flipped = TIE.copy()
    flipped[[1, 2]] = flipped[[2, 1]]  # +3 first, -3 second: still row 1
    pivots = []
    host_dense_inverse(4, *csr_of(flipped), pivots)
    assert pivots[0] == 1


def test_singular_inputs_in_the_model():
    cases_ = singular_cases()
    m, (rp, ci, v) = cases_["zero_column"]
    assert host_dense_inverse(m, rp, ci, v)[1] == 17 + 1  # a structurally zero column c: info = c + 1
    for c in (0, 39):
        keep = np.ones((m, m), dtype=bool)
        keep[:, c] = False
        assert host_dense_inverse(m, *csr_of(to_dense(m, m, rp, ci, v) + np.eye(m), keep))[1] == c + 1
    m, (rp, ci, v) = cases_["nan_entry"]
    info = host_dense_inverse(m, rp, ci, v)[1]
    assert 1 <= info <= m  # the NaN spreads until a column holds nothing else: that step is flagged
    m, (rp, ci, v) = cases_["empty_row"]
    assert 1 <= host_dense_inverse(m, rp, ci, v)[1] <= m
    m, (rp, ci, v) = cases_["no_entries"]
    assert host_dense_inverse(m, rp, ci, v)[1] == 1
    assert host_dense_inverse(0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0)) [1] == 0


def test_host_apply_is_row_sum():
    rng = np.random.default_rng(3)
    for tag in ("one", "r63", "r65", "r130", "r257"):
        m, (rp, ci, v) = cases()[tag]
        inv = inverse(tag)[0]
        b = rng.standard_normal(m)
        x = host_dense_apply(m, inv, b)
        exact = inv.astype(np.longdouble) @ b.astype(np.longdouble)
        scale = np.abs(inv) @ np.abs(b)
        assert np.all(np.abs(x - exact) <= (m // 64 + 8) * 2.0 ** -52 * scale), tag  # m / 64 + 6 additions deep, one rounding per product
        i = m // 2
        lanes = [np.float64(0.0)] * 64
        for l in range(min(64, m)):  # lane l: its terms in order, from its first
            acc = inv[i, l] * b[l]
            for j in range(l + 64, m, 64):
                acc = acc + inv[i, j] * b[j]
            lanes[l] = acc
        while len(lanes) > 1:
            lanes = [lanes[t] + lanes[t + 1] for t in range(0, len(lanes), 2)]
        assert x[i] == lanes[0], tag
