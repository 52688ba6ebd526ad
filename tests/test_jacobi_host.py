"""CPU side of the damped Jacobi / l1-Jacobi smoother (no GPU): the C ABI declares and exports the two entries, they and the Python wrappers
refuse bad arguments before any launch, the compiled kernels use no scratch, no AGPR and no atomic, keep 8 waves per SIMD and hold no fused
operation outside a division's own expansion, every size-selected branch of the new code names the GPU tests that cross it, the engine file
stays stateless and launch-only, and the definitions are restated here in numpy, bit for bit, and exported to the GPU suite as its references:
the two inverse diagonals (host_jacobi_diagonal) and the sweep in its four modes with the documented summation order (host_jacobi_sweep).

The models are checked against independent formulations: the sweep against dense x + omega D^-1 (b - A x) in extended precision, row by row
within the row's rounding bound; the scaled l1 diagonal against its two theorems -- D - A is positive semidefinite on every symmetric positive
definite case at hand and one sweep at omega = 1 strictly reduces the energy norm of the error; D scales as A does, to 1e-13, on the matrix
scaled over six decades."""
import ctypes
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import spmv_acc_amd
from test_amg_host import IRREGULAR_TAGS, problem, scaling
from test_amg_host import TAGS as GRID_TAGS
from test_coo_host import SHARED, _FakeTensor, _f, _i
from test_gs_host import CHUNK_ROWS, HELPERS, ROW_SWEEP, TAGS, cases, lane_group, row_sum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "spmv_acc_amd/csrc/"
NEW_SOURCES = ("jacobi.hpp", "k_jacobi.hip", "jacobi.cpp")
DIAGONAL = "test_diagonal_is_the_host_model"
SWEEP = "test_sweep_is_the_host_model"
STRIDE = "test_jacobi_grid_stride_at_test_size"
CONTRACT = "test_sweep_contract"
KINDS = ("jacobi", "l1")

# (rule, file, regex that must match the source, GPU tests of tests/test_gpu_jacobi.py that cross it at test size, what it selects)
JACOBI_SIZE_RULES = [
    ("kJacobiTile", CSRC + "jacobi.hpp", r"constexpr int kJacobiTile = kGsChunkRows;",
     [DIAGONAL, SWEEP, STRIDE], "rows per workgroup: one chunk of 64 (path: 31 full chunks and one of 16; star, k130: short last chunks; one: a chunk of "
                                "one row), its passes dealt out to the four wavefronts"),
    ("kJacobiMaxRows", CSRC + "jacobi.hpp", r"constexpr int kJacobiMaxRows = kGsMaxRows;",
     [CONTRACT], "more rows than 32-bit gather offsets reach: SPMV_ACC_ERR_TOO_LARGE on the host"),
    ("the row limit's refusal", CSRC + "jacobi.cpp", r"if \(m > kJacobiMaxRows\)",
     [CONTRACT], "the sweep refuses 2^29 + 1 rows before any launch"),
    ("the lane group's rule", CSRC + ROW_SWEEP, r"while \(g < kWave && static_cast<u64>\(g\) \* kGsTermsPerLane \* rows_here < terms\) \{",
     [DIAGONAL, SWEEP], "the smallest G with G * 4 * rows of the chunk >= the chunk's terms: G = 1 (path, lonely), 2 (grid7), 4 (fem), 8 (grid27), 16, "
                        "32 (the bands), 64 (k130); test_the_lane_groups_of_the_cases holds the cases to that"),
    ("the passes of a chunk", CSRC + ROW_SWEEP, r"for \(int done = wave \* per_pass; done < rows_here; done \+= \(kThreads / kWave\) \* per_pass\) \{",
     [DIAGONAL, SWEEP], "a chunk of fewer rows than passes x rows per pass leaves wavefronts without a pass (one: one row; k130's last chunk: 2 rows at G = 64)"),
    ("tile loop", CSRC + ROW_SWEEP,
     r"for \(long long tile = blockIdx\.x; tile < ntiles; tile \+= gridDim\.x\) \{ // \(block-uniform\)\n    const long long base = first \+ tile \* kGsTile",
     [STRIDE], "blocks stride over the chunks beyond the grid (the stride test: 1 331 chunks over 64 workgroups)"),
    ("row loops of the inverse diagonal and the zero start", CSRC + "k_jacobi.hip", r"r < m; r \+= stride\) \{",
     [STRIDE], "one row per lane, striding (the stride test: 85 184 rows over 64 workgroups)"),
    ("kMaxGridBlocks (grid striding)", CSRC + SHARED, r"const long long cap = max_grid_blocks\(\);",
     [STRIDE], "every kernel of the two entries strides over the work beyond max_grid_blocks() workgroups"),
    ("kMaxGridBlocks (grid striding): the sweep's call", CSRC + "k_jacobi.hip", r"dim3\(grid_for\(m, kJacobiTile\)\)",
     [STRIDE], "the launchers take the shared grid"),
    ("a row without a diagonal", CSRC + "k_jacobi.hip", r"dinv\[i\] = has_diag \? 1\.0 / s : 0\.0;",
     [DIAGONAL], "+0.0 (fem_holes, grid7_holes, empties, one_empty); kind 0: the binary search misses"),
    ("a column outside [0, m)", CSRC + ROW_SWEEP, r"return static_cast<unsigned>\(t\.c\) >= static_cast<unsigned>\(m\) \? 0\.0 : w;",
     [CONTRACT], "the term +0.0, and no address is formed from the column"),
    ("the zero start", CSRC + "jacobi.cpp", r"if \(d_x_in\) launch_jacobi_sweep\(",
     [SWEEP, "test_captured_and_replayed"], "x_in == NULL: the one-row-per-lane kernel that does not read the matrix"),
    ("the two diagonals", CSRC + "jacobi.cpp", r"if \(kind == 0\) \{",
     [DIAGONAL], "kind 0: one launch; kind 1: the roots (launch_strength_sd) and the row sums"),
    ("no rows", CSRC + "jacobi.cpp", r"if \(m == 0\) return kOk;",
     [DIAGONAL, SWEEP], "m == 0 (the case none): nothing is launched"),
    ("int32 block arithmetic", CSRC + HELPERS, r"inline bool too_large\(long long v\) \{ return v > INT_MAX - \(1 << 16\); \}",
     [CONTRACT], "m or nnz beyond this: SPMV_ACC_ERR_TOO_LARGE, as the other entries"),
]


def test_jacobi_size_rules_name_their_tests():
    gpu_tests = open(os.path.join(ROOT, "tests", "test_gpu_jacobi.py")).read()
    defined = set(re.findall(r"^def (test_\w+)\(", gpu_tests, flags=re.M))
    for name, path, pattern, tests, what in JACOBI_SIZE_RULES:
        assert re.search(pattern, open(os.path.join(ROOT, path)).read()), f"{name}: no longer matches {path}: {pattern}"
        assert tests and what
        for t in tests:
            assert t in defined, f"{name}: names {t}, which is not a test of tests/test_gpu_jacobi.py"
    registered = " ".join(r[0] + " " + r[2] for r in JACOBI_SIZE_RULES)
    found = 0
    for f in NEW_SOURCES:
        for k in re.findall(r"constexpr\s+[\w:<> ]+?\s+(k[A-Z]\w*)\s*=", open(os.path.join(ROOT, CSRC, f)).read()):
            found += 1
            assert k in registered, f"{f}: constant {k} is not in JACOBI_SIZE_RULES"
    assert found == 2
    # every loop over work is one of the registered forms: the one tile loop stands in the shared body (kJacobiTile is kGsTile)
    kernels, body = open(os.path.join(ROOT, CSRC, "k_jacobi.hip")).read(), open(os.path.join(ROOT, CSRC, ROW_SWEEP)).read()
    assert body.count("tile += gridDim.x") == 1 and kernels.count("tile += gridDim.x") == 0 and kernels.count("+= stride)") == 2
    assert "constexpr int kGsTile = kGsChunkRows;" in open(os.path.join(ROOT, CSRC, "gs.hpp")).read()
    # the l1 diagonal and the sweep share that body with the Gauss-Seidel sweep: all rows are the one colour
    assert kernels.count("lane_group_rows(m, nnz, rowptr, colindex, value, 0, m, rows);") == 2 and kernels.count("lane_group_rows(") == 2


PROTOTYPES = (
    r"int spmv_acc_csr_jacobi_diagonal\(int m, int nnz, const int \*d_rowptr, const int \*d_colindex, const double \*d_value,\s*"
    r"int kind, double \*d_dinv, double \*d_work\);",
    r"int spmv_acc_csr_jacobi_sweep\(int m, int nnz, const int \*d_rowptr, const int \*d_colindex, const double \*d_value,\s*"
    r"const double \*d_dinv, double omega, const double \*d_b, const double \*d_x_in,\s*double \*d_x_out, double \*d_r_out\);",
)


def test_jacobi_entries_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "spmv_acc.h")).read()
    for proto in PROTOTYPES:
        assert re.search(proto, header), proto
    for entry in ("1", "2"):
        block = re.search(r"/\* ---- damped Jacobi / l1-Jacobi, " + entry + r".*?\*/", header, flags=re.S)
        assert block, entry
        for word in ("replaces: nothing in the reference", "COST", "CHECKS", "CANNOT CHECK", "profiles/jacobi_bench.md"):
            assert word in block.group(0), (entry, word)
    declared = set(re.findall(r"\b(sparse_spmv|spmv_acc_[a-z_0-9]+)\s*\(", header))
    assert declared == set(spmv_acc_amd.C_ABI_SYMBOLS), declared ^ set(spmv_acc_amd.C_ABI_SYMBOLS)
    lib = spmv_acc_amd.load_library()
    for s in ("spmv_acc_csr_jacobi_diagonal", "spmv_acc_csr_jacobi_sweep"):
        assert s in spmv_acc_amd.C_ABI_SYMBOLS and hasattr(lib, s), s
    assert lib.spmv_acc_csr_jacobi_diagonal.restype is ctypes.c_int and lib.spmv_acc_csr_jacobi_sweep.restype is ctypes.c_int
    assert len(lib.spmv_acc_csr_jacobi_diagonal.argtypes) == 8 and len(lib.spmv_acc_csr_jacobi_sweep.argtypes) == 11
    assert lib.spmv_acc_csr_jacobi_sweep.argtypes[6] is ctypes.c_double and lib.spmv_acc_csr_jacobi_diagonal.argtypes[5] is ctypes.c_int
    for f in ("csr_jacobi_diagonal", "csr_jacobi_sweep"):
        assert callable(getattr(spmv_acc_amd, f))
    makefile, cmake = open(os.path.join(ROOT, CSRC, "Makefile")).read(), open(os.path.join(ROOT, "CMakeLists.txt")).read()
    for f in ("k_jacobi.hip", "jacobi.cpp"):  # both builds compile the new files
        assert f in makefile and f in cmake, f
    assert "jacobi.hpp" in makefile
    assert " k_jacobi " in open(os.path.join(ROOT, "tools", "resource_usage.sh")).read()
    # the header documents the definition, the order and both theorems
    doc = open(os.path.join(ROOT, CSRC, "jacobi.hpp")).read().split("#pragma once")[0]
    for word in ("THE DIAGONALS", "THE SWEEP", "THE SUMMATION ORDER", "ZERO START", "AM-GM", "D >= A", "S A S", "2^32"):
        assert word in doc, word


BAD, TOO_LARGE = 2, 4  # SPMV_ACC_ERR_BAD_ARGUMENT, SPMV_ACC_ERR_TOO_LARGE


def test_bad_arguments_are_refused_without_a_gpu():
    """The C entries check their arguments before they touch the device: the error codes come back on a machine without one."""
    lib = spmv_acc_amd.load_library()
    one = 8  # (never dereferenced: a non-null pointer value)
    at = [k << 20 for k in range(1, 6)]  # five arrays far apart

    def diagonal(m=4, nnz=8, rp=one, ci=one, v=one, kind=1, dinv=at[0], work=at[1]):
        return lib.spmv_acc_csr_jacobi_diagonal(m, nnz, rp, ci, v, kind, dinv, work)

    for neg in ("m", "nnz"):
        assert diagonal(**{neg: -1}) == BAD, neg
        assert b"spmv_acc_csr_jacobi_diagonal: negative" in lib.spmv_acc_last_error_string()
    for kind in (-1, 2, 7):
        assert diagonal(kind=kind) == BAD and b"kind" in lib.spmv_acc_last_error_string()
    for null in ("rp", "ci", "v", "dinv", "work"):
        assert diagonal(**{null: None}) == BAD, null
        assert b"spmv_acc_csr_jacobi_diagonal: null" in lib.spmv_acc_last_error_string(), null
    for big in (2 ** 31 - 1, 2 ** 31 - 2 ** 16):
        for which in ("m", "nnz"):
            assert diagonal(**{which: big}) == TOO_LARGE, which
            assert b"spmv_acc_csr_jacobi_diagonal:" in lib.spmv_acc_last_error_string()
    assert diagonal(m=2 ** 29 + 1) == TOO_LARGE and b"2^29" in lib.spmv_acc_last_error_string()
    for work in (at[0], at[0] + 8, at[0] - 24, at[0] + 24):
        assert diagonal(work=work) == BAD and b"overlaps" in lib.spmv_acc_last_error_string(), work
    # no rows: nothing to do, the device is not touched; kind 0 needs no work vector (no device here: only the refusals can be told apart)
    assert diagonal(m=0, nnz=0, rp=None, ci=None, v=None, dinv=None, work=None) == 0 and lib.spmv_acc_last_error() == 0
    assert diagonal(m=0, nnz=0, rp=None, ci=None, v=None, kind=0, dinv=None, work=None) == 0 and lib.spmv_acc_last_error() == 0

    def sweep(m=4, nnz=8, rp=one, ci=one, v=one, dinv=at[0], omega=1.0, b=at[1], x_in=at[2], x_out=at[3], r_out=at[4]):
        return lib.spmv_acc_csr_jacobi_sweep(m, nnz, rp, ci, v, dinv, omega, b, x_in, x_out, r_out)

    for neg in ("m", "nnz"):
        assert sweep(**{neg: -1}) == BAD, neg
        assert b"spmv_acc_csr_jacobi_sweep: negative" in lib.spmv_acc_last_error_string()
    for null in ("rp", "ci", "v", "dinv", "b"):
        assert sweep(**{null: None}) == BAD, null
        assert b"spmv_acc_csr_jacobi_sweep: null" in lib.spmv_acc_last_error_string(), null
    assert sweep(x_out=None, r_out=None) == BAD and b"null x_out and r_out" in lib.spmv_acc_last_error_string()
    assert sweep(x_in=None, x_out=None, r_out=None) == BAD
    for omega in (np.inf, -np.inf, np.nan):
        assert sweep(omega=omega) == BAD and b"omega is not finite" in lib.spmv_acc_last_error_string(), omega
    names = ("x_out", "r_out", "x_in", "b", "dinv")
    for a in range(5):  # any overlap among the five
        for o in range(a + 1, 5):
            for shift in (0, 8, -24, 24):
                place = dict(x_out=at[3], r_out=at[4], x_in=at[2], b=at[1], dinv=at[0])
                place[names[o]] = place[names[a]] + shift
                assert sweep(**place) == BAD, (names[a], names[o], shift)
                msg = lib.spmv_acc_last_error_string()
                assert (names[a] + " overlaps " + names[o]).encode() in msg and b"out of place" in msg, msg
    for big in (2 ** 31 - 1, 2 ** 31 - 2 ** 16):
        for which in ("m", "nnz"):
            assert sweep(**{which: big}) == TOO_LARGE, which
            assert b"spmv_acc_csr_jacobi_sweep:" in lib.spmv_acc_last_error_string()
    assert sweep(m=2 ** 29 + 1) == TOO_LARGE and b"2^29" in lib.spmv_acc_last_error_string()
    assert sweep(m=0, nnz=0, rp=None, ci=None, v=None, dinv=None, b=None, x_in=None, x_out=None, r_out=None) == 0
    assert lib.spmv_acc_last_error() == 0
    lib.spmv_acc_clear_error()


def test_wrappers_refuse_bad_arguments():
    E = spmv_acc_amd.SpmvAccError
    m, nnz = 10, 30

    def diagonal(match, mm=m, rp=_i(m + 1), ci=_i(nnz), v=_f(nnz), kind="l1"):
        with pytest.raises(E, match=match):
            spmv_acc_amd.csr_jacobi_diagonal(mm, rp, ci, v, kind=kind)

    diagonal("not on the GPU", ci=_i(nnz, cuda=False))
    diagonal("dtype", rp=_FakeTensor(m + 1, dtype="torch.int64"))
    diagonal("dtype", ci=_f(nnz))
    diagonal("dtype", v=_i(nnz))
    diagonal("not contiguous", v=_f(nnz, contiguous=False))
    diagonal("elements", rp=_i(m))
    diagonal("elements", v=_f(nnz - 1))
    diagonal("as many", v=_f(nnz + 1))
    diagonal("on cuda:1", v=_f(nnz, device="cuda:1"))
    diagonal("torch tensor", rp=None)
    diagonal("torch tensor", v=[0.0] * nnz)
    diagonal("negative", mm=-1)
    diagonal("kind", kind="l2")
    diagonal("kind", kind=1)

    good = dict(rp=_i(m + 1), ci=_i(nnz), v=_f(nnz), dinv=_f(m), b=_f(m), x_in=_f(m), x_out=_f(m), r_out=_f(m))

    def sweep(match, mm=m, omega=1.0, **bad):
        a = dict(good, **bad)
        with pytest.raises(E, match=match):
            spmv_acc_amd.csr_jacobi_sweep(mm, a["rp"], a["ci"], a["v"], a["dinv"], a["b"], a["x_in"], x_out=a["x_out"], r_out=a["r_out"], omega=omega)

    sweep("not on the GPU", v=_f(nnz, cuda=False))
    sweep("not on the GPU", dinv=_f(m, cuda=False))
    sweep("dtype", rp=_FakeTensor(m + 1, dtype="torch.int64"))
    sweep("dtype", v=_i(nnz))
    sweep("dtype", b=_i(m))
    sweep("dtype", x_in=_i(m))
    sweep("dtype", r_out=_i(m))
    sweep("not contiguous", x_out=_f(m, contiguous=False))
    sweep("elements", rp=_i(m))
    sweep("elements", v=_f(nnz - 1))
    sweep("elements", b=_f(m - 1))
    sweep("elements", dinv=_f(m - 1))
    sweep("elements", x_in=_f(m - 1))
    sweep("elements", x_out=_f(m - 1))
    sweep("elements", r_out=_f(m - 1))
    sweep("as many", v=_f(nnz + 1))
    sweep("on cuda:1", x_out=_f(m, device="cuda:1"))
    sweep("torch tensor", v=None)
    sweep("torch tensor", dinv=None)
    sweep("torch tensor", b=[0.0] * m)
    sweep("torch tensor", x_in=3.0)
    sweep("torch tensor", r_out=[0.0] * m)
    sweep("negative", mm=-1)
    sweep("nothing to write", x_out=None, r_out=None)
    sweep("omega", omega=float("nan"))
    sweep("omega", omega=float("inf"))
    sweep("omega", omega="1")


def test_jacobi_entries_keep_no_state():
    """As test_gs_entries_keep_no_state: the engine file neither finds nor makes a plan, counts no plan work, reads no tunable and keeps
    nothing static; BOTH entries are launch-only: no allocation, no synchronise, no copy, no memset."""
    src = open(os.path.join(ROOT, CSRC, "jacobi.cpp")).read()
    code = re.sub(r"//[^\n]*", "", src)
    for word in ("get_plan", "g_plans", "t_plan_work", "t_last_plan", "tune_", "TimingPhase", "TuneTimer", "static std::", "thread_local", "g_tunables"):
        assert word not in code, word
    assert not re.search(r"\bstatic\b(?! const char \*const kEntry)", code), "a static other than the entries' names"
    for word in ("hipMalloc", "hipFree", "Synchronize", "hipMemcpy", "hipMemset", "plan_work_allowed", "pattern_census", "launch_gs_"):
        assert word not in code, word
    assert '#include "' + HELPERS + '"' in src and '#include "strength.hpp"' in src
    diagonal, sweep = code.split("int run_csr_jacobi_diagonal")[1].split("int run_csr_jacobi_sweep")
    assert re.findall(r"\blaunch_\w+\(", diagonal) == ["launch_jacobi_inverse(", "launch_strength_sd(", "launch_jacobi_l1(", "launch_error("]
    assert re.findall(r"\blaunch_\w+\(", sweep) == ["launch_jacobi_sweep(", "launch_jacobi_start(", "launch_error("]  # one launch, either form
    for body in (diagonal, sweep):  # every refusal stands before the stream is taken
        assert body.index("hipStream_t st = t_stream;") > max(mt.start() for mt in re.finditer(r"return entry_error\(kEntry, kErr(BadArgument|TooLarge)", body))
        assert body.index("if (m == 0) return kOk;") < body.index("hipStream_t st = t_stream;")
    assert set(re.findall(r"\b(\w*(?:too_large|overlap))\(", code)) == {"too_large", "overlap"}  # entry_helpers.hpp's, no copies
    # the files that must not change with this feature still offer what it calls
    for f, offered in (("structure_passes.hpp", "row_extent("), ("structure_passes.hpp", "grid_for("), ("strength.hpp", "void launch_strength_sd("),
                       ("gs.hpp", "constexpr int kGsTermsPerLane = 4;"), ("device_utils.hpp", "group_sum_dyn(")):
        assert offered in open(os.path.join(ROOT, CSRC, f)).read(), (f, offered)


KERNELS = ("jacobi_inverse_kernel", "jacobi_start_kernel", "jacobi_sweep_kernel", "jacobi_l1_kernel")
# as recorded in k_jacobi.hip's header comment
RECORDED_VGPRS = dict(jacobi_inverse_kernel=12, jacobi_start_kernel=10, jacobi_sweep_kernel=39, jacobi_l1_kernel=52)


def test_jacobi_kernels_fit_their_register_budget(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_table

    asm = tmp_path / "k_jacobi.s"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-DKERNEL_STRATEGY_ADAPTIVE",
                        "-I" + os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-S",
                        os.path.join(ROOT, CSRC, "k_jacobi.hip"), "-o", str(asm)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    text = asm.read_text()
    assert set(re.findall(r"\.wavefront_size:\s*(\d+)", text)) == {"64"}  # wave64, every kernel of the file
    bodies = {}
    for mt in re.finditer(r"^(_ZN8spmv_acc\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, flags=re.M | re.S):
        bodies[mt.group(1)] = mt.group(2)
    assert len(bodies) == len(KERNELS), sorted(bodies)

    def body(name):
        return next(b for k, b in bodies.items() if name in k)

    def fused(b):
        return b.count("v_fma_f64") + b.count("v_fmac_f64")

    for k, b in bodies.items():
        assert "atomic" not in b, k  # no atomics anywhere
        assert "s_sleep" not in b, k  # ... and nothing waits
    # contraction is off.  The sweep and the zero start hold no division and so no fused operation at all: products and sums are instructions
    # of their own
    for name in ("jacobi_sweep_kernel", "jacobi_start_kernel"):
        assert fused(body(name)) == 0 and "v_div_" not in body(name), name
    assert "v_mul_f64" in body("jacobi_sweep_kernel") and "v_add_f64" in body("jacobi_sweep_kernel")
    assert body("jacobi_start_kernel").count("v_mul_f64") == 2  # omega * dinv, then * b
    # the inverse diagonal is one division and nothing else: what it holds IS a division's own expansion ...
    inverse = body("jacobi_inverse_kernel")
    assert inverse.count("v_div_fixup_f64") == 1 and "v_add_f64" not in inverse
    per_division = fused(inverse)
    assert per_division > 0 and inverse.count("v_mul_f64") == 1  # (the expansion's own product)
    # ... and the l1 kernel's fused operations are exactly those of its divisions (the ratios and the final reciprocal), no more
    l1 = body("jacobi_l1_kernel")
    divisions = l1.count("v_div_fixup_f64")
    assert divisions >= 5 and fused(l1) == per_division * divisions, (divisions, fused(l1), per_division)
    assert l1.count("v_mul_f64") > divisions and "v_add_f64" in l1  # |a_ij| * ratio and the sums, rounded on their own
    header = open(os.path.join(ROOT, CSRC, "k_jacobi.hip")).read().split("#include")[0]
    rows = [k for k in resource_table.parse(r.stderr) if "rocprim" not in k["name"]]
    assert sorted(k["name"] for k in rows) == sorted(KERNELS), sorted(k["name"] for k in rows)
    for k in rows:
        assert k["scratch"] == 0 and k["agprs"] == 0 and k["vgprs"] <= 64 and k["occupancy"] >= 8, k
        want = RECORDED_VGPRS[k["name"]]
        assert re.search(k["name"] + r", " + str(want) + r"\b", header), (k["name"], "the count recorded in the header comment")
        assert abs(k["vgprs"] - want) <= 4, (k, "left the count recorded in k_jacobi.hip (a few registers of compiler drift are allowed)")


# ---- the definitions (jacobi.hpp), in numpy, bit for bit: the GPU suite's references -----------------------------------------------------------------
def extents(m, rp, nnz):
    """The clamped extents of all rows (passes::row_extent)."""
    lo = np.clip(np.asarray(rp[:m], dtype=np.int64), 0, nnz)
    hi = np.clip(np.maximum(np.asarray(rp[1:m + 1], dtype=np.int64), lo), None, nnz)
    return lo, hi


def positions(lo, hi):
    """(owner, pos): every (row, position) of the clamped extents, row by row (crafted extents may overlap: a position may have two owners)."""
    lens = hi - lo
    owner = np.repeat(np.arange(lo.size, dtype=np.int64), lens)
    first = np.concatenate([[0], np.cumsum(lens)])[:-1]
    return owner, lo[owner] + (np.arange(owner.size, dtype=np.int64) - first[owner])


def chunk_sums(terms, owner, lo, hi):
    """The sums of all rows in the documented order: chunks of CHUNK_ROWS consecutive rows, G by lane_group from the chunk's clamped lengths,
    then row_sum's order for every row of the chunk at once (test_chunk_sums_is_row_sum holds the two together).  terms: one per entry of
    positions(lo, hi)."""
    m = lo.size
    lens = hi - lo
    first = np.concatenate([[0], np.cumsum(lens)])
    place = np.arange(owner.size, dtype=np.int64) - first[owner]  # the term's number within its row
    out = np.zeros(m)
    with np.errstate(all="ignore"):
        for base in range(0, m, CHUNK_ROWS):
            rows = np.arange(base, min(base + CHUNK_ROWS, m))
            a, b = first[rows[0]], first[rows[-1] + 1]
            g = lane_group(int(b - a), rows.size)
            steps = max(-(-int(lens[rows].max()) // g), 1)
            padded = np.zeros((rows.size, steps * g))
            padded[owner[a:b] - base, place[a:b]] = terms[a:b]
            live = (np.arange(steps * g)[None, :] < lens[rows][:, None]).reshape(rows.size, steps, g)
            padded = padded.reshape(rows.size, steps, g)
            part = padded[:, 0, :].copy()  # (a lane without a term holds +0.0)
            for s in range(1, steps):
                part = np.where(live[:, s, :], part + padded[:, s, :], part)
            while part.shape[1] > 1:
                part = part[:, 0::2] + part[:, 1::2]
            out[rows] = part[:, 0]
    return out


def stored_diagonal(m, rp, ci):
    """(position or -1) of every row's diagonal as the one-row-per-lane kernels find it: passes::first_at_least on the clamped row, all rows
    in step."""
    lo, hi = extents(m, rp, ci.size)
    i = np.arange(m, dtype=np.int64)
    a, b = lo.copy(), hi.copy()
    while np.any(a < b):
        open_ = a < b
        mid = np.where(open_, a + (b - a) // 2, 0)
        less = ci[np.minimum(mid, max(ci.size - 1, 0))] < i if ci.size else np.zeros(m, dtype=bool)
        a = np.where(open_ & less, mid + 1, a)
        b = np.where(open_ & ~less, mid, b)
    found = (a < hi) & (ci[np.minimum(a, max(ci.size - 1, 0))] == i) if ci.size else np.zeros(m, dtype=bool)
    return np.where(found, a, -1)


def host_jacobi_diagonal(m, rp, ci, v, kind="l1"):
    """dinv as spmv_acc_csr_jacobi_diagonal leaves it."""
    assert kind in KINDS
    ci64, v = np.asarray(ci, dtype=np.int64), np.asarray(v, dtype=np.float64)
    if m == 0:
        return np.zeros(0)
    at = stored_diagonal(m, rp, ci64)
    a_ii = v[np.maximum(at, 0)] if v.size else np.zeros(m)
    with np.errstate(all="ignore"):
        if kind == "jacobi":
            return np.where(at >= 0, 1.0 / a_ii, 0.0)
        g = np.where(at >= 0, np.sqrt(np.abs(a_ii)), 0.0)
        lo, hi = extents(m, rp, ci64.size)
        owner, pos = positions(lo, hi)
        cols = ci64[pos]
        inside = (cols >= 0) & (cols < m)
        ratio = g[owner] / g[np.where(inside, cols, 0)]  # rounded first
        d = chunk_sums(np.where(inside, np.abs(v[pos]) * ratio, 0.0), owner, lo, hi)
        has = np.bincount(owner[cols == owner], minlength=m) > 0  # (met in passing, as the sweep's lanes meet it)
        return np.where(has, 1.0 / d, 0.0)


def host_jacobi_sweep(m, rp, ci, v, dinv, b, x_in, omega=1.0):
    """(x_out, r_out) as spmv_acc_csr_jacobi_sweep leaves them; x_in None: the zero start."""
    ci64, v = np.asarray(ci, dtype=np.int64), np.asarray(v, dtype=np.float64)
    b, dinv, omega = np.asarray(b, dtype=np.float64), np.asarray(dinv, dtype=np.float64), np.float64(omega)
    with np.errstate(all="ignore"):
        w = omega * dinv
        if x_in is None:
            return w * b, b.copy()
        x_in = np.asarray(x_in, dtype=np.float64)
        if m == 0:
            return np.zeros(0), np.zeros(0)
        lo, hi = extents(m, rp, ci64.size)
        owner, pos = positions(lo, hi)
        cols = ci64[pos]
        inside = (cols >= 0) & (cols < m)
        terms = np.where(inside, v[pos] * x_in[np.where(inside, cols, 0)], 0.0)  # every product rounded on its own
        t = b - chunk_sums(terms, owner, lo, hi)
        step = w * t
        return x_in + step, t


def test_chunk_sums_is_row_sum():
    """The vectorised order of this file is test_gs_host.row_sum's, row by row, on every case: the Gauss-Seidel sweep's order."""
    rng = np.random.default_rng(7)
    for tag in TAGS:
        m, (rp, ci, v) = cases()[tag]
        t = rng.standard_normal(ci.size) * 10.0 ** rng.integers(-6, 6, ci.size)
        lo, hi = extents(m, rp, ci.size)
        owner, pos = positions(lo, hi)
        got = chunk_sums(t[pos], owner, lo, hi)
        for base in range(0, m, CHUNK_ROWS):
            rows = range(base, min(base + CHUNK_ROWS, m))
            g = lane_group(int(sum(hi[i] - lo[i] for i in rows)), len(rows))
            for i in rows:
                assert got[i].tobytes() == np.float64(row_sum(t[lo[i]:hi[i]], g)).tobytes(), (tag, i)


def test_the_lane_groups_of_the_cases():
    """The chunks of consecutive rows cross every lane group, chunks of one row and short last chunks (JACOBI_SIZE_RULES)."""
    groups, short = set(), set()
    for tag in TAGS:
        m, (rp, ci, _) = cases()[tag]
        lens = np.diff(rp)
        for base in range(0, m, CHUNK_ROWS):
            rows = lens[base:base + CHUNK_ROWS]
            groups.add(lane_group(int(rows.sum()), rows.size))
            short.add(rows.size)
    assert groups == {1, 2, 4, 8, 16, 32, 64}, groups
    assert {1, 2, 16, 64} <= short, short


def dense(m, A):
    rp, ci, v = A
    D = np.zeros((m, m), dtype=np.longdouble)
    D[np.repeat(np.arange(m), np.diff(rp)), ci] = v
    return D


def test_host_sweep_against_the_dense_update():
    """x + omega D^-1 (b - A x) with dense numpy in extended precision, every row within its own rounding bound
    (len + 4) 2^-53 (|b_i| + sum |a_ij| |x_j|) |w_i| + 2^-53 |x_i|; the residual mode within (len + 1) 2^-53 of the same scale; the zero start
    and the both-at-once mode are the same numbers."""
    rng = np.random.default_rng(11)
    for tag in ("fem", "grid7", "grid27", "path", "star", "k130", "band50", "lonely"):
        m, A = cases()[tag]
        rp, ci, v = A
        D = dense(m, A)
        b, x = rng.standard_normal(m), rng.standard_normal(m)
        for kind, omega in (("l1", 1.0), ("jacobi", 0.7)):
            dinv = host_jacobi_diagonal(m, rp, ci, v, kind)
            got_x, got_r = host_jacobi_sweep(m, rp, ci, v, dinv, b, x, omega)
            w = np.float64(omega) * dinv
            exact_r = b.astype(np.longdouble) - D @ x.astype(np.longdouble)
            exact_x = x.astype(np.longdouble) + w.astype(np.longdouble) * exact_r
            scale = np.abs(b) + np.asarray(np.abs(D) @ np.abs(x), dtype=np.float64)
            bound = (np.diff(rp) + 4) * 2.0 ** -53 * scale * np.abs(w) + 2.0 ** -53 * np.abs(x)
            assert np.all(np.abs(got_x - exact_x) <= bound), (tag, kind, float(np.max(np.abs(got_x - exact_x) / bound)))
            assert np.all(np.abs(got_r - exact_r) <= (np.diff(rp) + 1) * 2.0 ** -53 * scale), (tag, kind)
        zx, zr = host_jacobi_sweep(m, rp, ci, v, dinv, b, None, 0.7)
        assert np.array_equal(zr, b) and np.array_equal(zx, (np.float64(0.7) * dinv) * b)
        fx, fr = host_jacobi_sweep(m, rp, ci, v, dinv, b, np.zeros(m), 0.7)
        assert np.array_equal(fx, zx) and np.array_equal(fr, zr), tag  # from an x of zeros: the same numbers


def test_host_diagonal_against_its_definition():
    """kind jacobi is 1 / a_ii; kind l1 against the dense sum |a_ij| g_i / g_j in extended precision to (len + 3) roundings; rows without a
    diagonal give +0.0 under both."""
    for tag in TAGS:
        m, A = cases()[tag]
        if m == 0:
            assert host_jacobi_diagonal(0, *A, "l1").size == 0 and host_jacobi_diagonal(0, *A, "jacobi").size == 0
            continue
        rp, ci, v = A
        D = dense(m, A)
        row = np.repeat(np.arange(m), np.diff(rp))
        has = np.zeros(m, dtype=bool)
        has[row[ci == row]] = True
        jac, l1 = host_jacobi_diagonal(m, rp, ci, v, "jacobi"), host_jacobi_diagonal(m, rp, ci, v, "l1")
        assert np.array_equal(jac[has], 1.0 / np.asarray(np.diag(D), dtype=np.float64)[has]), tag
        for dinv in (jac, l1):
            assert np.all(dinv[~has] == 0.0) and not np.any(np.signbit(dinv[~has])), tag
        g = np.sqrt(np.abs(np.diag(D)))
        clean = has & np.array([bool(np.all(has[ci[rp[i]:rp[i + 1]]])) for i in range(m)])  # rows whose neighbours all hold a diagonal
        assert clean.sum() > 0 or tag in ("one_empty",), tag
        with np.errstate(all="ignore"):
            exact = np.asarray((np.abs(D) * (g[:, None] / np.where(g > 0, g, 1)[None, :])).sum(axis=1), dtype=np.float64)
        assert np.all(np.abs(1.0 / l1[clean] - exact[clean]) <= (np.diff(rp)[clean] + 3) * 2.0 ** -52 * exact[clean]), tag
        dirty = has & ~clean  # a neighbour without a diagonal: |a_ij| g_i / 0 = inf, 1 / inf = +0.0
        assert np.all(l1[dirty] == 0.0), tag


def spd_cases():
    """(tag, m, A) of every symmetric positive definite matrix at hand: grid7, the four grid hierarchies' and the five irregular ones."""
    yield ("grid7",) + cases()["grid7"]
    for tag in GRID_TAGS + IRREGULAR_TAGS:
        m, A = problem(tag)[:2]
        yield tag, m, A


@functools.lru_cache(maxsize=None)
def l1_inverse(tag):
    m, A = next((m, A) for t, m, A in spd_cases() if t == tag)
    return host_jacobi_diagonal(m, *A, "l1")


SPD_TAGS = ("grid7",) + GRID_TAGS + IRREGULAR_TAGS


@pytest.mark.parametrize("tag", SPD_TAGS)
def test_the_l1_diagonal_bounds_the_matrix(tag):
    """D - A is positive semidefinite (smallest eigenvalue >= -1e-12 ||A||), and one l1 sweep at omega = 1 strictly reduces the energy norm of
    the error."""
    assert "fem_scaled" in SPD_TAGS and len(SPD_TAGS) == 10
    m, A = next((m, A) for t, m, A in spd_cases() if t == tag)
    rp, ci, v = A
    D = np.asarray(dense(m, A), dtype=np.float64)
    assert np.array_equal(D, D.T) and np.all(np.diag(D) > 0)
    dinv = l1_inverse(tag)
    # (on the matrix scaled over six decades the eigenvalues are taken of the symmetrically scaled pencil: the same signs, by Sylvester)
    s = 1.0 / np.sqrt(np.diag(D))
    gap = (np.diag(1.0 / dinv) - D) * s[:, None] * s[None, :]
    norm = float(np.linalg.norm(D * s[:, None] * s[None, :], 2))
    low = float(np.linalg.eigvalsh(gap).min())
    print(f"{tag}: smallest eigenvalue of the scaled D - A {low:.3e}, ||A|| {norm:.3e}")
    assert low >= -1e-12 * norm, (tag, low)
    plain = float(np.linalg.eigvalsh(np.diag(1.0 / dinv) - D).min())
    assert plain >= -1e-12 * float(np.linalg.norm(D, 2)), (tag, plain)
    rng = np.random.default_rng(17)
    star = rng.standard_normal(m) * (1.0 / scaling() if tag == "fem_scaled" else 1.0)
    b = np.asarray(dense(m, A) @ star.astype(np.longdouble), dtype=np.float64)

    def energy(e):
        e = e.astype(np.longdouble)
        return float(np.sqrt(e @ (dense(m, A) @ e)))

    x = np.zeros(m)
    norms = [energy(x - star)]
    for _ in range(3):
        x = host_jacobi_sweep(m, rp, ci, v, dinv, b, x, 1.0)[0]
        norms.append(energy(x - star))
    assert all(later < earlier for earlier, later in zip(norms, norms[1:])), (tag, norms)


def test_the_l1_diagonal_scales_with_the_matrix():
    """fem_scaled is S A S of fem_mixed with S = diag(d): its l1 diagonal is d_i^2 times the twin's, to 1e-13 relative."""
    (m, A), (ms, As) = problem("fem_mixed")[:2], problem("fem_scaled")[:2]
    d = scaling()
    row = np.repeat(np.arange(m), np.diff(A[0]))
    assert m == ms and np.array_equal(A[0], As[0]) and np.array_equal(A[1], As[1]) and np.array_equal(As[2], A[2] * (d[row] * d[A[1]]))
    twin, scaled = 1.0 / l1_inverse("fem_mixed"), 1.0 / l1_inverse("fem_scaled")
    err = np.abs(scaled - d * d * twin) / (d * d * twin)
    print(f"largest relative difference {err.max():.3e}")
    assert err.max() <= 1e-13
    # the plain row sum of |a_ij| has no such property: it is the wrong diagonal on this matrix by orders of magnitude
    plain = np.bincount(row, np.abs(As[2]), m)
    assert np.max(plain / scaled) > 1e2
