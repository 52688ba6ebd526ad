"""CPU side of the multicolour Gauss-Seidel / SOR smoother (no GPU): the C ABI declares and exports the two entries, they and the Python
wrappers refuse bad arguments before any launch, the compiled kernels use no scratch, no AGPR and no atomic and fit 64 VGPRs, every
size-selected branch of the new code names the GPU tests that cross it, the engine file stays stateless, and the definitions are restated here
in numpy and exported to the GPU suite as its references: the colouring (host_csr_color, the sequential greedy; host_csr_color_rounds, the round
form, which must give the same colours) and the sweep with its documented summation order (host_gs_sweep, bit for bit), checked against an
independent formulation: on the colour-permuted matrix one forward sweep with omega = 1 solves (D + L) x' = b - U x."""
import ctypes
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import spmv_acc_amd
from spmv_acc_amd import synth
from test_coo_host import HELPERS, SHARED, _FakeTensor, _f, _i, host_assemble  # (HELPERS: defined below the files this one imports from)
from test_extract_host import host_csr_permute

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "spmv_acc_amd/csrc/"
NEW_SOURCES = ("gs.hpp", "k_gs.hip", "gs.cpp")
ROW_SWEEP = "row_sweep.hpp"  # the one row-sum body of gs_color_kernel and the two Jacobi kernels: test_jacobi_host.py's table names it too
ENTRY_FILES = ("gs.cpp", "agg.cpp", "strength.cpp", "dense.cpp")  # the four that share the pattern census
SOLVER_FILES = ("cg.cpp", "jacobi.cpp")
STRUCTURAL_FILES = ("coo.cpp", "transpose.cpp", "spmm.cpp", "spgemm.cpp", "csr_add.cpp", "extract.cpp")
COLOR = "test_color_is_the_host_model"
SWEEP = "test_sweep_is_the_host_model"
STRIDE = "test_gs_grid_stride_at_test_size"
COLOR_CONTRACT = "test_color_contract"
SWEEP_CONTRACT = "test_sweep_contract"
CHUNK_ROWS, TERMS_PER_LANE, WINDOW = 64, 4, 64  # kGsChunkRows, kGsTermsPerLane, kGsColorWindow (GS_SIZE_RULES holds them to the source)

# (rule, file, regex that must match the source, GPU tests of tests/test_gpu_gs.py that cross it at test size, what it selects)
GS_SIZE_RULES = [
    ("kGsColorWindow", CSRC + "gs.hpp", r"constexpr int kGsColorWindow = 64;",
     [COLOR, "test_color_cap_too_small"], "colours per window of the free-colour search (k130: 130 colours, the window is left twice; band50: 67, once; the meshes stay "
                                          "in the first)"),
    ("the next window", CSRC + "k_gs.hip", r"while \(used == ~0ull\) \{",
     [COLOR], "a row whose neighbours hold all 64 colours of a window scans its row again for the next (k130: rows of rank 64 and 128 and beyond)"),
    ("kGsRoundsPerRead", CSRC + "gs.hpp", r"constexpr int kGsRoundsPerRead = 8;",
     [COLOR], "rounds between two reads: star ends inside the first group (2 rounds), grid27 needs 5 groups (34), k130 17 (130)"),
    ("no progress", CSRC + "gs.cpp", r"if \(now >= remaining\)",
     [COLOR], "the host loop ends: the count falls after every group of rounds on every case (the error branch needs a pattern the census refuses)"),
    ("kGsCounts", CSRC + "gs.hpp", r"constexpr int kGsCounts = 6;",
     [COLOR, COLOR_CONTRACT], "six groups of per-wavefront counts: the census' five errors and the rows without a diagonal"),
    ("kGsChunkRows", CSRC + "gs.hpp", r"constexpr int kGsChunkRows = 64;",
     [SWEEP], "rows per chunk of a sweep launch: colours of fewer than 64 rows (k130: 1, star: 1 and 299), of several chunks with a short last "
              "one (path: 667 = 10 x 64 + 27)"),
    ("kGsTile", CSRC + "gs.hpp", r"constexpr int kGsTile = kGsChunkRows;",
     [SWEEP, STRIDE], "rows per workgroup: one chunk, its passes dealt out to the four wavefronts (G = 1: three leave at once; G = 64: 16 passes "
                      "each; path: colours of 11 workgroups; the stride test's largest colours: 400 and more)"),
    ("the passes of a chunk", CSRC + ROW_SWEEP, r"for \(int done = wave \* per_pass; done < rows_here; done \+= \(kThreads / kWave\) \* per_pass\) \{",
     [SWEEP], "a chunk of fewer rows than passes x rows per pass leaves wavefronts without a pass (k130, star's hub: chunks of one row)"),
    ("kGsTermsPerLane", CSRC + "gs.hpp", r"constexpr int kGsTermsPerLane = 4;",
     [SWEEP], "the lane group: G = 1 (path, star's leaves), 2 (grid7), 4 (fem), 8 (grid27), 16 (band25), 32 (band50), 64 (k130, star's hub)"),
    ("the lane group's rule", CSRC + ROW_SWEEP, r"while \(g < kWave && static_cast<u64>\(g\) \* kGsTermsPerLane \* rows_here < terms\) \{",
     [SWEEP], "the smallest G with G * 4 * rows of the chunk >= the chunk's terms, at most 64 (star's hub: 300 terms in a chunk of one row)"),
    ("kGsMaxRows", CSRC + "gs.hpp", r"constexpr int kGsMaxRows = 1 << 29;",
     [SWEEP_CONTRACT], "more rows than 32-bit gather offsets reach: SPMV_ACC_ERR_TOO_LARGE on the host"),
    ("kEntryAlign", CSRC + HELPERS, r"constexpr size_t kEntryAlign = 256;",
     [COLOR], "workspace parts are padded to 256 B (row counts that are no multiple of 64: most cases)"),
    ("census grid", CSRC + SHARED, r"return grid > static_cast<unsigned>\(kCooCheckBlocks\) \? static_cast<unsigned>\(kCooCheckBlocks\) : grid;",
     [STRIDE, COLOR_CONTRACT], "one count slot per wavefront of at most 1 024 workgroups"),
    ("census grid: the colouring's calls", CSRC + "k_gs.hip", r"dim3\(census_grid_for\(m, kThreads\)\)",
     [STRIDE, COLOR], "the census and every round take the shared census grid, one row per lane"),
    ("row loops of the census and the rounds", CSRC + "k_gs.hip", r"r < m; r \+= stride\) \{",
     [STRIDE], "one row per lane, striding (the stride test: 64 000 rows over 64 workgroups); the census: r <= m"),
    ("tile loop of the sweep", CSRC + ROW_SWEEP,
     r"for \(long long tile = blockIdx\.x; tile < ntiles; tile \+= gridDim\.x\) \{ // \(block-uniform\)\n    const long long base = first \+ tile \* kGsTile",
     [STRIDE], "blocks stride over the tiles of a colour beyond the grid"),
    ("kMaxGridBlocks (grid striding)", CSRC + SHARED, r"const long long cap = max_grid_blocks\(\);",
     [STRIDE], "every kernel of the two entries strides over the work beyond max_grid_blocks() workgroups"),
    ("kMaxGridBlocks (grid striding): the sweep's call", CSRC + "k_gs.hip", r"dim3\(grid_for\(static_cast<long long>\(last\) - first, kGsTile\)\)",
     [STRIDE], "the launchers take the shared grid"),
    ("colour pointer pass", CSRC + "k_gs.hip", r"c < count; c \+= stride\)",
     [COLOR, "test_color_cap_too_small"], "one colour per lane: min(cap_colors, m) + 1 entries (the wrapper's 1 024 exceed m on k130 and star)"),
    ("more colours than the caller's array", CSRC + "gs.cpp", r"if \(ncolors > cap_colors\)",
     ["test_color_cap_too_small"], "SPMV_ACC_ERR_TOO_LARGE with the count; the wrapper calls again"),
    ("a row without a diagonal", CSRC + "k_gs.hip", r"if \(!has_diag\) return;",
     [SWEEP, SWEEP_CONTRACT], "left untouched (the cases with diagonals removed); a row index outside [0, m) is skipped"),
    ("omega == 1", CSRC + "k_gs.hip", r"if \(omega == 1\.0\) \{",
     [SWEEP], "x[i] = g without the relaxation's two roundings; else x + omega * (g - x)"),
    ("no rows", CSRC + "gs.cpp", r"if \(m == 0\) \{",
     [COLOR], "m == 0: no colour, nothing is read or allocated"),
    ("int32 block arithmetic", CSRC + HELPERS, r"inline bool too_large\(long long v\) \{ return v > INT_MAX - \(1 << 16\); \}",
     [COLOR_CONTRACT], "m or nnz beyond this: SPMV_ACC_ERR_TOO_LARGE, as the other entries"),
    ("the census is shared", CSRC + "gs.cpp", r"pattern_census\(st, kEntry, ",
     [COLOR_CONTRACT, COLOR], "the refusals and their text are entry_helpers.hpp's, the same for the four entries; the count of rows without a diagonal comes back from it"),
]


def test_gs_size_rules_name_their_tests():
    gpu_tests = open(os.path.join(ROOT, "tests", "test_gpu_gs.py")).read()
    defined = set(re.findall(r"^def (test_\w+)\(", gpu_tests, flags=re.M))
    for name, path, pattern, tests, what in GS_SIZE_RULES:
        assert re.search(pattern, open(os.path.join(ROOT, path)).read()), f"{name}: no longer matches {path}: {pattern}"
        assert tests and what
        for t in tests:
            assert t in defined, f"{name}: names {t}, which is not a test of tests/test_gpu_gs.py"
    # every named constant of the new files is registered above (tests/size_thresholds.py does not scan them)
    registered = " ".join(r[0] + " " + r[2] for r in GS_SIZE_RULES)
    found = 0
    for f in NEW_SOURCES:
        for k in re.findall(r"constexpr\s+[\w:<> ]+?\s+(k[A-Z]\w*)\s*=", open(os.path.join(ROOT, CSRC, f)).read()):
            found += 1
            assert k in registered, f"{f}: constant {k} is not in GS_SIZE_RULES"
    assert found == 7
    # ... and so is the one constant of the shared host helpers, whose census lives with the colouring
    shared = re.findall(r"constexpr\s+[\w:<> ]+?\s+(k[A-Z]\w*)\s*=", open(os.path.join(ROOT, CSRC, HELPERS)).read())
    assert shared == ["kEntryAlign"] and shared[0] in registered
    header = open(os.path.join(ROOT, CSRC, "gs.hpp")).read()
    assert f"constexpr int kGsChunkRows = {CHUNK_ROWS};" in header and f"constexpr int kGsTermsPerLane = {TERMS_PER_LANE};" in header
    assert f"constexpr int kGsColorWindow = {WINDOW};" in header
    # every loop over work is one of the registered forms: the one tile loop stands in the shared body, which the sweep calls once
    kernels, body = open(os.path.join(ROOT, CSRC, "k_gs.hip")).read(), open(os.path.join(ROOT, CSRC, ROW_SWEEP)).read()
    assert body.count("tile += gridDim.x") == 1 and kernels.count("tile += gridDim.x") == 0 and kernels.count("+= stride)") == 4
    assert "+= stride)" not in body and kernels.count("lane_group_rows(") == 1
    assert kernels.count("lane_group_rows(m, nnz, rowptr, colindex, value, first, last, rows);") == 1


PROTOTYPES = (
    r"int spmv_acc_csr_color\(int m, int nnz, const int \*d_rowptr, const int \*d_colindex,\s*"
    r"int \*d_color, int \*d_color_rows, int cap_colors, int \*h_color_ptr,\s*int \*h_ncolors, int \*h_no_diag\);",
    r"int spmv_acc_csr_gs_sweep\(int m, int nnz, const int \*d_rowptr, const int \*d_colindex, const double \*d_value,\s*"
    r"int ncolors, const int \*h_color_ptr, const int \*d_color_rows,\s*double omega, int direction, const double \*d_b, double \*d_x\);",
)


def test_gs_entries_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "spmv_acc.h")).read()
    for proto in PROTOTYPES:
        assert re.search(proto, header), proto
    for entry in ("1", "2"):
        block = re.search(r"/\* ---- multicolour Gauss-Seidel / SOR, " + entry + r".*?\*/", header, flags=re.S)
        assert block and "replaces: nothing in the reference" in block.group(0) and "COST" in block.group(0) and "CHECKS" in block.group(0), entry
    assert "A + A^T" in header and "CANNOT CHECK" in header
    # the header declares exactly what the package lists
    declared = set(re.findall(r"\b(sparse_spmv|spmv_acc_[a-z_0-9]+)\s*\(", header))
    assert declared == set(spmv_acc_amd.C_ABI_SYMBOLS), declared ^ set(spmv_acc_amd.C_ABI_SYMBOLS)
    lib = spmv_acc_amd.load_library()
    for s in ("spmv_acc_csr_color", "spmv_acc_csr_gs_sweep"):
        assert s in spmv_acc_amd.C_ABI_SYMBOLS and hasattr(lib, s), s
    assert lib.spmv_acc_csr_color.restype is ctypes.c_int and lib.spmv_acc_csr_gs_sweep.restype is ctypes.c_int
    assert len(lib.spmv_acc_csr_color.argtypes) == 10 and len(lib.spmv_acc_csr_gs_sweep.argtypes) == 12
    assert lib.spmv_acc_csr_gs_sweep.argtypes[8] is ctypes.c_double
    for f in ("csr_color", "csr_gs_sweep"):
        assert callable(getattr(spmv_acc_amd, f))
    assert "csr_permute(" in spmv_acc_amd.csr_color.__doc__ and "color_rows=None" in spmv_acc_amd.csr_color.__doc__
    for f in ("k_gs.hip", "gs.cpp"):  # both builds compile the new files
        assert f in open(os.path.join(ROOT, CSRC, "Makefile")).read() and f in open(os.path.join(ROOT, "CMakeLists.txt")).read(), f
    assert "gs.hpp" in open(os.path.join(ROOT, CSRC, "Makefile")).read()
    assert " k_gs;" in open(os.path.join(ROOT, "tools", "resource_usage.sh")).read()


BAD, TOO_LARGE = 2, 4  # SPMV_ACC_ERR_BAD_ARGUMENT, SPMV_ACC_ERR_TOO_LARGE


def test_bad_arguments_are_refused_without_a_gpu():
    """The C entries check their arguments before they touch the device: the error codes come back on a machine without one."""
    lib = spmv_acc_amd.load_library()
    one = 8  # (never dereferenced: a non-null pointer value)
    h_ptr = (ctypes.c_int * 5)(*([-5] * 5))
    h_n, h_d = ctypes.c_int(-5), ctypes.c_int(-5)

    def color(m=4, nnz=8, rp=one, ci=one, col=one, rows=one, cap=4, hp=h_ptr, hn=ctypes.byref(h_n), hd=ctypes.byref(h_d)):
        return lib.spmv_acc_csr_color(m, nnz, rp, ci, col, rows, cap, hp, hn, hd)

    for neg in ("m", "nnz"):
        assert color(**{neg: -1}) == BAD, neg
        assert b"spmv_acc_csr_color: negative" in lib.spmv_acc_last_error_string()
    for cap in (0, -3):
        assert color(cap=cap) == BAD and b"cap_colors" in lib.spmv_acc_last_error_string()
    for null in ("rp", "ci", "col", "rows", "hp", "hn", "hd"):
        assert color(**{null: None}) == BAD, null
        assert b"spmv_acc_csr_color: null" in lib.spmv_acc_last_error_string(), null
    for big in (2 ** 31 - 1, 2 ** 31 - 2 ** 16):
        for which in ("m", "nnz"):
            assert color(**{which: big}) == TOO_LARGE, which
            assert b"spmv_acc_csr_color:" in lib.spmv_acc_last_error_string()
    assert color(m=0, nnz=3) == BAD and b"without rows" in lib.spmv_acc_last_error_string()
    assert h_n.value == -5 and h_d.value == -5 and list(h_ptr) == [-5] * 5
    assert color(m=0, nnz=0, rp=None, ci=None, col=None, rows=None) == 0  # no rows: no colour, the device is not touched
    assert h_n.value == 0 and h_d.value == 0 and h_ptr[0] == 0 and list(h_ptr)[1:] == [-5] * 4 and lib.spmv_acc_last_error() == 0

    good_ptr = (ctypes.c_int * 4)(0, 2, 3, 4)
    b_at, x_at = 1 << 20, 2 << 20

    def sweep(m=4, nnz=8, rp=one, ci=one, v=one, nc=3, hp=good_ptr, rows=one, omega=1.0, direction=2, b=b_at, x=x_at):
        return lib.spmv_acc_csr_gs_sweep(m, nnz, rp, ci, v, nc, hp, rows, omega, direction, b, x)

    for neg in ("m", "nnz", "nc"):
        assert sweep(**{neg: -1}) == BAD, neg
        assert b"spmv_acc_csr_gs_sweep: negative" in lib.spmv_acc_last_error_string()
    for direction in (-1, 3, 7):
        assert sweep(direction=direction) == BAD and b"direction" in lib.spmv_acc_last_error_string()
    for null in ("rp", "ci", "v", "hp", "b", "x"):
        assert sweep(**{null: None}) == BAD, null
        assert b"spmv_acc_csr_gs_sweep: null" in lib.spmv_acc_last_error_string(), null
    for ptr in ((1, 2, 3, 4), (0, 2, 3, 5), (0, 2, 3, 3), (0, 3, 2, 4), (0, -1, 3, 4)):
        assert sweep(hp=(ctypes.c_int * 4)(*ptr)) == BAD, ptr
        assert b"h_color_ptr" in lib.spmv_acc_last_error_string()
    assert sweep(nc=2) == BAD and sweep(nc=0, hp=(ctypes.c_int * 1)(0)) == BAD  # does not end at m
    for b, x in ((x_at, x_at), (x_at + 8, x_at), (x_at - 24, x_at), (x_at + 24, x_at)):
        assert sweep(b=b, x=x) == BAD and b"overlaps" in lib.spmv_acc_last_error_string(), (b, x)
    for big in (2 ** 31 - 1, 2 ** 31 - 2 ** 16):
        for which in ("m", "nnz", "nc"):
            assert sweep(**{which: big}, hp=(ctypes.c_int * 1)(0)) == TOO_LARGE, which
            assert b"spmv_acc_csr_gs_sweep:" in lib.spmv_acc_last_error_string()
    assert sweep(m=2 ** 29 + 1, hp=(ctypes.c_int * 4)(0, 2, 3, 2 ** 29 + 1)) == TOO_LARGE and b"2^29" in lib.spmv_acc_last_error_string()
    # nothing to do: no rows
    assert sweep(m=0, nnz=0, rp=None, ci=None, v=None, nc=0, hp=(ctypes.c_int * 1)(0), rows=None, b=None, x=None) == 0
    assert lib.spmv_acc_last_error() == 0
    lib.spmv_acc_clear_error()


def test_wrappers_refuse_bad_arguments():
    E = spmv_acc_amd.SpmvAccError
    m, nnz = 10, 30

    def color(match, mm=m, rp=_i(m + 1), ci=_i(nnz)):
        with pytest.raises(E, match=match):
            spmv_acc_amd.csr_color(mm, rp, ci)

    color("not on the GPU", ci=_i(nnz, cuda=False))
    color("dtype", rp=_FakeTensor(m + 1, dtype="torch.int64"))
    color("dtype", ci=_f(nnz))
    color("not contiguous", ci=_i(nnz, contiguous=False))
    color("elements", rp=_i(m))
    color("on cuda:1", ci=_i(nnz, device="cuda:1"))
    color("torch tensor", rp=None)
    color("torch tensor", ci=[0] * nnz)
    color("negative", mm=-1)

    good = dict(rp=_i(m + 1), ci=_i(nnz), v=_f(nnz), ptr=[0, 4, 7, 10], rows=_i(m), b=_f(m), x=_f(m))

    def sweep(match, mm=m, omega=1.0, direction="symmetric", sweeps=1, **bad):
        a = dict(good, **bad)
        with pytest.raises(E, match=match):
            spmv_acc_amd.csr_gs_sweep(mm, a["rp"], a["ci"], a["v"], a["ptr"], a["rows"], a["b"], a["x"], omega=omega, direction=direction, sweeps=sweeps)

    sweep("not on the GPU", v=_f(nnz, cuda=False))
    sweep("not on the GPU", rows=_i(m, cuda=False))
    sweep("dtype", rp=_FakeTensor(m + 1, dtype="torch.int64"))
    sweep("dtype", v=_i(nnz))
    sweep("dtype", b=_i(m))
    sweep("dtype", rows=_f(m))
    sweep("not contiguous", x=_f(m, contiguous=False))
    sweep("elements", rp=_i(m))
    sweep("elements", v=_f(nnz - 1))
    sweep("elements", b=_f(m - 1))
    sweep("elements", x=_f(m - 1))
    sweep("as many", v=_f(nnz + 1))
    sweep("as many", rows=_i(m - 1))
    sweep("as many", rows=_i(m + 1))
    sweep("on cuda:1", x=_f(m, device="cuda:1"))
    sweep("torch tensor", v=None)
    sweep("torch tensor", b=[0.0] * m)
    sweep("torch tensor", x=3.0)
    sweep("torch tensor", rows=list(range(m)))
    sweep("negative", mm=-1)
    sweep("negative", sweeps=-1)
    sweep("direction", direction="sideways")
    sweep("direction", direction=2)
    sweep("color_ptr", ptr=None)
    sweep("color_ptr", ptr=[])
    sweep("color_ptr", ptr=[1, 4, 10])
    sweep("color_ptr", ptr=[0, 4, 9])
    sweep("color_ptr", ptr=[0, 7, 4, 10])


def test_gs_entries_keep_no_state():
    """As test_extract_entries_keep_no_state: the engine file neither finds nor makes a plan, counts no plan work, reads no tunable and keeps
    nothing static; the colouring's one allocation is freed on every way out; the sweep is launch-only."""
    src = open(os.path.join(ROOT, CSRC, "gs.cpp")).read()
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
    for launch in ("pattern_census", "launch_gs_round", "launch_gs_keys", "launch_coo_sort", "launch_gs_color_ptr"):
        assert launch in after, launch
    bare = [ln.strip() for ln in after.splitlines() if re.search(r"\breturn\b(?! leave\()", ln)]
    # (the one way out that may skip leave(): the scratch query before the allocation)
    assert bare == ['return entry_error(kEntry, kErrHip, "radix sort workspace query failed");'], bare
    # the host loop can end: one comparison guards every further group of rounds
    loop = after.split("while (remaining != 0) {")[1].split("\n  }\n")[0]
    assert "if (now >= remaining)" in loop and "return leave(entry_error(kEntry, kErrHip" in loop and "remaining = now;" in loop
    assert after.index("pattern_census(") < after.index("uncolour the rows") < after.index("launch_gs_round(")  # the census is judged before anything is written
    assert 'pattern_census(st, kEntry, m, nnz, d_rowptr, d_colindex, d_slots, "colour the pattern of A + A^T instead", ' in after
    sweep = code.split("int run_csr_gs_sweep")[1]
    assert "hipMalloc" not in sweep and "Synchronize" not in sweep and "hipMemcpy" not in sweep and "hipMemset" not in sweep  # launch-only: capturable
    assert "plan_work_allowed" not in sweep and sweep.count("launch_gs_color(") == 1 and "launch_gs_" not in sweep.replace("launch_gs_color(", "")


def test_entry_helpers_keep_no_state():
    """What the entry files share on the host keeps nothing either: plain inline functions, no static, no device allocation; the census of
    gs.cpp, agg.cpp, strength.cpp and dense.cpp is one memset, one launch, one copy and one synchronise, in that order, and its refusal text
    stands here alone; and no entry file, structural, AMG or solver, keeps a copy of a helper or of the check after its launches."""
    code = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, CSRC, HELPERS)).read())
    for word in ("get_plan", "g_plans", "t_plan_work", "t_last_plan", "tune_", "TimingPhase", "TuneTimer", "static std::", "thread_local", "g_tunables"):
        assert word not in code, word
    assert not re.search(r"\bstatic\b", code) and "hipMalloc" not in code and "hipFree" not in code
    functions = re.findall(r"^(\w[\w ]*?)\b(\w+)\(", code, flags=re.M)
    assert [name for _, name in functions] == ["entry_error", "launch_error", "aligned_up", "too_large", "overlap", "slot_sum", "pattern_census"], functions
    assert all(kind.startswith("inline ") for kind, _ in functions), functions
    census = code.split("inline int pattern_census(hipStream_t st, const char *entry, ")[1].split("\n}\n")[0]
    calls = ("hipMemsetAsync(", "launch_gs_census(", "hipMemcpyAsync(", "hipStreamSynchronize(")
    assert all(census.count(c) == 1 for c in calls) and [census.index(c) for c in calls] == sorted(census.index(c) for c in calls)
    assert re.findall(r"\blaunch_\w+\(", census) == ["launch_gs_census("]
    assert [census.index(t) for t in ('"zero the census"', '"read the census"', '"census"')] == sorted(census.index(t) for t in ('"zero the census"', '"read the census"', '"census"'))
    assert census.count("nothing was written") == 1 and census.count("ends of rowptr that are not 0 and nnz") == 1
    # the mirrors are judged and reported under the advice's null check alone
    assert census.count("bad[4]") == 2 and census.count("without their mirror") == 1
    assert "(mirror_advice ? bad[4] : 0)" in census
    clause = next(ln for ln in census.splitlines() if "without their mirror" in ln)
    assert clause.strip().startswith("if (mirror_advice) what += ") and "bad[4]" in clause and '" + mirror_advice + ")"' in clause
    assert census.index("without their mirror") < census.index("nothing was written")
    assert census.count("if (no_diag) *no_diag = bad[5];") == 1 and census.count("bad[5]") == 1
    # the copies are gone from the four entry files, and the refusal's text with them
    for f in ENTRY_FILES:
        entry = open(os.path.join(ROOT, CSRC, f)).read()
        assert '#include "' + HELPERS + '"' in entry, f
        for gone in ("launch_gs_census(", "bad[kGsCounts]", "ends of rowptr", "nothing was written", "kCooCheckSlots; ++s"):
            assert gone not in entry, (f, gone)
        assert not re.search(r"\b(gs|agg|strength|dense)_(error|too_large|aligned_up|overlap)\(", entry), f
        assert set(re.findall(r"\b(\w*(?:too_large|aligned_up|overlap))\(", entry)) <= {"too_large", "aligned_up", "overlap"}, f
        assert not re.search(r"constexpr size_t k\w*Align", entry), f
    # nor does a structural entry file or a solver's keep a copy: the error, the round-up, the size rule, a written-out slot sum
    for f in ENTRY_FILES + SOLVER_FILES + STRUCTURAL_FILES:
        entry = open(os.path.join(ROOT, CSRC, f)).read()
        assert '#include "' + HELPERS + '"' in entry, f
        assert not re.search(r"\b(coo|trans|spgemm|csr_add|extract|spmm|cg|jacobi)_(error|too_large|aligned_up)\(", entry), f
        assert not re.search(r"constexpr size_t k\w*Align", entry) and "INT_MAX - (1 << 16)" not in entry, f
        for gone in ("kCooCheckSlots; ++s", "for (unsigned c : slots)", "set_error(code, std::string(entry)"):
            assert gone not in entry, (f, gone)
        if f not in SOLVER_FILES:  # (cg.cpp's first_overlap is a table walk on overlap())
            assert set(re.findall(r"\b(\w*(?:too_large|aligned_up|overlap))\(", entry)) <= {"too_large", "aligned_up", "overlap"}, f
        # the check after an entry's launches stands in the header alone; spmm.cpp's keeps a pending error and is its own
        if f != "spmm.cpp":
            assert "kernel launch failed" not in entry and not re.search(r"\blaunch_err\b", entry) and "hipGetErrorString" not in entry, f
            assert "launch_error(kEntry)" in entry, f
    assert code.count('"kernel launch failed: "') == 1 and code.count("hipGetErrorString(") == 1 and not re.search(r"\blaunch_err\b", code)
    launch_check = code.split("inline int launch_error(const char *entry) {")[1].split("\n}\n")[0]
    assert launch_check.count("hipGetLastError()") == 1 and code.count("hipGetLastError()") == 1
    assert "return kOk;" in launch_check and "entry_error(entry, kErrHip, " in launch_check
    assert HELPERS in open(os.path.join(ROOT, CSRC, "Makefile")).read()


ROW_SWEEP_FUNCTIONS = ["row_term_load", "row_gather", "row_term", "lane_group_rows"]


def test_row_sweep_keeps_no_state():
    """What gs_color_kernel, jacobi_sweep_kernel and jacobi_l1_kernel share on the device is a fixed list of forced-inline functions: no atomic,
    no LDS, no barrier and no constant of its own (the tile constants stay in gs.hpp); and the copies are gone from the two kernel files."""
    src = open(os.path.join(ROOT, CSRC, ROW_SWEEP)).read()
    code = re.sub(r"//[^\n]*", "", src)
    for word in ("atomic", "__shared__", "__syncthreads", "constexpr", "__global__"):
        assert word not in code, word
    assert not re.search(r"\bstatic\b", code)
    functions = re.findall(r"^(\w[\w ]*?)\b(\w+)\(", code, flags=re.M)
    assert [name for _, name in functions] == ROW_SWEEP_FUNCTIONS, functions
    assert all(kind.startswith("__device__ __forceinline__ ") for kind, _ in functions), functions
    assert code.count("struct ") == 1 and "struct RowTerm {" in code  # the term record, defined once
    assert '#include "gs.hpp"' in src and '#include "structure_passes.hpp"' in src and "namespace passes {" in src
    for f in ("k_gs.hip", "k_jacobi.hip"):
        kernels = open(os.path.join(ROOT, CSRC, f)).read()
        assert '#include "' + ROW_SWEEP + '"' in kernels, f
        for gone in ("GsTerm", "JacobiTerm", "gs_load", "jacobi_load", "gs_gather", "jacobi_gather", "gs_term(", "jacobi_term(", "jacobi_rows", "bool opened",
                     "readfirstlane"):
            assert gone not in kernels, (f, gone)
    assert ROW_SWEEP in open(os.path.join(ROOT, CSRC, "Makefile")).read()
    # structure_passes.hpp does not take the body in: it is built on coo.hpp and held to its own function list
    assert "lane_group_rows" not in open(os.path.join(ROOT, CSRC, "structure_passes.hpp")).read()


KERNELS = ("gs_census_kernel", "gs_round_kernel", "gs_keys_kernel", "gs_color_ptr_kernel", "gs_color_kernel")
# as recorded in k_gs.hip's header comment
RECORDED_VGPRS = dict(gs_census_kernel=26, gs_round_kernel=20, gs_keys_kernel=8, gs_color_ptr_kernel=9, gs_color_kernel=47)


def test_gs_kernels_fit_their_register_budget(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_table

    asm = tmp_path / "k_gs.s"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-DKERNEL_STRATEGY_ADAPTIVE",
                        "-I" + os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-S",
                        os.path.join(ROOT, CSRC, "k_gs.hip"), "-o", str(asm)], capture_output=True, text=True, timeout=900)
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
    sweep_body = next(b for k, b in bodies.items() if "gs_color_kernel" in k)
    # contraction is off: products and sums are instructions of their own; the only fused operations are the division's own expansion
    assert "v_mul_f64" in sweep_body and "v_add_f64" in sweep_body and sweep_body.count("v_div_fixup_f64") == 1
    division = sweep_body[sweep_body.index("v_div_scale_f64"):sweep_body.index("v_div_fixup_f64")]
    outside = sweep_body.replace(division, "")
    assert "v_fma_f64" not in outside and "v_fmac_f64" not in outside and "v_fma" in division
    header = open(os.path.join(ROOT, CSRC, "k_gs.hip")).read().split("#include")[0]
    rows = [k for k in resource_table.parse(r.stderr) if "rocprim" not in k["name"]]
    assert sorted(k["name"] for k in rows) == sorted(KERNELS), sorted(k["name"] for k in rows)
    for k in rows:
        assert k["scratch"] == 0 and k["agprs"] == 0 and k["vgprs"] <= 64 and k["occupancy"] >= 8, k
        want = RECORDED_VGPRS[k["name"]]
        assert re.search(k["name"] + r", " + str(want) + r"\b", header), (k["name"], "the count recorded in the header comment")
        assert k["vgprs"] <= want + 4, (k, "grew past the count recorded in k_gs.hip (a few registers of compiler drift are allowed)")


# ---- the colouring (gs.hpp), in numpy: the GPU suite's reference -------------------------------------------------------------------------------
def mix32(v):
    x = np.asarray(v, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    return x


def priorities(m):
    v = np.arange(m, dtype=np.uint64)
    return (mix32(v) << np.uint64(32)) | v


def color_outputs(m, rp, ci, color):
    """(color, color_rows, color_ptr, no_diag) as the entry returns them, from the colours."""
    color = np.asarray(color, dtype=np.int32)
    ncolors = int(color.max()) + 1 if m else 0
    color_rows = np.argsort(color, kind="stable").astype(np.int32)
    color_ptr = np.concatenate([[0], np.cumsum(np.bincount(color, minlength=ncolors))]).astype(np.int64).tolist() if m else [0]
    row = np.repeat(np.arange(m), np.diff(rp))
    no_diag = m - int(np.unique(row[ci == row]).size)
    return color, color_rows, color_ptr, no_diag


def host_csr_color(m, rp, ci):
    """The definition: the rows in descending priority, each the smallest colour no already-coloured off-diagonal neighbour holds."""
    color = np.full(m, -1, dtype=np.int64)
    for v in np.argsort(priorities(m))[::-1]:
        nb = ci[rp[v]:rp[v + 1]]
        held = set(color[nb[nb != v]].tolist())
        c = 0
        while c in held:
            c += 1
        color[v] = c
    return color_outputs(m, rp, ci, color)


def host_csr_color_rounds(m, rp, ci):
    """The round form (Jones-Plassmann): (colours, rounds).  A round reads the colours of the round before; an uncoloured row with an uncoloured
    neighbour of higher priority waits, any other takes the smallest colour none of its neighbours holds."""
    prio = priorities(m)
    color = np.full(m, -1, dtype=np.int64)
    rounds = 0
    while (color < 0).any():
        before = color.copy()
        for v in np.flatnonzero(before < 0):
            nb = ci[rp[v]:rp[v + 1]]
            nb = nb[nb != v]
            if np.any((before[nb] < 0) & (prio[nb] > prio[v])):
                continue
            held = set(before[nb].tolist())
            c = 0
            while c in held:
                c += 1
            color[v] = c
        rounds += 1
        assert (color < 0).sum() < (before < 0).sum()
    return color.astype(np.int32), rounds


# ---- the sweep (gs.hpp), in numpy, bit for bit: the GPU suite's reference --------------------------------------------------------------------------
def lane_group(total_terms, rows_here):
    g = 1
    while g < 64 and g * TERMS_PER_LANE * rows_here < total_terms:
        g *= 2
    return g


def row_sum(terms, g):
    """The documented order: lane l adds the terms l, l + g, ... starting from its first (none: +0.0), then a balanced tree over neighbours."""
    steps = -(-terms.size // g) if terms.size else 0
    padded = np.zeros(max(steps, 1) * g)
    padded[:terms.size] = terms
    live = np.arange(max(steps, 1) * g) < terms.size
    padded, live = padded.reshape(-1, g), live.reshape(-1, g)
    part = padded[0].copy()
    for k in range(1, steps):
        part = np.where(live[k], part + padded[k], part)
    while part.size > 1:
        part = part[0::2] + part[1::2]
    return part[0]


def host_gs_sweep(m, rp, ci, val, color_ptr, color_rows, b, x, omega=1.0, direction="symmetric"):
    """One sweep of x (a copy is returned).  color_rows None: colour c is the row range itself.  Rows outside [0, m) are skipped, extents are
    clamped, a column outside [0, m) gives the term +0.0, a row without a diagonal is left as it is."""
    x = np.array(x, dtype=np.float64)
    nnz = ci.size
    ncolors = len(color_ptr) - 1
    order = {"forward": list(range(ncolors)), "backward": list(range(ncolors - 1, -1, -1))}
    order["symmetric"] = order["forward"] + order["backward"]
    omega = np.float64(omega)
    with np.errstate(all="ignore"):
        for c in order[direction]:
            for base in range(color_ptr[c], color_ptr[c + 1], CHUNK_ROWS):
                pos = np.arange(base, min(base + CHUNK_ROWS, color_ptr[c + 1]))
                rows = pos if color_rows is None else np.asarray(color_rows)[pos].astype(np.int64)
                extents = []
                for i in rows:
                    if 0 <= i < m:
                        lo = min(max(int(rp[i]), 0), nnz)
                        extents.append((lo, min(max(int(rp[i + 1]), lo), nnz)))
                    else:
                        extents.append((0, 0))
                g = lane_group(sum(hi - lo for lo, hi in extents), pos.size)
                for i, (lo, hi) in zip(rows, extents):
                    if not 0 <= i < m:
                        continue
                    cols, v = ci[lo:hi].astype(np.int64), val[lo:hi]
                    inside = (cols >= 0) & (cols < m)
                    terms = v * x[np.where(inside, cols, 0)]  # every product rounded on its own
                    terms[~inside | (cols == i)] = 0.0
                    on_diag = np.flatnonzero(cols == i)
                    if on_diag.size == 0:
                        continue
                    s = row_sum(terms, g)
                    gs = (np.float64(b[i]) - s) / v[on_diag[0]]
                    x[i] = gs if omega == 1.0 else x[i] + omega * (gs - x[i])
    return x


# ---- the cases of the GPU suite, made once ----------------------------------------------------------------------------------------------------
def csr_from_pattern(m, pairs, rng, dominant=False):
    """A CSR with strictly ascending rows from a set of (i, j); dominant: symmetric values with a diagonal above its row's absolute sum (SPD)."""
    i, j = np.array(sorted(set(pairs)), dtype=np.int64).reshape(-1, 2).T
    rp = np.zeros(m + 1, dtype=np.int32)
    np.cumsum(np.bincount(i, minlength=m), out=rp[1:])
    if dominant:
        lo, hi = np.minimum(i, j), np.maximum(i, j)
        v = -(1.0 + ((lo * 7919 + hi * 104729) % 1000) / 1000.0)  # a function of the unordered pair: symmetric
        off = np.bincount(i[i != j], weights=-v[i != j], minlength=m)
        v = np.where(i == j, off[i] + 1.0, v)
    else:
        v = rng.uniform(0.5, 2.0, i.size) * rng.choice([-1.0, 1.0], i.size)
    return rp, j.astype(np.int32), v.astype(np.float64)


def stencil_pairs(nx, ny, nz, full):
    """The 7-point (full False) or 27-point stencil on an nx x ny x nz grid, row (a * ny + b) * nz + c, with the diagonal."""
    pairs = []
    idx = np.arange(nx * ny * nz).reshape(nx, ny, nz)
    for a in range(nx):
        for b in range(ny):
            for c in range(nz):
                for da in (-1, 0, 1):
                    for db in (-1, 0, 1):
                        for dc in (-1, 0, 1):
                            if not full and abs(da) + abs(db) + abs(dc) > 1:
                                continue
                            p, q, r = a + da, b + db, c + dc
                            if 0 <= p < nx and 0 <= q < ny and 0 <= r < nz:
                                pairs.append((int(idx[a, b, c]), int(idx[p, q, r])))
    return pairs


def without_diagonals(A, which):
    """The same matrix with the diagonal entries of the rows `which` removed."""
    rp, ci, v = A
    row = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    keep = ~((ci == row) & np.isin(row, which))
    new_rp = np.zeros_like(rp)
    np.cumsum(np.bincount(row[keep], minlength=rp.size - 1), out=new_rp[1:])
    return new_rp, ci[keep], v[keep]


# (tag, rows, colours, rounds): from a CPU run of the two host models (test_the_cases_and_their_colourings holds the cases to it)
TABLE = (("fem", 450, 7, 16), ("grid7", 504, 5, 12), ("grid27", 504, 15, 34), ("path", 2000, 3, 6), ("star", 300, 2, 2), ("k130", 130, 130, 130))
FURTHER = ("band25", "band50", "fem_holes", "grid7_holes", "lonely", "empties", "one", "one_empty", "none")
TAGS = tuple(t[0] for t in TABLE) + FURTHER


def _cases():
    rng = np.random.default_rng(2029)
    row, col, val = synth.fem_quads_coo(24, 17, seed=5)
    rp, ci, order, start = host_assemble(450, 450, row, col)
    fem = (rp, ci, rng.uniform(0.5, 2.0, ci.size) * rng.choice([-1.0, 1.0], ci.size))
    yield "fem", 450, fem
    g7 = csr_from_pattern(504, stencil_pairs(9, 8, 7, False), rng, dominant=True)
    yield "grid7", 504, g7
    yield "grid27", 504, csr_from_pattern(504, stencil_pairs(9, 8, 7, True), rng)
    yield "path", 2000, csr_from_pattern(2000, [(i, j) for i in range(2000) for j in (i - 1, i, i + 1) if 0 <= j < 2000], rng)
    star = [(i, i) for i in range(300)] + [(0, j) for j in range(1, 300)] + [(j, 0) for j in range(1, 300)]
    yield "star", 300, csr_from_pattern(300, star, rng)
    yield "k130", 130, csr_from_pattern(130, [(i, j) for i in range(130) for j in range(130)], rng)
    for tag, half in (("band25", 25), ("band50", 50)):
        yield tag, 200, csr_from_pattern(200, [(i, j) for i in range(200) for j in range(i - half, i + half + 1) if 0 <= j < 200], rng)
    yield "fem_holes", 450, without_diagonals(fem, rng.permutation(450)[:40])
    yield "grid7_holes", 504, without_diagonals(g7, np.arange(0, 504, 5))
    lonely = [(i, i) for i in range(150)] + [(i, j) for i in range(0, 150, 3) for j in (i - 3, i + 3) if 0 <= j < 150]
    yield "lonely", 150, csr_from_pattern(150, lonely, rng)  # two rows of three hold only their diagonal
    holes = [(i, j) for i in range(100) for j in (i - 4, i, i + 4) if 0 <= j < 100 and i % 4 < 2 and j % 4 < 2]
    yield "empties", 100, csr_from_pattern(100, holes, rng)  # every other pair of rows is empty, the first and the last rows included
    yield "one", 1, (np.array([0, 1], np.int32), np.array([0], np.int32), np.array([-2.5]))
    yield "one_empty", 1, (np.array([0, 0], np.int32), np.zeros(0, np.int32), np.zeros(0))
    yield "none", 0, (np.array([0], np.int32), np.zeros(0, np.int32), np.zeros(0))


@functools.lru_cache(maxsize=None)
def cases():
    """tag -> (m, (rowptr, colindex, value)); made once and shared, nothing changes them."""
    return {tag: (m, A) for tag, m, A in _cases()}


@functools.lru_cache(maxsize=None)
def coloring(tag):
    """(color, color_rows, color_ptr, no_diag) of the host for a case, computed once."""
    m, (rp, ci, _) = cases()[tag]
    return host_csr_color(m, rp, ci)


def is_proper(m, rp, ci, color):
    row = np.repeat(np.arange(m), np.diff(rp))
    off = ci != row
    return not np.any(color[row[off]] == color[ci[off]])


def test_mix32_and_the_priorities():
    def scalar(x):  # the header's five lines, in Python integers
        x ^= x >> 16
        x = (x * 0x7FEB352D) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846CA68B) & 0xFFFFFFFF
        x ^= x >> 16
        return x

    for v in (0, 1, 2, 63, 64, 1000, 2 ** 31 - 1, 2 ** 32 - 1):
        assert int(mix32(v)) == scalar(v), v
    assert scalar(0) == 0 and scalar(1) != 1
    p = priorities(5000)
    assert np.unique(p).size == 5000 and np.array_equal(p & np.uint64(0xFFFFFFFF), np.arange(5000, dtype=np.uint64))
    header = open(os.path.join(ROOT, CSRC, "gs.hpp")).read()
    for line in ("x ^= x >> 16;", "x *= 0x7feb352du;", "x ^= x >> 15;", "x *= 0x846ca68bu;"):
        assert line in header, line


def test_the_cases_and_their_colourings():
    """Every case is what the colouring demands (square, rebased, strictly ascending rows, symmetric pattern); the sequential model and the
    round model give the same colours; every colouring is proper; rows, colours and rounds are the table's."""
    assert set(TAGS) == set(cases())
    counted = {}
    for tag in TAGS:
        m, (rp, ci, v) = cases()[tag]
        assert rp.size == m + 1 and rp[0] == 0 and rp[m] == ci.size == v.size and np.all(np.diff(rp) >= 0), tag
        row = np.repeat(np.arange(m), np.diff(rp))
        inner = np.ones(ci.size, dtype=bool)
        inner[rp[:-1][np.diff(rp) > 0]] = False
        assert ci.size < 2 or np.all(np.diff(ci.astype(np.int64))[inner[1:]] > 0), tag
        pattern = set(zip(row.tolist(), ci.tolist()))
        assert all((j, i) in pattern for i, j in pattern), tag
        color, color_rows, color_ptr, no_diag = coloring(tag)
        by_rounds, rounds = host_csr_color_rounds(m, rp, ci)
        assert np.array_equal(color, by_rounds), tag
        assert is_proper(m, rp, ci, color), tag
        assert color_ptr[0] == 0 and color_ptr[-1] == m and np.all(np.diff(color_ptr) > 0 if m else True), tag  # every colour below the largest is used
        assert np.array_equal(np.sort(color_rows), np.arange(m)) and np.all(np.diff(color[color_rows]) >= 0), tag
        for c in range(len(color_ptr) - 1):
            assert np.all(np.diff(color_rows[color_ptr[c]:color_ptr[c + 1]]) > 0), (tag, c)  # ascending rows inside a colour: the sort is stable
        counted[tag] = (m, len(color_ptr) - 1, rounds, no_diag)
    for tag, rows, colours, rounds in TABLE:
        assert counted[tag][:3] == (rows, colours, rounds), (tag, counted[tag])
        assert counted[tag][3] == 0, tag
    m, (rp, ci, _) = cases()["star"]
    assert np.diff(rp)[0] == 300 and np.all(np.diff(rp)[1:] == 2)  # one row of 299 off-diagonal entries and its diagonal
    assert counted["fem_holes"][3] == 40 and counted["grid7_holes"][3] == 101 and counted["one_empty"][1:] == (1, 1, 1) and counted["none"] == (0, 0, 0, 0)
    assert counted["empties"][3] == 50 and np.diff(cases()["empties"][1][0])[[0, 1, 2, 3, -1]].tolist() == [2, 2, 0, 0, 0]
    assert np.sum(np.diff(cases()["lonely"][1][0]) == 1) == 100
    # the lane groups the sweep cases cross (GS_SIZE_RULES kGsTermsPerLane)
    groups = set()
    for tag in TAGS:
        m, (rp, ci, _) = cases()[tag]
        color, color_rows, color_ptr, _ = coloring(tag)
        for c in range(len(color_ptr) - 1):
            for base in range(color_ptr[c], color_ptr[c + 1], CHUNK_ROWS):
                rows = color_rows[base:min(base + CHUNK_ROWS, color_ptr[c + 1])]
                groups.add(lane_group(int(np.diff(rp)[rows].sum()), rows.size))
    assert groups == {1, 2, 4, 8, 16, 32, 64}, groups


def test_row_sum_is_the_documented_order():
    rng = np.random.default_rng(3)
    t = rng.standard_normal(300) * 10.0 ** rng.integers(-8, 8, 300)
    assert row_sum(t[:1], 1) == t[0] and row_sum(t[:0], 4) == 0.0
    s = t[0]
    for k in range(1, 300):
        s = s + t[k]
    assert row_sum(t, 1) == s  # one lane: a host loop from the first term
    for g in (2, 4, 8, 16, 32, 64):
        for n in (1, g - 1, g, g + 1, 3 * g + 2, 300):
            part = []
            for lane in range(g):
                mine = t[:n][lane::g]
                acc = mine[0] if mine.size else 0.0
                for w in mine[1:]:
                    acc = acc + w
                part.append(acc)
            while len(part) > 1:
                part = [part[2 * k] + part[2 * k + 1] for k in range(len(part) // 2)]
            assert row_sum(t[:n], g) == part[0], (g, n)
    # a first term of -0.0 is kept (the sum does not start from +0.0)
    assert np.signbit(row_sum(np.array([-0.0]), 1)) and not np.signbit(row_sum(np.array([-0.0]), 2))
    assert lane_group(0, 1) == 1 and lane_group(4 * 64, 64) == 1 and lane_group(4 * 64 + 1, 64) == 2 and lane_group(300, 1) == 64 and lane_group(10 ** 9, 64) == 64


def test_host_sweep_against_the_triangular_system():
    """Permuted by colour, one forward sweep with omega = 1 is x' = (D + L)^-1 (b - U x): dense numpy triangles in extended precision.  The
    system is checked in its row form -- row i of (D + L) x' against row i of b - U x, over a_ii --, so that every row is held to its own
    rounding bound (len + 3) 2^-53 (|b_i| + sum |a_ij| |x_j|) / |a_ii| and one row's rounding is not counted against the rows that read it."""
    rng = np.random.default_rng(11)
    for tag in ("fem", "grid7", "grid27", "path", "star", "k130", "band50"):
        m, (rp, ci, v) = cases()[tag]
        color, color_rows, color_ptr, _ = coloring(tag)
        p_rp, p_ci, _, p_v = host_csr_permute(m, (rp, ci, v), color_rows)
        b, x = rng.standard_normal(m), rng.standard_normal(m)
        new = host_gs_sweep(m, p_rp, p_ci, p_v, color_ptr, None, b, x, 1.0, "forward")
        D = np.zeros((m, m), dtype=np.longdouble)
        row = np.repeat(np.arange(m), np.diff(p_rp))
        D[row, p_ci] = p_v
        lower, upper = np.tril(D), np.triu(D, 1)
        rhs = b.astype(np.longdouble) - upper @ x.astype(np.longdouble)
        diag = np.diag(D)
        residual = np.abs(lower @ new.astype(np.longdouble) - rhs) / np.abs(diag)
        scale = (np.abs(b) + np.abs(np.tril(D, -1)) @ np.abs(new) + np.abs(upper) @ np.abs(x)) / np.abs(diag)
        bound = (np.diff(p_rp) + 3) * 2.0 ** -53 * scale
        assert np.all(residual <= bound), (tag, float(np.max(residual / bound)))
        # inside a colour no row reads another: the block of (D + L) of every colour is diagonal
        for c in range(len(color_ptr) - 1):
            blk = lower[color_ptr[c]:color_ptr[c + 1], color_ptr[c]:color_ptr[c + 1]]
            assert np.count_nonzero(blk) == np.count_nonzero(np.diag(blk)), (tag, c)
    # backward is forward on the reversed colours; symmetric is the two in turn; omega relaxes
    m, (rp, ci, v) = cases()["grid7"]
    color, color_rows, color_ptr, _ = coloring("grid7")
    b, x = rng.standard_normal(m), rng.standard_normal(m)
    f = host_gs_sweep(m, rp, ci, v, color_ptr, color_rows, b, x, 1.0, "forward")
    fb = host_gs_sweep(m, rp, ci, v, color_ptr, color_rows, b, f, 1.0, "backward")
    assert np.array_equal(fb, host_gs_sweep(m, rp, ci, v, color_ptr, color_rows, b, x, 1.0, "symmetric"))
    first = color_rows[:color_ptr[1]]
    relaxed = host_gs_sweep(m, rp, ci, v, color_ptr, color_rows, b, x, 0.5, "forward")
    assert np.array_equal(relaxed[first], x[first] + 0.5 * (f[first] - x[first]))
