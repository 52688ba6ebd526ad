"""CPU side of the conjugate-gradient vector passes and of pcg (no GPU): the C ABI declares and exports the four entries, they and the Python
wrappers refuse bad arguments before any launch, the compiled kernels use no scratch, no AGPR and no atomic and fit 64 VGPRs, every
size-selected branch of the new code names the GPU tests that cross it, the engine file stays stateless and launch-only, and the definitions
are restated here in numpy and exported to the GPU suite as its references: the dot product in its two levels of row_sum (host_cg_dot), the
three entries on a dict-shaped state block (host_cg_start, host_cg_update, host_cg_direction), bit for bit, and the solve composed of them
(host_pcg) on host_spmv and host_amg_cycle.

MEASURED with this file's model (b = rhs(m) of tests/test_amg_host.py, x0 = 0): AMG-PCG at rtol 1e-10 on the four hierarchies --
iterations, the true relative residual |b - A x| / |b| of the final x, and the cycles the stationary amg_cycle loop needs to reach that
same residual:
    grid24   12   1.9e-11   27
    grid48   14   1.9e-11   35
    aniso48  13   3.7e-11   28
    aniso24  12   3.2e-11   25
PCG_RESIDUAL_BOUND is ten times the largest of them, 3.7e-10, rounded up to a power of ten: 1e-9.  No history entry of the eight solves
(both summation orders) lies within 1e-6 relative of tol2 (the nearest, on grid48, is 0.27 tol2 away), so the device's count must equal the
host's.

The spreads the GPU suite's tolerances come from (two host restatements that differ only in the SpMVs' summation order, forward against
reversed row sums; the dot products are the same pure function in both), the largest over the named solves:
  AMG-PCG, every iteration: the iterate, relative to its largest magnitude: 4.5e-16, 8.9e-16, 1.11e-15 and 1.0e-15 on the four hierarchies
    (PCG_ITERATE_SPREAD 1.2e-15); the history, entry by entry relative: 9.7e-14, 1.8e-14, 2.7e-14 and 2.8e-14 (PCG_HISTORY_SPREAD 1e-13);
  plain and Jacobi CG on grid24, rtol 1e-8, the first 10 iterations: the iterate 3.9e-16, the history 9.8e-16 (CG_ITERATE_SPREAD 4e-16,
    CG_HISTORY_SPREAD 1e-15) -- the same figures for both, the grid's diagonal being the constant 4, whose inverse scales exactly --; the
    iteration counts to rtol 1e-8 are 77 in both orders, plain and Jacobi: a difference of 0 (CG_COUNT_SPREAD), so the GPU suite allows 1.

THE IRREGULAR CASES of tests/test_amg_host.py (b = rhs_of(tag), x0 = 0, rtol 1e-10), and "amg22": fem_weak from the seeded non-zero start
x0_of with pre = post = 2.  MEASURED with this file's model, the same in both summation orders -- iterations, the true relative residual, the
iterates' spread, the largest per-entry spread of the history, and how far the last entry above the threshold tol2 and the first one below
it lie from it, relative to the entry:
    fem_weak       12   1.2e-11   5.2e-16   6.5e-14   0.36 above, 68 below
    fem_mixed       9   6.0e-12   2.9e-16   2.4e-14   0.46 above, 280 below
    fem_scaled      9   1.8e-11   1.9e-16   3.4e-14   0.79 above, 32 below
    graph608       11   3.4e-11   1.5e-16   1.7e-09   0.95 above, 7.7 below
    graph608_two    9   7.9e-11   3.6e-17   6.2e-14   0.99 above, 0.61 below
    fem_weak amg22 10   2.8e-11   7.2e-15   1.7e-13   0.86 above, 13 below
The iterates of the five fit under PCG_ITERATE_SPREAD; amg22 has its own, PCG22_ITERATE_SPREAD 7.5e-15.  The history takes no single relative
tolerance: the tail of a converging history is rounding noise relative to itself (graph608: 1.7e-09 at its worst entry, 2e-16 at others), so
entry k is held to 100 times that entry's own forward-against-reversed spread, at least 100 * 2^-52 (history_tolerances).  The two entries
on either side of the threshold lie at least 0.36 of themselves from it, their tolerances are at most 1.7e-07: the device's count must be the
host's.  Ten times the largest true residual, 7.9e-10, rounded up to a power of ten is PCG_RESIDUAL_BOUND again.  Nobody has measured the
device's spreads on these cases: the tolerances come from this model alone."""
import ctypes
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import spmv_acc_amd
from test_amg_host import IRREGULAR_TAGS, TAGS, hierarchy, host_amg_cycle, host_spmv, problem, rhs_of
from test_coo_host import SHARED, _FakeTensor, _f, _i
from test_gs_host import HELPERS, row_sum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "spmv_acc_amd/csrc/"
NEW_SOURCES = ("cg.hpp", "k_cg.hip", "cg.cpp")
ENTRIES = "test_each_entry_is_the_host_model"
FROZEN = "test_frozen_state"
STRIDE = "test_cg_grid_stride_at_test_size"
CAPTURE = "test_update_and_direction_captured_and_replayed"
CONTRACT = "test_cg_contract"
AMG_PCG = "test_amg_pcg_is_the_host_model"
PLAIN = "test_plain_and_jacobi_cg_on_grid24"
CHECK_EVERY = "test_check_every_independence"
PARTIAL, FINISH, STATE, DOTS, BATCH = 1024, 256, 9, 3, 4  # kCgPartial, kCgFinishThreads, kCgState, kCgDots, kCgBatch (CG_SIZE_RULES holds them to the source)
WORDS = ("status", "iterations", "bb", "rr", "rz", "pq", "alpha", "beta", "tol2")  # the state block, in order
# the vector lengths of the GPU suite's entry tests: none, one term, a wavefront's 64 lanes and its neighbours, a chunk of 1024 and its
# neighbours, several chunks with a ragged last one, the smallest of them at which a finish lane adds a second partial (258 chunks), and
# 1026 chunks: lanes 0 and 1 of the finish enter its four-loads-ahead loop (the sizes users run take it), lane 2 and the others do not
SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 4 * 1024 + 17, 256 * 1024 + 1025, 1025 * 1024 + 1)
STRIDE_SIZE = 256 * 1024 + 1025  # the grid-stride test's: 258 chunks are 65 workgroups

PCG_RTOL, CG_RTOL, CG_FIRST = 1e-10, 1e-8, 10
PCG_COUNTS = dict(grid24=12, grid48=14, aniso48=13, aniso24=12)  # (the docstring; test_host_amg_pcg holds them to this file's model)
PCG_RESIDUAL_BOUND = 1e-9
PCG_ITERATE_SPREAD, PCG_HISTORY_SPREAD = 1.2e-15, 1e-13
CG_ITERATE_SPREAD, CG_HISTORY_SPREAD, CG_COUNT_SPREAD = 4e-16, 1e-15, 0
CG_COUNTS = dict(plain=77, jacobi=77)

# (rule, file, regex that must match the source, GPU tests of tests/test_gpu_cg.py that cross it at test size, what it selects)
CG_SIZE_RULES = [
    ("kCgPartial", CSRC + "cg.hpp", r"constexpr int kCgPartial = 1024;",
     [ENTRIES], "terms per partial: n = 1 .. 1023 are one ragged chunk, 1024 one full chunk, 1025 a full and a ragged one of one term, 4113 four and 17"),
    ("a full chunk", CSRC + "k_cg.hip", r"if \(left >= kCgPartial\) \{ // \(wave-uniform\)",
     [ENTRIES], "a full chunk tests no index (n >= 1024); the ragged last chunk walks its terms lane by lane (every n that is no multiple of 1024)"),
    ("the ragged last chunk", CSRC + "k_cg.hip", r"for \(long long i = base \+ lane; i < n; i \+= kWave\) \{",
     [ENTRIES], "n = 1 and 63 leave lanes without a term (+0.0), 64 fills the wavefront, 65 gives lane 0 a second term"),
    ("kCgBatch", CSRC + "cg.hpp", r"constexpr int kCgBatch = 4;",
     [ENTRIES], "a full chunk is four batches of four 512-B steps (every n >= 1024)"),
    ("kCgFinishThreads", CSRC + "cg.hpp", r"constexpr int kCgFinishThreads = 256;",
     [ENTRIES, STRIDE], "one workgroup combines the partials: up to 256 chunks one a lane (n <= 4113: lanes without a partial), 258 chunks give lanes 0 and 1 a second"),
    ("the finish's first partial", CSRC + "k_cg.hip", r"if \(c < nchunks\) \{",
     [ENTRIES], "a lane without a partial holds +0.0 (n = 0: all of them)"),
    ("four partials in flight", CSRC + "k_cg.hip", r"for \(; c \+ 3 \* kCgFinishThreads < nchunks; c \+= 4 \* kCgFinishThreads\) \{",
     [ENTRIES], "entered by the lanes t with t + 1024 < chunks: from 1 025 chunks on (n > 1 048 576).  n = 1 049 601 is 1 026 chunks: lanes 0 and 1 add "
                "four partials in the loop and none behind it, lanes 2 .. 255 take the one-by-one loop alone"),
    ("the finish's further partials", CSRC + "k_cg.hip", r"for \(; c < nchunks; c \+= kCgFinishThreads\) part \+= mine\[c\];",
     [ENTRIES, STRIDE], "258 chunks: lanes 0 and 1 add a second partial; 1 026 chunks: lanes 2 .. 255 add three one by one"),
    ("kWavesPerBlock", CSRC + "k_cg.hip", r"constexpr int kWavesPerBlock = kThreads / kWave;",
     [ENTRIES, STRIDE], "chunks per workgroup, one per wavefront: one chunk leaves three wavefronts without (n <= 1024), 258 chunks are 65 workgroups"),
    ("chunk loop", CSRC + "k_cg.hip", r"c < nchunks; c \+= stride\) \{ // \(wave-uniform\)",
     [STRIDE], "wavefronts stride over the chunks beyond the grid (258 chunks over 64 workgroups)"),
    ("kMaxGridBlocks (grid striding)", CSRC + SHARED, r"const long long cap = max_grid_blocks\(\);",
     [STRIDE], "every pass clamps its grid with passes::grid_for"),
    ("kMaxGridBlocks (grid striding): the passes' call", CSRC + "k_cg.hip", r"return grid_for\(cg_chunks\(n\), kWavesPerBlock\);",
     [STRIDE], "the launchers take the shared grid"),
    ("kCgDots", CSRC + "cg.hpp", r"constexpr int kCgDots = 3;",
     [ENTRIES], "the start's three dots off one pass, each with its own partials (dot d at d * chunks)"),
    ("kCgState", CSRC + "cg.hpp", r"constexpr int kCgState = 9;",
     [ENTRIES, FROZEN, CAPTURE], "the nine words of the state block (a replayed iteration carries on from the block the replay before left)"),
    ("frozen", CSRC + "k_cg.hip", r"if \(state\[kCgStatus\] != 0\) return;",
     [FROZEN, CHECK_EVERY, AMG_PCG], "every kernel of the update and the direction returns before it writes (pcg's batches of 8 run past the 12 to 14 iterations of AMG-PCG)"),
    ("the first status", CSRC + "k_cg.hip", r"const u64 status = !finite\(rz\) \? 3 : \(rr <= tol2 \? 1 : \(rz <= 0\.0 \? 3 : 0\)\);",
     [ENTRIES, FROZEN], "b = 0 and an exact x0 converge at the start; a NaN or a negative r.z break down"),
    ("breakdown 2", CSRC + "k_cg.hip", r"if \(finite\(pq\) && pq > 0\.0\) state\[kCgAlpha\] = ",
     [FROZEN], "p.q not finite (an inf, a NaN in p) or <= 0 (p = 0)"),
    ("breakdown 3", CSRC + "k_cg.hip", r"if \(finite\(rz_new\) && rz_new >= 0\.0\) \{",
     [FROZEN], "the new r.z not finite or < 0 (a negative dinv)"),
    ("the history's room", CSRC + "k_cg.hip", r"if \(done < static_cast<u64>\(hist_cap > 0 \? hist_cap : 0\)\) hist\[done\] = rr;",
     [ENTRIES, PLAIN], "hist[k] while k < hist_cap (the entry tests give room for two entries and take three iterations)"),
    ("jacobi fused", CSRC + "k_cg.hip", r"if \(dinv\) SPMV_ACC_LAUNCH\(cg_rz_pass_kernel<true>",
     [ENTRIES, PLAIN], "with d_dinv the pass writes z = dinv r; without it z is read (z == r: no preconditioner)"),
    ("no terms", CSRC + "k_cg.hip", r"if \(n <= 0\) return;",
     [ENTRIES], "n = 0: no pass is launched, the finishes are: every dot is +0.0 and the start converges at once"),
    ("int32 block arithmetic", CSRC + HELPERS, r"inline bool too_large\(long long v\) \{ return v > INT_MAX - \(1 << 16\); \}",
     [CONTRACT], "n beyond this: SPMV_ACC_ERR_TOO_LARGE, as the other entries"),
]


def test_cg_size_rules_name_their_tests():
    gpu_tests = open(os.path.join(ROOT, "tests", "test_gpu_cg.py")).read()
    defined = set(re.findall(r"^def (test_\w+)\(", gpu_tests, flags=re.M))
    for name, path, pattern, tests, what in CG_SIZE_RULES:
        assert re.search(pattern, open(os.path.join(ROOT, path)).read()), f"{name}: no longer matches {path}: {pattern}"
        assert tests and what
        for t in tests:
            assert t in defined, f"{name}: names {t}, which is not a test of tests/test_gpu_cg.py"
    # every named constant of the new files is registered above (tests/size_thresholds.py does not scan them)
    registered = " ".join(r[0] + " " + r[2] for r in CG_SIZE_RULES)
    found = 0
    for f in NEW_SOURCES:
        for k in re.findall(r"constexpr\s+[\w:<> ]+?\s+(k[A-Z]\w*)\s*=", open(os.path.join(ROOT, CSRC, f)).read()):
            found += 1
            assert k in registered, f"{f}: constant {k} is not in CG_SIZE_RULES"
    assert found == 6
    header = open(os.path.join(ROOT, CSRC, "cg.hpp")).read()
    for name, value in (("kCgPartial", PARTIAL), ("kCgFinishThreads", FINISH), ("kCgState", STATE), ("kCgDots", DOTS), ("kCgBatch", BATCH)):
        assert f"constexpr int {name} = {value};" in header, name
    assert spmv_acc_amd.CG_STATE == STATE and spmv_acc_amd.CG_WORDS == WORDS and len(spmv_acc_amd.CG_STATUS) == 4
    words = re.search(r"enum CgWord \{ ([^}]*) \};", header).group(1).replace(" = 0", "").split(", ")
    assert [w[3:].lower() for w in words] == list(WORDS), words  # kCgStatus, kCgIterations, ...: the documented order
    kernels = open(os.path.join(ROOT, CSRC, "k_cg.hip")).read()
    assert kernels.count("+= stride)") == 1 and kernels.count("gridDim.x") == 1  # every loop over work is the registered chunk loop
    for n, want in ((0, 0), (1, 3), (1024, 3), (1025, 6), (STRIDE_SIZE, 3 * 258), (SIZES[-1], 3 * 1026)):
        assert spmv_acc_amd.cg_partials(n) == want, n


PROTOTYPES = (
    r"int spmv_acc_cg_partials\(int n, size_t \*h_count\);",
    r"int spmv_acc_cg_start\(int n, double rtol, const double \*d_b, const double \*d_r, const double \*d_z, double \*d_p, double \*d_partials,\s*"
    r"unsigned long long \*d_state, double \*d_hist, int hist_cap\);",
    r"int spmv_acc_cg_update\(int n, const double \*d_p, const double \*d_q, double \*d_x, double \*d_r, double \*d_partials, unsigned long long \*d_state,\s*"
    r"double \*d_hist, int hist_cap\);",
    r"int spmv_acc_cg_direction\(int n, const double \*d_r, double \*d_z, const double \*d_dinv, double \*d_p, double \*d_partials,\s*"
    r"unsigned long long \*d_state\);",
)
SYMBOLS = ("spmv_acc_cg_partials", "spmv_acc_cg_start", "spmv_acc_cg_update", "spmv_acc_cg_direction")


def test_cg_entries_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "spmv_acc.h")).read()
    for proto in PROTOTYPES:
        assert re.search(proto, header), proto
    for entry in ("1", "2", "3", "4"):
        block = re.search(r"/\* ---- conjugate-gradient vector passes, " + entry + r".*?\*/", header, flags=re.S)
        assert block, entry
        for word in ("replaces: nothing in the reference", "COST", "CHECKS", "CANNOT CHECK"):
            assert word in block.group(0), (entry, word)
    layout = re.search(r"THE STATE BLOCK.*?IEEE divisions", header, flags=re.S).group(0)
    assert [layout.index(f"[{k}] {w}") for k, w in enumerate(WORDS)] == sorted(layout.index(f"[{k}] {w}") for k, w in enumerate(WORDS))
    # the header declares exactly what the package lists
    declared = set(re.findall(r"\b(sparse_spmv|spmv_acc_[a-z_0-9]+)\s*\(", header))
    assert declared == set(spmv_acc_amd.C_ABI_SYMBOLS), declared ^ set(spmv_acc_amd.C_ABI_SYMBOLS)
    lib = spmv_acc_amd.load_library()
    for s in SYMBOLS:
        assert s in spmv_acc_amd.C_ABI_SYMBOLS and hasattr(lib, s) and getattr(lib, s).restype is ctypes.c_int, s
    assert [len(getattr(lib, s).argtypes) for s in SYMBOLS] == [2, 10, 9, 7]
    assert lib.spmv_acc_cg_start.argtypes[1] is ctypes.c_double
    for f in ("cg_partials", "cg_start", "cg_update", "cg_direction", "pcg", "jacobi_inverse", "CgResult"):
        assert callable(getattr(spmv_acc_amd, f)), f
    assert spmv_acc_amd.CgResult._fields == ("status", "iterations", "rr", "bb", "history")
    assert "ZERO START" in spmv_acc_amd.pcg.__doc__ and "SYMMETRIC SWEEPS" in spmv_acc_amd.pcg.__doc__ and "symmetric operator" in spmv_acc_amd.pcg.__doc__
    for f in ("k_cg.hip", "cg.cpp"):  # both builds compile the new files
        assert f in open(os.path.join(ROOT, CSRC, "Makefile")).read() and f in open(os.path.join(ROOT, "CMakeLists.txt")).read(), f
    assert " cg.hpp " in open(os.path.join(ROOT, CSRC, "Makefile")).read()
    assert " k_cg " in open(os.path.join(ROOT, "tools", "resource_usage.sh")).read()
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "spmv_acc_cg_update" in text and "pcg" in text, doc


BAD, TOO_LARGE = 2, 4  # SPMV_ACC_ERR_BAD_ARGUMENT, SPMV_ACC_ERR_TOO_LARGE


def test_bad_arguments_are_refused_without_a_gpu():
    """The C entries check their arguments before they touch the device: the error codes come back on a machine without one."""
    lib = spmv_acc_amd.load_library()
    count = ctypes.c_size_t(77)
    assert lib.spmv_acc_cg_partials(-1, ctypes.byref(count)) == BAD and b"spmv_acc_cg_partials: negative" in lib.spmv_acc_last_error_string()
    assert lib.spmv_acc_cg_partials(5, None) == BAD and b"spmv_acc_cg_partials: null" in lib.spmv_acc_last_error_string()
    for big in (2 ** 31 - 1, 2 ** 31 - 2 ** 16):
        assert lib.spmv_acc_cg_partials(big, ctypes.byref(count)) == TOO_LARGE
    assert count.value == 77
    largest = 2 ** 31 - 2 ** 16 - 1
    assert lib.spmv_acc_cg_partials(largest, ctypes.byref(count)) == 0 and count.value == 3 * -(-largest // PARTIAL) and lib.spmv_acc_last_error() == 0

    # n = 100 doubles (800 B) per vector, 3 partials, 9 state words and 4 history entries, all at distinct places (never dereferenced)
    n = 100
    at = {name: (k + 1) << 20 for k, name in enumerate(("b", "r", "z", "p", "q", "x", "dinv", "partials", "state", "hist"))}
    size = dict(b=n, r=n, z=n, p=n, q=n, x=n, dinv=n, partials=3, state=STATE, hist=4)

    def start(nn=n, rtol=1e-8, cap=4, **over):
        a = dict(at, **over)
        return lib.spmv_acc_cg_start(nn, rtol, a["b"], a["r"], a["z"], a["p"], a["partials"], a["state"], a["hist"], cap)

    def update(nn=n, cap=4, **over):
        a = dict(at, **over)
        return lib.spmv_acc_cg_update(nn, a["p"], a["q"], a["x"], a["r"], a["partials"], a["state"], a["hist"], cap)

    def direction(nn=n, jacobi=False, **over):
        a = dict(at, **over)
        return lib.spmv_acc_cg_direction(nn, a["r"], a["z"], a["dinv"] if jacobi or "dinv" in over else None, a["p"], a["partials"], a["state"])

    def refused(call, name, code, *needles, **kw):
        assert call(**kw) == code, (name, kw)
        msg = lib.spmv_acc_last_error_string()
        assert msg.startswith(name.encode() + b": ") and all(s in msg for s in needles), (msg, kw)

    entries = (("spmv_acc_cg_start", start, ("b", "r", "z", "p"), ("p", "partials", "state", "hist"), ("b", "r", "z")),
               ("spmv_acc_cg_update", update, ("p", "q", "x", "r"), ("x", "r", "partials", "state", "hist"), ("p", "q")),
               ("spmv_acc_cg_direction", direction, ("r", "z", "p"), ("p", "partials", "state"), ("r", "z")))
    for name, call, vectors, written, read in entries:
        refused(call, name, BAD, b"negative n", nn=-1)
        for big in (2 ** 31 - 1, 2 ** 31 - 2 ** 16):
            refused(call, name, TOO_LARGE, b"int32", nn=big)
        for null in vectors + ("partials", "state"):
            refused(call, name, BAD, b"null", **{null: None})
        # every pair of written arrays, and every written array against every read one: the first element, the last, and one past either end
        for w in written:
            for other in written + read:
                if other == w:
                    continue
                for where in (at[other], at[other] + 8 * (size[other] - 1), at[other] - 8 * (size[w] - 1)):
                    refused(call, name, BAD, b" overlaps ", **{w: where})  # (adjacent arrays and z == r are accepted: the GPU suite, on real arrays)
    for name, call in (("spmv_acc_cg_start", start), ("spmv_acc_cg_update", update)):
        refused(call, name, BAD, b"negative hist_cap", cap=-1)
        refused(call, name, BAD, b"null hist", hist=None)
    for rtol in (-1e-8, float("nan"), float("inf"), -float("inf")):
        refused(start, "spmv_acc_cg_start", BAD, b"rtol", rtol=rtol)
    # Jacobi: z is written, so it may be neither r nor dinv
    refused(direction, "spmv_acc_cg_direction", BAD, b"z overlaps r", jacobi=True, z=at["r"])
    refused(direction, "spmv_acc_cg_direction", BAD, b"z overlaps dinv", jacobi=True, z=at["dinv"] + 8)
    refused(direction, "spmv_acc_cg_direction", BAD, b"p overlaps", jacobi=True, p=at["dinv"])
    lib.spmv_acc_clear_error()


def test_wrappers_refuse_bad_arguments():
    E = spmv_acc_amd.SpmvAccError
    n = 2000
    good = dict(b=_f(n), r=_f(n), z=_f(n), p=_f(n), q=_f(n), x=_f(n), dinv=_f(n), partials=_f(6), state=_FakeTensor(STATE, dtype="torch.int64"), hist=_f(5))

    def start(match, nn=n, rtol=1e-8, **bad):
        a = dict(good, **bad)
        with pytest.raises(E, match=match):
            spmv_acc_amd.cg_start(nn, rtol, a["b"], a["r"], a["z"], a["p"], a["partials"], a["state"], a["hist"])

    def update(match, nn=n, **bad):
        a = dict(good, **bad)
        with pytest.raises(E, match=match):
            spmv_acc_amd.cg_update(nn, a["p"], a["q"], a["x"], a["r"], a["partials"], a["state"], a["hist"])

    def direction(match, nn=n, **bad):
        a = dict(good, **bad)
        with pytest.raises(E, match=match):
            spmv_acc_amd.cg_direction(nn, a["r"], a["z"], a["p"], a["partials"], a["state"], a["dinv"])

    for call, vectors in ((start, ("b", "r", "z", "p")), (update, ("p", "q", "x", "r")), (direction, ("r", "z", "p", "dinv"))):
        call("negative", nn=-1)
        for v in vectors:
            call("not on the GPU", **{v: _f(n, cuda=False)})
            call("dtype", **{v: _i(n)})
            call("not contiguous", **{v: _f(n, contiguous=False)})
            call("as many", **{v: _f(n - 1)})
            call("as many", **{v: _f(n + 1)})
            call("on cuda:1", **{v: _f(n, device="cuda:1")})
            if v != "dinv":
                call("torch tensor", **{v: None})
            call("torch tensor", **{v: [0.0] * n})
        call("elements", partials=_f(5))
        call("dtype", partials=_i(6))
        call("torch tensor", partials=None)
        call("state block", state=_f(STATE))
        call("state block", state=_FakeTensor(STATE - 1, dtype="torch.int64"))
        call("not on the GPU", state=_FakeTensor(STATE, dtype="torch.int64", cuda=False))
        call("torch tensor", state=None)
    for call in (start, update):
        call("dtype", hist=_i(5))
        call("torch tensor", hist=[0.0])
    for rtol in (-1.0, float("nan"), float("inf"), "tight"):
        start("rtol", rtol=rtol)

    # pcg and jacobi_inverse, before any entry is called
    m, nnz = 10, 30
    A = (_i(m + 1), _i(nnz), _f(nnz))

    def solve(match, mm=m, A=A, b=_f(m), x=_f(m), **kw):
        with pytest.raises(E, match=match):
            spmv_acc_amd.pcg(mm, *A, b, x, **kw)

    solve("negative", mm=-1)
    for rtol in (-1.0, float("nan"), float("inf")):
        solve("rtol", rtol=rtol)
    solve("maxiter", maxiter=-1)
    solve("check_every", check_every=0)
    solve("negative sweeps", pre=-1)
    solve("torch tensor", b=None)
    solve("torch tensor", A=(None, A[1], A[2]))
    solve("as many", b=_f(m - 1))
    solve("as many", x=_f(m + 1))
    solve("inverse diagonal", precond=_f(m - 1))
    solve("torch tensor", precond=3.0)
    levels = spmv_acc_amd.AmgHierarchy([], spmv_acc_amd.amg.AmgCoarsest(m + 1, A, None, "coarse_rows"))
    solve("finest level has 11 rows, the matrix 10", precond=levels)
    with pytest.raises(E, match="negative"):
        spmv_acc_amd.jacobi_inverse(-1, *A)
    with pytest.raises(E, match="torch tensor"):
        spmv_acc_amd.jacobi_inverse(m, A[0], None, A[2])


def test_cg_entries_keep_no_state():
    """The engine file neither finds nor makes a plan, counts no plan work, reads no tunable and keeps nothing static; the three device entries
    are launch-only -- no allocation, no copy, no memset, no synchronisation, no capture check --, refuse before their first launch, and
    enqueue their launches in the documented order."""
    src = open(os.path.join(ROOT, CSRC, "cg.cpp")).read()
    code = re.sub(r"//[^\n]*", "", src)
    for word in ("get_plan", "g_plans", "t_plan_work", "t_last_plan", "tune_", "TimingPhase", "TuneTimer", "static std::", "thread_local", "g_tunables",
                 "hipMalloc", "hipFree", "hipMemcpy", "hipMemset", "Synchronize", "plan_work_allowed", "stream_capturing", "while ("):
        assert word not in code, word
    assert not re.search(r"\bstatic\b(?! const char \*const kEntry)", code), "a static other than the entries' names"
    assert '#include "' + HELPERS + '"' in src and not re.search(r"\b(cg)_(error|too_large|aligned_up|overlap)\(", code)
    order = dict(run_cg_start=("launch_cg_start_pass", "launch_cg_start_finish"),
                 run_cg_update=("launch_cg_pq_pass", "launch_cg_pq_finish", "launch_cg_update_pass", "launch_cg_rr_finish"),
                 run_cg_direction=("launch_cg_rz_pass", "launch_cg_rz_finish", "launch_cg_direction_pass"))
    for entry, launches in order.items():
        body = code.split("int " + entry + "(")[1].split("\n}\n")[0]
        assert re.findall(r"\blaunch_\w+(?=\(st, )", body) == list(launches), entry  # two, four and three launches, in the documented order
        before = body.split(launches[0] + "(")[0]
        assert before.count("first_overlap(") >= 1 and "common_refusals(kEntry, n, d_partials, d_state)" in before  # refused before any launch
        assert body.index("note_stream_use();") < body.index(launches[0] + "(") and body.rstrip().endswith("return launch_error(kEntry);")
    partials = code.split("int run_cg_partials(")[1].split("\n}\n")[0]
    assert "launch_" not in partials and "t_stream" not in partials  # host arithmetic only
    kernels = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, CSRC, "k_cg.hip")).read())
    assert "atomic" not in kernels.lower() and "while (" not in kernels and "cooperative" not in kernels.lower()
    assert kernels.count("__shared__") == 1 and kernels.count("__syncthreads()") == 1  # LDS in the finish alone, behind one barrier
    # frozen: the seven kernels of the update and the direction read the status before anything else
    for name in ("cg_pq_pass_kernel", "cg_pq_finish_kernel", "cg_update_pass_kernel", "cg_rr_finish_kernel", "cg_rz_pass_kernel", "cg_rz_finish_kernel",
                 "cg_direction_pass_kernel"):
        body = kernels.split("void " + name + "(")[1].split("{", 1)[1]
        first = [ln.strip() for ln in body.splitlines() if ln.strip() and not ln.strip().startswith("#pragma")][0]
        assert first.startswith("if (state[kCgStatus] != 0) return;"), (name, first)
    for name in ("cg_start_pass_kernel", "cg_start_finish_kernel"):
        assert "kCgStatus] != 0" not in kernels.split("void " + name + "(")[1].split("\n}\n")[0], name


KERNELS = ("cg_start_pass_kernel", "cg_start_finish_kernel", "cg_pq_pass_kernel", "cg_pq_finish_kernel", "cg_update_pass_kernel", "cg_rr_finish_kernel",
           "cg_rz_pass_kernel", "cg_rz_finish_kernel", "cg_direction_pass_kernel")
# as recorded in k_cg.hip's header comment (cg_rz_pass_kernel: the larger of its two instances)
RECORDED_VGPRS = dict(cg_start_pass_kernel=58, cg_start_finish_kernel=24, cg_pq_pass_kernel=34, cg_pq_finish_kernel=18, cg_update_pass_kernel=62,
                      cg_rr_finish_kernel=18, cg_rz_pass_kernel=40, cg_rz_finish_kernel=18, cg_direction_pass_kernel=28)


def test_cg_kernels_fit_their_register_budget(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_table

    asm = tmp_path / "k_cg.s"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-DKERNEL_STRATEGY_ADAPTIVE",
                        "-I" + os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-S",
                        os.path.join(ROOT, CSRC, "k_cg.hip"), "-o", str(asm)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    text = asm.read_text()
    assert set(re.findall(r"\.wavefront_size:\s*(\d+)", text)) == {"64"}  # wave64, every kernel of the file
    bodies = {}
    for mt in re.finditer(r"^(_ZN8spmv_acc\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, flags=re.M | re.S):
        bodies[mt.group(1)] = mt.group(2)
    assert len(bodies) == len(KERNELS) + 1, sorted(bodies)  # (cg_rz_pass_kernel twice: with and without dinv)
    for k, b in bodies.items():
        assert "atomic" not in b, k  # no atomics anywhere
        assert "s_sleep" not in b, k  # ... and nothing waits
        # contraction is off: products and sums are instructions of their own; the only fused operations are an IEEE division's own expansion
        outside = re.sub(r"v_div_scale_f64.*?v_div_fixup_f64", "", b, flags=re.S)
        assert "v_fma_f64" not in outside and "v_fmac_f64" not in outside, k
        divisions = len(re.findall(r"v_div_fixup_f64", b))
        assert divisions == (1 if "cg_pq_finish" in k or "cg_rz_finish" in k else 0), (k, divisions)  # alpha and beta, nothing else
        if "_pass_kernel" in k:
            assert "v_mul_f64" in b and ("v_add_f64" in b) and "ds_" not in b.replace("ds_swizzle", "").replace("ds_bpermute", ""), k  # no LDS array in a pass
    header = open(os.path.join(ROOT, CSRC, "k_cg.hip")).read().split("#include")[0]
    rows = [k for k in resource_table.parse(r.stderr) if "rocprim" not in k["name"]]
    for k in rows:
        k["name"] = re.sub(r"<.*", "", k["name"])
    assert sorted(set(k["name"] for k in rows)) == sorted(KERNELS) and len(rows) == len(KERNELS) + 1, sorted(k["name"] for k in rows)
    for k in rows:
        assert k["scratch"] == 0 and k["agprs"] == 0 and k["vgprs"] <= 64 and k["occupancy"] >= 8, k
        want = RECORDED_VGPRS[k["name"]]
        assert re.search(k["name"] + r", " + str(want) + r"\b", header), (k["name"], "the count recorded in the header comment")
        assert k["vgprs"] <= want + 4, (k, "grew past the count recorded in k_cg.hip (a few registers of compiler drift are allowed)")


# ---- the dot product and the three entries (cg.hpp), in numpy, bit for bit: the GPU suite's reference ------------------------------------------------
def host_cg_dot(u, v):
    """cg.hpp THE DOT PRODUCT: the terms rounded on their own, one row_sum(., 64) per chunk of 1024 terms, row_sum(partials, 256)."""
    with np.errstate(all="ignore"):
        terms = np.asarray(u, dtype=np.float64) * np.asarray(v, dtype=np.float64)
        partials = np.array([row_sum(terms[c:c + PARTIAL], 64) for c in range(0, terms.size, PARTIAL)], dtype=np.float64)
        return np.float64(row_sum(partials, FINISH))


def host_cg_start(rtol, b, r, z, hist=None):
    """(p, state): cg.hpp THE START's finish.  hist (may be None) is written in place."""
    bb, rr, rz = host_cg_dot(b, b), host_cg_dot(r, r), host_cg_dot(r, z)
    with np.errstate(all="ignore"):
        tol2 = (np.float64(rtol) * np.float64(rtol)) * bb
    status = 3 if not np.isfinite(rz) else (1 if rr <= tol2 else (3 if rz <= 0.0 else 0))
    if hist is not None and hist.size > 0:
        hist[0] = rr
    state = dict(status=status, iterations=0, bb=bb, rr=rr, rz=rz, pq=np.float64(0.0), alpha=np.float64(0.0), beta=np.float64(0.0), tol2=tol2)
    return np.array(z, dtype=np.float64), state


def host_cg_update(p, q, x, r, state, hist=None):
    """(x, r, state), new arrays and a new dict: cg.hpp THE UPDATE's finishes.  Frozen: with a status other than 0 everything is returned as it is."""
    x, r, state = np.array(x, dtype=np.float64), np.array(r, dtype=np.float64), dict(state)
    if state["status"] != 0:
        return x, r, state
    pq = host_cg_dot(p, q)
    state["pq"] = pq
    if not (np.isfinite(pq) and pq > 0.0):
        state["status"] = 2
        return x, r, state
    with np.errstate(all="ignore"):
        alpha = state["rz"] / pq
        state["alpha"] = alpha
        x = x + alpha * p  # (numpy rounds the product and the sum on their own)
        r = r - alpha * q
    rr = host_cg_dot(r, r)
    state["rr"] = rr
    state["iterations"] += 1
    if hist is not None and state["iterations"] < hist.size:
        hist[state["iterations"]] = rr
    if rr <= state["tol2"]:
        state["status"] = 1
    return x, r, state


def host_cg_direction(r, z, p, state, dinv=None):
    """(z, p, state): cg.hpp THE DIRECTION's finish.  dinv: z = dinv * r first.  Frozen likewise; on status 3 z is written (Jacobi) but p is not."""
    z, p, state = np.array(z, dtype=np.float64), np.array(p, dtype=np.float64), dict(state)
    if state["status"] != 0:
        return z, p, state
    with np.errstate(all="ignore"):
        if dinv is not None:
            z = dinv * r
        rz_new = host_cg_dot(r, z)
        if not (np.isfinite(rz_new) and rz_new >= 0.0):
            state["status"] = 3
            return z, p, state
        beta = rz_new / state["rz"]
        state["beta"], state["rz"] = beta, rz_new
        p = z + beta * p
    return z, p, state


def state_words(state):
    """The state dict as the nine 64-bit words of the device's block."""
    out = np.zeros(STATE, dtype=np.uint64)
    out[0], out[1] = state["status"], state["iterations"]
    out[2:] = np.array([state[w] for w in WORDS[2:]], dtype=np.float64).view(np.uint64)
    return out


def host_pcg(A, b, x0, precond=None, rtol=1e-8, maxiter=1000, reverse=False, pre=1, post=1):
    """pcg restated: precond None, an inverse diagonal (an array), or a host hierarchy (a tuple: one host_amg_cycle from a zero start with `pre`
    and `post` symmetric sweeps).  reverse: the SpMVs add their rows from the last entry.  Returns dict(status, iterations, history (an array of iterations + 1 entries), iterates (x
    after each iteration), x, state)."""
    m = b.size
    hist = np.zeros(maxiter + 1)
    amg = precond if isinstance(precond, tuple) else None
    dinv = None if amg is not None or precond is None else np.asarray(precond, dtype=np.float64)
    x = np.array(x0, dtype=np.float64)
    r = b - host_spmv(A, x, reverse)

    def M(r):
        return host_amg_cycle(amg, r, np.zeros(m), pre, post, reverse=reverse) if amg is not None else (dinv * r if dinv is not None else r)

    z = M(r)
    p, state = host_cg_start(rtol, b, r, z, hist)
    iterates = []
    while state["status"] == 0 and state["iterations"] < maxiter:
        q = host_spmv(A, p, reverse)
        x, r, state = host_cg_update(p, q, x, r, state, hist)
        if state["status"] != 2:
            iterates.append(x)
        if amg is not None and state["status"] == 0:
            z = M(r)
        z, p, state = host_cg_direction(r, r if precond is None else z, p, state, dinv)
    return dict(status=state["status"], iterations=state["iterations"], history=hist[:state["iterations"] + 1].copy(), iterates=tuple(iterates), x=x, state=state)


# ---- the solves of the GPU suite, made once and shared --------------------------------------------------------------------------------------------
def matrix(tag):
    """(m, A) of the finest level of a hierarchy of tests/test_amg_host.py."""
    return problem(tag)[:2]


def inverse_diagonal(tag):
    m, (rp, ci, v) = matrix(tag)
    row = np.repeat(np.arange(m), np.diff(rp))
    return 1.0 / v[ci == row]


@functools.lru_cache(maxsize=None)
def solve(tag, kind, reverse=False):
    """The host solve of the GPU suite: kind "amg" (rtol 1e-10), "plain" or "jacobi" (rtol 1e-8), b = rhs_of(tag), x0 = 0; or "amg22": AMG-PCG
    with pre = post = 2 from the non-zero start x0_of(tag)."""
    m, A = matrix(tag)
    if kind == "amg22":
        return host_pcg(A, rhs_of(tag), x0_of(tag), hierarchy(tag), rtol=PCG_RTOL, reverse=reverse, pre=2, post=2)
    precond = {"amg": hierarchy(tag), "plain": None, "jacobi": None if kind != "jacobi" else inverse_diagonal(tag)}[kind]
    return host_pcg(A, rhs_of(tag), np.zeros(m), precond, rtol=PCG_RTOL if kind == "amg" else CG_RTOL, reverse=reverse)


def x0_of(tag):
    """The non-zero start of the "amg22" solve: standard normal, seeded."""
    return np.random.default_rng(22).standard_normal(matrix(tag)[0])


def history_tolerances(tag, kind="amg"):
    """Entry by entry, the relative tolerance the device's history is held to on the irregular cases: 100 times that entry's own forward
    against reversed spread, at least 100 * 2^-52 (the tail of a converging history is rounding noise relative to itself)."""
    fwd, rev = solve(tag, kind)["history"], solve(tag, kind, True)["history"]
    assert fwd.size == rev.size
    return np.maximum(100.0 * np.abs(fwd - rev) / fwd, 100.0 * 2.0 ** -52)


def true_residual(tag, x):
    m, A = matrix(tag)
    b = rhs_of(tag)
    return float(np.linalg.norm(b - host_spmv(A, x)) / np.linalg.norm(b))


@functools.lru_cache(maxsize=None)
def stationary_cycles(tag, target, cap=80):
    """Cycles of the stationary amg_cycle loop (x0 = 0) until the true relative residual is at most target."""
    m, A = matrix(tag)
    b, x = rhs_of(tag), np.zeros(m)
    for k in range(1, cap + 1):
        x = host_amg_cycle(hierarchy(tag), b, x)
        if np.linalg.norm(b - host_spmv(A, x)) <= target * np.linalg.norm(b):
            return k
    return cap + 1


def test_the_dot_is_two_levels_of_row_sum():
    rng = np.random.default_rng(41)
    u = rng.standard_normal(3 * PARTIAL + 100) * 10.0 ** rng.integers(-6, 6, 3 * PARTIAL + 100)
    v = rng.standard_normal(u.size)
    assert host_cg_dot(u[:0], v[:0]) == 0.0 and not np.signbit(host_cg_dot(u[:0], v[:0]))  # n = 0: +0.0
    assert host_cg_dot(u[:1], v[:1]) == u[0] * v[0]
    for n in (63, 64, 65, PARTIAL, PARTIAL + 1, u.size):
        terms = u[:n] * v[:n]
        parts = []
        for c in range(0, n, PARTIAL):  # lane by lane, in Python floats
            chunk = terms[c:c + PARTIAL]
            lanes = []
            for lane in range(64):
                mine = chunk[lane::64]
                acc = mine[0] if mine.size else 0.0
                for w in mine[1:]:
                    acc = acc + w
                lanes.append(acc)
            while len(lanes) > 1:
                lanes = [lanes[2 * k] + lanes[2 * k + 1] for k in range(len(lanes) // 2)]
            parts.append(lanes[0])
        lanes = [0.0] * FINISH
        for k, s in enumerate(parts):
            lanes[k % FINISH] = s if k < FINISH else lanes[k % FINISH] + s
        while len(lanes) > 1:
            lanes = [lanes[2 * k] + lanes[2 * k + 1] for k in range(len(lanes) // 2)]
        assert host_cg_dot(u[:n], v[:n]) == lanes[0], n
        assert abs(host_cg_dot(u[:n], v[:n]) - np.dot(u[:n], v[:n])) <= 4 * n * 2.0 ** -53 * np.dot(np.abs(u[:n]), np.abs(v[:n]))
    # 258 partials: lanes 0 and 1 of the finish add a second one
    big = rng.standard_normal(STRIDE_SIZE)
    parts = np.array([row_sum((big * big)[c:c + PARTIAL], 64) for c in range(0, big.size, PARTIAL)])
    assert parts.size == 258
    lanes = parts[:FINISH].copy()
    lanes[0], lanes[1] = lanes[0] + parts[256], lanes[1] + parts[257]
    assert host_cg_dot(big, big) == row_sum(lanes, FINISH)
    assert np.isnan(host_cg_dot(np.array([1.0, np.nan]), np.ones(2))) and host_cg_dot(np.array([np.inf]), np.ones(1)) == np.inf


def test_the_entries_on_a_small_system():
    """The three host entries composed by hand are textbook CG: on a 3 x 3 SPD system the solve ends in three iterations, the state's scalars are
    the recurrence's, the history is r.r, a frozen state changes nothing, and the start's and the breakdowns' statuses are the documented ones."""
    A = np.array([[4.0, 1.0, 0.0], [1.0, 3.0, 1.0], [0.0, 1.0, 2.0]])
    b = np.array([1.0, 2.0, 3.0])
    hist = np.full(8, -1.0)
    x = np.zeros(3)
    r = b - A @ x
    p, st = host_cg_start(1e-12, b, r, r, hist)
    assert st["status"] == 0 and st["iterations"] == 0 and st["bb"] == st["rr"] == st["rz"] == 14.0 and hist[0] == 14.0
    assert st["tol2"] == (np.float64(1e-12) * np.float64(1e-12)) * np.float64(14.0)
    for k in range(1, 4):
        x, r, st = host_cg_update(p, A @ p, x, r, st, hist)
        assert st["iterations"] == k and hist[k] == st["rr"] == host_cg_dot(r, r)
        z, p, st = host_cg_direction(r, r, p, st)
    assert st["status"] == 1 and np.allclose(A @ x, b, rtol=0, atol=1e-12) and np.all(hist[4:] == -1.0)
    x2, r2, st2 = host_cg_update(p, A @ p, x, r, st, hist)  # frozen
    z2, p2, st3 = host_cg_direction(r2, r2, p, st2)
    assert np.array_equal(x2, x) and np.array_equal(r2, r) and np.array_equal(p2, p) and st2 == st and st3 == st and np.all(hist[4:] == -1.0)
    assert np.array_equal(state_words(st)[:2], [1, 3]) and state_words(st)[3:4].view(np.float64)[0] == st["rr"]
    # the start: b = 0 and an exact x0 converge at once; a NaN or a non-positive r.z break down
    assert host_cg_start(1e-8, np.zeros(3), np.zeros(3), np.zeros(3))[1]["status"] == 1
    assert host_cg_start(0.0, b, np.zeros(3), np.zeros(3))[1]["status"] == 1  # rr = 0 <= tol2 = 0
    assert host_cg_start(1e-8, b, b, -b)[1]["status"] == 3 and host_cg_start(1e-8, b, b, b * np.nan)[1]["status"] == 3
    assert host_cg_start(1e-8, b, b, np.zeros(3))[1]["status"] == 3  # r.z = 0 while r.r > tol2
    # the update: p = 0, an inf and a NaN in p give status 2 and leave x and r alone
    _, st = host_cg_start(1e-8, b, b, b)
    for bad in (np.zeros(3), np.array([np.inf, 0.0, 0.0]), np.array([np.nan, 1.0, 1.0])):
        with np.errstate(all="ignore"):
            x2, r2, st2 = host_cg_update(bad, A @ bad, np.ones(3), b, st)
        assert st2["status"] == 2 and st2["iterations"] == 0 and np.array_equal(x2, np.ones(3)) and np.array_equal(r2, b)
    # the direction: a negative inverse diagonal gives status 3, z written, p kept
    z2, p2, st2 = host_cg_direction(b, np.zeros(3), b, st, dinv=-np.ones(3))
    assert st2["status"] == 3 and np.array_equal(z2, -b) and np.array_equal(p2, b) and st2["rz"] == st["rz"]


@pytest.mark.parametrize("tag", TAGS)
def test_host_amg_pcg(tag):
    """AMG-PCG at rtol 1e-10: the pinned iteration count, no history entry near the threshold (so that the device's count must be the same),
    the true residual below the bound, and fewer than half the cycles the stationary loop needs for that residual."""
    for reverse in (False, True):
        s = solve(tag, "amg", reverse)
        assert s["status"] == 1 and s["iterations"] == PCG_COUNTS[tag] and len(s["iterates"]) == s["iterations"], (tag, reverse, s["iterations"])
        tol2 = s["state"]["tol2"]
        nearest = float(np.min(np.abs(s["history"] - tol2) / tol2))
        assert nearest > 1e-6, (tag, reverse, nearest)
        assert np.all(s["history"][:-1] > tol2) and s["history"][-1] <= tol2
    s = solve(tag, "amg")
    res = true_residual(tag, s["x"])
    cycles = stationary_cycles(tag, res)
    factor = (s["history"][-1] / s["history"][0]) ** (0.5 / s["iterations"])
    print(f"{tag}: {s['iterations']} iterations, factor per iteration {factor:.2f}, true relative residual {res:.2e}, stationary cycles to the same {cycles}")
    assert res <= PCG_RESIDUAL_BOUND / 10 and 2 * s["iterations"] < cycles <= 80, (tag, res, cycles)


PCG_IRREGULAR_COUNTS = dict(fem_weak=12, fem_mixed=9, fem_scaled=9, graph608=11, graph608_two=9)  # (the docstring; held to this file's model)
PCG22_COUNT = 10  # fem_weak from the start x0_of with pre = post = 2
PCG22_ITERATE_SPREAD = 7.5e-15
IRREGULAR_SOLVES = tuple((t, "amg") for t in IRREGULAR_TAGS) + (("fem_weak", "amg22"),)


def solve_count(tag, kind):
    return PCG22_COUNT if kind == "amg22" else PCG_IRREGULAR_COUNTS[tag]


def iterate_spread(kind):
    return PCG22_ITERATE_SPREAD if kind == "amg22" else PCG_ITERATE_SPREAD


@pytest.mark.parametrize("tag,kind", IRREGULAR_SOLVES)
def test_host_amg_pcg_on_the_irregular_cases(tag, kind):
    """AMG-PCG at rtol 1e-10 on the irregular cases (and fem_weak from a non-zero start with pre = post = 2): the pinned count in both summation
    orders, and, in both, the last history entry above the threshold and the first one below it farther from it than that entry's tolerance
    (history_tolerances) -- so the device's count must be the host's --; the true residual a tenth of the bound."""
    tols = history_tolerances(tag, kind)
    for reverse in (False, True):
        s = solve(tag, kind, reverse)
        n = s["iterations"]
        assert s["status"] == 1 and n == solve_count(tag, kind) and len(s["iterates"]) == n and n > 5, (tag, kind, reverse, n)
        tol2, h = s["state"]["tol2"], s["history"]
        assert np.all(h[:-1] > tol2) and h[-1] <= tol2
        for k in (n - 1, n):
            assert abs(h[k] - tol2) > tols[k] * h[k], (tag, kind, reverse, k, h[k], tol2, tols[k])
    s = solve(tag, kind)
    res = true_residual(tag, s["x"])
    print(f"{tag} {kind}: {s['iterations']} iterations, true relative residual {res:.2e}, threshold margins "
          f"{abs(s['history'][-2] - tol2) / s['history'][-2]:.2g} above and {abs(s['history'][-1] - tol2) / s['history'][-1]:.2g} below")
    assert res <= PCG_RESIDUAL_BOUND / 10, (tag, kind, res)
    if kind == "amg22":  # the options change the solve: another count, other iterates than pre = post = 1 from zero
        assert not np.array_equal(s["x"], solve(tag, "amg")["x"]) and np.any(x0_of(tag) != 0.0)


@pytest.mark.parametrize("tag,kind", IRREGULAR_SOLVES)
def test_the_irregular_spreads(tag, kind):
    """The iterates' spread fits under its constant; the history's is per entry (history_tolerances): its largest is printed for the docstring."""
    a, b = solve(tag, kind), solve(tag, kind, True)
    its, hist = spread(a, b)
    print(f"{tag} {kind}: forward against reversed: iterates {its:.3g}, history {hist:.3g} at the worst entry; tolerances {history_tolerances(tag, kind).min():.3g} to "
          f"{history_tolerances(tag, kind).max():.3g}")
    assert its <= iterate_spread(kind), (tag, kind, its)


def spread(a, b, upto=None):
    """(iterates, history): the largest difference of two solves over their first `upto` iterations (None: all; the counts must then agree)."""
    k = min(a["iterations"], b["iterations"]) if upto is None else upto
    assert upto is not None or a["iterations"] == b["iterations"]
    its = max(float(np.max(np.abs(u - v)) / np.max(np.abs(u))) for u, v in zip(a["iterates"][:k], b["iterates"][:k]))
    ha, hb = a["history"][:k + 1], b["history"][:k + 1]
    return its, float(np.max(np.abs(ha - hb) / ha))


@pytest.mark.parametrize("tag", TAGS)
def test_the_spreads(tag):
    """The spreads of the module docstring, measured again: the GPU suite's tolerances are 100 times these constants."""
    its, hist = spread(solve(tag, "amg"), solve(tag, "amg", True))
    print(f"{tag}: AMG-PCG forward against reversed: iterates {its:.3g}, history {hist:.3g}")
    assert its <= PCG_ITERATE_SPREAD and hist <= PCG_HISTORY_SPREAD, (tag, its, hist)
    if tag == "grid24":
        for kind in ("plain", "jacobi"):
            fwd, rev = solve(tag, kind), solve(tag, kind, True)
            its, hist = spread(fwd, rev, CG_FIRST)
            print(f"{tag}: {kind} CG forward against reversed, first {CG_FIRST}: iterates {its:.3g}, history {hist:.3g}; iterations {fwd['iterations']} and {rev['iterations']}")
            assert its <= CG_ITERATE_SPREAD and hist <= CG_HISTORY_SPREAD, (kind, its, hist)
            assert fwd["status"] == rev["status"] == 1 and fwd["iterations"] == CG_COUNTS[kind]
            assert abs(fwd["iterations"] - rev["iterations"]) <= CG_COUNT_SPREAD, (kind, fwd["iterations"], rev["iterations"])


if __name__ == "__main__":
    for t in TAGS:
        a, b = solve(t, "amg"), solve(t, "amg", True)
        res = true_residual(t, a["x"])
        near = min(float(np.min(np.abs(s["history"] - s["state"]["tol2"]) / s["state"]["tol2"])) for s in (a, b))
        print(t, a["iterations"], b["iterations"], f"{res:.3e}", stationary_cycles(t, res), spread(a, b), f"nearest {near:.3g}")
    for kind in ("plain", "jacobi"):
        a, b = solve("grid24", kind), solve("grid24", kind, True)
        print(kind, a["iterations"], b["iterations"], spread(a, b, CG_FIRST))
    for t, kind in IRREGULAR_SOLVES:
        a, b = solve(t, kind), solve(t, kind, True)
        print(t, kind, a["iterations"], b["iterations"], f"{true_residual(t, a['x']):.3e}", spread(a, b), f"largest tolerance {history_tolerances(t, kind).max():.3g}")
