"""GPU suite (-m gpu) of the C++ strategy surface: the 19 C++-linkage entries of include/api/spmv.h and include/spmv_acc_strategies.hpp, called the
way the reference's executables call them (tests/cxx/surface_driver.cpp: ONE process, every entry on every case and alpha / beta pair of
tests/cxx_surface_cases.py, tunable strict_strategy = 1), and the two-width split forms of k_vector_row.hip through the C ABI.

Every y is held to the CPU oracle by tests/test_gpu_parity.py::check (the project's SCALED_TOL / REL_TOL and the reference's own verdict); a wrapper
that forwards to the wrong strategy still gives a correct y, so the kernel each plan recorded is compared with what the wrapper's name promises."""
import os
import subprocess

import numpy as np
import pytest

import cxx_surface_cases as T
import spmv_acc_amd
from test_gpu_parity import check

pytestmark = pytest.mark.gpu

ROWBLOCK, PLUS, FLAT_TILE, VECTOR_TILE, VECTOR_ROW, WAVE_ROW, LIGHT, BLOCK_ROW, SCALE_ONLY = 0, 1, 2, 4, 5, 6, 7, 8, 10  # enum spmv_acc_kernel
NO_PLAN = -2
UNSUPPORTED_TRANS = 1  # enum spmv_acc_error


@pytest.fixture(scope="module")
def surface(hiplib, tmp_path_factory):
    """The driver's records {(tag, pair index or 'trans', call): (y, error word, last kernel)}: compiled once, run once."""
    tmp = tmp_path_factory.mktemp("cxx_surface")
    exe, inp, outp = tmp / "surface_driver", tmp / "cases.bin", tmp / "out.bin"
    subprocess.run(T.hipcc_command("surface_driver.cpp", exe), check=True)
    T.write_input(inp)
    r = subprocess.run([str(exe), str(inp), str(outp)], env=dict(os.environ, SPMV_ACC_TUNABLES="strict_strategy=1"), capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return T.read_output(outp)


@pytest.fixture(scope="module")
def inputs():
    """{tag: (rowptr, cols, vals, x, y0)}"""
    return {tag: (rowptr, cols, vals) + T.vectors(tag, rowptr.size - 1, n) for tag, rowptr, cols, vals, n in T.CASES}


def _check_call(oracle, surface, inputs, tag, k, alpha, beta, checked):
    """Every call of one (case, pair) against the oracle.  Calls that returned the same bits are checked once."""
    rowptr, cols, vals, x, y0 = inputs[tag]
    y_start = y0 if beta != 0.0 else np.zeros_like(y0)  # (beta == 0: the entry was handed NaNs, which it must not read; the reference starts from anything)
    seen = set()
    for call in T.CALLS:
        y, err, _ = surface[(tag, k, call)]
        assert not np.isnan(y).any(), (tag, alpha, beta, call, "NaN in y", np.nonzero(np.isnan(y))[0][:8].tolist())
        if alpha == 0.0:
            assert np.array_equal(y, beta * y0), (tag, call, "alpha = 0 must give exactly beta * y0")
        key = y.tobytes()
        if key not in seen:
            seen.add(key)
            check(oracle, y, alpha, beta, rowptr, cols, vals, x, y_start, ("cxx", tag, alpha, beta, call))
        checked.append(call)


def test_every_entry_gives_the_oracles_y(oracle, surface, inputs):
    """Every entry, every hint set of the two hinted wrappers, every case, every alpha / beta pair: y passes check, the error word is 0."""
    for tag in T.TAGS:
        for k, (alpha, beta) in enumerate(T.ALPHA_BETA):
            checked = []
            _check_call(oracle, surface, inputs, tag, k, alpha, beta, checked)
            assert checked == T.CALLS
            errors = {call: surface[(tag, k, call)][1] for call in T.CALLS if surface[(tag, k, call)][1] != 0}
            assert not errors, (tag, alpha, beta, errors)


# What each wrapper's plan must have recorded under strict_strategy = 1, with the line of spmv_acc_amd/csrc/dispatch.cpp (cxx_api.cpp for the wrapper's
# strategy) it was read from.  PLUS beside ROWBLOCK / VECTOR_TILE is the family's rescue of unbalanced rows (run_rowblock, dispatch.cpp:221-222).
EXPECTED_KERNEL = {
    "flat": {FLAT_TILE},                        # kFlat -> run_flat, strict: :19, :79
    "segment_sum_flat": {FLAT_TILE},            # kFlat under FlatSegmentSumScope (cxx_api.cpp): :79
    "adaptive_flat": {FLAT_TILE},               # kFlat, the hints are not used (cxx_api.cpp): :79
    "line_enhance": {ROWBLOCK, PLUS},           # kLineEnhance -> run_rowblock :1096-1098, :326, rescue :537
    "adaptive_enhance": {ROWBLOCK, PLUS},       # kLineEnhance
    "adaptive_line": {ROWBLOCK, PLUS},          # kLine :1097
    "line": {ROWBLOCK, PLUS},                   # kLine :1097
    "thread_row": {ROWBLOCK, PLUS},             # kThreadRow -> run_rowblock with one lane per row :1089-1094
    "default": {ROWBLOCK, PLUS},                # kDefault -> run_rowblock, uneven switch allowed :1085-1087
    "vec_row": {VECTOR_TILE, PLUS},             # kVectorRow, tile form :1074, the rescue :1064
    "wf_row": {WAVE_ROW},                       # kWfRow :1081-1083
    "light": {LIGHT},                           # kLight :1032-1044
    "block_row": {BLOCK_ROW},                   # kBlockRowOrdinary :1046-1048
    "csr_adaptive_plus<true>": {PLUS},          # kAdaptivePlus -> run_plus :1149, :537
    "csr_adaptive_plus<false>": {PLUS},
}
ANY_KERNEL = ("sparse_csr_spmv", "sparse_spmv", "adaptive")  # the active strategy / adaptive: the engine's choice, any kernel (>= 0)


def test_every_wrapper_ran_the_kernel_its_name_says(surface):
    for tag in T.TAGS:
        for k in range(len(T.ALPHA_BETA)):
            kernel = {call: surface[(tag, k, call)][2] for call in T.CALLS}
            where = (tag, T.ALPHA_BETA[k])
            # the hand-launched split makes no plan: no record on the fresh matrix, whatever its hints
            for h in T.HINT_NAMES:
                assert kernel[f"adaptive_vec_row[{h}]"] == NO_PLAN, (where, h, kernel[f"adaptive_vec_row[{h}]"])
            # ... and leaves the record of the call before it alone
            assert kernel["adaptive_vec_row[after]"] == kernel["csr_adaptive_plus<false>"], where
            for call in T.CALLS:
                if call.startswith("adaptive_vec_row["):
                    continue
                name = call.split("[")[0]
                if tag == "no_entries":
                    assert kernel[call] == SCALE_ONLY, (where, call, kernel[call])  # dispatch.cpp:979-982
                elif name in ANY_KERNEL:
                    assert kernel[call] >= 0, (where, call, kernel[call])
                else:
                    assert kernel[call] in EXPECTED_KERNEL[name], (where, call, kernel[call])
    assert set(EXPECTED_KERNEL) | set(ANY_KERNEL) | {"adaptive_vec_row"} == {c.split("[")[0] for c in T.CALLS}


def test_trans_is_reported_by_every_entry_and_not_applied(oracle, surface, inputs):
    """trans = 1: every entry, adaptive_vec_row_sparse_spmv included, leaves SPMV_ACC_ERR_UNSUPPORTED_TRANS and the non-transposed product."""
    alpha, beta = T.TRANS_PAIR
    checked = []
    _check_call(oracle, surface, inputs, T.TRANS_CASE, "trans", alpha, beta, checked)
    assert checked == T.CALLS
    silent = {call: surface[(T.TRANS_CASE, "trans", call)][1] for call in T.CALLS if surface[(T.TRANS_CASE, "trans", call)][1] != UNSUPPORTED_TRANS}
    assert not silent, silent


@pytest.fixture(scope="module")
def torch_dev(hiplib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.mark.parametrize("tile_form", [1, 0])
def test_split_forms_through_the_c_abi(torch_dev, oracle, hiplib, inputs, tile_form):
    """`adaptive` under adaptive_timed = 0, adaptive_split = 1 on the split cases: the two-width launch of vector_tile_kernel (vector_tile = 1) or
    vector_row_kernel (vector_tile = 0).  y passes check, the plan says branch 1 and names the kernel that ran, and the out-of-place entry gives
    the in-place bits on the same settled plan."""
    torch = torch_dev
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    want_kernel = "vector_tile" if tile_form else "vector_row"
    try:
        for name, value in (("adaptive_timed", 0), ("adaptive_split", 1), ("vector_tile", tile_form)):
            assert hiplib.spmv_acc_set_tunable(name.encode(), value) == 0
        for tag in T.SPLIT_CASES:
            rowptr, cols, vals, x, y0 = inputs[tag]
            m, n, nnz = rowptr.size - 1, x.size, int(rowptr[-1])
            drp, dci, dv, dx = dev(rowptr), dev(cols), dev(vals), dev(x)
            try:
                for alpha, beta in T.ALPHA_BETA:
                    y_dev = y0 if beta != 0.0 else np.full(m, np.nan)  # beta == 0 never reads y
                    y_ref = y0 if beta != 0.0 else np.zeros(m)
                    runs = []
                    for _ in range(3):  # the first call of a (strategy, beta class) may be served by the plan's rule twin; nothing is timed on this path
                        dy = dev(y_dev)
                        spmv_acc_amd.csr_spmv(alpha, beta, m, n, nnz, drp, dci, dv, dx, dy, strategy="adaptive", h_rowptr=rowptr)
                        torch.cuda.synchronize()
                        runs.append(dy.cpu().numpy())
                        info = spmv_acc_amd.query_plan(drp, m)
                        assert info["adaptive_branch"] == 1 and info["last_kernel"] == want_kernel, (tag, alpha, beta, info)
                    assert info["settled"], (tag, alpha, beta, info)
                    for got in runs:
                        assert not np.isnan(got).any(), (tag, alpha, beta)
                        check(oracle, got, alpha, beta, rowptr, cols, vals, x, y_ref, ("split", tile_form, tag, alpha, beta))
                    if alpha == 0.0:
                        assert np.array_equal(runs[-1], beta * y0), (tag, "alpha = 0 must give exactly beta * y0")
                    d_in, d_out = dev(y_dev), torch.full((m,), float("nan"), dtype=torch.float64, device="cuda")
                    spmv_acc_amd.csr_spmv(alpha, beta, m, n, nnz, drp, dci, dv, dx, d_out, strategy="adaptive", h_rowptr=rowptr, y_in=d_in)
                    torch.cuda.synchronize()
                    assert np.array_equal(d_out.cpu().numpy(), runs[-1]), (tag, alpha, beta, "out of place differs from in place")
                    assert np.array_equal(d_in.cpu().numpy(), y_dev, equal_nan=True), (tag, alpha, beta, "y_in was written")
                    assert spmv_acc_amd.query_plan(drp, m)["last_kernel"] == want_kernel
            finally:
                spmv_acc_amd.release_plans(drp)
    finally:
        hiplib.spmv_acc_reset_tunables()
