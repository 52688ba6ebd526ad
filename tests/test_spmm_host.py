"""CPU side of the CSR SpMM entry (no GPU): the C ABI declares and exports it, the Python wrapper refuses bad arguments before any launch,
the compiled kernels fit their register budget, and every size-selected branch of the SpMM code names the GPU tests that cross it."""
import os
import re
import subprocess
import sys

import pytest

import spmv_acc_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "spmv_acc_amd/csrc/"

# (rule, file, regex that must match the source, GPU tests of tests/test_gpu_spmm.py that cross it at test size, what it selects)
SPMM_SIZE_RULES = [
    ("kSpmmPanel", CSRC + "spmm.hpp", r"constexpr int kSpmmPanel = 32;",
     ["test_spmm_parity", "test_spmm_unrebased_row_range", "test_spmm_grid_stride_at_test_size"],
     "k > 32: one pass over the matrix per panel of 32 columns, the last one narrower (k = 33, 64 in the parity test)"),
    ("team width (spmm_team_lanes)", CSRC + "k_spmm.hip", r"while \(2 \* ts < kp && ts < kSpmmTeamMax\) ts <<= 1;",
     ["test_spmm_parity", "test_spmm_bitwise_invariants"], "row-major: 1, 2, 4, 8 or 16 lanes per row from the panel width"),
    ("kp == 1 (8-B gathers)", CSRC + "k_spmm.hip", r"if \(kp == 1\) launch_rows<1, true>",
     ["test_spmm_contract", "test_spmm_parity"], "row-major panel of one column: the SINGLE instance"),
    ("kSpmmLongRow", CSRC + "spmm.hpp", r"constexpr int kSpmmLongRow = 256;",
     ["test_spmm_parity", "test_spmm_unrebased_row_range", "test_spmm_stale_plan_values_edit_and_release"],
     "rows of more non-zeros are cut into pieces + fix-up (hub rows of 257, 3 000 and 120 001 non-zeros)"),
    ("kSpmmPiece", CSRC + "spmm.hpp", r"constexpr int kSpmmPiece = 256;",
     ["test_spmm_parity", "test_spmm_unrebased_row_range"], "non-zeros per piece of a long row (the fix-up adds up to 470 pieces per row)"),
    ("kMaxGridBlocks (grid striding)", CSRC + "structure_passes.hpp", r"const long long cap = max_grid_blocks\(\);",
     ["test_spmm_grid_stride_at_test_size"], "every SpMM kernel strides over the rows beyond max_grid_blocks() workgroups"),
    ("kMaxGridBlocks (grid striding): SpMM's call", CSRC + "k_spmm.hip", r"dim3\(grid_for\(A\.m, kThreads / TS\)\)",
     ["test_spmm_grid_stride_at_test_size"], "the SpMM launchers take the shared grid"),
    ("k == 1 route", CSRC + "spmm.cpp", r"if \(k == 1 && \(!row_major \|\| \(ldx == 1 && ldy == 1\)\)\)",
     ["test_spmm_bitwise_invariants", "test_spmm_contract"], "k = 1 with contiguous vectors: the SpMV path under the active strategy"),
    ("64-bit offsets", CSRC + "k_spmm.hip", r"long long ldx, long long ldy",
     ["test_spmm_offsets_beyond_int32"], "all X / Y offsets are 64-bit (one form only: no 32-bit gather variant)"),
]


def test_spmm_size_rules_name_their_tests():
    gpu_tests = open(os.path.join(ROOT, "tests", "test_gpu_spmm.py")).read()
    defined = set(re.findall(r"^def (test_\w+)\(", gpu_tests, flags=re.M))
    for name, path, pattern, tests, what in SPMM_SIZE_RULES:
        assert re.search(pattern, open(os.path.join(ROOT, path)).read()), f"{name}: no longer matches {path}: {pattern}"
        assert tests and what
        for t in tests:
            assert t in defined, f"{name}: names {t}, which is not a test of tests/test_gpu_spmm.py"


def test_spmm_is_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "spmv_acc.h")).read()
    assert re.search(r"int spmv_acc_csr_spmm\(int layout, int k, double alpha, double beta, int m, int n, int nnz,", header)
    assert "SPMV_ACC_ROW_MAJOR = 0" in header and "SPMV_ACC_COL_MAJOR = 1" in header
    assert "spmv_acc_csr_spmm" in spmv_acc_amd.C_ABI_SYMBOLS
    lib = spmv_acc_amd.load_library()
    assert hasattr(lib, "spmv_acc_csr_spmm")


class _FakeTensor:
    """Enough of a torch tensor for the wrapper's checks to run without a GPU (it never reaches the C entry)."""

    def __init__(self, shape, strides, dtype="torch.float64", cuda=True, device="cuda:0"):
        self.shape, self._strides, self.dtype, self.is_cuda, self.device = tuple(shape), tuple(strides), dtype, cuda, device

    def stride(self):
        return self._strides

    def dim(self):
        return len(self.shape)

    def data_ptr(self):
        raise AssertionError("the wrapper must refuse before it takes a pointer")


def _refused(X, Y, m=10, n=12, match=None):
    with pytest.raises(spmv_acc_amd.SpmvAccError, match=match):
        spmv_acc_amd.csr_spmm(1.0, 1.0, m, n, 5, None, None, None, X, Y)


def test_spmm_wrapper_refuses_bad_arguments():
    ok_x, ok_y = _FakeTensor((12, 4), (4, 1)), _FakeTensor((10, 4), (4, 1))
    _refused(_FakeTensor((12, 4), (4, 1), cuda=False), ok_y, match="not on the GPU")
    _refused(ok_x, _FakeTensor((10, 4), (4, 1), dtype="torch.float32"), match="dtype")
    _refused(_FakeTensor((12, 4), (2, 1)), ok_y, match="neither row-major")  # ld < k
    _refused(ok_x, _FakeTensor((10, 4), (8, 2)), match="neither row-major")  # no unit stride
    _refused(_FakeTensor((12, 4), (1, 11)), ok_y, match="neither row-major")  # column-major with ld < n
    _refused(_FakeTensor((11, 4), (4, 1)), ok_y, match="shape")  # X rows != n
    _refused(ok_x, _FakeTensor((9, 4), (4, 1)), match="shape")  # Y rows != m
    _refused(ok_x, _FakeTensor((10, 3), (3, 1)), match="columns")  # k mismatch
    _refused(ok_x, _FakeTensor((10, 4), (1, 10)), match="one layout")  # row-major X, column-major Y
    _refused([[0.0]], ok_y, match="torch tensor")


def test_spmm_kernel_instances_fit_eight_waves_per_simd(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_table

    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-DKERNEL_STRATEGY_ADAPTIVE",
                        "-I" + os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-S",
                        os.path.join(ROOT, CSRC, "k_spmm.hip"), "-o", str(tmp_path / "k_spmm.s")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [k for k in resource_table.parse(r.stderr) if k["name"].startswith("spmm_")]
    assert len([k for k in rows if k["name"].startswith("spmm_rows_kernel<")]) >= 5, rows
    for k in rows:
        assert k["scratch"] == 0 and k["agprs"] == 0, k
        if k["name"].startswith("spmm_rows_kernel<"):
            assert k["vgprs"] <= 64 and k["occupancy"] >= 8, k
