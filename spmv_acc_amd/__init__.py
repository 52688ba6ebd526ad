"""spmv_acc_amd -- Python plumbing over the C ABI of libspmv_acc.so (include/spmv_acc.h).

The product is the HIP library; this module only loads it with ctypes and passes raw device
pointers (``tensor.data_ptr()``).  There is no CPU fallback: every compute entry point raises if the
library is missing.  (The CPU oracle lives under ``oracle/`` and is test infrastructure only.)

Reference interface mirrored (names and argument meaning): ``sparse_spmv`` (src/acc/api/spmv.h:27-28),
``sparse_csr_spmv`` (api/spmv.h:20-21) and the KERNEL_STRATEGY names (src/configure.cmake:17-40).
"""
from __future__ import annotations

import ctypes
import math
import os
from typing import Optional, Sequence

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libspmv_acc.so")

STRATEGIES = (
    "default", "adaptive", "thread_row", "wf_row", "block_row_ordinary", "light",
    "vector_row", "line_enhance", "line", "flat", "adaptive_plus",
)
# the strategies BASELINE.json's north_star names (+ the row-block preprocessing entry)
HOT_STRATEGIES = ("default", "adaptive", "flat", "line_enhance", "line", "vector_row", "adaptive_plus")

_c_int_p = ctypes.POINTER(ctypes.c_int)
_c_double_p = ctypes.POINTER(ctypes.c_double)

# every symbol include/spmv_acc.h declares (tests check the library exports all of them)
C_ABI_SYMBOLS = (
    "sparse_spmv", "spmv_acc_csr_spmv", "spmv_acc_csr_spmv_strategy", "spmv_acc_set_strategy",
    "spmv_acc_set_strategy_id", "spmv_acc_get_strategy", "spmv_acc_strategy_name", "spmv_acc_parse_strategy",
    "spmv_acc_break_points", "spmv_acc_break_points_len", "spmv_acc_adaptive_plus_analyze",
    "spmv_acc_adaptive_plus_vec", "spmv_acc_adaptive_branch", "spmv_acc_partition_rows", "spmv_acc_stage_csr",
    "spmv_acc_free_device", "spmv_acc_release_plans", "spmv_acc_cached_plans", "spmv_acc_query_plan",
    "spmv_acc_set_stream", "spmv_acc_get_stream", "spmv_acc_last_error", "spmv_acc_last_error_string",
    "spmv_acc_clear_error", "spmv_acc_time_spmv", "spmv_acc_version", "spmv_acc_set_tunable",
    "spmv_acc_get_tunable", "spmv_acc_reset_tunables", "spmv_acc_time_spmv_total", "spmv_acc_copy_ceiling_gbs", "spmv_acc_adaptive_plus_analyze_device", "spmv_acc_prepare",
    "spmv_acc_last_prepare_us", "spmv_acc_sharded_spmv", "spmv_acc_shard_prepare", "spmv_acc_csr_spmv_chunks", "spmv_acc_query_plan_settled", "spmv_acc_query_plan_col16", "spmv_acc_query_plan_col_bits", "spmv_acc_time_spmv_cold", "spmv_acc_csr_spmv_oop", "spmv_acc_check_plans",
    "spmv_acc_query_plan_beta0", "spmv_acc_query_plan_slab_passes", "spmv_acc_shard_create", "spmv_acc_shard_step", "spmv_acc_shard_pipeline",
    "spmv_acc_shard_destroy", "spmv_acc_rccl_comm_init_all", "spmv_acc_rccl_comm_destroy", "spmv_acc_set_tune_cache",
    "spmv_acc_prepare_beta", "spmv_acc_time_spmv_events", "spmv_acc_refresh_values", "spmv_acc_time_spmv_region", "spmv_acc_query_plan_last_kernel", "spmv_acc_time_spmv_kernels",
    "spmv_acc_csr_spmm", "spmv_acc_csr_transpose", "spmv_acc_csr_transpose_values", "spmv_acc_csr_spmv_t",
    "spmv_acc_coo_to_csr", "spmv_acc_coo_to_csr_values",
    "spmv_acc_csr_spgemm_products", "spmv_acc_csr_spgemm", "spmv_acc_csr_spgemm_values",
    "spmv_acc_csr_add", "spmv_acc_csr_add_values",
    "spmv_acc_csr_extract", "spmv_acc_csr_extract_values",
    "spmv_acc_csr_color", "spmv_acc_csr_gs_sweep",
    "spmv_acc_csr_jacobi_diagonal", "spmv_acc_csr_jacobi_sweep",
    "spmv_acc_csr_aggregate", "spmv_acc_csr_tentative_values",
    "spmv_acc_csr_strength", "spmv_acc_csr_strength_values",
    "spmv_acc_csr_dense_inverse", "spmv_acc_dense_apply",
    "spmv_acc_cg_partials", "spmv_acc_cg_start", "spmv_acc_cg_update", "spmv_acc_cg_direction",
)

_lib = None


class SpmvAccError(RuntimeError):
    pass


def load_library(path: Optional[str] = None) -> ctypes.CDLL:
    """Load libspmv_acc.so (built by ``__graft_entry__.build()`` / ``make -C spmv_acc_amd/csrc``)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise SpmvAccError(
            f"{p} not found: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C spmv_acc_amd/csrc`. There is no CPU fallback."
        )
    # One HIP runtime per process: torch wheels bundle their own libamdhip64.so.7 / libhsa-runtime64 and
    # initialise it for device memory.  If libspmv_acc.so were loaded first, its NEEDED libamdhip64.so.7 would
    # bring in /opt/rocm's copy, and the second runtime to initialise finds no device.  Importing torch first
    # makes the soname resolve to the runtime torch already loaded (kernels + tensors then share one context).
    try:
        import torch  # noqa: F401
    except ImportError:  # C/C++ consumers link the library directly; Python without torch still works
        pass
    lib = ctypes.CDLL(p)
    vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.sparse_spmv.argtypes = [ci, cd, cd, ci, ci, vp, vp, vp, vp, vp]
    lib.sparse_spmv.restype = None
    lib.spmv_acc_csr_spmv.argtypes = [ci, cd, cd, ci, ci, ci, vp, vp, vp, vp, vp, vp]
    lib.spmv_acc_csr_spmv.restype = None
    lib.spmv_acc_csr_spmv_strategy.argtypes = [ci, ci, cd, cd, ci, ci, ci, vp, vp, vp, vp, vp, vp]
    lib.spmv_acc_csr_spmv_strategy.restype = None
    lib.spmv_acc_set_strategy.argtypes = [ctypes.c_char_p]
    lib.spmv_acc_set_strategy_id.argtypes = [ci]
    lib.spmv_acc_strategy_name.argtypes = [ci]
    lib.spmv_acc_strategy_name.restype = ctypes.c_char_p
    lib.spmv_acc_parse_strategy.argtypes = [ctypes.c_char_p]
    lib.spmv_acc_break_points.argtypes = [vp, ci, ci, ci, vp, ci]
    lib.spmv_acc_break_points_len.argtypes = [ci, ci]
    lib.spmv_acc_adaptive_plus_analyze.argtypes = [ci, ci, ci, ci, vp, vp, ci, vp]
    lib.spmv_acc_adaptive_plus_vec.argtypes = [ci, ci]
    lib.spmv_acc_adaptive_plus_analyze_device.argtypes = [ci, ci, ci, ci, vp, vp, ci, vp]
    lib.spmv_acc_adaptive_branch.argtypes = [ci, ci, ci, ci, ci]
    lib.spmv_acc_partition_rows.argtypes = [ci, ci, ci, vp, vp]
    lib.spmv_acc_stage_csr.argtypes = [ci, ci, ci, vp, vp, vp, vp, vp] + [ctypes.POINTER(vp)] * 5
    lib.spmv_acc_free_device.argtypes = [vp]
    lib.spmv_acc_prepare.argtypes = [ci, ci, ci, ci, vp, vp, vp, vp, vp, ctypes.POINTER(ctypes.c_float)]
    lib.spmv_acc_release_plans.argtypes = [vp]
    lib.spmv_acc_release_plans.restype = None
    lib.spmv_acc_query_plan.argtypes = [vp, ci, vp]
    lib.spmv_acc_set_stream.argtypes = [vp]
    lib.spmv_acc_set_stream.restype = None
    lib.spmv_acc_get_stream.restype = vp
    lib.spmv_acc_last_error_string.restype = ctypes.c_char_p
    lib.spmv_acc_clear_error.restype = None
    lib.spmv_acc_time_spmv.argtypes = [ci, ci, cd, cd, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.spmv_acc_time_spmv_events.argtypes = [ci, ci, cd, cd, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, ctypes.c_uint]
    lib.spmv_acc_time_spmv_cold.argtypes = [ci, ci, cd, cd, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, ctypes.c_longlong, vp]
    lib.spmv_acc_version.restype = ctypes.c_char_p
    lib.spmv_acc_set_tunable.argtypes = [ctypes.c_char_p, ci]
    lib.spmv_acc_get_tunable.argtypes = [ctypes.c_char_p]
    lib.spmv_acc_reset_tunables.restype = None
    lib.spmv_acc_time_spmv_total.argtypes = [ci, ci, cd, cd, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp]
    lib.spmv_acc_time_spmv_kernels.argtypes = [ci, ci, cd, cd, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.spmv_acc_time_spmv_region.argtypes = [ci, ci, cd, cd, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp]
    lib.spmv_acc_copy_ceiling_gbs.argtypes = [vp, vp, ctypes.c_longlong, ci]
    lib.spmv_acc_copy_ceiling_gbs.restype = cd
    lib.spmv_acc_last_prepare_us.restype = cd
    lib.spmv_acc_sharded_spmv.argtypes = [vp, ci, cd, cd, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp]
    lib.spmv_acc_csr_spmv_oop.argtypes = [ci, ci, cd, cd, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp]
    lib.spmv_acc_csr_spmv_oop.restype = None
    lib.spmv_acc_query_plan_beta0.argtypes = [vp, ci]
    lib.spmv_acc_query_plan_slab_passes.argtypes = [vp, ci]
    lib.spmv_acc_query_plan_settled.argtypes = [vp, ci]
    lib.spmv_acc_query_plan_col16.argtypes = [vp, ci]
    lib.spmv_acc_query_plan_col_bits.argtypes = [vp, ci]
    lib.spmv_acc_query_plan_last_kernel.argtypes = [vp, ci]
    lib.spmv_acc_shard_create.argtypes = [ctypes.POINTER(vp), vp, ci, ci, ci, ci, ci, vp, vp, vp, ci]
    lib.spmv_acc_shard_step.argtypes = [vp, cd, cd, vp, vp, vp]
    lib.spmv_acc_shard_pipeline.argtypes = [vp]
    lib.spmv_acc_shard_destroy.argtypes = [vp]
    lib.spmv_acc_rccl_comm_init_all.argtypes = [ctypes.POINTER(vp), ci, vp]
    lib.spmv_acc_rccl_comm_destroy.argtypes = [vp]
    lib.spmv_acc_set_tune_cache.argtypes = [ctypes.c_char_p]
    lib.spmv_acc_set_tune_cache.restype = None
    lib.spmv_acc_refresh_values.argtypes = [vp]
    lib.spmv_acc_prepare_beta.argtypes = [ci, cd, ci, ci, ci, vp, vp, vp, vp, vp, ctypes.POINTER(ctypes.c_float)]
    lib.spmv_acc_shard_prepare.argtypes = [vp, cd, vp]
    lib.spmv_acc_csr_spmv_chunks.argtypes = [ci, cd, cd, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    ll = ctypes.c_longlong
    lib.spmv_acc_csr_spmm.argtypes = [ci, ci, cd, cd, ci, ci, ci, vp, vp, vp, vp, vp, ll, vp, ll]
    lib.spmv_acc_csr_spmm.restype = ci
    lib.spmv_acc_csr_transpose.argtypes = [ci, ci, ci, vp, vp, vp, vp, vp, vp, vp]
    lib.spmv_acc_csr_transpose.restype = ci
    lib.spmv_acc_csr_transpose_values.argtypes = [ci, vp, vp, vp]
    lib.spmv_acc_csr_transpose_values.restype = ci
    lib.spmv_acc_csr_spmv_t.argtypes = [cd, cd, ci, ci, ci, vp, vp, vp, vp, vp]
    lib.spmv_acc_csr_spmv_t.restype = ci
    lib.spmv_acc_coo_to_csr.argtypes = [ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, _c_int_p]
    lib.spmv_acc_coo_to_csr.restype = ci
    lib.spmv_acc_coo_to_csr_values.argtypes = [ci, ci, vp, vp, vp, vp]
    lib.spmv_acc_coo_to_csr_values.restype = ci
    lib.spmv_acc_csr_spgemm_products.argtypes = [ci, ci, ci, vp, vp, vp, ctypes.POINTER(ctypes.c_longlong)]
    lib.spmv_acc_csr_spgemm_products.restype = ci
    lib.spmv_acc_csr_spgemm.argtypes = [ci, ci, ci, ci, vp, vp, vp, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, _c_int_p]
    lib.spmv_acc_csr_spgemm.restype = ci
    lib.spmv_acc_csr_spgemm_values.argtypes = [ci, ci, vp, vp, vp, vp, vp, vp]
    lib.spmv_acc_csr_spgemm_values.restype = ci
    lib.spmv_acc_csr_add.argtypes = [ci, ci, ci, vp, vp, ci, vp, vp, ctypes.c_double, vp, ctypes.c_double, vp, vp, vp, vp, vp, vp, _c_int_p]
    lib.spmv_acc_csr_add.restype = ci
    lib.spmv_acc_csr_add_values.argtypes = [ci, ci, ci, vp, vp, ctypes.c_double, vp, ctypes.c_double, vp, vp]
    lib.spmv_acc_csr_add_values.restype = ci
    lib.spmv_acc_csr_extract.argtypes = [ci, ci, ci, vp, vp, vp, ci, vp, ci, vp, ci, ci, vp, vp, vp, vp, _c_int_p]
    lib.spmv_acc_csr_extract.restype = ci
    lib.spmv_acc_csr_extract_values.argtypes = [ci, ci, vp, vp, vp]
    lib.spmv_acc_csr_extract_values.restype = ci
    lib.spmv_acc_csr_color.argtypes = [ci, ci, vp, vp, vp, vp, ci, _c_int_p, _c_int_p, _c_int_p]
    lib.spmv_acc_csr_color.restype = ci
    lib.spmv_acc_csr_gs_sweep.argtypes = [ci, ci, vp, vp, vp, ci, _c_int_p, vp, cd, ci, vp, vp]
    lib.spmv_acc_csr_gs_sweep.restype = ci
    lib.spmv_acc_csr_jacobi_diagonal.argtypes = [ci, ci, vp, vp, vp, ci, vp, vp]
    lib.spmv_acc_csr_jacobi_diagonal.restype = ci
    lib.spmv_acc_csr_jacobi_sweep.argtypes = [ci, ci, vp, vp, vp, vp, cd, vp, vp, vp, vp]
    lib.spmv_acc_csr_jacobi_sweep.restype = ci
    lib.spmv_acc_csr_aggregate.argtypes = [ci, ci, vp, vp, vp, vp, vp, _c_int_p]
    lib.spmv_acc_csr_aggregate.restype = ci
    lib.spmv_acc_csr_tentative_values.argtypes = [ci, ci, vp, vp, vp, vp, vp, vp, vp]
    lib.spmv_acc_csr_tentative_values.restype = ci
    lib.spmv_acc_csr_strength.argtypes = [ci, ci, vp, vp, vp, cd, vp, vp, vp, vp, _c_int_p, _c_int_p]
    lib.spmv_acc_csr_strength.restype = ci
    lib.spmv_acc_csr_strength_values.argtypes = [ci, ci, ci, vp, vp, vp, vp, vp, cd, vp, vp]
    lib.spmv_acc_csr_strength_values.restype = ci
    lib.spmv_acc_csr_dense_inverse.argtypes = [ci, ci, vp, vp, vp, vp, _c_int_p]
    lib.spmv_acc_csr_dense_inverse.restype = ci
    lib.spmv_acc_dense_apply.argtypes = [ci, vp, vp, vp]
    lib.spmv_acc_dense_apply.restype = ci
    lib.spmv_acc_cg_partials.argtypes = [ci, ctypes.POINTER(ctypes.c_size_t)]
    lib.spmv_acc_cg_partials.restype = ci
    lib.spmv_acc_cg_start.argtypes = [ci, cd, vp, vp, vp, vp, vp, vp, vp, ci]
    lib.spmv_acc_cg_start.restype = ci
    lib.spmv_acc_cg_update.argtypes = [ci, vp, vp, vp, vp, vp, vp, vp, ci]
    lib.spmv_acc_cg_update.restype = ci
    lib.spmv_acc_cg_direction.argtypes = [ci, vp, vp, vp, vp, vp, vp]
    lib.spmv_acc_cg_direction.restype = ci
    if path is None:
        _lib = lib
    return lib


def strategy_id(name_or_id) -> int:
    if isinstance(name_or_id, int):
        return name_or_id
    s = load_library().spmv_acc_parse_strategy(str(name_or_id).encode())
    if s < 0:
        raise SpmvAccError(f"unknown KERNEL_STRATEGY {name_or_id!r}")
    return s


def _check(lib) -> None:
    code = lib.spmv_acc_last_error()
    if code not in (0, 1):  # 1 = unsupported trans: reported, not fatal (reference ignores trans)
        msg = lib.spmv_acc_last_error_string().decode()
        lib.spmv_acc_clear_error()
        raise SpmvAccError(f"spmv_acc error {code}: {msg}")


def _ptr(t) -> int:
    """Raw pointer of a torch tensor / numpy array / int (0 for None)."""
    if t is None:
        return 0
    if isinstance(t, int):
        return t
    if hasattr(t, "data_ptr"):
        return t.data_ptr()
    return t.ctypes.data


def _require_cuda(*tensors) -> None:
    for t in tensors:
        if t is not None and hasattr(t, "is_cuda") and not t.is_cuda:
            raise SpmvAccError("device pointers required: tensor is not on the GPU (no CPU fallback)")


def _require(lib, **named) -> None:
    """Torch tensors handed to the C ABI are passed as raw pointers, so what the kernels assume is checked here: on the GPU,
    all on one device, contiguous, int32 indices / float64 values, and at least as many elements as the shape says.
    name -> (tensor, "i32" | "f64", minimum element count); raw integer pointers and None pass through unchecked.
    Also points the library stream at torch's current stream on that device, so the launches are ordered with the caller's
    other torch work (the default stream is HIP's NULL stream, the reference's behaviour)."""
    device = None
    for name, (t, kind, count) in named.items():
        if t is None or not hasattr(t, "is_cuda"):
            continue
        if not t.is_cuda:
            raise SpmvAccError(f"{name}: device pointers required, tensor is not on the GPU (no CPU fallback)")
        want = "torch.int32" if kind == "i32" else "torch.float64"
        if str(t.dtype) != want:
            raise SpmvAccError(f"{name}: dtype {t.dtype}, the library reads {want} (int32 indices, fp64 values)")
        if not t.is_contiguous():
            raise SpmvAccError(f"{name}: tensor is not contiguous")
        if t.numel() < count:
            raise SpmvAccError(f"{name}: {t.numel()} elements, the shape needs at least {count}")
        if device is None:
            device = t.device
        elif t.device != device:
            raise SpmvAccError(f"{name}: on {t.device}, other arguments on {device}")
    if device is not None:
        import torch

        lib.spmv_acc_set_stream(torch.cuda.current_stream(device).cuda_stream)


def _csr_args(lib, m, n, nnz, rowptr, colindex, value, x, y=None, y0=None) -> None:
    k = max(nnz, 0)
    _require(lib, rowptr=(rowptr, "i32", m + 1), colindex=(colindex, "i32", k), value=(value, "f64", k),
             x=(x, "f64", n), y=(y, "f64", m), y0=(y0, "f64", m))


def sparse_spmv(trans: int, alpha: float, beta: float, m: int, n: int, rowptr, colindex, value, x, y) -> None:
    """Ten-argument entry with the active strategy; all tensors on the GPU; y updated in place (async)."""
    lib = load_library()
    _csr_args(lib, m, n, -1, rowptr, colindex, value, x, y)
    lib.sparse_spmv(trans, alpha, beta, m, n, _ptr(rowptr), _ptr(colindex), _ptr(value), _ptr(x), _ptr(y))
    _check(lib)


def csr_spmv(alpha: float, beta: float, m: int, n: int, nnz: int, rowptr, colindex, value, x, y,
             strategy=None, h_rowptr=None, trans: int = 0, y_in=None) -> None:
    """Descriptor entry (sparse_csr_spmv flattened).  ``h_rowptr``: optional host (numpy int32) rowptr.
    ``y_in``: out-of-place form, y = alpha*A*x + beta*y_in (spmv_acc_csr_spmv_oop); None = in place."""
    lib = load_library()
    _csr_args(lib, m, n, nnz, rowptr, colindex, value, x, y, y_in)
    if y_in is not None:
        lib.spmv_acc_csr_spmv_oop(-1 if strategy is None else strategy_id(strategy), trans, alpha, beta, m, n, nnz,
                                  _ptr(h_rowptr), _ptr(rowptr), _ptr(colindex), _ptr(value), _ptr(x), _ptr(y_in), _ptr(y))
        _check(lib)
        return
    args = (trans, alpha, beta, m, n, nnz, _ptr(h_rowptr), _ptr(rowptr), _ptr(colindex), _ptr(value), _ptr(x), _ptr(y))
    if strategy is None:
        lib.spmv_acc_csr_spmv(*args)
    else:
        lib.spmv_acc_csr_spmv_strategy(strategy_id(strategy), *args)
    _check(lib)


SPMM_ROW_MAJOR, SPMM_COL_MAJOR = 0, 1  # enum spmv_acc_layout


def _spmm_layouts(name, t, rows: int, k: int):
    """The layouts (with their leading dimension) an (rows, k) view can be passed as: {layout: ld}."""
    s0, s1 = t.stride()
    out = {}
    if (s1 == 1 or k <= 1) and s0 >= max(k, 1):
        out[SPMM_ROW_MAJOR] = s0
    if (s0 == 1 or rows <= 1) and s1 >= max(rows, 1):
        out[SPMM_COL_MAJOR] = s1
    if not out and rows > 0 and k > 0:
        raise SpmvAccError(f"{name}: strides {tuple(t.stride())} of a ({rows}, {k}) view are neither row-major (unit stride on dim 1, "
                           f"leading dimension >= k) nor column-major (unit stride on dim 0, leading dimension >= {rows})")
    return out


def csr_spmm(alpha: float, beta: float, m: int, n: int, nnz: int, rowptr, colindex, value, X, Y, h_rowptr=None) -> None:
    """Y = alpha*A*X + beta*Y for the k columns of X (spmv_acc_csr_spmm, async on torch's current stream).  X: (n, k) float64 GPU tensor,
    Y: (m, k); both row-major (unit stride on dim 1) or both column-major (unit stride on dim 0), views with a larger leading dimension
    included.  The layout and leading dimensions are read from the strides; any other stride pattern is refused."""
    lib = load_library()
    for name, t, rows in (("X", X, n), ("Y", Y, m)):
        if not hasattr(t, "is_cuda") or not hasattr(t, "stride"):
            raise SpmvAccError(f"{name}: a torch tensor on the GPU is required")
        if not t.is_cuda:
            raise SpmvAccError(f"{name}: device pointers required, tensor is not on the GPU (no CPU fallback)")
        if str(t.dtype) != "torch.float64":
            raise SpmvAccError(f"{name}: dtype {t.dtype}, the library reads torch.float64")
        if t.dim() != 2 or t.shape[0] != rows:
            raise SpmvAccError(f"{name}: shape {tuple(t.shape)}, expected ({rows}, k)")
    if X.shape[1] != Y.shape[1]:
        raise SpmvAccError(f"X has {X.shape[1]} columns, Y has {Y.shape[1]}")
    if X.device != Y.device:
        raise SpmvAccError(f"Y: on {Y.device}, X on {X.device}")
    k = int(X.shape[1])
    lx, ly = _spmm_layouts("X", X, n, k), _spmm_layouts("Y", Y, m, k)
    if not lx or not ly:  # (an empty view: nothing is computed, any consistent arguments do)
        layout, ldx, ldy = SPMM_ROW_MAJOR, k, k
    else:
        both = [lay for lay in (SPMM_ROW_MAJOR, SPMM_COL_MAJOR) if lay in lx and lay in ly]
        if not both:
            raise SpmvAccError("X and Y must share one layout (both row-major or both column-major)")
        layout = both[0]
        ldx, ldy = lx[layout], ly[layout]
    _require(lib, rowptr=(rowptr, "i32", m + 1), colindex=(colindex, "i32", max(nnz, 0)), value=(value, "f64", max(nnz, 0)))
    if hasattr(rowptr, "device") and rowptr.device != X.device:
        raise SpmvAccError(f"X: on {X.device}, rowptr on {rowptr.device}")
    lib.spmv_acc_set_stream(__import__("torch").cuda.current_stream(X.device).cuda_stream)
    lib.spmv_acc_csr_spmm(layout, k, alpha, beta, m, n, nnz, _ptr(h_rowptr), _ptr(rowptr), _ptr(colindex), _ptr(value), _ptr(X), ldx,
                          _ptr(Y), ldy)
    _check(lib)


def _require_tensors(**named) -> None:
    """The transposed entries take torch tensors only (they write through raw pointers and, for csr_transpose, allocate beside them)."""
    for name, t in named.items():
        if t is None or not hasattr(t, "is_cuda") or not hasattr(t, "data_ptr"):
            raise SpmvAccError(f"{name}: a torch tensor on the GPU is required")


def csr_spmv_t(alpha: float, beta: float, m: int, n: int, nnz: int, rowptr, colindex, value, x, y) -> None:
    """y = alpha*A^T*x + beta*y straight from the caller's CSR (spmv_acc_csr_spmv_t, async on torch's current stream): x holds m
    entries, y holds n.  Stateless (no plan) and capturable from its first call; adds with fp64 atomics, so the last bits of y depend on
    arrival order -- refused under tunable deterministic = 1 (transpose once with csr_transpose instead).  rowptr may be an un-rebased
    row sub-range with nnz = its END offset.  x and y must not overlap."""
    lib = load_library()
    if m < 0 or n < 0:
        raise SpmvAccError(f"negative shape ({m}, {n})")
    _require_tensors(rowptr=rowptr, colindex=colindex, value=value, x=x, y=y)
    k = max(nnz, 0)
    _require(lib, rowptr=(rowptr, "i32", m + 1), colindex=(colindex, "i32", k), value=(value, "f64", k), x=(x, "f64", m), y=(y, "f64", n))
    rc = lib.spmv_acc_csr_spmv_t(alpha, beta, m, n, nnz, _ptr(rowptr), _ptr(colindex), _ptr(value), _ptr(x), _ptr(y))
    if rc != 0:
        _check(lib)
        raise SpmvAccError(f"csr_spmv_t failed ({rc})")


def csr_transpose(m: int, n: int, nnz: int, rowptr, colindex, value=None, want_perm: bool = False):
    """Stable device transpose (spmv_acc_csr_transpose): returns new GPU tensors (t_rowptr, t_colindex, t_value | None[, perm]) holding the
    CSR of A^T -- an n x m matrix any entry of this module runs on.  Inside a column the entries keep their source order, so the result is
    bit for bit a host stable argsort of colindex.  value=None: structure only.  perm[p] = source position of output entry p (for
    csr_transpose_values).  nnz < 0: read from rowptr[m].  Synchronises; not capturable."""
    import torch

    lib = load_library()
    if m < 0 or n < 0:
        raise SpmvAccError(f"negative shape ({m}, {n})")
    _require_tensors(rowptr=rowptr, colindex=colindex)
    if value is not None:
        _require_tensors(value=value)
    if nnz < 0:
        _require(lib, rowptr=(rowptr, "i32", m + 1))
        nnz = int(rowptr[m].item()) if m > 0 else 0
        if nnz < 0:
            raise SpmvAccError(f"rowptr[m] = {nnz}")
    _require(lib, rowptr=(rowptr, "i32", m + 1), colindex=(colindex, "i32", nnz), value=(value, "f64", nnz))
    dev = rowptr.device
    t_rowptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
    t_colindex = torch.empty(nnz, dtype=torch.int32, device=dev)
    t_value = None if value is None else torch.empty(nnz, dtype=torch.float64, device=dev)
    perm = torch.empty(nnz, dtype=torch.int32, device=dev) if want_perm else None
    rc = lib.spmv_acc_csr_transpose(m, n, nnz, _ptr(rowptr), _ptr(colindex), _ptr(value), _ptr(t_rowptr), _ptr(t_colindex), _ptr(t_value),
                                    _ptr(perm))
    if rc != 0:
        _check(lib)
        raise SpmvAccError(f"csr_transpose failed ({rc})")
    return (t_rowptr, t_colindex, t_value, perm) if want_perm else (t_rowptr, t_colindex, t_value)


def csr_transpose_values(perm, value, out) -> None:
    """out[p] = value[perm[p]] (spmv_acc_csr_transpose_values, async on torch's current stream, capturable): the transposed values after an
    in-place edit of ``value``, with the ``perm`` csr_transpose returned."""
    lib = load_library()
    _require_tensors(perm=perm, value=value, out=out)
    nnz = int(perm.numel())
    _require(lib, perm=(perm, "i32", nnz), value=(value, "f64", nnz), out=(out, "f64", nnz))
    rc = lib.spmv_acc_csr_transpose_values(nnz, _ptr(perm), _ptr(value), _ptr(out))
    if rc != 0:
        _check(lib)
        raise SpmvAccError(f"csr_transpose_values failed ({rc})")


def coo_to_csr(m: int, n: int, row, col, val=None, want_map: bool = False):
    """Device assembly of an m x n CSR from unsorted triples with duplicates (spmv_acc_coo_to_csr): returns new GPU tensors (rowptr, colindex,
    value | None[, order, start]).  Rows sorted by column, duplicates summed in ascending input position (bit for bit a host stable sort and,
    for runs of up to 64 triples, a host loop; longer runs in the wavefront order include/spmv_acc.h documents).  val=None: structure only.
    order / start: the map csr entry j = triples order[start[j] : start[j + 1]], for coo_to_csr_values.  The C entry writes into arrays of
    the upper bound len(row); this wrapper allocates those and returns EXACT-size tensors by cloning the used prefixes (colindex, value:
    nnz; start: nnz + 1; order keeps len(row)), so a matrix with 5 x duplicates does not keep triple-sized arrays alive.  Synchronises; not
    capturable."""
    import torch

    lib = load_library()
    if m < 0 or n < 0:
        raise SpmvAccError(f"negative shape ({m}, {n})")
    _require_tensors(row=row, col=col)
    if val is not None:
        _require_tensors(val=val)
    nnz_coo = int(row.numel())
    if int(col.numel()) > nnz_coo or (val is not None and int(val.numel()) > nnz_coo):  # (fewer: the "elements" check below)
        raise SpmvAccError(f"row holds {nnz_coo} elements, col and val must hold as many")
    _require(lib, row=(row, "i32", nnz_coo), col=(col, "i32", nnz_coo), val=(val, "f64", nnz_coo))
    dev = row.device
    rowptr = torch.empty(m + 1, dtype=torch.int32, device=dev)
    colindex = torch.empty(nnz_coo, dtype=torch.int32, device=dev)
    value = None if val is None else torch.empty(nnz_coo, dtype=torch.float64, device=dev)
    order = torch.empty(nnz_coo, dtype=torch.int32, device=dev) if want_map else None
    start = (torch.empty if nnz_coo else torch.zeros)(nnz_coo + 1, dtype=torch.int32, device=dev) if want_map else None  # (no triples: start = [0])
    h_nnz = ctypes.c_int(0)
    args = (row, col, val, rowptr, colindex, value, order, start) if nnz_coo else (None, None, None, rowptr, None, None, None, None)
    rc = lib.spmv_acc_coo_to_csr(m, n, nnz_coo, *(_ptr(t) for t in args), ctypes.byref(h_nnz))  # (empty tensors have null pointers: not passed)
    if rc != 0:
        _check(lib)
        raise SpmvAccError(f"coo_to_csr failed ({rc})")
    nnz = int(h_nnz.value)
    out = (rowptr, colindex[:nnz].clone(), None if value is None else value[:nnz].clone())
    return out + (order, start[:nnz + 1].clone()) if want_map else out


def coo_to_csr_values(order, start, val, out) -> None:
    """out[j] = sum of val[order[start[j] : start[j + 1]]] (spmv_acc_coo_to_csr_values, async on torch's current stream, capturable): the CSR
    values of new triple values on a known pattern, with the map coo_to_csr(..., want_map=True) returned; len(out) = len(start) - 1 = nnz.
    The same summation orders as coo_to_csr, so the same ``val`` gives the same bits."""
    lib = load_library()
    _require_tensors(order=order, start=start, val=val, out=out)
    nnz_coo, nnz = int(order.numel()), int(start.numel()) - 1
    if nnz < 0:
        raise SpmvAccError("start: 0 elements, the map of an empty matrix still holds one")
    _require(lib, order=(order, "i32", nnz_coo), start=(start, "i32", nnz + 1), val=(val, "f64", nnz_coo), out=(out, "f64", nnz))
    rc = lib.spmv_acc_coo_to_csr_values(nnz_coo, nnz, _ptr(order), _ptr(start), _ptr(val), _ptr(out))
    if rc != 0:
        _check(lib)
        raise SpmvAccError(f"coo_to_csr_values failed ({rc})")


def _spgemm_args(lib, m, k, n, a_rowptr, a_colindex, a_value, b_rowptr, b_colindex, b_value):
    """The checks the two structural SpGEMM wrappers share; returns (nnz_a, nnz_b) = the lengths of the index arrays."""
    if m < 0 or k < 0 or n < 0:
        raise SpmvAccError(f"negative shape ({m}, {k}) * ({k}, {n})")
    _require_tensors(a_rowptr=a_rowptr, a_colindex=a_colindex, b_rowptr=b_rowptr)
    named = dict(a_rowptr=(a_rowptr, "i32", m + 1), a_colindex=(a_colindex, "i32", 0), b_rowptr=(b_rowptr, "i32", k + 1))
    nnz_a, nnz_b = int(a_colindex.numel()), -1
    if b_colindex is not None:
        _require_tensors(b_colindex=b_colindex)
        nnz_b = int(b_colindex.numel())
        named["b_colindex"] = (b_colindex, "i32", 0)
    if (a_value is None) != (b_value is None):
        raise SpmvAccError("a_value and b_value must both be given or both be None (structure only)")
    if a_value is not None:
        _require_tensors(a_value=a_value, b_value=b_value)
        if int(a_value.numel()) > nnz_a or int(b_value.numel()) > nnz_b:  # (fewer: the "elements" check below)
            raise SpmvAccError(f"a_colindex / b_colindex hold {nnz_a} / {nnz_b} elements, a_value / b_value must hold as many")
        named.update(a_value=(a_value, "f64", nnz_a), b_value=(b_value, "f64", nnz_b))
    _require(lib, **named)
    return nnz_a, nnz_b


def csr_spgemm_products(m: int, k: int, a_rowptr, a_colindex, b_rowptr) -> int:
    """The number of scalar products a_ik * b_kj of C = A * B (spmv_acc_csr_spgemm_products): the expansion's size and the upper bound on
    nnz(C).  A is m x k, B is k x n, rebased CSR; len(a_colindex) must be a_rowptr[m] (slice a longer array).  Synchronises; not
    capturable.  Raises SpmvAccError (with the count in its message) when the count is beyond what csr_spgemm takes."""
    lib = load_library()
    nnz_a, _ = _spgemm_args(lib, m, k, 0, a_rowptr, a_colindex, None, b_rowptr, None, None)
    h = ctypes.c_longlong(0)
    rc = lib.spmv_acc_csr_spgemm_products(m, k, nnz_a, _ptr(a_rowptr), _ptr(a_colindex) if nnz_a else 0, _ptr(b_rowptr), ctypes.byref(h))
    if rc != 0:
        _check(lib)
        raise SpmvAccError(f"csr_spgemm_products failed ({rc})")
    return int(h.value)


def csr_spgemm(m: int, k: int, n: int, a_rowptr, a_colindex, a_value, b_rowptr, b_colindex, b_value, want_map: bool = False):
    """Device sparse product C = A * B (spmv_acc_csr_spgemm), A m x k and B k x n in rebased CSR whose rows need not be sorted: returns
    new GPU tensors (rowptr, colindex, value | None[, pa, pb, start]).  Rows of C strictly ascending in column; every value the sum of its
    products a[pa[p]] * b[pb[p]], p in [start[j], start[j + 1]), each rounded before it is added, in the order include/spmv_acc.h
    documents -- a pure function of the inputs, bit for bit.  a_value = b_value = None: structure only.  pa / pb / start: the map for
    csr_spgemm_values.  len(a_colindex) / len(b_colindex) must be a_rowptr[m] / b_rowptr[k].  This wrapper queries the product count,
    allocates arrays of that upper bound and returns EXACT-size tensors by cloning the used prefixes (colindex, value: nnz(C); start:
    nnz(C) + 1; pa and pb keep the product count).  Synchronises; not capturable."""
    import torch

    lib = load_library()
    _require_tensors(b_colindex=b_colindex)
    nnz_a, nnz_b = _spgemm_args(lib, m, k, n, a_rowptr, a_colindex, a_value, b_rowptr, b_colindex, b_value)
    nprod = csr_spgemm_products(m, k, a_rowptr, a_colindex, b_rowptr)
    dev = a_rowptr.device
    rowptr = torch.empty(m + 1, dtype=torch.int32, device=dev)
    colindex = torch.empty(nprod, dtype=torch.int32, device=dev)
    value = None if a_value is None else torch.empty(nprod, dtype=torch.float64, device=dev)
    pa = torch.empty(nprod, dtype=torch.int32, device=dev) if want_map else None
    pb = torch.empty(nprod, dtype=torch.int32, device=dev) if want_map else None
    start = (torch.empty if nprod else torch.zeros)(nprod + 1, dtype=torch.int32, device=dev) if want_map else None  # (no products: start = [0])
    h_nnz = ctypes.c_int(0)
    ins = tuple(_ptr(t) if t is not None and t.numel() and (nprod or i % 2 == 0) else 0  # (empty tensors: null pointers; no products: no values)
                for i, t in enumerate((a_colindex, a_value, b_colindex, b_value)))
    outs = tuple(_ptr(t) if nprod else 0 for t in (colindex, value, pa, pb, start))
    rc = lib.spmv_acc_csr_spgemm(m, k, n, nnz_a, _ptr(a_rowptr), ins[0], ins[1], nnz_b, _ptr(b_rowptr), ins[2], ins[3], nprod, _ptr(rowptr),
                                 *outs, ctypes.byref(h_nnz))
    if rc != 0:
        _check(lib)
        raise SpmvAccError(f"csr_spgemm failed ({rc})")
    nnz = int(h_nnz.value)
    out = (rowptr, colindex[:nnz].clone(), None if value is None else value[:nnz].clone())
    return out + (pa, pb, start[:nnz + 1].clone()) if want_map else out


def csr_spgemm_values(pa, pb, start, a_value, b_value, out) -> None:
    """out[j] = sum of a_value[pa[p]] * b_value[pb[p]] over p in [start[j], start[j + 1]) (spmv_acc_csr_spgemm_values, async on torch's
    current stream, capturable): the values of C for new values of A and / or B on known patterns, with the map csr_spgemm(...,
    want_map=True) returned; len(out) = len(start) - 1 = nnz(C).  The same rounding and summation order as csr_spgemm, so the same values
    give the same bits.  pa / pb cannot be checked against the value arrays: pass the map as csr_spgemm returned it."""
    lib = load_library()
    _require_tensors(pa=pa, pb=pb, start=start, a_value=a_value, b_value=b_value, out=out)
    nprod, nnz_c = int(pa.numel()), int(start.numel()) - 1
    if nnz_c < 0:
        raise SpmvAccError("start: 0 elements, the map of an empty product still holds one")
    _require(lib, pa=(pa, "i32", nprod), pb=(pb, "i32", nprod), start=(start, "i32", nnz_c + 1), a_value=(a_value, "f64", 1 if nprod else 0),
             b_value=(b_value, "f64", 1 if nprod else 0), out=(out, "f64", nnz_c))
    rc = lib.spmv_acc_csr_spgemm_values(nprod, nnz_c, _ptr(pa), _ptr(pb), _ptr(start), _ptr(a_value), _ptr(b_value), _ptr(out))
    if rc != 0:
        _check(lib)
        raise SpmvAccError(f"csr_spgemm_values failed ({rc})")


def csr_add(m: int, n: int, a_rowptr, a_colindex, a_value, b_rowptr, b_colindex, b_value, alpha: float = 1.0, beta: float = 1.0,
            want_map: bool = False):
    """Device sparse add C = alpha * A + beta * B (spmv_acc_csr_add), A and B both m x n in rebased CSR with every row strictly ascending in
    column (what coo_to_csr, csr_transpose and csr_spgemm return): returns new GPU tensors (rowptr, colindex, value | None[, ia, ib]).  Row i of
    C is the sorted union of the two rows, nothing pruned; ia[j] / ib[j] = the position of entry j in A's / B's arrays or -1; value[j] =
    alpha * a[ia[j]] + beta * b[ib[j]] with each product rounded and an absent side left out (not added as 0.0) -- unique, bit for bit.
    a_value = b_value = None: structure only.  ia / ib: the map for csr_add_values.  len(a_colindex) / len(b_colindex) must be a_rowptr[m] /
    b_rowptr[m].  This wrapper allocates arrays of the upper bound nnz_a + nnz_b and returns EXACT-size tensors by cloning the used prefixes.
    Synchronises; not capturable."""
    import torch

    lib = load_library()
    if m < 0 or n < 0:
        raise SpmvAccError(f"negative shape ({m}, {n})")
    _require_tensors(a_rowptr=a_rowptr, a_colindex=a_colindex, b_rowptr=b_rowptr, b_colindex=b_colindex)
    nnz_a, nnz_b = int(a_colindex.numel()), int(b_colindex.numel())
    named = dict(a_rowptr=(a_rowptr, "i32", m + 1), a_colindex=(a_colindex, "i32", 0), b_rowptr=(b_rowptr, "i32", m + 1),
                 b_colindex=(b_colindex, "i32", 0))
    if (a_value is None) != (b_value is None):
        raise SpmvAccError("a_value and b_value must both be given or both be None (structure only)")
    if a_value is not None:
        _require_tensors(a_value=a_value, b_value=b_value)
        if int(a_value.numel()) > nnz_a or int(b_value.numel()) > nnz_b:  # (fewer: the "elements" check below)
            raise SpmvAccError(f"a_colindex / b_colindex hold {nnz_a} / {nnz_b} elements, a_value / b_value must hold as many")
        named.update(a_value=(a_value, "f64", nnz_a), b_value=(b_value, "f64", nnz_b))
    _require(lib, **named)
    cap = nnz_a + nnz_b
    dev = a_rowptr.device
    rowptr = torch.empty(m + 1, dtype=torch.int32, device=dev)
    colindex = torch.empty(cap, dtype=torch.int32, device=dev)
    value = None if a_value is None else torch.empty(cap, dtype=torch.float64, device=dev)
    ia = torch.empty(cap, dtype=torch.int32, device=dev) if want_map else None
    ib = torch.empty(cap, dtype=torch.int32, device=dev) if want_map else None
    h_nnz = ctypes.c_int(0)
    # (empty tensors have null pointers.  An index array without elements is not read; the value pointers form a group with c_value, so the
    # one of a matrix without non-zeros -- never read either -- stands in as rowptr's, and with nothing to add the whole group stays null)
    values = (0, 0, 0) if value is None or cap == 0 else tuple(_ptr(t) if t.numel() else _ptr(rowptr) for t in (a_value, b_value, value))
    maps = tuple(_ptr(t) if t is not None and cap else 0 for t in (ia, ib))
    rc = lib.spmv_acc_csr_add(m, n, nnz_a, _ptr(a_rowptr), _ptr(a_colindex) if nnz_a else 0, nnz_b, _ptr(b_rowptr), _ptr(b_colindex) if nnz_b else 0,
                              alpha, values[0], beta, values[1], _ptr(rowptr), _ptr(colindex) if cap else 0, values[2], maps[0], maps[1],
                              ctypes.byref(h_nnz))
    if rc != 0:
        _check(lib)
        raise SpmvAccError(f"csr_add failed ({rc})")
    nnz = int(h_nnz.value)
    out = (rowptr, colindex[:nnz].clone(), None if value is None else value[:nnz].clone())
    return out + (ia[:nnz].clone(), ib[:nnz].clone()) if want_map else out


def csr_add_values(ia, ib, a_value, b_value, out, alpha: float = 1.0, beta: float = 1.0) -> None:
    """out[j] = alpha * a_value[ia[j]] + beta * b_value[ib[j]] by csr_add's rule (spmv_acc_csr_add_values, async on torch's current stream,
    capturable): the values of C for new values of A and / or B, or a new alpha / beta, on known patterns, with the map csr_add(...,
    want_map=True) returned; len(out) = len(ia) = len(ib) = nnz(C).  A map index outside the value array (-1 included) counts as absent; both
    absent gives +0.0.  The same kernel as csr_add, so the same values give the same bits.  A captured launch keeps the alpha and beta it was
    captured with.  out must not overlap a_value or b_value."""
    lib = load_library()
    _require_tensors(ia=ia, ib=ib, a_value=a_value, b_value=b_value, out=out)
    nnz_c = int(ia.numel())
    if int(ib.numel()) > nnz_c or int(out.numel()) > nnz_c:  # (fewer: the "elements" check below)
        raise SpmvAccError(f"ia holds {nnz_c} elements, ib and out must hold as many")
    _require(lib, ia=(ia, "i32", nnz_c), ib=(ib, "i32", nnz_c), a_value=(a_value, "f64", 0), b_value=(b_value, "f64", 0), out=(out, "f64", nnz_c))
    nnz_a, nnz_b = int(a_value.numel()), int(b_value.numel())
    rc = lib.spmv_acc_csr_add_values(nnz_c, nnz_a, nnz_b, _ptr(ia) if nnz_c else 0, _ptr(ib) if nnz_c else 0, alpha, _ptr(a_value) if nnz_a else 0,
                                     beta, _ptr(b_value) if nnz_b else 0, _ptr(out) if nnz_c else 0)
    if rc != 0:
        _check(lib)
        raise SpmvAccError(f"csr_add_values failed ({rc})")


_INT_MIN, _INT_MAX = -2 ** 31, 2 ** 31 - 1


def csr_extract(m: int, n: int, rowptr, colindex, value, rows=None, colmap=None, nc=None, diag_lo=None, diag_hi=None, want_map: bool = False):
    """Device extraction C = A[rows, colmap] with a diagonal band (spmv_acc_csr_extract), A m x n in rebased CSR whose rows may be in any column
    order and may repeat a column: returns new GPU tensors (rowptr, colindex, value | None[, map]).  Row i of C is row rows[i] of A (distinct
    rows; None: every row, in order); a column c becomes colmap[c], a negative colmap[c] drops it, the others are distinct and < nc (None: the
    identity, nc = n; nc defaults to n); an entry at (i, j) of C is kept iff diag_lo <= j - i <= diag_hi (None: unbounded on that side; 0, 0 the
    diagonal; None, 0 the lower triangle; 1, None the strict upper).  Every row of C ascends in new column, equal columns (only where A's row
    repeats one) in A's order; value[j] = a_value[map[j]], the bits copied -- unique, bit for bit.  value = None: structure only.  map: for
    csr_extract_values.  len(colindex) must be rowptr[m].  This wrapper allocates arrays of the upper bound len(colindex) and returns
    EXACT-size tensors by cloning the used prefixes.  Synchronises; not capturable."""
    import torch

    lib = load_library()
    if m < 0 or n < 0:
        raise SpmvAccError(f"negative shape ({m}, {n})")
    _require_tensors(rowptr=rowptr, colindex=colindex)
    nnz_a = int(colindex.numel())
    named = dict(rowptr=(rowptr, "i32", m + 1), colindex=(colindex, "i32", 0))
    if value is not None:
        _require_tensors(value=value)
        if int(value.numel()) > nnz_a:  # (fewer: the "elements" check below)
            raise SpmvAccError(f"colindex holds {nnz_a} elements, value must hold as many")
        named["value"] = (value, "f64", nnz_a)
    mc = m
    if rows is not None:
        _require_tensors(rows=rows)
        mc = int(rows.numel())
        named["rows"] = (rows, "i32", 0)
    if colmap is not None:
        _require_tensors(colmap=colmap)
        if int(colmap.numel()) > n:  # (fewer: the "elements" check below)
            raise SpmvAccError(f"colmap holds {int(colmap.numel())} elements, A has {n} columns: it must hold as many")
        named["colmap"] = (colmap, "i32", n)
    nc = n if nc is None else int(nc)
    if nc < 0:
        raise SpmvAccError(f"negative nc ({nc})")
    if colmap is None and nc != n:
        raise SpmvAccError(f"colmap=None is the identity: nc ({nc}) must be n ({n})")
    lo = _INT_MIN if diag_lo is None else int(diag_lo)
    hi = _INT_MAX if diag_hi is None else int(diag_hi)
    if not (_INT_MIN <= lo <= _INT_MAX and _INT_MIN <= hi <= _INT_MAX):
        raise SpmvAccError(f"diag_lo / diag_hi ({lo}, {hi}) outside int32")
    _require(lib, **named)
    dev = rowptr.device
    c_rowptr = torch.empty(mc + 1, dtype=torch.int32, device=dev)
    c_colindex = torch.empty(nnz_a, dtype=torch.int32, device=dev)
    c_value = None if value is None else torch.empty(nnz_a, dtype=torch.float64, device=dev)
    cmap = torch.empty(nnz_a, dtype=torch.int32, device=dev) if want_map else None
    h_nnz = ctypes.c_int(0)
    # (empty tensors have null pointers.  An array without elements is not read; the two value pointers form a group, so with no non-zeros
    # both stay null)
    values = (0, 0) if value is None or nnz_a == 0 else (_ptr(value), _ptr(c_value))
    rc = lib.spmv_acc_csr_extract(m, n, nnz_a, _ptr(rowptr), _ptr(colindex) if nnz_a else 0, values[0], mc,
                                  _ptr(rows) if rows is not None and mc else (0 if rows is None else _ptr(c_rowptr)), nc,
                                  _ptr(colmap) if colmap is not None and n else (0 if colmap is None else _ptr(c_rowptr)), lo, hi, _ptr(c_rowptr),
                                  _ptr(c_colindex) if nnz_a else 0, values[1], _ptr(cmap) if want_map and nnz_a else 0, ctypes.byref(h_nnz))
    if rc != 0:
        _check(lib)
        raise SpmvAccError(f"csr_extract failed ({rc})")
    nnz = int(h_nnz.value)
    out = (c_rowptr, c_colindex[:nnz].clone(), None if c_value is None else c_value[:nnz].clone())
    return out + (cmap[:nnz].clone(),) if want_map else out


def csr_extract_values(map, a_value, out) -> None:
    """out[j] = a_value[map[j]] (spmv_acc_csr_extract_values, async on torch's current stream, capturable): the values of C for new values of
    A on a known pattern, with the map csr_extract(..., want_map=True) or csr_permute(..., want_map=True) returned; len(out) = len(map) =
    nnz(C).  A map index outside the value array (-1 included) gives +0.0.  The same kernel as csr_extract, so the same values give the same
    bits.  out must not overlap a_value."""
    lib = load_library()
    _require_tensors(map=map, a_value=a_value, out=out)
    nnz_c = int(map.numel())
    if int(out.numel()) > nnz_c:  # (fewer: the "elements" check below)
        raise SpmvAccError(f"map holds {nnz_c} elements, out must hold as many")
    _require(lib, map=(map, "i32", nnz_c), a_value=(a_value, "f64", 0), out=(out, "f64", nnz_c))
    nnz_a = int(a_value.numel())
    rc = lib.spmv_acc_csr_extract_values(nnz_c, nnz_a, _ptr(map) if nnz_c else 0, _ptr(a_value) if nnz_a else 0, _ptr(out) if nnz_c else 0)
    if rc != 0:
        _check(lib)
        raise SpmvAccError(f"csr_extract_values failed ({rc})")


def csr_permute(m: int, rowptr, colindex, value, perm, want_map: bool = False):
    """The symmetric permutation C = P A P^T of a square m x m CSR: C[i, j] = A[perm[i], perm[j]] (csr_extract with rows = perm and colmap =
    the inverse of perm, built on the device).  perm: m int32 entries on the GPU, a permutation of [0, m).  Its length and range are checked
    here, with a reduction, before it is used as an index; a repeated entry leaves a hole in the inverse and is refused by the C entry's
    distinct-rows check.  Returns what csr_extract returns."""
    import torch

    lib = load_library()
    if m < 0:
        raise SpmvAccError(f"negative shape ({m}, {m})")
    _require_tensors(perm=perm)
    if int(perm.numel()) != m:
        raise SpmvAccError(f"perm holds {int(perm.numel())} elements, a permutation of the {m} rows must hold as many")
    _require(lib, perm=(perm, "i32", m))
    inverse = torch.full((m,), -1, dtype=torch.int32, device=perm.device)
    if m:
        low, high = int(perm.min()), int(perm.max())
        if low < 0 or high >= m:
            raise SpmvAccError(f"perm: values in [{low}, {high}], a permutation of the rows holds [0, {m})")
        inverse[perm.long()] = torch.arange(m, dtype=torch.int32, device=perm.device)
    return csr_extract(m, m, rowptr, colindex, value, rows=perm, colmap=inverse, nc=m, want_map=want_map)


_GS_DIRECTIONS = {"forward": 0, "backward": 1, "symmetric": 2}
_GS_FIRST_CAP = 1024  # colours csr_color makes room for before it asks the entry how many there are


def csr_color(m: int, rowptr, colindex):
    """The multicolour ordering of a square m x m CSR with strictly ascending rows and a symmetric pattern (spmv_acc_csr_color): returns
    (color, color_rows, color_ptr, no_diag).  color[v]: the colour of row v, the greedy colouring in descending priority (mix32(v) << 32) | v
    -- unique, a pure function of the pattern.  color_rows: the rows in ascending (colour, row), int32 on the GPU.  color_ptr: a HOST list,
    colour c owns color_rows[color_ptr[c]:color_ptr[c + 1]]; len(color_ptr) - 1 colours.  no_diag: rows without a stored diagonal (a sweep
    leaves them untouched).  len(colindex) must be rowptr[m].  An unsymmetric matrix: colour the pattern of A + A^T (csr_transpose, csr_add).
    Synchronises; not capturable.

    Sweeps on the original matrix:   csr_gs_sweep(m, rowptr, colindex, value, color_ptr, color_rows, b, x)
    The colour-permuted, coalesced form -- every colour a contiguous row range:
        p_rowptr, p_colindex, p_value = csr_permute(m, rowptr, colindex, value, perm=color_rows)
        pb, px = b[color_rows.long()], x[color_rows.long()]
        csr_gs_sweep(m, p_rowptr, p_colindex, p_value, color_ptr, None, pb, px)        # color_rows=None
        x[color_rows.long()] = px"""
    import torch

    lib = load_library()
    if m < 0:
        raise SpmvAccError(f"negative shape ({m}, {m})")
    _require_tensors(rowptr=rowptr, colindex=colindex)
    nnz = int(colindex.numel())
    _require(lib, rowptr=(rowptr, "i32", m + 1), colindex=(colindex, "i32", 0))
    dev = rowptr.device
    color = torch.empty(m, dtype=torch.int32, device=dev)
    color_rows = torch.empty(m, dtype=torch.int32, device=dev)
    cap = _GS_FIRST_CAP
    for attempt in range(2):  # (the second with the count the first returned)
        h_ptr = (ctypes.c_int * (cap + 1))()
        h_ncolors, h_no_diag = ctypes.c_int(0), ctypes.c_int(0)
        rc = lib.spmv_acc_csr_color(m, nnz, _ptr(rowptr), _ptr(colindex) if nnz else 0, _ptr(color) if m else 0, _ptr(color_rows) if m else 0,
                                    cap, h_ptr, ctypes.byref(h_ncolors), ctypes.byref(h_no_diag))
        if rc == 4 and attempt == 0 and h_ncolors.value > cap:  # SPMV_ACC_ERR_TOO_LARGE: more colours than the first array holds
            lib.spmv_acc_clear_error()
            cap = int(h_ncolors.value)
            continue
        break
    if rc != 0:
        _check(lib)
        raise SpmvAccError(f"csr_color failed ({rc})")
    return color, color_rows, [int(h_ptr[c]) for c in range(h_ncolors.value + 1)], int(h_no_diag.value)


def csr_gs_sweep(m: int, rowptr, colindex, value, color_ptr, color_rows, b, x, omega: float = 1.0, direction="symmetric", sweeps: int = 1) -> None:
    """`sweeps` multicolour Gauss-Seidel (omega = 1) / SOR sweeps of x towards A x = b, in place (spmv_acc_csr_gs_sweep, async on torch's
    current stream, capturable): direction "forward", "backward" or "symmetric" (forward, then backward); color_ptr and color_rows from
    csr_color on the same pattern.  color_rows=None: the matrix, b and x are permuted by colour (csr_color's docstring) and colour c is the row
    range color_ptr[c]:color_ptr[c + 1].  One launch per non-empty colour and direction.  Bit for bit a pure function of the arrays and of
    color_ptr.  A row without a stored diagonal is left untouched.  b must not overlap x."""
    lib = load_library()
    if m < 0:
        raise SpmvAccError(f"negative shape ({m}, {m})")
    if direction not in _GS_DIRECTIONS:
        raise SpmvAccError(f"direction {direction!r}: one of {tuple(_GS_DIRECTIONS)}")
    if int(sweeps) < 0:
        raise SpmvAccError(f"negative sweeps ({sweeps})")
    _require_tensors(rowptr=rowptr, colindex=colindex, value=value, b=b, x=x)
    nnz = int(colindex.numel())
    if int(value.numel()) > nnz:  # (fewer: the "elements" check below)
        raise SpmvAccError(f"colindex holds {nnz} elements, value must hold as many")
    named = dict(rowptr=(rowptr, "i32", m + 1), colindex=(colindex, "i32", 0), value=(value, "f64", nnz), b=(b, "f64", m), x=(x, "f64", m))
    if color_rows is not None:
        _require_tensors(color_rows=color_rows)
        if int(color_rows.numel()) != m:
            raise SpmvAccError(f"color_rows holds {int(color_rows.numel())} elements, the {m} rows in colour order must be as many")
        named["color_rows"] = (color_rows, "i32", m)
    try:
        ptr = [int(p) for p in color_ptr]
    except TypeError:
        raise SpmvAccError("color_ptr: a host list of ints (csr_color returns it)") from None
    if not ptr or ptr[0] != 0 or ptr[-1] != m or any(hi < lo for lo, hi in zip(ptr, ptr[1:])):
        raise SpmvAccError(f"color_ptr must ascend from 0 to m = {m}")
    _require(lib, **named)
    h_ptr = (ctypes.c_int * len(ptr))(*ptr)
    for _ in range(int(sweeps)):
        rc = lib.spmv_acc_csr_gs_sweep(m, nnz, _ptr(rowptr), _ptr(colindex) if nnz else 0, _ptr(value) if nnz else 0, len(ptr) - 1, h_ptr,
                                       _ptr(color_rows) if color_rows is not None and m else 0, float(omega), _GS_DIRECTIONS[direction],
                                       _ptr(b) if m else 0, _ptr(x) if m else 0)
        if rc != 0:
            _check(lib)
            raise SpmvAccError(f"csr_gs_sweep failed ({rc})")


_JACOBI_KINDS = {"jacobi": 0, "l1": 1}


def csr_jacobi_diagonal(m: int, rowptr, colindex, value, kind="l1"):
    """The inverse diagonal csr_jacobi_sweep takes, of a square m x m CSR with ascending rows (spmv_acc_csr_jacobi_diagonal, async on torch's
    current stream, capturable): returns dinv, fp64 on the GPU.  kind "jacobi": 1 / a_ii.  kind "l1": 1 / d_i with the scaled l1 diagonal
    d_i = sum_j |a_ij| sqrt(|a_ii|) / sqrt(|a_jj|), which bounds a symmetric A with a positive diagonal from above (D >= A: the sweep
    contracts in the energy norm for every omega in (0, 2)) and scales as A does under A -> S A S.  +0.0 where a row stores no diagonal.  The
    work vector of kind "l1" (m doubles) is allocated here.  Bit for bit a pure function of the arrays.  len(colindex) must be rowptr[m]."""
    import torch

    lib = load_library()
    if m < 0:
        raise SpmvAccError(f"negative shape ({m}, {m})")
    if kind not in _JACOBI_KINDS:
        raise SpmvAccError(f"kind {kind!r}: one of {tuple(_JACOBI_KINDS)}")
    _require_tensors(rowptr=rowptr, colindex=colindex, value=value)
    nnz = int(colindex.numel())
    if int(value.numel()) > nnz:  # (fewer: the "elements" check below)
        raise SpmvAccError(f"colindex holds {nnz} elements, value must hold as many")
    _require(lib, rowptr=(rowptr, "i32", m + 1), colindex=(colindex, "i32", 0), value=(value, "f64", nnz))
    dinv = torch.empty(m, dtype=torch.float64, device=rowptr.device)
    work = torch.empty(m, dtype=torch.float64, device=rowptr.device) if kind == "l1" else None
    rc = lib.spmv_acc_csr_jacobi_diagonal(m, nnz, _ptr(rowptr), _ptr(colindex) if nnz else 0, _ptr(value) if nnz else 0, _JACOBI_KINDS[kind],
                                          _ptr(dinv) if m else 0, _ptr(work) if work is not None and m else 0)
    if rc != 0:
        _check(lib)
        raise SpmvAccError(f"csr_jacobi_diagonal failed ({rc})")
    return dinv


def csr_jacobi_sweep(m: int, rowptr, colindex, value, dinv, b, x_in, x_out=None, r_out=None, omega: float = 1.0) -> None:
    """One damped Jacobi sweep towards A x = b, out of place, in ONE launch (spmv_acc_csr_jacobi_sweep, async on torch's current stream,
    capturable): with t = b - A x_in, r_out = t (if given) and x_out = x_in + omega * dinv * t (if given); at least one of the two.  x_in=None
    is the zero start: the matrix is not read, t = b, x_out = omega * dinv * b.  dinv from csr_jacobi_diagonal.  Bit for bit a pure function of
    the arrays and omega.  x_out, r_out, x_in, b and dinv must not overlap: ping-pong between two vectors."""
    lib = load_library()
    if m < 0:
        raise SpmvAccError(f"negative shape ({m}, {m})")
    if not (isinstance(omega, (int, float)) and math.isfinite(omega)):
        raise SpmvAccError(f"omega = {omega}: a finite relaxation factor is required")
    if x_out is None and r_out is None:
        raise SpmvAccError("x_out and r_out are both None: nothing to write")
    _require_tensors(rowptr=rowptr, colindex=colindex, value=value, dinv=dinv, b=b)
    optional = {name: t for name, t in (("x_in", x_in), ("x_out", x_out), ("r_out", r_out)) if t is not None}
    _require_tensors(**optional)
    nnz = int(colindex.numel())
    if int(value.numel()) > nnz:  # (fewer: the "elements" check below)
        raise SpmvAccError(f"colindex holds {nnz} elements, value must hold as many")
    named = dict(rowptr=(rowptr, "i32", m + 1), colindex=(colindex, "i32", 0), value=(value, "f64", nnz), dinv=(dinv, "f64", m), b=(b, "f64", m))
    named.update({name: (t, "f64", m) for name, t in optional.items()})
    _require(lib, **named)
    rc = lib.spmv_acc_csr_jacobi_sweep(m, nnz, _ptr(rowptr), _ptr(colindex) if nnz else 0, _ptr(value) if nnz else 0, _ptr(dinv) if m else 0,
                                       float(omega), _ptr(b) if m else 0, _ptr(x_in) if x_in is not None and m else 0,
                                       _ptr(x_out) if x_out is not None and m else 0, _ptr(r_out) if r_out is not None and m else 0)
    if rc != 0:
        _check(lib)
        raise SpmvAccError(f"csr_jacobi_sweep failed ({rc})")


def csr_aggregate(m: int, rowptr, colindex):
    """Aggregation coarsening of a square m x m CSR pattern with strictly ascending rows and a symmetric pattern -- the strength graph; for
    the matrix itself its own pattern -- (spmv_acc_csr_aggregate): returns (agg, agg_ptr, agg_rows, naggs).  The roots are the
    lexicographically first distance-2 maximal independent set in descending priority (mix32(v) << 32) | v, numbered in ascending row order;
    a row next to a root joins it, every other row joins the smallest aggregate among its assigned neighbours -- unique, a pure function of the
    pattern.  agg[v]: the aggregate of row v.  agg_rows: the rows in ascending (aggregate, row).  agg_ptr: naggs + 1 entries, aggregate a
    owns agg_rows[agg_ptr[a]:agg_ptr[a + 1]].  All int32 on the GPU; naggs a host int.  len(colindex) must be rowptr[m].  Synchronises; not
    capturable.  The strength graph of a value threshold is csr_strength's kept pattern (see csr_smooth_prolongator for the whole level).

    The Galerkin product A_c = P^T A P on the device, P from csr_tentative:
        agg, agg_ptr, agg_rows, naggs = csr_aggregate(m, rowptr, colindex)
        P, R, bc = csr_tentative(m, agg, agg_ptr, agg_rows, b)                        # P = (p_rowptr, p_colindex, p_value), R = P^T
        AP = csr_spgemm(m, m, naggs, rowptr, colindex, value, *P)
        c_rowptr, c_colindex, c_value = csr_spgemm(naggs, m, naggs, *R, *AP)          # bc: the near-nullspace vector of the next level"""
    import torch

    lib = load_library()
    if m < 0:
        raise SpmvAccError(f"negative shape ({m}, {m})")
    _require_tensors(rowptr=rowptr, colindex=colindex)
    nnz = int(colindex.numel())
    _require(lib, rowptr=(rowptr, "i32", m + 1), colindex=(colindex, "i32", 0))
    dev = rowptr.device
    agg = torch.empty(m, dtype=torch.int32, device=dev)
    agg_rows = torch.empty(m, dtype=torch.int32, device=dev)
    agg_ptr = torch.zeros(m + 1, dtype=torch.int32, device=dev)  # (no rows: agg_ptr = [0], the entry touches nothing)
    h_naggs = ctypes.c_int(0)
    rc = lib.spmv_acc_csr_aggregate(m, nnz, _ptr(rowptr), _ptr(colindex) if nnz else 0, _ptr(agg) if m else 0, _ptr(agg_rows) if m else 0,
                                    _ptr(agg_ptr) if m else 0, ctypes.byref(h_naggs))
    if rc != 0:
        _check(lib)
        raise SpmvAccError(f"csr_aggregate failed ({rc})")
    naggs = int(h_naggs.value)
    return agg, agg_ptr[:naggs + 1].clone(), agg_rows, naggs


def csr_tentative_values(m: int, agg, agg_ptr, agg_rows, b, p_value, r_value, bc) -> None:
    """The values of the tentative prolongator on the aggregates of csr_aggregate, in place (spmv_acc_csr_tentative_values, async on torch's
    current stream, capturable): bc[a] = the 2-norm of b over aggregate a, p_value[i] = b[i] / bc[agg[i]], r_value[p] = p_value[agg_rows[p]].
    b=None: all ones.  r_value=None: not wanted.  naggs = len(agg_ptr) - 1 = len(bc).  Bit for bit a pure function of the arrays; a zero norm
    gives +0.0, not a division by zero.  b and bc must not overlap an output."""
    lib = load_library()
    if m < 0:
        raise SpmvAccError(f"negative shape ({m}, {m})")
    _require_tensors(agg=agg, agg_ptr=agg_ptr, agg_rows=agg_rows, p_value=p_value, bc=bc)
    naggs = int(agg_ptr.numel()) - 1
    if naggs < 0:
        raise SpmvAccError("agg_ptr: 0 elements, the pointer of no aggregate still holds one")
    for name, t, count, what in (("agg", agg, m, f"the aggregates of the {m} rows"), ("agg_rows", agg_rows, m, f"the {m} rows in aggregate order"),
                                 ("bc", bc, naggs, f"the norms of the {naggs} aggregates of agg_ptr")):
        if int(t.numel()) != count:
            raise SpmvAccError(f"{name} holds {int(t.numel())} elements, {what} must be as many")
    named = dict(agg=(agg, "i32", m), agg_ptr=(agg_ptr, "i32", naggs + 1), agg_rows=(agg_rows, "i32", m), p_value=(p_value, "f64", m),
                 bc=(bc, "f64", naggs))
    if b is not None:
        _require_tensors(b=b)
        named["b"] = (b, "f64", m)
    if r_value is not None:
        _require_tensors(r_value=r_value)
        named["r_value"] = (r_value, "f64", m)
    _require(lib, **named)
    rc = lib.spmv_acc_csr_tentative_values(m, naggs, _ptr(agg) if m else 0, _ptr(agg_ptr), _ptr(agg_rows) if m else 0,
                                           _ptr(b) if b is not None and m else 0, _ptr(p_value) if m else 0,
                                           _ptr(r_value) if r_value is not None and m else 0, _ptr(bc) if naggs else 0)
    if rc != 0:
        _check(lib)
        raise SpmvAccError(f"csr_tentative_values failed ({rc})")


def csr_tentative(m: int, agg, agg_ptr, agg_rows, b=None):
    """The tentative prolongator of smoothed aggregation and its transpose as CSR matrices, from csr_aggregate's arrays: returns
    ((p_rowptr, p_colindex, p_value), (r_rowptr, r_colindex, r_value), bc).  P is m x naggs with one entry per row: p_rowptr = arange(m + 1),
    p_colindex IS agg; R = P^T is naggs x m with ascending rows: r_rowptr IS agg_ptr, r_colindex IS agg_rows (no copies).  The values and bc:
    csr_tentative_values, which also refreshes them in place for a new b."""
    import torch

    _require_tensors(agg=agg, agg_ptr=agg_ptr)
    if m < 0:
        raise SpmvAccError(f"negative shape ({m}, {m})")
    dev = agg.device
    naggs = max(int(agg_ptr.numel()) - 1, 0)
    p_value = torch.empty(m, dtype=torch.float64, device=dev)
    r_value = torch.empty(m, dtype=torch.float64, device=dev)
    bc = torch.empty(naggs, dtype=torch.float64, device=dev)
    csr_tentative_values(m, agg, agg_ptr, agg_rows, b, p_value, r_value, bc)
    p_rowptr = torch.arange(m + 1, dtype=torch.int32, device=dev)
    return (p_rowptr, agg, p_value), (agg_ptr, agg_rows, r_value), bc


def csr_strength_values(m: int, s_rowptr, s_colindex, map, drop_ptr, value, s_value, diag, omega: float = 0.0) -> None:
    """The values that go with csr_strength's kept pattern, in place (spmv_acc_csr_strength_values, async on torch's current stream,
    capturable): diag[i] = a_ii plus the sum of row i's dropped entries (+0.0 for a row of S without a diagonal, whose lump is discarded), and
    s_value on S's structure: omega == 0.0 the filtered matrix A_F (diag on the diagonal, A's values elsewhere, bits copied); omega != 0.0
    M = I - omega D_F^-1 A_F (1 - omega on the diagonal, -omega * v / diag[i] elsewhere; a row with a zero diag is an identity row).
    nnz = len(map) = len(value), nnz_s = len(s_colindex) = len(s_value), len(diag) = m.  value holds A's CURRENT values in A's order.  Bit for
    bit a pure function of the arrays and omega.  value and diag must not overlap s_value, diag must not overlap value."""
    lib = load_library()
    if m < 0:
        raise SpmvAccError(f"negative shape ({m}, {m})")
    _require_tensors(s_rowptr=s_rowptr, s_colindex=s_colindex, map=map, drop_ptr=drop_ptr, value=value, s_value=s_value, diag=diag)
    nnz, nnz_s = int(map.numel()), int(s_colindex.numel())
    if nnz_s > nnz:
        raise SpmvAccError(f"s_colindex holds {nnz_s} elements, map {nnz}: the kept pattern has at most as many entries as the matrix")
    for name, t, count, what in (("value", value, nnz, f"the values of the {nnz} positions of map"),
                                 ("s_value", s_value, nnz_s, f"the values of the {nnz_s} entries of s_colindex"),
                                 ("diag", diag, m, f"the diagonal of the {m} rows")):
        if int(t.numel()) != count:
            raise SpmvAccError(f"{name} holds {int(t.numel())} elements, {what} must be as many")
    if not math.isfinite(omega):
        raise SpmvAccError(f"omega = {omega}: a finite relaxation factor is required")
    _require(lib, s_rowptr=(s_rowptr, "i32", m + 1), s_colindex=(s_colindex, "i32", nnz_s), map=(map, "i32", nnz), drop_ptr=(drop_ptr, "i32", m + 1),
             value=(value, "f64", nnz), s_value=(s_value, "f64", nnz_s), diag=(diag, "f64", m))
    rc = lib.spmv_acc_csr_strength_values(m, nnz, nnz_s, _ptr(s_rowptr), _ptr(s_colindex) if nnz_s else 0, _ptr(map) if nnz else 0, _ptr(drop_ptr),
                                          _ptr(value) if nnz else 0, float(omega), _ptr(s_value) if nnz_s else 0, _ptr(diag) if m else 0)
    if rc != 0:
        _check(lib)
        raise SpmvAccError(f"csr_strength_values failed ({rc})")


def csr_strength(m: int, rowptr, colindex, value, theta: float):
    """The strength-of-connection filter of a square m x m CSR with strictly ascending rows and a symmetric pattern (values may be unsymmetric)
    at the threshold theta >= 0 (spmv_acc_csr_strength): returns ((s_rowptr, s_colindex, s_value), map, drop_ptr, diag, no_diag).
    With sd[i] = sqrt(|a_ii|) (+0.0 without a stored diagonal) an off-diagonal (i, j) is kept iff |a_ij| >= (sd[i] * sd[j]) * theta or
    |a_ji| >= the same; a stored diagonal is always kept: a symmetric pattern whatever the values, unique to the bit.  S = (s_rowptr, s_colindex)
    holds the kept entries in A's order -- the strength graph csr_aggregate takes --; s_value = the filtered matrix A_F, the dropped entries of a
    row lumped onto its diagonal, which is diag (csr_strength_values with omega = 0).  map: A's positions, the kept ones ascending then the
    dropped ones ascending; drop_ptr[i]: where row i's dropped positions begin in map.  no_diag: rows without a stored diagonal (a host int).
    len(colindex) must be rowptr[m].  Synchronises; not capturable.  Refresh the values for new values of A with csr_strength_values."""
    import torch

    lib = load_library()
    if m < 0:
        raise SpmvAccError(f"negative shape ({m}, {m})")
    _require_tensors(rowptr=rowptr, colindex=colindex, value=value)
    nnz = int(colindex.numel())
    if int(value.numel()) != nnz:
        raise SpmvAccError(f"value holds {int(value.numel())} elements, the {nnz} entries of colindex must be as many")
    if not (math.isfinite(theta) and theta >= 0.0):
        raise SpmvAccError(f"theta = {theta}: a finite threshold >= 0 is required")
    _require(lib, rowptr=(rowptr, "i32", m + 1), colindex=(colindex, "i32", 0), value=(value, "f64", 0))
    dev = rowptr.device
    s_rowptr = torch.zeros(m + 1, dtype=torch.int32, device=dev)  # (no rows: [0], the entry touches nothing)
    drop_ptr = torch.zeros(m + 1, dtype=torch.int32, device=dev)
    s_colindex = torch.empty(nnz, dtype=torch.int32, device=dev)
    map = torch.empty(nnz, dtype=torch.int32, device=dev)
    h_nnz_s, h_no_diag = ctypes.c_int(0), ctypes.c_int(0)
    rc = lib.spmv_acc_csr_strength(m, nnz, _ptr(rowptr), _ptr(colindex) if nnz else 0, _ptr(value) if nnz else 0, float(theta), _ptr(s_rowptr) if m else 0,
                                   _ptr(s_colindex) if nnz else 0, _ptr(map) if nnz else 0, _ptr(drop_ptr) if m else 0, ctypes.byref(h_nnz_s),
                                   ctypes.byref(h_no_diag))
    if rc != 0:
        _check(lib)
        raise SpmvAccError(f"csr_strength failed ({rc})")
    nnz_s = int(h_nnz_s.value)
    s_colindex = s_colindex[:nnz_s]
    s_value = torch.empty(nnz_s, dtype=torch.float64, device=dev)
    diag = torch.empty(m, dtype=torch.float64, device=dev)
    csr_strength_values(m, s_rowptr, s_colindex, map, drop_ptr, value, s_value, diag, 0.0)
    return (s_rowptr, s_colindex, s_value), map, drop_ptr, diag, int(h_no_diag.value)


def csr_smooth_prolongator(m: int, naggs: int, s_rowptr, s_colindex, map, drop_ptr, value, P, omega: float):
    """The prolongator of smoothed aggregation, P_s = (I - omega D_F^-1 A_F) T, as a CSR (p_rowptr, p_colindex, p_value) of m x naggs:
    csr_strength_values(..., omega) into a fresh value array M on S's structure, then csr_spgemm(m, m, naggs, s_rowptr, s_colindex, M, *P).
    P = (t_rowptr, t_colindex, t_value) is the tentative prolongator T of csr_tentative; value holds A's values in A's order.

    One level of an aggregation AMG setup on the device:
        S, map, drop_ptr, diag, _ = csr_strength(m, rowptr, colindex, value, theta)     # S = (s_rowptr, s_colindex, A_F's values)
        agg, agg_ptr, agg_rows, naggs = csr_aggregate(m, S[0], S[1])                      # aggregates of the strength graph
        T, _, bc = csr_tentative(m, agg, agg_ptr, agg_rows, b)
        Ps = csr_smooth_prolongator(m, naggs, S[0], S[1], map, drop_ptr, value, T, omega)
        Rs = csr_transpose(m, naggs, Ps[1].numel(), *Ps)                                  # R = P_s^T
        AP = csr_spgemm(m, m, naggs, rowptr, colindex, value, *Ps)
        c_rowptr, c_colindex, c_value = csr_spgemm(naggs, m, naggs, *Rs, *AP)             # A_c = R A P_s; bc: the next level's b
    omega = 4 / (3 rho(D_F^-1 A_F)) is the caller's to estimate, with diag and the SpMV on A_F (a few power iterations); 2/3 suits a
    diagonally dominant A_F.  (omega = 0 would multiply T by A_F itself, which is no prolongator: pass the omega of the smoother.)
    spmv_acc_amd.amg.amg_setup runs this recipe level by level down to a dense coarsest solve, and amg_cycle applies the V-cycle."""
    import torch

    if m < 0 or naggs < 0:
        raise SpmvAccError(f"negative shape ({m}, {naggs})")
    _require_tensors(s_colindex=s_colindex)
    if not isinstance(P, (tuple, list)) or len(P) != 3:
        raise SpmvAccError("P: the tentative prolongator as (p_rowptr, p_colindex, p_value) is required")
    m_value = torch.empty(int(s_colindex.numel()), dtype=torch.float64, device=s_colindex.device)
    diag = torch.empty(m, dtype=torch.float64, device=s_colindex.device)
    csr_strength_values(m, s_rowptr, s_colindex, map, drop_ptr, value, m_value, diag, omega)
    return csr_spgemm(m, m, naggs, s_rowptr, s_colindex, m_value, *P)


DENSE_MAX_ROWS = 4096  # kDenseMaxRows (spmv_acc_amd/csrc/dense.hpp): the rows csr_dense_inverse takes


def csr_dense_inverse(m: int, rowptr, colindex, value):
    """The dense inverse of a small square m x m CSR with strictly ascending rows (spmv_acc_csr_dense_inverse), m <= DENSE_MAX_ROWS: returns
    (inv, info).  inv: a torch fp64 tensor of shape (m, m) on the GPU, row-major, by Gauss-Jordan elimination with partial pivoting in the
    unblocked order include/spmv_acc.h documents -- a pure function of the arrays, bit for bit.  info == 0: inv is valid; info == k + 1: the
    pivot of step k was zero, NaN or infinite (a singular matrix) and inv is unspecified.  The pattern need not be symmetric.  len(colindex)
    and len(value) must be rowptr[m].  Synchronises; not capturable.  3 m launches: the solve of the coarsest level of a hierarchy, computed
    once; dense_apply multiplies by it per cycle."""
    import torch

    lib = load_library()
    if m < 0:
        raise SpmvAccError(f"negative shape ({m}, {m})")
    _require_tensors(rowptr=rowptr, colindex=colindex, value=value)
    nnz = int(colindex.numel())
    if int(value.numel()) != nnz:
        raise SpmvAccError(f"value holds {int(value.numel())} elements, the {nnz} entries of colindex must be as many")
    if m > DENSE_MAX_ROWS:
        raise SpmvAccError(f"{m} rows: csr_dense_inverse takes at most {DENSE_MAX_ROWS} (too large for a dense inverse: coarsen further)")
    _require(lib, rowptr=(rowptr, "i32", m + 1), colindex=(colindex, "i32", 0), value=(value, "f64", 0))
    inv = torch.empty((m, m), dtype=torch.float64, device=rowptr.device)
    h_info = ctypes.c_int(0)
    rc = lib.spmv_acc_csr_dense_inverse(m, nnz, _ptr(rowptr), _ptr(colindex) if nnz else 0, _ptr(value) if nnz else 0, _ptr(inv) if m else 0,
                                        ctypes.byref(h_info))
    if rc != 0:
        _check(lib)
        raise SpmvAccError(f"csr_dense_inverse failed ({rc})")
    return inv, int(h_info.value)


def dense_apply(m: int, inv, b, x) -> None:
    """x = inv b with the (m, m) row-major inverse of csr_dense_inverse (spmv_acc_dense_apply, async on torch's current stream, capturable):
    one wavefront per row, the products rounded on their own and added in csr_gs_sweep's order with a lane group of 64 -- bit for bit a pure
    function of the arrays.  b, x: m fp64 entries each; b must not overlap x, and neither may overlap inv."""
    lib = load_library()
    if m < 0:
        raise SpmvAccError(f"negative shape ({m}, {m})")
    _require_tensors(inv=inv, b=b, x=x)
    if int(inv.numel()) != m * m:
        raise SpmvAccError(f"inv holds {int(inv.numel())} elements, the inverse of {m} rows must hold {m * m}")
    for name, t in (("b", b), ("x", x)):
        if int(t.numel()) != m:
            raise SpmvAccError(f"{name} holds {int(t.numel())} elements, a vector of the {m} rows must hold as many")
    _require(lib, inv=(inv, "f64", m * m), b=(b, "f64", m), x=(x, "f64", m))
    rc = lib.spmv_acc_dense_apply(m, _ptr(inv) if m else 0, _ptr(b) if m else 0, _ptr(x) if m else 0)
    if rc != 0:
        _check(lib)
        raise SpmvAccError(f"dense_apply failed ({rc})")


CG_STATE = 9  # kCgState (spmv_acc_amd/csrc/cg.hpp): the 8-byte words of the state block
CG_STATUS = ("running", "converged", "breakdown: p.q is not finite or <= 0", "breakdown: r.z is not finite or < 0")  # state word 0
# the words of the state block, in order (include/spmv_acc.h): the first two are integers, the others doubles
CG_WORDS = ("status", "iterations", "bb", "rr", "rz", "pq", "alpha", "beta", "tol2")


def cg_partials(n: int) -> int:
    """The doubles the partials buffer of cg_start / cg_update / cg_direction must hold for vectors of n entries (spmv_acc_cg_partials)."""
    lib = load_library()
    count = ctypes.c_size_t(0)
    rc = lib.spmv_acc_cg_partials(n, ctypes.byref(count))
    if rc != 0:
        _check(lib)
        raise SpmvAccError(f"cg_partials failed ({rc})")
    return int(count.value)


def _cg_args(lib, n, partials, state, hist, **vectors):
    """The checks the three CG wrappers share: n fp64 entries per vector, the partials buffer of cg_partials(n), the state block as CG_STATE
    int64 words, the optional history.  Returns hist_cap."""
    if n < 0:
        raise SpmvAccError(f"negative n ({n})")
    _require_tensors(partials=partials, state=state, **vectors)
    for name, t in vectors.items():
        if int(t.numel()) != n:
            raise SpmvAccError(f"{name} holds {int(t.numel())} elements, a vector of the {n} rows must hold as many")
    if str(state.dtype) != "torch.int64" or int(state.numel()) != CG_STATE:
        raise SpmvAccError(f"state: {int(state.numel())} elements of {state.dtype}, the state block is {CG_STATE} torch.int64 words")
    if not state.is_cuda:
        raise SpmvAccError("state: device pointers required, tensor is not on the GPU (no CPU fallback)")
    if not state.is_contiguous():
        raise SpmvAccError("state: tensor is not contiguous")
    named = {name: (t, "f64", n) for name, t in vectors.items()}
    named["partials"] = (partials, "f64", cg_partials(n))
    hist_cap = 0
    if hist is not None:
        _require_tensors(hist=hist)
        hist_cap = int(hist.numel())
        named["hist"] = (hist, "f64", 0)
    _require(lib, **named)
    if state.device != partials.device:
        raise SpmvAccError(f"state: on {state.device}, other arguments on {partials.device}")
    return hist_cap


def cg_start(n: int, rtol: float, b, r, z, p, partials, state, hist=None) -> None:
    """The start of a conjugate-gradient solve (spmv_acc_cg_start, async on torch's current stream, capturable, two launches): the caller has
    computed r = b - A x and z = M r (z is r: no preconditioner).  One pass takes b.b, r.r and r.z and writes p = z; one finish workgroup
    sets the state block: iterations 0, tol2 = (rtol * rtol) * b.b, status 1 at once if r.r <= tol2, 3 if r.z is not finite or <= 0.
    partials: cg_partials(n) fp64 entries; state: CG_STATE int64 words (CG_WORDS; view(torch.float64) reads the doubles); hist: optional fp64
    tensor, hist[k] receives r.r of iteration k while k < len(hist).  Every dot product is bit for bit a pure function of its two arrays."""
    lib = load_library()
    if not (isinstance(rtol, (int, float)) and math.isfinite(rtol) and rtol >= 0.0):
        raise SpmvAccError(f"rtol = {rtol}: a finite tolerance >= 0 is required")
    hist_cap = _cg_args(lib, n, partials, state, hist, b=b, r=r, z=z, p=p)
    rc = lib.spmv_acc_cg_start(n, float(rtol), _ptr(b) if n else 0, _ptr(r) if n else 0, _ptr(z) if n else 0, _ptr(p) if n else 0,
                               _ptr(partials) if n else 0, _ptr(state), _ptr(hist) if hist_cap else 0, hist_cap)
    if rc != 0:
        _check(lib)
        raise SpmvAccError(f"cg_start failed ({rc})")


def cg_update(n: int, p, q, x, r, partials, state, hist=None) -> None:
    """x += alpha p, r -= alpha q with alpha = r.z / p.q computed on the device (spmv_acc_cg_update, async, capturable, four launches); the
    caller has computed q = A p.  Status 2 if p.q is not finite or <= 0; then r.r, the history, iterations + 1, and status 1 if r.r <= tol2.
    With a status other than 0 nothing at all is written: iterations enqueued past the end of a solve change no bit."""
    lib = load_library()
    hist_cap = _cg_args(lib, n, partials, state, hist, p=p, q=q, x=x, r=r)
    rc = lib.spmv_acc_cg_update(n, _ptr(p) if n else 0, _ptr(q) if n else 0, _ptr(x) if n else 0, _ptr(r) if n else 0, _ptr(partials) if n else 0,
                                _ptr(state), _ptr(hist) if hist_cap else 0, hist_cap)
    if rc != 0:
        _check(lib)
        raise SpmvAccError(f"cg_update failed ({rc})")


def cg_direction(n: int, r, z, p, partials, state, dinv=None) -> None:
    """p = z + beta p with beta = r.z_new / r.z computed on the device (spmv_acc_cg_direction, async, capturable, three launches).  dinv (an
    fp64 tensor of n entries): z = dinv * r is written first, the Jacobi preconditioner fused; None: z is the caller's z = M r (z is r: no
    preconditioner).  Status 3 if the new r.z is not finite or < 0.  With a status other than 0 nothing at all is written."""
    lib = load_library()
    vectors = dict(r=r, z=z, p=p)
    if dinv is not None:
        vectors["dinv"] = dinv
    _cg_args(lib, n, partials, state, None, **vectors)
    rc = lib.spmv_acc_cg_direction(n, _ptr(r) if n else 0, _ptr(z) if n else 0, _ptr(dinv) if dinv is not None and n else 0, _ptr(p) if n else 0,
                                   _ptr(partials) if n else 0, _ptr(state))
    if rc != 0:
        _check(lib)
        raise SpmvAccError(f"cg_direction failed ({rc})")


def prepare(m: int, n: int, nnz: int, rowptr, colindex, value, x, strategy=None, h_rowptr=None, beta: float = 1.0) -> float:
    """Build the plan of ``strategy`` for this matrix (structural passes + per-matrix timings) without touching any y, for the
    beta class the caller will run in (beta == 0 / beta != 0).  Returns the device milliseconds it took."""
    lib = load_library()
    _csr_args(lib, m, n, nnz, rowptr, colindex, value, x)
    ms = ctypes.c_float(0.0)
    sid = lib.spmv_acc_get_strategy() if strategy is None else strategy_id(strategy)
    rc = lib.spmv_acc_prepare_beta(sid, beta, m, n, nnz, _ptr(h_rowptr), _ptr(rowptr), _ptr(colindex), _ptr(value), _ptr(x),
                                   ctypes.byref(ms))
    if rc != 0:
        _check(lib)
    return float(ms.value)


def break_points(rowptr, m: int, nnz: int, stride: int, out) -> None:
    """Device form of the row-block preprocessing pass into ``out`` (GPU int32, break_points_len entries)."""
    lib = load_library()
    _require(lib, rowptr=(rowptr, "i32", m + 1), out=(out, "i32", 1))
    rc = lib.spmv_acc_break_points(_ptr(rowptr), m, nnz, stride, _ptr(out), out.numel())
    if rc != 0:
        _check(lib)


def break_points_len(nnz: int, stride: int) -> int:
    return load_library().spmv_acc_break_points_len(nnz, stride)


def adaptive_plus_analyze(h_rowptr, m: int, min_nnz_per_block: int = 2048, threads_per_block: int = 512,
                          vec_size: int = 1):
    """Host form of the row-block preprocessing pass.  Returns (blocks, break_points, first_block_of_row)."""
    import numpy as np

    lib = load_library()
    h_rowptr = np.ascontiguousarray(h_rowptr, dtype=np.int32)
    nnz = int(h_rowptr[m])
    bp = np.zeros(m + 2 + nnz // (2 * min_nnz_per_block), dtype=np.int32)  # rows + long-row slices
    fbr = np.zeros(m + 1, dtype=np.int32)
    blocks = lib.spmv_acc_adaptive_plus_analyze(m, min_nnz_per_block, threads_per_block, vec_size, _ptr(h_rowptr),
                                                _ptr(bp), bp.size, _ptr(fbr))
    if blocks < 0:
        raise SpmvAccError(f"adaptive_plus_analyze failed ({blocks})")
    return blocks, bp[: blocks + 1].copy(), fbr


def adaptive_plus_analyze_device(rowptr, m: int, nnz: int, min_nnz_per_block: int = 1024, threads_per_block: int = 256,
                                 vec_size: int = 1):
    """Device form of the same pass (GPU int32 rowptr).  Returns (blocks, break_points, first_block_of_row) as GPU tensors."""
    import torch

    lib = load_library()
    _require(lib, rowptr=(rowptr, "i32", m + 1))
    cap = m + 2 + nnz // (2 * min_nnz_per_block)
    bp = torch.empty(cap, dtype=torch.int32, device=rowptr.device)
    fbr = torch.empty(m + 1, dtype=torch.int32, device=rowptr.device)
    blocks = lib.spmv_acc_adaptive_plus_analyze_device(m, min_nnz_per_block, threads_per_block, vec_size, _ptr(rowptr),
                                                       _ptr(bp), cap, _ptr(fbr))
    if blocks < 0:
        _check(lib)
        raise SpmvAccError(f"adaptive_plus_analyze_device failed ({blocks})")
    return blocks, bp[: blocks + 1], fbr


def adaptive_branch(m: int, h_rowptr) -> int:
    return load_library().spmv_acc_adaptive_branch(m, int(h_rowptr[m // 4]), int(h_rowptr[m // 2]),
                                                   int(h_rowptr[3 * m // 4]), int(h_rowptr[m]))


def partition_rows(m: int, parts: int, mode: int = 0, h_rowptr=None):
    import numpy as np

    lib = load_library()
    out = np.zeros(parts + 1, dtype=np.int32)
    if h_rowptr is not None:
        h_rowptr = np.ascontiguousarray(h_rowptr, dtype=np.int32)
    rc = lib.spmv_acc_partition_rows(m, parts, mode, _ptr(h_rowptr), _ptr(out))
    if rc != 0:
        _check(lib)
        raise SpmvAccError("partition_rows failed")
    return out


EVENT_DISABLE_SYSTEM_FENCE = 0x20000000  # hipEventDisableSystemFence


def time_spmv(strategy, iters: int, alpha: float, beta: float, m: int, n: int, nnz: int, rowptr, colindex, value,
              x, y, y0=None, h_rowptr=None, event_flags: int = 0) -> Sequence[float]:
    """Per-launch durations (ms) from hipEvents recorded on the library stream around each SpMV; y restored from y0 (device
    copy) before each launch, outside the event pair.  event_flags: hipEventCreateWithFlags flags (0 = hipEventDefault)."""
    lib = load_library()
    _csr_args(lib, m, n, nnz, rowptr, colindex, value, x, y, y0)
    out = (ctypes.c_float * iters)()
    rc = lib.spmv_acc_time_spmv_events(strategy_id(strategy), iters, alpha, beta, m, n, nnz, _ptr(h_rowptr), _ptr(rowptr),
                                       _ptr(colindex), _ptr(value), _ptr(x), _ptr(y), _ptr(y0),
                                       ctypes.cast(out, ctypes.c_void_p), event_flags)
    if rc != 0:
        msg = lib.spmv_acc_last_error_string().decode()
        raise SpmvAccError(f"time_spmv failed ({rc}): {msg}")
    return list(out)


def time_spmv_cold(strategy, iters: int, alpha: float, beta: float, m: int, n: int, nnz: int, rowptr, colindex, value, x, y, y0, flush,
                   h_rowptr=None) -> Sequence[float]:
    """The per-launch protocol with a cold cache hierarchy (spmv_acc_time_spmv_cold): before every timed launch, after y has been restored, the copy
    kernel moves `flush` (a device tensor of >= 2 x the 256 MB Infinity Cache; its second half is overwritten with its first) under the default
    cache policy.  Context for the fractions, never a gate."""
    lib = load_library()
    _csr_args(lib, m, n, nnz, rowptr, colindex, value, x, y, y0)
    out = (ctypes.c_float * iters)()
    rc = lib.spmv_acc_time_spmv_cold(strategy_id(strategy), iters, alpha, beta, m, n, nnz, _ptr(h_rowptr), _ptr(rowptr), _ptr(colindex),
                                     _ptr(value), _ptr(x), _ptr(y), _ptr(y0), _ptr(flush), int(flush.numel() * flush.element_size()),
                                     ctypes.cast(out, ctypes.c_void_p))
    if rc != 0:
        raise SpmvAccError(f"time_spmv_cold failed ({rc}): {lib.spmv_acc_last_error_string().decode()}")
    return list(out)


def time_spmv_total(strategy, iters: int, alpha: float, beta: float, m: int, n: int, nnz: int, rowptr, colindex, value,
                    x, y, h_rowptr=None) -> float:
    """Total milliseconds of `iters` back-to-back SpMVs between ONE hipEvent pair on the library stream."""
    lib = load_library()
    _csr_args(lib, m, n, nnz, rowptr, colindex, value, x, y)
    out = ctypes.c_float(0.0)
    rc = lib.spmv_acc_time_spmv_total(strategy_id(strategy), iters, alpha, beta, m, n, nnz, _ptr(h_rowptr), _ptr(rowptr),
                                      _ptr(colindex), _ptr(value), _ptr(x), _ptr(y), ctypes.addressof(out))
    if rc != 0:
        raise SpmvAccError(f"time_spmv_total failed ({rc}): {lib.spmv_acc_last_error_string().decode()}")
    return float(out.value)


def time_spmv_kernels(strategy, iters: int, alpha: float, beta: float, m: int, n: int, nnz: int, rowptr, colindex, value, x, y, y0=None):
    """The per-launch protocol with the library's kernel clock on: returns (event_ms, kernel_ms, launches) per call -- the event pair around
    the call (the reference harness's figure) and the sum of the call's own kernel durations (what rocprofv3 --kernel-trace reports)."""
    lib = load_library()
    _csr_args(lib, m, n, nnz, rowptr, colindex, value, x, y, y0)
    ev = (ctypes.c_float * iters)()
    kn = (ctypes.c_float * iters)()
    ln = (ctypes.c_int * iters)()
    rc = lib.spmv_acc_time_spmv_kernels(strategy_id(strategy), iters, alpha, beta, m, n, nnz, None, _ptr(rowptr), _ptr(colindex), _ptr(value),
                                        _ptr(x), _ptr(y), _ptr(y0), ctypes.cast(ev, ctypes.c_void_p), ctypes.cast(kn, ctypes.c_void_p),
                                        ctypes.cast(ln, ctypes.c_void_p))
    if rc != 0:
        raise SpmvAccError(f"time_spmv_kernels failed ({rc}): {lib.spmv_acc_last_error_string().decode()}")
    return list(ev), list(kn), list(ln)


def time_spmv_region(strategy, iters: int, alpha: float, beta: float, m: int, n: int, nnz: int, rowptr, colindex, value, x, y):
    """`iters` back-to-back SpMVs between ONE hipEvent pair and nothing else (no plan work, no allocation: settle the plan with prepare() first).
    Returns a closure: each call runs one region and returns its total milliseconds -- argument checking and pointer conversion happen HERE, once,
    so that a wall clock around the closure reads the region itself."""
    lib = load_library()
    _csr_args(lib, m, n, nnz, rowptr, colindex, value, x, y)
    out = ctypes.c_float(0.0)
    args = (strategy_id(strategy), iters, alpha, beta, m, n, nnz, None, _ptr(rowptr), _ptr(colindex), _ptr(value), _ptr(x), _ptr(y),
            ctypes.addressof(out))
    fn = lib.spmv_acc_time_spmv_region

    def run() -> float:
        rc = fn(*args)
        if rc != 0:
            raise SpmvAccError(f"time_spmv_region failed ({rc}): {lib.spmv_acc_last_error_string().decode()}")
        return float(out.value)

    return run


def copy_ceiling_gbs(dst, src, reps: int = 5) -> float:
    """Streaming-copy ceiling in GB/s (read + write) for two equally sized GPU tensors."""
    lib = load_library()
    _require_cuda(dst, src)
    nbytes = (src.numel() * src.element_size()) // 16 * 16
    return float(lib.spmv_acc_copy_ceiling_gbs(_ptr(dst), _ptr(src), nbytes, reps))


def release_plans(rowptr=None) -> None:
    load_library().spmv_acc_release_plans(_ptr(rowptr))


def set_tune_cache(path: Optional[str]) -> None:
    """Persist the per-matrix timed choices in ``path`` (None: off); see include/spmv_acc.h."""
    load_library().spmv_acc_set_tune_cache(path.encode() if path else None)


def refresh_values(rowptr) -> int:
    """After changing ``value`` in place while the opt-in column slabs (tunable col_slabs) are in use: re-copy the values into the
    plan's slabs.  Returns the number of plans refreshed."""
    return int(load_library().spmv_acc_refresh_values(_ptr(rowptr)))


def check_plans() -> int:
    """After a device synchronisation: drop every cached plan (any thread's) whose stale-plan guard has fired; returns how
    many.  ``_check`` / spmv_acc_last_error only ask the plan the calling thread used last."""
    return int(load_library().spmv_acc_check_plans())


KERNEL_NAMES = {0: "rowblock", 1: "rowblock_plus", 2: "flat_tile", 3: "slab_passes", 4: "vector_tile", 5: "vector_row", 6: "wave_row", 7: "light",
                8: "block_row", 9: "col_slabs", 10: "scale_only"}  # include/spmv_acc.h: enum spmv_acc_kernel


def query_plan(rowptr, m: int):
    import numpy as np

    out = np.zeros(9, dtype=np.int32)
    found = load_library().spmv_acc_query_plan(_ptr(rowptr), m, _ptr(out))
    if not found:
        return None
    keys = ("nnz", "adaptive_branch", "vec", "flat_tiles", "plus_blocks", "aligned16", "stream_policy", "flat_fixup", "adaptive_family")
    info = dict(zip(keys, (int(v) for v in out)))
    info["slab_passes"] = max(0, int(load_library().spmv_acc_query_plan_slab_passes(_ptr(rowptr), m)))
    info["settled"] = int(load_library().spmv_acc_query_plan_settled(_ptr(rowptr), m)) == 1
    info["col16"] = int(load_library().spmv_acc_query_plan_col16(_ptr(rowptr), m))
    info["col_bits"] = int(load_library().spmv_acc_query_plan_col_bits(_ptr(rowptr), m))
    info["last_kernel"] = KERNEL_NAMES.get(int(load_library().spmv_acc_query_plan_last_kernel(_ptr(rowptr), m)), "none")
    return info


def set_strategy(name: str) -> None:
    lib = load_library()
    if lib.spmv_acc_set_strategy(name.encode()) != 0:
        lib.spmv_acc_clear_error()
        raise SpmvAccError(f"unknown KERNEL_STRATEGY {name!r}")


def get_strategy() -> str:
    lib = load_library()
    return lib.spmv_acc_strategy_name(lib.spmv_acc_get_strategy()).decode()


from .amg import AmgHierarchy, amg_cycle, amg_setup  # noqa: E402  (the hierarchy and the V-cycle, composed from the entries above)
from .cg import CgResult, jacobi_inverse, pcg  # noqa: E402  (preconditioned conjugate gradients, composed from the entries above)
