// transpose.cpp -- the transposed product's three entries (include/spmv_acc.h spmv_acc_csr_transpose, spmv_acc_csr_transpose_values,
// spmv_acc_csr_spmv_t; kernels in k_transpose.hip, size rules in transpose.hpp).
//
// None of them makes, finds or touches a plan, and nothing derived from the caller's arrays survives a call: the transposed arrays belong to
// the caller (who then runs any entry of the library on them: the whole tuned engine serves A^T), and the stateless product reads the caller's
// CSR on every call.  The `trans` argument of the other entries keeps its reported-not-applied behaviour.
#include "engine_internal.hpp"
#include "entry_helpers.hpp"
#include "transpose.hpp"

namespace spmv_acc {

using namespace detail;

int run_csr_transpose(int m, int n, int nnz, const int *d_rowptr, const int *d_colindex, const double *d_value, int *d_t_rowptr,
                      int *d_t_colindex, double *d_t_value, int *d_perm) {
  static const char *const kEntry = "spmv_acc_csr_transpose";
  clear_error();
  apply_env_tunables();
  if (m < 0 || n < 0) return entry_error(kEntry, kErrBadArgument, "negative m or n");
  if (!d_t_rowptr) return entry_error(kEntry, kErrBadArgument, "null t_rowptr");
  if ((d_value == nullptr) != (d_t_value == nullptr))
    return entry_error(kEntry, kErrBadArgument, "value and t_value must both be given or both be NULL (structure only)");
  if (too_large(m) || too_large(n) || too_large(nnz))
    return entry_error(kEntry, kErrTooLarge, "m, n or nnz does not leave room for block arithmetic in int32; shard the matrix");
  if (m > 0 && nnz != 0 && !d_rowptr) return entry_error(kEntry, kErrBadArgument, "null rowptr");
  hipStream_t st = t_stream;
  note_stream_use();
  const ScopedSet<bool> capture_flag(t_capturing, stream_capturing(st));
  if (!plan_work_allowed("the transpose's workspace")) return last_error_code_only();
  if (m > 0 && nnz != 0) { // rowptr[0] and rowptr[m]: the matrix must be rebased, and nnz is theirs
    int ends[2] = {0, 0};
    if (!hip_ok(hipMemcpyAsync(&ends[0], d_rowptr, sizeof(int), hipMemcpyDeviceToHost, st), "read rowptr[0]") ||
        !hip_ok(hipMemcpyAsync(&ends[1], d_rowptr + m, sizeof(int), hipMemcpyDeviceToHost, st), "read rowptr[m]") ||
        !hip_ok(hipStreamSynchronize(st), "read rowptr[0], rowptr[m]"))
      return last_error_code_only();
    if (ends[0] != 0)
      return entry_error(kEntry, kErrBadArgument, "rowptr[0] != 0: an un-rebased row sub-range cannot be transposed in place; rebase it first");
    if (ends[1] < 0 || (nnz >= 0 && ends[1] != nnz)) return entry_error(kEntry, kErrBadArgument, "nnz is not rowptr[m]");
    nnz = ends[1];
    if (too_large(nnz)) return entry_error(kEntry, kErrTooLarge, "nnz does not leave room for block arithmetic in int32; shard the matrix");
  }
  if (m == 0 || n == 0 || nnz <= 0) { // an empty matrix: t_rowptr is all zeros, nothing else is written
    if (nnz > 0 && n == 0) return entry_error(kEntry, kErrBadArgument, "non-zeros in a matrix without columns");
    if (!hip_ok(hipMemsetAsync(d_t_rowptr, 0, sizeof(int) * (static_cast<size_t>(n) + 1), st), "zero t_rowptr")) return last_error_code_only();
    return kOk;
  }
  if (!d_colindex || !d_t_colindex) return entry_error(kEntry, kErrBadArgument, "null colindex / t_colindex with nnz != 0");

  // one allocation: the sorted keys (then each non-zero's row), perm when the caller wants none, the census counter, the sort's scratch
  size_t sort_bytes = 0;
  if (!launch_transpose_sort(st, d_colindex, nnz, n, nullptr, nullptr, nullptr, &sort_bytes)) {
    (void)hipGetLastError();
    return entry_error(kEntry, kErrHip, "radix sort workspace query failed");
  }
  const size_t ints = aligned_up(sizeof(int) * static_cast<size_t>(nnz));
  const size_t off_perm = ints, off_bad = off_perm + (d_perm ? 0 : ints), off_sort = off_bad + kEntryAlign;
  char *ws = nullptr;
  if (!hip_ok(hipMalloc(reinterpret_cast<void **>(&ws), off_sort + aligned_up(sort_bytes)), "hipMalloc transpose workspace")) return last_error_code_only();
  int *keys = reinterpret_cast<int *>(ws);
  int *perm = d_perm ? d_perm : reinterpret_cast<int *>(ws + off_perm);
  unsigned *d_bad = reinterpret_cast<unsigned *>(ws + off_bad);
  // every way out below passes here: the stream has run (or failed) before the workspace goes
  const auto leave = [&](int code) {
    (void)hipStreamSynchronize(st);
    (void)hipFree(ws);
    (void)hipGetLastError();
    return code;
  };
  unsigned bad = 0;
  bool ok = hip_ok(hipMemsetAsync(d_bad, 0, sizeof(unsigned), st), "zero the column census");
  if (ok) {
    launch_transpose_check(st, d_colindex, nnz, n, d_bad);
    ok = hip_ok(hipMemcpyAsync(&bad, d_bad, sizeof(unsigned), hipMemcpyDeviceToHost, st), "read the column census") &&
         hip_ok(hipStreamSynchronize(st), "column census");
  }
  if (!ok) return leave(last_error_code_only());
  if (bad != 0)
    return leave(entry_error(kEntry, kErrBadArgument, std::to_string(bad) + " column indices outside [0, n): nothing was written"));
  if (!launch_transpose_sort(st, d_colindex, nnz, n, keys, perm, ws + off_sort, &sort_bytes)) return leave(entry_error(kEntry, kErrHip, "radix sort failed"));
  launch_transpose_rowptr(st, keys, nnz, n, d_t_rowptr);
  launch_transpose_rows(st, d_rowptr, m, nnz, keys); // (the sorted keys have served: their array now holds each non-zero's row)
  launch_transpose_gather(st, nnz, perm, keys, d_value, d_t_colindex, d_t_value);
  if (const int rc = launch_error(kEntry)) return leave(rc);
  if (!hip_ok(hipStreamSynchronize(st), "transpose")) return leave(last_error_code_only());
  return leave(kOk);
}

int run_csr_transpose_values(int nnz, const int *d_perm, const double *d_value, double *d_t_value) {
  static const char *const kEntry = "spmv_acc_csr_transpose_values";
  clear_error();
  apply_env_tunables();
  if (nnz < 0) return entry_error(kEntry, kErrBadArgument, "negative nnz");
  if (too_large(nnz)) return entry_error(kEntry, kErrTooLarge, "nnz does not leave room for block arithmetic in int32");
  if (nnz == 0) return kOk;
  if (!d_perm || !d_value || !d_t_value) return entry_error(kEntry, kErrBadArgument, "null perm / value / t_value");
  hipStream_t st = t_stream;
  note_stream_use();
  launch_transpose_values(st, nnz, d_perm, d_value, d_t_value);
  return launch_error(kEntry);
}

int run_csr_spmv_t(double alpha, double beta, int m, int n, int nnz, const int *d_rowptr, const int *d_colindex, const double *d_value,
                   const double *dx, double *dy) {
  static const char *const kEntry = "spmv_acc_csr_spmv_t";
  clear_error();
  apply_env_tunables();
  if (m < 0 || n < 0) return entry_error(kEntry, kErrBadArgument, "negative m or n");
  if (too_large(m) || too_large(n) || too_large(nnz))
    return entry_error(kEntry, kErrTooLarge, "m, n or nnz does not leave room for block arithmetic in int32; shard the matrix");
  if (g_tunables[kT_deterministic].val > 0)
    return entry_error(kEntry, kErrBadArgument,
                       "tunable deterministic = 1: this entry adds with fp64 atomics, its sums depend on arrival order; transpose once with "
                       "spmv_acc_csr_transpose and run spmv_acc_csr_spmv on the result (bitwise reproducible); nothing was enqueued");
  if (n == 0) return kOk; // (y is empty)
  if (!dy) return entry_error(kEntry, kErrBadArgument, "null y");
  const bool product = m > 0 && nnz != 0 && alpha != 0.0;
  if (product && (!d_rowptr || !d_colindex || !d_value || !dx)) return entry_error(kEntry, kErrBadArgument, "null rowptr / colindex / value / x");
  hipStream_t st = t_stream;
  note_stream_use();
  if (product && nnz < 0) { // the view's end offset from the device: the one case that synchronises
    const ScopedSet<bool> capture_flag(t_capturing, stream_capturing(st));
    if (!plan_work_allowed("reading rowptr[m] (nnz < 0)")) return last_error_code_only();
    if (!hip_ok(hipMemcpyAsync(&nnz, d_rowptr + m, sizeof(int), hipMemcpyDeviceToHost, st), "read rowptr[m]") ||
        !hip_ok(hipStreamSynchronize(st), "read rowptr[m]"))
      return last_error_code_only();
    if (nnz < 0) return entry_error(kEntry, kErrBadArgument, "rowptr[m] is negative");
    if (too_large(nnz)) return entry_error(kEntry, kErrTooLarge, "nnz does not leave room for block arithmetic in int32; shard the matrix");
  }
  if (beta != 1.0) launch_spmv_t_scale(st, n, beta, dy);
  if (product && nnz > 0) launch_spmv_t_scatter(st, m, n, nnz, alpha, d_rowptr, d_colindex, d_value, dx, dy);
  return launch_error(kEntry);
}

} // namespace spmv_acc
