// dense.cpp -- the two entries of the dense coarse-level solve (include/spmv_acc.h spmv_acc_csr_dense_inverse, spmv_acc_dense_apply; kernels in
// k_dense.hip, the census in k_gs.hip; the inverse's definition, the apply's summation order and the size rules in dense.hpp).
//
// Neither makes, finds or touches a plan, and nothing derived from the caller's arrays survives a call: the inverse belongs to the caller, who
// hands it back to the apply.  The apply is launch-only: one kernel, nothing else.
#include "dense.hpp"
#include "engine_internal.hpp"
#include "entry_helpers.hpp"

namespace spmv_acc {

using namespace detail;

int run_csr_dense_inverse(int m, int nnz, const int *d_rowptr, const int *d_colindex, const double *d_value, double *d_inv, int *h_info) {
  static const char *const kEntry = "spmv_acc_csr_dense_inverse";
  clear_error();
  apply_env_tunables();
  if (m < 0 || nnz < 0) return entry_error(kEntry, kErrBadArgument, "negative m or nnz");
  if (!h_info) return entry_error(kEntry, kErrBadArgument, "null h_info");
  if (m > 0 && (!d_rowptr || !d_inv)) return entry_error(kEntry, kErrBadArgument, "null rowptr / inv");
  if (m > 0 && nnz > 0 && (!d_colindex || !d_value)) return entry_error(kEntry, kErrBadArgument, "null colindex / value of a matrix with non-zeros");
  if (m > kDenseMaxRows)
    return entry_error(kEntry, kErrTooLarge, std::to_string(m) + " rows, the dense inverse takes at most " + std::to_string(kDenseMaxRows) +
                                                 " (128 MiB of inverse, 256 MiB of workspace): coarsen further");
  if (too_large(nnz)) return entry_error(kEntry, kErrTooLarge, "nnz does not leave room for block arithmetic in int32");
  hipStream_t st = t_stream;
  note_stream_use();
  const ScopedSet<bool> capture_flag(t_capturing, stream_capturing(st));
  if (!plan_work_allowed("the dense inverse's workspace")) return last_error_code_only();
  if (m == 0) {
    if (nnz > 0) return entry_error(kEntry, kErrBadArgument, "nnz is not rowptr[m], which is 0 without rows");
    *h_info = 0;
    return kOk;
  }

  // one allocation, freed in leave(): the count groups; the step's state; the pivot row (16 B per row) and the multipliers (8 B per row);
  // E = [A | I], 16 m B per row
  char *ws = nullptr;
  // every way out below passes here: the stream has run (or failed) before the workspace goes
  const auto leave = [&](int code) {
    (void)hipStreamSynchronize(st);
    (void)hipFree(ws);
    (void)hipGetLastError();
    return code;
  };
  const size_t rows = static_cast<size_t>(m);
  const size_t slots_bytes = aligned_up(sizeof(unsigned) * kGsCounts * kCooCheckSlots), state_bytes = aligned_up(sizeof(unsigned long long) * kDenseState),
               prow_bytes = aligned_up(sizeof(double) * 2 * rows), f_bytes = aligned_up(sizeof(double) * rows),
               e_bytes = aligned_up(sizeof(double) * 2 * rows * rows);
  const size_t off_state = slots_bytes, off_prow = off_state + state_bytes, off_f = off_prow + prow_bytes, off_e = off_f + f_bytes;
  if (!hip_ok(hipMalloc(reinterpret_cast<void **>(&ws), off_e + e_bytes), "hipMalloc dense inverse workspace")) return leave(last_error_code_only());
  unsigned *d_slots = reinterpret_cast<unsigned *>(ws);
  unsigned long long *state = reinterpret_cast<unsigned long long *>(ws + off_state);
  double *prow = reinterpret_cast<double *>(ws + off_prow);
  double *f = reinterpret_cast<double *>(ws + off_f);
  double *E = reinterpret_cast<double *>(ws + off_e);

  // the census, before anything is written (the colouring's; its fifth count, the mirrors, is not judged: the pattern need not be symmetric)
  if (const int rc = pattern_census(st, kEntry, m, nnz, d_rowptr, d_colindex, d_slots, nullptr, nullptr)) return leave(rc);

  // E = [A | I]; the steps, three launches each, in the order of the definition; the right half; info, read once
  if (!hip_ok(hipMemsetAsync(state, 0, sizeof(unsigned long long) * kDenseState, st), "zero the step's state")) return leave(last_error_code_only());
  launch_dense_fill(st, m, E);
  launch_dense_scatter(st, m, nnz, d_rowptr, d_colindex, d_value, E);
  for (int k = 0; k < m; ++k) {
    launch_dense_pivot(st, m, k, E, state);
    launch_dense_row(st, m, k, E, state, prow, f);
    launch_dense_update(st, m, k, E, prow, f);
  }
  launch_dense_copy(st, m, E, d_inv);
  if (const int rc = launch_error(kEntry)) return leave(rc);
  unsigned long long info = 0;
  if (!hip_ok(hipMemcpyAsync(&info, state + 2, sizeof(info), hipMemcpyDeviceToHost, st), "read info") || !hip_ok(hipStreamSynchronize(st), "dense inverse"))
    return leave(last_error_code_only());
  if (info > static_cast<unsigned long long>(m)) // (cannot happen: a step number)
    return leave(entry_error(kEntry, kErrHip, "the elimination returned the step " + std::to_string(info)));
  *h_info = static_cast<int>(info);
  return leave(kOk);
}

int run_dense_apply(int m, const double *d_inv, const double *d_b, double *d_x) {
  static const char *const kEntry = "spmv_acc_dense_apply";
  clear_error();
  apply_env_tunables();
  if (m < 0) return entry_error(kEntry, kErrBadArgument, "negative m");
  if (m > 0 && (!d_inv || !d_b || !d_x)) return entry_error(kEntry, kErrBadArgument, "null inv / b / x");
  if (too_large(m)) return entry_error(kEntry, kErrTooLarge, "m does not leave room for block arithmetic in int32");
  const long long mm = static_cast<long long>(m) * m;
  if (overlap(d_b, m, d_x, m)) return entry_error(kEntry, kErrBadArgument, "b overlaps x");
  if (overlap(d_inv, mm, d_x, m) || overlap(d_inv, mm, d_b, m)) return entry_error(kEntry, kErrBadArgument, "b or x overlaps inv");
  if (m == 0) return kOk; // no rows: nothing to launch
  hipStream_t st = t_stream;
  note_stream_use();
  launch_dense_apply(st, m, d_inv, d_b, d_x);
  return launch_error(kEntry);
}

} // namespace spmv_acc
