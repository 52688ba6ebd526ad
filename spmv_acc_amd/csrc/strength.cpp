// strength.cpp -- the two entries of the strength-of-connection filter (include/spmv_acc.h spmv_acc_csr_strength, spmv_acc_csr_strength_values;
// kernels in k_strength.hip, the census in k_gs.hip, the scan in k_coo.hip; the kept pattern's definition, the values' summation order and the
// size rules in strength.hpp).
//
// Neither makes, finds or touches a plan, and nothing derived from the caller's arrays survives a call: the kept pattern and the partition
// belong to the caller, who hands them back to the values pass.  The values pass is launch-only: two kernels, nothing else.
#include "strength.hpp"
#include "engine_internal.hpp"
#include "entry_helpers.hpp"

#include <cmath>

namespace spmv_acc {

using namespace detail;

int run_csr_strength(int m, int nnz, const int *d_rowptr, const int *d_colindex, const double *d_value, double theta, int *d_s_rowptr,
                     int *d_s_colindex, int *d_map, int *d_drop_ptr, int *h_nnz_s, int *h_no_diag) {
  static const char *const kEntry = "spmv_acc_csr_strength";
  clear_error();
  apply_env_tunables();
  if (m < 0 || nnz < 0) return entry_error(kEntry, kErrBadArgument, "negative m or nnz");
  if (!h_nnz_s || !h_no_diag) return entry_error(kEntry, kErrBadArgument, "null h_nnz_s / h_no_diag");
  if (m > 0 && (!d_rowptr || !d_s_rowptr || !d_drop_ptr)) return entry_error(kEntry, kErrBadArgument, "null rowptr / s_rowptr / drop_ptr");
  if (m > 0 && nnz > 0 && (!d_colindex || !d_value || !d_s_colindex || !d_map))
    return entry_error(kEntry, kErrBadArgument, "null colindex / value / s_colindex / map of a matrix with non-zeros");
  if (!std::isfinite(theta) || theta < 0.0) return entry_error(kEntry, kErrBadArgument, "theta must be finite and at least 0");
  if (too_large(m) || too_large(nnz))
    return entry_error(kEntry, kErrTooLarge, "m or nnz does not leave room for block arithmetic in int32");
  hipStream_t st = t_stream;
  note_stream_use();
  const ScopedSet<bool> capture_flag(t_capturing, stream_capturing(st));
  if (!plan_work_allowed("the strength filter's workspace")) return last_error_code_only();
  if (m == 0) {
    if (nnz > 0) return entry_error(kEntry, kErrBadArgument, "nnz is not rowptr[m], which is 0 without rows");
    *h_nnz_s = 0;
    *h_no_diag = 0;
    return kOk;
  }

  // one allocation, freed in leave(): the count groups; the roots of the diagonal (8 B per row); the keep flags and their scan (4 B per entry
  // and one more, each); the scratch of the scan
  char *ws = nullptr;
  // every way out below passes here: the stream has run (or failed) before the workspace goes
  const auto leave = [&](int code) {
    (void)hipStreamSynchronize(st);
    (void)hipFree(ws);
    (void)hipGetLastError();
    return code;
  };
  size_t scan_bytes = 0;
  if (!launch_coo_scan(st, nullptr, nnz, nullptr, nullptr, &scan_bytes)) {
    (void)hipGetLastError();
    return entry_error(kEntry, kErrHip, "scan workspace query failed");
  }
  const size_t rows = static_cast<size_t>(m), entries = static_cast<size_t>(nnz);
  const size_t slots_bytes = aligned_up(sizeof(unsigned) * kGsCounts * kCooCheckSlots), sd_bytes = aligned_up(sizeof(double) * rows),
               ints = aligned_up(sizeof(int) * (entries + 1)), tmp_bytes = aligned_up(scan_bytes);
  const size_t off_sd = slots_bytes, off_flag = off_sd + sd_bytes, off_pos = off_flag + ints, off_tmp = off_pos + ints;
  if (!hip_ok(hipMalloc(reinterpret_cast<void **>(&ws), off_tmp + tmp_bytes), "hipMalloc strength workspace")) return leave(last_error_code_only());
  unsigned *d_slots = reinterpret_cast<unsigned *>(ws);
  double *sd = reinterpret_cast<double *>(ws + off_sd);
  int *flag = reinterpret_cast<int *>(ws + off_flag);
  int *pos = reinterpret_cast<int *>(ws + off_pos);

  // the census, before anything is written
  unsigned long long no_diag = 0;
  if (const int rc = pattern_census(st, kEntry, m, nnz, d_rowptr, d_colindex, d_slots, "filter A + A^T instead", &no_diag)) return leave(rc);

  // the roots, the flags, their scan, the row pointers and the partition
  launch_strength_sd(st, m, nnz, d_rowptr, d_colindex, d_value, sd);
  launch_strength_flags(st, m, nnz, d_rowptr, d_colindex, d_value, sd, theta, flag);
  if (!launch_coo_scan(st, flag, nnz, pos, ws + off_tmp, &scan_bytes)) return leave(entry_error(kEntry, kErrHip, "scan failed"));
  launch_strength_ptrs(st, m, nnz, d_rowptr, pos, d_s_rowptr, d_drop_ptr);
  launch_strength_scatter(st, nnz, d_colindex, flag, pos, d_s_colindex, d_map);
  if (const int rc = launch_error(kEntry)) return leave(rc);
  int nnz_s = -1;
  if (!hip_ok(hipMemcpyAsync(&nnz_s, pos + entries, sizeof(int), hipMemcpyDeviceToHost, st), "read the number of kept entries") ||
      !hip_ok(hipStreamSynchronize(st), "strength filter"))
    return leave(last_error_code_only());
  if (nnz_s < 0 || nnz_s > nnz) // (cannot happen: a sum of nnz flags)
    return leave(entry_error(kEntry, kErrHip, std::to_string(nnz_s) + " kept entries of " + std::to_string(nnz)));
  *h_nnz_s = nnz_s;
  *h_no_diag = static_cast<int>(no_diag);
  return leave(kOk);
}

int run_csr_strength_values(int m, int nnz, int nnz_s, const int *d_s_rowptr, const int *d_s_colindex, const int *d_map, const int *d_drop_ptr,
                            const double *d_value, double omega, double *d_s_value, double *d_diag) {
  static const char *const kEntry = "spmv_acc_csr_strength_values";
  clear_error();
  apply_env_tunables();
  if (m < 0 || nnz < 0 || nnz_s < 0) return entry_error(kEntry, kErrBadArgument, "negative m, nnz or nnz_s");
  if (nnz_s > nnz) return entry_error(kEntry, kErrBadArgument, "nnz_s exceeds nnz: S holds a part of A's entries");
  if (m > 0 && (!d_s_rowptr || !d_drop_ptr || !d_diag)) return entry_error(kEntry, kErrBadArgument, "null s_rowptr / drop_ptr / diag");
  if (m > 0 && nnz > 0 && (!d_map || !d_value)) return entry_error(kEntry, kErrBadArgument, "null map / value of a matrix with non-zeros");
  if (m > 0 && nnz_s > 0 && (!d_s_colindex || !d_s_value)) return entry_error(kEntry, kErrBadArgument, "null s_colindex / s_value of a kept pattern with entries");
  if (!std::isfinite(omega)) return entry_error(kEntry, kErrBadArgument, "omega must be finite");
  if (too_large(m) || too_large(nnz))
    return entry_error(kEntry, kErrTooLarge, "m or nnz does not leave room for block arithmetic in int32");
  if (overlap(d_value, nnz, d_s_value, nnz_s) || overlap(d_diag, m, d_s_value, nnz_s))
    return entry_error(kEntry, kErrBadArgument, "value or diag overlaps an output: s_value");
  if (overlap(d_diag, m, d_value, nnz)) return entry_error(kEntry, kErrBadArgument, "diag overlaps value");
  if (m == 0) return kOk; // no rows: nothing to launch
  hipStream_t st = t_stream;
  note_stream_use();
  launch_strength_diag(st, m, nnz, nnz_s, d_s_rowptr, d_s_colindex, d_map, d_drop_ptr, d_value, d_diag);
  launch_strength_values(st, m, nnz, nnz_s, d_s_rowptr, d_s_colindex, d_map, d_value, d_diag, omega, d_s_value);
  return launch_error(kEntry);
}

} // namespace spmv_acc
