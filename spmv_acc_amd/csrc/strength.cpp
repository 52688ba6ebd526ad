// strength.cpp -- the two entries of the strength-of-connection filter (include/spmv_acc.h spmv_acc_csr_strength, spmv_acc_csr_strength_values;
// kernels in k_strength.hip, the census in k_gs.hip, the scan in k_coo.hip; the kept pattern's definition, the values' summation order and the
// size rules in strength.hpp).
//
// Neither makes, finds or touches a plan, and nothing derived from the caller's arrays survives a call: the kept pattern and the partition
// belong to the caller, who hands them back to the values pass.  The values pass is launch-only: two kernels, nothing else.
#include "strength.hpp"
#include "engine_internal.hpp"

#include <cmath>

namespace spmv_acc {

using namespace detail;

namespace {

int strength_error(const char *entry, int code, const std::string &what) {
  set_error(code, std::string(entry) + ": " + what);
  return code;
}

constexpr size_t kStrengthAlign = 256; // workspace parts start on 256-B boundaries
size_t strength_aligned_up(size_t b) { return (b + kStrengthAlign - 1) / kStrengthAlign * kStrengthAlign; }

// the sizes every entry of the library accepts (plan.cpp: room for block arithmetic in int32)
bool strength_too_large(long long v) { return v > INT_MAX - (1 << 16); }

// [a, a + na) and [b, b + nb) share a byte (doubles; a null array shares nothing)
bool strength_overlap(const double *a, long long na, const double *b, long long nb) { return a && b && na > 0 && nb > 0 && a < b + nb && b < a + na; }

} // namespace

int run_csr_strength(int m, int nnz, const int *d_rowptr, const int *d_colindex, const double *d_value, double theta, int *d_s_rowptr,
                     int *d_s_colindex, int *d_map, int *d_drop_ptr, int *h_nnz_s, int *h_no_diag) {
  static const char *const kEntry = "spmv_acc_csr_strength";
  clear_error();
  apply_env_tunables();
  if (m < 0 || nnz < 0) return strength_error(kEntry, kErrBadArgument, "negative m or nnz");
  if (!h_nnz_s || !h_no_diag) return strength_error(kEntry, kErrBadArgument, "null h_nnz_s / h_no_diag");
  if (m > 0 && (!d_rowptr || !d_s_rowptr || !d_drop_ptr)) return strength_error(kEntry, kErrBadArgument, "null rowptr / s_rowptr / drop_ptr");
  if (m > 0 && nnz > 0 && (!d_colindex || !d_value || !d_s_colindex || !d_map))
    return strength_error(kEntry, kErrBadArgument, "null colindex / value / s_colindex / map of a matrix with non-zeros");
  if (!std::isfinite(theta) || theta < 0.0) return strength_error(kEntry, kErrBadArgument, "theta must be finite and at least 0");
  if (strength_too_large(m) || strength_too_large(nnz))
    return strength_error(kEntry, kErrTooLarge, "m or nnz does not leave room for block arithmetic in int32");
  hipStream_t st = t_stream;
  note_stream_use();
  const ScopedSet<bool> capture_flag(t_capturing, stream_capturing(st));
  if (!plan_work_allowed("the strength filter's workspace")) return last_error_code_only();
  if (m == 0) {
    if (nnz > 0) return strength_error(kEntry, kErrBadArgument, "nnz is not rowptr[m], which is 0 without rows");
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
    return strength_error(kEntry, kErrHip, "scan workspace query failed");
  }
  const size_t rows = static_cast<size_t>(m), entries = static_cast<size_t>(nnz);
  const size_t slots_bytes = strength_aligned_up(sizeof(unsigned) * kGsCounts * kCooCheckSlots), sd_bytes = strength_aligned_up(sizeof(double) * rows),
               ints = strength_aligned_up(sizeof(int) * (entries + 1)), tmp_bytes = strength_aligned_up(scan_bytes);
  const size_t off_sd = slots_bytes, off_flag = off_sd + sd_bytes, off_pos = off_flag + ints, off_tmp = off_pos + ints;
  if (!hip_ok(hipMalloc(reinterpret_cast<void **>(&ws), off_tmp + tmp_bytes), "hipMalloc strength workspace")) return leave(last_error_code_only());
  unsigned *d_slots = reinterpret_cast<unsigned *>(ws);
  double *sd = reinterpret_cast<double *>(ws + off_sd);
  int *flag = reinterpret_cast<int *>(ws + off_flag);
  int *pos = reinterpret_cast<int *>(ws + off_pos);

  // the census, before anything is written
  std::vector<unsigned> slots(static_cast<size_t>(kGsCounts) * kCooCheckSlots, 0u);
  bool ok = hip_ok(hipMemsetAsync(d_slots, 0, sizeof(unsigned) * kGsCounts * kCooCheckSlots, st), "zero the census");
  if (ok) {
    launch_gs_census(st, m, nnz, d_rowptr, d_colindex, d_slots);
    ok = hip_ok(hipMemcpyAsync(slots.data(), d_slots, sizeof(unsigned) * kGsCounts * kCooCheckSlots, hipMemcpyDeviceToHost, st), "read the census") &&
         hip_ok(hipStreamSynchronize(st), "census");
  }
  if (!ok) return leave(last_error_code_only());
  unsigned long long bad[kGsCounts] = {0, 0, 0, 0, 0, 0};
  for (int g = 0; g < kGsCounts; ++g)
    for (int s = 0; s < kCooCheckSlots; ++s) bad[g] += slots[static_cast<size_t>(g) * kCooCheckSlots + s];
  if (bad[0] + bad[1] + bad[2] + bad[3] + bad[4] != 0) {
    return leave(strength_error(kEntry, kErrBadArgument,
                                std::to_string(bad[0]) + " ends of rowptr that are not 0 and nnz, " + std::to_string(bad[1]) +
                                    " rows with a descending or out-of-range rowptr extent, " + std::to_string(bad[2]) + " columns outside [0, m), " +
                                    std::to_string(bad[3]) + " positions where a row does not strictly ascend, " + std::to_string(bad[4]) +
                                    " off-diagonal entries without their mirror (filter A + A^T instead): nothing was written"));
  }

  // the roots, the flags, their scan, the row pointers and the partition
  launch_strength_sd(st, m, nnz, d_rowptr, d_colindex, d_value, sd);
  launch_strength_flags(st, m, nnz, d_rowptr, d_colindex, d_value, sd, theta, flag);
  if (!launch_coo_scan(st, flag, nnz, pos, ws + off_tmp, &scan_bytes)) return leave(strength_error(kEntry, kErrHip, "scan failed"));
  launch_strength_ptrs(st, m, nnz, d_rowptr, pos, d_s_rowptr, d_drop_ptr);
  launch_strength_scatter(st, nnz, d_colindex, flag, pos, d_s_colindex, d_map);
  const hipError_t launch_err = hipGetLastError();
  if (launch_err != hipSuccess) return leave(strength_error(kEntry, kErrHip, std::string("kernel launch failed: ") + hipGetErrorString(launch_err)));
  int nnz_s = -1;
  if (!hip_ok(hipMemcpyAsync(&nnz_s, pos + entries, sizeof(int), hipMemcpyDeviceToHost, st), "read the number of kept entries") ||
      !hip_ok(hipStreamSynchronize(st), "strength filter"))
    return leave(last_error_code_only());
  if (nnz_s < 0 || nnz_s > nnz) // (cannot happen: a sum of nnz flags)
    return leave(strength_error(kEntry, kErrHip, std::to_string(nnz_s) + " kept entries of " + std::to_string(nnz)));
  *h_nnz_s = nnz_s;
  *h_no_diag = static_cast<int>(bad[5]);
  return leave(kOk);
}

int run_csr_strength_values(int m, int nnz, int nnz_s, const int *d_s_rowptr, const int *d_s_colindex, const int *d_map, const int *d_drop_ptr,
                            const double *d_value, double omega, double *d_s_value, double *d_diag) {
  static const char *const kEntry = "spmv_acc_csr_strength_values";
  clear_error();
  apply_env_tunables();
  if (m < 0 || nnz < 0 || nnz_s < 0) return strength_error(kEntry, kErrBadArgument, "negative m, nnz or nnz_s");
  if (nnz_s > nnz) return strength_error(kEntry, kErrBadArgument, "nnz_s exceeds nnz: S holds a part of A's entries");
  if (m > 0 && (!d_s_rowptr || !d_drop_ptr || !d_diag)) return strength_error(kEntry, kErrBadArgument, "null s_rowptr / drop_ptr / diag");
  if (m > 0 && nnz > 0 && (!d_map || !d_value)) return strength_error(kEntry, kErrBadArgument, "null map / value of a matrix with non-zeros");
  if (m > 0 && nnz_s > 0 && (!d_s_colindex || !d_s_value)) return strength_error(kEntry, kErrBadArgument, "null s_colindex / s_value of a kept pattern with entries");
  if (!std::isfinite(omega)) return strength_error(kEntry, kErrBadArgument, "omega must be finite");
  if (strength_too_large(m) || strength_too_large(nnz))
    return strength_error(kEntry, kErrTooLarge, "m or nnz does not leave room for block arithmetic in int32");
  if (strength_overlap(d_value, nnz, d_s_value, nnz_s) || strength_overlap(d_diag, m, d_s_value, nnz_s))
    return strength_error(kEntry, kErrBadArgument, "value or diag overlaps an output: s_value");
  if (strength_overlap(d_diag, m, d_value, nnz)) return strength_error(kEntry, kErrBadArgument, "diag overlaps value");
  if (m == 0) return kOk; // no rows: nothing to launch
  hipStream_t st = t_stream;
  note_stream_use();
  launch_strength_diag(st, m, nnz, nnz_s, d_s_rowptr, d_s_colindex, d_map, d_drop_ptr, d_value, d_diag);
  launch_strength_values(st, m, nnz, nnz_s, d_s_rowptr, d_s_colindex, d_map, d_value, d_diag, omega, d_s_value);
  const hipError_t launch_err = hipGetLastError();
  if (launch_err != hipSuccess) return strength_error(kEntry, kErrHip, std::string("kernel launch failed: ") + hipGetErrorString(launch_err));
  return kOk;
}

} // namespace spmv_acc
