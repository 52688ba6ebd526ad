// cg.cpp -- the entries of the conjugate-gradient vector passes (include/spmv_acc.h spmv_acc_cg_partials, spmv_acc_cg_start,
// spmv_acc_cg_update, spmv_acc_cg_direction; kernels in k_cg.hip; the dot product's definition, the state block and the size rules in cg.hpp).
//
// None makes, finds or touches a plan, and nothing derived from the caller's arrays survives a call: the vectors, the state block and the
// partials buffer belong to the caller.  All three device entries are launch-only: kernels, nothing else -- no allocation, no copy, no
// synchronisation, no host read --, so they may be captured, and every refusal is made on the host before the first launch.
#include "cg.hpp"
#include "engine_internal.hpp"
#include "entry_helpers.hpp"

#include <cmath>

namespace spmv_acc {

using namespace detail;

namespace {

// an array of an entry, for the overlap rule: `count` doubles (the state block's words are as wide)
struct CgArray {
  const char *name;
  const void *at;
  long long count;
};

// No two written arrays may share a byte, and no written array may share one with a read array.  Returns the refusal's text, empty if none
std::string first_overlap(const CgArray *written, int nwritten, const CgArray *read, int nread) {
  const auto hit = [](const CgArray &a, const CgArray &b) {
    return overlap(static_cast<const double *>(a.at), a.count, static_cast<const double *>(b.at), b.count);
  };
  for (int i = 0; i < nwritten; ++i) {
    for (int j = i + 1; j < nwritten; ++j)
      if (hit(written[i], written[j])) return std::string(written[i].name) + " overlaps " + written[j].name;
    for (int j = 0; j < nread; ++j)
      if (hit(written[i], read[j])) return std::string(written[i].name) + " overlaps " + read[j].name;
  }
  return std::string();
}

// what the three device entries refuse alike: the size, the state block, the partials buffer
int common_refusals(const char *entry, int n, const double *d_partials, const unsigned long long *d_state) {
  if (n < 0) return entry_error(entry, kErrBadArgument, "negative n");
  if (too_large(n)) return entry_error(entry, kErrTooLarge, "n does not leave room for block arithmetic in int32");
  if (!d_state) return entry_error(entry, kErrBadArgument, "null state");
  if (n > 0 && !d_partials) return entry_error(entry, kErrBadArgument, "null partials");
  return kOk;
}

} // namespace

int run_cg_partials(int n, size_t *h_count) {
  static const char *const kEntry = "spmv_acc_cg_partials";
  clear_error();
  if (n < 0) return entry_error(kEntry, kErrBadArgument, "negative n");
  if (!h_count) return entry_error(kEntry, kErrBadArgument, "null h_count");
  if (too_large(n)) return entry_error(kEntry, kErrTooLarge, "n does not leave room for block arithmetic in int32");
  *h_count = static_cast<size_t>(kCgDots) * static_cast<size_t>(cg_chunks(n));
  return kOk;
}

int run_cg_start(int n, double rtol, const double *d_b, const double *d_r, const double *d_z, double *d_p, double *d_partials,
                 unsigned long long *d_state, double *d_hist, int hist_cap) {
  static const char *const kEntry = "spmv_acc_cg_start";
  clear_error();
  apply_env_tunables();
  if (const int rc = common_refusals(kEntry, n, d_partials, d_state)) return rc;
  if (n > 0 && (!d_b || !d_r || !d_z || !d_p)) return entry_error(kEntry, kErrBadArgument, "null b / r / z / p");
  if (!(std::isfinite(rtol) && rtol >= 0.0)) return entry_error(kEntry, kErrBadArgument, "rtol is not a finite number >= 0");
  if (hist_cap < 0) return entry_error(kEntry, kErrBadArgument, "negative hist_cap");
  if (hist_cap > 0 && !d_hist) return entry_error(kEntry, kErrBadArgument, "null hist with hist_cap > 0");
  const long long nparts = kCgDots * cg_chunks(n);
  const CgArray written[] = {{"p", d_p, n}, {"partials", d_partials, nparts}, {"state", d_state, kCgState}, {"hist", d_hist, hist_cap}};
  const CgArray read[] = {{"b", d_b, n}, {"r", d_r, n}, {"z", d_z, n}}; // (z may be r: both are only read)
  const std::string clash = first_overlap(written, 4, read, 3);
  if (!clash.empty()) return entry_error(kEntry, kErrBadArgument, clash);
  hipStream_t st = t_stream;
  note_stream_use();
  launch_cg_start_pass(st, n, d_b, d_r, d_z, d_p, d_partials);
  launch_cg_start_finish(st, n, rtol, d_partials, d_state, d_hist, hist_cap);
  return launch_error(kEntry);
}

int run_cg_update(int n, const double *d_p, const double *d_q, double *d_x, double *d_r, double *d_partials, unsigned long long *d_state,
                  double *d_hist, int hist_cap) {
  static const char *const kEntry = "spmv_acc_cg_update";
  clear_error();
  apply_env_tunables();
  if (const int rc = common_refusals(kEntry, n, d_partials, d_state)) return rc;
  if (n > 0 && (!d_p || !d_q || !d_x || !d_r)) return entry_error(kEntry, kErrBadArgument, "null p / q / x / r");
  if (hist_cap < 0) return entry_error(kEntry, kErrBadArgument, "negative hist_cap");
  if (hist_cap > 0 && !d_hist) return entry_error(kEntry, kErrBadArgument, "null hist with hist_cap > 0");
  const long long nparts = kCgDots * cg_chunks(n);
  const CgArray written[] = {{"x", d_x, n}, {"r", d_r, n}, {"partials", d_partials, nparts}, {"state", d_state, kCgState}, {"hist", d_hist, hist_cap}};
  const CgArray read[] = {{"p", d_p, n}, {"q", d_q, n}};
  const std::string clash = first_overlap(written, 5, read, 2);
  if (!clash.empty()) return entry_error(kEntry, kErrBadArgument, clash);
  hipStream_t st = t_stream;
  note_stream_use();
  launch_cg_pq_pass(st, n, d_p, d_q, d_state, d_partials);
  launch_cg_pq_finish(st, n, d_partials, d_state);
  launch_cg_update_pass(st, n, d_p, d_q, d_x, d_r, d_state, d_partials);
  launch_cg_rr_finish(st, n, d_partials, d_state, d_hist, hist_cap);
  return launch_error(kEntry);
}

int run_cg_direction(int n, const double *d_r, double *d_z, const double *d_dinv, double *d_p, double *d_partials, unsigned long long *d_state) {
  static const char *const kEntry = "spmv_acc_cg_direction";
  clear_error();
  apply_env_tunables();
  if (const int rc = common_refusals(kEntry, n, d_partials, d_state)) return rc;
  if (n > 0 && (!d_r || !d_z || !d_p)) return entry_error(kEntry, kErrBadArgument, "null r / z / p");
  const long long nparts = kCgDots * cg_chunks(n);
  std::string clash;
  if (d_dinv) { // z = dinv r is written: z may be neither r nor dinv
    const CgArray written[] = {{"z", d_z, n}, {"p", d_p, n}, {"partials", d_partials, nparts}, {"state", d_state, kCgState}};
    const CgArray read[] = {{"r", d_r, n}, {"dinv", d_dinv, n}};
    clash = first_overlap(written, 4, read, 2);
  } else { // z is the caller's and only read: it may be r
    const CgArray written[] = {{"p", d_p, n}, {"partials", d_partials, nparts}, {"state", d_state, kCgState}};
    const CgArray read[] = {{"r", d_r, n}, {"z", d_z, n}};
    clash = first_overlap(written, 3, read, 2);
  }
  if (!clash.empty()) return entry_error(kEntry, kErrBadArgument, clash);
  hipStream_t st = t_stream;
  note_stream_use();
  launch_cg_rz_pass(st, n, d_r, d_z, d_dinv, d_state, d_partials);
  launch_cg_rz_finish(st, n, d_partials, d_state);
  launch_cg_direction_pass(st, n, d_z, d_p, d_state);
  return launch_error(kEntry);
}

} // namespace spmv_acc
