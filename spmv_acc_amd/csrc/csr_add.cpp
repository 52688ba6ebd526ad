// csr_add.cpp -- the two entries of the device CSR sparse add C = alpha * A + beta * B (include/spmv_acc.h spmv_acc_csr_add, spmv_acc_csr_add_values;
// kernels in k_csr_add.hip; the definition, the rank formulas and the size rules in csr_add.hpp).
//
// Neither makes, finds or touches a plan, and nothing derived from the caller's arrays survives a call: C and the map belong to the caller, who
// then runs any entry of the library on C.  The first sum's values come from the values entry's kernel, so re-running the same values repeats
// its bits.
#include "csr_add.hpp"
#include "engine_internal.hpp"
#include "entry_helpers.hpp"

namespace spmv_acc {

using namespace detail;

namespace {

// the census of one matrix, for the error string
std::string csr_add_counts(const char *name, const unsigned long long *b) {
  return std::string(name) + ": " + std::to_string(b[0]) + " columns outside [0, n), " + std::to_string(b[1]) +
         " positions not ascending inside a row, " + std::to_string(b[2]) + " rows with a descending or out-of-range rowptr extent";
}

const char *const kAddRowRanges = "; rows of C are independent: add row ranges of A and B";

} // namespace

int run_csr_add(int m, int n, int nnz_a, const int *d_a_rowptr, const int *d_a_colindex, int nnz_b, const int *d_b_rowptr, const int *d_b_colindex,
                double alpha, const double *d_a_value, double beta, const double *d_b_value, int *d_c_rowptr, int *d_c_colindex, double *d_c_value,
                int *d_ia, int *d_ib, int *h_nnz) {
  static const char *const kEntry = "spmv_acc_csr_add";
  clear_error();
  apply_env_tunables();
  if (m < 0 || n < 0) return entry_error(kEntry, kErrBadArgument, "negative m or n");
  if (!d_c_rowptr || !h_nnz) return entry_error(kEntry, kErrBadArgument, "null c_rowptr / h_nnz");
  if ((d_a_value == nullptr) != (d_c_value == nullptr) || (d_b_value == nullptr) != (d_c_value == nullptr))
    return entry_error(kEntry, kErrBadArgument, "a_value, b_value and c_value must all be given or all be NULL (structure only)");
  if ((d_ia == nullptr) != (d_ib == nullptr)) return entry_error(kEntry, kErrBadArgument, "ia and ib must both be given or both be NULL (no map)");
  if (too_large(m) || too_large(n) || too_large(nnz_a) || too_large(nnz_b) ||
      too_large(static_cast<long long>(nnz_a < 0 ? 0 : nnz_a) + (nnz_b < 0 ? 0 : nnz_b)))
    return entry_error(kEntry, kErrTooLarge,
                       std::string("m, n, nnz_a, nnz_b or nnz_a + nnz_b does not leave room for block arithmetic in int32") + kAddRowRanges);
  if (m > 0 && (!d_a_rowptr || !d_b_rowptr)) return entry_error(kEntry, kErrBadArgument, "null a_rowptr / b_rowptr");
  if (m > 0 && ((nnz_a != 0 && !d_a_colindex) || (nnz_b != 0 && !d_b_colindex)))
    return entry_error(kEntry, kErrBadArgument, "null a_colindex / b_colindex of a matrix with non-zeros");
  if (m > 0 && (nnz_a != 0 || nnz_b != 0) && !d_c_colindex)
    return entry_error(kEntry, kErrBadArgument, "null c_colindex with nnz_a + nnz_b != 0");
  hipStream_t st = t_stream;
  note_stream_use();
  const ScopedSet<bool> capture_flag(t_capturing, stream_capturing(st));
  if (!plan_work_allowed("the sum's workspace")) return last_error_code_only();
  const auto nothing_to_add = [&]() { // d_c_rowptr is all zeros, nothing else is written, nothing is allocated
    if (!hip_ok(hipMemsetAsync(d_c_rowptr, 0, sizeof(int) * (static_cast<size_t>(m) + 1), st), "zero c_rowptr") ||
        !hip_ok(hipStreamSynchronize(st), "zero c_rowptr"))
      return last_error_code_only();
    *h_nnz = 0;
    return static_cast<int>(kOk);
  };
  if (m == 0) {
    if (nnz_a > 0 || nnz_b > 0) return entry_error(kEntry, kErrBadArgument, "nnz_a / nnz_b is not rowptr[m], which is 0 without rows");
    return nothing_to_add();
  }
  { // rowptr[0] and rowptr[m] of both: the matrices must be rebased, and nnz_a / nnz_b are theirs
    int ends[4] = {0, 0, 0, 0};
    if (!hip_ok(hipMemcpyAsync(&ends[0], d_a_rowptr, sizeof(int), hipMemcpyDeviceToHost, st), "read a_rowptr[0]") ||
        !hip_ok(hipMemcpyAsync(&ends[1], d_a_rowptr + m, sizeof(int), hipMemcpyDeviceToHost, st), "read a_rowptr[m]") ||
        !hip_ok(hipMemcpyAsync(&ends[2], d_b_rowptr, sizeof(int), hipMemcpyDeviceToHost, st), "read b_rowptr[0]") ||
        !hip_ok(hipMemcpyAsync(&ends[3], d_b_rowptr + m, sizeof(int), hipMemcpyDeviceToHost, st), "read b_rowptr[m]") ||
        !hip_ok(hipStreamSynchronize(st), "read the ends of a_rowptr and b_rowptr"))
      return last_error_code_only();
    if (ends[0] != 0 || ends[2] != 0)
      return entry_error(kEntry, kErrBadArgument, "a_rowptr[0] != 0 or b_rowptr[0] != 0: an un-rebased row sub-range cannot be added; rebase it first");
    if (ends[1] < 0 || (nnz_a >= 0 && ends[1] != nnz_a)) return entry_error(kEntry, kErrBadArgument, "nnz_a is not a_rowptr[m]");
    if (ends[3] < 0 || (nnz_b >= 0 && ends[3] != nnz_b)) return entry_error(kEntry, kErrBadArgument, "nnz_b is not b_rowptr[m]");
    nnz_a = ends[1];
    nnz_b = ends[3];
    if (too_large(nnz_a) || too_large(nnz_b) || too_large(static_cast<long long>(nnz_a) + nnz_b))
      return entry_error(kEntry, kErrTooLarge, std::string("nnz_a, nnz_b or nnz_a + nnz_b does not leave room for block arithmetic in int32") + kAddRowRanges);
  }
  if (nnz_a == 0 && nnz_b == 0) return nothing_to_add();

  // one allocation.  Per non-zero of A (+ 1): the match code and its scan, 4 B each.  The six census slot arrays.  ia and ib, 4 B per possible
  // entry each, when the caller wants values but no map.  The scan's scratch
  const size_t na = static_cast<size_t>(nnz_a), cap = na + static_cast<size_t>(nnz_b);
  size_t scan_bytes = 0;
  if (!launch_csr_add_scan(st, nullptr, nnz_a, nullptr, nullptr, &scan_bytes)) {
    (void)hipGetLastError();
    return entry_error(kEntry, kErrHip, "scan workspace query failed");
  }
  const bool own_map = d_ia == nullptr && d_c_value != nullptr; // (structure only and no map: no map is written at all)
  const size_t ints = aligned_up(sizeof(int) * (na + 1)), slots_bytes = aligned_up(sizeof(unsigned) * 6 * kCooCheckSlots);
  const size_t map_bytes = own_map ? aligned_up(sizeof(int) * cap) : 0;
  const size_t off_ms = ints, off_slots = off_ms + ints, off_ia = off_slots + slots_bytes, off_ib = off_ia + map_bytes, off_tmp = off_ib + map_bytes;
  char *ws = nullptr;
  if (!hip_ok(hipMalloc(reinterpret_cast<void **>(&ws), off_tmp + aligned_up(scan_bytes)), "hipMalloc sum workspace")) return last_error_code_only();
  int *bpos = reinterpret_cast<int *>(ws);
  int *ms = reinterpret_cast<int *>(ws + off_ms);
  unsigned *d_slots = reinterpret_cast<unsigned *>(ws + off_slots);
  int *ia = own_map ? reinterpret_cast<int *>(ws + off_ia) : d_ia;
  int *ib = own_map ? reinterpret_cast<int *>(ws + off_ib) : d_ib;
  // every way out below passes here: the stream has run (or failed) before the workspace goes
  const auto leave = [&](int code) {
    (void)hipStreamSynchronize(st);
    (void)hipFree(ws);
    (void)hipGetLastError();
    return code;
  };
  // the census, before anything reads through a column or a row extent
  std::vector<unsigned> slots(6 * kCooCheckSlots, 0u);
  bool ok = hip_ok(hipMemsetAsync(d_slots, 0, sizeof(unsigned) * 6 * kCooCheckSlots, st), "zero the census");
  if (ok) {
    launch_csr_add_census(st, m, n, nnz_a, d_a_rowptr, d_a_colindex, nnz_b, d_b_rowptr, d_b_colindex, d_slots);
    ok = hip_ok(hipMemcpyAsync(slots.data(), d_slots, sizeof(unsigned) * 6 * kCooCheckSlots, hipMemcpyDeviceToHost, st), "read the census") &&
         hip_ok(hipStreamSynchronize(st), "census");
  }
  if (!ok) return leave(last_error_code_only());
  unsigned long long bad[6] = {0, 0, 0, 0, 0, 0}, any_bad = 0;
  for (int g = 0; g < 6; ++g) {
    bad[g] = slot_sum(slots.data() + static_cast<size_t>(g) * kCooCheckSlots);
    any_bad += bad[g];
  }
  if (any_bad != 0) {
    return leave(entry_error(kEntry, kErrBadArgument,
                             csr_add_counts("A", bad) + "; " + csr_add_counts("B", bad + 3) +
                                 ": nothing was written (rows must be strictly ascending in column: spmv_acc_coo_to_csr sorts and merges such a matrix)"));
  }
  // ranks
  int matched = -1;
  launch_csr_add_match(st, m, nnz_a, d_a_rowptr, d_a_colindex, nnz_b, d_b_rowptr, d_b_colindex, bpos);
  if (!launch_csr_add_scan(st, bpos, nnz_a, ms, ws + off_tmp, &scan_bytes)) return leave(entry_error(kEntry, kErrHip, "scan of the matches failed"));
  if (!hip_ok(hipMemcpyAsync(&matched, ms + na, sizeof(int), hipMemcpyDeviceToHost, st), "read the number of matches") ||
      !hip_ok(hipStreamSynchronize(st), "match and scan"))
    return leave(last_error_code_only());
  if (matched < 0 || matched > nnz_a || matched > nnz_b)
    return leave(entry_error(kEntry, kErrHip, "the scan of the matches returned " + std::to_string(matched)));
  const int nnz_c = nnz_a + nnz_b - matched; // the values' launch is sized by it
  launch_csr_add_rowptr(st, m, nnz_a, d_a_rowptr, d_b_rowptr, ms, d_c_rowptr);
  launch_csr_add_place_a(st, nnz_a, nnz_b, d_a_colindex, bpos, ms, d_c_colindex, ia, ib);
  launch_csr_add_place_b(st, m, nnz_a, d_a_rowptr, d_a_colindex, nnz_b, d_b_rowptr, d_b_colindex, ms, d_c_colindex, ia, ib);
  if (d_c_value) launch_csr_add_values(st, nnz_c, nnz_a, nnz_b, ia, ib, alpha, d_a_value, beta, d_b_value, d_c_value);
  if (const int rc = launch_error(kEntry)) return leave(rc);
  if (!hip_ok(hipStreamSynchronize(st), "sum")) return leave(last_error_code_only());
  *h_nnz = nnz_c;
  return leave(kOk);
}

int run_csr_add_values(int nnz_c, int nnz_a, int nnz_b, const int *d_ia, const int *d_ib, double alpha, const double *d_a_value, double beta,
                       const double *d_b_value, double *d_c_value) {
  static const char *const kEntry = "spmv_acc_csr_add_values";
  clear_error();
  apply_env_tunables();
  if (nnz_c < 0 || nnz_a < 0 || nnz_b < 0) return entry_error(kEntry, kErrBadArgument, "negative nnz_c, nnz_a or nnz_b");
  if (too_large(nnz_c) || too_large(nnz_a) || too_large(nnz_b))
    return entry_error(kEntry, kErrTooLarge, "nnz_c, nnz_a or nnz_b does not leave room for block arithmetic in int32");
  if (nnz_c == 0) return kOk;
  if (!d_ia || !d_ib || !d_c_value || (nnz_a > 0 && !d_a_value) || (nnz_b > 0 && !d_b_value))
    return entry_error(kEntry, kErrBadArgument, "null ia / ib / c_value, or null a_value / b_value of a matrix with non-zeros");
  hipStream_t st = t_stream;
  note_stream_use();
  launch_csr_add_values(st, nnz_c, nnz_a, nnz_b, d_ia, d_ib, alpha, d_a_value, beta, d_b_value, d_c_value);
  return launch_error(kEntry);
}

} // namespace spmv_acc
