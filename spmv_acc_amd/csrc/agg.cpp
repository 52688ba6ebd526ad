// agg.cpp -- the two entries of the aggregation coarsening (include/spmv_acc.h spmv_acc_csr_aggregate, spmv_acc_csr_tentative_values; kernels in
// k_agg.hip, the census, sort keys and pointer pass in k_gs.hip; the aggregates' definition, the values' summation order and the size rules in
// agg.hpp).
//
// Neither makes, finds or touches a plan, and nothing derived from the caller's arrays survives a call: the aggregates belong to the caller, who
// hands them back to the values pass.  The values pass is launch-only: two kernels, nothing else.
#include "agg.hpp"
#include "engine_internal.hpp"
#include "entry_helpers.hpp"

namespace spmv_acc {

using namespace detail;

int run_csr_aggregate(int m, int nnz, const int *d_rowptr, const int *d_colindex, int *d_agg, int *d_agg_rows, int *d_agg_ptr, int *h_naggs) {
  static const char *const kEntry = "spmv_acc_csr_aggregate";
  clear_error();
  apply_env_tunables();
  if (m < 0 || nnz < 0) return entry_error(kEntry, kErrBadArgument, "negative m or nnz");
  if (!h_naggs) return entry_error(kEntry, kErrBadArgument, "null h_naggs");
  if (m > 0 && (!d_rowptr || !d_agg || !d_agg_rows || !d_agg_ptr)) return entry_error(kEntry, kErrBadArgument, "null rowptr / agg / agg_rows / agg_ptr");
  if (m > 0 && nnz > 0 && !d_colindex) return entry_error(kEntry, kErrBadArgument, "null colindex of a matrix with non-zeros");
  if (too_large(m) || too_large(nnz))
    return entry_error(kEntry, kErrTooLarge, "m or nnz does not leave room for block arithmetic in int32");
  hipStream_t st = t_stream;
  note_stream_use();
  const ScopedSet<bool> capture_flag(t_capturing, stream_capturing(st));
  if (!plan_work_allowed("the aggregation's workspace")) return last_error_code_only();
  if (m == 0) {
    if (nnz > 0) return entry_error(kEntry, kErrBadArgument, "nnz is not rowptr[m], which is 0 without rows");
    *h_naggs = 0;
    return kOk;
  }

  // one allocation, freed in leave(): the count groups; the keys and T1 (8 B per row each, later the sort's keys and sorted keys); the root flags
  // and their scan (4 B per row and one more, each); assignment A's buffer (4 B per row); the scratch of the scan and of the radix sort
  char *ws = nullptr;
  // every way out below passes here: the stream has run (or failed) before the workspace goes
  const auto leave = [&](int code) {
    (void)hipStreamSynchronize(st);
    (void)hipFree(ws);
    (void)hipGetLastError();
    return code;
  };
  const int key_bits = coo_index_bits(m); // (an aggregate id is below the number of roots: below m)
  size_t sort_bytes = 0, scan_bytes = 0;
  if (!launch_coo_sort(st, nullptr, m, key_bits, nullptr, nullptr, nullptr, &sort_bytes) ||
      !launch_coo_scan(st, nullptr, m, nullptr, nullptr, &scan_bytes)) {
    (void)hipGetLastError();
    return entry_error(kEntry, kErrHip, "scan / radix sort workspace query failed");
  }
  const size_t rows = static_cast<size_t>(m);
  const size_t slots_bytes = aligned_up(sizeof(unsigned) * kGsCounts * kCooCheckSlots), keys_bytes = aligned_up(sizeof(unsigned long long) * rows),
               ints = aligned_up(sizeof(int) * (rows + 1)), tmp_bytes = aligned_up(sort_bytes > scan_bytes ? sort_bytes : scan_bytes);
  const size_t off_key = slots_bytes, off_t1 = off_key + keys_bytes, off_flag = off_t1 + keys_bytes, off_id = off_flag + ints,
               off_first = off_id + ints, off_tmp = off_first + ints;
  if (!hip_ok(hipMalloc(reinterpret_cast<void **>(&ws), off_tmp + tmp_bytes), "hipMalloc aggregation workspace")) return leave(last_error_code_only());
  unsigned *d_slots = reinterpret_cast<unsigned *>(ws);
  unsigned long long *key = reinterpret_cast<unsigned long long *>(ws + off_key);
  unsigned long long *t1 = reinterpret_cast<unsigned long long *>(ws + off_t1);
  int *flag = reinterpret_cast<int *>(ws + off_flag);
  int *id = reinterpret_cast<int *>(ws + off_id);
  int *first = reinterpret_cast<int *>(ws + off_first);

  // the census, before anything is written
  if (const int rc = pattern_census(st, kEntry, m, nnz, d_rowptr, d_colindex, d_slots, "aggregate the pattern of A + A^T instead", nullptr))
    return leave(rc);

  // the rounds: T1 from the keys, then the keys decided in place from T1; kAggRoundsPerRead rounds between two reads
  launch_agg_init(st, m, key);
  std::vector<unsigned> slots(kCooCheckSlots, 0u);
  unsigned long long remaining = static_cast<unsigned long long>(m);
  while (remaining != 0) {
    for (int r = 0; r < kAggRoundsPerRead; ++r) {
      launch_agg_max(st, m, nnz, d_rowptr, d_colindex, key, t1);
      launch_agg_decide(st, m, nnz, d_rowptr, d_colindex, t1, key, d_slots);
    }
    if (!hip_ok(hipMemcpyAsync(slots.data(), d_slots, sizeof(unsigned) * kCooCheckSlots, hipMemcpyDeviceToHost, st), "read the undecided count") ||
        !hip_ok(hipStreamSynchronize(st), "aggregation rounds"))
      return leave(last_error_code_only());
    const unsigned long long now = slot_sum(slots.data());
    if (now >= remaining) // (cannot happen on a pattern that passed the census: the undecided row of highest priority is decided in every round)
      return leave(entry_error(kEntry, kErrHip, std::to_string(kAggRoundsPerRead) + " rounds decided no row while " + std::to_string(now) +
                                                    " remain: no further round is issued"));
    remaining = now;
  }

  // the roots numbered by a scan of their flags; assignment A into the workspace, B from it into the caller's array
  launch_agg_flags(st, m, key, flag);
  if (!launch_coo_scan(st, flag, m, id, ws + off_tmp, &scan_bytes)) return leave(entry_error(kEntry, kErrHip, "scan failed"));
  launch_agg_assign_roots(st, m, nnz, d_rowptr, d_colindex, flag, id, first);
  launch_agg_assign_rest(st, m, nnz, d_rowptr, d_colindex, first, d_agg, d_slots);
  if (const int rc = launch_error(kEntry)) return leave(rc);
  int naggs = -1;
  if (!hip_ok(hipMemcpyAsync(&naggs, id + rows, sizeof(int), hipMemcpyDeviceToHost, st), "read the number of aggregates") ||
      !hip_ok(hipMemcpyAsync(slots.data(), d_slots, sizeof(unsigned) * kCooCheckSlots, hipMemcpyDeviceToHost, st), "read the unassigned count") ||
      !hip_ok(hipStreamSynchronize(st), "assignment"))
    return leave(last_error_code_only());
  const unsigned long long unassigned = slot_sum(slots.data());
  if (unassigned != 0 || naggs < 1 || naggs > m) // (cannot happen: the roots are maximal, so every row has an assigned neighbour after A)
    return leave(entry_error(kEntry, kErrHip, std::to_string(unassigned) + " rows without an aggregate after the two assignment passes, " +
                                                  std::to_string(naggs) + " roots: agg holds -1 in those rows, agg_rows and agg_ptr were not written"));

  // agg_rows = the order of a stable sort by aggregate; agg_ptr from the sorted keys (the rounds' two key arrays hold the sort's keys now)
  unsigned long long *keys = key, *sorted = t1;
  launch_gs_keys(st, m, d_agg, keys);
  if (!launch_coo_sort(st, keys, m, key_bits, sorted, d_agg_rows, ws + off_tmp, &sort_bytes)) return leave(entry_error(kEntry, kErrHip, "radix sort failed"));
  launch_gs_color_ptr(st, m, sorted, m + 1, d_agg_ptr);
  if (const int rc = launch_error(kEntry)) return leave(rc);
  if (!hip_ok(hipStreamSynchronize(st), "aggregation")) return leave(last_error_code_only());
  *h_naggs = naggs;
  return leave(kOk);
}

int run_csr_tentative_values(int m, int naggs, const int *d_agg, const int *d_agg_ptr, const int *d_agg_rows, const double *d_b,
                             double *d_p_value, double *d_r_value, double *d_bc) {
  static const char *const kEntry = "spmv_acc_csr_tentative_values";
  clear_error();
  apply_env_tunables();
  if (m < 0 || naggs < 0) return entry_error(kEntry, kErrBadArgument, "negative m or naggs");
  if (m > 0 && (!d_agg || !d_agg_ptr || !d_agg_rows || !d_p_value)) return entry_error(kEntry, kErrBadArgument, "null agg / agg_ptr / agg_rows / p_value");
  if (m > 0 && naggs > 0 && !d_bc) return entry_error(kEntry, kErrBadArgument, "null bc of a prolongator with aggregates");
  if (too_large(m) || too_large(naggs))
    return entry_error(kEntry, kErrTooLarge, "m or naggs does not leave room for block arithmetic in int32");
  if (overlap(d_b, m, d_p_value, m) || overlap(d_b, m, d_r_value, m) || overlap(d_b, m, d_bc, naggs))
    return entry_error(kEntry, kErrBadArgument, "b overlaps an output");
  if (overlap(d_bc, naggs, d_p_value, m) || overlap(d_bc, naggs, d_r_value, m) || overlap(d_p_value, m, d_r_value, m))
    return entry_error(kEntry, kErrBadArgument, "bc, p_value and r_value overlap");
  if (m == 0) return kOk; // no rows: nothing to launch
  hipStream_t st = t_stream;
  note_stream_use();
  launch_agg_norms(st, m, naggs, d_agg_ptr, d_agg_rows, d_b, d_bc);
  launch_agg_values(st, m, naggs, d_agg, d_agg_rows, d_b, d_bc, d_p_value, d_r_value);
  return launch_error(kEntry);
}

} // namespace spmv_acc
