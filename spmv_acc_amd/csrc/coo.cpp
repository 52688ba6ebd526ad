// coo.cpp -- the two entries of the device COO -> CSR assembly (include/spmv_acc.h spmv_acc_coo_to_csr, spmv_acc_coo_to_csr_values; kernels in
// k_coo.hip, size rules and the summation order in coo.hpp).
//
// Neither makes, finds or touches a plan, and nothing derived from the caller's arrays survives a call: the CSR and the map belong to the
// caller, who then runs any entry of the library on the CSR.  The first entry's values come from the second entry's kernel, so a re-assembly
// of the same values repeats the first assembly's bits.
#include "coo.hpp"
#include "engine_internal.hpp"
#include "entry_helpers.hpp"

namespace spmv_acc {

using namespace detail;

int run_coo_to_csr(int m, int n, int nnz_coo, const int *d_row, const int *d_col, const double *d_val, int *d_rowptr, int *d_colindex,
                   double *d_value, int *d_order, int *d_start, int *h_nnz) {
  static const char *const kEntry = "spmv_acc_coo_to_csr";
  clear_error();
  apply_env_tunables();
  if (m < 0 || n < 0 || nnz_coo < 0) return entry_error(kEntry, kErrBadArgument, "negative m, n or nnz_coo");
  if (!d_rowptr || !h_nnz) return entry_error(kEntry, kErrBadArgument, "null rowptr / h_nnz");
  if ((d_val == nullptr) != (d_value == nullptr))
    return entry_error(kEntry, kErrBadArgument, "val and value must both be given or both be NULL (structure only)");
  if ((d_order == nullptr) != (d_start == nullptr))
    return entry_error(kEntry, kErrBadArgument, "order and start must both be given or both be NULL (no map)");
  if (too_large(m) || too_large(n) || too_large(nnz_coo))
    return entry_error(kEntry, kErrTooLarge, "m, n or nnz_coo does not leave room for block arithmetic in int32; assemble row ranges");
  if (nnz_coo > 0 && (!d_row || !d_col || !d_colindex)) return entry_error(kEntry, kErrBadArgument, "null row / col / colindex with nnz_coo != 0");
  if (nnz_coo > 0 && (m == 0 || n == 0)) return entry_error(kEntry, kErrBadArgument, "triples in a matrix without rows or columns");
  hipStream_t st = t_stream;
  note_stream_use();
  const ScopedSet<bool> capture_flag(t_capturing, stream_capturing(st));
  if (!plan_work_allowed("the assembly's workspace")) return last_error_code_only();
  if (nnz_coo == 0) { // no triples: rowptr is all zeros, nothing else is written
    if (!hip_ok(hipMemsetAsync(d_rowptr, 0, sizeof(int) * (static_cast<size_t>(m) + 1), st), "zero rowptr") ||
        !hip_ok(hipStreamSynchronize(st), "zero rowptr"))
      return last_error_code_only();
    *h_nnz = 0;
    return kOk;
  }

  // one allocation: the packed keys (after the sort: the run-head flags and their scan), the sorted keys, order and start when the caller wants
  // no map, the census slots, and the scratch of the sort and the scan (they run one after the other)
  const int col_bits = coo_index_bits(n), key_bits = coo_index_bits(m) + col_bits;
  const size_t count = static_cast<size_t>(nnz_coo);
  size_t sort_bytes = 0, scan_bytes = 0;
  if (!launch_coo_sort(st, nullptr, nnz_coo, key_bits, nullptr, nullptr, nullptr, &sort_bytes) ||
      !launch_coo_scan(st, nullptr, nnz_coo, nullptr, nullptr, &scan_bytes)) {
    (void)hipGetLastError();
    return entry_error(kEntry, kErrHip, "radix sort / scan workspace query failed");
  }
  const size_t keys_bytes = aligned_up(sizeof(unsigned long long) * (count + 1)); // (+ 1: room for the two int arrays of count + 1 that follow)
  const size_t ints = aligned_up(sizeof(int) * (count + 1));
  const size_t off_sorted = keys_bytes, off_order = off_sorted + keys_bytes, off_start = off_order + (d_order ? 0 : ints);
  const size_t off_slots = off_start + (d_start ? 0 : ints), off_tmp = off_slots + aligned_up(sizeof(unsigned) * kCooCheckSlots);
  char *ws = nullptr;
  if (!hip_ok(hipMalloc(reinterpret_cast<void **>(&ws), off_tmp + aligned_up(sort_bytes > scan_bytes ? sort_bytes : scan_bytes)),
              "hipMalloc assembly workspace"))
    return last_error_code_only();
  unsigned long long *keys = reinterpret_cast<unsigned long long *>(ws);
  unsigned long long *sorted = reinterpret_cast<unsigned long long *>(ws + off_sorted);
  int *head = reinterpret_cast<int *>(ws); // (over the unsorted keys, once the sort has read them)
  int *index = head + count + 1;
  int *order = d_order ? d_order : reinterpret_cast<int *>(ws + off_order);
  int *start = d_start ? d_start : reinterpret_cast<int *>(ws + off_start);
  unsigned *d_slots = reinterpret_cast<unsigned *>(ws + off_slots);
  // every way out below passes here: the stream has run (or failed) before the workspace goes
  const auto leave = [&](int code) {
    (void)hipStreamSynchronize(st);
    (void)hipFree(ws);
    (void)hipGetLastError();
    return code;
  };
  std::vector<unsigned> slots(kCooCheckSlots, 0u);
  bool ok = hip_ok(hipMemsetAsync(d_slots, 0, sizeof(unsigned) * kCooCheckSlots, st), "zero the range census");
  if (ok) {
    launch_coo_check(st, d_row, d_col, nnz_coo, m, n, d_slots);
    ok = hip_ok(hipMemcpyAsync(slots.data(), d_slots, sizeof(unsigned) * kCooCheckSlots, hipMemcpyDeviceToHost, st), "read the range census") &&
         hip_ok(hipStreamSynchronize(st), "range census");
  }
  if (!ok) return leave(last_error_code_only());
  const unsigned long long bad = slot_sum(slots.data());
  if (bad != 0)
    return leave(entry_error(kEntry, kErrBadArgument,
                             std::to_string(bad) + " triples with a row outside [0, m) or a column outside [0, n): nothing was written"));
  launch_coo_keys(st, d_row, d_col, nnz_coo, col_bits, keys);
  if (!launch_coo_sort(st, keys, nnz_coo, key_bits, sorted, order, ws + off_tmp, &sort_bytes)) return leave(entry_error(kEntry, kErrHip, "radix sort failed"));
  launch_coo_heads(st, sorted, nnz_coo, head);
  if (!launch_coo_scan(st, head, nnz_coo, index, ws + off_tmp, &scan_bytes)) return leave(entry_error(kEntry, kErrHip, "scan failed"));
  int nnz = 0; // the number of runs: the values' launch is sized by it
  if (!hip_ok(hipMemcpyAsync(&nnz, index + count, sizeof(int), hipMemcpyDeviceToHost, st), "read the number of distinct positions") ||
      !hip_ok(hipStreamSynchronize(st), "sort and scan"))
    return leave(last_error_code_only());
  if (nnz < 1 || nnz > nnz_coo) return leave(entry_error(kEntry, kErrHip, "the scan of the run heads returned " + std::to_string(nnz)));
  launch_coo_entries(st, sorted, head, index, nnz_coo, col_bits, start, d_colindex);
  launch_coo_rowptr(st, sorted, index, nnz_coo, m, col_bits, d_rowptr);
  if (d_value) launch_coo_values(st, nnz_coo, nnz, order, start, d_val, d_value);
  if (const int rc = launch_error(kEntry)) return leave(rc);
  if (!hip_ok(hipStreamSynchronize(st), "assembly")) return leave(last_error_code_only());
  *h_nnz = nnz;
  return leave(kOk);
}

int run_coo_to_csr_values(int nnz_coo, int nnz, const int *d_order, const int *d_start, const double *d_val, double *d_value) {
  static const char *const kEntry = "spmv_acc_coo_to_csr_values";
  clear_error();
  apply_env_tunables();
  if (nnz_coo < 0 || nnz < 0) return entry_error(kEntry, kErrBadArgument, "negative nnz_coo or nnz");
  if (too_large(nnz_coo) || too_large(nnz)) return entry_error(kEntry, kErrTooLarge, "nnz_coo or nnz does not leave room for block arithmetic in int32");
  if (nnz > nnz_coo) return entry_error(kEntry, kErrBadArgument, "nnz > nnz_coo: more distinct positions than triples");
  if (nnz == 0) return kOk;
  if (!d_order || !d_start || !d_val || !d_value) return entry_error(kEntry, kErrBadArgument, "null order / start / val / value");
  hipStream_t st = t_stream;
  note_stream_use();
  launch_coo_values(st, nnz_coo, nnz, d_order, d_start, d_val, d_value);
  return launch_error(kEntry);
}

} // namespace spmv_acc
