// spgemm.cpp -- the three entries of the device CSR SpGEMM C = A * B (include/spmv_acc.h spmv_acc_csr_spgemm_products, spmv_acc_csr_spgemm,
// spmv_acc_csr_spgemm_values; kernels in k_spgemm.hip and, from the sort on, k_coo.hip; size rules and the two orders in spgemm.hpp).
//
// None makes, finds or touches a plan, and nothing derived from the caller's arrays survives a call: C and the map belong to the caller, who
// then runs any entry of the library on C.  The first product's values come from the values entry's kernel, so re-running the same values
// repeats its bits.  The count entry and the main entry are one routine: the count entry stops after the reduction.
#include "spgemm.hpp"
#include "engine_internal.hpp"
#include "entry_helpers.hpp"

namespace spmv_acc {

using namespace detail;

namespace {

const char *const kRowRanges = "; rows of C are independent: multiply row ranges of A";

// Both device entries.  h_nprod != nullptr: the count entry (B's columns, n and every output of the product are unused).
int spgemm_run(const char *kEntry, int m, int k, int n, int nnz_a, const int *d_a_rowptr, const int *d_a_colindex, const double *d_a_value,
               int nnz_b, const int *d_b_rowptr, const int *d_b_colindex, const double *d_b_value, int nprod, int *d_c_rowptr, int *d_c_colindex,
               double *d_c_value, int *d_pa, int *d_pb, int *d_start, int *h_nnz, long long *h_nprod) {
  const bool count_only = h_nprod != nullptr;
  clear_error();
  apply_env_tunables();
  if (m < 0 || k < 0 || n < 0 || nprod < 0) return entry_error(kEntry, kErrBadArgument, "negative m, k, n or nprod");
  if (!count_only) {
    if (!d_c_rowptr || !h_nnz) return entry_error(kEntry, kErrBadArgument, "null c_rowptr / h_nnz");
    if ((d_a_value == nullptr) != (d_c_value == nullptr) || (d_b_value == nullptr) != (d_c_value == nullptr))
      return entry_error(kEntry, kErrBadArgument, "a_value, b_value and c_value must all be given or all be NULL (structure only)");
    if ((d_pa == nullptr) != (d_start == nullptr) || (d_pb == nullptr) != (d_start == nullptr))
      return entry_error(kEntry, kErrBadArgument, "pa, pb and start must all be given or all be NULL (no map)");
  }
  if (too_large(m) || too_large(k) || too_large(n) || too_large(nnz_a) || too_large(nnz_b) ||
      too_large(nprod))
    return entry_error(kEntry, kErrTooLarge,
                       std::string("m, k, n, nnz_a, nnz_b or nprod does not leave room for block arithmetic in int32") + kRowRanges);
  const bool has_a = m > 0 && k > 0 && nnz_a != 0 && nnz_b != 0; // (otherwise no product exists, whatever the arrays hold)
  if (has_a && (!d_a_rowptr || !d_a_colindex || !d_b_rowptr)) return entry_error(kEntry, kErrBadArgument, "null a_rowptr / a_colindex / b_rowptr");
  if (has_a && !count_only && !d_b_colindex) return entry_error(kEntry, kErrBadArgument, "null b_colindex");
  if (!count_only && nprod > 0 && !d_c_colindex) return entry_error(kEntry, kErrBadArgument, "null c_colindex with nprod != 0");
  hipStream_t st = t_stream;
  note_stream_use();
  const ScopedSet<bool> capture_flag(t_capturing, stream_capturing(st));
  if (!plan_work_allowed("the product's workspace")) return last_error_code_only();
  if (has_a) { // rowptr[0] and rowptr[last] of both: the matrices must be rebased, and nnz_a / nnz_b are theirs
    int ends[4] = {0, 0, 0, 0};
    if (!hip_ok(hipMemcpyAsync(&ends[0], d_a_rowptr, sizeof(int), hipMemcpyDeviceToHost, st), "read a_rowptr[0]") ||
        !hip_ok(hipMemcpyAsync(&ends[1], d_a_rowptr + m, sizeof(int), hipMemcpyDeviceToHost, st), "read a_rowptr[m]") ||
        !hip_ok(hipMemcpyAsync(&ends[2], d_b_rowptr, sizeof(int), hipMemcpyDeviceToHost, st), "read b_rowptr[0]") ||
        !hip_ok(hipMemcpyAsync(&ends[3], d_b_rowptr + k, sizeof(int), hipMemcpyDeviceToHost, st), "read b_rowptr[k]") ||
        !hip_ok(hipStreamSynchronize(st), "read the ends of a_rowptr and b_rowptr"))
      return last_error_code_only();
    if (ends[0] != 0 || ends[2] != 0)
      return entry_error(kEntry, kErrBadArgument, "a_rowptr[0] != 0 or b_rowptr[0] != 0: an un-rebased row sub-range cannot be multiplied; rebase it first");
    if (ends[1] < 0 || (nnz_a >= 0 && ends[1] != nnz_a)) return entry_error(kEntry, kErrBadArgument, "nnz_a is not a_rowptr[m]");
    if (ends[3] < 0 || (nnz_b >= 0 && ends[3] != nnz_b)) return entry_error(kEntry, kErrBadArgument, "nnz_b is not b_rowptr[k]");
    nnz_a = ends[1];
    nnz_b = ends[3];
    if (too_large(nnz_a) || too_large(nnz_b))
      return entry_error(kEntry, kErrTooLarge, std::string("nnz_a or nnz_b does not leave room for block arithmetic in int32") + kRowRanges);
  }
  const auto no_products = [&]() { // d_c_rowptr is all zeros, nothing else is written
    if (count_only) {
      *h_nprod = 0;
      return static_cast<int>(kOk);
    }
    if (nprod != 0) return entry_error(kEntry, kErrBadArgument, "nprod is not the number of products, which is 0");
    if (!hip_ok(hipMemsetAsync(d_c_rowptr, 0, sizeof(int) * (static_cast<size_t>(m) + 1), st), "zero c_rowptr") ||
        !hip_ok(hipStreamSynchronize(st), "zero c_rowptr"))
      return last_error_code_only();
    *h_nnz = 0;
    return static_cast<int>(kOk);
  };
  if (!has_a || nnz_a <= 0 || nnz_b <= 0) return no_products();

  // one allocation.  Per non-zero of A: its count and the scan (8 B each), its row (4 B).  Per product (the caller's nprod: checked against the
  // scan before anything of that size is written): the packed keys (after the sort: the run-head flags and their scan) and the sorted keys, 8 B
  // each; pa, pb and start when the caller wants no map.  The two census slot arrays, one 64-bit total, and the scratch of the reduction, the two
  // scans and the sort (they run one after the other)
  const int col_bits = coo_index_bits(n), key_bits = coo_index_bits(m) + col_bits;
  const size_t count = static_cast<size_t>(nprod), na = static_cast<size_t>(nnz_a);
  size_t reduce_bytes = 0, off_bytes = 0, sort_bytes = 0, scan_bytes = 0;
  bool sized = count_only ? launch_spgemm_reduce(st, nullptr, nnz_a, nullptr, nullptr, &reduce_bytes)
                          : launch_spgemm_scan(st, nullptr, nnz_a, nullptr, nullptr, &off_bytes);
  if (sized && !count_only && nprod > 0)
    sized = launch_coo_sort(st, nullptr, nprod, key_bits, nullptr, nullptr, nullptr, &sort_bytes) &&
            launch_coo_scan(st, nullptr, nprod, nullptr, nullptr, &scan_bytes);
  if (!sized) {
    (void)hipGetLastError();
    return entry_error(kEntry, kErrHip, "reduction / scan / radix sort workspace query failed");
  }
  const size_t tmp_bytes = std::max(std::max(reduce_bytes, off_bytes), std::max(sort_bytes, scan_bytes));
  const size_t longs = aligned_up(sizeof(long long) * (na + 1)), slots_bytes = aligned_up(sizeof(unsigned) * kCooCheckSlots);
  const size_t keys_bytes = count_only ? 0 : aligned_up(sizeof(unsigned long long) * (count + 1)); // (+ 1: room for the two int arrays of count + 1 that follow)
  const size_t ints = count_only ? 0 : aligned_up(sizeof(int) * (count + 1));
  const size_t off_off = longs, off_arow = off_off + longs, off_slots_a = off_arow + aligned_up(sizeof(int) * na);
  const size_t off_slots_b = off_slots_a + slots_bytes, off_total = off_slots_b + slots_bytes, off_keys = off_total + kEntryAlign;
  const size_t off_sorted = off_keys + keys_bytes, off_pa = off_sorted + keys_bytes, off_pb = off_pa + (d_pa ? 0 : ints);
  const size_t off_start = off_pb + (d_pb ? 0 : ints), off_tmp = off_start + (d_start ? 0 : ints);
  char *ws = nullptr;
  if (!hip_ok(hipMalloc(reinterpret_cast<void **>(&ws), off_tmp + aligned_up(tmp_bytes)), "hipMalloc product workspace")) return last_error_code_only();
  long long *counts = reinterpret_cast<long long *>(ws);
  long long *off = reinterpret_cast<long long *>(ws + off_off);
  int *arow = reinterpret_cast<int *>(ws + off_arow);
  unsigned *d_slots_a = reinterpret_cast<unsigned *>(ws + off_slots_a);
  long long *d_total = reinterpret_cast<long long *>(ws + off_total);
  unsigned long long *keys = reinterpret_cast<unsigned long long *>(ws + off_keys);
  unsigned long long *sorted = reinterpret_cast<unsigned long long *>(ws + off_sorted);
  int *head = reinterpret_cast<int *>(ws + off_keys); // (over the unsorted keys, once the sort has read them)
  int *index = head + count + 1;
  int *pa = d_pa ? d_pa : reinterpret_cast<int *>(ws + off_pa);
  int *pb = d_pb ? d_pb : reinterpret_cast<int *>(ws + off_pb);
  int *start = d_start ? d_start : reinterpret_cast<int *>(ws + off_start);
  // every way out below passes here: the stream has run (or failed) before the workspace goes
  const auto leave = [&](int code) {
    (void)hipStreamSynchronize(st);
    (void)hipFree(ws);
    (void)hipGetLastError();
    return code;
  };
  // the range census, before anything reads through a column: A's against [0, k), B's (main entry) against [0, n)
  std::vector<unsigned> slots(2 * kCooCheckSlots, 0u);
  bool ok = hip_ok(hipMemsetAsync(d_slots_a, 0, 2 * slots_bytes, st), "zero the range census");
  if (ok) {
    launch_coo_check(st, d_a_colindex, d_a_colindex, nnz_a, k, k, d_slots_a);
    if (!count_only) launch_coo_check(st, d_b_colindex, d_b_colindex, nnz_b, n, n, reinterpret_cast<unsigned *>(ws + off_slots_b));
    ok = hip_ok(hipMemcpyAsync(slots.data(), d_slots_a, sizeof(unsigned) * kCooCheckSlots, hipMemcpyDeviceToHost, st), "read the range census") &&
         hip_ok(hipMemcpyAsync(slots.data() + kCooCheckSlots, ws + off_slots_b, sizeof(unsigned) * kCooCheckSlots, hipMemcpyDeviceToHost, st),
                "read the range census") &&
         hip_ok(hipStreamSynchronize(st), "range census");
  }
  if (!ok) return leave(last_error_code_only());
  const unsigned long long bad_a = slot_sum(slots.data()), bad_b = slot_sum(slots.data() + kCooCheckSlots);
  if (bad_a != 0 || bad_b != 0)
    return leave(entry_error(kEntry, kErrBadArgument,
                             std::to_string(bad_a) + " columns of A outside [0, k) and " + std::to_string(bad_b) +
                                 " columns of B outside [0, n): nothing was written"));
  // the products of every non-zero of A and their total
  long long total = -1;
  launch_spgemm_counts(st, m, nnz_a, d_a_rowptr, d_a_colindex, d_b_rowptr, nnz_b, counts, count_only ? nullptr : arow);
  if (count_only ? !launch_spgemm_reduce(st, counts, nnz_a, d_total, ws + off_tmp, &reduce_bytes)
                 : !launch_spgemm_scan(st, counts, nnz_a, off, ws + off_tmp, &off_bytes))
    return leave(entry_error(kEntry, kErrHip, "reduction / scan of the product counts failed"));
  if (!hip_ok(hipMemcpyAsync(&total, count_only ? d_total : off + na, sizeof(long long), hipMemcpyDeviceToHost, st), "read the number of products") ||
      !hip_ok(hipStreamSynchronize(st), "product counts"))
    return leave(last_error_code_only());
  if (total < 0) return leave(entry_error(kEntry, kErrHip, "the product counts add up to " + std::to_string(total)));
  if (count_only) *h_nprod = total; // (returned even when it is too large for the main entry)
  if (too_large(total))
    return leave(entry_error(kEntry, kErrTooLarge,
                             std::to_string(total) + " products do not leave room for block arithmetic in int32" + kRowRanges +
                                 (count_only ? "" : ": nothing was written")));
  if (count_only) return leave(kOk);
  if (total != nprod)
    return leave(entry_error(kEntry, kErrBadArgument,
                             "nprod is not the number of products, which is " + std::to_string(total) + ": nothing was written"));
  if (nprod == 0) return leave(no_products()); // (A only meets empty rows of B)

  launch_spgemm_expand(st, nnz_a, nprod, off, arow, d_a_colindex, d_b_rowptr, nnz_b, d_b_colindex, col_bits, keys);
  if (!launch_coo_sort(st, keys, nprod, key_bits, sorted, pa, ws + off_tmp, &sort_bytes)) return leave(entry_error(kEntry, kErrHip, "radix sort failed"));
  launch_coo_heads(st, sorted, nprod, head);
  if (!launch_coo_scan(st, head, nprod, index, ws + off_tmp, &scan_bytes)) return leave(entry_error(kEntry, kErrHip, "scan failed"));
  int nnz_c = 0; // the number of runs: the values' launch is sized by it
  if (!hip_ok(hipMemcpyAsync(&nnz_c, index + count, sizeof(int), hipMemcpyDeviceToHost, st), "read the number of distinct positions") ||
      !hip_ok(hipStreamSynchronize(st), "sort and scan"))
    return leave(last_error_code_only());
  if (nnz_c < 1 || nnz_c > nprod) return leave(entry_error(kEntry, kErrHip, "the scan of the run heads returned " + std::to_string(nnz_c)));
  launch_coo_entries(st, sorted, head, index, nprod, col_bits, start, d_c_colindex);
  launch_coo_rowptr(st, sorted, index, nprod, m, col_bits, d_c_rowptr);
  if (d_pa || d_c_value) launch_spgemm_map(st, m, nnz_a, nprod, sorted, col_bits, off, d_a_rowptr, d_a_colindex, d_b_rowptr, nnz_b, pa, pb);
  if (d_c_value) launch_spgemm_values(st, nprod, nnz_c, pa, pb, start, d_a_value, d_b_value, d_c_value);
  if (const int rc = launch_error(kEntry)) return leave(rc);
  if (!hip_ok(hipStreamSynchronize(st), "product")) return leave(last_error_code_only());
  *h_nnz = nnz_c;
  return leave(kOk);
}

} // namespace

int run_csr_spgemm_products(int m, int k, int nnz_a, const int *d_a_rowptr, const int *d_a_colindex, const int *d_b_rowptr, long long *h_nprod) {
  static const char *const kEntry = "spmv_acc_csr_spgemm_products";
  if (!h_nprod) {
    clear_error();
    return entry_error(kEntry, kErrBadArgument, "null h_nprod");
  }
  return spgemm_run(kEntry, m, k, 0, nnz_a, d_a_rowptr, d_a_colindex, nullptr, -1, d_b_rowptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr,
                    nullptr, nullptr, nullptr, nullptr, h_nprod);
}

int run_csr_spgemm(int m, int k, int n, int nnz_a, const int *d_a_rowptr, const int *d_a_colindex, const double *d_a_value, int nnz_b,
                   const int *d_b_rowptr, const int *d_b_colindex, const double *d_b_value, int nprod, int *d_c_rowptr, int *d_c_colindex,
                   double *d_c_value, int *d_pa, int *d_pb, int *d_start, int *h_nnz) {
  static const char *const kEntry = "spmv_acc_csr_spgemm";
  return spgemm_run(kEntry, m, k, n, nnz_a, d_a_rowptr, d_a_colindex, d_a_value, nnz_b, d_b_rowptr, d_b_colindex, d_b_value, nprod, d_c_rowptr,
                    d_c_colindex, d_c_value, d_pa, d_pb, d_start, h_nnz, nullptr);
}

int run_csr_spgemm_values(int nprod, int nnz_c, const int *d_pa, const int *d_pb, const int *d_start, const double *d_a_value,
                          const double *d_b_value, double *d_c_value) {
  static const char *const kEntry = "spmv_acc_csr_spgemm_values";
  clear_error();
  apply_env_tunables();
  if (nprod < 0 || nnz_c < 0) return entry_error(kEntry, kErrBadArgument, "negative nprod or nnz_c");
  if (too_large(nprod) || too_large(nnz_c))
    return entry_error(kEntry, kErrTooLarge, "nprod or nnz_c does not leave room for block arithmetic in int32");
  if (nnz_c > nprod) return entry_error(kEntry, kErrBadArgument, "nnz_c > nprod: more entries than products");
  if (nnz_c == 0) return kOk;
  if (!d_pa || !d_pb || !d_start || !d_a_value || !d_b_value || !d_c_value)
    return entry_error(kEntry, kErrBadArgument, "null pa / pb / start / a_value / b_value / c_value");
  hipStream_t st = t_stream;
  note_stream_use();
  launch_spgemm_values(st, nprod, nnz_c, d_pa, d_pb, d_start, d_a_value, d_b_value, d_c_value);
  return launch_error(kEntry);
}

} // namespace spmv_acc
