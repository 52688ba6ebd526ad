// extract.cpp -- the two entries of the device CSR extraction C = A[rows, colmap] with a diagonal band (include/spmv_acc.h spmv_acc_csr_extract,
// spmv_acc_csr_extract_values; kernels in k_extract.hip; the definition, the steps and the size rules in extract.hpp).
//
// Neither makes, finds or touches a plan, and nothing derived from the caller's arrays survives a call: C and the map belong to the caller, who
// then runs any entry of the library on C.  The first call's values come from the values entry's kernel, so re-running the same values repeats
// its bits.
#include "extract.hpp"
#include "engine_internal.hpp"
#include "entry_helpers.hpp"

namespace spmv_acc {

using namespace detail;

namespace {

constexpr int kExtractCounts = 7; // count groups of kCooCheckSlots: the census' five, the candidates' columns, the descents

const char *const kExtractRowRanges = "; rows of C are independent: extract row ranges";

} // namespace

int run_csr_extract(int m, int n, int nnz_a, const int *d_a_rowptr, const int *d_a_colindex, const double *d_a_value, int mc, const int *d_rows,
                    int nc, const int *d_colmap, int diag_lo, int diag_hi, int *d_c_rowptr, int *d_c_colindex, double *d_c_value, int *d_map,
                    int *h_nnz) {
  static const char *const kEntry = "spmv_acc_csr_extract";
  clear_error();
  apply_env_tunables();
  if (m < 0 || n < 0 || mc < 0 || nc < 0) return entry_error(kEntry, kErrBadArgument, "negative m, n, mc or nc");
  if (!d_c_rowptr || !h_nnz) return entry_error(kEntry, kErrBadArgument, "null c_rowptr / h_nnz");
  if ((d_a_value == nullptr) != (d_c_value == nullptr))
    return entry_error(kEntry, kErrBadArgument, "a_value and c_value must both be given or both be NULL (structure only)");
  if (too_large(m) || too_large(n) || too_large(mc) || too_large(nc) || too_large(nnz_a))
    return entry_error(kEntry, kErrTooLarge, std::string("m, n, mc, nc or nnz_a does not leave room for block arithmetic in int32") + kExtractRowRanges);
  if (!d_rows && mc != m) return entry_error(kEntry, kErrBadArgument, "rows == NULL selects every row: mc must equal m");
  if (!d_colmap && nc != n) return entry_error(kEntry, kErrBadArgument, "colmap == NULL is the identity: nc must equal n");
  if (m > 0 && mc > 0 && !d_a_rowptr) return entry_error(kEntry, kErrBadArgument, "null a_rowptr");
  if (m > 0 && mc > 0 && nnz_a != 0 && (!d_a_colindex || !d_c_colindex))
    return entry_error(kEntry, kErrBadArgument, "null a_colindex / c_colindex of a matrix with non-zeros");
  hipStream_t st = t_stream;
  note_stream_use();
  const ScopedSet<bool> capture_flag(t_capturing, stream_capturing(st));
  if (!plan_work_allowed("the extraction's workspace")) return last_error_code_only();
  const auto zero_rowptr = [&]() {
    return hip_ok(hipMemsetAsync(d_c_rowptr, 0, sizeof(int) * (static_cast<size_t>(mc) + 1), st), "zero c_rowptr") &&
           hip_ok(hipStreamSynchronize(st), "zero c_rowptr");
  };
  const auto nothing_to_extract = [&]() { // d_c_rowptr is all zeros, nothing else is written, nothing is allocated
    if (!zero_rowptr()) return last_error_code_only();
    *h_nnz = 0;
    return static_cast<int>(kOk);
  };
  if (m == 0) {
    if (nnz_a > 0) return entry_error(kEntry, kErrBadArgument, "nnz_a is not a_rowptr[m], which is 0 without rows");
    return nothing_to_extract();
  }
  if (mc == 0) return nothing_to_extract();
  { // a_rowptr[0] and a_rowptr[m]: the matrix must be rebased, and nnz_a is its
    int ends[2] = {0, 0};
    if (!hip_ok(hipMemcpyAsync(&ends[0], d_a_rowptr, sizeof(int), hipMemcpyDeviceToHost, st), "read a_rowptr[0]") ||
        !hip_ok(hipMemcpyAsync(&ends[1], d_a_rowptr + m, sizeof(int), hipMemcpyDeviceToHost, st), "read a_rowptr[m]") ||
        !hip_ok(hipStreamSynchronize(st), "read the ends of a_rowptr"))
      return last_error_code_only();
    if (ends[0] != 0)
      return entry_error(kEntry, kErrBadArgument, "a_rowptr[0] != 0: an un-rebased row sub-range cannot be extracted from; rebase it first");
    if (ends[1] < 0 || (nnz_a >= 0 && ends[1] != nnz_a)) return entry_error(kEntry, kErrBadArgument, "nnz_a is not a_rowptr[m]");
    nnz_a = ends[1];
    if (too_large(nnz_a))
      return entry_error(kEntry, kErrTooLarge, std::string("nnz_a does not leave room for block arithmetic in int32") + kExtractRowRanges);
    if (nnz_a != 0 && (!d_a_colindex || !d_c_colindex))
      return entry_error(kEntry, kErrBadArgument, "null a_colindex / c_colindex of a matrix with non-zeros");
  }
  if (nnz_a == 0) return nothing_to_extract();

  // three allocations, each sized once its count is known, all freed in leave().
  // 1. by rows and columns: the marks (4 B per row of A with rows, 4 B per column of C with colmap), the selected rows' lengths and their scan
  //    (8 B per row of C), the seven count groups, the scan's scratch
  // 2. by candidates S: newcol and its scan, 4 B each (+ 1); the map, 4 B, when the caller wants values but no map; the scan's scratch
  // 3. only when a row of the compaction descends, by C entries: the keys and the sorted keys, 8 B each, the order, 4 B, a copy of the map,
  //    4 B, where one is written; the radix sort's scratch
  char *ws_rows = nullptr, *ws_cand = nullptr, *ws_sort = nullptr;
  // every way out below passes here: the stream has run (or failed) before the workspace goes
  const auto leave = [&](int code) {
    (void)hipStreamSynchronize(st);
    (void)hipFree(ws_rows);
    (void)hipFree(ws_cand);
    (void)hipFree(ws_sort);
    (void)hipGetLastError();
    return code;
  };
  const size_t rows_c = static_cast<size_t>(mc) + 1;
  size_t scan_rows_bytes = 0;
  if (!launch_extract_scan(st, nullptr, rows_c, nullptr, nullptr, &scan_rows_bytes)) {
    (void)hipGetLastError();
    return entry_error(kEntry, kErrHip, "scan workspace query failed");
  }
  const size_t inv_row_bytes = d_rows ? aligned_up(sizeof(int) * static_cast<size_t>(m)) : 0;
  const size_t inv_col_bytes = d_colmap ? aligned_up(sizeof(int) * static_cast<size_t>(nc)) : 0;
  const size_t ptr_bytes = aligned_up(sizeof(int) * rows_c), slots_bytes = aligned_up(sizeof(unsigned) * kExtractCounts * kCooCheckSlots);
  const size_t off_inv_col = inv_row_bytes, off_len = off_inv_col + inv_col_bytes, off_src = off_len + ptr_bytes, off_slots = off_src + ptr_bytes,
               off_tmp_rows = off_slots + slots_bytes;
  if (!hip_ok(hipMalloc(reinterpret_cast<void **>(&ws_rows), off_tmp_rows + aligned_up(scan_rows_bytes)), "hipMalloc extraction workspace"))
    return leave(last_error_code_only());
  int *inv_row = d_rows ? reinterpret_cast<int *>(ws_rows) : nullptr;
  int *inv_col = d_colmap ? reinterpret_cast<int *>(ws_rows + off_inv_col) : nullptr;
  int *len = reinterpret_cast<int *>(ws_rows + off_len);
  int *src_ptr = reinterpret_cast<int *>(ws_rows + off_src);
  unsigned *d_slots = reinterpret_cast<unsigned *>(ws_rows + off_slots);
  // the census of rows and colmap, before anything reads through them
  std::vector<unsigned> slots(static_cast<size_t>(5) * kCooCheckSlots, 0u);
  int S = -1;
  bool ok = hip_ok(hipMemsetAsync(d_slots, 0, sizeof(unsigned) * kExtractCounts * kCooCheckSlots, st), "zero the census");
  if (ok) {
    launch_extract_mark(st, mc, m, d_rows, inv_row, n, nc, d_colmap, inv_col);
    launch_extract_census(st, mc, m, nnz_a, d_rows, d_a_rowptr, inv_row, n, nc, d_colmap, inv_col, len, d_slots);
    if (!launch_extract_scan(st, len, rows_c, src_ptr, ws_rows + off_tmp_rows, &scan_rows_bytes))
      return leave(entry_error(kEntry, kErrHip, "scan of the selected rows' lengths failed"));
    ok = hip_ok(hipMemcpyAsync(slots.data(), d_slots, sizeof(unsigned) * 5 * kCooCheckSlots, hipMemcpyDeviceToHost, st), "read the census") &&
         hip_ok(hipMemcpyAsync(&S, src_ptr + mc, sizeof(int), hipMemcpyDeviceToHost, st), "read the number of candidates") &&
         hip_ok(hipStreamSynchronize(st), "census");
  }
  if (!ok) return leave(last_error_code_only());
  unsigned long long bad[5] = {0, 0, 0, 0, 0}, any_bad = 0;
  for (int g = 0; g < 5; ++g) {
    bad[g] = slot_sum(slots.data() + static_cast<size_t>(g) * kCooCheckSlots);
    any_bad += bad[g];
  }
  if (any_bad != 0) {
    return leave(entry_error(kEntry, kErrBadArgument,
                             std::to_string(bad[0]) + " rows outside [0, m), " + std::to_string(bad[1]) + " repeated rows, " + std::to_string(bad[2]) +
                                 " selected rows with a descending or out-of-range rowptr extent, " + std::to_string(bad[3]) +
                                 " colmap values >= nc, " + std::to_string(bad[4]) + " repeated colmap values: nothing was written"));
  }
  if (S < 0 || S > nnz_a) return leave(entry_error(kEntry, kErrHip, "the scan of the selected rows' lengths returned " + std::to_string(S)));
  const auto nothing_kept = [&]() { // as nothing_to_extract, from inside the allocations
    if (!zero_rowptr()) return leave(last_error_code_only());
    *h_nnz = 0;
    return leave(kOk);
  };
  if (S == 0) return nothing_kept();

  // candidates
  const size_t cand = static_cast<size_t>(S) + 1;
  size_t scan_cand_bytes = 0;
  if (!launch_extract_scan_kept(st, nullptr, cand, nullptr, nullptr, &scan_cand_bytes)) return leave(entry_error(kEntry, kErrHip, "scan workspace query failed"));
  const bool own_map = d_map == nullptr && d_c_value != nullptr; // (structure only and no map: no map is written at all)
  const size_t cand_bytes = aligned_up(sizeof(int) * cand), own_map_bytes = own_map ? aligned_up(sizeof(int) * cand) : 0;
  const size_t off_pos = cand_bytes, off_map = off_pos + cand_bytes, off_tmp_cand = off_map + own_map_bytes;
  if (!hip_ok(hipMalloc(reinterpret_cast<void **>(&ws_cand), off_tmp_cand + aligned_up(scan_cand_bytes)), "hipMalloc candidate workspace"))
    return leave(last_error_code_only());
  int *newcol = reinterpret_cast<int *>(ws_cand);
  int *pos = reinterpret_cast<int *>(ws_cand + off_pos);
  int *map = own_map ? reinterpret_cast<int *>(ws_cand + off_map) : d_map;
  unsigned *d_columns = d_slots + static_cast<size_t>(5) * kCooCheckSlots, *d_descents = d_slots + static_cast<size_t>(6) * kCooCheckSlots;
  int nnz_c = -1;
  slots.assign(kCooCheckSlots, 0u);
  launch_extract_candidates(st, mc, nnz_a, S, d_rows, d_a_rowptr, d_a_colindex, src_ptr, n, d_colmap, diag_lo, diag_hi, newcol, d_columns);
  if (!launch_extract_scan_kept(st, newcol, cand, pos, ws_cand + off_tmp_cand, &scan_cand_bytes))
    return leave(entry_error(kEntry, kErrHip, "scan of the kept candidates failed"));
  if (!hip_ok(hipMemcpyAsync(slots.data(), d_columns, sizeof(unsigned) * kCooCheckSlots, hipMemcpyDeviceToHost, st), "read the column census") ||
      !hip_ok(hipMemcpyAsync(&nnz_c, pos + S, sizeof(int), hipMemcpyDeviceToHost, st), "read the number of kept candidates") ||
      !hip_ok(hipStreamSynchronize(st), "candidates and scan"))
    return leave(last_error_code_only());
  const unsigned long long bad_columns = slot_sum(slots.data());
  if (bad_columns != 0)
    return leave(entry_error(kEntry, kErrBadArgument,
                             std::to_string(bad_columns) + " candidates with a column outside [0, n): nothing was written"));
  if (nnz_c < 0 || nnz_c > S) return leave(entry_error(kEntry, kErrHip, "the scan of the kept candidates returned " + std::to_string(nnz_c)));
  if (nnz_c == 0) return nothing_kept();

  // the compaction, and whether it is the answer
  launch_extract_rowptr(st, mc, src_ptr, pos, d_c_rowptr);
  launch_extract_scatter(st, mc, nnz_a, S, nnz_a, d_rows, d_a_rowptr, src_ptr, newcol, pos, d_c_colindex, map);
  launch_extract_descents(st, mc, nnz_c, d_c_rowptr, d_c_colindex, d_descents);
  slots.assign(kCooCheckSlots, 0u);
  if (!hip_ok(hipMemcpyAsync(slots.data(), d_descents, sizeof(unsigned) * kCooCheckSlots, hipMemcpyDeviceToHost, st), "read the descents") ||
      !hip_ok(hipStreamSynchronize(st), "compaction"))
    return leave(last_error_code_only());
  const unsigned long long descents = slot_sum(slots.data());
  if (descents != 0) { // some row is not ascending: one stable sort by (row, column)
    const int col_bits = coo_index_bits(nc), key_bits = coo_index_bits(mc) + col_bits;
    const size_t count = static_cast<size_t>(nnz_c);
    size_t sort_bytes = 0;
    if (!launch_coo_sort(st, nullptr, nnz_c, key_bits, nullptr, nullptr, nullptr, &sort_bytes))
      return leave(entry_error(kEntry, kErrHip, "radix sort workspace query failed"));
    const size_t keys_bytes = aligned_up(sizeof(unsigned long long) * count), ints = aligned_up(sizeof(int) * count);
    const size_t off_sorted = keys_bytes, off_order = off_sorted + keys_bytes, off_map_tmp = off_order + ints, off_tmp_sort = off_map_tmp + (map ? ints : 0);
    if (!hip_ok(hipMalloc(reinterpret_cast<void **>(&ws_sort), off_tmp_sort + aligned_up(sort_bytes)), "hipMalloc sort workspace"))
      return leave(last_error_code_only());
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(ws_sort);
    unsigned long long *sorted = reinterpret_cast<unsigned long long *>(ws_sort + off_sorted);
    int *order = reinterpret_cast<int *>(ws_sort + off_order);
    int *map_tmp = map ? reinterpret_cast<int *>(ws_sort + off_map_tmp) : nullptr;
    if (map && !hip_ok(hipMemcpyAsync(map_tmp, map, sizeof(int) * count, hipMemcpyDeviceToDevice, st), "copy the compaction's map"))
      return leave(last_error_code_only());
    launch_extract_keys(st, mc, nnz_c, d_c_rowptr, d_c_colindex, col_bits, keys);
    if (!launch_coo_sort(st, keys, nnz_c, key_bits, sorted, order, ws_sort + off_tmp_sort, &sort_bytes))
      return leave(entry_error(kEntry, kErrHip, "radix sort failed"));
    launch_extract_sorted(st, nnz_c, sorted, col_bits, order, map_tmp, d_c_colindex, map);
  }
  if (d_c_value) launch_extract_values(st, nnz_c, nnz_a, map, d_a_value, d_c_value);
  if (const int rc = launch_error(kEntry)) return leave(rc);
  if (!hip_ok(hipStreamSynchronize(st), "extraction")) return leave(last_error_code_only());
  *h_nnz = nnz_c;
  return leave(kOk);
}

int run_csr_extract_values(int nnz_c, int nnz_a, const int *d_map, const double *d_a_value, double *d_c_value) {
  static const char *const kEntry = "spmv_acc_csr_extract_values";
  clear_error();
  apply_env_tunables();
  if (nnz_c < 0 || nnz_a < 0) return entry_error(kEntry, kErrBadArgument, "negative nnz_c or nnz_a");
  if (too_large(nnz_c) || too_large(nnz_a))
    return entry_error(kEntry, kErrTooLarge, "nnz_c or nnz_a does not leave room for block arithmetic in int32");
  if (nnz_c == 0) return kOk;
  if (!d_map || !d_c_value || (nnz_a > 0 && !d_a_value))
    return entry_error(kEntry, kErrBadArgument, "null map / c_value, or null a_value of a matrix with non-zeros");
  hipStream_t st = t_stream;
  note_stream_use();
  launch_extract_values(st, nnz_c, nnz_a, d_map, d_a_value, d_c_value);
  return launch_error(kEntry);
}

} // namespace spmv_acc
