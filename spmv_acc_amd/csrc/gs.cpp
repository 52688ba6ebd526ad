// gs.cpp -- the two entries of the multicolour Gauss-Seidel / SOR smoother (include/spmv_acc.h spmv_acc_csr_color, spmv_acc_csr_gs_sweep;
// kernels in k_gs.hip; the colouring's definition, the sweep's summation order and the size rules in gs.hpp).
//
// Neither makes, finds or touches a plan, and nothing derived from the caller's arrays survives a call: the colours belong to the caller, who
// hands them back to the sweep.  The sweep is launch-only: one kernel per non-empty colour, nothing else.
#include "gs.hpp"
#include "engine_internal.hpp"
#include "entry_helpers.hpp"

namespace spmv_acc {

using namespace detail;

int run_csr_color(int m, int nnz, const int *d_rowptr, const int *d_colindex, int *d_color, int *d_color_rows, int cap_colors, int *h_color_ptr,
                  int *h_ncolors, int *h_no_diag) {
  static const char *const kEntry = "spmv_acc_csr_color";
  clear_error();
  apply_env_tunables();
  if (m < 0 || nnz < 0) return entry_error(kEntry, kErrBadArgument, "negative m or nnz");
  if (cap_colors < 1) return entry_error(kEntry, kErrBadArgument, "cap_colors < 1");
  if (!h_color_ptr || !h_ncolors || !h_no_diag) return entry_error(kEntry, kErrBadArgument, "null h_color_ptr / h_ncolors / h_no_diag");
  if (m > 0 && (!d_rowptr || !d_color || !d_color_rows)) return entry_error(kEntry, kErrBadArgument, "null rowptr / color / color_rows");
  if (m > 0 && nnz > 0 && !d_colindex) return entry_error(kEntry, kErrBadArgument, "null colindex of a matrix with non-zeros");
  if (too_large(m) || too_large(nnz))
    return entry_error(kEntry, kErrTooLarge, "m or nnz does not leave room for block arithmetic in int32");
  hipStream_t st = t_stream;
  note_stream_use();
  const ScopedSet<bool> capture_flag(t_capturing, stream_capturing(st));
  if (!plan_work_allowed("the colouring's workspace")) return last_error_code_only();
  if (m == 0) {
    if (nnz > 0) return entry_error(kEntry, kErrBadArgument, "nnz is not rowptr[m], which is 0 without rows");
    h_color_ptr[0] = 0;
    *h_ncolors = 0;
    *h_no_diag = 0;
    return kOk;
  }

  // one allocation, freed in leave(): the count groups, the second colour array (4 B per row), the keys and the sorted keys (8 B each), the
  // colour pointer on the device (at most 4 B per row), the radix sort's scratch
  char *ws = nullptr;
  // every way out below passes here: the stream has run (or failed) before the workspace goes
  const auto leave = [&](int code) {
    (void)hipStreamSynchronize(st);
    (void)hipFree(ws);
    (void)hipGetLastError();
    return code;
  };
  const int key_bits = coo_index_bits(m); // (a colour is at most the row's degree: below m)
  const int ptr_count = (cap_colors < m ? cap_colors : m) + 1;
  size_t sort_bytes = 0;
  if (!launch_coo_sort(st, nullptr, m, key_bits, nullptr, nullptr, nullptr, &sort_bytes)) {
    (void)hipGetLastError();
    return entry_error(kEntry, kErrHip, "radix sort workspace query failed");
  }
  const size_t rows = static_cast<size_t>(m);
  const size_t slots_bytes = aligned_up(sizeof(unsigned) * kGsCounts * kCooCheckSlots), ints = aligned_up(sizeof(int) * rows),
               keys_bytes = aligned_up(sizeof(unsigned long long) * rows), ptr_bytes = aligned_up(sizeof(int) * static_cast<size_t>(ptr_count));
  const size_t off_other = slots_bytes, off_keys = off_other + ints, off_sorted = off_keys + keys_bytes, off_ptr = off_sorted + keys_bytes,
               off_tmp = off_ptr + ptr_bytes;
  if (!hip_ok(hipMalloc(reinterpret_cast<void **>(&ws), off_tmp + aligned_up(sort_bytes)), "hipMalloc colouring workspace"))
    return leave(last_error_code_only());
  unsigned *d_slots = reinterpret_cast<unsigned *>(ws);
  int *other = reinterpret_cast<int *>(ws + off_other);
  unsigned long long *keys = reinterpret_cast<unsigned long long *>(ws + off_keys);
  unsigned long long *sorted = reinterpret_cast<unsigned long long *>(ws + off_sorted);
  int *d_ptr = reinterpret_cast<int *>(ws + off_ptr);

  // the census, before anything is written
  unsigned long long no_diag = 0;
  if (const int rc = pattern_census(st, kEntry, m, nnz, d_rowptr, d_colindex, d_slots, "colour the pattern of A + A^T instead", &no_diag))
    return leave(rc);

  // the rounds: the caller's array and the workspace's take turns, kGsRoundsPerRead (even) rounds between two reads
  if (!hip_ok(hipMemsetAsync(d_color, 0xFF, sizeof(int) * rows, st), "uncolour the rows")) return leave(last_error_code_only());
  std::vector<unsigned> slots(kCooCheckSlots, 0u);
  unsigned long long remaining = static_cast<unsigned long long>(m);
  while (remaining != 0) {
    for (int r = 0; r < kGsRoundsPerRead; r += 2) {
      launch_gs_round(st, m, nnz, d_rowptr, d_colindex, d_color, other, d_slots);
      launch_gs_round(st, m, nnz, d_rowptr, d_colindex, other, d_color, d_slots);
    }
    if (!hip_ok(hipMemcpyAsync(slots.data(), d_slots, sizeof(unsigned) * kCooCheckSlots, hipMemcpyDeviceToHost, st), "read the uncoloured count") ||
        !hip_ok(hipStreamSynchronize(st), "colouring rounds"))
      return leave(last_error_code_only());
    const unsigned long long now = slot_sum(slots.data());
    if (now >= remaining) // (cannot happen on a pattern that passed the census: the uncoloured row of highest priority never waits)
      return leave(entry_error(kEntry, kErrHip, std::to_string(kGsRoundsPerRead) + " rounds coloured no row while " + std::to_string(now) +
                                                    " remain: no further round is issued"));
    remaining = now;
  }

  // color_rows = the order of a stable sort by colour; the colour pointer from the sorted keys
  unsigned long long last_key = 0;
  std::vector<int> ptr(static_cast<size_t>(ptr_count), 0);
  launch_gs_keys(st, m, d_color, keys);
  if (!launch_coo_sort(st, keys, m, key_bits, sorted, d_color_rows, ws + off_tmp, &sort_bytes))
    return leave(entry_error(kEntry, kErrHip, "radix sort failed"));
  launch_gs_color_ptr(st, m, sorted, ptr_count, d_ptr);
  if (const int rc = launch_error(kEntry)) return leave(rc);
  if (!hip_ok(hipMemcpyAsync(&last_key, sorted + (rows - 1), sizeof(last_key), hipMemcpyDeviceToHost, st), "read the largest colour") ||
      !hip_ok(hipMemcpyAsync(ptr.data(), d_ptr, sizeof(int) * static_cast<size_t>(ptr_count), hipMemcpyDeviceToHost, st), "read the colour pointer") ||
      !hip_ok(hipStreamSynchronize(st), "colouring"))
    return leave(last_error_code_only());
  if (last_key >= static_cast<unsigned long long>(m)) return leave(entry_error(kEntry, kErrHip, "the sort returned the colour " + std::to_string(last_key)));
  const int ncolors = static_cast<int>(last_key) + 1;
  *h_ncolors = ncolors;
  *h_no_diag = static_cast<int>(no_diag);
  if (ncolors > cap_colors)
    return leave(entry_error(kEntry, kErrTooLarge, std::to_string(ncolors) + " colours, h_color_ptr holds " + std::to_string(cap_colors) +
                                                       ": color and *h_ncolors are valid, call again with a larger array"));
  for (int c = 0; c <= ncolors; ++c) h_color_ptr[c] = ptr[static_cast<size_t>(c)];
  return leave(kOk);
}

int run_csr_gs_sweep(int m, int nnz, const int *d_rowptr, const int *d_colindex, const double *d_value, int ncolors, const int *h_color_ptr,
                     const int *d_color_rows, double omega, int direction, const double *d_b, double *d_x) {
  static const char *const kEntry = "spmv_acc_csr_gs_sweep";
  clear_error();
  apply_env_tunables();
  if (m < 0 || nnz < 0 || ncolors < 0) return entry_error(kEntry, kErrBadArgument, "negative m, nnz or ncolors");
  if (direction < 0 || direction > 2) return entry_error(kEntry, kErrBadArgument, "direction is not 0 (forward), 1 (backward) or 2 (symmetric)");
  if (!h_color_ptr) return entry_error(kEntry, kErrBadArgument, "null h_color_ptr");
  if (m > 0 && (!d_rowptr || !d_b || !d_x)) return entry_error(kEntry, kErrBadArgument, "null rowptr / b / x");
  if (m > 0 && nnz > 0 && (!d_colindex || !d_value)) return entry_error(kEntry, kErrBadArgument, "null colindex / value of a matrix with non-zeros");
  if (too_large(nnz) || too_large(ncolors))
    return entry_error(kEntry, kErrTooLarge, "nnz or ncolors does not leave room for block arithmetic in int32");
  if (m > kGsMaxRows) return entry_error(kEntry, kErrTooLarge, "more than 2^29 rows: x is gathered through 32-bit byte offsets; sweep row blocks of the matrix");
  if (h_color_ptr[0] != 0 || h_color_ptr[ncolors] != m) return entry_error(kEntry, kErrBadArgument, "h_color_ptr does not run from 0 to m");
  for (int c = 0; c < ncolors; ++c)
    if (h_color_ptr[c + 1] < h_color_ptr[c]) return entry_error(kEntry, kErrBadArgument, "h_color_ptr descends at colour " + std::to_string(c));
  if (overlap(d_b, m, d_x, m)) return entry_error(kEntry, kErrBadArgument, "b overlaps x");
  if (m == 0) return kOk; // no rows: nothing to launch
  hipStream_t st = t_stream;
  note_stream_use();
  const auto colour = [&](int c) { launch_gs_color(st, m, nnz, d_rowptr, d_colindex, d_value, h_color_ptr[c], h_color_ptr[c + 1], d_color_rows, omega, d_b, d_x); };
  if (direction != 1)
    for (int c = 0; c < ncolors; ++c) colour(c);
  if (direction != 0)
    for (int c = ncolors - 1; c >= 0; --c) colour(c);
  return launch_error(kEntry);
}

} // namespace spmv_acc
