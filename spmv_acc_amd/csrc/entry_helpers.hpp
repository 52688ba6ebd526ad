// entry_helpers.hpp -- the host building blocks that the stateless entry files share: the structural entries (coo.cpp, transpose.cpp, spmm.cpp,
// spgemm.cpp, csr_add.cpp, extract.cpp) and the AMG chain and its solvers (gs.cpp, agg.cpp, strength.cpp, dense.cpp, cg.cpp, jacobi.cpp).  One
// definition each of the entry's error, the check after an entry's launches, the workspace alignment and its round-up, the int32 size rule, the
// overlap of two double arrays, the sum of one group of count slots, and the pattern census (k_gs.hip's) with its judgement and its refusal
// text -- the input contract that the four AMG entries (gs, agg, strength, dense), and amg_setup through them, refuse in the same words.  Plain
// inline helpers: no state and no device allocation (the census' host copy of the slots is a local, as it was in every entry).
//
// Deliberately not here: the leave lambda, the one hipMalloc / hipFree and the workspace layout of an entry, its preamble (clear_error, the
// tunables, the capture flag, plan_work_allowed) and its argument checks -- they are what differs between the entries, and they stay where
// the entry can be read from top to bottom.  Nor spmm.cpp's and dispatch.cpp's launch checks, which keep an error that is already pending.
//
// No reference counterpart: hpcde/spmv-acc reads a finished matrix from a file on the host.
#pragma once

#include "gs.hpp"
#include "engine_internal.hpp"

namespace spmv_acc {
namespace detail {

// leaves "<entry>: <what>" and the code in the calling thread's error slot; returns the code
inline int entry_error(const char *entry, int code, const std::string &what) {
  set_error(code, std::string(entry) + ": " + what);
  return code;
}

// after an entry's launches: kOk, or the launch's failure left as the entry's error (one hipGetLastError)
inline int launch_error(const char *entry) {
  const hipError_t err = hipGetLastError();
  if (err == hipSuccess) return kOk;
  return entry_error(entry, kErrHip, std::string("kernel launch failed: ") + hipGetErrorString(err));
}

constexpr size_t kEntryAlign = 256; // workspace parts start on 256-B boundaries
inline size_t aligned_up(size_t b) { return (b + kEntryAlign - 1) / kEntryAlign * kEntryAlign; }

// the sizes every entry of the library accepts (plan.cpp: room for block arithmetic in int32)
inline bool too_large(long long v) { return v > INT_MAX - (1 << 16); }

// [a, a + na) and [b, b + nb) share a byte (doubles; a null array shares nothing)
inline bool overlap(const double *a, long long na, const double *b, long long nb) { return a && b && na > 0 && nb > 0 && a < b + nb && b < a + na; }

// the sum of one group of per-wavefront counts, read back to the host (kCooCheckSlots values)
inline unsigned long long slot_sum(const unsigned *slots) {
  unsigned long long sum = 0;
  for (int s = 0; s < kCooCheckSlots; ++s) sum += slots[s];
  return sum;
}

// The census of a square CSR pattern, before anything is written: zeroes the kGsCounts groups of d_slots, runs launch_gs_census (gs.hpp: its
// counts (a) .. (f)), reads the groups back with one copy and one synchronise, and judges them.  With a mirror_advice the counts (a) .. (e) must
// be zero and the text names the advice after the mirror count; with nullptr the mirrors (e) are neither judged nor reported (a pattern that
// need not be symmetric).  *no_diag (may be null) = (f), the rows without a diagonal entry, which is not an error.  Returns kOk, or the code it
// has left in the error slot (entry_error, or hip_ok after a failed HIP call).  m > 0
inline int pattern_census(hipStream_t st, const char *entry, int m, int nnz, const int *d_rowptr, const int *d_colindex, unsigned *d_slots,
                          const char *mirror_advice, unsigned long long *no_diag) {
  const size_t count = static_cast<size_t>(kGsCounts) * kCooCheckSlots;
  std::vector<unsigned> slots(count, 0u);
  if (!hip_ok(hipMemsetAsync(d_slots, 0, sizeof(unsigned) * count, st), "zero the census")) return last_error_code_only();
  launch_gs_census(st, m, nnz, d_rowptr, d_colindex, d_slots);
  if (!hip_ok(hipMemcpyAsync(slots.data(), d_slots, sizeof(unsigned) * count, hipMemcpyDeviceToHost, st), "read the census") ||
      !hip_ok(hipStreamSynchronize(st), "census"))
    return last_error_code_only();
  unsigned long long bad[kGsCounts];
  for (int g = 0; g < kGsCounts; ++g) bad[g] = slot_sum(slots.data() + static_cast<size_t>(g) * kCooCheckSlots);
  if (no_diag) *no_diag = bad[5];
  if (bad[0] + bad[1] + bad[2] + bad[3] + (mirror_advice ? bad[4] : 0) == 0) return kOk;
  std::string what = std::to_string(bad[0]) + " ends of rowptr that are not 0 and nnz, " + std::to_string(bad[1]) +
                     " rows with a descending or out-of-range rowptr extent, " + std::to_string(bad[2]) + " columns outside [0, m), " +
                     std::to_string(bad[3]) + " positions where a row does not strictly ascend";
  if (mirror_advice) what += ", " + std::to_string(bad[4]) + " off-diagonal entries without their mirror (" + mirror_advice + ")";
  return entry_error(entry, kErrBadArgument, what + ": nothing was written");
}

} // namespace detail
} // namespace spmv_acc
