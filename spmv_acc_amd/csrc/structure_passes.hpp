// structure_passes.hpp -- the device building blocks that the structure-pass kernel files share (k_coo, k_spgemm, k_csr_add, k_extract, k_transpose;
// k_spmm takes the grid helper): one definition each of the clamped grid, the clamped row, the two binary searches, the wavefront's row search,
// the census count without atomics, and the run summation whose order coo.hpp documents.  Plain inline helpers, no constants of its own: the
// tile constants stay with their features, kCooLongRun / kCooCheckBlocks / kCooCheckSlots in coo.hpp.
//
// No reference counterpart: hpcde/spmv-acc reads a finished matrix from a file on the host.
#pragma once

#include "coo.hpp"
#include "device_utils.hpp"
#include "kernels.hpp"

namespace spmv_acc {
namespace passes {

using dev::kWave;

// ---- grids (host) ---------------------------------------------------------------------------------------------------------------------
// workgroups for `items` at `per_block` each, at least one, at most max_grid_blocks(): the kernels stride over the work beyond the grid
inline unsigned grid_for(long long items, int per_block) {
  long long b = (items + per_block - 1) / per_block;
  const long long cap = max_grid_blocks();
  return static_cast<unsigned>(b < 1 ? 1 : (b > cap ? cap : b));
}

// a grid whose wavefronts each own a count slot (count_to_slot below)
inline unsigned census_grid_for(long long items, int per_block) {
  const unsigned grid = grid_for(items, per_block);
  return grid > static_cast<unsigned>(kCooCheckBlocks) ? static_cast<unsigned>(kCooCheckBlocks) : grid;
}

// ---- rows and searches ------------------------------------------------------------------------------------------------------------------
// row i as positions [lo, *hi) inside the matrix' arrays, whatever rowptr holds (0 <= i < the rows of rowptr)
__device__ __forceinline__ int row_extent(const int *__restrict__ rowptr, int nnz, int i, int *hi) {
  int lo = rowptr[i], h = rowptr[i + 1];
  lo = lo < 0 ? 0 : (lo > nnz ? nnz : lo);
  *hi = h < lo ? lo : (h > nnz ? nnz : h);
  return lo;
}

// the last r in [lo, hi] with ptr[r] <= q (lo itself if there is none): with an ascending ptr and ptr[lo] <= q < ptr[hi + 1] the row that holds
// item q (empty rows are passed over).  Reads ptr[lo + 1 .. hi] only and stays inside [lo, hi] whatever ptr holds.  The compare takes the widths
// of its caller's T and Q
template <typename T, typename Q> __device__ __forceinline__ int last_at_most(const T *__restrict__ ptr, int lo, int hi, Q q) {
  while (lo < hi) {
    const int mid = lo + (hi - lo + 1) / 2;
    if (ptr[mid] <= q) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// for a wavefront that owns the consecutive items [first, last]: the rows of the two ends in ptr[0 .. rows), every lane the same two searches
// (returns the first's, leaves the last's in *r_last).  A wavefront inside one long row then searches nothing further
template <typename T, typename Q> __device__ __forceinline__ int wave_end_rows(const T *__restrict__ ptr, int rows, Q first, Q last, int *r_last) {
  const int r_first = last_at_most(ptr, 0, rows - 1, first);
  *r_last = last_at_most(ptr, r_first, rows - 1, last);
  return r_first;
}

// ... and the row of its own item q between them
template <typename T, typename Q> __device__ __forceinline__ int wave_row_of(const T *__restrict__ ptr, int rows, Q first, Q last, Q q) {
  int r_last;
  const int r_first = wave_end_rows(ptr, rows, first, last, &r_last);
  return last_at_most(ptr, r_first, r_last, q);
}

// the first position p in [lo, hi) with key[p] >= c (hi if there is none)
template <typename K, typename C> __device__ __forceinline__ int first_at_least(const K *__restrict__ key, int lo, int hi, C c) {
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (key[mid] < c) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// ---- census -----------------------------------------------------------------------------------------------------------------------------
// the per-wavefront count of a census kernel into its slot of `group` (blockIdx.x < kCooCheckBlocks: census_grid_for); every lane of the
// wavefront calls it.  An integer count without an atomic: the host adds up the slots
__device__ __forceinline__ void count_to_slot(unsigned count, unsigned *__restrict__ group) {
  for (int off = kWave / 2; off > 0; off >>= 1) count += __shfl_xor(count, off, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0) group[blockIdx.x * (kThreads / kWave) + threadIdx.x / kWave] = count;
}

// ---- run summation (THE SUMMATION ORDER of coo.hpp) -------------------------------------------------------------------------------------
// A source names the terms of the sorted positions p in three phases, so that a step issues all index loads, then all gathers, then the
// arithmetic:  index(p) = what position p names,  load(idx) = the value gather(s),  term(idx, raw) = the term to add;  fetch(p) = all three.
// Contraction is off in the sums: a term that is a product (k_spgemm) is rounded on its own and never fused into the addition next to it.

// the wavefront form for the run [a, end), end - a > 64: lane l adds the terms at a + l, a + l + 64, ... in that order, then the 64 partial sums
// are combined as a balanced tree over neighbouring lanes.  All 64 lanes must call it; every lane returns the sum.
template <typename Source> __device__ __forceinline__ double wave_run_sum(const Source &src, int a, int end, int lane) {
#pragma clang fp contract(off)
  int p = a + lane;
  double part = src.fetch(p);
  p += kWave;
  for (; p + 3 * kWave < end; p += 4 * kWave) { // four independent terms in flight, added in order
    const double v0 = src.fetch(p), v1 = src.fetch(p + kWave);
    const double v2 = src.fetch(p + 2 * kWave), v3 = src.fetch(p + 3 * kWave);
    part += v0;
    part += v1;
    part += v2;
    part += v3;
  }
  for (; p < end; p += kWave) part += src.fetch(p);
  return dev::group_sum<64>(part);
}

// The body of a values kernel: value[j] = the sum of run j = [start[j], start[j + 1]) of the source's terms, j < count.  One workgroup per tile
// of 4 * 64 * PER_LANE entries (the kernel files hold their tile constants to that), blocks stride over the tiles beyond the grid.  Lane l of a
// wavefront owns the PER_LANE entries base + l + 64 k and walks their runs together: step t issues the t-th index load of all of them, then the
// gathers, then the adds -- straight-line code with selects, no branch per run.  Runs longer than kCooLongRun sit the lane pass out and are
// summed by the whole wavefront, one after the other.  The map is the CALLER's array: every run is clamped to [0, limit].  limit > 0.
template <int PER_LANE, typename Source>
__device__ __forceinline__ void sum_runs(int limit, int count, const int *__restrict__ start, const Source &src, double *__restrict__ value) {
#pragma clang fp contract(off)
  constexpr int chunk = kWave * PER_LANE, tile_items = (kThreads / kWave) * chunk;
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const long long ntiles = (static_cast<long long>(count) + tile_items - 1) / tile_items;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) { // (block-uniform)
    const long long base = tile * tile_items + static_cast<long long>(wave) * chunk;
    if (base >= count) continue; // (wave-uniform)
    int s[PER_LANE];
    int len[PER_LANE]; // the run's length; NEGATED where it is longer than kCooLongRun (such a run sits the lane pass out)
    double acc[PER_LANE];
    int rounds = 0;
    bool any_long = false;
#pragma unroll
    for (int k = 0; k < PER_LANE; ++k) {
      const long long j = base + k * kWave + lane;
      int a = 0, b = 0;
      if (j < count) {
        a = dev::load_stream(start + j);
        b = dev::load_stream(start + j + 1);
      }
      a = a < 0 ? 0 : (a > limit ? limit : a);
      b = b < a ? a : (b > limit ? limit : b);
      s[k] = a;
      const int l = b - a;
      len[k] = l > kCooLongRun ? -l : l;
      any_long |= l > kCooLongRun;
      rounds = l <= kCooLongRun && l > rounds ? l : rounds;
      acc[k] = 0.0; // (an empty run -- a crafted map -- sums to 0.0)
    }
    for (int t = 0; t < rounds; ++t) {
      decltype(src.index(0)) idx[PER_LANE];
      decltype(src.load(idx[0])) raw[PER_LANE];
#pragma unroll
      for (int k = 0; k < PER_LANE; ++k) idx[k] = src.index(t < len[k] ? s[k] + t : 0);
#pragma unroll
      for (int k = 0; k < PER_LANE; ++k) raw[k] = src.load(idx[k]);
#pragma unroll
      for (int k = 0; k < PER_LANE; ++k) {
        const double vk = src.term(idx[k], raw[k]);
        acc[k] = t < len[k] ? (t == 0 ? vk : acc[k] + vk) : acc[k]; // (the sum starts from its first term, not from 0.0)
      }
    }
    if (__ballot(any_long)) { // (wave-uniform; never taken on a mesh)
#pragma unroll
      for (int k = 0; k < PER_LANE; ++k) {
        unsigned long long todo = __ballot(len[k] < 0);
        while (todo) { // the wavefront takes its long runs one at a time, in lane order
          const int owner = __ffsll(static_cast<long long>(todo)) - 1;
          todo &= todo - 1;
          const int a = __shfl(s[k], owner, kWave);
          const int l = -__shfl(len[k], owner, kWave);
          const double sum = wave_run_sum(src, a, a + l, lane);
          if (lane == owner) acc[k] = sum;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < PER_LANE; ++k) {
      const long long j = base + k * kWave + lane;
      if (j < count) value[j] = acc[k];
    }
  }
}

} // namespace passes
} // namespace spmv_acc
