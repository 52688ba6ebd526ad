// k_coo.hip -- the kernels of the device COO -> CSR assembly (size rules, the summation order and launcher declarations in coo.hpp, engine
// in coo.cpp).
//
// No reference counterpart: hpcde/spmv-acc reads a finished matrix from a file on the host.
//
// 1. Structure.  The CSR of a triple list = its triples ordered by (row, column, input position) with equal (row, column) merged.  The order
//    comes from ONE stable radix sort of the pairs (row << bits(n) | col, q) on the bits that can differ (rocPRIM, header-only, as the
//    transpose uses it; the key is 64 bits wide, so a 70 000 x 70 000 matrix with its 34 key bits is no special case).  Around it: a range
//    census of rows and columns (nothing is sorted or written if one lies outside the shape; per-wavefront counts in slots of their own, no
//    atomic), run-head flags, their exclusive scan (rocPRIM) = each sorted triple's CSR entry, the run starts and columns written by the
//    heads, and rowptr by one binary search per row in the sorted keys.  No float is touched.
//
// 2. Values (coo_values_kernel, the per-step hot path and the first assembly's last launch).  value[j] = the sum of val[order[p]] over run j
//    = [start[j], start[j + 1]).  Streams start (4 B per entry) and order (4 B per triple), gathers 8 B per triple -- after a shuffle every
//    gather is its own 128-B request (profiles/r05_gather_request_size_microbench.txt), which is what the pass costs -- and writes 8 B per
//    entry.  FEM runs are 1, 2 or 4 triples long, so a lane that walked one run at a time would keep one dependent pair of loads in flight.
//    Lane l of a wavefront owns the kCooPerLane entries base + l + 64 k instead and walks them together: step t issues the t-th order load of
//    all six runs, then the six gathers, then the six adds -- straight-line code with selects, no branch per run -- so six
//    independent chains are in flight per lane and the start / value accesses of a wavefront are contiguous.  Runs longer than kCooLongRun
//    sit the lane pass out and are summed by the whole wavefront, one after the other, in the order coo.hpp documents: a position hit 10^5
//    times is 1 563 steps of a wavefront, not 10^5 of a lane.  Every order entry is checked before it becomes an address and every run is
//    clamped to [0, nnz_coo]; the sums depend on the map alone (no atomics), so a re-assembly repeats the first assembly's bits.
#include "coo.hpp"
#include "device_utils.hpp"
#include "kernels.hpp"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

namespace spmv_acc {
namespace {

using namespace dev;

typedef unsigned long long u64;

unsigned coo_grid(long long items, int per_block) {
  long long b = (items + per_block - 1) / per_block;
  const long long cap = max_grid_blocks();
  return static_cast<unsigned>(b < 1 ? 1 : (b > cap ? cap : b));
}

__global__ __launch_bounds__(kThreads) void coo_check_kernel(const int *__restrict__ row, const int *__restrict__ col, int nnz_coo, int m, int n,
                                                             unsigned *__restrict__ slots) {
  const long long stride = static_cast<long long>(gridDim.x) * kThreads;
  unsigned mine = 0;
  for (long long q = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; q < nnz_coo; q += stride)
    mine += (static_cast<unsigned>(row[q]) >= static_cast<unsigned>(m) || static_cast<unsigned>(col[q]) >= static_cast<unsigned>(n)) ? 1u : 0u;
  for (int off = kWave / 2; off > 0; off >>= 1) mine += __shfl_xor(mine, off, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0) slots[blockIdx.x * (kThreads / kWave) + threadIdx.x / kWave] = mine; // (blockIdx.x < kCooCheckBlocks)
}

__global__ __launch_bounds__(kThreads) void coo_keys_kernel(const int *__restrict__ row, const int *__restrict__ col, int nnz_coo, int col_bits,
                                                            u64 *__restrict__ keys) {
  const long long stride = static_cast<long long>(gridDim.x) * kThreads;
  for (long long q = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; q < nnz_coo; q += stride) // (the census has passed: both in range)
    keys[q] = static_cast<u64>(static_cast<unsigned>(row[q])) << col_bits | static_cast<unsigned>(col[q]);
}

__global__ __launch_bounds__(kThreads) void coo_heads_kernel(const u64 *__restrict__ keys, int nnz_coo, int *__restrict__ head) {
  const long long stride = static_cast<long long>(gridDim.x) * kThreads;
  for (long long p = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; p <= nnz_coo; p += stride)
    head[p] = p < nnz_coo && (p == 0 || keys[p] != keys[p - 1]) ? 1 : 0;
}

__global__ __launch_bounds__(kThreads) void coo_entries_kernel(const u64 *__restrict__ keys, const int *__restrict__ head,
                                                               const int *__restrict__ index, int nnz_coo, int col_bits, int *__restrict__ start,
                                                               int *__restrict__ colindex) {
  const long long stride = static_cast<long long>(gridDim.x) * kThreads;
  const u64 col_mask = (1ULL << col_bits) - 1;
  for (long long p = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; p <= nnz_coo; p += stride) {
    if (p == nnz_coo) {
      start[index[p]] = nnz_coo; // (index[nnz_coo] = the number of runs <= nnz_coo: the closing offset)
    } else if (head[p]) {
      const int j = index[p]; // (a count of heads before p: 0 <= j <= p)
      start[j] = static_cast<int>(p);
      colindex[j] = static_cast<int>(keys[p] & col_mask);
    }
  }
}

__global__ __launch_bounds__(kThreads) void coo_rowptr_kernel(const u64 *__restrict__ keys, const int *__restrict__ index, int nnz_coo, int m,
                                                              int col_bits, int *__restrict__ rowptr) {
  const long long stride = static_cast<long long>(gridDim.x) * kThreads;
  for (long long r = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; r <= m; r += stride) {
    const u64 want = static_cast<u64>(r) << col_bits;
    int lo = 0, hi = nnz_coo; // first p in [0, nnz_coo] with keys[p] >= want: a run head or the end, so index[p] is the row's first entry
    while (lo < hi) {
      const int mid = lo + (hi - lo) / 2;
      if (keys[mid] < want) lo = mid + 1;
      else hi = mid;
    }
    rowptr[r] = index[lo];
  }
}

// val[order[p]] for 0 <= p < nnz_coo; an order entry outside [0, nnz_coo) reads val[0] and counts as +0.0
__device__ __forceinline__ double coo_fetch(const int *__restrict__ order, const double *__restrict__ val, int nnz_coo, int p) {
  const int q = order[p];
  const bool ok = static_cast<unsigned>(q) < static_cast<unsigned>(nnz_coo);
  const double v = val[ok ? q : 0];
  return ok ? v : 0.0;
}

// the wavefront form of coo.hpp's order for the run [a, end), end - a > 64: lane l adds the values at a + l, a + l + 64, ... in that order, then
// the 64 partial sums are combined as a balanced tree over neighbouring lanes.  All 64 lanes must call it; every lane returns the sum.
__device__ __forceinline__ double coo_wave_run_sum(const int *__restrict__ order, const double *__restrict__ val, int nnz_coo, int a, int end,
                                                   int lane) {
  int p = a + lane;
  double part = coo_fetch(order, val, nnz_coo, p);
  p += kWave;
  for (; p + 3 * kWave < end; p += 4 * kWave) { // four independent gathers in flight, added in order
    const double v0 = coo_fetch(order, val, nnz_coo, p), v1 = coo_fetch(order, val, nnz_coo, p + kWave);
    const double v2 = coo_fetch(order, val, nnz_coo, p + 2 * kWave), v3 = coo_fetch(order, val, nnz_coo, p + 3 * kWave);
    part += v0;
    part += v1;
    part += v2;
    part += v3;
  }
  for (; p < end; p += kWave) part += coo_fetch(order, val, nnz_coo, p);
  return group_sum<64>(part);
}

// One workgroup per tile of kCooTile CSR entries, blocks stride over the tiles beyond the grid.  nnz_coo > 0 (the launcher checks).
__global__ __launch_bounds__(kThreads) void coo_values_kernel(int nnz_coo, int nnz, const int *__restrict__ order, const int *__restrict__ start,
                                                              const double *__restrict__ val, double *__restrict__ value) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const long long ntiles = (static_cast<long long>(nnz) + kCooTile - 1) / kCooTile;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) { // (block-uniform)
    const long long base = tile * kCooTile + static_cast<long long>(wave) * kCooWaveChunk;
    if (base >= nnz) continue; // (wave-uniform)
    int s[kCooPerLane];
    int len[kCooPerLane]; // the run's length; NEGATED where it is longer than kCooLongRun (such a run sits the lane pass out)
    double acc[kCooPerLane];
    int rounds = 0;
    bool any_long = false;
#pragma unroll
    for (int k = 0; k < kCooPerLane; ++k) {
      const long long j = base + k * kWave + lane;
      int a = 0, b = 0;
      if (j < nnz) {
        a = load_stream(start + j);
        b = load_stream(start + j + 1);
      }
      a = a < 0 ? 0 : (a > nnz_coo ? nnz_coo : a); // the map is the CALLER's array here: every run is clamped to [0, nnz_coo]
      b = b < a ? a : (b > nnz_coo ? nnz_coo : b);
      s[k] = a;
      const int l = b - a;
      len[k] = l > kCooLongRun ? -l : l;
      any_long |= l > kCooLongRun;
      rounds = l <= kCooLongRun && l > rounds ? l : rounds;
      acc[k] = 0.0; // (an empty run -- a crafted map -- sums to 0.0)
    }
    for (int t = 0; t < rounds; ++t) {
      int q[kCooPerLane];
      double v[kCooPerLane];
#pragma unroll
      for (int k = 0; k < kCooPerLane; ++k) q[k] = order[t < len[k] ? s[k] + t : 0];
#pragma unroll
      for (int k = 0; k < kCooPerLane; ++k) v[k] = val[static_cast<unsigned>(q[k]) < static_cast<unsigned>(nnz_coo) ? q[k] : 0];
#pragma unroll
      for (int k = 0; k < kCooPerLane; ++k) {
        const double vk = static_cast<unsigned>(q[k]) < static_cast<unsigned>(nnz_coo) ? v[k] : 0.0;
        acc[k] = t < len[k] ? (t == 0 ? vk : acc[k] + vk) : acc[k];
      }
    }
    if (__ballot(any_long)) { // (wave-uniform; never taken on a mesh)
#pragma unroll
      for (int k = 0; k < kCooPerLane; ++k) {
        unsigned long long todo = __ballot(len[k] < 0);
        while (todo) { // the wavefront takes its long runs one at a time, in lane order
          const int owner = __ffsll(static_cast<long long>(todo)) - 1;
          todo &= todo - 1;
          const int a = __shfl(s[k], owner, kWave);
          const int l = -__shfl(len[k], owner, kWave);
          const double sum = coo_wave_run_sum(order, val, nnz_coo, a, a + l, lane);
          if (lane == owner) acc[k] = sum;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kCooPerLane; ++k) {
      const long long j = base + k * kWave + lane;
      if (j < nnz) value[j] = acc[k];
    }
  }
}

} // namespace

void launch_coo_check(hipStream_t stream, const int *row, const int *col, int nnz_coo, int m, int n, unsigned *slots) {
  if (nnz_coo <= 0) return;
  unsigned grid = coo_grid(nnz_coo, 4 * kThreads);
  if (grid > static_cast<unsigned>(kCooCheckBlocks)) grid = kCooCheckBlocks;
  SPMV_ACC_LAUNCH(coo_check_kernel, dim3(grid), dim3(kThreads), 0, stream, row, col, nnz_coo, m, n, slots);
}

void launch_coo_keys(hipStream_t stream, const int *row, const int *col, int nnz_coo, int col_bits, unsigned long long *keys) {
  if (nnz_coo <= 0) return;
  SPMV_ACC_LAUNCH(coo_keys_kernel, dim3(coo_grid(nnz_coo, kThreads)), dim3(kThreads), 0, stream, row, col, nnz_coo, col_bits, keys);
}

bool launch_coo_sort(hipStream_t stream, const unsigned long long *keys, int nnz_coo, int key_bits, unsigned long long *keys_out, int *order,
                     void *tmp, size_t *tmp_bytes) {
  return rocprim::radix_sort_pairs(tmp, *tmp_bytes, keys, keys_out, rocprim::counting_iterator<int>(0), order, static_cast<size_t>(nnz_coo), 0u,
                                   static_cast<unsigned>(key_bits), stream) == hipSuccess;
}

void launch_coo_heads(hipStream_t stream, const unsigned long long *keys, int nnz_coo, int *head) {
  SPMV_ACC_LAUNCH(coo_heads_kernel, dim3(coo_grid(static_cast<long long>(nnz_coo) + 1, kThreads)), dim3(kThreads), 0, stream, keys, nnz_coo, head);
}

bool launch_coo_scan(hipStream_t stream, const int *head, int nnz_coo, int *index, void *tmp, size_t *tmp_bytes) {
  return rocprim::exclusive_scan(tmp, *tmp_bytes, head, index, 0, static_cast<size_t>(nnz_coo) + 1, rocprim::plus<int>(), stream) == hipSuccess;
}

void launch_coo_entries(hipStream_t stream, const unsigned long long *keys, const int *head, const int *index, int nnz_coo, int col_bits,
                        int *start, int *colindex) {
  SPMV_ACC_LAUNCH(coo_entries_kernel, dim3(coo_grid(static_cast<long long>(nnz_coo) + 1, kThreads)), dim3(kThreads), 0, stream, keys, head, index,
                  nnz_coo, col_bits, start, colindex);
}

void launch_coo_rowptr(hipStream_t stream, const unsigned long long *keys, const int *index, int nnz_coo, int m, int col_bits, int *rowptr) {
  SPMV_ACC_LAUNCH(coo_rowptr_kernel, dim3(coo_grid(static_cast<long long>(m) + 1, kThreads)), dim3(kThreads), 0, stream, keys, index, nnz_coo, m,
                  col_bits, rowptr);
}

void launch_coo_values(hipStream_t stream, int nnz_coo, int nnz, const int *order, const int *start, const double *val, double *value) {
  if (nnz <= 0 || nnz_coo <= 0) return;
  SPMV_ACC_LAUNCH(coo_values_kernel, dim3(coo_grid(nnz, kCooTile)), dim3(kThreads), 0, stream, nnz_coo, nnz, order, start, val, value);
}

} // namespace spmv_acc
