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
// 2. Values (coo_values_kernel = structure_passes.hpp sum_runs on CooTerms; the per-step hot path and the first assembly's last launch).  value[j] = the sum of val[order[p]] over run j
//    = [start[j], start[j + 1]).  Streams start (4 B per entry) and order (4 B per triple), gathers 8 B per triple -- after a shuffle every
//    gather is its own 128-B request (profiles/r05_gather_request_size_microbench.txt), which is what the pass costs -- and writes 8 B per
//    entry.  FEM runs are 1, 2 or 4 triples long, so a lane that walked one run at a time would keep one dependent pair of loads in flight.
//    Lane l of a wavefront owns the kCooPerLane entries base + l + 64 k instead and walks them together: step t issues the t-th order load of
//    all six runs, then the six gathers, then the six adds -- straight-line code with selects, no branch per run -- so six
//    independent chains are in flight per lane and the start / value accesses of a wavefront are contiguous.  Runs longer than kCooLongRun
//    sit the lane pass out and are summed by the whole wavefront, one after the other, in the order coo.hpp documents: a position hit 10^5
//    times is 1 563 steps of a wavefront, not 10^5 of a lane.  Every order entry is checked before it becomes an address and every run is
//    clamped to [0, nnz_coo]; the sums depend on the map alone (no atomics), so a re-assembly repeats the first assembly's bits.
#include "structure_passes.hpp"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

namespace spmv_acc {
namespace {

using namespace dev;
using namespace passes;

typedef unsigned long long u64;

__global__ __launch_bounds__(kThreads) void coo_check_kernel(const int *__restrict__ row, const int *__restrict__ col, int nnz_coo, int m, int n,
                                                             unsigned *__restrict__ slots) {
  const long long stride = static_cast<long long>(gridDim.x) * kThreads;
  unsigned mine = 0;
  for (long long q = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; q < nnz_coo; q += stride)
    mine += (static_cast<unsigned>(row[q]) >= static_cast<unsigned>(m) || static_cast<unsigned>(col[q]) >= static_cast<unsigned>(n)) ? 1u : 0u;
  count_to_slot(mine, slots);
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
    rowptr[r] = index[first_at_least(keys, 0, nnz_coo, want)]; // (a run head or the end, so index[p] is the row's first entry)
  }
}

// the terms of the assembly's runs: val[order[p]] for 0 <= p < nnz_coo; an order entry outside [0, nnz_coo) reads val[0] and counts as +0.0
struct CooTerms {
  const int *__restrict__ order;
  const double *__restrict__ val;
  int nnz_coo;
  __device__ __forceinline__ int index(int p) const { return order[p]; }
  __device__ __forceinline__ double load(int q) const { return val[static_cast<unsigned>(q) < static_cast<unsigned>(nnz_coo) ? q : 0]; }
  __device__ __forceinline__ double term(int q, double v) const { return static_cast<unsigned>(q) < static_cast<unsigned>(nnz_coo) ? v : 0.0; }
  __device__ __forceinline__ double fetch(int p) const {
    const int q = index(p);
    return term(q, load(q));
  }
};

static_assert(kCooWaveChunk == kWave * kCooPerLane && kCooTile == (kThreads / kWave) * kCooWaveChunk, "sum_runs derives its tile from kCooPerLane");

// One workgroup per tile of kCooTile CSR entries, blocks stride over the tiles beyond the grid.  nnz_coo > 0 (the launcher checks).
__global__ __launch_bounds__(kThreads) void coo_values_kernel(int nnz_coo, int nnz, const int *__restrict__ order, const int *__restrict__ start,
                                                              const double *__restrict__ val, double *__restrict__ value) {
  sum_runs<kCooPerLane>(nnz_coo, nnz, start, CooTerms{order, val, nnz_coo}, value);
}

} // namespace

void launch_coo_check(hipStream_t stream, const int *row, const int *col, int nnz_coo, int m, int n, unsigned *slots) {
  if (nnz_coo <= 0) return;
  SPMV_ACC_LAUNCH(coo_check_kernel, dim3(census_grid_for(nnz_coo, 4 * kThreads)), dim3(kThreads), 0, stream, row, col, nnz_coo, m, n, slots);
}

void launch_coo_keys(hipStream_t stream, const int *row, const int *col, int nnz_coo, int col_bits, unsigned long long *keys) {
  if (nnz_coo <= 0) return;
  SPMV_ACC_LAUNCH(coo_keys_kernel, dim3(grid_for(nnz_coo, kThreads)), dim3(kThreads), 0, stream, row, col, nnz_coo, col_bits, keys);
}

bool launch_coo_sort(hipStream_t stream, const unsigned long long *keys, int nnz_coo, int key_bits, unsigned long long *keys_out, int *order,
                     void *tmp, size_t *tmp_bytes) {
  return rocprim::radix_sort_pairs(tmp, *tmp_bytes, keys, keys_out, rocprim::counting_iterator<int>(0), order, static_cast<size_t>(nnz_coo), 0u,
                                   static_cast<unsigned>(key_bits), stream) == hipSuccess;
}

void launch_coo_heads(hipStream_t stream, const unsigned long long *keys, int nnz_coo, int *head) {
  SPMV_ACC_LAUNCH(coo_heads_kernel, dim3(grid_for(static_cast<long long>(nnz_coo) + 1, kThreads)), dim3(kThreads), 0, stream, keys, nnz_coo, head);
}

bool launch_coo_scan(hipStream_t stream, const int *head, int nnz_coo, int *index, void *tmp, size_t *tmp_bytes) {
  return rocprim::exclusive_scan(tmp, *tmp_bytes, head, index, 0, static_cast<size_t>(nnz_coo) + 1, rocprim::plus<int>(), stream) == hipSuccess;
}

void launch_coo_entries(hipStream_t stream, const unsigned long long *keys, const int *head, const int *index, int nnz_coo, int col_bits,
                        int *start, int *colindex) {
  SPMV_ACC_LAUNCH(coo_entries_kernel, dim3(grid_for(static_cast<long long>(nnz_coo) + 1, kThreads)), dim3(kThreads), 0, stream, keys, head, index,
                  nnz_coo, col_bits, start, colindex);
}

void launch_coo_rowptr(hipStream_t stream, const unsigned long long *keys, const int *index, int nnz_coo, int m, int col_bits, int *rowptr) {
  SPMV_ACC_LAUNCH(coo_rowptr_kernel, dim3(grid_for(static_cast<long long>(m) + 1, kThreads)), dim3(kThreads), 0, stream, keys, index, nnz_coo, m,
                  col_bits, rowptr);
}

void launch_coo_values(hipStream_t stream, int nnz_coo, int nnz, const int *order, const int *start, const double *val, double *value) {
  if (nnz <= 0 || nnz_coo <= 0) return;
  SPMV_ACC_LAUNCH(coo_values_kernel, dim3(grid_for(nnz, kCooTile)), dim3(kThreads), 0, stream, nnz_coo, nnz, order, start, val, value);
}

} // namespace spmv_acc
