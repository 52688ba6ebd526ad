// k_extract.hip -- the kernels of the device CSR extraction C = A[rows, colmap] with a diagonal band (the definition, the steps, size rules and
// launcher declarations in extract.hpp, engine in extract.cpp).
//
// No reference counterpart: hpcde/spmv-acc multiplies a matrix by a vector.
//
// Every pass is cut by CANDIDATES (the entries of the selected rows of A) or by C ENTRIES, never by rows: a row of 20 000 entries is 313
// wavefronts of the structure passes, each lane with one short binary search in lines its neighbours share.  No atomics anywhere: every output
// is written by exactly one lane, at a place computed from the inputs alone -- but for the distinctness marks, where equal stores race and the
// verdict (how many lose) does not depend on which one wins.  VGPRs as compiled for gfx950 (wave64; no scratch, no AGPR, 8 waves per SIMD in all):
// 1. Marks (extract_mark_kernel, 18 VGPRs): inv_row[rows[i]] = i, inv_col[colmap[c]] = c, only through values inside the arrays.
// 2. Census (extract_census_kernel, 16): the marks read back (a repeated row or new column loses all but one of its stores), rows and colmap
//    values out of range, extents of the selected rows; per-wavefront counts in slots of their own, added on the host.  Nothing else reads
//    through rows or colmap unless all five counts are zero.  It also leaves the selected rows' lengths for the scan.
// 3. Candidates (extract_candidates_kernel, 20): extract.hpp step 3, with the last count of the census: columns outside [0, n), which are not
//    turned into an address of colmap.
// 4. Row pointer (extract_rowptr_kernel, 18): one lane per row, two loads.
// 5. Scatter (extract_scatter_kernel, 20): step 5; the search for the row only where a map is written.
// 6. Descents (extract_descents_kernel, 20), keys (extract_keys_kernel, 18), sorted (extract_sorted_kernel, 9): step 6.
// 7. Values (extract_values_kernel, 26; the per-step hot path and the first call's last launch): per C entry it streams 4 B of map, gathers 8 B
//    and stores 8 B.  Lane l of a wavefront owns the kExtractPerLane entries base + l + 64 k: all map loads are issued, then all gathers, then
//    the stores.  The bits are copied: no arithmetic touches a value.
#include "extract.hpp"
#include "structure_passes.hpp"

#include <algorithm>

#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

namespace spmv_acc {
namespace {

using namespace dev;
using namespace passes;
using u64 = unsigned long long;

__global__ __launch_bounds__(kThreads) void extract_mark_kernel(int mc, int m, const int *__restrict__ rows, int *__restrict__ inv_row, int n, int nc,
                                                                const int *__restrict__ colmap, int *__restrict__ inv_col) {
  const long long stride = static_cast<long long>(gridDim.x) * kThreads;
  const long long first = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x;
  if (rows != nullptr)
    for (long long i = first; i < mc; i += stride) {
      const int r = rows[i];
      if (static_cast<unsigned>(r) < static_cast<unsigned>(m)) inv_row[r] = static_cast<int>(i);
    }
  if (colmap != nullptr)
    for (long long c = first; c < n; c += stride) {
      const int v = colmap[c];
      if (static_cast<unsigned>(v) < static_cast<unsigned>(nc)) inv_col[v] = static_cast<int>(c);
    }
}

// gridDim.x <= kCooCheckBlocks; slots: extract.hpp launch_extract_census.  mc > 0, m > 0.
__global__ __launch_bounds__(kThreads) void extract_census_kernel(int mc, int m, int nnz_a, const int *__restrict__ rows, const int *__restrict__ a_rowptr,
                                                                  const int *__restrict__ inv_row, int n, int nc, const int *__restrict__ colmap,
                                                                  const int *__restrict__ inv_col, int *__restrict__ len,
                                                                  unsigned *__restrict__ slots) {
  unsigned rows_out = 0, rows_again = 0, bad_extents = 0, map_out = 0, map_again = 0;
  const long long stride = static_cast<long long>(gridDim.x) * kThreads;
  const long long first = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x;
  for (long long i = first; i <= mc; i += stride) {
    int length = 0;
    if (i < mc) {
      const int r = rows != nullptr ? rows[i] : static_cast<int>(i);
      if (static_cast<unsigned>(r) >= static_cast<unsigned>(m)) {
        rows_out += 1u;
      } else {
        rows_again += rows != nullptr && inv_row[r] != i ? 1u : 0u;
        const int lo = a_rowptr[r], hi = a_rowptr[r + 1];
        bad_extents += lo < 0 || hi > nnz_a || hi < lo ? 1u : 0u;
        int h;
        const int l = row_extent(a_rowptr, nnz_a, r, &h);
        length = h - l;
      }
    }
    len[i] = length;
  }
  if (colmap != nullptr)
    for (long long c = first; c < n; c += stride) {
      const int v = colmap[c];
      if (v >= nc) map_out += 1u;
      else if (v >= 0) map_again += inv_col[v] != c ? 1u : 0u;
    }
  count_to_slot(rows_out, slots);
  count_to_slot(rows_again, slots + kCooCheckSlots);
  count_to_slot(bad_extents, slots + 2 * kCooCheckSlots);
  count_to_slot(map_out, slots + 3 * kCooCheckSlots);
  count_to_slot(map_again, slots + 4 * kCooCheckSlots);
}

// One workgroup per tile of kExtractRankTile of the S + 1 items, blocks stride over the tiles beyond the grid; gridDim.x <= kCooCheckBlocks.
// mc > 0, S > 0; the census has passed: rows and colmap hold what extract.hpp demands.
__global__ __launch_bounds__(kThreads) void extract_candidates_kernel(int mc, int nnz_a, int S, const int *__restrict__ rows,
                                                                      const int *__restrict__ a_rowptr, const int *__restrict__ a_colindex,
                                                                      const int *__restrict__ src_ptr, int n, const int *__restrict__ colmap,
                                                                      int diag_lo, int diag_hi, int *__restrict__ newcol,
                                                                      unsigned *__restrict__ slots) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  unsigned out_of_range = 0;
  const long long items = static_cast<long long>(S) + 1;
  const long long ntiles = (items + kExtractRankTile - 1) / kExtractRankTile;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) { // (block-uniform)
    const long long base = tile * kExtractRankTile + static_cast<long long>(wave) * kWave;
    if (base >= items) continue; // (wave-uniform)
    const long long last = (base + kWave < items ? base + kWave : items) - 1;
    const long long s = base + lane;
    if (s > last) continue;
    if (s == S) {
      newcol[s] = -1; // (the scan's closing element: not kept)
      continue;
    }
    const int i = wave_row_of(src_ptr, mc, base, last < S ? last : S - 1, s);
    int hi;
    const int lo = row_extent(a_rowptr, nnz_a, rows != nullptr ? rows[i] : i, &hi);
    long long q = lo + (s - src_ptr[i]); // (lo <= q < hi by the census; held inside A's arrays regardless)
    q = q < 0 ? 0 : (q >= nnz_a ? nnz_a - 1 : q);
    const int c = load_stream(a_colindex + q);
    int kept = -1;
    if (static_cast<unsigned>(c) >= static_cast<unsigned>(n)) {
      out_of_range += 1u;
    } else {
      const int j = colmap != nullptr ? colmap[c] : c;
      const long long d = static_cast<long long>(j) - i;
      if (j >= 0 && d >= diag_lo && d <= diag_hi) kept = j;
    }
    newcol[s] = kept;
  }
  count_to_slot(out_of_range, slots);
}

__global__ __launch_bounds__(kThreads) void extract_rowptr_kernel(int mc, const int *__restrict__ src_ptr, const int *__restrict__ pos,
                                                                  int *__restrict__ c_rowptr) {
  const long long stride = static_cast<long long>(gridDim.x) * kThreads;
  for (long long i = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; i <= mc; i += stride) c_rowptr[i] = pos[src_ptr[i]];
}

// One workgroup per tile of kExtractRankTile candidates.  mc > 0, S > 0, cap = nnz_a > 0: the size of the caller's arrays.
__global__ __launch_bounds__(kThreads) void extract_scatter_kernel(int mc, int nnz_a, int S, int cap, const int *__restrict__ rows,
                                                                   const int *__restrict__ a_rowptr, const int *__restrict__ src_ptr,
                                                                   const int *__restrict__ newcol, const int *__restrict__ pos,
                                                                   int *__restrict__ c_colindex, int *__restrict__ map) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const long long ntiles = (static_cast<long long>(S) + kExtractRankTile - 1) / kExtractRankTile;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) { // (block-uniform)
    const long long base = tile * kExtractRankTile + static_cast<long long>(wave) * kWave;
    if (base >= S) continue; // (wave-uniform)
    const long long last = (base + kWave < S ? base + kWave : S) - 1;
    const long long s = base + lane;
    if (s > last) continue;
    const int col = load_stream(newcol + s);
    if (col < 0) continue;
    int j = load_stream(pos + s); // (0 <= j < nnz(C) <= S <= nnz_a; held inside the caller's arrays regardless)
    j = j < 0 ? 0 : (j >= cap ? cap - 1 : j);
    c_colindex[j] = col;
    if (map != nullptr) {
      const int i = wave_row_of(src_ptr, mc, base, last, s);
      int hi;
      const int lo = row_extent(a_rowptr, nnz_a, rows != nullptr ? rows[i] : i, &hi);
      long long q = lo + (s - src_ptr[i]);
      q = q < 0 ? 0 : (q >= nnz_a ? nnz_a - 1 : q);
      map[j] = static_cast<int>(q);
    }
  }
}

// One workgroup per tile of kExtractRankTile C entries; gridDim.x <= kCooCheckBlocks.  mc > 0, nnz_c > 0.
__global__ __launch_bounds__(kThreads) void extract_descents_kernel(int mc, int nnz_c, const int *__restrict__ c_rowptr,
                                                                    const int *__restrict__ c_colindex, unsigned *__restrict__ slots) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  unsigned descents = 0;
  const long long ntiles = (static_cast<long long>(nnz_c) + kExtractRankTile - 1) / kExtractRankTile;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) { // (block-uniform)
    const long long base = tile * kExtractRankTile + static_cast<long long>(wave) * kWave;
    if (base >= nnz_c) continue; // (wave-uniform)
    const long long last = (base + kWave < nnz_c ? base + kWave : nnz_c) - 1;
    const long long j = base + lane;
    if (j > last) continue;
    const int i = wave_row_of(c_rowptr, mc, base, last, j);
    descents += j > c_rowptr[i] && c_colindex[j] < c_colindex[j - 1] ? 1u : 0u;
  }
  count_to_slot(descents, slots);
}

// One workgroup per tile of kExtractRankTile C entries.  mc > 0, nnz_c > 0.
__global__ __launch_bounds__(kThreads) void extract_keys_kernel(int mc, int nnz_c, const int *__restrict__ c_rowptr, const int *__restrict__ c_colindex,
                                                                int col_bits, u64 *__restrict__ keys) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const long long ntiles = (static_cast<long long>(nnz_c) + kExtractRankTile - 1) / kExtractRankTile;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) { // (block-uniform)
    const long long base = tile * kExtractRankTile + static_cast<long long>(wave) * kWave;
    if (base >= nnz_c) continue; // (wave-uniform)
    const long long last = (base + kWave < nnz_c ? base + kWave : nnz_c) - 1;
    const long long j = base + lane;
    if (j > last) continue;
    const int i = wave_row_of(c_rowptr, mc, base, last, j);
    keys[j] = static_cast<u64>(static_cast<unsigned>(i)) << col_bits | static_cast<unsigned>(c_colindex[j]);
  }
}

__global__ __launch_bounds__(kThreads) void extract_sorted_kernel(int nnz_c, int nnz_sorted, const u64 *__restrict__ keys, int col_bits,
                                                                  const int *__restrict__ order, const int *__restrict__ map_tmp,
                                                                  int *__restrict__ c_colindex, int *__restrict__ map) {
  const long long stride = static_cast<long long>(gridDim.x) * kThreads;
  const u64 mask = (1ull << col_bits) - 1;
  for (long long j = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; j < nnz_c; j += stride) {
    c_colindex[j] = static_cast<int>(keys[j] & mask);
    if (map != nullptr) {
      const int o = load_stream(order + j); // (a permutation of [0, nnz_c): held inside map_tmp regardless)
      map[j] = map_tmp[static_cast<unsigned>(o) < static_cast<unsigned>(nnz_sorted) ? o : 0];
    }
  }
}

// One workgroup per tile of kExtractTile C entries, blocks stride over the tiles beyond the grid.  nnz_c > 0 (the launcher checks).
__global__ __launch_bounds__(kThreads) void extract_values_kernel(int nnz_c, int nnz_a, const int *__restrict__ map, const double *__restrict__ a_value,
                                                                  double *__restrict__ value) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const long long ntiles = (static_cast<long long>(nnz_c) + kExtractTile - 1) / kExtractTile;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) { // (block-uniform)
    const long long base = tile * kExtractTile + static_cast<long long>(wave) * kExtractWaveChunk;
    if (base >= nnz_c) continue; // (wave-uniform)
    int u[kExtractPerLane];
    double v[kExtractPerLane];
#pragma unroll
    for (int k = 0; k < kExtractPerLane; ++k) {
      const long long j = base + k * kWave + lane;
      u[k] = -1;
      if (j < nnz_c) u[k] = load_stream(map + j);
    }
#pragma unroll
    for (int k = 0; k < kExtractPerLane; ++k) { // the map is the CALLER's array here: an index outside the value array gives +0.0
      v[k] = 0.0;
      if (static_cast<unsigned>(u[k]) < static_cast<unsigned>(nnz_a)) v[k] = a_value[u[k]];
    }
#pragma unroll
    for (int k = 0; k < kExtractPerLane; ++k) {
      const long long j = base + k * kWave + lane;
      if (j < nnz_c) value[j] = v[k];
    }
  }
}

struct ExtractKept { // the scan's input: 1 where the candidate is kept
  __host__ __device__ int operator()(int col) const { return col >= 0 ? 1 : 0; }
};

} // namespace

void launch_extract_mark(hipStream_t stream, int mc, int m, const int *rows, int *inv_row, int n, int nc, const int *colmap, int *inv_col) {
  if (rows == nullptr && colmap == nullptr) return;
  const long long items = std::max(rows != nullptr ? static_cast<long long>(mc) : 0, colmap != nullptr ? static_cast<long long>(n) : 0);
  if (items <= 0) return;
  SPMV_ACC_LAUNCH(extract_mark_kernel, dim3(grid_for(items, kThreads)), dim3(kThreads), 0, stream, mc, m, rows, inv_row, n, nc, colmap, inv_col);
}

void launch_extract_census(hipStream_t stream, int mc, int m, int nnz_a, const int *rows, const int *a_rowptr, const int *inv_row, int n, int nc,
                           const int *colmap, const int *inv_col, int *len, unsigned *slots) {
  if (mc <= 0 || m <= 0) return;
  const long long items = std::max(static_cast<long long>(mc) + 1, colmap != nullptr ? static_cast<long long>(n) : 0);
  SPMV_ACC_LAUNCH(extract_census_kernel, dim3(census_grid_for(items, kThreads)), dim3(kThreads), 0, stream, mc, m, nnz_a, rows, a_rowptr, inv_row, n,
                  nc, colmap, inv_col, len, slots);
}

bool launch_extract_scan(hipStream_t stream, const int *in, size_t count, int *out, void *tmp, size_t *tmp_bytes) {
  return rocprim::exclusive_scan(tmp, *tmp_bytes, in, out, 0, count, rocprim::plus<int>(), stream) == hipSuccess;
}

bool launch_extract_scan_kept(hipStream_t stream, const int *newcol, size_t count, int *pos, void *tmp, size_t *tmp_bytes) {
  return rocprim::exclusive_scan(tmp, *tmp_bytes, rocprim::make_transform_iterator(newcol, ExtractKept()), pos, 0, count, rocprim::plus<int>(),
                                 stream) == hipSuccess;
}

void launch_extract_candidates(hipStream_t stream, int mc, int nnz_a, int S, const int *rows, const int *a_rowptr, const int *a_colindex,
                               const int *src_ptr, int n, const int *colmap, int diag_lo, int diag_hi, int *newcol, unsigned *slots) {
  if (mc <= 0 || S <= 0) return;
  SPMV_ACC_LAUNCH(extract_candidates_kernel, dim3(census_grid_for(static_cast<long long>(S) + 1, kExtractRankTile)), dim3(kThreads), 0, stream, mc,
                  nnz_a, S, rows, a_rowptr, a_colindex, src_ptr, n, colmap, diag_lo, diag_hi, newcol, slots);
}

void launch_extract_rowptr(hipStream_t stream, int mc, const int *src_ptr, const int *pos, int *c_rowptr) {
  if (mc < 0) return;
  SPMV_ACC_LAUNCH(extract_rowptr_kernel, dim3(grid_for(static_cast<long long>(mc) + 1, kThreads)), dim3(kThreads), 0, stream, mc, src_ptr, pos,
                  c_rowptr);
}

void launch_extract_scatter(hipStream_t stream, int mc, int nnz_a, int S, int cap, const int *rows, const int *a_rowptr, const int *src_ptr,
                            const int *newcol, const int *pos, int *c_colindex, int *map) {
  if (mc <= 0 || S <= 0 || cap <= 0) return;
  SPMV_ACC_LAUNCH(extract_scatter_kernel, dim3(grid_for(S, kExtractRankTile)), dim3(kThreads), 0, stream, mc, nnz_a, S, cap, rows, a_rowptr, src_ptr,
                  newcol, pos, c_colindex, map);
}

void launch_extract_descents(hipStream_t stream, int mc, int nnz_c, const int *c_rowptr, const int *c_colindex, unsigned *slots) {
  if (mc <= 0 || nnz_c <= 0) return;
  SPMV_ACC_LAUNCH(extract_descents_kernel, dim3(census_grid_for(nnz_c, kExtractRankTile)), dim3(kThreads), 0, stream, mc, nnz_c, c_rowptr, c_colindex,
                  slots);
}

void launch_extract_keys(hipStream_t stream, int mc, int nnz_c, const int *c_rowptr, const int *c_colindex, int col_bits, unsigned long long *keys) {
  if (mc <= 0 || nnz_c <= 0) return;
  SPMV_ACC_LAUNCH(extract_keys_kernel, dim3(grid_for(nnz_c, kExtractRankTile)), dim3(kThreads), 0, stream, mc, nnz_c, c_rowptr, c_colindex, col_bits,
                  keys);
}

void launch_extract_sorted(hipStream_t stream, int nnz_c, const unsigned long long *keys, int col_bits, const int *order, const int *map_tmp,
                           int *c_colindex, int *map) {
  if (nnz_c <= 0) return;
  SPMV_ACC_LAUNCH(extract_sorted_kernel, dim3(grid_for(nnz_c, kThreads)), dim3(kThreads), 0, stream, nnz_c, nnz_c, keys, col_bits, order, map_tmp,
                  c_colindex, map);
}

void launch_extract_values(hipStream_t stream, int nnz_c, int nnz_a, const int *map, const double *a_value, double *value) {
  if (nnz_c <= 0) return;
  SPMV_ACC_LAUNCH(extract_values_kernel, dim3(grid_for(nnz_c, kExtractTile)), dim3(kThreads), 0, stream, nnz_c, nnz_a, map, a_value, value);
}

} // namespace spmv_acc
