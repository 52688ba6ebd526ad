// k_csr_add.hip -- the kernels of the device CSR sparse add C = alpha * A + beta * B (the definition, the rank formulas, size rules and launcher
// declarations in csr_add.hpp, engine in csr_add.cpp).
//
// No reference counterpart: hpcde/spmv-acc multiplies a matrix by a vector.
//
// Every pass is cut by NON-ZEROS or by C ENTRIES, never by rows: a row of 200 000 entries is 3 125 wavefronts of the structure passes, each lane with
// one binary search of 18 steps in lines its neighbours share, not 200 000 steps of a lane.  No atomics anywhere: every output is written by exactly
// one lane, at a place computed from the inputs alone.
//
// 1. Census (csr_add_census_kernel), both matrices in one launch (blockIdx.y picks one): columns outside [0, n), positions inside a row whose column
//    does not exceed its predecessor's, rows whose extent descends or leaves [0, nnz] -- per-wavefront counts in slots of their own, added on the
//    host.  Nothing else runs unless all six counts are zero, so the passes below see strictly ascending rows; they still clamp every row into the
//    arrays and every place into [0, nnz_a + nnz_b).
// 2. Match (csr_add_match_kernel): csr_add.hpp step 1.  One int per non-zero of A carries both the rank and the match (pos or ~pos).
// 3. Row pointer (csr_add_rowptr_kernel): step 3, one lane per row, three loads -- O(1) per row, whatever the row holds.
// 4. Places (csr_add_place_a_kernel: a pure stream, no search; csr_add_place_b_kernel: one search in A's row): steps 4 and 5.
// 5. Values (csr_add_values_kernel, the per-step hot path and the first call's last launch): per C entry it streams 8 B of map, gathers up to two
//    values and stores 8 B.  Both maps ascend apart from their -1 gaps, so the gathers of a wavefront fall into a few consecutive lines.  Lane l of a
//    wavefront owns the kCsrAddPerLane entries base + l + 64 k: all map loads are issued, then all gathers, then the arithmetic.  Each product is
//    rounded on its own and the sum is one addition (fp contraction is off: a fused multiply-add would round once where the definition rounds twice);
//    an absent side is left out by a select, never added as 0.0 (which would turn -0.0 into +0.0).
#include "csr_add.hpp"
#include "structure_passes.hpp"

#include <algorithm>

#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

namespace spmv_acc {
namespace {

using namespace dev;
using namespace passes;

// gridDim.x <= kCooCheckBlocks; slots: csr_add.hpp launch_csr_add_census.  m > 0.
__global__ __launch_bounds__(kThreads) void csr_add_census_kernel(int m, int n, int nnz_a, const int *__restrict__ a_rowptr,
                                                                  const int *__restrict__ a_colindex, int nnz_b, const int *__restrict__ b_rowptr,
                                                                  const int *__restrict__ b_colindex, unsigned *__restrict__ slots) {
  const bool second = blockIdx.y != 0; // (block-uniform)
  const int *__restrict__ rowptr = second ? b_rowptr : a_rowptr;
  const int *__restrict__ col = second ? b_colindex : a_colindex;
  const int nnz = second ? nnz_b : nnz_a;
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  unsigned out_of_range = 0, not_ascending = 0, bad_rows = 0;
  const long long ntiles = (static_cast<long long>(nnz) + kCsrAddRankTile - 1) / kCsrAddRankTile;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) { // (block-uniform)
    const long long base = tile * kCsrAddRankTile + static_cast<long long>(wave) * kWave;
    if (base >= nnz) continue; // (wave-uniform)
    const long long last = (base + kWave < nnz ? base + kWave : nnz) - 1;
    const long long q = base + lane;
    if (q > last) continue;
    const int i = wave_row_of(rowptr, m, base, last, q); // (inside [0, m) whatever rowptr holds; a rowptr that does not ascend is counted below)
    int hi;
    const int lo = row_extent(rowptr, nnz, i, &hi);
    const int c = col[q];
    out_of_range += static_cast<unsigned>(c) >= static_cast<unsigned>(n) ? 1u : 0u;
    not_ascending += q > lo && c <= col[q - 1] ? 1u : 0u;
  }
  const long long stride = static_cast<long long>(gridDim.x) * kThreads;
  for (long long r = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; r < m; r += stride) {
    const int lo = rowptr[r], hi = rowptr[r + 1];
    bad_rows += lo < 0 || hi > nnz || hi < lo ? 1u : 0u;
  }
  unsigned *mine = slots + (second ? 3 * kCooCheckSlots : 0); // (a slot of its own per wavefront and count)
  count_to_slot(out_of_range, mine);
  count_to_slot(not_ascending, mine + kCooCheckSlots);
  count_to_slot(bad_rows, mine + 2 * kCooCheckSlots);
}

// One workgroup per tile of kCsrAddRankTile of the nnz_a + 1 items, blocks stride over the tiles beyond the grid.  m > 0.
__global__ __launch_bounds__(kThreads) void csr_add_match_kernel(int m, int nnz_a, const int *__restrict__ a_rowptr, const int *__restrict__ a_colindex,
                                                                 int nnz_b, const int *__restrict__ b_rowptr, const int *__restrict__ b_colindex,
                                                                 int *__restrict__ bpos) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const long long items = static_cast<long long>(nnz_a) + 1;
  const long long ntiles = (items + kCsrAddRankTile - 1) / kCsrAddRankTile;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) { // (block-uniform)
    const long long base = tile * kCsrAddRankTile + static_cast<long long>(wave) * kWave;
    if (base >= items) continue; // (wave-uniform)
    const long long last = (base + kWave < items ? base + kWave : items) - 1;
    const long long q = base + lane;
    if (q > last) continue;
    if (q == nnz_a) {
      bpos[q] = -1; // (the scan's closing element: no match)
      continue;
    }
    const int i = wave_row_of(a_rowptr, m, base, last, q);
    int hi;
    const int lo = row_extent(b_rowptr, nnz_b, i, &hi);
    const int c = a_colindex[q];
    const int pos = first_at_least(b_colindex, lo, hi, c);
    bpos[q] = pos < hi && b_colindex[pos] == c ? pos : ~pos;
  }
}

__global__ __launch_bounds__(kThreads) void csr_add_rowptr_kernel(int m, int nnz_a, const int *__restrict__ a_rowptr, const int *__restrict__ b_rowptr,
                                                                  const int *__restrict__ ms, int *__restrict__ c_rowptr) {
  const long long stride = static_cast<long long>(gridDim.x) * kThreads;
  for (long long r = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; r <= m; r += stride) {
    int lo = a_rowptr[r];
    lo = lo < 0 ? 0 : (lo > nnz_a ? nnz_a : lo);
    c_rowptr[r] = a_rowptr[r] + b_rowptr[r] - ms[lo];
  }
}

// One workgroup per tile of kCsrAddRankTile non-zeros of A.  cap = nnz_a + nnz_b > 0: the size of the caller's arrays.
__global__ __launch_bounds__(kThreads) void csr_add_place_a_kernel(int nnz_a, int cap, const int *__restrict__ a_colindex, const int *__restrict__ bpos,
                                                                   const int *__restrict__ ms, int *__restrict__ c_colindex, int *__restrict__ ia,
                                                                   int *__restrict__ ib) {
  const long long ntiles = (static_cast<long long>(nnz_a) + kCsrAddRankTile - 1) / kCsrAddRankTile;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) { // (block-uniform)
    const long long q = tile * kCsrAddRankTile + threadIdx.x;
    if (q >= nnz_a) continue;
    const int code = load_stream(bpos + q);
    const int pos = code < 0 ? ~code : code;
    int j = static_cast<int>(q) + pos - load_stream(ms + q); // (0 <= j < nnz(C) by the census; held inside the caller's arrays regardless)
    j = j < 0 ? 0 : (j >= cap ? cap - 1 : j);
    c_colindex[j] = load_stream(a_colindex + q);
    if (ia != nullptr) {
      ia[j] = static_cast<int>(q);
      ib[j] = code < 0 ? -1 : pos;
    }
  }
}

// One workgroup per tile of kCsrAddRankTile non-zeros of B.  m > 0, cap = nnz_a + nnz_b.
__global__ __launch_bounds__(kThreads) void csr_add_place_b_kernel(int m, int nnz_a, const int *__restrict__ a_rowptr, const int *__restrict__ a_colindex,
                                                                   int nnz_b, int cap, const int *__restrict__ b_rowptr,
                                                                   const int *__restrict__ b_colindex, const int *__restrict__ ms,
                                                                   int *__restrict__ c_colindex, int *__restrict__ ia, int *__restrict__ ib) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const long long ntiles = (static_cast<long long>(nnz_b) + kCsrAddRankTile - 1) / kCsrAddRankTile;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) { // (block-uniform)
    const long long base = tile * kCsrAddRankTile + static_cast<long long>(wave) * kWave;
    if (base >= nnz_b) continue; // (wave-uniform)
    const long long last = (base + kWave < nnz_b ? base + kWave : nnz_b) - 1;
    const long long t = base + lane;
    if (t > last) continue;
    const int i = wave_row_of(b_rowptr, m, base, last, t);
    int hi;
    const int lo = row_extent(a_rowptr, nnz_a, i, &hi);
    const int c = b_colindex[t];
    const int apos = first_at_least(a_colindex, lo, hi, c); // (0 <= apos <= nnz_a: ms holds nnz_a + 1 elements)
    if (apos < hi && a_colindex[apos] == c) continue;            // A holds the column: its lane wrote the entry
    int j = static_cast<int>(t) + apos - ms[apos];
    j = j < 0 ? 0 : (j >= cap ? cap - 1 : j);
    c_colindex[j] = c;
    if (ia != nullptr) {
      ia[j] = -1;
      ib[j] = static_cast<int>(t);
    }
  }
}

// One workgroup per tile of kCsrAddTile C entries, blocks stride over the tiles beyond the grid.  nnz_c > 0 (the launcher checks).
__global__ __launch_bounds__(kThreads) void csr_add_values_kernel(int nnz_c, int nnz_a, int nnz_b, const int *__restrict__ ia, const int *__restrict__ ib,
                                                                  double alpha, const double *__restrict__ a_value, double beta,
                                                                  const double *__restrict__ b_value, double *__restrict__ value) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const long long ntiles = (static_cast<long long>(nnz_c) + kCsrAddTile - 1) / kCsrAddTile;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) { // (block-uniform)
    const long long base = tile * kCsrAddTile + static_cast<long long>(wave) * kCsrAddWaveChunk;
    if (base >= nnz_c) continue; // (wave-uniform)
    int ua[kCsrAddPerLane], ub[kCsrAddPerLane];
    double va[kCsrAddPerLane], vb[kCsrAddPerLane];
#pragma unroll
    for (int k = 0; k < kCsrAddPerLane; ++k) {
      const long long j = base + k * kWave + lane;
      ua[k] = -1;
      ub[k] = -1;
      if (j < nnz_c) {
        ua[k] = load_stream(ia + j);
        ub[k] = load_stream(ib + j);
      }
    }
#pragma unroll
    for (int k = 0; k < kCsrAddPerLane; ++k) { // the map is the CALLER's array here: an index outside the value array counts as absent
      va[k] = 0.0;
      vb[k] = 0.0;
      if (static_cast<unsigned>(ua[k]) < static_cast<unsigned>(nnz_a)) va[k] = a_value[ua[k]];
      if (static_cast<unsigned>(ub[k]) < static_cast<unsigned>(nnz_b)) vb[k] = b_value[ub[k]];
    }
#pragma unroll
    for (int k = 0; k < kCsrAddPerLane; ++k) {
      const long long j = base + k * kWave + lane;
      const bool has_a = static_cast<unsigned>(ua[k]) < static_cast<unsigned>(nnz_a);
      const bool has_b = static_cast<unsigned>(ub[k]) < static_cast<unsigned>(nnz_b);
      const double ta = alpha * va[k], tb = beta * vb[k]; // each rounded on its own (contraction is off in this kernel)
      const double both = ta + tb;
      if (j < nnz_c) value[j] = has_a ? (has_b ? both : ta) : (has_b ? tb : 0.0);
    }
  }
}

struct CsrAddMatched { // the scan's input: 1 where the non-zero of A is matched
  __host__ __device__ int operator()(int code) const { return code >= 0 ? 1 : 0; }
};

} // namespace

void launch_csr_add_census(hipStream_t stream, int m, int n, int nnz_a, const int *a_rowptr, const int *a_colindex, int nnz_b, const int *b_rowptr,
                           const int *b_colindex, unsigned *slots) {
  if (m <= 0) return;
  const long long items = std::max(static_cast<long long>(std::max(nnz_a, nnz_b)), static_cast<long long>(m));
  SPMV_ACC_LAUNCH(csr_add_census_kernel, dim3(census_grid_for(items, kCsrAddRankTile), 2), dim3(kThreads), 0, stream, m, n, nnz_a, a_rowptr, a_colindex,
                  nnz_b, b_rowptr, b_colindex, slots);
}

void launch_csr_add_match(hipStream_t stream, int m, int nnz_a, const int *a_rowptr, const int *a_colindex, int nnz_b, const int *b_rowptr,
                          const int *b_colindex, int *bpos) {
  if (m <= 0) return;
  SPMV_ACC_LAUNCH(csr_add_match_kernel, dim3(grid_for(static_cast<long long>(nnz_a) + 1, kCsrAddRankTile)), dim3(kThreads), 0, stream, m, nnz_a,
                  a_rowptr, a_colindex, nnz_b, b_rowptr, b_colindex, bpos);
}

bool launch_csr_add_scan(hipStream_t stream, const int *bpos, int nnz_a, int *ms, void *tmp, size_t *tmp_bytes) {
  return rocprim::exclusive_scan(tmp, *tmp_bytes, rocprim::make_transform_iterator(bpos, CsrAddMatched()), ms, 0, static_cast<size_t>(nnz_a) + 1,
                                 rocprim::plus<int>(), stream) == hipSuccess;
}

void launch_csr_add_rowptr(hipStream_t stream, int m, int nnz_a, const int *a_rowptr, const int *b_rowptr, const int *ms, int *c_rowptr) {
  if (m <= 0) return;
  SPMV_ACC_LAUNCH(csr_add_rowptr_kernel, dim3(grid_for(static_cast<long long>(m) + 1, kThreads)), dim3(kThreads), 0, stream, m, nnz_a, a_rowptr,
                  b_rowptr, ms, c_rowptr);
}

void launch_csr_add_place_a(hipStream_t stream, int nnz_a, int nnz_b, const int *a_colindex, const int *bpos, const int *ms, int *c_colindex, int *ia,
                            int *ib) {
  if (nnz_a <= 0) return;
  SPMV_ACC_LAUNCH(csr_add_place_a_kernel, dim3(grid_for(nnz_a, kCsrAddRankTile)), dim3(kThreads), 0, stream, nnz_a, nnz_a + nnz_b, a_colindex, bpos,
                  ms, c_colindex, ia, ib);
}

void launch_csr_add_place_b(hipStream_t stream, int m, int nnz_a, const int *a_rowptr, const int *a_colindex, int nnz_b, const int *b_rowptr,
                            const int *b_colindex, const int *ms, int *c_colindex, int *ia, int *ib) {
  if (m <= 0 || nnz_b <= 0) return;
  SPMV_ACC_LAUNCH(csr_add_place_b_kernel, dim3(grid_for(nnz_b, kCsrAddRankTile)), dim3(kThreads), 0, stream, m, nnz_a, a_rowptr, a_colindex, nnz_b,
                  nnz_a + nnz_b, b_rowptr, b_colindex, ms, c_colindex, ia, ib);
}

void launch_csr_add_values(hipStream_t stream, int nnz_c, int nnz_a, int nnz_b, const int *ia, const int *ib, double alpha, const double *a_value,
                           double beta, const double *b_value, double *value) {
  if (nnz_c <= 0) return;
  SPMV_ACC_LAUNCH(csr_add_values_kernel, dim3(grid_for(nnz_c, kCsrAddTile)), dim3(kThreads), 0, stream, nnz_c, nnz_a, nnz_b, ia, ib, alpha, a_value,
                  beta, b_value, value);
}

} // namespace spmv_acc
