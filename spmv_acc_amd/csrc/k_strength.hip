// k_strength.hip -- the kernels of the strength-of-connection filter and of the prolongator smoother (the kept pattern's definition, the values
// and their summation order, size rules and launcher declarations in strength.hpp, engine in strength.cpp).  The census is k_gs.hip's, the
// scan k_coo.hip's.
//
// No reference counterpart: hpcde/spmv-acc multiplies a matrix by a vector.
//
// No atomics and no waiting anywhere: every output is written by exactly one lane, at a place computed from the inputs alone; every dependency
// is a kernel boundary.  VGPRs as compiled for gfx950 (wave64; no scratch, no AGPR, 8 waves per SIMD in all):
// 1. Roots (strength_sd_kernel, 14 VGPRs): one row per lane, the diagonal by a binary search of the row, sd[i] = sqrt(|a_ii|).
// 2. Flags (strength_flags_kernel, 24; the analysis' hot path): one ENTRY per lane, the row by the wavefront's row search; per off-diagonal entry
//    one column, two gathers of sd, a binary search of the mirror row and the mirror's value: kept iff either value reaches the edge's rhs.
//    The comparisons are exact, so the mapping of lanes to entries cannot change a bit: a form with one ROW per lane gave the same arrays,
//    faster on a 9-point mesh and twice as slow on a 27-point grid (strength.hpp PASSES holds the figures).
// 3. Row pointers (strength_ptrs_kernel, 22): one row per lane, s_rowptr and drop_ptr from the scan at the row's first position.
// 4. Scatter (strength_scatter_kernel, 13): one entry per lane; a kept entry leaves its column and its position at its rank among the kept, a
//    dropped one its position at its rank among the dropped, behind all the kept: the stable partition.
// 5. Diagonal (strength_diag_kernel, 34; per step): structure_passes.hpp sum_runs on the dropped values of each row, then every lane adds the
//    stored diagonal of S's row to the lump it has just written (the same lane, the same addresses: program order).
// 6. Values (strength_values_kernel, 54; per step, the hot path): lane l of a wavefront owns the kStrengthPerLane entries base + l + 64 k of S: all
//    map and column loads are issued, then the row searches between the wavefront's two end rows, then the gathers of value and diag, then the
//    stores.  omega == 0 copies bits; otherwise one multiplication and one division per off-diagonal, each rounded on its own.
#include "strength.hpp"
#include "structure_passes.hpp"

#include <hip/hip_runtime.h>

namespace spmv_acc {
namespace {

using namespace dev;
using namespace passes;

// m > 0; the census has passed.
__global__ __launch_bounds__(kThreads) void strength_sd_kernel(int m, int nnz, const int *__restrict__ rowptr, const int *__restrict__ colindex,
                                                               const double *__restrict__ value, double *__restrict__ sd) {
  const long long stride = static_cast<long long>(gridDim.x) * kThreads;
  for (long long r = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; r < m; r += stride) {
    const int i = static_cast<int>(r);
    int hi;
    const int lo = row_extent(rowptr, nnz, i, &hi);
    const int p = first_at_least(colindex, lo, hi, i);
    double root = 0.0; // (a row without a stored diagonal)
    if (p < hi && colindex[p] == i) root = sqrt(fabs(value[p]));
    sd[i] = root;
  }
}

// the edge's right-hand side: the two roots first (the product commutes: both ends of an edge get the same bits), then theta
__device__ __forceinline__ double strength_rhs(double sd_i, double sd_j, double theta) {
#pragma clang fp contract(off)
  const double roots = sd_i * sd_j;
  return roots * theta;
}

// One workgroup per tile of kStrengthRankTile of the nnz + 1 items, blocks stride over the tiles beyond the grid.  m > 0; the census has
// passed: every column lies in [0, m) and every off-diagonal entry has its mirror (neither is relied on for an address).
__global__ __launch_bounds__(kThreads) void strength_flags_kernel(int m, int nnz, const int *__restrict__ rowptr, const int *__restrict__ colindex,
                                                                  const double *__restrict__ value, const double *__restrict__ sd, double theta,
                                                                  int *__restrict__ flag) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const long long items = static_cast<long long>(nnz) + 1;
  const long long ntiles = (items + kStrengthRankTile - 1) / kStrengthRankTile;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) { // (block-uniform)
    const long long base = tile * kStrengthRankTile + static_cast<long long>(wave) * kWave;
    if (base >= items) continue; // (wave-uniform)
    const long long last = (base + kWave < items ? base + kWave : items) - 1;
    const long long p = base + lane;
    if (p > last) continue;
    if (p == nnz) {
      flag[p] = 0; // (the scan's closing element: not kept)
      continue;
    }
    const int i = wave_row_of(rowptr, m, base, last < nnz ? last : static_cast<long long>(nnz) - 1, p);
    const int j = load_stream(colindex + p);
    int keep = 1; // (a stored diagonal entry is always kept)
    if (j != i) {
      keep = 0;
      if (static_cast<unsigned>(j) < static_cast<unsigned>(m)) { // (a column outside [0, m) is never an address)
        const double rhs = strength_rhs(sd[i], sd[j], theta);
        bool strong = fabs(load_stream(value + p)) >= rhs;
        int chi;
        const int clo = row_extent(rowptr, nnz, j, &chi);
        const int q = first_at_least(colindex, clo, chi, i);
        if (q < chi && colindex[q] == i) strong = strong || fabs(value[q]) >= rhs; // (a search that misses: the entry's own comparison alone)
        keep = strong ? 1 : 0;
      }
    }
    flag[p] = keep;
  }
}

__global__ __launch_bounds__(kThreads) void strength_ptrs_kernel(int m, int nnz, const int *__restrict__ rowptr, const int *__restrict__ pos,
                                                                 int *__restrict__ s_rowptr, int *__restrict__ drop_ptr) {
  const long long stride = static_cast<long long>(gridDim.x) * kThreads;
  const int nnz_s = pos[nnz];
  for (long long i = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; i <= m; i += stride) {
    int p = rowptr[i]; // (0 <= p <= nnz by the census; held inside the scan regardless)
    p = p < 0 ? 0 : (p > nnz ? nnz : p);
    const int kept = pos[p];
    s_rowptr[i] = kept;
    drop_ptr[i] = nnz_s + (p - kept);
  }
}

// One workgroup per tile of kStrengthRankTile entries of A.  nnz > 0.
__global__ __launch_bounds__(kThreads) void strength_scatter_kernel(int nnz, const int *__restrict__ colindex, const int *__restrict__ flag,
                                                                    const int *__restrict__ pos, int *__restrict__ s_colindex,
                                                                    int *__restrict__ map) {
  const int nnz_s = pos[nnz];
  const long long ntiles = (static_cast<long long>(nnz) + kStrengthRankTile - 1) / kStrengthRankTile;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) { // (block-uniform)
    const long long p = tile * kStrengthRankTile + threadIdx.x;
    if (p >= nnz) continue;
    const int kept = load_stream(pos + p);
    const bool keep = load_stream(flag + p) != 0;
    long long k = keep ? kept : static_cast<long long>(nnz_s) + (p - kept); // (0 <= k < nnz: a permutation; held inside the caller's arrays regardless)
    k = k < 0 ? 0 : (k >= nnz ? static_cast<long long>(nnz) - 1 : k);
    map[k] = static_cast<int>(p);
    if (keep) s_colindex[k] = load_stream(colindex + p);
  }
}

// the terms of a row's dropped run: value at position map[p] of A (0 <= p < nnz); a position outside [0, nnz) reads value[0] and counts as +0.0
struct StrengthTerms {
  const int *__restrict__ map;
  const double *__restrict__ value;
  int nnz;
  __device__ __forceinline__ int index(int p) const { return map[p]; }
  __device__ __forceinline__ double load(int u) const { return value[static_cast<unsigned>(u) < static_cast<unsigned>(nnz) ? u : 0]; }
  __device__ __forceinline__ double term(int u, double v) const { return static_cast<unsigned>(u) < static_cast<unsigned>(nnz) ? v : 0.0; }
  __device__ __forceinline__ double fetch(int p) const {
    const int u = index(p);
    return term(u, load(u));
  }
};

static_assert(kStrengthLumpWaveChunk == kWave * kStrengthLumpPerLane && kStrengthLumpTile == (kThreads / kWave) * kStrengthLumpWaveChunk,
              "sum_runs derives its tile from kStrengthLumpPerLane");

// the lumped diagonal of row i from its lump (strength.hpp THE VALUES, 1).  0 <= i < m
__device__ __forceinline__ double strength_lumped(int i, int nnz, int nnz_s, const int *__restrict__ s_rowptr, const int *__restrict__ s_colindex,
                                                  const int *__restrict__ map, const int *__restrict__ drop_ptr,
                                                  const double *__restrict__ value, double lump) {
#pragma clang fp contract(off)
  int hi;
  const int lo = row_extent(s_rowptr, nnz_s, i, &hi);
  const int q = first_at_least(s_colindex, lo, hi, i);
  if (q >= hi || s_colindex[q] != i) return 0.0; // (no diagonal in S's row: the lump is discarded)
  const int u = map[q];
  const double a = static_cast<unsigned>(u) < static_cast<unsigned>(nnz) ? value[u] : 0.0;
  int dhi;
  const int dlo = row_extent(drop_ptr, nnz, i, &dhi);
  return dhi > dlo ? a + lump : a; // (an empty run: the bits of a_ii)
}

// One workgroup per tile of kStrengthLumpTile rows, blocks stride over the tiles beyond the grid.  m > 0 (the launcher checks).
__global__ __launch_bounds__(kThreads) void strength_diag_kernel(int m, int nnz, int nnz_s, const int *__restrict__ s_rowptr,
                                                                 const int *__restrict__ s_colindex, const int *__restrict__ map,
                                                                 const int *__restrict__ drop_ptr, const double *__restrict__ value, double *diag) {
  sum_runs<kStrengthLumpPerLane>(nnz, m, drop_ptr, StrengthTerms{map, value, nnz}, diag);
  // the diagonal, by the lane that wrote the lump (sum_runs' own tiling)
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const long long ntiles = (static_cast<long long>(m) + kStrengthLumpTile - 1) / kStrengthLumpTile;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) { // (block-uniform)
    const long long base = tile * kStrengthLumpTile + static_cast<long long>(wave) * kStrengthLumpWaveChunk;
#pragma unroll
    for (int k = 0; k < kStrengthLumpPerLane; ++k) {
      const long long i = base + k * kWave + lane;
      if (i < m) diag[i] = strength_lumped(static_cast<int>(i), nnz, nnz_s, s_rowptr, s_colindex, map, drop_ptr, value, diag[i]);
    }
  }
}

// the value of S's entry in row i at column c (strength.hpp THE VALUES, 2): v = A's value there, d = diag[i]
__device__ __forceinline__ double strength_entry(bool on_diag, double v, double d, double omega) {
#pragma clang fp contract(off)
  if (omega == 0.0) return on_diag ? d : v; // the filtered matrix: bits copied
  if (d == 0.0) return on_diag ? 1.0 : 0.0; // an identity row
  if (on_diag) return 1.0 - omega;
  const double scaled = -omega * v;
  return scaled / d;
}

static_assert(kStrengthWaveChunk == kWave * kStrengthPerLane && kStrengthTile == (kThreads / kWave) * kStrengthWaveChunk,
              "a workgroup's tile is its four wavefronts' chunks");

// One workgroup per tile of kStrengthTile S entries, blocks stride over the tiles beyond the grid.  m > 0, nnz_s > 0 (the launcher checks).
__global__ __launch_bounds__(kThreads) void strength_values_kernel(int m, int nnz, int nnz_s, const int *__restrict__ s_rowptr,
                                                                   const int *__restrict__ s_colindex, const int *__restrict__ map,
                                                                   const double *__restrict__ value, const double *__restrict__ diag, double omega,
                                                                   double *__restrict__ s_value) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const long long ntiles = (static_cast<long long>(nnz_s) + kStrengthTile - 1) / kStrengthTile;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) { // (block-uniform)
    const long long base = tile * kStrengthTile + static_cast<long long>(wave) * kStrengthWaveChunk;
    if (base >= nnz_s) continue; // (wave-uniform)
    const long long last = (base + kStrengthWaveChunk < nnz_s ? base + kStrengthWaveChunk : nnz_s) - 1;
    int r_last;
    const int r_first = wave_end_rows(s_rowptr, m, base, last, &r_last); // (inside [0, m) whatever s_rowptr holds)
    int u[kStrengthPerLane], c[kStrengthPerLane], row[kStrengthPerLane];
    double v[kStrengthPerLane], d[kStrengthPerLane];
#pragma unroll
    for (int k = 0; k < kStrengthPerLane; ++k) {
      const long long j = base + k * kWave + lane;
      u[k] = -1;
      c[k] = -1;
      if (j < nnz_s) {
        u[k] = load_stream(map + j);
        c[k] = load_stream(s_colindex + j);
      }
    }
#pragma unroll
    for (int k = 0; k < kStrengthPerLane; ++k) {
      const long long j = base + k * kWave + lane;
      row[k] = j < nnz_s ? last_at_most(s_rowptr, r_first, r_last, j) : r_first;
    }
#pragma unroll
    for (int k = 0; k < kStrengthPerLane; ++k) { // the map is the CALLER's array here: an index outside the value array gives +0.0
      v[k] = 0.0;
      if (static_cast<unsigned>(u[k]) < static_cast<unsigned>(nnz)) v[k] = value[u[k]];
      d[k] = diag[row[k]];
    }
#pragma unroll
    for (int k = 0; k < kStrengthPerLane; ++k) {
      const long long j = base + k * kWave + lane;
      if (j < nnz_s) s_value[j] = strength_entry(c[k] == row[k], v[k], d[k], omega);
    }
  }
}

} // namespace

void launch_strength_sd(hipStream_t stream, int m, int nnz, const int *rowptr, const int *colindex, const double *value, double *sd) {
  if (m <= 0) return;
  SPMV_ACC_LAUNCH(strength_sd_kernel, dim3(grid_for(m, kThreads)), dim3(kThreads), 0, stream, m, nnz, rowptr, colindex, value, sd);
}

void launch_strength_flags(hipStream_t stream, int m, int nnz, const int *rowptr, const int *colindex, const double *value, const double *sd,
                           double theta, int *flag) {
  if (m <= 0) return;
  SPMV_ACC_LAUNCH(strength_flags_kernel, dim3(grid_for(static_cast<long long>(nnz) + 1, kStrengthRankTile)), dim3(kThreads), 0, stream, m, nnz,
                  rowptr, colindex, value, sd, theta, flag);
}

void launch_strength_ptrs(hipStream_t stream, int m, int nnz, const int *rowptr, const int *pos, int *s_rowptr, int *drop_ptr) {
  if (m <= 0) return;
  SPMV_ACC_LAUNCH(strength_ptrs_kernel, dim3(grid_for(static_cast<long long>(m) + 1, kThreads)), dim3(kThreads), 0, stream, m, nnz, rowptr, pos,
                  s_rowptr, drop_ptr);
}

void launch_strength_scatter(hipStream_t stream, int nnz, const int *colindex, const int *flag, const int *pos, int *s_colindex, int *map) {
  if (nnz <= 0) return;
  SPMV_ACC_LAUNCH(strength_scatter_kernel, dim3(grid_for(nnz, kStrengthRankTile)), dim3(kThreads), 0, stream, nnz, colindex, flag, pos, s_colindex,
                  map);
}

void launch_strength_diag(hipStream_t stream, int m, int nnz, int nnz_s, const int *s_rowptr, const int *s_colindex, const int *map,
                          const int *drop_ptr, const double *value, double *diag) {
  if (m <= 0) return;
  SPMV_ACC_LAUNCH(strength_diag_kernel, dim3(grid_for(m, kStrengthLumpTile)), dim3(kThreads), 0, stream, m, nnz, nnz_s, s_rowptr, s_colindex, map,
                  drop_ptr, value, diag);
}

void launch_strength_values(hipStream_t stream, int m, int nnz, int nnz_s, const int *s_rowptr, const int *s_colindex, const int *map,
                            const double *value, const double *diag, double omega, double *s_value) {
  if (m <= 0 || nnz_s <= 0) return;
  SPMV_ACC_LAUNCH(strength_values_kernel, dim3(grid_for(nnz_s, kStrengthTile)), dim3(kThreads), 0, stream, m, nnz, nnz_s, s_rowptr, s_colindex, map,
                  value, diag, omega, s_value);
}

} // namespace spmv_acc
