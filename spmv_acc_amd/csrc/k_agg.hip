// k_agg.hip -- the kernels of the aggregation coarsening (the aggregates' definition, the round form, the tentative values and their summation
// order, size rules and launcher declarations in agg.hpp, engine in agg.cpp).  The census, the sort keys and the pointer pass are k_gs.hip's.
//
// No reference counterpart: hpcde/spmv-acc multiplies a matrix by a vector.
//
// No atomics and no waiting anywhere: every output is written by exactly one lane, every dependency is a kernel boundary.  VGPRs as compiled
// for gfx950 (wave64; no scratch, no AGPR, 8 waves per SIMD in all):
// 1. Neighbourhood pass (agg_max_kernel, 26 VGPRs; the analysis' hot path, twice per round): kAggLaneGroup lanes per row, grid-striding.  A row reads
//    its columns and gathers one 64-bit key per entry, four entries a step, all loads of a step before any compare (max is idempotent: a
//    position beyond the row reads the row's first again); the maximum over the row and its own key goes to the other buffer.  A root's row is
//    not read: its maximum is kAggRoot.
// 2. Deciding pass (agg_decide_kernel, 36): the same gather on T1 for the undecided rows only -- after the first rounds most rows skip it --;
//    the row's key is decided in place (it reads T1 of others and its own key only); the rows still undecided are counted per wavefront.
// 3. Keys (agg_init_kernel, 7), root flags (agg_flags_kernel, 8), assignment A (agg_assign_roots_kernel, 12) and B (agg_assign_rest_kernel, 11):
//    one row per lane, run once per call; B reads A's buffer and writes the caller's, and counts the rows it could not assign.
// 4. Norms (agg_norms_kernel, 32; per step): structure_passes.hpp sum_runs on the squares b[agg_rows[p]]^2, each rounded on its own, then every
//    lane takes the square root of the sums it has just written (the same lane, the same addresses: program order).
// 5. Values (agg_values_kernel, 18; per step): p_value[i] = b[i] / bc[agg[i]], r_value[p] = the same quotient for row agg_rows[p], recomputed.
#include "agg.hpp"
#include "structure_passes.hpp"

#include <hip/hip_runtime.h>

namespace spmv_acc {
namespace {

using namespace dev;
using namespace passes;
using u64 = unsigned long long;

static_assert(kAggLaneGroup >= 1 && kAggLaneGroup <= kWave && (kAggLaneGroup & (kAggLaneGroup - 1)) == 0, "a lane group is a power of two inside a wavefront");

__device__ __forceinline__ u64 larger(u64 a, u64 b) { return a > b ? a : b; }
__device__ __forceinline__ u64 key_of(const u64 *__restrict__ in, int m, int u, u64 otherwise) {
  return static_cast<unsigned>(u) < static_cast<unsigned>(m) ? in[u] : otherwise; // (a column outside [0, m) is never an address)
}

// the maximum of `in` over the closed neighbourhood of row v, `own` = in[v]; lane l of the row's G lanes, every lane returns it
template <int G>
__device__ __forceinline__ u64 neighbourhood_max(int m, int nnz, const int *__restrict__ rowptr, const int *__restrict__ colindex,
                                                 const u64 *__restrict__ in, int v, int l, u64 own) {
  int hi;
  const int lo = row_extent(rowptr, nnz, v, &hi);
  u64 best = own;
  for (int p = lo + l; p < hi; p += 4 * G) { // four entries a step; a position beyond the row reads p again
    const int p1 = p + G, p2 = p + 2 * G, p3 = p + 3 * G;
    const int u0 = colindex[p], u1 = colindex[p1 < hi ? p1 : p], u2 = colindex[p2 < hi ? p2 : p], u3 = colindex[p3 < hi ? p3 : p];
    const u64 k0 = key_of(in, m, u0, own), k1 = key_of(in, m, u1, own), k2 = key_of(in, m, u2, own), k3 = key_of(in, m, u3, own);
    best = larger(larger(best, k0), larger(larger(k1, k2), k3));
  }
  for (int off = G / 2; off > 0; off >>= 1) best = larger(best, __shfl_xor(best, off, kWave));
  return best;
}

// gridDim.x <= kCooCheckBlocks.  m > 0; the census has passed.  in and out are different arrays.
template <int G>
__global__ __launch_bounds__(kThreads) void agg_max_kernel(int m, int nnz, const int *__restrict__ rowptr, const int *__restrict__ colindex,
                                                           const u64 *__restrict__ in, u64 *__restrict__ out) {
  const int l = threadIdx.x & (G - 1);
  const long long stride = static_cast<long long>(gridDim.x) * (kThreads / G);
  for (long long r = static_cast<long long>(blockIdx.x) * (kThreads / G) + threadIdx.x / G; r < m; r += stride) { // (uniform in a lane group)
    const int v = static_cast<int>(r);
    u64 best = in[v];
    if (best != kAggRoot) best = neighbourhood_max<G>(m, nnz, rowptr, colindex, in, v, l, best);
    if (l == 0) out[v] = best;
  }
}

// gridDim.x <= kCooCheckBlocks.  m > 0.  t1 and key are different arrays; key[v] is read and written by the lanes of row v only.
template <int G>
__global__ __launch_bounds__(kThreads) void agg_decide_kernel(int m, int nnz, const int *__restrict__ rowptr, const int *__restrict__ colindex,
                                                              const u64 *__restrict__ t1, u64 *__restrict__ key, unsigned *__restrict__ slots) {
  unsigned undecided = 0;
  const int l = threadIdx.x & (G - 1);
  const long long stride = static_cast<long long>(gridDim.x) * (kThreads / G);
  for (long long r = static_cast<long long>(blockIdx.x) * (kThreads / G) + threadIdx.x / G; r < m; r += stride) { // (uniform in a lane group)
    const int v = static_cast<int>(r);
    const u64 mine = key[v];
    if (mine == kAggRoot || mine == kAggOut) continue;
    const u64 t2 = neighbourhood_max<G>(m, nnz, rowptr, colindex, t1, v, l, t1[v]);
    if (t2 == kAggRoot) { // a root within distance 2
      if (l == 0) key[v] = kAggOut;
    } else if (t2 == mine) { // nothing undecided of higher priority within distance 2
      if (l == 0) key[v] = kAggRoot;
    } else {
      undecided += l == 0 ? 1u : 0u;
    }
  }
  count_to_slot(undecided, slots);
}

__global__ __launch_bounds__(kThreads) void agg_init_kernel(int m, u64 *__restrict__ key) {
  const long long stride = static_cast<long long>(gridDim.x) * kThreads;
  for (long long v = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; v < m; v += stride) key[v] = agg_key(static_cast<unsigned>(v));
}

__global__ __launch_bounds__(kThreads) void agg_flags_kernel(int m, const u64 *__restrict__ key, int *__restrict__ flag) {
  const long long stride = static_cast<long long>(gridDim.x) * kThreads;
  for (long long v = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; v <= m; v += stride) flag[v] = v < m && key[v] == kAggRoot ? 1 : 0;
}

__global__ __launch_bounds__(kThreads) void agg_assign_roots_kernel(int m, int nnz, const int *__restrict__ rowptr, const int *__restrict__ colindex,
                                                                    const int *__restrict__ flag, const int *__restrict__ id,
                                                                    int *__restrict__ first) {
  const long long stride = static_cast<long long>(gridDim.x) * kThreads;
  for (long long r = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; r < m; r += stride) {
    const int v = static_cast<int>(r);
    int a = -1;
    if (flag[v]) {
      a = id[v];
    } else {
      int hi;
      const int lo = row_extent(rowptr, nnz, v, &hi);
      for (int p = lo; p < hi && a < 0; ++p) { // (at most one neighbour is a root)
        const int u = colindex[p];
        if (static_cast<unsigned>(u) < static_cast<unsigned>(m) && flag[u]) a = id[u];
      }
    }
    first[v] = a;
  }
}

// gridDim.x <= kCooCheckBlocks.  first and agg are different arrays.
__global__ __launch_bounds__(kThreads) void agg_assign_rest_kernel(int m, int nnz, const int *__restrict__ rowptr, const int *__restrict__ colindex,
                                                                   const int *__restrict__ first, int *__restrict__ agg,
                                                                   unsigned *__restrict__ slots) {
  unsigned unassigned = 0;
  const long long stride = static_cast<long long>(gridDim.x) * kThreads;
  for (long long r = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; r < m; r += stride) {
    const int v = static_cast<int>(r);
    int a = first[v];
    if (a < 0) {
      int hi;
      const int lo = row_extent(rowptr, nnz, v, &hi);
      unsigned best = ~0u; // (-1 as unsigned is the largest: the smallest assigned id wins)
      for (int p = lo; p < hi; ++p) {
        const int u = colindex[p];
        if (static_cast<unsigned>(u) >= static_cast<unsigned>(m)) continue;
        const unsigned f = static_cast<unsigned>(first[u]);
        best = f < best ? f : best;
      }
      a = static_cast<int>(best);
    }
    agg[v] = a;
    unassigned += a < 0 ? 1u : 0u;
  }
  count_to_slot(unassigned, slots);
}

// the terms of an aggregate's run: the rounded square of b at row agg_rows[p] (0 <= p < m); a row outside [0, m) reads b[0] and counts as +0.0
struct AggTerms {
  const int *__restrict__ agg_rows;
  const double *__restrict__ b; // nullptr: all ones
  int m;
  __device__ __forceinline__ int index(int p) const { return agg_rows[p]; }
  __device__ __forceinline__ double load(int i) const { return b != nullptr ? b[static_cast<unsigned>(i) < static_cast<unsigned>(m) ? i : 0] : 1.0; }
  __device__ __forceinline__ double term(int i, double v) const {
#pragma clang fp contract(off)
    const double prod = v * v; // rounded here, added by the caller
    return static_cast<unsigned>(i) < static_cast<unsigned>(m) ? prod : 0.0;
  }
  __device__ __forceinline__ double fetch(int p) const {
    const int i = index(p);
    return term(i, load(i));
  }
};

static_assert(kAggWaveChunk == kWave * kAggPerLane && kAggTile == (kThreads / kWave) * kAggWaveChunk, "sum_runs derives its tile from kAggPerLane");

// One workgroup per tile of kAggTile aggregates, blocks stride over the tiles beyond the grid.  m > 0, naggs > 0 (the launcher checks).
__global__ __launch_bounds__(kThreads) void agg_norms_kernel(int m, int naggs, const int *__restrict__ agg_ptr, const int *__restrict__ agg_rows,
                                                             const double *__restrict__ b, double *bc) {
  sum_runs<kAggPerLane>(m, naggs, agg_ptr, AggTerms{agg_rows, b, m}, bc);
  // the square roots, by the lane that wrote the sum (sum_runs' own tiling)
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const long long ntiles = (static_cast<long long>(naggs) + kAggTile - 1) / kAggTile;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) { // (block-uniform)
    const long long base = tile * kAggTile + static_cast<long long>(wave) * kAggWaveChunk;
#pragma unroll
    for (int k = 0; k < kAggPerLane; ++k) {
      const long long j = base + k * kWave + lane;
      if (j < naggs) bc[j] = sqrt(bc[j]);
    }
  }
}

// the entry of P in row i (agg.hpp): b[i] / bc[agg[i]], +0.0 for a zero norm or an aggregate outside [0, naggs).  0 <= i < m
__device__ __forceinline__ double agg_quotient(int naggs, const int *__restrict__ agg, const double *__restrict__ b, const double *__restrict__ bc, int i) {
  const int a = agg[i];
  if (static_cast<unsigned>(a) >= static_cast<unsigned>(naggs)) return 0.0;
  const double d = bc[a];
  return d == 0.0 ? 0.0 : (b != nullptr ? b[i] : 1.0) / d;
}

__global__ __launch_bounds__(kThreads) void agg_values_kernel(int m, int naggs, const int *__restrict__ agg, const int *__restrict__ agg_rows,
                                                              const double *__restrict__ b, const double *__restrict__ bc,
                                                              double *__restrict__ p_value, double *__restrict__ r_value) {
  const long long stride = static_cast<long long>(gridDim.x) * kThreads;
  for (long long t = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; t < m; t += stride) {
    const int i = static_cast<int>(t);
    p_value[i] = agg_quotient(naggs, agg, b, bc, i);
    if (r_value != nullptr) {
      const int j = load_stream(agg_rows + i);
      r_value[i] = static_cast<unsigned>(j) < static_cast<unsigned>(m) ? agg_quotient(naggs, agg, b, bc, j) : 0.0;
    }
  }
}

} // namespace

void launch_agg_max(hipStream_t stream, int m, int nnz, const int *rowptr, const int *colindex, const unsigned long long *in,
                    unsigned long long *out) {
  if (m <= 0) return;
  SPMV_ACC_LAUNCH(agg_max_kernel<kAggLaneGroup>, dim3(census_grid_for(m, kThreads / kAggLaneGroup)), dim3(kThreads), 0, stream, m, nnz, rowptr,
                  colindex, in, out);
}

void launch_agg_decide(hipStream_t stream, int m, int nnz, const int *rowptr, const int *colindex, const unsigned long long *t1,
                       unsigned long long *key, unsigned *slots) {
  if (m <= 0) return;
  SPMV_ACC_LAUNCH(agg_decide_kernel<kAggLaneGroup>, dim3(census_grid_for(m, kThreads / kAggLaneGroup)), dim3(kThreads), 0, stream, m, nnz, rowptr,
                  colindex, t1, key, slots);
}

void launch_agg_init(hipStream_t stream, int m, unsigned long long *key) {
  if (m <= 0) return;
  SPMV_ACC_LAUNCH(agg_init_kernel, dim3(grid_for(m, kThreads)), dim3(kThreads), 0, stream, m, key);
}

void launch_agg_flags(hipStream_t stream, int m, const unsigned long long *key, int *flag) {
  if (m <= 0) return;
  SPMV_ACC_LAUNCH(agg_flags_kernel, dim3(grid_for(static_cast<long long>(m) + 1, kThreads)), dim3(kThreads), 0, stream, m, key, flag);
}

void launch_agg_assign_roots(hipStream_t stream, int m, int nnz, const int *rowptr, const int *colindex, const int *flag, const int *id,
                             int *first) {
  if (m <= 0) return;
  SPMV_ACC_LAUNCH(agg_assign_roots_kernel, dim3(grid_for(m, kThreads)), dim3(kThreads), 0, stream, m, nnz, rowptr, colindex, flag, id, first);
}

void launch_agg_assign_rest(hipStream_t stream, int m, int nnz, const int *rowptr, const int *colindex, const int *first, int *agg,
                            unsigned *slots) {
  if (m <= 0) return;
  SPMV_ACC_LAUNCH(agg_assign_rest_kernel, dim3(census_grid_for(m, kThreads)), dim3(kThreads), 0, stream, m, nnz, rowptr, colindex, first, agg,
                  slots);
}

void launch_agg_norms(hipStream_t stream, int m, int naggs, const int *agg_ptr, const int *agg_rows, const double *b, double *bc) {
  if (m <= 0 || naggs <= 0) return;
  SPMV_ACC_LAUNCH(agg_norms_kernel, dim3(grid_for(naggs, kAggTile)), dim3(kThreads), 0, stream, m, naggs, agg_ptr, agg_rows, b, bc);
}

void launch_agg_values(hipStream_t stream, int m, int naggs, const int *agg, const int *agg_rows, const double *b, const double *bc,
                       double *p_value, double *r_value) {
  if (m <= 0) return;
  SPMV_ACC_LAUNCH(agg_values_kernel, dim3(grid_for(m, kThreads)), dim3(kThreads), 0, stream, m, naggs, agg, agg_rows, b, bc, p_value, r_value);
}

} // namespace spmv_acc
