// k_dense.hip -- the kernels of the dense coarse-level solve (the inverse's definition, the apply's summation order, size rules and launcher
// declarations in dense.hpp, engine in dense.cpp).
//
// No reference counterpart: hpcde/spmv-acc multiplies a matrix by a vector.
//
// No atomics and no waiting on another workgroup anywhere: every output is written by exactly one lane, every dependency is a kernel boundary;
// the pivot search is ONE workgroup, which combines its lanes in LDS behind its own barrier.  VGPRs as compiled for gfx950 (wave64; no scratch,
// no AGPR, 8 waves per SIMD in all):
// 1. Fill (dense_fill_kernel, 9) and scatter (dense_scatter_kernel, 16): E = [0 | I], then the stored entries of A, one row per lane (rows
//    strictly ascend, so no position is written twice; a column outside [0, m) is never turned into an address).
// 2. Pivot search (dense_pivot_kernel, 10; one workgroup): a lane walks the rows k + t, k + t + 256, ... of column k and keeps the largest
//    non-NaN magnitude with the smallest row (its rows ascend, so `>` alone keeps the smallest); the 256 candidates are combined as a tree in
//    LDS by (magnitude, then smaller row); lane 0 writes p, piv and the first info.
// 3. Row pass (dense_row_kernel, 28): lanes [0, 2m) swap and scale one column of the rows k and p each, lanes [2m, 3m) copy the multipliers.
// 4. Update (dense_update_kernel, 10): a workgroup owns kDenseTile columns of one row -- the row and its multiplier are block-uniform, no lane
//    divides --; the product and the subtraction are two instructions (contraction is off).
// 5. Copy (dense_copy_kernel, 8): the right half of E to inv.
// 6. Apply (dense_apply_kernel, 40; the per-step hot path): one wavefront per row; a step loads four 512-B lines of the row and of b before
//    any arithmetic and adds the four products in order; the 64 partial sums go through the DPP butterfly (neighbouring lanes first: the
//    balanced tree of gs.hpp).  inv is read with the default cache policy: a coarsest level is applied once per cycle and is small enough to
//    be found in the cache again (supposed, not timed against the streaming policy).
#include "dense.hpp"
#include "structure_passes.hpp"

#include <climits>

namespace spmv_acc {
namespace {

using namespace dev;
using namespace passes;
using u64 = unsigned long long;

static_assert(kDenseTile == kThreads && kDensePivotThreads == kThreads && kDenseRowsPerBlock == kThreads / kWave, "one lane per item of a tile");

// the tiles of a row-major array of `rows` rows whose rows are cut into pieces of kDenseTile columns: tile -> (row, first column)
__device__ __forceinline__ int tiles_per_row(int width) { return (width + kDenseTile - 1) / kDenseTile; }

__global__ __launch_bounds__(kThreads) void dense_fill_kernel(int m, double *__restrict__ E) {
  const int w = 2 * m, tpr = tiles_per_row(w);
  const long long ntiles = static_cast<long long>(m) * tpr;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) { // (block-uniform)
    const int i = static_cast<int>(tile / tpr);
    const int j = static_cast<int>(tile - static_cast<long long>(i) * tpr) * kDenseTile + threadIdx.x;
    if (j < w) E[static_cast<size_t>(i) * w + j] = j == m + i ? 1.0 : 0.0;
  }
}

// m > 0; the census has passed (rows are read clamped all the same)
__global__ __launch_bounds__(kThreads) void dense_scatter_kernel(int m, int nnz, const int *__restrict__ rowptr, const int *__restrict__ colindex,
                                                                 const double *__restrict__ value, double *__restrict__ E) {
  const int w = 2 * m;
  const long long stride = static_cast<long long>(gridDim.x) * kThreads;
  for (long long r = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; r < m; r += stride) {
    const int i = static_cast<int>(r);
    int hi;
    const int lo = row_extent(rowptr, nnz, i, &hi);
    for (int p = lo; p < hi; ++p) {
      const int c = colindex[p];
      if (static_cast<unsigned>(c) < static_cast<unsigned>(m)) E[static_cast<size_t>(i) * w + c] = value[p];
    }
  }
}

// ONE workgroup.  0 <= k < m.  state: dense.hpp launch_dense_pivot
__global__ __launch_bounds__(kThreads) void dense_pivot_kernel(int m, int k, const double *__restrict__ E, u64 *__restrict__ state) {
  __shared__ double s_mag[kDensePivotThreads];
  __shared__ int s_row[kDensePivotThreads];
  const int w = 2 * m, t = threadIdx.x;
  double best = -1.0; // below every magnitude: a lane without a non-NaN entry never wins
  int row = INT_MAX;
  for (int i = k + t; i < m; i += kDensePivotThreads) {
    const double a = fabs(E[static_cast<size_t>(i) * w + k]);
    if (a > best) { // (a NaN compares false; the lane's rows ascend, so a tie keeps the smaller row)
      best = a;
      row = i;
    }
  }
  s_mag[t] = best;
  s_row[t] = row;
  __syncthreads();
  for (int off = kDensePivotThreads / 2; off > 0; off >>= 1) {
    if (t < off) {
      const double om = s_mag[t + off];
      const int orow = s_row[t + off];
      if (om > s_mag[t] || (om == s_mag[t] && orow < s_row[t])) {
        s_mag[t] = om;
        s_row[t] = orow;
      }
    }
    __syncthreads();
  }
  if (t == 0) {
    const int p = s_row[0] == INT_MAX ? k : s_row[0]; // all NaN: p = k
    const double piv = E[static_cast<size_t>(p) * w + k];
    state[0] = static_cast<u64>(p);
    state[1] = static_cast<u64>(__double_as_longlong(piv));
    const bool bad = !(fabs(piv) > 0.0 && fabs(piv) < __builtin_huge_val()); // zero, NaN or infinite
    if (bad && state[2] == 0) state[2] = static_cast<u64>(k + 1);
  }
}

// 0 <= k < m.  Lanes [0, 2m): column j of the rows k and p; lanes [2m, 3m): the multiplier of row i.  E is read and written (different
// elements: dense.hpp PASSES b): not __restrict__.
__global__ __launch_bounds__(kThreads) void dense_row_kernel(int m, int k, double *E, const u64 *__restrict__ state, double *__restrict__ prow,
                                                             double *__restrict__ f) {
#pragma clang fp contract(off)
  const int w = 2 * m;
  int p = static_cast<int>(state[0]);
  p = p < k || p >= m ? k : p; // (the pivot launch wrote a row of [k, m): never another address whatever the state holds)
  const double piv = __longlong_as_double(static_cast<long long>(state[1]));
  const long long items = 3ll * m;
  const long long stride = static_cast<long long>(gridDim.x) * kThreads;
  for (long long t = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; t < items; t += stride) {
    if (t < w) {
      const int j = static_cast<int>(t);
      const double a_k = E[static_cast<size_t>(k) * w + j];
      const double a_p = p != k ? E[static_cast<size_t>(p) * w + j] : a_k;
      const double q = a_p / piv;
      E[static_cast<size_t>(k) * w + j] = q;
      prow[j] = q;
      if (p != k) {
        E[static_cast<size_t>(p) * w + j] = a_k;
        if (j == k) f[p] = a_k; // the multiplier of the row that was row k
      }
    } else {
      const int i = static_cast<int>(t - w);
      if (i != k && i != p) f[i] = E[static_cast<size_t>(i) * w + k];
    }
  }
}

// 0 <= k < m.  One workgroup per kDenseTile columns of one row.
__global__ __launch_bounds__(kThreads) void dense_update_kernel(int m, int k, double *__restrict__ E, const double *__restrict__ prow,
                                                                const double *__restrict__ f) {
#pragma clang fp contract(off)
  const int w = 2 * m, tpr = tiles_per_row(w);
  const long long ntiles = static_cast<long long>(m) * tpr;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) { // (block-uniform)
    const int i = static_cast<int>(tile / tpr);
    if (i == k) continue;
    const int j = static_cast<int>(tile - static_cast<long long>(i) * tpr) * kDenseTile + threadIdx.x;
    if (j < w) {
      const double prod = f[i] * prow[j];
      E[static_cast<size_t>(i) * w + j] = E[static_cast<size_t>(i) * w + j] - prod;
    }
  }
}

__global__ __launch_bounds__(kThreads) void dense_copy_kernel(int m, const double *__restrict__ E, double *__restrict__ inv) {
  const int w = 2 * m, tpr = tiles_per_row(m);
  const long long ntiles = static_cast<long long>(m) * tpr;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) { // (block-uniform)
    const int i = static_cast<int>(tile / tpr);
    const int j = static_cast<int>(tile - static_cast<long long>(i) * tpr) * kDenseTile + threadIdx.x;
    if (j < m) inv[static_cast<size_t>(i) * m + j] = E[static_cast<size_t>(i) * w + m + j];
  }
}

// One wavefront per row, kDenseRowsPerBlock rows per workgroup, blocks stride over the rows beyond the grid.  m > 0.
__global__ __launch_bounds__(kThreads) void dense_apply_kernel(int m, const double *__restrict__ inv, const double *__restrict__ b,
                                                               double *__restrict__ x) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const long long stride = static_cast<long long>(gridDim.x) * kDenseRowsPerBlock;
  for (long long r = static_cast<long long>(blockIdx.x) * kDenseRowsPerBlock + wave; r < m; r += stride) { // (wave-uniform)
    const double *__restrict__ row = inv + static_cast<size_t>(r) * m;
    double part = 0.0; // a lane without a term holds +0.0
    int j = lane;
    if (j < m) {
      part = row[j] * b[j]; // the sum starts from the lane's first term, not from 0.0
      j += kWave;
      for (; j + 3 * kWave < m; j += 4 * kWave) { // four independent terms in flight, added in order
        const double r0 = row[j], r1 = row[j + kWave], r2 = row[j + 2 * kWave], r3 = row[j + 3 * kWave];
        const double b0 = b[j], b1 = b[j + kWave], b2 = b[j + 2 * kWave], b3 = b[j + 3 * kWave];
        const double t0 = r0 * b0, t1 = r1 * b1, t2 = r2 * b2, t3 = r3 * b3;
        part += t0;
        part += t1;
        part += t2;
        part += t3;
      }
      for (; j < m; j += kWave) {
        const double t0 = row[j] * b[j];
        part += t0;
      }
    }
    const double s = group_sum<64>(part);
    if (lane == 0) x[r] = s;
  }
}

} // namespace

void launch_dense_fill(hipStream_t stream, int m, double *E) {
  if (m <= 0 || m > kDenseMaxRows) return;
  SPMV_ACC_LAUNCH(dense_fill_kernel, dim3(grid_for(static_cast<long long>(m) * ((2 * m + kDenseTile - 1) / kDenseTile), 1)), dim3(kThreads), 0, stream,
                  m, E);
}

void launch_dense_scatter(hipStream_t stream, int m, int nnz, const int *rowptr, const int *colindex, const double *value, double *E) {
  if (m <= 0 || m > kDenseMaxRows || nnz <= 0) return;
  SPMV_ACC_LAUNCH(dense_scatter_kernel, dim3(grid_for(m, kDenseTile)), dim3(kThreads), 0, stream, m, nnz, rowptr, colindex, value, E);
}

void launch_dense_pivot(hipStream_t stream, int m, int k, const double *E, unsigned long long *state) {
  if (m <= 0 || m > kDenseMaxRows || k < 0 || k >= m) return;
  SPMV_ACC_LAUNCH(dense_pivot_kernel, dim3(1), dim3(kThreads), 0, stream, m, k, E, state);
}

void launch_dense_row(hipStream_t stream, int m, int k, double *E, const unsigned long long *state, double *prow, double *f) {
  if (m <= 0 || m > kDenseMaxRows || k < 0 || k >= m) return;
  SPMV_ACC_LAUNCH(dense_row_kernel, dim3(grid_for(3ll * m, kDenseTile)), dim3(kThreads), 0, stream, m, k, E, state, prow, f);
}

void launch_dense_update(hipStream_t stream, int m, int k, double *E, const double *prow, const double *f) {
  if (m <= 0 || m > kDenseMaxRows || k < 0 || k >= m) return;
  SPMV_ACC_LAUNCH(dense_update_kernel, dim3(grid_for(static_cast<long long>(m) * ((2 * m + kDenseTile - 1) / kDenseTile), 1)), dim3(kThreads), 0,
                  stream, m, k, E, prow, f);
}

void launch_dense_copy(hipStream_t stream, int m, const double *E, double *inv) {
  if (m <= 0 || m > kDenseMaxRows) return;
  SPMV_ACC_LAUNCH(dense_copy_kernel, dim3(grid_for(static_cast<long long>(m) * ((m + kDenseTile - 1) / kDenseTile), 1)), dim3(kThreads), 0, stream, m,
                  E, inv);
}

void launch_dense_apply(hipStream_t stream, int m, const double *inv, const double *b, double *x) {
  if (m <= 0) return; // (the apply has no cap of its own: inv is the caller's m * m doubles)
  SPMV_ACC_LAUNCH(dense_apply_kernel, dim3(grid_for(m, kDenseRowsPerBlock)), dim3(kThreads), 0, stream, m, inv, b, x);
}

} // namespace spmv_acc
