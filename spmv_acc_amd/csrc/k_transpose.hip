// k_transpose.hip -- the kernels of the transposed product (size rules and launcher declarations in transpose.hpp, engine in transpose.cpp).
//
// No reference counterpart: hpcde/spmv-acc never reads `trans` (api/spmv.h:13).
//
// 1. The stable device transpose.  CSR of A^T = the non-zeros of A ordered by (column, source position q).  The order comes from ONE stable
//    radix sort of the pairs (colindex[q], q) on the low bits that can differ below n (rocPRIM, header-only, as the row-block analysis and the
//    column encoding use its scan), so (t_colindex, t_value, perm) are a pure function of the input: a hub column of 10^5 entries is as ordered
//    as a column of two, and no float is ever added.  Around it: a bounds census of the columns (nothing is sorted or written if one lies
//    outside [0, n)), t_rowptr by one binary search per column in the sorted keys, each non-zero's row by one binary search in rowptr (the
//    lanes of a wavefront walk the same path), and one gather pass.
//
// 2. The scatter pass of spmv_acc_csr_spmv_t: y[col] += alpha * a * x[row] in STORAGE order.  The non-zero stream is cut into fixed tiles of
//    kTransTile, whatever the rows look like (a row of 120 001 non-zeros is 59 tiles like any other 120 001 non-zeros); lane l of a wavefront
//    owns the non-zeros base + l + 64 k, so every stream load is a contiguous 256 / 512 B per wavefront and -- where a row's columns are
//    neighbours -- so are the destinations of one atomic instruction, the shape the hardware adds at full rate.  Each wavefront finds the rows
//    of its 512 non-zeros' ends by binary search in rowptr and each lane its non-zeros' rows between them.  The adds are vector
//    global_atomic_add_f64 without return (no compare-and-swap loop: tests/test_transpose_host.py reads the assembly).  This is the one kernel
//    of the library whose sums depend on arrival order.  Every column is checked against n before it becomes an address.
#include "structure_passes.hpp"
#include "transpose.hpp"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

namespace spmv_acc {
namespace {

using namespace dev;
using namespace passes;

__global__ __launch_bounds__(kThreads) void transpose_check_kernel(const int *__restrict__ ci, int nnz, int n, unsigned *__restrict__ bad) {
  const long long stride = static_cast<long long>(gridDim.x) * kThreads;
  unsigned mine = 0;
  for (long long q = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; q < nnz; q += stride)
    mine += static_cast<unsigned>(ci[q]) >= static_cast<unsigned>(n) ? 1u : 0u;
  if (mine) atomicAdd(bad, mine); // (an integer count: no order to keep; never taken on a valid matrix)
}

__global__ __launch_bounds__(kThreads) void transpose_rowptr_kernel(const int *__restrict__ keys, int nnz, int n, int *__restrict__ t_rowptr) {
  const long long stride = static_cast<long long>(gridDim.x) * kThreads;
  for (long long c = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; c <= n; c += stride) t_rowptr[c] = first_at_least(keys, 0, nnz, c);
}

__global__ __launch_bounds__(kThreads) void transpose_rows_kernel(const int *__restrict__ rp, int m, int nnz, int *__restrict__ row_of) {
  const long long stride = static_cast<long long>(gridDim.x) * kThreads;
  for (long long q = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; q < nnz; q += stride)
    row_of[q] = last_at_most(rp, 0, m - 1, static_cast<int>(q));
}

__global__ __launch_bounds__(kThreads) void transpose_gather_kernel(int nnz, const int *__restrict__ perm, const int *__restrict__ row_of,
                                                                    const double *__restrict__ value, int *__restrict__ t_colindex,
                                                                    double *__restrict__ t_value) {
  const long long stride = static_cast<long long>(gridDim.x) * kThreads;
  for (long long p = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; p < nnz; p += stride) {
    const int q = perm[p]; // (the sort's own output: a permutation of 0 .. nnz - 1)
    t_colindex[p] = row_of[q];
    if (value) t_value[p] = value[q];
  }
}

// perm is the CALLER's array here: an entry outside [0, nnz) reads nothing (its output keeps its value)
__global__ __launch_bounds__(kThreads) void transpose_values_kernel(int nnz, const int *__restrict__ perm, const double *__restrict__ value,
                                                                    double *__restrict__ t_value) {
  const long long stride = static_cast<long long>(gridDim.x) * kThreads;
  for (long long p = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; p < nnz; p += stride) {
    const int q = perm[p];
    if (static_cast<unsigned>(q) < static_cast<unsigned>(nnz)) t_value[p] = value[q];
  }
}

__global__ __launch_bounds__(kThreads) void spmv_t_scale_kernel(int n, double beta, double *__restrict__ y) {
  const long long stride = static_cast<long long>(gridDim.x) * kThreads;
  for (long long c = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; c < n; c += stride) y[c] = beta == 0.0 ? 0.0 : beta * y[c];
}

// One workgroup per tile of kTransTile non-zeros in ABSOLUTE numbering (tile t = non-zeros [t * kTransTile, ...)), from the tile that holds
// rp[0] on: an un-rebased row sub-range (rowptr + r0, whole colindex / value arrays) starts at its own first tile.  Blocks stride over the
// tiles beyond the grid.  The view ends at min(rp[m], nnz_end): no non-zero without a row is ever read.
__global__ __launch_bounds__(kThreads) void spmv_t_scatter_kernel(int m, int n, int nnz_end, double alpha, const int *__restrict__ rp,
                                                                  const int *__restrict__ ci, const double *__restrict__ v,
                                                                  const double *__restrict__ x, double *__restrict__ y) {
  const int lo = rp[0];
  const int end_rp = rp[m];
  const int hi = end_rp < nnz_end ? end_rp : nnz_end;
  if (lo < 0 || hi <= lo) return;
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const long long ntiles = (static_cast<long long>(hi) + kTransTile - 1) / kTransTile;
  for (long long tile = lo / kTransTile + blockIdx.x; tile < ntiles; tile += gridDim.x) { // (block-uniform)
    const long long base = tile * kTransTile + static_cast<long long>(wave) * kTransWaveChunk;
    const long long b = base > lo ? base : lo;
    const long long e = base + kTransWaveChunk < hi ? base + kTransWaveChunk : hi;
    if (b >= e) continue; // (wave-uniform)
    int col[kTransPerLane];
    double a[kTransPerLane];
    bool in[kTransPerLane];
#pragma unroll
    for (int k = 0; k < kTransPerLane; ++k) {
      const long long q = base + k * kWave + lane;
      in[k] = q >= b && q < e;
      col[k] = in[k] ? load_stream(ci + q) : -1;
      a[k] = in[k] ? load_stream(v + q) : 0.0;
    }
    // the rows of the wavefront's first and last non-zero (every lane the same search), then each non-zero's row between them: a wavefront inside
    // one long row searches nothing, 512 non-zeros of 3 per row take 8 steps in lines the whole wavefront shares
    int r_last;
    const int r_first = wave_end_rows(rp, m, static_cast<int>(b), static_cast<int>(e - 1), &r_last);
    int xrow = -1;
    double xr = 0.0;
#pragma unroll
    for (int k = 0; k < kTransPerLane; ++k) {
      if (!in[k]) continue;
      const int row = last_at_most(rp, r_first, r_last, static_cast<int>(base + k * kWave + lane));
      if (row != xrow) { // x[row] once per piece of a row
        xr = x[row];
        xrow = row;
      }
      if (static_cast<unsigned>(col[k]) < static_cast<unsigned>(n)) unsafeAtomicAdd(y + col[k], alpha * a[k] * xr);
    }
  }
}

} // namespace

void launch_transpose_check(hipStream_t stream, const int *ci, int nnz, int n, unsigned *bad) {
  if (nnz <= 0) return;
  SPMV_ACC_LAUNCH(transpose_check_kernel, dim3(grid_for(nnz, 4 * kThreads)), dim3(kThreads), 0, stream, ci, nnz, n, bad);
}

bool launch_transpose_sort(hipStream_t stream, const int *ci, int nnz, int n, int *keys_out, int *perm, void *tmp, size_t *tmp_bytes) {
  return rocprim::radix_sort_pairs(tmp, *tmp_bytes, ci, keys_out, rocprim::counting_iterator<int>(0), perm, static_cast<size_t>(nnz), 0u,
                                   static_cast<unsigned>(transpose_sort_bits(n)), stream) == hipSuccess;
}

void launch_transpose_rowptr(hipStream_t stream, const int *keys, int nnz, int n, int *t_rowptr) {
  SPMV_ACC_LAUNCH(transpose_rowptr_kernel, dim3(grid_for(static_cast<long long>(n) + 1, kThreads)), dim3(kThreads), 0, stream, keys, nnz, n,
                  t_rowptr);
}

void launch_transpose_rows(hipStream_t stream, const int *rp, int m, int nnz, int *row_of) {
  if (nnz <= 0 || m <= 0) return;
  SPMV_ACC_LAUNCH(transpose_rows_kernel, dim3(grid_for(nnz, kThreads)), dim3(kThreads), 0, stream, rp, m, nnz, row_of);
}

void launch_transpose_gather(hipStream_t stream, int nnz, const int *perm, const int *row_of, const double *value, int *t_colindex,
                             double *t_value) {
  if (nnz <= 0) return;
  SPMV_ACC_LAUNCH(transpose_gather_kernel, dim3(grid_for(nnz, kThreads)), dim3(kThreads), 0, stream, nnz, perm, row_of, value, t_colindex,
                  t_value);
}

void launch_transpose_values(hipStream_t stream, int nnz, const int *perm, const double *value, double *t_value) {
  if (nnz <= 0) return;
  SPMV_ACC_LAUNCH(transpose_values_kernel, dim3(grid_for(nnz, kThreads)), dim3(kThreads), 0, stream, nnz, perm, value, t_value);
}

void launch_spmv_t_scale(hipStream_t stream, int n, double beta, double *y) {
  if (n <= 0) return;
  SPMV_ACC_LAUNCH(spmv_t_scale_kernel, dim3(grid_for(n, kThreads)), dim3(kThreads), 0, stream, n, beta, y);
}

void launch_spmv_t_scatter(hipStream_t stream, int m, int n, int nnz_end, double alpha, const int *rp, const int *ci, const double *v,
                           const double *x, double *y) {
  if (m <= 0 || n <= 0 || nnz_end <= 0) return;
  // (a grid for every tile up to nnz_end: the tiles below the view's first non-zero do not exist for the kernel, their blocks leave at once)
  SPMV_ACC_LAUNCH(spmv_t_scatter_kernel, dim3(grid_for(nnz_end, kTransTile)), dim3(kThreads), 0, stream, m, n, nnz_end, alpha, rp, ci, v, x, y);
}

} // namespace spmv_acc
