// k_jacobi.hip -- the kernels of the damped Jacobi / l1-Jacobi smoother (the diagonals' definition, the sweep's summation order, size rules and
// launcher declarations in jacobi.hpp, engine in jacobi.cpp).
//
// No reference counterpart: hpcde/spmv-acc multiplies a matrix by a vector.
//
// No atomics and no waiting anywhere: every output is written by exactly one lane, and a sweep is one launch that reads x_in and writes other
// arrays.  VGPRs as compiled for gfx950 (wave64; no scratch, no AGPR, 8 waves per SIMD in all):
// 1. Inverse diagonal (jacobi_inverse_kernel, 12 VGPRs): one row per lane, the diagonal by a binary search of the clamped row (as
//    k_strength.hip's roots), dinv[i] = 1 / a_ii.
// 2. Scaled l1 diagonal (jacobi_l1_kernel, 52) and 3. sweep (jacobi_sweep_kernel, 39; the per-step hot path): the policies L1Rows and SweepRows
//    on row_sweep.hpp's lane_group_rows, the one row-sum body that gs_color_kernel runs too (chunks of 64 rows, the lane group G, the passes,
//    the four terms a step, the butterfly and the diagonal's ballot are described there), over the positions [0, m), which are the rows.  The
//    vector -- x_in, or the roots g -- is gathered through 32-bit byte offsets (device_utils.hpp gather_u32; m <= kJacobiMaxRows).
//    Contraction is off: the sweep holds no fused operation at all, the diagonals none outside their divisions' own expansion.
// 4. Zero start (jacobi_start_kernel, 10): one row per lane, x_out = (omega * dinv) * b, r_out = b; the matrix is not read.
#include "jacobi.hpp"
#include "row_sweep.hpp"

namespace spmv_acc {
namespace {

using namespace dev;
using namespace passes;

__global__ __launch_bounds__(kThreads) void jacobi_inverse_kernel(int m, int nnz, const int *__restrict__ rowptr, const int *__restrict__ colindex,
                                                                  const double *__restrict__ value, double *__restrict__ dinv) {
  const long long stride = static_cast<long long>(gridDim.x) * kThreads;
  for (long long r = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; r < m; r += stride) {
    const int i = static_cast<int>(r);
    int hi;
    const int lo = row_extent(rowptr, nnz, i, &hi);
    const int p = first_at_least(colindex, lo, hi, i);
    double inv = 0.0; // (a row without a stored diagonal)
    if (p < hi && colindex[p] == i) inv = 1.0 / value[p];
    dinv[i] = inv;
  }
}

__global__ __launch_bounds__(kThreads) void jacobi_start_kernel(int m, const double *__restrict__ dinv, double omega, const double *__restrict__ b,
                                                                double *__restrict__ x_out, double *__restrict__ r_out) {
#pragma clang fp contract(off)
  const long long stride = static_cast<long long>(gridDim.x) * kThreads;
  for (long long r = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; r < m; r += stride) {
    const double t = b[r];
    const double w = omega * dinv[r];
    if (r_out != nullptr) r_out[r] = t;
    if (x_out != nullptr) x_out[r] = w * t;
  }
}

// What a row's lane group does with its terms (row_sweep.hpp names the members): the rows are the positions themselves.
struct SweepRows {
  const double *__restrict__ x_in;
  const double *__restrict__ dinv;
  const double *__restrict__ b;
  double omega;
  double *__restrict__ x_out;
  double *__restrict__ r_out;
  __device__ __forceinline__ const double *gathered() const { return x_in; }
  __device__ __forceinline__ int row_at(long long pos) const { return static_cast<int>(pos); }
  __device__ __forceinline__ double begin(int) const { return 0.0; }
  __device__ __forceinline__ double term(double v, double xc, double, bool) const {
#pragma clang fp contract(off)
    return v * xc;
  }
  __device__ __forceinline__ void finish(int i, double s, bool, double) const {
#pragma clang fp contract(off)
    const double t = b[i] - s;
    const double w = omega * dinv[i];
    if (r_out != nullptr) r_out[i] = t;
    if (x_out != nullptr) {
      const double step = w * t;
      x_out[i] = x_in[i] + step;
    }
  }
};

struct L1Rows {
  const double *__restrict__ g;
  double *__restrict__ dinv;
  __device__ __forceinline__ const double *gathered() const { return g; }
  __device__ __forceinline__ int row_at(long long pos) const { return static_cast<int>(pos); }
  __device__ __forceinline__ double begin(int i) const { return i >= 0 ? g[i] : 0.0; }
  __device__ __forceinline__ double term(double v, double gj, double gi, bool) const {
#pragma clang fp contract(off)
    const double ratio = gi / gj; // (rounded first, then the product)
    return fabs(v) * ratio;
  }
  __device__ __forceinline__ void finish(int i, double s, bool has_diag, double) const { dinv[i] = has_diag ? 1.0 / s : 0.0; }
};

// x_in is read by every row and x_out / r_out are other arrays (jacobi.cpp refuses an overlap): all __restrict__
__global__ __launch_bounds__(kThreads) void jacobi_sweep_kernel(int m, int nnz, const int *__restrict__ rowptr, const int *__restrict__ colindex,
                                                                const double *__restrict__ value, const double *__restrict__ dinv, double omega,
                                                                const double *__restrict__ b, const double *__restrict__ x_in,
                                                                double *__restrict__ x_out, double *__restrict__ r_out) {
  const SweepRows rows{x_in, dinv, b, omega, x_out, r_out};
  lane_group_rows(m, nnz, rowptr, colindex, value, 0, m, rows);
}

__global__ __launch_bounds__(kThreads) void jacobi_l1_kernel(int m, int nnz, const int *__restrict__ rowptr, const int *__restrict__ colindex,
                                                             const double *__restrict__ value, const double *__restrict__ g,
                                                             double *__restrict__ dinv) {
  const L1Rows rows{g, dinv};
  lane_group_rows(m, nnz, rowptr, colindex, value, 0, m, rows);
}

} // namespace

void launch_jacobi_inverse(hipStream_t stream, int m, int nnz, const int *rowptr, const int *colindex, const double *value, double *dinv) {
  if (m <= 0) return;
  SPMV_ACC_LAUNCH(jacobi_inverse_kernel, dim3(grid_for(m, kThreads)), dim3(kThreads), 0, stream, m, nnz, rowptr, colindex, value, dinv);
}

void launch_jacobi_l1(hipStream_t stream, int m, int nnz, const int *rowptr, const int *colindex, const double *value, const double *g,
                      double *dinv) {
  if (m <= 0 || m > kJacobiMaxRows) return;
  SPMV_ACC_LAUNCH(jacobi_l1_kernel, dim3(grid_for(m, kJacobiTile)), dim3(kThreads), 0, stream, m, nnz, rowptr, colindex, value, g, dinv);
}

void launch_jacobi_sweep(hipStream_t stream, int m, int nnz, const int *rowptr, const int *colindex, const double *value, const double *dinv,
                         double omega, const double *b, const double *x_in, double *x_out, double *r_out) {
  if (m <= 0 || m > kJacobiMaxRows) return;
  SPMV_ACC_LAUNCH(jacobi_sweep_kernel, dim3(grid_for(m, kJacobiTile)), dim3(kThreads), 0, stream, m, nnz, rowptr, colindex, value, dinv, omega, b,
                  x_in, x_out, r_out);
}

void launch_jacobi_start(hipStream_t stream, int m, const double *dinv, double omega, const double *b, double *x_out, double *r_out) {
  if (m <= 0) return;
  SPMV_ACC_LAUNCH(jacobi_start_kernel, dim3(grid_for(m, kThreads)), dim3(kThreads), 0, stream, m, dinv, omega, b, x_out, r_out);
}

} // namespace spmv_acc
