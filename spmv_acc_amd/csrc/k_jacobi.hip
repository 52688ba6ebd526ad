// k_jacobi.hip -- the kernels of the damped Jacobi / l1-Jacobi smoother (the diagonals' definition, the sweep's summation order, size rules and
// launcher declarations in jacobi.hpp, engine in jacobi.cpp).
//
// No reference counterpart: hpcde/spmv-acc multiplies a matrix by a vector.
//
// No atomics and no waiting anywhere: every output is written by exactly one lane, and a sweep is one launch that reads x_in and writes other
// arrays.  VGPRs as compiled for gfx950 (wave64; no scratch, no AGPR, 8 waves per SIMD in all):
// 1. Inverse diagonal (jacobi_inverse_kernel, 12 VGPRs): one row per lane, the diagonal by a binary search of the clamped row (as
//    k_strength.hip's roots), dinv[i] = 1 / a_ii.
// 2. Scaled l1 diagonal (jacobi_l1_kernel, 50) and 3. sweep (jacobi_sweep_kernel, 38; the per-step hot path): one body, jacobi_rows.  A workgroup
//    owns 64 consecutive rows; each of its wavefronts reads their extents one per lane, chooses the lane group G from their mean length
//    (jacobi.hpp) and takes every fourth pass of 64 / G rows: per row, G lanes stream colindex and value and gather the vector -- x_in, or the
//    roots g -- a step loads up to four terms per lane, all of them before any arithmetic (on a mesh a row is one step), and adds them in
//    order; the G partial sums go through the DPP butterfly (neighbouring lanes first: the balanced tree).  This restates gs_color_kernel's
//    row sum without the colour's row indirection and without the diagonal's exclusion; the two are not shared yet.  The vector is gathered
//    through 32-bit byte offsets (device_utils.hpp gather_u32; m <= kJacobiMaxRows).  Contraction is off: the sweep holds no fused operation
//    at all, the diagonals none outside their divisions' own expansion.
// 4. Zero start (jacobi_start_kernel, 10): one row per lane, x_out = (omega * dinv) * b, r_out = b; the matrix is not read.
#include "jacobi.hpp"
#include "structure_passes.hpp"

namespace spmv_acc {
namespace {

using namespace dev;
using namespace passes;
using u64 = unsigned long long;

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

// What a row's lane group does with its terms.  gathered(): the vector the columns index;  begin(i): a per-row value every lane of the group
// holds (i < 0: a lane without a row);  term(): the term of one stored entry with a column inside [0, m);  finish(): lane 0 of the group, the
// row's sum in hand.
struct SweepRows {
  const double *__restrict__ x_in;
  const double *__restrict__ dinv;
  const double *__restrict__ b;
  double omega;
  double *__restrict__ x_out;
  double *__restrict__ r_out;
  __device__ __forceinline__ const double *gathered() const { return x_in; }
  __device__ __forceinline__ double begin(int) const { return 0.0; }
  __device__ __forceinline__ double term(double v, double xc, double) const {
#pragma clang fp contract(off)
    return v * xc;
  }
  __device__ __forceinline__ void finish(int i, double s, bool) const {
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
  __device__ __forceinline__ double begin(int i) const { return i >= 0 ? g[i] : 0.0; }
  __device__ __forceinline__ double term(double v, double gj, double gi) const {
#pragma clang fp contract(off)
    const double ratio = gi / gj; // (rounded first, then the product)
    return fabs(v) * ratio;
  }
  __device__ __forceinline__ void finish(int i, double s, bool has_diag) const { dinv[i] = has_diag ? 1.0 / s : 0.0; }
};

struct JacobiTerm {
  int c;
  double v;
};
__device__ __forceinline__ JacobiTerm jacobi_load(const int *__restrict__ colindex, const double *__restrict__ value, int p) {
  JacobiTerm t;
  t.c = colindex[p];
  t.v = value[p];
  return t;
}
// (m <= kJacobiMaxRows: the byte offset of a column inside [0, m) fits 32 bits; a column outside is never an address)
__device__ __forceinline__ double jacobi_gather(const double *vec, int m, int c) {
  return static_cast<unsigned>(c) < static_cast<unsigned>(m) ? gather_u32(vec, c) : 0.0;
}
template <typename Rows>
__device__ __forceinline__ double jacobi_term(const Rows &rows, const JacobiTerm &t, double vc, double mine, int m, int i, bool *has) {
  *has = *has || t.c == i;
  const double w = rows.term(t.v, vc, mine);
  return static_cast<unsigned>(t.c) >= static_cast<unsigned>(m) ? 0.0 : w;
}

// One workgroup per chunk of kJacobiTile consecutive rows, blocks stride over the chunks beyond the grid.  Every wavefront of the workgroup
// reads the chunk's extents and finds the same G; the chunk's G passes of 64 / G rows are dealt out to the four wavefronts in turn.
template <typename Rows>
__device__ __forceinline__ void jacobi_rows(int m, int nnz, const int *__restrict__ rowptr, const int *__restrict__ colindex,
                                            const double *__restrict__ value, const Rows &rows) {
#pragma clang fp contract(off)
  const double *vec = rows.gathered();
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const long long ntiles = (static_cast<long long>(m) + kJacobiTile - 1) / kJacobiTile;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) { // (block-uniform)
    const long long base = tile * kJacobiTile; // (< m; the workgroup's four wavefronts share the chunk and deal its passes out)
    const int rows_here = m - base < kJacobiTile ? static_cast<int>(m - base) : kJacobiTile;
    // lane r holds the clamped extent of row base + r
    int my_lo = 0, my_hi = 0;
    if (lane < rows_here) my_lo = row_extent(rowptr, nnz, static_cast<int>(base) + lane, &my_hi);
    u64 total = static_cast<u64>(my_hi - my_lo);
    for (int off = kWave / 2; off > 0; off >>= 1) total += __shfl_xor(total, off, kWave);
    const u64 terms = static_cast<u64>(__builtin_amdgcn_readfirstlane(static_cast<int>(total >> 32))) << 32 |
                      static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(total)));
    int g = 1, log_g = 0; // the lane group (jacobi.hpp): the smallest G with G * kGsTermsPerLane * rows_here >= terms, at most 64
    while (g < kWave && static_cast<u64>(g) * kGsTermsPerLane * rows_here < terms) {
      g <<= 1;
      ++log_g;
    }
    const int per_pass = kWave >> log_g; // rows per pass
    const int slot = lane >> log_g;      // this lane's row of the pass
    const int l = lane & (g - 1);        // ... and its place in the row's lane group
    for (int done = wave * per_pass; done < rows_here; done += (kThreads / kWave) * per_pass) { // (wave-uniform)
      const int k = done + slot; // (< 64: per_pass divides 64)
      const int i = k < rows_here ? static_cast<int>(base) + k : -1;
      const int lo = __shfl(my_lo, k, kWave), hi = __shfl(my_hi, k, kWave); // (an empty extent beyond the chunk's rows)
      const double mine = rows.begin(i);
      bool has = false;
      double part = 0.0;
      bool opened = false; // the sum starts from the lane's first term, not from 0.0
      for (int p = lo + l; p < hi; p += 4 * g) { // up to four terms a step (on a mesh: one step), every load issued before the arithmetic
        const int p1 = p + g, p2 = p + 2 * g, p3 = p + 3 * g;
        const bool live1 = p1 < hi, live2 = p2 < hi, live3 = p3 < hi; // (a position beyond the row reads p again and is not added)
        const JacobiTerm t0 = jacobi_load(colindex, value, p), t1 = jacobi_load(colindex, value, live1 ? p1 : p);
        const JacobiTerm t2 = jacobi_load(colindex, value, live2 ? p2 : p), t3 = jacobi_load(colindex, value, live3 ? p3 : p);
        const double v0 = jacobi_gather(vec, m, t0.c), v1 = jacobi_gather(vec, m, t1.c);
        const double v2 = jacobi_gather(vec, m, t2.c), v3 = jacobi_gather(vec, m, t3.c);
        const double w0 = jacobi_term(rows, t0, v0, mine, m, i, &has), w1 = jacobi_term(rows, t1, v1, mine, m, i, &has);
        const double w2 = jacobi_term(rows, t2, v2, mine, m, i, &has), w3 = jacobi_term(rows, t3, v3, mine, m, i, &has);
        part = opened ? part + w0 : w0;
        opened = true;
        part = live1 ? part + w1 : part;
        part = live2 ? part + w2 : part;
        part = live3 ? part + w3 : part;
      }
      const double s = group_sum_dyn(part, g);
      u64 holders = __ballot(has) >> (slot << log_g); // the lanes of this row's group that met the diagonal
      if (g < kWave) holders &= (1ull << g) - 1;
      if (l == 0 && i >= 0) rows.finish(i, s, holders != 0);
    }
  }
}

// x_in is read by every row and x_out / r_out are other arrays (jacobi.cpp refuses an overlap): all __restrict__
__global__ __launch_bounds__(kThreads) void jacobi_sweep_kernel(int m, int nnz, const int *__restrict__ rowptr, const int *__restrict__ colindex,
                                                                const double *__restrict__ value, const double *__restrict__ dinv, double omega,
                                                                const double *__restrict__ b, const double *__restrict__ x_in,
                                                                double *__restrict__ x_out, double *__restrict__ r_out) {
  const SweepRows rows{x_in, dinv, b, omega, x_out, r_out};
  jacobi_rows(m, nnz, rowptr, colindex, value, rows);
}

__global__ __launch_bounds__(kThreads) void jacobi_l1_kernel(int m, int nnz, const int *__restrict__ rowptr, const int *__restrict__ colindex,
                                                             const double *__restrict__ value, const double *__restrict__ g,
                                                             double *__restrict__ dinv) {
  const L1Rows rows{g, dinv};
  jacobi_rows(m, nnz, rowptr, colindex, value, rows);
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
