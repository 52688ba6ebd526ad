// k_gs.hip -- the kernels of the multicolour Gauss-Seidel / SOR smoother (the colouring's definition, the sweep's summation order, size rules
// and launcher declarations in gs.hpp, engine in gs.cpp).
//
// No reference counterpart: hpcde/spmv-acc multiplies a matrix by a vector.
//
// No atomics and no waiting anywhere: every output is written by exactly one lane, every dependency is a kernel boundary.  VGPRs as compiled
// for gfx950 (wave64; no scratch, no AGPR, 8 waves per SIMD in all):
// 1. Census (gs_census_kernel, 26 VGPRs): one row per lane.  The ends of rowptr, the row's extent, its columns' range and strict ascent, the
//    mirror (j, i) of every off-diagonal (i, j) by a binary search in row j, the rows without a diagonal; per-wavefront counts in slots of
//    their own, added on the host.  Nothing else runs unless the five error counts are zero.
// 2. Round (gs_round_kernel, 20): one row per lane; an uncoloured row reads its neighbours' colours of the round before, waits behind an
//    uncoloured neighbour of higher priority, else takes the lowest clear bit of the 64-colour window's mask.  Every row writes its colour (or
//    -1) to the other buffer; the rows still uncoloured are counted per wavefront.
// 3. Keys (gs_keys_kernel, 8) and colour pointer (gs_color_ptr_kernel, 9): the colour as the sort key of the library's stable radix sort, whose
//    order IS color_rows; color_ptr[c] by a binary search in the sorted keys.
// 4. Sweep of one colour (gs_color_kernel, 47; the per-step hot path): the policy ColorRows on row_sweep.hpp's lane_group_rows, the one row-sum
//    body that the Jacobi kernels run too (chunks of 64 positions of the colour, the lane group G, the passes, the four terms a step, the
//    butterfly and the diagonal's ballot are described there).  What is this kernel's own: the row of a position comes through color_rows, the
//    diagonal's term is +0.0, lane 0 of the group divides by the diagonal and relaxes.  Contraction is off.
//    colindex and value are read with the default cache policy: the backward half of a symmetric sweep starts on the colours the forward half
//    read last (supposed to help while they are still cached; the two policies were not timed against each other).  x is gathered through
//    32-bit byte offsets (device_utils.hpp gather_u32; m <= kGsMaxRows): with 64-bit gather addresses the kernel takes 65 VGPRs, 7 waves per SIMD.
#include "row_sweep.hpp"

namespace spmv_acc {
namespace {

using namespace dev;
using namespace passes;
using u64 = unsigned long long;

// gridDim.x <= kCooCheckBlocks; slots: gs.hpp launch_gs_census.  m > 0.
__global__ __launch_bounds__(kThreads) void gs_census_kernel(int m, int nnz, const int *__restrict__ rowptr, const int *__restrict__ colindex,
                                                             unsigned *__restrict__ slots) {
  unsigned bad_ends = 0, bad_extents = 0, cols_out = 0, not_ascending = 0, no_mirror = 0, no_diag = 0;
  const long long stride = static_cast<long long>(gridDim.x) * kThreads;
  for (long long r = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; r <= m; r += stride) {
    if (r == 0) bad_ends += rowptr[0] != 0 ? 1u : 0u;
    if (r == m) {
      bad_ends += rowptr[m] != nnz ? 1u : 0u;
      continue;
    }
    const int i = static_cast<int>(r);
    const int raw_lo = rowptr[i], raw_hi = rowptr[i + 1];
    bad_extents += raw_lo < 0 || raw_hi > nnz || raw_hi < raw_lo ? 1u : 0u;
    int hi;
    const int lo = row_extent(rowptr, nnz, i, &hi);
    bool diag = false;
    int before = -1;
    for (int p = lo; p < hi; ++p) {
      const int c = load_stream(colindex + p);
      not_ascending += p > lo && c <= before ? 1u : 0u;
      before = c;
      if (static_cast<unsigned>(c) >= static_cast<unsigned>(m)) {
        cols_out += 1u;
        continue;
      }
      if (c == i) {
        diag = true;
        continue;
      }
      int chi;
      const int clo = row_extent(rowptr, nnz, c, &chi);
      const int q = first_at_least(colindex, clo, chi, i);
      no_mirror += q >= chi || colindex[q] != i ? 1u : 0u;
    }
    no_diag += diag ? 0u : 1u;
  }
  count_to_slot(bad_ends, slots);
  count_to_slot(bad_extents, slots + kCooCheckSlots);
  count_to_slot(cols_out, slots + 2 * kCooCheckSlots);
  count_to_slot(not_ascending, slots + 3 * kCooCheckSlots);
  count_to_slot(no_mirror, slots + 4 * kCooCheckSlots);
  count_to_slot(no_diag, slots + 5 * kCooCheckSlots);
}

// gridDim.x <= kCooCheckBlocks.  m > 0; the census has passed.  color_in and color_out are different arrays.
__global__ __launch_bounds__(kThreads) void gs_round_kernel(int m, int nnz, const int *__restrict__ rowptr, const int *__restrict__ colindex,
                                                            const int *__restrict__ color_in, int *__restrict__ color_out,
                                                            unsigned *__restrict__ slots) {
  unsigned uncoloured = 0;
  const long long stride = static_cast<long long>(gridDim.x) * kThreads;
  for (long long r = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; r < m; r += stride) {
    const int v = static_cast<int>(r);
    int color = color_in[v];
    if (color < 0) {
      int hi;
      const int lo = row_extent(rowptr, nnz, v, &hi);
      const u64 mine = gs_priority(static_cast<unsigned>(v));
      bool wait = false;
      u64 used = 0; // the colours of the window [base, base + kGsColorWindow) that a neighbour holds
      for (int p = lo; p < hi && !wait; ++p) {
        const int u = colindex[p];
        if (u == v || static_cast<unsigned>(u) >= static_cast<unsigned>(m)) continue;
        const int cu = color_in[u];
        if (cu < 0) wait = gs_priority(static_cast<unsigned>(u)) > mine;
        else if (cu < kGsColorWindow) used |= 1ull << cu;
      }
      if (!wait) {
        int base = 0;
        while (used == ~0ull) { // the window is full: the next one (a row of degree d ends within d / 64 + 1 windows)
          base += kGsColorWindow;
          used = 0;
          for (int p = lo; p < hi; ++p) {
            const int u = colindex[p];
            if (u == v || static_cast<unsigned>(u) >= static_cast<unsigned>(m)) continue;
            const unsigned off = static_cast<unsigned>(color_in[u] - base); // (an uncoloured neighbour, -1 - base, lands far outside)
            if (off < static_cast<unsigned>(kGsColorWindow)) used |= 1ull << off;
          }
        }
        color = base + (__ffsll(static_cast<long long>(~used)) - 1);
      }
    }
    color_out[v] = color;
    uncoloured += color < 0 ? 1u : 0u;
  }
  count_to_slot(uncoloured, slots);
}

__global__ __launch_bounds__(kThreads) void gs_keys_kernel(int m, const int *__restrict__ color, u64 *__restrict__ keys) {
  const long long stride = static_cast<long long>(gridDim.x) * kThreads;
  for (long long v = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; v < m; v += stride)
    keys[v] = static_cast<u64>(static_cast<unsigned>(color[v]));
}

__global__ __launch_bounds__(kThreads) void gs_color_ptr_kernel(int m, const u64 *__restrict__ sorted, int count, int *__restrict__ ptr) {
  const long long stride = static_cast<long long>(gridDim.x) * kThreads;
  for (long long c = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; c < count; c += stride)
    ptr[c] = first_at_least(sorted, 0, m, static_cast<u64>(c));
}

// What a row's lane group does in a colour's sweep (row_sweep.hpp names the members): the row comes through color_rows, the diagonal's term is
// +0.0, and a row without a stored diagonal is left untouched.  x is read and written (different elements, by the colouring): not __restrict__.
struct ColorRows {
  const int *__restrict__ color_rows;
  double omega;
  const double *__restrict__ b;
  double *x;
  __device__ __forceinline__ const double *gathered() const { return x; }
  __device__ __forceinline__ int row_at(long long pos) const {
    return color_rows != nullptr ? load_stream(color_rows + pos) : static_cast<int>(pos);
  }
  __device__ __forceinline__ double begin(int) const { return 0.0; }
  __device__ __forceinline__ double term(double v, double xc, double, bool on_diag) const {
#pragma clang fp contract(off)
    const double prod = v * xc;
    return on_diag ? 0.0 : prod;
  }
  __device__ __forceinline__ void finish(int i, double s, bool has_diag, double a_ii) const {
#pragma clang fp contract(off)
    if (!has_diag) return;
    const double gs = (b[i] - s) / a_ii;
    if (omega == 1.0) {
      x[i] = gs;
    } else {
      const double xi = x[i];
      x[i] = xi + omega * (gs - xi);
    }
  }
};

__global__ __launch_bounds__(kThreads) void gs_color_kernel(int m, int nnz, const int *__restrict__ rowptr, const int *__restrict__ colindex,
                                                            const double *__restrict__ value, int first, int last,
                                                            const int *__restrict__ color_rows, double omega, const double *__restrict__ b,
                                                            double *x) {
  const ColorRows rows{color_rows, omega, b, x};
  lane_group_rows(m, nnz, rowptr, colindex, value, first, last, rows);
}

} // namespace

void launch_gs_census(hipStream_t stream, int m, int nnz, const int *rowptr, const int *colindex, unsigned *slots) {
  if (m <= 0) return;
  SPMV_ACC_LAUNCH(gs_census_kernel, dim3(census_grid_for(static_cast<long long>(m) + 1, kThreads)), dim3(kThreads), 0, stream, m, nnz, rowptr,
                  colindex, slots);
}

void launch_gs_round(hipStream_t stream, int m, int nnz, const int *rowptr, const int *colindex, const int *color_in, int *color_out,
                     unsigned *slots) {
  if (m <= 0) return;
  SPMV_ACC_LAUNCH(gs_round_kernel, dim3(census_grid_for(m, kThreads)), dim3(kThreads), 0, stream, m, nnz, rowptr, colindex, color_in, color_out,
                  slots);
}

void launch_gs_keys(hipStream_t stream, int m, const int *color, unsigned long long *keys) {
  if (m <= 0) return;
  SPMV_ACC_LAUNCH(gs_keys_kernel, dim3(grid_for(m, kThreads)), dim3(kThreads), 0, stream, m, color, keys);
}

void launch_gs_color_ptr(hipStream_t stream, int m, const unsigned long long *sorted, int count, int *ptr) {
  if (m <= 0 || count <= 0) return;
  SPMV_ACC_LAUNCH(gs_color_ptr_kernel, dim3(grid_for(count, kThreads)), dim3(kThreads), 0, stream, m, sorted, count, ptr);
}

void launch_gs_color(hipStream_t stream, int m, int nnz, const int *rowptr, const int *colindex, const double *value, int first, int last,
                     const int *color_rows, double omega, const double *b, double *x) {
  if (m <= 0 || m > kGsMaxRows || nnz <= 0 || first >= last) return;
  SPMV_ACC_LAUNCH(gs_color_kernel, dim3(grid_for(static_cast<long long>(last) - first, kGsTile)), dim3(kThreads), 0, stream, m, nnz, rowptr,
                  colindex, value, first, last, color_rows, omega, b, x);
}

} // namespace spmv_acc
