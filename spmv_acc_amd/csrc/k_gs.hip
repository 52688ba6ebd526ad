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
// 4. Sweep of one colour (gs_color_kernel, 48; the per-step hot path): a workgroup owns 64 consecutive rows of the colour; each of its wavefronts reads
//    their extents one per lane, chooses the lane group G from their mean length (gs.hpp) and takes every fourth pass of 64 / G rows: per row, G lanes stream colindex
//    and value and gather x -- a step loads up to four terms per lane, all of them before any arithmetic (on a mesh a row is one step: straight-line
//    selects), and adds them in order --; the G partial sums go through the DPP butterfly
//    (neighbouring lanes first: the balanced tree of gs.hpp).  The diagonal is found in passing (a ballot names its lane).  Contraction is off.
//    colindex and value are read with the default cache policy: the backward half of a symmetric sweep starts on the colours the forward half
//    read last (supposed to help while they are still cached; the two policies were not timed against each other).  x is gathered through
//    32-bit byte offsets (device_utils.hpp gather_u32; m <= kGsMaxRows): with 64-bit gather addresses the kernel takes 65 VGPRs, 7 waves per SIMD.
#include "gs.hpp"
#include "structure_passes.hpp"

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

// the term of position p of row i (gs.hpp): +0.0 at the diagonal, which is noted, and for a column outside [0, m)
struct GsTerm {
  int c;
  double v;
};
__device__ __forceinline__ GsTerm gs_load(const int *__restrict__ colindex, const double *__restrict__ value, int p) {
  GsTerm t;
  t.c = colindex[p];
  t.v = value[p];
  return t;
}
// (m <= kGsMaxRows: the byte offset of a column inside [0, m) fits 32 bits)
__device__ __forceinline__ double gs_gather(const double *x, int m, int c) {
  return static_cast<unsigned>(c) < static_cast<unsigned>(m) ? gather_u32(x, c) : 0.0;
}
__device__ __forceinline__ double gs_term(const GsTerm &t, double xc, int m, int i, bool *has, double *diag) {
#pragma clang fp contract(off)
  const bool on_diag = t.c == i;
  *has = *has || on_diag;
  *diag = on_diag ? t.v : *diag;
  const double prod = t.v * xc;
  return on_diag || static_cast<unsigned>(t.c) >= static_cast<unsigned>(m) ? 0.0 : prod;
}

// One workgroup per chunk of kGsTile = kGsChunkRows positions of the colour [first, last), blocks stride over the chunks beyond the grid.  Every
// wavefront of the workgroup reads the chunk's extents and finds the same G; the chunk's G passes of 64 / G rows are dealt out to the four
// wavefronts in turn (G = 1: one pass, three wavefronts leave at once), so a launch holds four times the wavefronts of one chunk per
// wavefront and none walks more than G / 4 passes one after the other.  x is read and written (different elements, by the colouring): not
// __restrict__.
__global__ __launch_bounds__(kThreads) void gs_color_kernel(int m, int nnz, const int *__restrict__ rowptr, const int *__restrict__ colindex,
                                                            const double *__restrict__ value, int first, int last,
                                                            const int *__restrict__ color_rows, double omega, const double *__restrict__ b,
                                                            double *x) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const long long ntiles = (static_cast<long long>(last) - first + kGsTile - 1) / kGsTile;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) { // (block-uniform)
    const long long base = first + tile * kGsTile; // (< last; the workgroup's four wavefronts share the chunk and deal its passes out)
    const int rows_here = last - base < kGsChunkRows ? static_cast<int>(last - base) : kGsChunkRows;
    // lane r holds the row of position base + r: its index (-1: none, or outside [0, m)) and its clamped extent
    int my_i = -1, my_lo = 0, my_hi = 0;
    if (lane < rows_here) {
      const int i = color_rows != nullptr ? load_stream(color_rows + base + lane) : static_cast<int>(base + lane);
      if (static_cast<unsigned>(i) < static_cast<unsigned>(m)) {
        my_i = i;
        my_lo = row_extent(rowptr, nnz, i, &my_hi);
      }
    }
    u64 total = static_cast<u64>(my_hi - my_lo);
    for (int off = kWave / 2; off > 0; off >>= 1) total += __shfl_xor(total, off, kWave);
    const u64 terms = static_cast<u64>(__builtin_amdgcn_readfirstlane(static_cast<int>(total >> 32))) << 32 |
                      static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(total)));
    int g = 1, log_g = 0; // the lane group (gs.hpp): the smallest G with G * kGsTermsPerLane * rows_here >= terms, at most 64
    while (g < kWave && static_cast<u64>(g) * kGsTermsPerLane * rows_here < terms) {
      g <<= 1;
      ++log_g;
    }
    const int per_pass = kWave >> log_g; // rows per pass
    const int slot = lane >> log_g;      // this lane's row of the pass
    const int l = lane & (g - 1);        // ... and its place in the row's lane group
    for (int done = wave * per_pass; done < rows_here; done += (kThreads / kWave) * per_pass) { // (wave-uniform)
      const int k = done + slot; // (< 64: per_pass divides 64)
      const int i = __shfl(my_i, k, kWave);
      const int lo = __shfl(my_lo, k, kWave), hi = __shfl(my_hi, k, kWave);
      bool has = false;
      double diag = 0.0, part = 0.0;
      bool opened = false; // the sum starts from the lane's first term, not from 0.0
      for (int p = lo + l; p < hi; p += 4 * g) { // up to four terms a step (on a mesh: one step), every load issued before the arithmetic
        const int p1 = p + g, p2 = p + 2 * g, p3 = p + 3 * g;
        const bool live1 = p1 < hi, live2 = p2 < hi, live3 = p3 < hi; // (a position beyond the row reads p again and is not added)
        const GsTerm t0 = gs_load(colindex, value, p), t1 = gs_load(colindex, value, live1 ? p1 : p);
        const GsTerm t2 = gs_load(colindex, value, live2 ? p2 : p), t3 = gs_load(colindex, value, live3 ? p3 : p);
        const double x0 = gs_gather(x, m, t0.c), x1 = gs_gather(x, m, t1.c), x2 = gs_gather(x, m, t2.c), x3 = gs_gather(x, m, t3.c);
        const double w0 = gs_term(t0, x0, m, i, &has, &diag), w1 = gs_term(t1, x1, m, i, &has, &diag);
        const double w2 = gs_term(t2, x2, m, i, &has, &diag), w3 = gs_term(t3, x3, m, i, &has, &diag);
        part = opened ? part + w0 : w0;
        opened = true;
        part = live1 ? part + w1 : part;
        part = live2 ? part + w2 : part;
        part = live3 ? part + w3 : part;
      }
      const double s = group_sum_dyn(part, g);
      // the diagonal: the first lane of the group that met it
      u64 holders = __ballot(has) >> (slot << log_g);
      if (g < kWave) holders &= (1ull << g) - 1;
      const int owner = holders != 0 ? (slot << log_g) + (__ffsll(static_cast<long long>(holders)) - 1) : lane;
      const double a_ii = __shfl(diag, owner, kWave);
      if (l == 0 && i >= 0 && holders != 0) { // a row without a stored diagonal is left untouched
        const double gs = (b[i] - s) / a_ii;
        if (omega == 1.0) {
          x[i] = gs;
        } else {
          const double xi = x[i];
          x[i] = xi + omega * (gs - xi);
        }
      }
    }
  }
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
