// row_sweep.hpp -- the one row-sum body of the smoothers' hot kernels (k_gs.hip gs_color_kernel; k_jacobi.hip jacobi_sweep_kernel and
// jacobi_l1_kernel): THE SUMMATION ORDER of gs.hpp as device code, defined once.  A change to that order -- a fifth term in flight, another
// rule for G -- is made here and nowhere else.  Plain inline helpers, no constants of its own: kGsChunkRows, kGsTile, kGsTermsPerLane and
// kGsMaxRows stay in gs.hpp.
//
// No reference counterpart: hpcde/spmv-acc multiplies a matrix by a vector.
#pragma once

#include "gs.hpp"
#include "structure_passes.hpp"

namespace spmv_acc {
namespace passes {

// one stored entry of a row
struct RowTerm {
  int c;
  double v;
};
__device__ __forceinline__ RowTerm row_term_load(const int *__restrict__ colindex, const double *__restrict__ value, int p) {
  RowTerm t;
  t.c = colindex[p];
  t.v = value[p];
  return t;
}
// (m <= kGsMaxRows: the byte offset of a column inside [0, m) fits 32 bits; a column outside is never an address)
__device__ __forceinline__ double row_gather(const double *vec, int m, int c) {
  return static_cast<unsigned>(c) < static_cast<unsigned>(m) ? dev::gather_u32(vec, c) : 0.0;
}
// the term of one stored entry of row i: the diagonal is noted and its value remembered, a column outside [0, m) gives +0.0
template <typename Rows>
__device__ __forceinline__ double row_term(const Rows &rows, const RowTerm &t, double vc, double mine, int m, int i, bool *has, double *diag) {
  const bool on_diag = t.c == i;
  *has = *has || on_diag;
  *diag = on_diag ? t.v : *diag;
  const double w = rows.term(t.v, vc, mine, on_diag);
  return static_cast<unsigned>(t.c) >= static_cast<unsigned>(m) ? 0.0 : w;
}

// The rows of the positions [first, last), kThreads lanes per workgroup.  One workgroup per chunk of kGsTile = kGsChunkRows positions, blocks
// stride over the chunks beyond the grid.  Every wavefront of the workgroup reads the chunk's extents one per lane and finds the same G (gs.hpp);
// the chunk's G passes of 64 / G rows are dealt out to the four wavefronts in turn (G = 1: one pass, three wavefronts leave at once), so a
// launch holds four times the wavefronts of one chunk per wavefront and none walks more than G / 4 passes one after the other.  Per row, G
// lanes stream colindex and value and gather the vector through 32-bit byte offsets -- a step loads up to four terms per lane, all of them
// before any arithmetic (on a mesh a row is one step: straight-line selects), and adds them in order --; the G partial sums go through the
// DPP butterfly (neighbouring lanes first: the balanced tree of gs.hpp).  The diagonal is found in passing (a ballot names its lane).
// What differs between the kernels is the policy `rows`:
//   gathered()                      the vector the columns index
//   row_at(pos)                     the row of a position (outside [0, m): the position is skipped)
//   begin(i)                        a per-row value that every lane of the row's group holds (i < 0: a lane without a row), handed to term()
//   term(v, vc, mine, on_diag)      the term of one stored entry whose column is inside [0, m), vc the gathered element
//   finish(i, s, has_diag, a_ii)    lane 0 of the group, i >= 0: the row's sum in hand, whether the row stores a diagonal and its value
template <typename Rows>
__device__ __forceinline__ void lane_group_rows(int m, int nnz, const int *__restrict__ rowptr, const int *__restrict__ colindex,
                                                const double *__restrict__ value, int first, int last, const Rows &rows) {
#pragma clang fp contract(off)
  using u64 = unsigned long long;
  const double *vec = rows.gathered();
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const long long ntiles = (static_cast<long long>(last) - first + kGsTile - 1) / kGsTile;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) { // (block-uniform)
    const long long base = first + tile * kGsTile; // (< last; the workgroup's four wavefronts share the chunk and deal its passes out)
    const int rows_here = last - base < kGsChunkRows ? static_cast<int>(last - base) : kGsChunkRows;
    // lane r holds the row of position base + r: its index (-1: none, or outside [0, m)) and its clamped extent
    int my_i = -1, my_lo = 0, my_hi = 0;
    if (lane < rows_here) {
      const int i = rows.row_at(base + lane);
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
      const int lo = __shfl(my_lo, k, kWave), hi = __shfl(my_hi, k, kWave); // (an empty extent beyond the chunk's rows)
      const double mine = rows.begin(i);
      bool has = false;
      double diag = 0.0, part = 0.0;
      bool opened = false; // the sum starts from the lane's first term, not from 0.0
      for (int p = lo + l; p < hi; p += 4 * g) { // up to four terms a step (on a mesh: one step), every load issued before the arithmetic
        const int p1 = p + g, p2 = p + 2 * g, p3 = p + 3 * g;
        const bool live1 = p1 < hi, live2 = p2 < hi, live3 = p3 < hi; // (a position beyond the row reads p again and is not added)
        const RowTerm t0 = row_term_load(colindex, value, p), t1 = row_term_load(colindex, value, live1 ? p1 : p);
        const RowTerm t2 = row_term_load(colindex, value, live2 ? p2 : p), t3 = row_term_load(colindex, value, live3 ? p3 : p);
        const double v0 = row_gather(vec, m, t0.c), v1 = row_gather(vec, m, t1.c), v2 = row_gather(vec, m, t2.c), v3 = row_gather(vec, m, t3.c);
        const double w0 = row_term(rows, t0, v0, mine, m, i, &has, &diag), w1 = row_term(rows, t1, v1, mine, m, i, &has, &diag);
        const double w2 = row_term(rows, t2, v2, mine, m, i, &has, &diag), w3 = row_term(rows, t3, v3, mine, m, i, &has, &diag);
        part = opened ? part + w0 : w0;
        opened = true;
        part = live1 ? part + w1 : part;
        part = live2 ? part + w2 : part;
        part = live3 ? part + w3 : part;
      }
      const double s = dev::group_sum_dyn(part, g);
      // the diagonal: the first lane of the group that met it
      u64 holders = __ballot(has) >> (slot << log_g);
      if (g < kWave) holders &= (1ull << g) - 1;
      const int owner = holders != 0 ? (slot << log_g) + (__ffsll(static_cast<long long>(holders)) - 1) : lane;
      const double a_ii = __shfl(diag, owner, kWave);
      if (l == 0 && i >= 0) rows.finish(i, s, holders != 0, a_ii);
    }
  }
}

} // namespace passes
} // namespace spmv_acc
