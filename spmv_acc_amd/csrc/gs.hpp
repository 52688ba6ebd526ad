// gs.hpp -- multicolour Gauss-Seidel / SOR for a square CSR: the definition of the colouring, the summation order of a sweep, size rules,
// launchers (k_gs.hip) and engine entries (gs.cpp) of
//   spmv_acc_csr_color     the colouring of the pattern (analysis: synchronises, not capturable), into caller-owned arrays,
//   spmv_acc_csr_gs_sweep  one forward, backward or symmetric sweep, one launch per colour (launch-only: the per-step hot path).
// Constants, no tunables: nothing here is timed per matrix and nothing outlives a call (no plan, no cache entry).
// tests/test_gs_host.py GS_SIZE_RULES names each rule and the GPU tests that cross it.
//
// THE COLOURING (a pure function of the pattern; tests/test_gs_host.py host_csr_color restates it in numpy).  A is square m x m, rebased CSR,
// rows strictly ascending, pattern symmetric.  Row v has the 64-bit priority (gs_mix32(v) << 32) | v, with
//   gs_mix32(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16      (32-bit unsigned arithmetic)
// -- distinct for distinct rows.  The rows are taken in DESCENDING priority; each gets the smallest colour >= 0 that no already-coloured
// off-diagonal neighbour holds.  That colouring is the answer: color[v], ncolors = 1 + the largest colour, color_rows = the rows in ascending
// (colour, row) -- a stable sort by colour, the perm csr_permute takes --, color_ptr[c] = the first position of colour c in color_rows.
//
// ROUNDS (Jones-Plassmann; host_csr_color_rounds).  In a round every uncoloured row looks at its off-diagonal neighbours in the colours of the
// round BEFORE (one buffer is read, another written, so a round sees no colour of its own making).  A row with an uncoloured neighbour of higher
// priority waits.  Otherwise all its higher-priority neighbours are coloured -- and no lower-priority one is: that one still waits for this row
// -- and their colours are final, so the row takes the smallest colour none of them holds: the sequential choice.  The free colour is found in
// windows of kGsColorWindow colours: a 64-bit mask of the window's used colours, its lowest clear bit, the next window if the mask is full.
// Whatever the timing, the result is the greedy colouring above, and the number of rounds is a function of the pattern too.  Rounds are
// enqueued kGsRoundsPerRead at a time; then the host reads how many rows are uncoloured (per-wavefront counts, no atomic).  A group of rounds
// that colours no row while some remain ends the call with an error: the loop cannot spin.
//
// WHY COLOURS AND NOT LEVELS.  A greedy colouring of a mesh matrix has tens of colours (a 9-point grid 7, a 27-point grid 15) where the level
// sets of its triangles run to thousands: a sweep is a short chain of wide launches, every dependency is a kernel boundary, and no kernel
// waits on another workgroup.
//
// THE SWEEP (tests/test_gs_host.py host_gs_sweep restates it bit for bit).  Colour c owns the positions [color_ptr[c], color_ptr[c + 1]) of
// color_rows (color_rows == NULL: the matrix is permuted by colour and the positions ARE the rows).  One launch per non-empty colour, in the
// order of the direction; every row i of the colour, in place:
//   s = the sum over the row's stored entries of the terms  value[p] * x[col[p]]  -- +0.0 at the diagonal's position and for a column outside
//       [0, m) --,   g = (b[i] - s) / a_ii,   x[i] = g if omega == 1.0 else x[i] + omega * (g - x[i]).
// Contraction is off: every product, the subtraction, the division and the relaxation are rounded on their own.  A row without a stored
// diagonal is left untouched, a row index outside [0, m) is skipped, a zero diagonal gives what IEEE division gives.
// THE SUMMATION ORDER (its device code: row_sweep.hpp, which the Jacobi kernels run too) is that of coo.hpp, generalised to a lane group of
// width G (a power of two, 1 .. 64): lane l adds the terms l, l + G, l + 2 G, ... of the row in that order, starting from its first (a lane
// without a term holds +0.0); the G partial sums are combined as a balanced binary tree over neighbouring lanes (q[i] = p[2 i] + p[2 i + 1],
// then the same on q, ... down to one).
// G IS CHOSEN ON THE DEVICE, per chunk: a workgroup owns kGsChunkRows consecutive positions of the colour, counted from the colour's first
// (the last chunk of a colour is shorter), adds up the (clamped) lengths of its rows and takes the smallest G with
// G * kGsTermsPerLane * rows of the chunk >= that sum, at most 64.  The entry is launch-only, so the host never learns a row length; the
// chunk's mean is the colour's mean where the colour is uniform (a mesh) and follows the rows where it is not (one hub row among short ones).
// The result is therefore a pure function of the arrays and of color_ptr -- of nothing else: not of the grid, not of timing.
// Rows of a colour do not read each other's x: that is the colouring's guarantee, and no order inside a launch matters.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>

#include "coo.hpp"

namespace spmv_acc {

constexpr int kGsColorWindow = 64;     // colours per window of the free-colour search: one 64-bit mask (K_130 crosses it twice)
constexpr int kGsRoundsPerRead = 8;    // rounds enqueued between two reads of the uncoloured count.  EVEN: the rounds alternate between the caller's
                                       // colour array and the workspace's, and after an even number the newest colours are in the caller's
constexpr int kGsCounts = 6;           // count groups of kCooCheckSlots: the census' five and the rows without a diagonal; the rounds reuse the first
constexpr int kGsChunkRows = 64;       // sweep: rows (positions of the colour) per chunk, one per lane while their extents are read: the unit G is chosen for;
constexpr int kGsTile = kGsChunkRows;  // ... a workgroup owns one chunk and deals its G passes of 64 / G rows out to its four wavefronts
constexpr int kGsTermsPerLane = 4;     // sweep: G is the smallest lane group that leaves a lane at most four terms of the chunk's mean row -- the four
                                       // independent (column, value, x) gathers the inner loop keeps in flight per lane, as wave_run_sum does: a
                                       // wider group would idle lanes on a mesh row (7 terms: G = 2, 27 terms: G = 8), a narrower one would walk
                                       // the row in dependent steps.  Reasoned from the loop's shape, not timed; not a tunable

constexpr int kGsMaxRows = 1 << 29;    // sweep: x is gathered through 32-bit byte offsets (8 * column < 2^32), which keeps the kernel at 8 waves
                                       // per SIMD; a matrix of more rows (an x beyond 4 GiB) is refused with SPMV_ACC_ERR_TOO_LARGE

// the 32-bit mixer of the priorities (constexpr: also device code)
constexpr unsigned gs_mix32(unsigned x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
constexpr unsigned long long gs_priority(unsigned v) { return static_cast<unsigned long long>(gs_mix32(v)) << 32 | v; }

// ---- launchers (k_gs.hip): enqueue only ----------------------------------------------------------------------------------------------------
// the census.  slots = kGsCounts groups of kCooCheckSlots per-wavefront counts (zeroed by the caller): (a) rowptr[0] != 0 or rowptr[m] != nnz,
// (b) rows whose extent descends or leaves [0, nnz], (c) columns outside [0, m), (d) positions where a row does not strictly ascend,
// (e) off-diagonal entries (i, j) whose mirror (j, i) is not stored, (f) rows without a diagonal entry (not an error).  Rows are read CLAMPED
// (row_extent) and a column outside [0, m) is never turned into an address.  m > 0
void launch_gs_census(hipStream_t stream, int m, int nnz, const int *rowptr, const int *colindex, unsigned *slots);
// one round: color_out from color_in (-1: uncoloured); slots[0 .. kCooCheckSlots) = per-wavefront counts of the rows still uncoloured in color_out
void launch_gs_round(hipStream_t stream, int m, int nnz, const int *rowptr, const int *colindex, const int *color_in, int *color_out,
                     unsigned *slots);
// keys[v] = color[v]
void launch_gs_keys(hipStream_t stream, int m, const int *color, unsigned long long *keys);
// ptr[c] = the first position p of the sorted keys with sorted[p] >= c, c = 0 .. count - 1 (m if there is none)
void launch_gs_color_ptr(hipStream_t stream, int m, const unsigned long long *sorted, int count, int *ptr);
// one colour of a sweep: the positions [first, last) of color_rows (nullptr: the rows themselves); 0 < m <= kGsMaxRows, nnz > 0, first < last
void launch_gs_color(hipStream_t stream, int m, int nnz, const int *rowptr, const int *colindex, const double *value, int first, int last,
                     const int *color_rows, double omega, const double *b, double *x);

// ---- engine entries (gs.cpp): return kOk or the error code they also leave in the calling thread's error slot --------------------------------
int run_csr_color(int m, int nnz, const int *d_rowptr, const int *d_colindex, int *d_color, int *d_color_rows, int cap_colors, int *h_color_ptr,
                  int *h_ncolors, int *h_no_diag);
int run_csr_gs_sweep(int m, int nnz, const int *d_rowptr, const int *d_colindex, const double *d_value, int ncolors, const int *h_color_ptr,
                     const int *d_color_rows, double omega, int direction, const double *d_b, double *d_x);

} // namespace spmv_acc
