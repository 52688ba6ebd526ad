// dense.hpp -- the dense solve of a small square CSR, for the coarsest level of a multigrid hierarchy: the definition of the inverse, the summation
// order of its apply, size rules, launchers (k_dense.hip) and engine entries (dense.cpp) of
//   spmv_acc_csr_dense_inverse  inv = A^-1 as a dense row-major m x m array by Gauss-Jordan elimination with partial pivoting (analysis:
//                               synchronises, not capturable), into a caller-owned array,
//   spmv_acc_dense_apply        x = inv b, one wavefront per row (launch-only: the per-step hot path).
// Constants, no tunables: nothing here is timed per matrix and nothing outlives a call (no plan, no cache entry).
// tests/test_dense_host.py DENSE_SIZE_RULES names each rule and the GPU tests that cross it.
//
// THE DEFINITION (a pure function of the arrays, unique to the bit; tests/test_dense_host.py host_dense_inverse restates it in numpy).  A is
// square m x m, rebased CSR, rows strictly ascending, columns in [0, m); the pattern need not be symmetric.
//   1. Start from E = [A | I], m x 2m.  Positions not stored are +0.0.
//   2. For k = 0 .. m - 1, steps 3 to 6.
//   3. The pivot row: p is the smallest i in [k, m) whose |E[i, k]| equals the maximum over the non-NaN magnitudes of E[k .. m - 1, k]; if all
//      of them are NaN, p = k.  Order-independent: a tree reduction gives the same p.
//   4. Swap rows k and p.  piv = E[k, k].  If piv is zero, NaN or infinite and no earlier step was flagged, info = k + 1.  The step is carried
//      out all the same.
//   5. Scale the pivot row: E[k, j] = E[k, j] / piv for every j -- an IEEE division, not a reciprocal multiply.
//   6. Every row i != k, with f = E[i, k] taken before the row changes: E[i, j] = E[i, j] - f * E[k, j], the product and the subtraction each
//      rounded on their own (contraction is off).
//   7. The result is the right half of E.
//   8. info == 0: the inverse is valid.  info != 0: the contents of inv are unspecified.
// The comparison contract is the bits, with -0.0 and +0.0 equal and NaNs compared by position.
// THE UNBLOCKED ORDER IS THE DEFINITION: the elimination is not blocked, and a step is a chain of launches (COST: 3 m launches and m passes
// over E): dependencies are kernel boundaries, no kernel waits on another workgroup and nothing is atomic.
// PASSES.  The census (the colouring's, k_gs.hip; its mirror count is not judged); E = [0 | I]; A scattered into the left half, one row per lane
// (rows strictly ascend: no position is written twice); then per step k
//   a. the pivot search, ONE workgroup of kDensePivotThreads lanes striding over the rows [k, m): every lane keeps the (magnitude, row) it
//      prefers, the workgroup combines them in LDS as a tree, and its first lane writes p, piv and -- if it is the first -- info: ordinary
//      stores to a state the next launches read;
//   b. the row pass over j < 2m: the old row k goes to row p, the scaled pivot row to row k and to the side buffer prow; the lane of column k
//      also leaves the old E[k, k] as the multiplier of row p; the lanes behind them copy the multipliers f[i] = E[i, k] of every row but k and p
//      to the side buffer (the column they read is written by the lane of column k in rows k and p only: no lane reads what another writes);
//   c. the rank-1 update E[i, j] -= f[i] * prow[j], i != k, one element per lane, reading the two side buffers and its own element only.
// Last, the right half is copied to inv and the host reads info, once.
//
// THE APPLY (tests/test_dense_host.py host_dense_apply restates it bit for bit).  x[i] = the sum of the terms inv[i, j] * b[j], each product
// rounded on its own, in THE SUMMATION ORDER of gs.hpp with G = 64: lane l adds the terms l, l + 64, ... in that order starting from its first
// (a lane without a term holds +0.0), the 64 partial sums are combined as the balanced tree over neighbouring lanes (tests/test_gs_host.py
// row_sum(terms, 64)).  One wavefront per row: a step reads a 512-B line of the row and of b.  b is not staged in LDS: it is m <= 4096 doubles
// that every wavefront reads in the same order, and stays in the L2.  The result is a pure function of the arrays: not of the grid, not of
// timing.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>

#include "gs.hpp"

namespace spmv_acc {

constexpr int kDenseMaxRows = 4096;       // the cap of the inverse: at 4096 rows inv is 128 MiB and the workspace E 256 MiB -- what a coarsest level may
                                          // cost beside a fine matrix of GiBs.  Reasoned from memory, not timed
constexpr int kDensePivotThreads = 256;   // the pivot search is one workgroup of four wavefronts: a column of at most 4096 rows is 16 strided reads a lane,
                                          // and one workgroup needs no second launch to combine.  Reasoned, not timed
constexpr int kDenseTile = 256;           // elements (fill, row pass, update, copy) or rows (scatter) per workgroup, one per lane
constexpr int kDenseRowsPerBlock = 4;     // apply: rows per workgroup, one per wavefront
constexpr int kDenseState = 3;            // the step's state on the device, in 8-byte words: p, piv, info -- written by the pivot workgroup only

// ---- launchers (k_dense.hip): enqueue only; 0 < m <= kDenseMaxRows; E is m x 2m row-major ------------------------------------------------------
// E = [0 | I]
void launch_dense_fill(hipStream_t stream, int m, double *E);
// the stored entries of A into the left half of E.  The census has passed
void launch_dense_scatter(hipStream_t stream, int m, int nnz, const int *rowptr, const int *colindex, const double *value, double *E);
// step k, a: state[0] = p (as an integer), state[1] = piv, state[2] = info (an integer; set to k + 1 if piv is not finite and non-zero and info is 0)
void launch_dense_pivot(hipStream_t stream, int m, int k, const double *E, unsigned long long *state);
// step k, b: the swap, the scaled pivot row (into E and prow[0 .. 2m)), the multipliers f[0 .. m) (f[k] is not written and not read)
void launch_dense_row(hipStream_t stream, int m, int k, double *E, const unsigned long long *state, double *prow, double *f);
// step k, c: E[i, j] -= f[i] * prow[j], i != k
void launch_dense_update(hipStream_t stream, int m, int k, double *E, const double *prow, const double *f);
// inv = the right half of E
void launch_dense_copy(hipStream_t stream, int m, const double *E, double *inv);
// x = inv b (THE APPLY)
void launch_dense_apply(hipStream_t stream, int m, const double *inv, const double *b, double *x);

// ---- engine entries (dense.cpp): return kOk or the error code they also leave in the calling thread's error slot --------------------------------
int run_csr_dense_inverse(int m, int nnz, const int *d_rowptr, const int *d_colindex, const double *d_value, double *d_inv, int *h_info);
int run_dense_apply(int m, const double *d_inv, const double *d_b, double *d_x);

} // namespace spmv_acc
