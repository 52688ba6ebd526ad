// jacobi.hpp -- damped Jacobi / l1-Jacobi for a square CSR: the definition of the two inverse diagonals, the summation order of a sweep, size
// rules, launchers (k_jacobi.hip) and engine entries (jacobi.cpp) of
//   spmv_acc_csr_jacobi_diagonal  dinv = 1 / a_ii (kind 0) or 1 / the scaled l1 diagonal (kind 1), once per set of values (launch-only),
//   spmv_acc_csr_jacobi_sweep     x_out = x_in + omega * dinv * (b - A x_in) and / or r_out = b - A x_in: ONE launch for all rows (launch-only:
//                                 the per-step hot path).
// Constants, no tunables: nothing here is timed per matrix and nothing outlives a call (no plan, no cache entry, no colouring).
// tests/test_jacobi_host.py JACOBI_SIZE_RULES names each rule and the GPU tests that cross it.
//
// THE DIAGONALS (tests/test_jacobi_host.py host_jacobi_diagonal restates them bit for bit).  A is square m x m, rebased CSR, rows ascending.
// No census runs: rows are read CLAMPED (passes::row_extent) and a column outside [0, m) is never turned into an address.
//   kind 0 (Jacobi):     dinv[i] = 1.0 / a_ii, a_ii the stored diagonal entry, found as launch_strength_sd finds it (the first position of the
//                        clamped row whose column is >= i, if its column is i);  +0.0 where the row stores none.
//   kind 1 (scaled l1):  g[i] = sqrt(|a_ii|), correctly rounded, +0.0 without a stored diagonal -- launch_strength_sd itself, into d_work --, then
//                        d_i = the sum over the row's stored entries of the terms  |a_ij| * fl(g[i] / g[j])  -- the quotient is rounded first,
//                        then the product; a column outside [0, m) contributes the term +0.0 at its position --,  dinv[i] = 1.0 / d_i;
//                        +0.0 where row i stores no diagonal entry (met in passing, as the Gauss-Seidel sweep meets it).
//   A missing or zero diagonal anywhere else in the sum gives what IEEE gives (x / 0 = inf, 1 / inf = +0, 0 / 0 = NaN): no further special case.
// WHY THE SCALED FORM.  For a symmetric A with a positive diagonal, the weighted AM-GM bound  2 |x_i x_j| <= t x_i^2 + x_j^2 / t  with
// t = g_i / g_j gives  x^T A x <= sum_i x_i^2 sum_j |a_ij| g_i / g_j = x^T D x:  D >= A, so I - omega D^-1 A contracts in the energy norm for
// every omega in (0, 2) and nobody has to pick a damping factor.  And D scales as A does: under A -> S A S with a diagonal S, g_i -> |s_i| g_i
// and d_i -> s_i^2 d_i, so the sweep on the scaled system is the scaled sweep.  The plain row sum of |a_ij| has the first property and not
// the second: on a matrix scaled over six decades it stalls conjugate gradients where this form needs the iterations of the unscaled twin.
//
// THE SWEEP (host_jacobi_sweep restates it bit for bit).  Every row i, out of place:
//   s = the sum over ALL the row's stored entries, the diagonal included, of the terms  value[p] * x_in[col[p]]  -- +0.0 for a column outside
//       [0, m) --,   t = b[i] - s,   w = omega * dinv[i],   r_out[i] = t (if r_out),   x_out[i] = x_in[i] + w * t (if x_out).
// Contraction is off: every product, the subtraction and the update's product and sum are rounded on their own.
// ZERO START (x_in == NULL): the matrix is not read;  t = b[i],  x_out[i] = w * b[i]  -- the first pre-sweep of a level whose x is zero.
// The sweep is out of place because Jacobi in place would race: x_out, r_out, x_in, b and dinv must not overlap each other.
// SIZE LIMIT: at most kJacobiMaxRows = 2^29 rows for the sweep and the scaled l1 diagonal, whose kernels gather through 32-bit byte offsets
// (8 * column < 2^32); more rows are refused with SPMV_ACC_ERR_TOO_LARGE before any launch.
// THE SUMMATION ORDER is the Gauss-Seidel sweep's, defined in gs.hpp (THE SUMMATION ORDER, G IS CHOSEN ON THE DEVICE) and run by the same device
// code (row_sweep.hpp), with the rows [0, m) as the one colour and no color_rows: the chunks are kJacobiTile = kGsChunkRows consecutive rows.
// The scaled l1 diagonal is summed in the same order.  Every result is therefore a pure function of the arrays -- not of the grid, not of
// timing.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>

#include "gs.hpp"

namespace spmv_acc {

constexpr int kJacobiTile = kGsChunkRows;   // rows per workgroup: one chunk of the summation order, its G passes of 64 / G rows dealt out to
                                            // the four wavefronts (as kGsTile).  The grid is one workgroup per chunk up to max_grid_blocks():
                                            // fewer, longer-lived workgroups were measured and buy nothing worth a rule (tools/jacobi_bench.py,
                                            // profiles/jacobi_bench.md, "The launch grid of the sweep": a quarter of the grid is 4 % faster
                                            // on one matrix and 2 % slower on the other, every smaller grid is slower on both)
constexpr int kJacobiMaxRows = kGsMaxRows;  // x_in (the sweep) and g (the l1 diagonal) are gathered through 32-bit byte offsets (8 * column <
                                            // 2^32), which keeps the kernels at 8 waves per SIMD; more rows: SPMV_ACC_ERR_TOO_LARGE

// ---- launchers (k_jacobi.hip): enqueue only ---------------------------------------------------------------------------------------------
// kind 0: dinv[i] = 1 / a_ii (+0.0 without a stored diagonal), one row per lane.  m > 0
void launch_jacobi_inverse(hipStream_t stream, int m, int nnz, const int *rowptr, const int *colindex, const double *value, double *dinv);
// kind 1: dinv[i] = 1 / d_i from g = launch_strength_sd's roots (THE DIAGONALS).  0 < m <= kJacobiMaxRows
void launch_jacobi_l1(hipStream_t stream, int m, int nnz, const int *rowptr, const int *colindex, const double *value, const double *g,
                      double *dinv);
// the sweep of all rows from x_in (not null); x_out or r_out may be null.  0 < m <= kJacobiMaxRows
void launch_jacobi_sweep(hipStream_t stream, int m, int nnz, const int *rowptr, const int *colindex, const double *value, const double *dinv,
                         double omega, const double *b, const double *x_in, double *x_out, double *r_out);
// the zero start: x_out[i] = (omega * dinv[i]) * b[i], r_out[i] = b[i]; either may be null.  m > 0
void launch_jacobi_start(hipStream_t stream, int m, const double *dinv, double omega, const double *b, double *x_out, double *r_out);

// ---- engine entries (jacobi.cpp): return kOk or the error code they also leave in the calling thread's error slot ----------------------------
int run_csr_jacobi_diagonal(int m, int nnz, const int *d_rowptr, const int *d_colindex, const double *d_value, int kind, double *d_dinv,
                            double *d_work);
int run_csr_jacobi_sweep(int m, int nnz, const int *d_rowptr, const int *d_colindex, const double *d_value, const double *d_dinv, double omega,
                         const double *d_b, const double *d_x_in, double *d_x_out, double *d_r_out);

} // namespace spmv_acc
