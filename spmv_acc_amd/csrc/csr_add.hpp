// csr_add.hpp -- device CSR sparse add C = alpha * A + beta * B by ranks: size rules, launchers (k_csr_add.hip) and engine entries (csr_add.cpp) of
//   spmv_acc_csr_add         structure (rowptr, colindex), the map (ia, ib) and the first values, into caller-owned arrays,
//   spmv_acc_csr_add_values  value[j] = alpha * a_value[ia[j]] + beta * b_value[ib[j]] through a kept map (launch-only: the per-step hot path).
// Constants, no tunables: nothing here is timed per matrix and nothing outlives a call (no plan, no cache entry).
// tests/test_csr_add_host.py CSR_ADD_SIZE_RULES names each rule and the GPU tests that cross it.
//
// THE DEFINITION.  A and B are m x n, rebased CSR, every row STRICTLY ascending in column (what spmv_acc_coo_to_csr, spmv_acc_csr_transpose and
// spmv_acc_csr_spgemm write).  Row i of C is the sorted union of row i of A and row i of B; nothing is pruned (an entry whose value cancels stays).
// ia[j] / ib[j] = the position of C entry j in A's / B's arrays, or -1 where that matrix has no entry there; at least one is >= 0.
// With ta = alpha * a_value[ia[j]] and tb = beta * b_value[ib[j]], each ROUNDED to fp64:  both present: value[j] = ta + tb;  only A: ta;  only B: tb.
// No fused multiply-add and no implicit + 0.0: an A-only -0.0 with alpha = 1 stays -0.0; alpha == 0 is not special (0 * Inf = NaN propagates);
// the pattern is the union whatever alpha and beta are.  In the values entry a map index outside [0, nnz_a) / [0, nnz_b) counts as absent, and an
// entry with both absent is +0.0.  tests/test_csr_add_host.py host_csr_add restates all of it in numpy.  The result is unique: no choice below
// can change a bit of it.
//
// STRUCTURE BY RANKS (chosen over a merge path: with strictly ascending rows no sort and no merge is needed, the place of every entry of C is a
// rank each non-zero computes on its own, and every pass is cut by non-zeros; the two forms were not timed against each other).
//   1. match:  for every non-zero q of A, in row i: pos = the first position of B's row i whose column is >= a_colindex[q]; bpos[q] = pos where
//              B holds that column there, ~pos (negative) where it does not.  bpos[nnz_a] = -1.
//   2. ms = the exclusive scan (rocPRIM) of [bpos[q] >= 0] over nnz_a + 1: the matched non-zeros of A before q.  nnz(C) = nnz_a + nnz_b - ms[nnz_a].
//   3. c_rowptr[i] = a_rowptr[i] + b_rowptr[i] - ms[a_rowptr[i]].
//   4. A's non-zero q is C entry j = q + pos - ms[q]  (= c_rowptr[i] + its rank in A's row + the B columns below it - the matches before it in
//      the row): colindex[j] = a_colindex[q], ia[j] = q, ib[j] = pos if matched, else -1.
//   5. B's non-zero t, in row i: apos = the first position of A's row i whose column is >= b_colindex[t].  A holds the column: skip (A's lane wrote
//      the entry).  Otherwise C entry j = t + apos - ms[apos]: colindex[j] = b_colindex[t], ia[j] = -1, ib[j] = t.
// The row of a non-zero comes from a search in rowptr: once per wavefront for the ends of its 64 consecutive non-zeros, then per lane between them.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>

#include "coo.hpp"

namespace spmv_acc {

constexpr int kCsrAddPerLane = 4;                       // values pass: C entries per lane, lane l of a wavefront owns j = base + l + 64 * k: four pairs
                                                        // of map loads, then four pairs of gathers in flight (k_csr_add.hip records the VGPRs)
constexpr int kCsrAddWaveChunk = 64 * kCsrAddPerLane;   // ... so one wavefront owns 256 consecutive entries,
constexpr int kCsrAddTile = 4 * kCsrAddWaveChunk;       // ... one workgroup a tile of 1024
constexpr int kCsrAddRankTile = 256;                    // structure passes (census, match, the two scatters): one non-zero per lane, a wavefront 64
                                                        // consecutive ones (one search in rowptr for their ends), a workgroup a tile of 256

// ---- launchers (k_csr_add.hip): enqueue only ----------------------------------------------------------------------------------------------
// (every row is read as [lo, hi) = rowptr[i], rowptr[i + 1] CLAMPED to 0 <= lo <= hi <= nnz, so positions stay inside the arrays whatever
// rowptr holds; m > 0 in all of them)
// the census of both matrices in one launch.  slots = 6 groups of kCooCheckSlots per-wavefront counts (zeroed by the caller): for A, then for B,
// (a) columns outside [0, n), (b) positions inside a row with col[q] <= col[q - 1], (c) rows whose rowptr extent descends or leaves [0, nnz]
void launch_csr_add_census(hipStream_t stream, int m, int n, int nnz_a, const int *a_rowptr, const int *a_colindex, int nnz_b, const int *b_rowptr,
                           const int *b_colindex, unsigned *slots);
// step 1: bpos[0 .. nnz_a]
void launch_csr_add_match(hipStream_t stream, int m, int nnz_a, const int *a_rowptr, const int *a_colindex, int nnz_b, const int *b_rowptr,
                          const int *b_colindex, int *bpos);
// step 2: ms[q] = the number of bpos[0 .. q) that are >= 0, q = 0 .. nnz_a.  tmp == nullptr: *tmp_bytes = the scratch it needs, nothing is enqueued
bool launch_csr_add_scan(hipStream_t stream, const int *bpos, int nnz_a, int *ms, void *tmp, size_t *tmp_bytes);
// step 3: c_rowptr[0 .. m]
void launch_csr_add_rowptr(hipStream_t stream, int m, int nnz_a, const int *a_rowptr, const int *b_rowptr, const int *ms, int *c_rowptr);
// steps 4 and 5.  ia and ib may both be null (structure only, no map); every j is held inside [0, nnz_a + nnz_b)
void launch_csr_add_place_a(hipStream_t stream, int nnz_a, int nnz_b, const int *a_colindex, const int *bpos, const int *ms, int *c_colindex,
                            int *ia, int *ib);
void launch_csr_add_place_b(hipStream_t stream, int m, int nnz_a, const int *a_rowptr, const int *a_colindex, int nnz_b, const int *b_rowptr,
                            const int *b_colindex, const int *ms, int *c_colindex, int *ia, int *ib);
// value[j] by the definition above, j < nnz_c
void launch_csr_add_values(hipStream_t stream, int nnz_c, int nnz_a, int nnz_b, const int *ia, const int *ib, double alpha, const double *a_value,
                           double beta, const double *b_value, double *value);

// ---- engine entries (csr_add.cpp): return kOk or the error code they also leave in the calling thread's error slot -----------------------------
int run_csr_add(int m, int n, int nnz_a, const int *d_a_rowptr, const int *d_a_colindex, int nnz_b, const int *d_b_rowptr, const int *d_b_colindex,
                double alpha, const double *d_a_value, double beta, const double *d_b_value, int *d_c_rowptr, int *d_c_colindex, double *d_c_value,
                int *d_ia, int *d_ib, int *h_nnz);
int run_csr_add_values(int nnz_c, int nnz_a, int nnz_b, const int *d_ia, const int *d_ib, double alpha, const double *d_a_value, double beta,
                       const double *d_b_value, double *d_c_value);

} // namespace spmv_acc
