// strength.hpp -- the strength-of-connection filter of a square CSR and the values that go with it: the definition of the kept pattern, of the
// lumped diagonal and of the prolongator smoother, size rules, launchers (k_strength.hip) and engine entries (strength.cpp) of
//   spmv_acc_csr_strength         the kept pattern S of A at a threshold theta and the stable partition of A's positions into kept and dropped
//                                 (analysis: synchronises, not capturable), into caller-owned arrays,
//   spmv_acc_csr_strength_values  the lumped diagonal and, on S's structure, the filtered matrix A_F (omega == 0) or the prolongator smoother
//                                 M = I - omega D_F^-1 A_F (launch-only: per step).
// Constants, no tunables: nothing here is timed per matrix and nothing outlives a call (no plan, no cache entry).
// tests/test_strength_host.py STRENGTH_SIZE_RULES names each rule and the GPU tests that cross it.
//
// THE KEPT PATTERN (a pure function of the arrays and theta, unique to the bit; tests/test_strength_host.py host_csr_strength restates it in
// numpy).  A is square m x m, rebased CSR, rows strictly ascending, pattern symmetric -- the colouring's contract (gs.hpp), checked by the
// colouring's census; the VALUES may be unsymmetric.  theta is finite and >= 0.
//   sd[i] = sqrt(|a_ii|), correctly rounded; +0.0 for a row without a stored diagonal.
//   For an off-diagonal entry p = (i, j):  rhs = fl(fl(sd[i] * sd[j]) * theta).  The product of the two roots commutes, so both ends of an edge
//   compute the same rhs; the form holds no square root per entry and a_ii * a_jj cannot overflow in it.  The entry is KEPT iff
//   |a_ij| >= rhs  OR  |a_ji| >= rhs,  a_ji the value at the mirror position, found by a binary search of row j (the census guarantees it is
//   stored; should a search ever miss, the entry's own comparison alone counts).  The comparisons are IEEE: a NaN on either side is false.
//   A stored diagonal entry is always kept.
// The kept pattern is therefore symmetric whatever the values: what csr_aggregate demands.  A row whose diagonal is zero or missing has rhs = 0
// against every neighbour with a finite diagonal and keeps those couplings (a NaN coupling fails both comparisons).
//   S          = the kept entries in A's order: a stable compaction, rows still strictly ascending, no sort.
//   map        = nnz entries, a stable partition of A's positions: map[0 .. nnz_s) the kept positions ascending (map[k] = the position in A of S's
//                entry k), map[nnz_s .. nnz) the dropped positions ascending.
//   s_rowptr[i] = the first kept entry of row i (m + 1 entries);  drop_ptr[i] = the first place of row i's dropped positions in map, in
//                [nnz_s, nnz] (m + 1 entries, drop_ptr[m] = nnz).
// PASSES.  The census; sd, one row per lane; the keep flag, one ENTRY per lane (the row by passes::wave_row_of, as k_extract: a long row is many
// wavefronts, and the comparisons are exact, so the mapping of lanes to entries cannot change a bit); the exclusive scan of the flags over
// nnz + 1; the two row pointers; the partitioning scatter; one read of nnz_s.  MEASURED on an MI355X with both mappings of the flags pass
// (kernel trace on tools/strength_bench.py's matrices, the same arrays from both): one entry per lane 1.50 ms on the 9-point mesh and 3.51 ms
// on the 27-point grid, one ROW per lane (the census' loop, no search for the row) 0.92 ms and 7.52 ms -- a lane that walks 27 entries reads
// and writes 64 lines per step where the entry form touches a few.  The entry form is kept: it loses 0.6 ms where rows are short, the row
// form 4 ms where they are not, and a row of tens of thousands of entries would be one lane's work.
//
// THE VALUES (tests/test_strength_host.py host_strength_values restates them bit for bit).  Two launches.
//   1, per row i.  The lump s_i = the sum of value[map[p]] over the run [drop_ptr[i], drop_ptr[i + 1]) clamped to [0, nnz], in THE SUMMATION
//      ORDER of coo.hpp (passes::sum_runs: a run of at most kCooLongRun terms by one lane from its first term, a longer one by a wavefront); a
//      map index outside [0, nnz) counts as +0.0.  The diagonal of S's row i is looked for by passes::first_at_least on s_colindex within the
//      row's extent clamped to [0, nnz_s], and read through map (+0.0 for a map index outside [0, nnz)):
//        diag[i] = a_ii, its bits copied, if the run is empty;  fl(a_ii + s_i) otherwise;  +0.0 if S's row holds no diagonal.
//      THE LUMP OF A ROW WITHOUT A STORED DIAGONAL IS DISCARDED: there is no entry of S to carry it, and the row sums of A_F then differ from
//      those of A in that row.
//   2, per S entry j in row i (the row by passes::wave_row_of on s_rowptr).  v = value[map[j]], +0.0 for an index outside [0, nnz).
//        omega == 0.0:  the filtered matrix A_F: the diagonal gets diag[i], an off-diagonal gets v, its bits copied.
//        omega != 0.0:  M = I - omega D_F^-1 A_F, so that the smoothed prolongator is one csr_spgemm(M, T):
//                       the diagonal gets  diag[i] == 0.0 ? 1.0 : fl(1.0 - omega),
//                       an off-diagonal    diag[i] == 0.0 ? +0.0 : fl(fl(-omega * v) / diag[i])      (a row with a zero diag is an identity row).
// Contraction is off wherever a value is computed.  The maps are the CALLER's arrays here: every extent is clamped and no index becomes an
// address unchecked.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>

#include "gs.hpp"

namespace spmv_acc {

constexpr int kStrengthRankTile = 256;  // flags pass and scatter: items per workgroup, one per lane: a wavefront owns 64 consecutive positions of A
constexpr int kStrengthLumpPerLane = 1; // diagonal pass: rows per lane of passes::sum_runs.  One, as the aggregation's norms (agg.hpp kAggPerLane):
                                        // a row's dropped run is a handful of dependent gathers and there are as many runs as rows, so what the
                                        // pass lacks is not loads in flight per lane.  Reasoned from that measurement, not timed again
constexpr int kStrengthLumpWaveChunk = 64 * kStrengthLumpPerLane;  // ... so one wavefront owns 64 consecutive rows,
constexpr int kStrengthLumpTile = 4 * kStrengthLumpWaveChunk;      // ... one workgroup a tile of 256
constexpr int kStrengthPerLane = 4;     // values pass: S entries per lane, lane l of a wavefront owns j = base + l + 64 k: all map loads of a lane are
                                        // issued, then the gathers, then the stores (extract.hpp kExtractPerLane's shape).  Reasoned, not timed
constexpr int kStrengthWaveChunk = 64 * kStrengthPerLane;  // ... so one wavefront owns 256 consecutive entries of S,
constexpr int kStrengthTile = 4 * kStrengthWaveChunk;      // ... one workgroup a tile of 1 024

// ---- launchers (k_strength.hip): enqueue only -----------------------------------------------------------------------------------------------
// sd[i] = sqrt(|a_ii|), +0.0 without a stored diagonal, i < m.  m > 0; the census has passed
void launch_strength_sd(hipStream_t stream, int m, int nnz, const int *rowptr, const int *colindex, const double *value, double *sd);
// flag[p] = 1 where entry p is kept (strength.hpp THE KEPT PATTERN), p < nnz; flag[nnz] = 0.  m > 0; the census has passed
void launch_strength_flags(hipStream_t stream, int m, int nnz, const int *rowptr, const int *colindex, const double *value, const double *sd,
                           double theta, int *flag);
// s_rowptr[i] = pos[rowptr[i]], drop_ptr[i] = pos[nnz] + rowptr[i] - pos[rowptr[i]], i <= m (pos = the exclusive scan of the flags)
void launch_strength_ptrs(hipStream_t stream, int m, int nnz, const int *rowptr, const int *pos, int *s_rowptr, int *drop_ptr);
// the partition: a kept p goes to s_colindex[pos[p]] and map[pos[p]], a dropped one to map[pos[nnz] + p - pos[p]].  nnz > 0
void launch_strength_scatter(hipStream_t stream, int nnz, const int *colindex, const int *flag, const int *pos, int *s_colindex, int *map);
// diag[i], i < m (strength.hpp THE VALUES, 1).  m > 0
void launch_strength_diag(hipStream_t stream, int m, int nnz, int nnz_s, const int *s_rowptr, const int *s_colindex, const int *map,
                          const int *drop_ptr, const double *value, double *diag);
// s_value[j], j < nnz_s (strength.hpp THE VALUES, 2).  m > 0
void launch_strength_values(hipStream_t stream, int m, int nnz, int nnz_s, const int *s_rowptr, const int *s_colindex, const int *map,
                            const double *value, const double *diag, double omega, double *s_value);

// ---- engine entries (strength.cpp): return kOk or the error code they also leave in the calling thread's error slot ---------------------------
int run_csr_strength(int m, int nnz, const int *d_rowptr, const int *d_colindex, const double *d_value, double theta, int *d_s_rowptr,
                     int *d_s_colindex, int *d_map, int *d_drop_ptr, int *h_nnz_s, int *h_no_diag);
int run_csr_strength_values(int m, int nnz, int nnz_s, const int *d_s_rowptr, const int *d_s_colindex, const int *d_map, const int *d_drop_ptr,
                            const double *d_value, double omega, double *d_s_value, double *d_diag);

} // namespace spmv_acc
