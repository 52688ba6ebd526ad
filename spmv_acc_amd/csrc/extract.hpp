// extract.hpp -- device CSR extraction C = A[rows, colmap] with a diagonal band: size rules, launchers (k_extract.hip) and engine entries
// (extract.cpp) of
//   spmv_acc_csr_extract         structure (rowptr, colindex), the map and the first values, into caller-owned arrays,
//   spmv_acc_csr_extract_values  value[j] = a_value[map[j]] through a kept map (launch-only: the per-step hot path).
// Constants, no tunables: nothing here is timed per matrix and nothing outlives a call (no plan, no cache entry).
// tests/test_extract_host.py EXTRACT_SIZE_RULES names each rule and the GPU tests that cross it.
//
// THE DEFINITION.  A is m x n, rebased CSR; its rows may be in any column order and may repeat a column.  Row i of C (mc x nc) is row rows[i]
// of A (rows distinct; NULL: rows[i] = i).  An entry with column c gets the new column colmap[c]; a negative colmap[c] drops it (the
// non-negative values are distinct and < nc; NULL: the identity).  An entry at (i, j) of C is kept iff diag_lo <= (long long)j - i <= diag_hi,
// in C's own indices.  Row i of C holds the kept entries in ascending new column; entries of equal new column -- only where A's row repeats a
// column -- stay in ascending position of A.  map[j] = the position of C entry j in A's arrays and value[j] = a_value[map[j]]: the bits are
// copied, nothing is pruned by value.  tests/test_extract_host.py host_csr_extract restates all of it in numpy.  The result is unique: no
// choice below can change a bit of it.
//
// STRUCTURE BY COMPACTION AND A CONDITIONAL SORT.  A candidate is an entry of a selected row of A.
//   1. census of rows and colmap (before anything reads through them); len[i] = the length of A's row rows[i].
//   2. src_ptr = the exclusive scan (rocPRIM) of len over mc + 1; S = src_ptr[mc] <= nnz_a candidates.
//   3. per candidate s, in C row i (a search in src_ptr): q = a_rowptr[rows[i]] + s - src_ptr[i], c = a_colindex[q] (counted when outside
//      [0, n): the rest of the census), newcol[s] = colmap[c] where it is >= 0 and inside the band, else -1.  newcol[S] = -1.
//   4. pos = the exclusive scan of [newcol[s] >= 0] over S + 1; c_rowptr[i] = pos[src_ptr[i]]; nnz(C) = pos[S].
//   5. scatter: colindex[pos[s]] = newcol[s], map[pos[s]] = q -- a stable compaction, C in A's order.
//   6. count the descents inside a row (col[j] < col[j - 1]).  None (an identity or order-preserving colmap on sorted rows: sub-blocks,
//      triangles, row gathers): the compaction is the answer.  Otherwise ONE stable radix sort of the keys i << coo_index_bits(nc) | col over
//      coo_index_bits(mc) + coo_index_bits(nc) bits; colindex from the sorted keys, map = map_tmp[order].  The row pointer does not change.
//      Both paths give the same bits (a stable sort of an ascending sequence is the identity); only the time differs.
// The row of a candidate or of a C entry comes from a search in src_ptr / c_rowptr: once per wavefront for the ends of its 64 consecutive
// items, then per lane between them.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>

#include "coo.hpp"

namespace spmv_acc {

constexpr int kExtractPerLane = 8;                        // values pass: C entries per lane, lane l of a wavefront owns j = base + l + 64 * k: eight map
                                                          // loads, then eight gathers in flight.  (Eight: 26 VGPRs; four take 18 and sixteen 52, all at
                                                          // 8 waves per SIMD -- eight gathers in flight per lane as the row-block SpMV keeps; the three were not timed)
constexpr int kExtractWaveChunk = 64 * kExtractPerLane;   // ... so one wavefront owns 512 consecutive entries,
constexpr int kExtractTile = 4 * kExtractWaveChunk;       // ... one workgroup a tile of 2048
constexpr int kExtractRankTile = 256;                     // structure passes (candidates, scatter, descents, keys): one item per lane, a wavefront 64
                                                          // consecutive ones (one search for their ends), a workgroup a tile of 256

// ---- launchers (k_extract.hip): enqueue only ----------------------------------------------------------------------------------------------
// (rows == nullptr: rows[i] = i; colmap == nullptr: the identity.  A's row r is read as [lo, hi) = a_rowptr[r], a_rowptr[r + 1] CLAMPED to
// 0 <= lo <= hi <= nnz_a, so positions stay inside the arrays whatever a_rowptr holds)
// the two steps of the distinctness test, step one: inv_row[rows[i]] = i for rows inside [0, m), inv_col[colmap[c]] = c for values inside
// [0, nc) -- plain stores, one of several equal ones wins.  Either pair may be null
void launch_extract_mark(hipStream_t stream, int mc, int m, const int *rows, int *inv_row, int n, int nc, const int *colmap, int *inv_col);
// ... step two and the rest of the census.  slots = 5 groups of kCooCheckSlots per-wavefront counts (zeroed by the caller): (a) rows outside
// [0, m), (b) rows with inv_row[rows[i]] != i (repeated), (c) selected rows whose extent descends or leaves [0, nnz_a], (d) colmap values >= nc,
// (e) non-negative colmap values with inv_col[colmap[c]] != c (repeated).  len[i] = the clamped length of the selected row (0 for a row outside
// [0, m)), len[mc] = 0
void launch_extract_census(hipStream_t stream, int mc, int m, int nnz_a, const int *rows, const int *a_rowptr, const int *inv_row, int n, int nc,
                           const int *colmap, const int *inv_col, int *len, unsigned *slots);
// out[p] = in[0] + ... + in[p - 1], p = 0 .. count - 1.  tmp == nullptr: *tmp_bytes = the scratch it needs, nothing is enqueued
bool launch_extract_scan(hipStream_t stream, const int *in, size_t count, int *out, void *tmp, size_t *tmp_bytes);
// ... of [newcol[s] >= 0]
bool launch_extract_scan_kept(hipStream_t stream, const int *newcol, size_t count, int *pos, void *tmp, size_t *tmp_bytes);
// step 3: newcol[0 .. S]; slots = kCooCheckSlots per-wavefront counts of the candidates with a column outside [0, n)
void launch_extract_candidates(hipStream_t stream, int mc, int nnz_a, int S, const int *rows, const int *a_rowptr, const int *a_colindex,
                               const int *src_ptr, int n, const int *colmap, int diag_lo, int diag_hi, int *newcol, unsigned *slots);
// step 4: c_rowptr[0 .. mc]
void launch_extract_rowptr(hipStream_t stream, int mc, const int *src_ptr, const int *pos, int *c_rowptr);
// step 5.  map may be null; every place is held inside [0, cap)
void launch_extract_scatter(hipStream_t stream, int mc, int nnz_a, int S, int cap, const int *rows, const int *a_rowptr, const int *src_ptr,
                            const int *newcol, const int *pos, int *c_colindex, int *map);
// step 6: slots = kCooCheckSlots per-wavefront counts of the C entries j, not the first of their row, with colindex[j] < colindex[j - 1]
void launch_extract_descents(hipStream_t stream, int mc, int nnz_c, const int *c_rowptr, const int *c_colindex, unsigned *slots);
// keys[j] = row of entry j << col_bits | colindex[j]
void launch_extract_keys(hipStream_t stream, int mc, int nnz_c, const int *c_rowptr, const int *c_colindex, int col_bits, unsigned long long *keys);
// colindex[j] = the column of sorted key j; map[j] = map_tmp[order[j]] (both map arrays may be null)
void launch_extract_sorted(hipStream_t stream, int nnz_c, const unsigned long long *keys, int col_bits, const int *order, const int *map_tmp,
                           int *c_colindex, int *map);
// value[j] = a_value[map[j]], +0.0 for a map index outside [0, nnz_a), j < nnz_c
void launch_extract_values(hipStream_t stream, int nnz_c, int nnz_a, const int *map, const double *a_value, double *value);

// ---- engine entries (extract.cpp): return kOk or the error code they also leave in the calling thread's error slot ----------------------------
int run_csr_extract(int m, int n, int nnz_a, const int *d_a_rowptr, const int *d_a_colindex, const double *d_a_value, int mc, const int *d_rows,
                    int nc, const int *d_colmap, int diag_lo, int diag_hi, int *d_c_rowptr, int *d_c_colindex, double *d_c_value, int *d_map,
                    int *h_nnz);
int run_csr_extract_values(int nnz_c, int nnz_a, const int *d_map, const double *d_a_value, double *d_c_value);

} // namespace spmv_acc
