// spgemm.hpp -- device CSR SpGEMM C = A * B by expand - sort - compress: size rules, launchers (k_spgemm.hip) and engine entries (spgemm.cpp) of
//   spmv_acc_csr_spgemm_products  the number of scalar products a_ik * b_kj = the expansion's size = the upper bound on nnz(C),
//   spmv_acc_csr_spgemm           structure (rowptr, colindex), the map (pa, pb, start) and the first values, into caller-owned arrays,
//   spmv_acc_csr_spgemm_values    value[j] = the sum of the products of C entry j through a kept map (launch-only: the per-step hot path).
// Constants, no tunables: nothing here is timed per matrix and nothing outlives a call (no plan, no cache entry).
// tests/test_spgemm_host.py SPGEMM_SIZE_RULES names each rule and the GPU tests that cross it.
//
// THE EXPANSION ORDER.  Product e enumerates A's non-zeros q in storage order and, for each, the entries t of B's row a_colindex[q] in storage
// order: e = off[q] + (t - b_rowptr[a_colindex[q]]), off = the exclusive scan of the lengths of B's rows a_colindex[q].  Its key is
// (row of q, b_colindex[t]), packed as coo.hpp packs a triple's.  ONE stable sort of (key, e) -- coo.hpp's launcher -- then products with equal
// (i, j) form a run in ascending e; run j is C entry j = sorted positions [start[j], start[j + 1]); pa[p] / pb[p] = the positions of the two
// factors of sorted product p in A's / B's arrays.
//
// THE SUMMATION ORDER is coo.hpp's, on the products v[t] = a_value[pa[start[j] + t]] * b_value[pb[start[j] + t]], each ROUNDED to fp64 before it
// is added (no fused multiply-add): runs of up to kCooLongRun products by one lane starting from v[0], longer ones by a wavefront -- strided
// partial sums, then the balanced tree.  tests/test_spgemm_host.py host_spgemm restates all of it in numpy.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>

#include "coo.hpp"

namespace spmv_acc {

constexpr int kSpgemmPerLane = 4;                          // values pass: C entries per lane, lane l of a wavefront owns j = base + l + 64 * k.  (Four: every
                                                           // step keeps two index loads and two gathers per entry in flight, twice the assembly's, whose six
                                                           // fill its 64 VGPRs; four take 54 VGPRs here, held to 8 waves per SIMD in k_spgemm.hip.)
constexpr int kSpgemmWaveChunk = 64 * kSpgemmPerLane;      // ... so one wavefront owns 256 consecutive entries,
constexpr int kSpgemmTile = 4 * kSpgemmWaveChunk;          // ... one workgroup a tile of 1024
constexpr int kSpgemmExpandPerLane = 4;                    // expansion: products per lane, lane l owns e = base + l + 64 * k
constexpr int kSpgemmExpandChunk = 64 * kSpgemmExpandPerLane; // ... a wavefront 256 consecutive products (one binary search in off for its ends),
constexpr int kSpgemmExpandTile = 4 * kSpgemmExpandChunk;  // ... a workgroup a tile of 1024: the product stream is cut evenly, whatever B's rows look like

// ---- launchers (k_spgemm.hip): enqueue only --------------------------------------------------------------------------------------------
// (every B row is read as [lo, hi) = b_rowptr[c], b_rowptr[c + 1] CLAMPED to 0 <= lo <= hi <= nnz_b, so a rowptr that does not ascend
// still yields positions inside B's arrays; the columns c of A have passed the range census before any of these runs)
// count[q] = the length of B's row a_colindex[q], arow[q] = the row of A that holds non-zero q, q < nnz_a; count[nnz_a] = 0.  arow may be null
void launch_spgemm_counts(hipStream_t stream, int m, int nnz_a, const int *a_rowptr, const int *a_colindex, const int *b_rowptr, int nnz_b,
                          long long *count, int *arow);
// *total = count[0] + ... + count[nnz_a - 1] (on the device).  tmp == nullptr: *tmp_bytes = the scratch it needs, nothing is enqueued
bool launch_spgemm_reduce(hipStream_t stream, const long long *count, int nnz_a, long long *total, void *tmp, size_t *tmp_bytes);
// off[q] = count[0] + ... + count[q - 1], q = 0 .. nnz_a (off[nnz_a] = the number of products).  tmp == nullptr: *tmp_bytes only
bool launch_spgemm_scan(hipStream_t stream, const long long *count, int nnz_a, long long *off, void *tmp, size_t *tmp_bytes);
// keys[e] = arow[q] << col_bits | b_colindex[t] for the product e = off[q] + (t - lo of B's row a_colindex[q]), e < nprod = off[nnz_a]
void launch_spgemm_expand(hipStream_t stream, int nnz_a, int nprod, const long long *off, const int *arow, const int *a_colindex,
                          const int *b_rowptr, int nnz_b, const int *b_colindex, int col_bits, unsigned long long *keys);
// on entry pa[p] = the product e of sorted position p (the sort's order) and keys = the sorted keys; on return pa[p] = its q, pb[p] = its t
void launch_spgemm_map(hipStream_t stream, int m, int nnz_a, int nprod, const unsigned long long *keys, int col_bits, const long long *off,
                       const int *a_rowptr, const int *a_colindex, const int *b_rowptr, int nnz_b, int *pa, int *pb);
// value[j] = the sum of a_value[pa[p]] * b_value[pb[p]] over run j = [start[j], start[j + 1]) in the order documented above, j < nnz_c
void launch_spgemm_values(hipStream_t stream, int nprod, int nnz_c, const int *pa, const int *pb, const int *start, const double *a_value,
                          const double *b_value, double *value);

// ---- engine entries (spgemm.cpp): return kOk or the error code they also leave in the calling thread's error slot ---------------------------
int run_csr_spgemm_products(int m, int k, int nnz_a, const int *d_a_rowptr, const int *d_a_colindex, const int *d_b_rowptr, long long *h_nprod);
int run_csr_spgemm(int m, int k, int n, int nnz_a, const int *d_a_rowptr, const int *d_a_colindex, const double *d_a_value, int nnz_b,
                   const int *d_b_rowptr, const int *d_b_colindex, const double *d_b_value, int nprod, int *d_c_rowptr, int *d_c_colindex,
                   double *d_c_value, int *d_pa, int *d_pb, int *d_start, int *h_nnz);
int run_csr_spgemm_values(int nprod, int nnz_c, const int *d_pa, const int *d_pb, const int *d_start, const double *d_a_value,
                          const double *d_b_value, double *d_c_value);

} // namespace spmv_acc
