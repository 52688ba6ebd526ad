// coo.hpp -- device assembly of a CSR from unsorted (row, col, value) triples with duplicates: size rules, launchers (k_coo.hip) and engine
// entries (coo.cpp) of
//   spmv_acc_coo_to_csr         structure (rowptr, colindex), the map (order, start) and the first values, into caller-owned arrays,
//   spmv_acc_coo_to_csr_values  value[j] = the sum of the triples of CSR entry j through a kept map (launch-only: the per-step hot path).
// Constants, no tunables: nothing here is timed per matrix and nothing outlives a call (no plan, no cache entry).
// tests/test_coo_host.py COO_SIZE_RULES names each rule and the GPU tests that cross it.
//
// THE SUMMATION ORDER (a pure function of the map; tests/test_coo_host.py coo_sum_model restates it in numpy).  Run j holds the values
// v[0 .. k) = d_val[d_order[d_start[j] + t]], t = 0 .. k - 1, in ascending input position.
//   k <= kCooLongRun:  one lane adds them in that order, starting from v[0] (not from 0.0): s = v[0]; s += v[1]; ... -- bitwise a host loop.
//   k >  kCooLongRun:  a whole wavefront.  Lane l adds v[l], v[l + 64], v[l + 128], ... in that order, starting from v[l] (every lane has
//                      one: k > 64), which gives 64 partial sums p[0 .. 64).  They are combined as a balanced binary tree over neighbouring
//                      lanes, six levels: q[i] = p[2 i] + p[2 i + 1] (32 sums), then r[i] = q[2 i] + q[2 i + 1] (16), ... down to one.
//                      (fp64 addition is commutative, so which of two partners is the left operand does not matter.)
// An entry of d_order outside [0, nnz_coo) -- never produced by the first entry -- counts as +0.0 in either form.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>

namespace spmv_acc {

constexpr int kCooLongRun = 64;                      // runs of more triples than this are summed by a wavefront, shorter ones by one lane
constexpr int kCooPerLane = 6;                       // summing pass: CSR entries per lane, lane l of a wavefront owns j = base + l + 64 * k.  (Six: with
                                                     // eight the kernel takes 80 VGPRs = 6 waves per SIMD; six in 60 VGPRs at 8 waves keeps as many in flight.)
constexpr int kCooWaveChunk = 64 * kCooPerLane;      // ... so one wavefront owns 384 consecutive entries,
constexpr int kCooTile = 4 * kCooWaveChunk;          // ... one workgroup a tile of 1536
constexpr int kCooCheckBlocks = 1024;                // range census: at most this many workgroups, each wavefront leaves its count in a slot of its own
constexpr int kCooCheckSlots = 4 * kCooCheckBlocks;  // ... which the host adds up (an integer count without an atomic)

// bits that can differ in an index below n (n = 4 000: 12); the packed sort key is row << coo_index_bits(n) | col, and only its low
// coo_index_bits(m) + coo_index_bits(n) bits are sorted (up to 62: the key is 64 bits wide whatever the shape)
inline int coo_index_bits(int n) {
  int bits = 1;
  while (bits < 31 && (1LL << bits) < n) ++bits;
  return bits;
}

// ---- launchers (k_coo.hip): enqueue only ---------------------------------------------------------------------------------------------
// slots[0 .. kCooCheckSlots) = per-wavefront counts of the triples with row outside [0, m) or col outside [0, n) (every slot is written)
void launch_coo_check(hipStream_t stream, const int *row, const int *col, int nnz_coo, int m, int n, unsigned *slots);
// keys[q] = row[q] << col_bits | col[q]
void launch_coo_keys(hipStream_t stream, const int *row, const int *col, int nnz_coo, int col_bits, unsigned long long *keys);
// stable sort of (keys[q], q): keys_out = the sorted keys, order[p] = input position of sorted entry p.  tmp == nullptr: *tmp_bytes = the
// scratch the sort needs, nothing is enqueued
bool launch_coo_sort(hipStream_t stream, const unsigned long long *keys, int nnz_coo, int key_bits, unsigned long long *keys_out, int *order,
                     void *tmp, size_t *tmp_bytes);
// head[p] = 1 where sorted entry p opens a run (p == 0 or its key differs from its predecessor's), p < nnz_coo; head[nnz_coo] = 0
void launch_coo_heads(hipStream_t stream, const unsigned long long *keys, int nnz_coo, int *head);
// index[p] = head[0] + ... + head[p - 1], p = 0 .. nnz_coo (index[nnz_coo] = the number of runs).  tmp == nullptr: *tmp_bytes only
bool launch_coo_scan(hipStream_t stream, const int *head, int nnz_coo, int *index, void *tmp, size_t *tmp_bytes);
// for every run head p: start[index[p]] = p, colindex[index[p]] = the key's column; start[index[nnz_coo]] = nnz_coo
void launch_coo_entries(hipStream_t stream, const unsigned long long *keys, const int *head, const int *index, int nnz_coo, int col_bits,
                        int *start, int *colindex);
// rowptr[r] = index[first p with key's row >= r], r = 0 .. m
void launch_coo_rowptr(hipStream_t stream, const unsigned long long *keys, const int *index, int nnz_coo, int m, int col_bits, int *rowptr);
// value[j] = the sum of run j in the order documented above, j < nnz
void launch_coo_values(hipStream_t stream, int nnz_coo, int nnz, const int *order, const int *start, const double *val, double *value);

// ---- engine entries (coo.cpp): return kOk or the error code they also leave in the calling thread's error slot ----------------------------
int run_coo_to_csr(int m, int n, int nnz_coo, const int *d_row, const int *d_col, const double *d_val, int *d_rowptr, int *d_colindex,
                   double *d_value, int *d_order, int *d_start, int *h_nnz);
int run_coo_to_csr_values(int nnz_coo, int nnz, const int *d_order, const int *d_start, const double *d_val, double *d_value);

} // namespace spmv_acc
