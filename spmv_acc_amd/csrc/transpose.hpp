// transpose.hpp -- the transposed product: size rules, launchers (k_transpose.hip) and engine entries (transpose.cpp) of
//   spmv_acc_csr_transpose         stable CSR -> CSR of A^T on the device, into caller-owned arrays,
//   spmv_acc_csr_transpose_values  t_value[p] = value[perm[p]] after an in-place edit of the values,
//   spmv_acc_csr_spmv_t            y = alpha * A^T * x + beta * y straight from the caller's CSR (fp64 atomic adds).
// Constants, no tunables: nothing here is timed per matrix and nothing outlives a call (no plan, no cache entry).
// tests/test_transpose_host.py TRANSPOSE_SIZE_RULES names each rule and the GPU tests that cross it.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>

namespace spmv_acc {

constexpr int kTransPerLane = 8;                        // scatter pass: non-zeros per lane, lane l of a wavefront owns q = base + l + 64 * k
constexpr int kTransWaveChunk = 64 * kTransPerLane;     // ... so one wavefront owns 512 consecutive non-zeros,
constexpr int kTransTile = 4 * kTransWaveChunk;         // ... one workgroup a fixed tile of 2048, whatever the row lengths

// radix-sort bits of the transpose: the columns are below n, so only the low bits that can differ are sorted (n = 4 000: 12 of 32)
inline int transpose_sort_bits(int n) {
  int bits = 1;
  while (bits < 31 && (1LL << bits) < n) ++bits;
  return bits;
}

// ---- launchers (k_transpose.hip): enqueue only ---------------------------------------------------------------------------------------
// *bad (pre-zeroed) += the entries of ci[0 .. nnz) outside [0, n)
void launch_transpose_check(hipStream_t stream, const int *ci, int nnz, int n, unsigned *bad);
// stable sort of (ci[q], q) by column: keys_out = the sorted columns, perm[p] = source position of output entry p.  tmp == nullptr: *tmp_bytes
// = the scratch the sort needs, nothing is enqueued
bool launch_transpose_sort(hipStream_t stream, const int *ci, int nnz, int n, int *keys_out, int *perm, void *tmp, size_t *tmp_bytes);
// t_rowptr[c] = first p with keys[p] >= c, c = 0 .. n
void launch_transpose_rowptr(hipStream_t stream, const int *keys, int nnz, int n, int *t_rowptr);
// row_of[q] = the row that holds non-zero q (rebased rowptr)
void launch_transpose_rows(hipStream_t stream, const int *rp, int m, int nnz, int *row_of);
// t_colindex[p] = row_of[perm[p]], t_value[p] = value[perm[p]] (value / t_value may be null: structure only)
void launch_transpose_gather(hipStream_t stream, int nnz, const int *perm, const int *row_of, const double *value, int *t_colindex, double *t_value);
void launch_transpose_values(hipStream_t stream, int nnz, const int *perm, const double *value, double *t_value);
// y[0 .. n) = beta * y (beta == 0: zeros, y is not read)
void launch_spmv_t_scale(hipStream_t stream, int n, double beta, double *y);
// y[ci[q]] += alpha * v[q] * x[row of q] over the view's non-zeros [rp[0], min(rp[m], nnz_end)); columns outside [0, n) are dropped
void launch_spmv_t_scatter(hipStream_t stream, int m, int n, int nnz_end, double alpha, const int *rp, const int *ci, const double *v,
                           const double *x, double *y);

// ---- engine entries (transpose.cpp): return kOk or the error code they also leave in the calling thread's error slot -------------------
int run_csr_transpose(int m, int n, int nnz, const int *d_rowptr, const int *d_colindex, const double *d_value, int *d_t_rowptr,
                      int *d_t_colindex, double *d_t_value, int *d_perm);
int run_csr_transpose_values(int nnz, const int *d_perm, const double *d_value, double *d_t_value);
int run_csr_spmv_t(double alpha, double beta, int m, int n, int nnz, const int *d_rowptr, const int *d_colindex, const double *d_value,
                   const double *dx, double *dy);

} // namespace spmv_acc
