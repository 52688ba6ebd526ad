// spmm.hpp -- the size rules of the CSR SpMM (k_spmm.hip kernels, spmm.cpp engine).  Constants, no tunables: SpMM runs no per-matrix timings, its
// shape is a rule on (m, nnz, k, layout).  tests/test_spmm_host.py SPMM_SIZE_RULES names each rule and the GPU tests that cross it.
#pragma once

namespace spmv_acc {

constexpr int kSpmmPanel = 32;    // columns of X / Y per pass over the matrix (k > kSpmmPanel: one pass per panel, the last one narrower)
constexpr int kSpmmLongRow = 256; // rows with more non-zeros are cut into pieces (a team walking a hub row alone would be latency-bound)
constexpr int kSpmmPiece = 256;   // non-zeros per piece of a long row: one wavefront, four per lane

} // namespace spmv_acc
