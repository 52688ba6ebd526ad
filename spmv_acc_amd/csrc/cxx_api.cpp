// cxx_api.cpp -- the C++-linkage symbols the reference's own executables link against
// (spmv-cli: cli/main.cpp:102,110,117; spmv-gpu-benchmark: benchmark/benchmark_spmv_acc.hpp:27-200).
// Each one has the reference's exact signature (hence the same mangled name) and forwards to the
// engine with the strategy it names.
#include <hip/hip_runtime.h>

#include "../../include/api/spmv.h"
#include "../../include/spmv_acc_strategies.hpp"
#include "engine.hpp"

using namespace spmv_acc;

namespace {
inline void go(int strategy, int trans, double alpha, double beta, const csr_desc<int, double> *h,
               const csr_desc<int, double> &d, const double *x, double *y) {
  run_spmv(strategy, trans, alpha, beta, d.rows, d.cols, d.nnz, h ? h->row_ptr : nullptr, d.row_ptr, d.col_index,
           d.values, x, y);
}
} // namespace

// src/acc/strategy_picker.cpp:19-65
void sparse_csr_spmv(int trans, const double alpha, const double beta, const csr_desc<int, double> h_csr_desc,
                     const csr_desc<int, double> d_csr_desc, const double *dx, double *dy) {
  go(active_strategy(), trans, alpha, beta, &h_csr_desc, d_csr_desc, dx, dy);
}

// src/acc/api/spmv_imp.cpp:10-18 (C++ linkage twin of the extern "C" export in c_api.cpp)
void sparse_spmv(int htrans, const double halpha, const double hbeta, int hm, int hn, const int *rowptr,
                 const int *colindex, const double *value, const double *x, double *y) {
  run_spmv(active_strategy(), htrans, halpha, hbeta, hm, hn, -1, nullptr, rowptr, colindex, value, x, y);
}

// hip/spmv_hip_acc_imp.cpp:29-35
void default_sparse_spmv(int trans, const double alpha, const double beta, const csr_desc<int, double> d_csr_desc,
                         const double *x, double *y) {
  go(kDefault, trans, alpha, beta, nullptr, d_csr_desc, x, y);
}

// hip-adaptive/adaptive.cpp:16-67
void adaptive_sparse_spmv(int trans, const double alpha, const double beta, const csr_desc<int, double> h_csr_desc,
                          const csr_desc<int, double> d_csr_desc, const double *x, double *y) {
  go(kAdaptive, trans, alpha, beta, &h_csr_desc, d_csr_desc, x, y);
}

// hip-flat/flat.cpp:47-57, 59-76, 84-131.  The reduce-width arguments of the reference (derived from the
// halves' nnz) are not needed: the tile kernel picks its lanes-per-row from each tile's own row count.
void flat_sparse_spmv(int trans, const double alpha, const double beta, const csr_desc<int, double> h_csr_desc,
                      const csr_desc<int, double> d_csr_desc, const double *x, double *y) {
  go(kFlat, trans, alpha, beta, &h_csr_desc, d_csr_desc, x, y);
}
void segment_sum_flat_sparse_spmv(int trans, const double alpha, const double beta,
                                  const csr_desc<int, double> h_csr_desc, const csr_desc<int, double> d_csr_desc,
                                  const double *x, double *y) {
  FlatSegmentSumScope scope; // same tiles and cut-row handling, rows reduced by the segmented scan over the tile
  go(kFlat, trans, alpha, beta, &h_csr_desc, d_csr_desc, x, y);
}
void adaptive_flat_sparse_spmv(const int, const int, int trans, const double alpha, const double beta,
                               const csr_desc<int, double> d_csr_desc, const double *x, double *y) {
  go(kFlat, trans, alpha, beta, nullptr, d_csr_desc, x, y);
}

// hip-line-enhance/line_enhance_spmv.cpp:8-21, 23-69
void line_enhance_sparse_spmv(int trans, const double alpha, const double beta, const csr_desc<int, double> d_csr_desc,
                              const double *x, double *y) {
  go(kLineEnhance, trans, alpha, beta, nullptr, d_csr_desc, x, y);
}
void adaptive_enhance_sparse_spmv(int trans, const double alpha, const double beta,
                                  const csr_desc<int, double> d_csr_desc, const double *x, double *y) {
  go(kLineEnhance, trans, alpha, beta, nullptr, d_csr_desc, x, y);
}

// hip-line/line_strategy.cpp:8-31, 52-77
void adaptive_line_sparse_spmv(int trans, const double alpha, const double beta, const csr_desc<int, double> d_csr_desc,
                               const double *x, double *y) {
  go(kLine, trans, alpha, beta, nullptr, d_csr_desc, x, y);
}
void line_sparse_spmv(int trans, const double alpha, const double beta, const csr_desc<int, double> d_csr_desc,
                      const double *x, double *y) {
  go(kLine, trans, alpha, beta, nullptr, d_csr_desc, x, y);
}

// hip-vector-row/vector_row.cpp:9-28, 30-38
void vec_row_sparse_spmv(int trans, const double alpha, const double beta, const csr_desc<int, double> d_csr_desc,
                         const double *x, double *y) {
  go(kVectorRow, trans, alpha, beta, nullptr, d_csr_desc, x, y);
}
void adaptive_vec_row_sparse_spmv(const int nnz_block_0, const int nnz_block_1, int trans, const double alpha,
                                  const double beta, const csr_desc<int, double> d_csr_desc, const double *x,
                                  double *y) {
  // the caller already knows the halves' nnz: build the samples the split needs without touching rowptr
  const int m = d_csr_desc.rows;
  // no plan and no engine call here, so the engine's word on the arguments is asked for directly: trans is reported, not applied
  if (!spmv_call_accepted(trans, m, d_csr_desc.cols, d_csr_desc.row_ptr, x, y)) return;
  if (d_csr_desc.nnz > 0 && (!d_csr_desc.col_index || !d_csr_desc.values)) {
    set_error(kErrBadArgument, "null colindex / value with nnz > 0");
    return;
  }
  CsrDev A;
  A.m = m;
  A.n = d_csr_desc.cols;
  A.nnz = d_csr_desc.nnz;
  A.rp = d_csr_desc.row_ptr;
  A.ci = d_csr_desc.col_index;
  A.v = d_csr_desc.values;
  // lanes per row for lanes that read an LDS tile: pow2 >= avg / 8, at least 2 (k_vector_row.hip; the reference's rule, which
  // sizes lanes that stream from global memory, is vector_row.cpp:15-27)
  auto vec_for = [](long long avg) {
    int w = 2;
    while (w < 64 && 8LL * w < avg) w <<= 1;
    return w;
  };
  const int half = m / 2;
  const int w0 = vec_for(half > 0 ? nnz_block_0 / half : 0);
  const int w1 = vec_for(nnz_block_1 / (m - half));
  // the two-width split on the tile machinery (k_vector_row.hip::vector_tile_kernel); no plan is involved: the caller passed
  // the only structural facts the split needs
  const double a0 = half > 0 ? static_cast<double>(nnz_block_0) / half : 0.0;
  const double a1 = static_cast<double>(nnz_block_1) / (m - half);
  launch_vector_tile(get_stream(), A, half, w0, w1, a0, a1, 1900, 16, kStreamPolicyNt, alpha, beta, x, y);
}

// legacy baselines kept resolvable
void thread_row_sparse_spmv(int trans, const double alpha, const double beta, const csr_desc<int, double> d_csr_desc,
                            const double *d_x, double *d_y) {
  go(kThreadRow, trans, alpha, beta, nullptr, d_csr_desc, d_x, d_y);
}
void wf_row_sparse_spmv(int htrans, const double halpha, const double hbeta, const csr_desc<int, double> d_csr_desc,
                        const double *hx, double *hy) {
  go(kWfRow, htrans, halpha, hbeta, nullptr, d_csr_desc, hx, hy);
}
void light_sparse_spmv(int trans, const double alpha, const double beta, const csr_desc<int, double> d_csr_desc,
                       const double *x, double *y) {
  go(kLight, trans, alpha, beta, nullptr, d_csr_desc, x, y);
}
void block_row_sparse_spmv(int trans, const double alpha, const double beta, const csr_desc<int, double> d_csr_desc,
                           const double *d_x, double *d_y) {
  go(kBlockRowOrdinary, trans, alpha, beta, nullptr, d_csr_desc, d_x, d_y);
}

// hip-csr-adaptive-plus/csr_adaptive_plus_spmv.cpp:132-168.  PROFILE fills the handle's three times
// (microseconds, :126-128).  Analysis results are cached in the plan, so from the second call on the
// analyze time is the cache lookup and destroy is a no-op (the reference re-analyses, re-uploads and
// frees on every call).
template <bool PROFILE, typename I, typename T>
void csr_adaptive_plus_sparse_spmv(SpMVAccHanele *handle, int trans, const T alpha, const T beta,
                                   const csr_desc<I, T> h_csr_desc, const csr_desc<I, T> d_csr_desc, const T *x, T *y) {
  if (!PROFILE || !handle) {
    go(kAdaptivePlus, trans, alpha, beta, &h_csr_desc, d_csr_desc, x, y);
    return;
  }
  hipStream_t st = get_stream();
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  (void)hipEventRecord(e0, st);
  go(kAdaptivePlus, trans, alpha, beta, &h_csr_desc, d_csr_desc, x, y);
  (void)hipEventRecord(e1, st);
  (void)hipEventSynchronize(e1);
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e0, e1);
  // the call that analysed (the first one on a matrix) reports its preparation -- analysis + per-matrix timings, host clock --
  // as analyze time and the rest of the event interval as kernel time; later calls find the plan and report 0
  const double prepared_us = last_prepare_us();
  const double total_us = 1000.0 * ms;
  handle->profile_analyze_time = prepared_us;
  handle->profile_kernel_time = prepared_us > 0.0 ? (total_us > prepared_us ? total_us - prepared_us : 0.0) : total_us;
  handle->profile_destroy_time = 0.0;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
}

template void csr_adaptive_plus_sparse_spmv<true, int, double>(SpMVAccHanele *, int, const double, const double,
                                                               const csr_desc<int, double>,
                                                               const csr_desc<int, double>, const double *, double *);
template void csr_adaptive_plus_sparse_spmv<false, int, double>(SpMVAccHanele *, int, const double, const double,
                                                                const csr_desc<int, double>,
                                                                const csr_desc<int, double>, const double *, double *);
