// surface_driver.cpp -- every entry of the C++ surface (include/api/spmv.h, include/spmv_acc_strategies.hpp) on every case and alpha / beta pair
// of tests/cxx_surface_cases.py, in ONE process: like api_driver.cpp it includes the headers at the reference's include paths and links
// libspmv_acc.so.  After each call it synchronises and writes y, the library's error word (cleared afterwards) and the kernel the matrix' plan
// recorded (spmv_acc_query_plan_last_kernel; -2 = no plan), all as doubles.  Call order: tests/cxx_surface_cases.py CALLS.  A second pass runs one
// case and pair with trans = 1.  A HIP call that fails ends the program at once with a non-zero status: nothing calls into the runtime after it.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "api/handle.h"
#include "api/spmv.h"
#include "api/types.h"
#include "hip-adaptive/adaptive.h"
#include "hip-block-row-ordinary/spmv_hip_acc_imp.h"
#include "hip-csr-adaptive-plus/csr_adaptive_plus_spmv.h"
#include "hip-flat/spmv_hip_acc_imp.h"
#include "hip-light/spmv_hip_acc_imp.h"
#include "hip-line-enhance/line_enhance_spmv.h"
#include "hip-line/line_strategy.h"
#include "hip-thread-row/thread_row.h"
#include "hip-vector-row/vector_row.h"
#include "hip-wf-row/spmv_hip.h"
#include "hip/spmv_hip_acc_imp.h"

// (spmv_acc.h is not included: it would make `sparse_spmv` the C-linkage twin, and this program is about the C++-linkage one)
extern "C" {
int spmv_acc_last_error(void);
void spmv_acc_clear_error(void);
int spmv_acc_query_plan_last_kernel(const int *d_rowptr, int m);
void spmv_acc_release_plans(const int *d_rowptr);
}

namespace {
bool ok(hipError_t e, const char *what) {
  if (e == hipSuccess) return true;
  std::fprintf(stderr, "surface_driver: %s: %s\n", what, hipGetErrorString(e));
  return false;
}
template <typename T> bool get(FILE *f, T *p, size_t count) { return std::fread(p, sizeof(T), count, f) == count; }

struct Case {
  int m = 0, n = 0, nnz = 0;
  std::vector<int> rp, ci;
  std::vector<double> v, x, y0;
};

struct Device {
  var_csr_desc<int, double> csr;
  double *x = nullptr, *y = nullptr;
  ~Device() { // (never reached after a failed HIP call: main leaves through give_up)
    (void)hipFree(csr.row_ptr);
    (void)hipFree(csr.col_index);
    (void)hipFree(csr.values);
    (void)hipFree(x);
    (void)hipFree(y);
  }
};
template <typename T> bool upload(T **d, const std::vector<T> &h) {
  *d = nullptr;
  if (h.empty()) return true; // an empty array stays a null pointer: `no_entries` has no colindex / value at all
  return ok(hipMalloc(reinterpret_cast<void **>(d), sizeof(T) * h.size()), "hipMalloc") &&
         ok(hipMemcpy(*d, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice), "upload");
}

// every entry on one (case, pair); false after a failed HIP call
bool run_all(const Case &c, var_csr_desc<int, double> &h, Device &D, int trans, double alpha, double beta, FILE *out) {
  const int m = c.m, n = c.n, nnz = c.nnz;
  std::vector<double> y_start = c.y0, y(m);
  if (beta == 0.0) y_start.assign(m, std::numeric_limits<double>::quiet_NaN()); // beta == 0 never reads y
  bool fine = true;
  auto call = [&](auto &&entry) {
    if (!fine) return;
    fine = ok(hipMemcpy(D.y, y_start.data(), sizeof(double) * m, hipMemcpyHostToDevice), "reset y");
    if (!fine) return;
    entry();
    fine = ok(hipDeviceSynchronize(), "synchronise after an entry") &&
           ok(hipMemcpy(y.data(), D.y, sizeof(double) * m, hipMemcpyDeviceToHost), "read y");
    if (!fine) return;
    const double err = spmv_acc_last_error();
    spmv_acc_clear_error();
    const double kernel = spmv_acc_query_plan_last_kernel(D.csr.row_ptr, m);
    std::fwrite(y.data(), sizeof(double), m, out);
    std::fwrite(&err, sizeof(double), 1, out);
    std::fwrite(&kernel, sizeof(double), 1, out);
  };
  const csr_desc<int, double> hc = h.as_const(), dc = D.csr.as_const();
  const double *dx = D.x;
  double *dy = D.y;
  const int first = c.rp[m / 2], second = nnz - c.rp[m / 2];
  const int hints[5][2] = {{first, second}, {0, 0}, {nnz, 0}, {0, nnz}, {INT_MAX, 1}};
  // first on the fresh matrix: the hand-launched split makes no plan
  for (const auto &hint : hints) call([&] { adaptive_vec_row_sparse_spmv(hint[0], hint[1], trans, alpha, beta, dc, dx, dy); });
  call([&] { sparse_csr_spmv(trans, alpha, beta, hc, dc, dx, dy); });
  call([&] { sparse_spmv(trans, alpha, beta, m, n, D.csr.row_ptr, D.csr.col_index, D.csr.values, dx, dy); });
  call([&] { default_sparse_spmv(trans, alpha, beta, dc, dx, dy); });
  call([&] { adaptive_sparse_spmv(trans, alpha, beta, hc, dc, dx, dy); });
  call([&] { flat_sparse_spmv(trans, alpha, beta, hc, dc, dx, dy); });
  call([&] { segment_sum_flat_sparse_spmv(trans, alpha, beta, hc, dc, dx, dy); });
  for (const auto &hint : hints) call([&] { adaptive_flat_sparse_spmv(hint[0], hint[1], trans, alpha, beta, dc, dx, dy); });
  call([&] { line_enhance_sparse_spmv(trans, alpha, beta, dc, dx, dy); });
  call([&] { adaptive_enhance_sparse_spmv(trans, alpha, beta, dc, dx, dy); });
  call([&] { adaptive_line_sparse_spmv(trans, alpha, beta, dc, dx, dy); });
  call([&] { line_sparse_spmv(trans, alpha, beta, dc, dx, dy); });
  call([&] { vec_row_sparse_spmv(trans, alpha, beta, dc, dx, dy); });
  call([&] { thread_row_sparse_spmv(trans, alpha, beta, dc, dx, dy); });
  call([&] { wf_row_sparse_spmv(trans, alpha, beta, dc, dx, dy); });
  call([&] { light_sparse_spmv(trans, alpha, beta, dc, dx, dy); });
  call([&] { block_row_sparse_spmv(trans, alpha, beta, dc, dx, dy); });
  SpMVAccHanele handle;
  call([&] { csr_adaptive_plus_sparse_spmv<true, int, double>(&handle, trans, alpha, beta, hc, dc, dx, dy); });
  call([&] { csr_adaptive_plus_sparse_spmv<false, int, double>(nullptr, trans, alpha, beta, hc, dc, dx, dy); });
  // once more with a plan in place: the hand-launched split leaves its record alone
  call([&] { adaptive_vec_row_sparse_spmv(first, second, trans, alpha, beta, dc, dx, dy); });
  // the next pair (or the next case, whose arrays may get the same addresses) starts without a plan
  if (fine) spmv_acc_release_plans(D.csr.row_ptr);
  return fine;
}
// after a failed HIP call: out at once, past every destructor that would call into the runtime again
[[noreturn]] void give_up() {
  std::fflush(stderr);
  std::_Exit(10);
}
} // namespace

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  int hdr[5];
  if (!get(f, hdr, 5) || hdr[0] != 0x43585853 || hdr[1] <= 0 || hdr[2] <= 0 || hdr[3] < 0 || hdr[3] >= hdr[1] || hdr[4] < 0 || hdr[4] >= hdr[2]) return 4;
  const int ncases = hdr[1], npairs = hdr[2];
  std::vector<double> pairs(2 * npairs);
  if (!get(f, pairs.data(), pairs.size())) return 4;
  std::vector<Case> cases(ncases);
  for (Case &c : cases) {
    int shape[3];
    if (!get(f, shape, 3) || shape[0] <= 0 || shape[1] <= 0 || shape[2] < 0) return 4;
    c.m = shape[0], c.n = shape[1], c.nnz = shape[2];
    c.rp.resize(c.m + 1), c.ci.resize(c.nnz), c.v.resize(c.nnz), c.x.resize(c.n), c.y0.resize(c.m);
    if (!get(f, c.rp.data(), c.rp.size()) || !get(f, c.ci.data(), c.ci.size()) || !get(f, c.v.data(), c.v.size()) ||
        !get(f, c.x.data(), c.x.size()) || !get(f, c.y0.data(), c.y0.size()))
      return 4;
    // the arrays are about to be handed to kernels: refuse a file whose structure is not a CSR matrix
    if (c.rp[0] != 0 || c.rp[c.m] != c.nnz) return 4;
    for (int i = 0; i < c.m; ++i)
      if (c.rp[i] > c.rp[i + 1]) return 4;
    for (int col : c.ci)
      if (col < 0 || col >= c.n) return 4;
  }
  std::fclose(f);
  FILE *out = std::fopen(argv[2], "wb");
  if (!out) return 3;
  if (!ok(hipSetDevice(0), "hipSetDevice")) give_up();

  for (int pass = 0; pass < 2; ++pass) { // 0: every case and pair; 1: one case and pair with trans = 1
    for (int k = pass == 0 ? 0 : hdr[3]; k < (pass == 0 ? ncases : hdr[3] + 1); ++k) {
      Case &c = cases[k];
      var_csr_desc<int, double> h;
      Device D;
      h.rows = D.csr.rows = c.m;
      h.cols = D.csr.cols = c.n;
      h.nnz = D.csr.nnz = c.nnz;
      h.row_ptr = c.rp.data();
      h.col_index = c.ci.data();
      h.values = c.v.data();
      if (!upload(&D.csr.row_ptr, c.rp) || !upload(&D.csr.col_index, c.ci) || !upload(&D.csr.values, c.v) || !upload(&D.x, c.x) ||
          !upload(&D.y, c.y0))
        give_up();
      for (int p = pass == 0 ? 0 : hdr[4]; p < (pass == 0 ? npairs : hdr[4] + 1); ++p)
        if (!run_all(c, h, D, pass == 0 ? operation_none : operation_transpose, pairs[2 * p], pairs[2 * p + 1], out)) give_up();
    }
  }
  return std::fclose(out) == 0 ? 0 : 3;
}
