// spmm.cpp -- one SpMM call: Y = alpha * A * X + beta * Y for k dense vectors (include/spmv_acc.h spmv_acc_csr_spmm, kernels in k_spmm.hip).
//
// The matrix's plan is the SpMV plan of the same arrays (get_plan, same key): one matrix used by both kinds of call has one plan, one stale-plan
// guard and one cross-stream order.  SpMM adds its own section to that plan (Plan::spmm: the long-row piece tables, from rowptr alone) and touches
// nothing else of it -- no timed choice, no settling, no rule twin, no zigzag counter, no tune-cache entry, nothing spmv_acc_query_plan* reports --
// and it reads the caller's colindex / values on every call (no plan-resident copy or encoding of caller data).  Its shape is a rule on (m, nnz,
// k, layout), so an SpMM is bitwise reproducible from its first call.
#include "engine_internal.hpp"
#include "entry_helpers.hpp"
#include "spmm.hpp"

namespace spmv_acc {

using namespace detail;

namespace {

constexpr int kSpmmRowMajor = 0; // SPMV_ACC_ROW_MAJOR (the engine does not include the C header)
constexpr int kSpmmColMajor = 1; // SPMV_ACC_COL_MAJOR

// The plan's SpMM section: the rows longer than kSpmmLongRow, cut into pieces of kSpmmPiece non-zeros, and the pieces' partial-sum scratch.
// Built once per plan from rowptr (the caller's host copy when it passes one, else one read of the device array); refused inside a capture.
bool ensure_spmm(Plan &p, const int *h_rowptr, hipStream_t st) {
  if (p.spmm_state >= 0) return true;
  if (!plan_work_allowed("the SpMM long-row tables")) return false;
  const int m = p.A.m;
  std::vector<int> copy;
  const int *rp = host_view(h_rowptr);
  if (!rp) {
    copy.resize(static_cast<size_t>(m) + 1);
    if (!hip_ok(hipMemcpyAsync(copy.data(), p.A.rp, sizeof(int) * copy.size(), hipMemcpyDeviceToHost, st), "read rowptr (SpMM)") ||
        !hip_ok(hipStreamSynchronize(st), "read rowptr (SpMM)"))
      return false;
    rp = copy.data();
  }
  std::vector<int> rows, first, piece;
  for (int r = 0; r < m; ++r) {
    const int b = rp[r], e = rp[r + 1];
    if (e - b <= kSpmmLongRow) continue;
    rows.push_back(r);
    first.push_back(static_cast<int>(piece.size() / 2));
    for (long long q = b; q < e; q += kSpmmPiece) {
      piece.push_back(static_cast<int>(q));
      piece.push_back(static_cast<int>(q + kSpmmPiece < e ? q + kSpmmPiece : e));
    }
  }
  if (rows.empty()) {
    p.spmm_state = 0;
    return true;
  }
  first.push_back(static_cast<int>(piece.size() / 2));
  SpmmLong &L = p.spmm;
  L.nlong = static_cast<int>(rows.size());
  L.npieces = static_cast<int>(piece.size() / 2);
  const bool ok =
      hip_ok(hipMalloc(reinterpret_cast<void **>(&L.rows), sizeof(int) * rows.size()), "hipMalloc SpMM rows") &&
      hip_ok(hipMalloc(reinterpret_cast<void **>(&L.first), sizeof(int) * first.size()), "hipMalloc SpMM pieces") &&
      hip_ok(hipMalloc(reinterpret_cast<void **>(&L.piece), sizeof(int) * piece.size()), "hipMalloc SpMM pieces") &&
      hip_ok(hipMalloc(reinterpret_cast<void **>(&L.partial), sizeof(double) * kSpmmPanel * static_cast<size_t>(L.npieces)), "hipMalloc SpMM partials") &&
      hip_ok(hipMemcpyAsync(L.rows, rows.data(), sizeof(int) * rows.size(), hipMemcpyHostToDevice, st), "upload SpMM rows") &&
      hip_ok(hipMemcpyAsync(L.first, first.data(), sizeof(int) * first.size(), hipMemcpyHostToDevice, st), "upload SpMM pieces") &&
      hip_ok(hipMemcpyAsync(L.piece, piece.data(), sizeof(int) * piece.size(), hipMemcpyHostToDevice, st), "upload SpMM pieces") &&
      hip_ok(hipStreamSynchronize(st), "upload SpMM tables"); // (the host vectors go out of scope)
  if (!ok) {
    p.free_spmm();
    return false;
  }
  p.spmm_state = 1;
  return true;
}

} // namespace

int run_spmm(int layout, int k, double alpha, double beta, int m, int n, int nnz, const int *h_rowptr, const int *d_rowptr, const int *d_colindex,
             const double *d_value, const double *dX, long long ldx, double *dY, long long ldy) {
  static const char *const kEntry = "spmv_acc_csr_spmm";
  clear_error();
  apply_env_tunables();
  if (layout != kSpmmRowMajor && layout != kSpmmColMajor) return entry_error(kEntry, kErrBadArgument, "layout must be SPMV_ACC_ROW_MAJOR or SPMV_ACC_COL_MAJOR");
  if (k < 0 || m < 0 || n < 0) return entry_error(kEntry, kErrBadArgument, "negative k, m or n");
  const bool row_major = layout == kSpmmRowMajor;
  if (row_major ? (ldx < k || ldy < k) : (ldx < n || ldy < m))
    return entry_error(kEntry, kErrBadArgument, row_major ? "row-major needs ldx >= k and ldy >= k" : "column-major needs ldx >= n and ldy >= m");
  if (k == 0 || m == 0) return kOk;
  if (!d_rowptr || !dY || (n > 0 && !dX)) return entry_error(kEntry, kErrBadArgument, "null rowptr / X / Y");
  if (nnz != 0 && n > 0 && (!d_colindex || !d_value)) return entry_error(kEntry, kErrBadArgument, "null colindex / value with nnz != 0");
  if (too_large(m)) return entry_error(kEntry, kErrTooLarge, "row count does not leave room for block arithmetic in int32; shard the matrix");

  // k == 1 with contiguous vectors (the two layouts coincide): the SpMV path under the active strategy, bitwise what spmv_acc_csr_spmv gives
  if (k == 1 && (!row_major || (ldx == 1 && ldy == 1))) {
    run_spmv(active_strategy(), 0, alpha, beta, m, n, nnz, h_rowptr, d_rowptr, d_colindex, d_value, dX, dY);
    return last_error_code_only();
  }
  hipStream_t st = t_stream;
  note_stream_use();
  t_capturing = stream_capturing(st);
  if (nnz == 0 || n == 0) {
    launch_spmm_scale(st, m, k, row_major, ldy, beta, dY);
  } else {
    const std::shared_ptr<Plan> p = get_plan(m, n, nnz, h_rowptr, d_rowptr, d_colindex, d_value);
    if (!p) return last_error_code_only() != kOk ? last_error_code_only() : entry_error(kEntry, kErrHip, "no plan");
    t_last_plan = p; // (spmv_acc_last_error reports a stale plan found by this call's kernels, as after an SpMV)
    std::lock_guard<std::mutex> plan_lock(p->mu);
    if (p->A.count() == 0) {
      launch_spmm_scale(st, m, k, row_major, ldy, beta, dY);
    } else {
      if (!ensure_spmm(*p, h_rowptr, st)) return last_error_code_only();
      // the plan's cross-stream order (run_spmv_call): a call on another stream than the plan's last one waits for that one's work
      if (p->launched && p->last_stream != st && !t_capturing) {
        if (!p->order_event && hipEventCreateWithFlags(&p->order_event, hipEventDisableTiming) != hipSuccess) p->order_event = nullptr;
        if (p->order_event && hipEventRecord(p->order_event, p->last_stream) == hipSuccess) (void)hipStreamWaitEvent(st, p->order_event, 0);
        (void)hipGetLastError();
      }
      p->last_stream = st;
      p->launched = true;
      CsrDev A = p->A;
      A.yin = nullptr;
      A.cold = nullptr;
      // one pass over the matrix per panel of kSpmmPanel columns (the last one narrower)
      for (int c0 = 0; c0 < k; c0 += kSpmmPanel) {
        const int kp = k - c0 < kSpmmPanel ? k - c0 : kSpmmPanel;
        const double *x = dX + (row_major ? c0 : c0 * ldx);
        double *y = dY + (row_major ? c0 : c0 * ldy);
        launch_spmm_rows(st, A, row_major, kp, ldx, ldy, alpha, beta, x, y);
        if (p->spmm_state == 1) launch_spmm_long(st, A, p->spmm, row_major, kp, ldx, ldy, alpha, beta, x, y);
      }
    }
  }
  const hipError_t launch_err = hipGetLastError();
  if (launch_err != hipSuccess && last_error_code_only() == kOk)
    set_error(kErrHip, std::string("spmv_acc_csr_spmm: kernel launch failed: ") + hipGetErrorString(launch_err));
  return last_error_code_only();
}

} // namespace spmv_acc
