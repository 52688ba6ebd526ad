// jacobi.cpp -- the two entries of the damped Jacobi / l1-Jacobi smoother (include/spmv_acc.h spmv_acc_csr_jacobi_diagonal,
// spmv_acc_csr_jacobi_sweep; kernels in k_jacobi.hip; the diagonals' definition, the sweep's summation order and the size rules in jacobi.hpp).
//
// Neither makes, finds or touches a plan, and nothing derived from the caller's arrays survives a call: the inverse diagonal belongs to the
// caller, who hands it back to the sweep.  Both are launch-only: the diagonal is one kernel (kind 0) or the roots' and one more (kind 1), the
// sweep one kernel for all rows; no allocation, no copy, no wait.
#include "jacobi.hpp"
#include "strength.hpp"
#include "engine_internal.hpp"
#include "entry_helpers.hpp"

#include <cmath>

namespace spmv_acc {

using namespace detail;

int run_csr_jacobi_diagonal(int m, int nnz, const int *d_rowptr, const int *d_colindex, const double *d_value, int kind, double *d_dinv,
                            double *d_work) {
  static const char *const kEntry = "spmv_acc_csr_jacobi_diagonal";
  clear_error();
  apply_env_tunables();
  if (m < 0 || nnz < 0) return entry_error(kEntry, kErrBadArgument, "negative m or nnz");
  if (kind < 0 || kind > 1) return entry_error(kEntry, kErrBadArgument, "kind is not 0 (Jacobi) or 1 (scaled l1)");
  if (m > 0 && (!d_rowptr || !d_dinv)) return entry_error(kEntry, kErrBadArgument, "null rowptr / dinv");
  if (m > 0 && nnz > 0 && (!d_colindex || !d_value)) return entry_error(kEntry, kErrBadArgument, "null colindex / value of a matrix with non-zeros");
  if (m > 0 && kind == 1 && !d_work) return entry_error(kEntry, kErrBadArgument, "null work, which the scaled l1 diagonal needs (m doubles)");
  if (too_large(m) || too_large(nnz))
    return entry_error(kEntry, kErrTooLarge, "m or nnz does not leave room for block arithmetic in int32");
  if (kind == 1 && m > kJacobiMaxRows)
    return entry_error(kEntry, kErrTooLarge, "more than 2^29 rows: the roots are gathered through 32-bit byte offsets");
  if (kind == 1 && overlap(d_work, m, d_dinv, m)) return entry_error(kEntry, kErrBadArgument, "work overlaps dinv");
  if (m == 0) return kOk; // no rows: nothing to launch
  hipStream_t st = t_stream;
  note_stream_use();
  if (kind == 0) {
    launch_jacobi_inverse(st, m, nnz, d_rowptr, d_colindex, d_value, d_dinv);
  } else {
    launch_strength_sd(st, m, nnz, d_rowptr, d_colindex, d_value, d_work);
    launch_jacobi_l1(st, m, nnz, d_rowptr, d_colindex, d_value, d_work, d_dinv);
  }
  return launch_error(kEntry);
}

int run_csr_jacobi_sweep(int m, int nnz, const int *d_rowptr, const int *d_colindex, const double *d_value, const double *d_dinv, double omega,
                         const double *d_b, const double *d_x_in, double *d_x_out, double *d_r_out) {
  static const char *const kEntry = "spmv_acc_csr_jacobi_sweep";
  clear_error();
  apply_env_tunables();
  if (m < 0 || nnz < 0) return entry_error(kEntry, kErrBadArgument, "negative m or nnz");
  if (!std::isfinite(omega)) return entry_error(kEntry, kErrBadArgument, "omega is not finite");
  if (m > 0 && (!d_rowptr || !d_dinv || !d_b)) return entry_error(kEntry, kErrBadArgument, "null rowptr / dinv / b");
  if (m > 0 && nnz > 0 && (!d_colindex || !d_value)) return entry_error(kEntry, kErrBadArgument, "null colindex / value of a matrix with non-zeros");
  if (m > 0 && !d_x_out && !d_r_out) return entry_error(kEntry, kErrBadArgument, "null x_out and r_out: nothing to write");
  if (too_large(m) || too_large(nnz))
    return entry_error(kEntry, kErrTooLarge, "m or nnz does not leave room for block arithmetic in int32");
  if (m > kJacobiMaxRows)
    return entry_error(kEntry, kErrTooLarge, "more than 2^29 rows: x_in is gathered through 32-bit byte offsets; sweep row blocks of the matrix");
  // out of place: in place the rows of one launch would race
  const double *const arrays[5] = {d_x_out, d_r_out, d_x_in, d_b, d_dinv};
  const char *const names[5] = {"x_out", "r_out", "x_in", "b", "dinv"};
  for (int a = 0; a < 5; ++a)
    for (int o = a + 1; o < 5; ++o)
      if (overlap(arrays[a], m, arrays[o], m))
        return entry_error(kEntry, kErrBadArgument, std::string(names[a]) + " overlaps " + names[o] + ": the sweep is out of place");
  if (m == 0) return kOk; // no rows: nothing to launch
  hipStream_t st = t_stream;
  note_stream_use();
  if (d_x_in) launch_jacobi_sweep(st, m, nnz, d_rowptr, d_colindex, d_value, d_dinv, omega, d_b, d_x_in, d_x_out, d_r_out);
  else launch_jacobi_start(st, m, d_dinv, omega, d_b, d_x_out, d_r_out); // the zero start: the matrix is not read
  return launch_error(kEntry);
}

} // namespace spmv_acc
