// Host-only call site of adaptive_vec_row_sparse_spmv (include/hip-vector-row/vector_row.h), built by tests/test_cxx_surface_host.py against
// libspmv_acc.so: the arguments the engine refuses for every other entry, handed to the one wrapper that launches without the engine.  Prints
// one line per call, "<name> <error word>".  Each call must come back with the engine's code before anything is handed to the HIP runtime, so
// the program runs on a machine without a GPU.  The non-null pointers are never dereferenced on the host; nothing here runs on a GPU.
#include <climits>
#include <cstdio>

#include "api/types.h"
#include "hip-vector-row/vector_row.h"

extern "C" {
int spmv_acc_last_error(void);
void spmv_acc_clear_error(void);
}

int main() {
  int *const rp = reinterpret_cast<int *>(0x1000);
  double *const d = reinterpret_cast<double *>(0x2000);
  auto report = [](const char *name) {
    std::printf("%s %d\n", name, spmv_acc_last_error());
    spmv_acc_clear_error();
  };
  spmv_acc_clear_error();
  adaptive_vec_row_sparse_spmv(2, 2, operation_none, 1.0, 1.0, csr_desc<int, double>(4, 4, 4, nullptr, rp, d), d, d);
  report("null_rowptr");
  adaptive_vec_row_sparse_spmv(2, 2, operation_none, 1.0, 1.0, csr_desc<int, double>(4, 4, 4, rp, rp, d), d, nullptr);
  report("null_y");
  adaptive_vec_row_sparse_spmv(2, 2, operation_none, 1.0, 1.0, csr_desc<int, double>(4, 4, 4, rp, rp, d), nullptr, d);
  report("null_x");
  adaptive_vec_row_sparse_spmv(2, 2, operation_none, 1.0, 1.0, csr_desc<int, double>(4, 4, 4, rp, nullptr, d), d, d);
  report("null_colindex");
  adaptive_vec_row_sparse_spmv(2, 2, operation_none, 1.0, 1.0, csr_desc<int, double>(INT_MAX - 65535, 4, 4, rp, rp, d), d, d);
  report("too_many_rows");
  adaptive_vec_row_sparse_spmv(0, 0, operation_transpose, 1.0, 1.0, csr_desc<int, double>(0, 4, 0, rp, rp, d), d, d);
  report("trans_without_rows");
  adaptive_vec_row_sparse_spmv(0, 0, operation_none, 1.0, 1.0, csr_desc<int, double>(0, 4, 0, nullptr, nullptr, nullptr), nullptr, nullptr);
  report("no_rows");
  return 0;
}
