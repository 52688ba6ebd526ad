/*
 * spmv_acc.h -- C ABI of the MI355X-native CSR SpMV engine (libspmv_acc.so).
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ or torch types.  Every entry point
 * names the reference interface (hpcde/spmv-acc, paths relative to the reference root) it replaces.
 * All matrix / vector pointers are DEVICE pointers (hipMalloc) unless a parameter says "host".
 * fp64 values, int32 indices, y = alpha*A*x + beta*y for any alpha, beta (src/acc/api/spmv.h:13-18).
 *
 * Calls are asynchronous: kernels are enqueued on the library stream (NULL stream unless
 * spmv_acc_set_stream was called) and the function returns; the caller synchronises
 * (as cli/main.cpp:104,111 does with hipDeviceSynchronize).  The reference API returns void and
 * checks nothing; errors here are reported out of band through spmv_acc_last_error().
 */
#ifndef SPMV_ACC_C_ABI_H
#define SPMV_ACC_C_ABI_H

#include <stddef.h> /* size_t (spmv_acc_cg_partials) */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- KERNEL_STRATEGY plugin surface ------------------------------------------------------------
 * replaces: the compile-time switch -DKERNEL_STRATEGY=<name> (config.cmake:15,
 * src/configure.cmake:17-40, src/building_config.h.in:24-34, src/acc/strategy_picker.cpp:19-65).
 * The build-time macro KERNEL_STRATEGY_<NAME> still selects the default; the environment variable
 * SPMV_ACC_KERNEL_STRATEGY and spmv_acc_set_strategy() override it at run time so one binary serves
 * every configuration.  Names are matched like the reference's CMake regex: case-insensitive
 * substring, "line_enhance" tested before "line". */
enum spmv_acc_strategy {
  SPMV_ACC_DEFAULT = 0,
  SPMV_ACC_ADAPTIVE = 1,
  SPMV_ACC_THREAD_ROW = 2,
  SPMV_ACC_WF_ROW = 3,
  SPMV_ACC_BLOCK_ROW_ORDINARY = 4,
  SPMV_ACC_LIGHT = 5,
  SPMV_ACC_VECTOR_ROW = 6,
  SPMV_ACC_LINE_ENHANCE = 7,
  SPMV_ACC_LINE = 8,
  SPMV_ACC_FLAT = 9,
  SPMV_ACC_ADAPTIVE_PLUS = 10 /* benchmark-only entry of the reference (benchmark_spmv_acc.hpp:186-200) */
};
int spmv_acc_set_strategy(const char *name); /* 0 on success, -1 unknown name */
int spmv_acc_set_strategy_id(int strategy);
int spmv_acc_get_strategy(void);
const char *spmv_acc_strategy_name(int strategy);
int spmv_acc_parse_strategy(const char *name); /* -1 if no match */

/* ---- primary entry -------------------------------------------------------------------------------
 * replaces: void sparse_spmv(int htrans, const double halpha, const double hbeta, int hm, int hn,
 *           const int *rowptr, const int *colindex, const double *value, const double *x, double *y)
 *           -- src/acc/api/spmv.h:27-28, src/acc/api/spmv_imp.cpp:10-18 (C++ linkage there; the same
 *           ten arguments with C linkage here).
 * The reference reads rowptr[hm] on the HOST (spmv_imp.cpp:14), which needs host-visible device
 * memory; here nnz and the strategy pickers' rowptr samples are fetched from the device once per
 * matrix and cached, so plain hipMalloc memory works.
 * (A C++ translation unit that has already included api/spmv.h sees that header's C++-linkage declaration;
 * the library exports both symbols, one name cannot carry two linkages in one TU.) */
#ifndef SPMV_ACC_AMD_API_SPMV_H
void sparse_spmv(int htrans, const double halpha, const double hbeta, int hm, int hn, const int *rowptr,
                 const int *colindex, const double *value, const double *x, double *y);
#endif

/* ---- descriptor entry, flattened to C --------------------------------------------------------------
 * replaces: void sparse_csr_spmv(int trans, const double alpha, const double beta,
 *           const csr_desc<int,double> h_csr_desc, const csr_desc<int,double> d_csr_desc,
 *           const double *dx, double *dy) -- src/acc/api/spmv.h:20-21, strategy_picker.cpp:19-65
 *           (the entry spmv-cli calls, cli/main.cpp:102,110,117).
 * h_rowptr: HOST copy of rowptr or NULL.  nnz: number of non-zeros, or -1 to read rowptr[m]. */
void spmv_acc_csr_spmv(int trans, double alpha, double beta, int m, int n, int nnz, const int *h_rowptr,
                       const int *d_rowptr, const int *d_colindex, const double *d_value, const double *dx,
                       double *dy);

/* ---- per-strategy entry ------------------------------------------------------------------------------
 * replaces: the L1 wrappers the benchmark harness calls directly (benchmark/benchmark_spmv_acc.hpp:27-200):
 *   default_sparse_spmv (hip/spmv_hip_acc_imp.cpp:29), adaptive_sparse_spmv (hip-adaptive/adaptive.cpp:16),
 *   flat_sparse_spmv (hip-flat/flat.cpp:47), line_enhance_sparse_spmv / adaptive_enhance_sparse_spmv
 *   (hip-line-enhance/line_enhance_spmv.cpp:8,23), adaptive_line_sparse_spmv (hip-line/line_strategy.cpp:52),
 *   vec_row_sparse_spmv (hip-vector-row/vector_row.cpp:9), csr_adaptive_plus_sparse_spmv
 *   (hip-csr-adaptive-plus/csr_adaptive_plus_spmv.cpp:132), ... selected by `strategy`. */
void spmv_acc_csr_spmv_strategy(int strategy, int trans, double alpha, double beta, int m, int n, int nnz,
                                const int *h_rowptr, const int *d_rowptr, const int *d_colindex,
                                const double *d_value, const double *dx, double *dy);

/* ---- out-of-place form (new) ---------------------------------------------------------------------------
 *     y_out = alpha * A * x + beta * y_in
 * replaces: nothing callable in the reference -- every entry there updates y in place (api/spmv.h:13-18), and its drivers
 * re-upload y0 before each call (cli/main.cpp:101,116).  A caller that keeps both vectors (x_{k+1} = f(y_k) iterations, the
 * row-sharded step below: old slice in one buffer, new slice inside the gathered vector) would otherwise copy y once per SpMV
 * (2 x 8 B per row; 61 of 218 us per sharded step on the headline matrix).  Same kernels, same sums: bit-identical to the
 * in-place entry on a copy of y_in.  strategy < 0: the active strategy.  dy_in may be NULL or equal to dy_out (in place);
 * the two vectors must not overlap partially (SPMV_ACC_ERR_BAD_ARGUMENT); dy_in is not read when beta == 0. */
void spmv_acc_csr_spmv_oop(int strategy, int trans, double alpha, double beta, int m, int n, int nnz, const int *h_rowptr,
                           const int *d_rowptr, const int *d_colindex, const double *d_value, const double *dx,
                           const double *dy_in, double *dy_out);

/* ---- CSR SpMM: one matrix, k vectors (new) --------------------------------------------------------------------------------
 * replaces: nothing in the reference (it has no multi-vector product; its callers make k SpMV calls, each re-reading the matrix).
 * Y = alpha * A * X + beta * Y for k dense vectors, one pass over the matrix per panel of up to 32 columns.
 *   Row-major:    X[i * ldx + j] (i < n, j < k, ldx >= k),  Y[r * ldy + j] (ldy >= k).
 *   Column-major: X[j * ldx + i] (ldx >= n),                Y[j * ldy + r] (ldy >= m).
 * Offsets are 64-bit; X and Y may be views that are only 8-B aligned (odd ld, a column slice).  X and Y must not overlap (not
 * detected).  Asynchronous on the calling thread's library stream; h_rowptr optional, as for spmv_acc_csr_spmv.
 * k == 0 or m == 0: nothing, returns SPMV_ACC_OK.  nnz == 0 or n == 0: Y = beta * Y.  beta == 0: Y is never read (NaNs in it do not
 * propagate).  Only the first k entries of each Y row (row-major) / column (column-major) are written; the padding up to ldy is not
 * touched.  A bad layout, k < 0, an ld below its minimum or a null pointer where data is needed: SPMV_ACC_ERR_BAD_ARGUMENT, nothing
 * is launched.  KERNEL_STRATEGY does not apply (one kernel family), except that k == 1 with contiguous vectors is served by the
 * SpMV path under the active strategy: bitwise what spmv_acc_csr_spmv gives.  The matrix shares its plan with SpMV calls; the first
 * uncaptured SpMM call on a matrix builds the plan's SpMM tables (from rowptr), later calls only launch and may be captured.
 * Returns 0 or an spmv_acc_error code (also left in spmv_acc_last_error). */
enum spmv_acc_layout { SPMV_ACC_ROW_MAJOR = 0, SPMV_ACC_COL_MAJOR = 1 };
int spmv_acc_csr_spmm(int layout, int k, double alpha, double beta, int m, int n, int nnz, const int *h_rowptr,
                      const int *d_rowptr, const int *d_colindex, const double *d_value,
                      const double *dX, long long ldx, double *dY, long long ldy);

/* ---- the transposed product, 1: a stable device transpose into caller-owned arrays (new) -------------------------------------------
 * replaces: nothing in the reference; it never reads `trans`, api/spmv.h:13.  (The `trans` argument of every other entry keeps its
 * behaviour: a non-zero value is reported as SPMV_ACC_ERR_UNSUPPORTED_TRANS and the non-transposed product is computed.)
 * Writes the CSR of A^T (the CSC of A) for the m x n matrix A: d_t_rowptr (n + 1 ints), d_t_colindex (nnz ints: the source ROW of each
 * entry), d_t_value (nnz doubles) and, where d_perm is not NULL, d_perm (nnz ints: the source position q of output entry p).  d_value and
 * d_t_value may both be NULL: structure only.  The caller owns the outputs and runs ANY entry of this library on them as an n x m matrix
 * -- every strategy, spmv_acc_prepare, the SpMM entry, the shards -- so the whole tuned engine serves y = alpha * A^T * x + beta * y.
 * STABLE and deterministic: inside output row c the entries appear in ascending source position, so the outputs are a pure function of
 * the inputs, bit for bit a host stable argsort of colindex (one radix sort of the (column, position) pairs; no float is added).
 * nnz < 0: rowptr[m] is read from the device.  The matrix must be rebased (rowptr[0] == 0; else SPMV_ACC_ERR_BAD_ARGUMENT), and a given
 * nnz must be rowptr[m].  m == 0, n == 0 or nnz == 0: d_t_rowptr is set to zeros, nothing else is written.  A column outside [0, n) is
 * never turned into an address: the columns are counted first, and if one is out of range nothing is written and
 * SPMV_ACC_ERR_BAD_ARGUMENT is returned.  Null pointers where data is needed, negative m or n: SPMV_ACC_ERR_BAD_ARGUMENT, nothing is
 * launched; m, n or nnz beyond int32 block arithmetic: SPMV_ACC_ERR_TOO_LARGE.
 * Runs on the calling thread's library stream and has finished when it returns (it allocates about 8 B per non-zero of workspace -- 12 B
 * without d_perm -- plus the sort's scratch, synchronises, and frees all of it, on the error paths too).  Inside a stream capture it
 * enqueues nothing and returns SPMV_ACC_ERR_BAD_ARGUMENT.  Makes and touches no plan.  After an in-place edit of `value` the next entry
 * refreshes d_t_value; after a change of structure transpose again (and release the plans of the old transposed arrays).
 * Cost and when to use it: see the third entry below.  Returns 0 or an spmv_acc_error code (also left in spmv_acc_last_error). */
int spmv_acc_csr_transpose(int m, int n, int nnz, const int *d_rowptr, const int *d_colindex, const double *d_value,
                           int *d_t_rowptr, int *d_t_colindex, double *d_t_value, int *d_perm);

/* ---- the transposed product, 2: values changed in place (new) ------------------------------------------------------------------------
 * replaces: nothing in the reference.  d_t_value[p] = d_value[d_perm[p]] for p < nnz, with the d_perm an earlier transpose of the same
 * structure returned: the structure is transposed once, the values follow at the cost of one gather pass.  One kernel on the calling
 * thread's library stream: asynchronous, no allocation, may be captured.  The explicit, caller-driven counterpart of
 * spmv_acc_refresh_values (no plan holds a copy of the caller's values on this route).  An entry of d_perm outside [0, nnz) is skipped.
 * Returns 0 or an spmv_acc_error code. */
int spmv_acc_csr_transpose_values(int nnz, const int *d_perm, const double *d_value, double *d_t_value);

/* ---- the transposed product, 3: y = alpha * A^T * x + beta * y straight from the caller's CSR (new) -----------------------------------
 * replaces: nothing in the reference; it never reads `trans`, api/spmv.h:13.  dx holds m doubles, dy holds n.  For callers who cannot
 * afford a second copy of the matrix, or who use A^T once.  STATELESS: no plan, no cache entry, no timing; nothing derived from the
 * caller's arrays survives the call.  So it is launches only from its FIRST call on a matrix and may always be captured into a hipGraph
 * (nnz < 0 reads rowptr[m] from the device and is refused inside a capture).  Two launches on the calling thread's library stream:
 * y = beta * y (beta == 0: y is written and never read, NaNs in it do not propagate; beta == 1: skipped), then one pass over the
 * non-zeros in storage order that adds alpha * a * x[row] to y[col] with fp64 hardware atomic adds.  alpha == 0 or nnz == 0: the first
 * launch only.  The non-zero stream is cut into fixed tiles, so the time does not depend on how the rows are distributed.
 * THE ONE ENTRY WHOSE SUMS DEPEND ON ARRIVAL ORDER: two calls on the same data may differ in the last bits of y (the error stays within
 * the usual bound relative to |alpha| * sum |a| |x| + |beta y|).  With tunable "deterministic" = 1 it enqueues nothing and returns
 * SPMV_ACC_ERR_BAD_ARGUMENT: use spmv_acc_csr_transpose and the ordinary product on its result, which is bitwise reproducible.
 * d_rowptr may be an un-rebased row sub-range (rowptr + r0 with the whole colindex / value arrays and nnz = the END offset
 * rowptr[r0 + m], the convention of the shards): a rank then gets its partial A_local^T * x_local.  Every column is checked in the kernel
 * and one outside [0, n) is dropped (here it would be a WRITE outside y).  x and y must not overlap (not detected), and y must be
 * ordinary device memory (hipMalloc): the hardware adds are not defined on fine-grained host-coherent allocations.
 * Returns 0 or an spmv_acc_error code (also left in spmv_acc_last_error).
 * COST, as measured (MI355X, tools/transpose_bench.py, profiles/transpose_bench.md): the pass runs at the rate the chip ADDS, not at the
 * rate it streams.  Headline stand-in (40.45 M non-zeros, settled SpMV 0.14 ms): 0.92 ms = 0.35 TB/s of added bytes, 6.3 x a settled SpMV on
 * the transposed copy (8 B per non-zero at the 1.3 TB/s the hardware reaches at its best access shape would be 0.25 ms; this column
 * pattern reaches a quarter of that).  FEM class (28.2 M): 0.48 ms, 0.47 TB/s, 9.7 x.  Power-law columns (R-MAT 22, 65.2 M): 7.9 ms,
 * 0.07 TB/s, 16 x -- every lane of an add lands on another line.  The device transpose costs 2.6 / 1.8 / 5.1 ms on the three (18 / 37 / 11
 * SpMVs), so TRANSPOSE ONCE when A^T is used more than about four times (FEM, headline class) and always on power-law columns; keep this
 * entry for one or two products and for matrices whose second copy does not fit. */
int spmv_acc_csr_spmv_t(double alpha, double beta, int m, int n, int nnz, const int *d_rowptr, const int *d_colindex,
                        const double *d_value, const double *dx, double *dy);

/* ---- assembly, 1: a CSR from unsorted (row, col, value) triples with duplicates, into caller-owned arrays (new) ----------------------
 * replaces: nothing in the reference; it reads a finished matrix from a file on the host (and its reader keeps duplicates apart).
 * For callers who BUILD their matrix on the device -- finite-element assembly: a long unsorted list of triples with many duplicates per
 * position, rebuilt on the same pattern at every time step or Newton iteration.  The m x n CSR this writes is clean: rows sorted by
 * column, no duplicates, int32 -- every tuned path of the library then sees the matrix in its best form.
 * Input: nnz_coo triples (d_row, d_col, d_val) in any order, any number of duplicates.  Outputs, all owned by the caller and sized by the
 * upper bound nnz_coo: d_rowptr (m + 1 ints), d_colindex (nnz_coo ints), d_value (nnz_coo doubles), the map d_order (nnz_coo ints) and
 * d_start (nnz_coo + 1 ints), and *h_nnz (a host int): the number of distinct positions = the CSR's nnz.  Only the first *h_nnz entries of
 * d_colindex and d_value and the first *h_nnz + 1 of d_start are written.  d_val and d_value may both be NULL (structure only); d_order
 * and d_start may both be NULL (the map then lives in the workspace and is dropped); one of a pair without the other is
 * SPMV_ACC_ERR_BAD_ARGUMENT.
 * A PURE FUNCTION of the inputs: the triples are ordered by (row, col, input position) with one stable radix sort, d_order[p] = the input
 * position of the p-th triple in that order; triples with the same (row, col) form a run, run j = positions [d_start[j], d_start[j + 1])
 * of d_order = CSR entry j, so inside a row the columns ascend strictly.  d_value[j] = the sum of the run's values in ascending input
 * position, starting from its first value (not from 0.0): runs of up to 64 triples are added by one lane, bitwise a host loop in that
 * order; longer ones by a wavefront -- lane l adds the values l, l + 64, ... in order, then the 64 partial sums are combined as a balanced
 * tree over neighbouring lanes (spmv_acc_amd/csrc/coo.hpp states the order in full) -- so that one position hit 10^5 times does not
 * serialise on a lane.  No atomics: two calls on the same input give the same bits, and tunable "deterministic" changes nothing.
 * Rows outside [0, m) and columns outside [0, n) are counted before anything is written: if there are any, nothing is written, the
 * return is SPMV_ACC_ERR_BAD_ARGUMENT and the error string holds their number; a bad index is never turned into an address.
 * nnz_coo == 0: d_rowptr is set to zeros, *h_nnz = 0, nothing else is touched.  nnz_coo > 0 with m == 0 or n == 0, negative sizes, null
 * pointers where data is needed: SPMV_ACC_ERR_BAD_ARGUMENT, nothing is launched; m, n or nnz_coo beyond int32 block arithmetic:
 * SPMV_ACC_ERR_TOO_LARGE.
 * Runs on the calling thread's library stream and has finished when it returns (it allocates about 16 B per triple of workspace -- 24 B
 * without the map -- plus the sort's scratch, synchronises, and frees all of it, on the error paths too).  Inside a stream capture it
 * enqueues nothing and returns SPMV_ACC_ERR_BAD_ARGUMENT.  Makes and touches no plan: hand the CSR to spmv_acc_prepare or any product
 * entry afterwards.  Returns 0 or an spmv_acc_error code (also left in spmv_acc_last_error). */
int spmv_acc_coo_to_csr(int m, int n, int nnz_coo,
                        const int *d_row, const int *d_col, const double *d_val,
                        int *d_rowptr, int *d_colindex, double *d_value,
                        int *d_order, int *d_start, int *h_nnz);

/* ---- assembly, 2: new values on a known pattern (new; the per-step hot path) -----------------------------------------------------------
 * replaces: nothing in the reference.  d_value[j] = the sum over p in [d_start[j], d_start[j + 1]) of d_val[d_order[p]] for j < nnz, with
 * the map (d_order, d_start) and nnz = *h_nnz an earlier spmv_acc_coo_to_csr on the same (row, col) list returned.  The summation orders
 * are exactly those of the first entry (which runs this kernel for its own values), so re-assembling the same d_val repeats its bits.
 * One kernel on the calling thread's library stream: asynchronous, no allocation, may be captured into a hipGraph.  The map is the
 * caller's array here: an entry of d_order outside [0, nnz_coo) is skipped (it counts as +0.0), a d_start interval that reaches outside
 * [0, nnz_coo] is clamped, and nothing outside the caller's arrays is read or written.  nnz > nnz_coo or a null pointer with nnz > 0:
 * SPMV_ACC_ERR_BAD_ARGUMENT; nnz == 0: nothing.  The explicit, caller-driven counterpart of spmv_acc_refresh_values (no plan holds a copy
 * of the caller's values on this route); if a plan does hold a copy of the CSR values the caller rewrites through this entry,
 * spmv_acc_refresh_values applies as after any in-place edit.  Returns 0 or an spmv_acc_error code.
 * COST, as measured (MI355X, tools/coo_bench.py, profiles/coo_bench.md; triples = every entry of the stand-in as 1 ... 4 duplicates,
 * shuffled; the box copied at 6.33 TB/s in the same run): the pass needs 12 B per triple (order + the gathered value) and 12 B per entry
 * (start + value).  Headline stand-in (101.1 M triples -> 40.45 M entries, settled SpMV 0.143 ms): 2.11 ms = 0.81 TB/s of needed bytes,
 * 14.8 SpMVs.  FEM class (70.5 M -> 28.2 M, SpMV 0.050 ms): 1.53 ms, 0.77 TB/s, 31 SpMVs.  That is the rate of the memory system, not of
 * the kernel: after a shuffle every 8-B gather is a 128-B request of its own, and 101.1 M x 128 B / 2.11 ms = 6.1 TB/s is what the box
 * copies at.  The same pass on triples in the CSR's storage order (contiguous gathers) takes 0.75 / 0.52 ms (2.26 TB/s): a caller who can
 * emit the triples in a roughly sorted order gets that.  The first entry takes 9.9 / 6.3 ms (70 / 128 SpMVs: once per pattern);
 * torch.sparse_coo_tensor(...).coalesce() on the same triples takes 34.3 / 23.5 ms for structure and values together, and is the only
 * form torch offers per step -- the values pass is 16 x / 15 x faster than it. */
int spmv_acc_coo_to_csr_values(int nnz_coo, int nnz, const int *d_order, const int *d_start,
                               const double *d_val, double *d_value);

/* ---- sparse product C = A * B, 1: the number of scalar products (new) -----------------------------------------------------------------
 * replaces: nothing in the reference; it multiplies a matrix by a vector.
 * A is m x k, B is k x n, both CSR, int32, fp64 and rebased (rowptr[0] == 0); rows need NOT be sorted and an input may hold duplicate
 * positions, which act as separate entries.  *h_nprod (a host 64-bit integer) = the number of scalar products a_ik * b_kj = the sum over
 * A's non-zeros of the length of B's row a_colindex[q] = the size of the expansion = the upper bound on nnz(C) by which the caller sizes
 * the arrays of the next entry.  One range census of A's columns, one count pass and one reduction on the calling thread's library stream;
 * synchronises; inside a stream capture it enqueues nothing and returns SPMV_ACC_ERR_BAD_ARGUMENT.  nnz_a < 0: a_rowptr[m] is read from
 * the device; a given nnz_a must be a_rowptr[m].  A column of A outside [0, k) is never turned into an address: SPMV_ACC_ERR_BAD_ARGUMENT
 * with their number in the error string.  A count beyond INT_MAX - 2^16 is still returned in *h_nprod, with SPMV_ACC_ERR_TOO_LARGE: the
 * next entry cannot take it; rows of C are independent, so multiply row ranges of A.  Makes and touches no plan. */
int spmv_acc_csr_spgemm_products(int m, int k, int nnz_a, const int *d_a_rowptr, const int *d_a_colindex,
                                 const int *d_b_rowptr, long long *h_nprod);

/* ---- sparse product C = A * B, 2: structure, map and first values, into caller-owned arrays (new) --------------------------------------
 * replaces: nothing in the reference.  For callers who form Galerkin products R * A * P, A^T * A (with spmv_acc_csr_transpose), pattern
 * powers or Schur-complement pieces on the device and rebuild them on the same pattern at every time step or Newton iteration.  The m x n
 * CSR this writes is clean -- every row strictly ascending in column, int32 -- whatever the inputs looked like.  An entry exists wherever
 * a product exists; a sum of 0.0 is kept.
 * Outputs, all owned by the caller and sized by nprod = the count of the first entry: d_c_rowptr (m + 1 ints), d_c_colindex (nprod ints),
 * d_c_value (nprod doubles), the map d_pa, d_pb (nprod ints each) and d_start (nprod + 1 ints), and *h_nnz (a host int) = nnz(C).  Only
 * the first *h_nnz entries of d_c_colindex / d_c_value and the first *h_nnz + 1 of d_start are written.  d_a_value, d_b_value, d_c_value
 * all NULL: structure only; d_pa, d_pb, d_start all NULL: the map lives in the workspace and is dropped; any other mix of NULLs inside
 * a group is SPMV_ACC_ERR_BAD_ARGUMENT.  nprod must equal the entry's own count (it guards an under-sized allocation), else
 * SPMV_ACC_ERR_BAD_ARGUMENT with the count in the error string.
 * A PURE FUNCTION of the inputs, by expand - sort - compress.  EXPANSION ORDER: product e enumerates A's non-zeros q in storage order
 * and, for each, the entries t of B's row a_colindex[q] in storage order: e = off[q] + (t - b_rowptr[a_colindex[q]]), off = the exclusive
 * scan of those rows' lengths; its key is (row of q, b_colindex[t]).  ONE stable radix sort of (key, e), the assembly's: products with
 * equal (i, j) then form a run in ascending e; run j is C entry j and covers sorted positions [d_start[j], d_start[j + 1]); d_pa[p] and
 * d_pb[p] are the positions of the two factors of sorted product p in A's and B's arrays.  VALUES: d_c_value[j] = the sum of the run's
 * products a_value[d_pa[p]] * b_value[d_pb[p]], each ROUNDED to fp64 before it is added (no fused multiply-add), in exactly the
 * assembly's summation order (spmv_acc_coo_to_csr above, spmv_acc_amd/csrc/coo.hpp): runs of up to 64 products by one lane starting from
 * the first product, bitwise a host loop; longer ones by a wavefront -- strided partial sums, then the balanced tree.  No atomics: two
 * calls on the same inputs give the same bits, and tunable "deterministic" changes nothing.  The values come from the next entry's kernel.
 * Columns of A outside [0, k) and of B outside [0, n) are counted before anything reads through them: if there are any, nothing is
 * written, the return is SPMV_ACC_ERR_BAD_ARGUMENT and the error string holds their numbers.  a_rowptr[0] != 0, b_rowptr[0] != 0, or a
 * given nnz_a / nnz_b that is not rowptr[last]: SPMV_ACC_ERR_BAD_ARGUMENT (nnz_a / nnz_b < 0: read from the device).  Null pointers where
 * data is needed, negative sizes: SPMV_ACC_ERR_BAD_ARGUMENT, nothing is launched.  No products (no non-zeros, or A only meets empty rows
 * of B; nprod == 0): d_c_rowptr is set to zeros, *h_nnz = 0, nothing else is touched.  m, k, n, nnz_a, nnz_b or the product count beyond
 * INT_MAX - 2^16: SPMV_ACC_ERR_TOO_LARGE with the count in the error string; rows of C are independent, so multiply row ranges of A.
 * Runs on the calling thread's library stream and has finished when it returns.  WORKSPACE, one allocation, freed on every path: 16 B per
 * product (the packed keys before and after the sort; no factor position is kept through the sort, the map is recomputed from the sorted
 * order) -- 28 B without the map -- plus 20 B per non-zero of A and the sort's scratch: the assembly's class.  Inside a stream capture it
 * enqueues nothing and returns SPMV_ACC_ERR_BAD_ARGUMENT.  Makes and touches no plan: hand C to spmv_acc_prepare or any product entry
 * afterwards.  Returns 0 or an spmv_acc_error code (also left in spmv_acc_last_error).
 * COST, as measured (MI355X, tools/spgemm_bench.py, profiles/spgemm_bench.md; the box copied at 6.41 TB/s in the same run): the time follows
 * the PRODUCT count, not nnz(C).  Headline stand-in, A^T * A (201.3 M products -> 112.7 M entries; settled SpMV on A 0.142 ms): 21.4 ms =
 * 150 SpMVs.  FEM class, A * A (868.7 M products -> 111.5 M entries, 7.8 products per entry; SpMV 0.059 ms): 81.6 ms = 1 393 SpMVs.
 * Galerkin-shaped R * (A * P) with an 8 : 1 aggregation, both products together: 9.0 ms (59.4 M products, 63 SpMVs) and 5.4 ms (33.9 M, 91
 * SpMVs).  torch.sparse CSR @ CSR (rocSPARSE, hash accumulation: structure and values in one step, no kept map, sums in no stated order)
 * takes 5.1 / 6.4 / 2.2 / 1.1 ms on the four: 4 x to 13 x FASTER than this entry for a product formed once -- most where many products
 * fall on one entry.  This entry pays per scalar product for being a pure function of its inputs and for the map of the next entry. */
int spmv_acc_csr_spgemm(int m, int k, int n,
                        int nnz_a, const int *d_a_rowptr, const int *d_a_colindex, const double *d_a_value,
                        int nnz_b, const int *d_b_rowptr, const int *d_b_colindex, const double *d_b_value,
                        int nprod, int *d_c_rowptr, int *d_c_colindex, double *d_c_value,
                        int *d_pa, int *d_pb, int *d_start, int *h_nnz);

/* ---- sparse product C = A * B, 3: new values of A and / or B on a known pattern (new; the per-step hot path) ----------------------------
 * replaces: nothing in the reference.  d_c_value[j] = the sum over p in [d_start[j], d_start[j + 1]) of d_a_value[d_pa[p]] *
 * d_b_value[d_pb[p]] for j < nnz_c, with the map (d_pa, d_pb, d_start), nprod and nnz_c = *h_nnz of an earlier spmv_acc_csr_spgemm on
 * the same two patterns.  Rounding and summation order are exactly the first entry's (which runs this kernel for its own values), so the
 * same values repeat its bits.  One kernel on the calling thread's library stream: asynchronous, no allocation, may be captured into a
 * hipGraph.  The map is the caller's array here: a d_start interval that reaches outside [0, nprod] is clamped; an entry of d_pa / d_pb
 * outside A's / B's value arrays CANNOT be checked (their lengths are not passed), so THE MAP MUST COME FROM THE FIRST ENTRY, unedited.
 * nnz_c > nprod or a null pointer with nnz_c > 0: SPMV_ACC_ERR_BAD_ARGUMENT; nnz_c == 0: nothing.  It streams 8 B of map per product
 * and 12 B per entry and gathers 16 B per product.  Returns 0 or an spmv_acc_error code.
 * COST, as measured (same run): headline stand-in A^T * A 1.85 ms = 3.34 TB/s of those needed bytes, 13 SpMVs (torch's whole product:
 * 5.1 ms); Galerkin-shaped R * (A * P) 0.98 ms (headline, 1.77 TB/s, 7 SpMVs; torch 2.2 ms) and 0.60 ms (FEM class, 1.50 TB/s, 10 SpMVs;
 * torch 1.1 ms); FEM class A * A, 868.7 M products on 111.5 M entries: 14.1 ms = 1.57 TB/s, 241 SpMVs -- SLOWER than torch's whole product
 * (6.4 ms): with 7.8 products per entry the 24 B streamed and gathered per product outweigh a hash accumulator's work per entry.  Keep the
 * map where a few products fall on an entry (Galerkin products, A^T * A of short rows); on dense-ish squares it does not pay. */
int spmv_acc_csr_spgemm_values(int nprod, int nnz_c, const int *d_pa, const int *d_pb, const int *d_start,
                               const double *d_a_value, const double *d_b_value, double *d_c_value);

/* ---- sparse add C = alpha * A + beta * B, 1: structure, map and first values, into caller-owned arrays (new) ----------------------------
 * replaces: nothing in the reference; it multiplies a matrix by a vector.  For callers who form M + dt * K, shifts A + sigma * I,
 * symmetrisations A + A^T (with spmv_acc_csr_transpose) or Galerkin corrections R * A * P + D on the device and rebuild them on the same
 * patterns at every step.
 * INPUTS: A and B are both m x n, CSR, int32, fp64, rebased (rowptr[0] == 0), and every row is STRICTLY ASCENDING in column -- sorted, no
 * duplicate -- which is what spmv_acc_coo_to_csr, spmv_acc_csr_transpose and spmv_acc_csr_spgemm write.  Explicit zeros are ordinary
 * entries.  nnz_a / nnz_b must be rowptr[m], or negative: read from the device.
 * THE RESULT IS UNIQUE (no implementation choice can change a bit of it).  PATTERN: row i of C is the sorted union of row i of A and row
 * i of B; nothing is pruned, an entry whose value cancels to 0.0 stays; *h_nnz (a host int) = nnz(C) <= nnz_a + nnz_b.  MAP: d_ia[j] =
 * the position of C entry j in A's arrays, or -1 where A has no entry there; d_ib[j] likewise for B; at least one of the two is >= 0.
 * VALUES: with ta = alpha * a_value[ia[j]] and tb = beta * b_value[ib[j]], each ROUNDED to fp64 (no fused multiply-add): both present:
 * c_value[j] = ta + tb; only A present: ta; only B present: tb.  No implicit + 0.0: an A-only -0.0 with alpha == 1 stays -0.0; alpha
 * == 0 is not special-cased, 0 * Inf = NaN propagates; the pattern is the union whatever alpha and beta are.  The values come from the
 * next entry's kernel, so they are bit-equal to what it gives on the returned map.
 * OUTPUTS, all owned by the caller: d_c_rowptr (m + 1 ints); d_c_colindex, d_c_value, d_ia, d_ib sized nnz_a + nnz_b (no count entry is
 * needed); only their first *h_nnz elements are written.  d_a_value, d_b_value, d_c_value all NULL: structure only; d_ia, d_ib both
 * NULL: no map is returned (with values, a copy lives in the workspace and is dropped); any other mix of NULLs inside a group is
 * SPMV_ACC_ERR_BAD_ARGUMENT (a matrix without non-zeros still passes a non-null value pointer; it is not read).  d_c_value must not
 * overlap d_a_value or d_b_value, and no output may overlap an input.
 * CHECKS.  On the host, before the device is touched: negative m or n, null pointers where data is needed: SPMV_ACC_ERR_BAD_ARGUMENT;
 * m, n, nnz_a, nnz_b or nnz_a + nnz_b beyond INT_MAX - 2^16: SPMV_ACC_ERR_TOO_LARGE -- rows of C are independent, so add row ranges of A
 * and B.  On the device, each SPMV_ACC_ERR_BAD_ARGUMENT: rowptr[0] != 0; a given nnz_a / nnz_b that is not rowptr[m]; and ONE CENSUS of
 * both matrices before anything reads through an index, counting (a) columns outside [0, n), (b) positions inside a row whose column
 * does not exceed its predecessor's, (c) rows whose rowptr extent descends or leaves [0, nnz]: if any count is non-zero nothing was
 * written and the error string holds the three counts per matrix (for (b): spmv_acc_coo_to_csr sorts and merges such a matrix).  An
 * empty A, an empty B, both empty or m == 0 succeed: C is the other matrix scaled, or d_c_rowptr all zeros (then nothing else is touched
 * and nothing is allocated).
 * Runs on the calling thread's library stream and has finished when it returns.  No sort: every entry's place in C is a rank each
 * non-zero computes on its own (one binary search in the other matrix' row; spmv_acc_amd/csrc/csr_add.hpp), all passes are cut by
 * non-zeros, none by rows, and there is no atomic: two calls on the same inputs give the same bits, tunable "deterministic" changes
 * nothing.  WORKSPACE, one allocation, freed on every path: 8 B per non-zero of A, 96 KiB of census counts and the scan's scratch, plus
 * 8 B per possible entry when values are wanted without a map.  Inside a stream capture it enqueues nothing and returns
 * SPMV_ACC_ERR_BAD_ARGUMENT.  Makes and touches no plan: hand C to spmv_acc_prepare or any product entry afterwards.  Returns 0 or an
 * spmv_acc_error code (also left in spmv_acc_last_error).
 * COST, as measured (MI355X, tools/csr_add_bench.py, profiles/csr_add_bench.md; the box copied at 6.59 TB/s in the same run; stand-ins made
 * canonical by spmv_acc_coo_to_csr first).  Headline stand-in (settled SpMV on A 0.145 ms): M + dt K on one pattern, 40.5 M + 40.5 M ->
 * 40.5 M entries, 6.2 ms = 43 SpMVs; A + sigma I, 40.5 M + 7.6 M -> 48.0 M, 5.1 ms = 35 SpMVs; torch.add on sparse-CSR tensors (structure
 * and values in one step, no kept map) takes 8.3 / 9.8 ms there.  FEM class (SpMV 0.049 ms): A + A^T, 28.2 M + 28.2 M -> 35.1 M, 4.1 ms =
 * 84 SpMVs; M + dt K 3.4 ms; A + sigma I 2.5 ms -- torch.add takes 1.57 / 1.20 / 1.28 ms: this entry is 2 x to 3 x SLOWER than torch for
 * a sum formed once on that class (and on the 9.4 M stand-in: 1.5 / 1.2 / 0.97 ms against 0.56 / 0.42 / 0.42).  It pays for the census,
 * for the map of the next entry and for two synchronising reads; how its time splits between the passes has not been separated. */
int spmv_acc_csr_add(int m, int n,
                     int nnz_a, const int *d_a_rowptr, const int *d_a_colindex,
                     int nnz_b, const int *d_b_rowptr, const int *d_b_colindex,
                     double alpha, const double *d_a_value, double beta, const double *d_b_value,
                     int *d_c_rowptr, int *d_c_colindex, double *d_c_value,
                     int *d_ia, int *d_ib, int *h_nnz);

/* ---- sparse add C = alpha * A + beta * B, 2: new values, alpha or beta on a known pattern (new; the per-step hot path) ------------------
 * replaces: nothing in the reference.  d_c_value[j] for j < nnz_c by the VALUES rule above, through the map (d_ia, d_ib) and nnz_c =
 * *h_nnz of an earlier spmv_acc_csr_add on the same two patterns; nnz_a / nnz_b are the lengths of the value arrays.  The first entry
 * runs this kernel for its own values, so the same values repeat its bits.  The map is the caller's array here: an index outside
 * [0, nnz_a) / [0, nnz_b) -- this includes -1 -- counts as absent and is never turned into an address; an entry with both absent is
 * +0.0.  d_c_value must NOT overlap d_a_value or d_b_value (entries are not read and written in the same order).
 * One kernel on the calling thread's library stream: asynchronous, no allocation, no synchronisation, no copy; may be captured into a
 * hipGraph.  alpha and beta are kernel arguments: a captured launch keeps the alpha and beta it was captured with, only the arrays'
 * contents follow the caller (capture again, or update the graph node, for a new dt).  Negative sizes, or a null pointer where data is
 * needed with nnz_c > 0: SPMV_ACC_ERR_BAD_ARGUMENT; a size beyond INT_MAX - 2^16: SPMV_ACC_ERR_TOO_LARGE; nnz_c == 0: nothing.  Per C
 * entry it streams 8 B of map, gathers 8 B per present operand (both maps ascend apart from the -1 gaps: near-sequential) and stores
 * 8 B.  Returns 0 or an spmv_acc_error code.
 * COST, as measured (same run): 0.90 to 0.92 of the box's copy rate on the bytes it needs, on every job of the two large stand-ins.
 * Headline stand-in, M + dt K: 0.214 ms = 6.05 TB/s, 1.5 SpMVs (torch's whole add: 8.3 ms); A + sigma I 0.193 ms.  FEM class: A + A^T
 * 0.170 ms, M + dt K 0.149 ms, A + sigma I 0.116 ms = 2.4 to 3.5 SpMVs, 8 x to 11 x faster than torch's whole add.  The 9.4 M stand-in
 * reads 0.93 to 1.02 of the copy rate (0.037 to 0.051 ms; supposed, not checked: part of its arrays stays in the last-level cache). */
int spmv_acc_csr_add_values(int nnz_c, int nnz_a, int nnz_b, const int *d_ia, const int *d_ib,
                            double alpha, const double *d_a_value, double beta, const double *d_b_value,
                            double *d_c_value);

/* ---- extraction C = A[rows, colmap] with a diagonal band, 1: structure, map and first values (new) ----------------------------------------
 * replaces: nothing in the reference.  Takes a matrix apart or renumbers it on the device: the symmetric permutation P A P^T (rows = perm,
 * colmap = its inverse), sub-blocks A[I, J] (Schur complements with spmv_acc_csr_spgemm and spmv_acc_csr_add, a local / halo column split),
 * the triangles and the diagonal of A as CSR matrices (L + D + U), and a row-sorted copy of an unsorted CSR (what spmv_acc_csr_add demands).
 * INPUTS: A is m x n, CSR, int32, fp64, rebased (rowptr[0] == 0); its rows may be in ANY column order and may repeat a column.  nnz_a must be
 * rowptr[m], or negative: read from the device.  d_rows[mc]: row i of C is row rows[i] of A; the rows must be distinct; NULL: rows[i] = i, and
 * then mc must equal m.  d_colmap[n]: an entry with column c gets the new column colmap[c]; a negative value drops the column, the non-negative
 * values must be distinct and < nc; NULL: the identity, and then nc must equal n; nc may exceed n (embedding).  diag_lo, diag_hi: an entry at
 * (i, j) of C is kept iff diag_lo <= (long long)j - i <= diag_hi, in C's OWN indices: INT_MIN, INT_MAX keeps everything; 0, 0 the diagonal;
 * INT_MIN, 0 the lower triangle; 1, INT_MAX the strict upper; diag_lo > diag_hi is legal and gives an empty C.
 * THE RESULT IS UNIQUE (no implementation choice can change a bit of it).  C is mc x nc.  Row i of C holds the kept entries of row rows[i] of
 * A in ascending new column; entries of equal new column occur only where A's row repeats a column, and stay in ascending position of A.  C
 * has strictly ascending rows exactly when the selected rows of A repeat no column.  MAP: d_map[j] = the position of C entry j in A's arrays.
 * VALUES: c_value[j] = a_value[map[j]], the bits copied with no arithmetic (-0.0 and NaN payloads survive); nothing is pruned by value.
 * *h_nnz (a host int) = nnz(C) <= nnz_a.  Rows of A that are not selected are never read, and so never checked.
 * OUTPUTS, all owned by the caller: d_c_rowptr (mc + 1 ints); d_c_colindex, d_c_value, d_map sized nnz_a (the upper bound, no count entry is
 * needed); only their first *h_nnz elements are written.  d_a_value and d_c_value both NULL: structure only; exactly one of them NULL is
 * SPMV_ACC_ERR_BAD_ARGUMENT.  d_map may be NULL (with values, a copy lives in the workspace and is dropped).  d_c_value must not overlap
 * d_a_value, and no output may overlap an input.
 * CHECKS.  On the host, before the device is touched: negative m, n, mc or nc, null pointers where data is needed, d_rows == NULL with mc != m,
 * d_colmap == NULL with nc != n: SPMV_ACC_ERR_BAD_ARGUMENT; m, n, mc, nc or nnz_a beyond INT_MAX - 2^16: SPMV_ACC_ERR_TOO_LARGE -- rows of C
 * are independent, so extract row ranges.  On the device, each SPMV_ACC_ERR_BAD_ARGUMENT: rowptr[0] != 0; a given nnz_a that is not rowptr[m];
 * and ONE CENSUS before anything reads through an index, counting (a) rows outside [0, m), (b) repeated rows, (c) selected rows whose rowptr
 * extent descends or leaves [0, nnz_a], (d) colmap values >= nc, (e) repeated non-negative colmap values, then (f) candidates -- entries of
 * the selected rows -- whose column lies outside [0, n): if any count is non-zero nothing was written and the error string holds the counts.
 * mc == 0, m == 0, nnz_a == 0 or no candidate: d_c_rowptr all zeros, *h_nnz = 0, nothing else is touched (so too when nothing is kept).
 * Runs on the calling thread's library stream and has finished when it returns.  A stable compaction of the candidates, then a count of the
 * descents inside the rows of the result: with none (sorted rows under an identity or order-preserving colmap: sub-blocks, triangles, row
 * gathers) that is the answer; otherwise one stable radix sort by (row, new column).  Both give the same bits.  All passes are cut by
 * candidates or C entries, none by rows, and there is no atomic: two calls on the same inputs give the same bits, tunable "deterministic"
 * changes nothing.  WORKSPACE, three allocations, freed on every path: 4 B per row of A (with d_rows), 4 B per column of C (with d_colmap),
 * 8 B per row of C, 112 KiB of census counts; per candidate 8 B, 12 B when values are wanted without a map; only when a sort is needed, per
 * entry of C 20 B without and 24 B with a map, and the radix sort's scratch (about 12 B per entry).  Inside a stream capture it enqueues
 * nothing and returns SPMV_ACC_ERR_BAD_ARGUMENT.  Makes and touches no plan.  Returns 0 or an spmv_acc_error code (also left in
 * spmv_acc_last_error).
 * COST, as measured (MI355X, tools/extract_bench.py, profiles/extract_bench.md; the box copied at 6.63 TB/s in the same run; stand-ins made
 * canonical by spmv_acc_coo_to_csr first; beside each the plain torch composition a user would write today: expand the rows, map, mask, one
 * stable sort of the keys, bincount -- its result equals this entry's bit for bit in every job).  Headline stand-in (40.5 M entries, settled
 * SpMV 0.146 ms): random row and column permutations (sort path) 12.5 ms = 85 SpMVs, torch 11.7 ms -- torch is 6 % FASTER there; the strict
 * lower triangle (no sort) 6.8 ms against 10.6 ms; a contiguous half-by-half block 3.7 ms against 5.7 ms.  FEM class (28.2 M entries, SpMV
 * 0.051 ms): a random symmetric permutation 6.5 ms = 128 SpMVs against 7.6 ms; strict lower 3.0 ms against 4.8 ms; block 2.1 ms against
 * 4.0 ms.  How the time splits between the census, the two scans, the sort and the four synchronising reads has not been separated. */
int spmv_acc_csr_extract(int m, int n, int nnz_a, const int *d_a_rowptr, const int *d_a_colindex, const double *d_a_value,
                         int mc, const int *d_rows, int nc, const int *d_colmap, int diag_lo, int diag_hi,
                         int *d_c_rowptr, int *d_c_colindex, double *d_c_value, int *d_map, int *h_nnz);

/* ---- extraction C = A[rows, colmap] with a diagonal band, 2: new values on a known pattern (new; the per-step hot path) --------------------
 * replaces: nothing in the reference.  d_c_value[j] = d_a_value[d_map[j]] for j < nnz_c, through the map and nnz_c = *h_nnz of an earlier
 * spmv_acc_csr_extract on the same pattern; nnz_a is the length of d_a_value.  The first entry runs this kernel for its own values, so the
 * same values repeat its bits.  The map is the caller's array here: an index outside [0, nnz_a) -- this includes -1 -- gives +0.0 and is
 * never turned into an address.  d_c_value must NOT overlap d_a_value (entries are not read and written in the same order).
 * (spmv_acc_csr_transpose_values cannot serve: it bounds its map by the one nnz it is given, and here nnz(C) != nnz(A).)
 * One kernel on the calling thread's library stream: asynchronous, no allocation, no synchronisation, no copy; may be captured into a
 * hipGraph.  Negative sizes, or a null pointer where data is needed with nnz_c > 0: SPMV_ACC_ERR_BAD_ARGUMENT; a size beyond INT_MAX - 2^16:
 * SPMV_ACC_ERR_TOO_LARGE; nnz_c == 0: nothing.  Per C entry it streams 4 B of map, gathers 8 B and stores 8 B: 20 B.  Returns 0 or an
 * spmv_acc_error code.
 * COST, as measured (same run; rates on the 20 B an entry needs, relative to the box's copy rate).  Headline stand-in: the monotone map of
 * the strict lower triangle, 38.6 M entries, 0.133 ms = 0.88 of the copy rate, 0.9 SpMVs; the map of random row and column permutations
 * 0.266 ms = 0.46 (every missed gather is a whole memory request).  FEM class: a random symmetric permutation, whose rows of 30 entries stay
 * contiguous runs of the map, 0.102 ms = 0.84; the strict lower triangle, 13.9 M entries out of every other run of A's values, 0.068 ms =
 * 0.62 (the lines it gathers from are half used; supposed, not checked).  torch.index_select(a_value, 0, map) into a preallocated tensor takes
 * 0.263 / 0.142 / 0.112 / 0.072 ms on the same four maps: within 1 % on the permuted headline map (torch ahead), 6 to 9 % slower elsewhere. */
int spmv_acc_csr_extract_values(int nnz_c, int nnz_a, const int *d_map, const double *d_a_value, double *d_c_value);

/* ---- multicolour Gauss-Seidel / SOR, 1: the colouring of the pattern (new; analysis) ------------------------------------------------------
 * replaces: nothing in the reference.  Colours the rows of a square matrix so that no two rows joined by a stored off-diagonal entry share a
 * colour; the rows of one colour can then be relaxed together, and a Gauss-Seidel sweep is one launch per colour (spmv_acc_csr_gs_sweep).
 * INPUTS: A is m x m, CSR, int32, rebased (rowptr[0] == 0, rowptr[m] == nnz); its rows STRICTLY ascend and its PATTERN is symmetric (values
 * are not read).  An unsymmetric matrix: colour the pattern of A + A^T from spmv_acc_csr_transpose and spmv_acc_csr_add -- those colours are
 * valid for A.
 * THE RESULT IS UNIQUE, a pure function of the pattern.  Row v has the 64-bit priority (mix32(v) << 32) | v with mix32(x): x ^= x >> 16;
 * x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 (32-bit unsigned).  The rows are taken in descending priority and each gets the
 * smallest colour >= 0 that no already-coloured off-diagonal neighbour holds.  On the device this is computed in Jones-Plassmann rounds (an
 * uncoloured row with no uncoloured neighbour of higher priority takes its colour; colours are read from the round before), which gives the
 * same colours whatever the timing; the number of rounds is a function of the pattern too.
 * OUTPUTS: d_color[m] = the colour of every row.  *h_ncolors = 1 + the largest colour (0 for m == 0).  d_color_rows[m] = the rows in ascending
 * (colour, row): a stable sort by colour, which is exactly the perm of a symmetric permutation C[i, j] = A[perm[i], perm[j]] that makes every
 * colour a contiguous row range.  h_color_ptr, a HOST array of cap_colors + 1 ints: colour c owns the positions [h_color_ptr[c],
 * h_color_ptr[c + 1]) of d_color_rows.  *h_no_diag = the number of rows that store no diagonal entry (the sweep leaves them untouched).
 * More than cap_colors colours: SPMV_ACC_ERR_TOO_LARGE, with *h_ncolors, *h_no_diag, d_color and d_color_rows valid and h_color_ptr not
 * written: call again with a larger array.
 * CHECKS.  On the host, before the device is touched: negative m or nnz, cap_colors < 1, null pointers where data is needed:
 * SPMV_ACC_ERR_BAD_ARGUMENT; m or nnz beyond INT_MAX - 2^16: SPMV_ACC_ERR_TOO_LARGE.  On the device ONE CENSUS, counting (a) rowptr[0] != 0 or
 * rowptr[m] != nnz, (b) rows whose rowptr extent descends or leaves [0, nnz], (c) columns outside [0, m), (d) positions where a row does not
 * strictly ascend, (e) off-diagonal entries (i, j) whose mirror (j, i) is not stored: if any count is non-zero, SPMV_ACC_ERR_BAD_ARGUMENT,
 * nothing was written and the error string holds the counts.  A bad index is never turned into an address.  A group of rounds that colours no
 * row while some remain (impossible on a pattern that passed the census) ends the call with SPMV_ACC_ERR_HIP instead of another round.
 * Runs on the calling thread's library stream and has finished when it returns.  No atomic, no kernel that waits on another workgroup: two
 * calls on the same pattern give the same arrays.  WORKSPACE, one allocation, freed on every path: 20 B per row, 4 B per colour of
 * h_color_ptr (at most per row), 96 KiB of census counts and the radix sort's scratch.  Inside a stream capture it enqueues nothing and
 * returns SPMV_ACC_ERR_BAD_ARGUMENT.  Makes and touches no plan.  Returns 0 or an spmv_acc_error code (also left in spmv_acc_last_error).
 * COST: rounds x one pass over rowptr and colindex (the census one more, with a binary search per off-diagonal entry), one row per lane --
 * a row of very many entries is walked by a single lane --, one synchronising read per 8 rounds, one radix sort of m keys.  As measured
 * (MI355X, tools/gs_bench.py, profiles/gs_bench.md): a 9-point FEM-quads matrix of 4.0 M rows and 36.0 M entries 2.38 ms = 32 settled SpMVs
 * (9 colours, 23 rounds); a 27-point grid of 3.4 M rows and 89.9 M entries 13.9 ms = 73 SpMVs (18 colours, 59 rounds). */
int spmv_acc_csr_color(int m, int nnz, const int *d_rowptr, const int *d_colindex,
                       int *d_color, int *d_color_rows, int cap_colors, int *h_color_ptr,
                       int *h_ncolors, int *h_no_diag);

/* ---- multicolour Gauss-Seidel / SOR, 2: one sweep (new; the per-step hot path) --------------------------------------------------------------
 * replaces: nothing in the reference.  One forward (direction 0: colours 0 .. ncolors - 1), backward (1: ncolors - 1 .. 0) or symmetric (2:
 * forward, then backward) sweep of x towards the solution of A x = b, with the colours of spmv_acc_csr_color: ncolors = *h_ncolors,
 * h_color_ptr (a host array) and d_color_rows as it left them.  d_color_rows == NULL: the matrix, b and x have been permuted by colour
 * (C[i, j] = A[perm[i], perm[j]] with perm = d_color_rows) and colour c IS the row range [h_color_ptr[c], h_color_ptr[c + 1]) -- the
 * coalesced form.  Every row i of a colour is updated in place:  s = the sum of value * x[col] over the row's stored entries with col != i,
 * g = (b[i] - s) / a_ii,  x[i] = g if omega == 1.0, else x[i] + omega * (g - x[i]).
 * BIT FOR BIT a pure function of the arrays and of h_color_ptr: every product, the subtraction, the division and the relaxation are rounded on
 * their own (no fused multiply-add); the diagonal's position and a column outside [0, m) contribute the term +0.0; a row's terms are added by
 * a group of G lanes, lane l the terms l, l + G, ... in order from its first, the G partial sums as a balanced tree over neighbouring lanes; G
 * (a power of two, 1 .. 64) is the smallest with 4 G >= the mean row length of the 64 consecutive rows of the colour that one workgroup owns
 * (spmv_acc_amd/csrc/gs.hpp spells it out, tests/test_gs_host.py host_gs_sweep restates it in numpy).
 * A row without a stored diagonal is left untouched; a zero diagonal gives what IEEE division gives; a row index outside [0, m) is skipped;
 * rowptr extents are clamped to [0, nnz]: crafted arrays cannot make it read or write outside the caller's arrays.  THE ENTRY CANNOT CHECK
 * THAT THE COLOURS ARE VALID FOR THE PATTERN: with two joined rows in one colour the launch races and the result is not defined (nothing
 * faults).
 * One launch per non-empty colour on the calling thread's library stream, in order: asynchronous, no allocation, no synchronisation, no
 * copy, no plan; may be captured into a hipGraph (one stream, no parallel branches).  CHECKS, on the host, nothing launched: null pointers
 * where data is needed, negative sizes, direction outside 0 .. 2, h_color_ptr not ascending from 0 to m, d_b overlapping d_x:
 * SPMV_ACC_ERR_BAD_ARGUMENT; a size beyond INT_MAX - 2^16: SPMV_ACC_ERR_TOO_LARGE.  Returns 0 or an spmv_acc_error code.
 * COST: per direction the bytes of one SpMV (12 B per non-zero, rowptr, b, x) in ncolors launches.  As measured (MI355X, tools/gs_bench.py,
 * profiles/gs_bench.md; one symmetric sweep beside two settled SpMVs of the engine on the same matrix in the same process): the FEM-quads
 * matrix above, 18 launches, 0.454 ms colour-permuted = 3.0 x two SpMVs (0.0753 ms each) and 0.813 ms through d_color_rows = 5.4 x; the
 * 27-point grid, 36 launches, 1.146 ms = 3.0 x (SpMV 0.190 ms) and 1.380 ms = 3.6 x.  Replayed from a graph: the same times.  A launch
 * with nothing to move costs 4.4 us replayed, so the launch count is a quarter to a fifth of the gap; the rest is the kernel (supposed, not
 * checked: x lines are fetched once per colour, and short rows fill their lane group's step only partly). */
int spmv_acc_csr_gs_sweep(int m, int nnz, const int *d_rowptr, const int *d_colindex, const double *d_value,
                          int ncolors, const int *h_color_ptr, const int *d_color_rows,
                          double omega, int direction, const double *d_b, double *d_x);

/* ---- damped Jacobi / l1-Jacobi, 1: the inverse diagonal (new; once per set of values) --------------------------------------------------------
 * replaces: nothing in the reference.  d_dinv (m doubles) for spmv_acc_csr_jacobi_sweep, of a square m x m CSR, int32, rebased, rows ascending.
 * kind 0 (Jacobi): dinv[i] = 1.0 / a_ii, a_ii the stored diagonal entry; +0.0 where row i stores none.  kind 1 (scaled l1): with
 * g[i] = sqrt(|a_ii|) (correctly rounded, +0.0 without a stored diagonal; written to d_work, m doubles, which kind 0 does not use and may
 * pass as NULL),  d_i = the sum over the row's stored entries of |a_ij| * fl(g[i] / g[j])  -- the quotient rounded first, then the product; a
 * column outside [0, m) contributes +0.0 --,  dinv[i] = 1.0 / d_i; +0.0 where row i stores no diagonal.  A zero or missing diagonal elsewhere
 * in the sum gives what IEEE gives (x / 0 = inf, 1 / inf = +0, 0 / 0 = NaN).  For a symmetric A with a positive diagonal D = diag(d_i) >= A,
 * so I - omega D^-1 A contracts in the energy norm for every omega in (0, 2), and D scales as A does under A -> S A S: no damping factor has to
 * be chosen, on a badly scaled matrix either.  BIT FOR BIT a pure function of the arrays: the terms are added in spmv_acc_csr_gs_sweep's order
 * on consecutive rows (a lane group G per 64 consecutive rows, lane l the terms l, l + G, ... from its first, a balanced tree over
 * neighbouring lanes; spmv_acc_amd/csrc/jacobi.hpp spells it out, tests/test_jacobi_host.py host_jacobi_diagonal restates it in numpy).
 * One launch (kind 0) or two (kind 1) on the calling thread's library stream: asynchronous, no allocation, no synchronisation, no copy, no
 * plan, no census; capturable.  rowptr extents are clamped to [0, nnz] and a column outside [0, m) is never turned into an address: crafted
 * arrays cannot make it read or write outside the caller's arrays.  CHECKS, on the host, nothing launched: null pointers where data is needed,
 * negative sizes, a kind other than 0 or 1, d_work overlapping d_dinv: SPMV_ACC_ERR_BAD_ARGUMENT; a size beyond INT_MAX - 2^16, or kind 1 with
 * more than 2^29 rows: SPMV_ACC_ERR_TOO_LARGE.  THE ENTRY CANNOT CHECK that A is symmetric or its diagonal positive, which the bound D >= A
 * rests on.  Returns 0 or an spmv_acc_error code.
 * COST: kind 0 reads rowptr and a binary search's worth of each row; kind 1 the bytes of one SpMV and one division per non-zero.  As measured
 * (MI355X, tools/jacobi_bench.py, profiles/jacobi_bench.md; this entry on preallocated d_dinv and d_work, nothing allocated in the timed
 * region), beside a settled SpMV of the engine on the same matrix in the same process: the FEM-quads matrix (4.0 M rows, 9-point), kind 0
 * 0.087 ms = 1.15 SpMVs (0.0760 ms each), kind 1 0.265 ms = 3.5; the 27-point grid (3.4 M rows), 0.241 ms = 1.2 SpMVs (0.1972 ms each) and
 * 0.511 ms = 2.6.  Against the colouring it replaces in an AMG setup (32-73 SpMVs a level):
 * a tenth or less. */
int spmv_acc_csr_jacobi_diagonal(int m, int nnz, const int *d_rowptr, const int *d_colindex, const double *d_value,
                                 int kind, double *d_dinv, double *d_work);

/* ---- damped Jacobi / l1-Jacobi, 2: one sweep, the residual, or both (new; the per-step hot path) ---------------------------------------------
 * replaces: nothing in the reference.  ONE launch for all rows, out of place.  For every row i:  s = the sum of value * x_in[col] over ALL the
 * row's stored entries, the diagonal included (a column outside [0, m) contributes +0.0),  t = b[i] - s,  w = omega * dinv[i];
 * r_out[i] = t if d_r_out is not NULL;  x_out[i] = x_in[i] + w * t if d_x_out is not NULL.  d_x_out alone: a sweep.  d_r_out alone: the
 * residual b - A x without a plan.  Both: the sweep and the residual it started from.  ZERO START, d_x_in == NULL: the matrix is not read,
 * t = b[i], x_out[i] = w * b[i] -- the first sweep from x = 0.  d_dinv from spmv_acc_csr_jacobi_diagonal (or the caller's own).
 * BIT FOR BIT a pure function of the arrays and omega: every product, the subtraction and the update's product and sum are rounded on their
 * own (no fused multiply-add); a row's terms are added by a group of G lanes, lane l the terms l, l + G, ... in order from its first, the G
 * partial sums as a balanced tree over neighbouring lanes; G (a power of two, 1 .. 64) is the smallest with 4 G >= the mean row length of the
 * 64 consecutive rows that one workgroup owns (spmv_acc_amd/csrc/jacobi.hpp; tests/test_jacobi_host.py host_jacobi_sweep restates it).
 * rowptr extents are clamped to [0, nnz]: crafted arrays cannot make it read or write outside the caller's arrays.
 * One launch on the calling thread's library stream: asynchronous, no allocation, no synchronisation, no copy, no plan, no atomics; may be
 * captured into a hipGraph.  CHECKS, on the host, nothing launched: null pointers where data is needed, both outputs NULL, negative sizes, an
 * omega that is not finite, any overlap among d_x_out, d_r_out, d_x_in, d_b and d_dinv (in place the rows would race):
 * SPMV_ACC_ERR_BAD_ARGUMENT; a size beyond INT_MAX - 2^16 or more than 2^29 rows (x_in is gathered through 32-bit byte offsets):
 * SPMV_ACC_ERR_TOO_LARGE.  THE ENTRY CANNOT CHECK that the iteration converges: that needs a symmetric positive definite A and, for kind 0's
 * diagonal, an omega below 2 / the largest eigenvalue of D^-1 A (2/3 is customary), which is the caller's to choose.  Returns 0 or an
 * spmv_acc_error code.
 * COST: the bytes of one SpMV (12 B per non-zero, rowptr, b, x_in) plus dinv and the outputs, in one launch.  As measured (MI355X,
 * tools/jacobi_bench.py, profiles/jacobi_bench.md), beside a settled SpMV of the engine on the same matrix in the same process: the FEM-quads
 * matrix, a sweep 0.190 ms = 2.5 SpMVs, the residual alone 0.176 ms = 2.3, the zero start 0.017 ms = 0.2; the 27-point grid, 0.308 ms = 1.6
 * SpMVs, 0.292 ms = 1.5 and 0.017 ms = 0.1.  THE KERNEL IS SLOWER THAN THE ENGINE: csr_spmv with y_in plus one torch pass does the same sweep in
 * 1.4 and 1.1 SpMVs.  What this entry buys is its contract -- no plan, no per-matrix timing, one documented order, the same bits from the
 * first call on -- and one launch where a symmetric multicolour sweep is 18 to 36: an AMG cycle on it costs 10.4 and 5.9 SpMVs against 41.7
 * and 39.8 on Gauss-Seidel, and AMG-PCG to 1e-8 takes 40 and 31 ms against 110 and 139 ms, in 1.6-1.7 times the iterations. */
int spmv_acc_csr_jacobi_sweep(int m, int nnz, const int *d_rowptr, const int *d_colindex, const double *d_value,
                              const double *d_dinv, double omega, const double *d_b, const double *d_x_in,
                              double *d_x_out, double *d_r_out);

/* ---- aggregation coarsening, 1: distance-2 independent roots and their aggregates (new; analysis) ------------------------------------------
 * replaces: nothing in the reference.  The coarsening step of an aggregation algebraic-multigrid setup on the device: it groups the rows of a
 * square matrix into aggregates and returns them as the CSR structures of the tentative prolongator P (m x naggs, one entry per row) and of
 * its transpose R, so that the Galerkin product R (A P) is two spmv_acc_csr_spgemm calls on the returned arrays, without a transpose.
 * INPUTS: the pattern of the STRENGTH GRAPH, m x m, CSR, int32, rebased (rowptr[0] == 0, rowptr[m] == nnz); its rows STRICTLY ascend and it
 * is symmetric (values are not read, a stored diagonal is not required).  For the matrix itself pass its own pattern.  A filter that drops
 * weak entries by a value threshold is out of scope of this entry: spmv_acc_csr_strength does it -- filter first (its kept pattern is what this
 * entry takes; spmv_acc_csr_extract keeps a sub-pattern), and for an unsymmetric matrix
 * aggregate the pattern of A + A^T (spmv_acc_csr_transpose, spmv_acc_csr_add).
 * THE RESULT IS UNIQUE, a pure function of the pattern.  Row v has the priority of spmv_acc_csr_color, (mix32(v) << 32) | v; distances are
 * counted over off-diagonal entries.  ROOTS: the rows are taken in descending priority and a row becomes a root if no root already chosen lies
 * within distance 2 of it -- the lexicographically first distance-2 maximal independent set; an isolated row is a root.  The roots are
 * numbered 0 .. naggs - 1 in ascending row order.  A: a non-root with a root neighbour joins that root's aggregate (there is at most one).
 * B: every remaining row joins the smallest aggregate id among its neighbours that were assigned as a root or in A.  On the device the roots
 * are found in rounds (a row is decided from the largest key within distance 2 of it, two passes over the pattern per round; 8 to 12 rounds on
 * a mesh), which gives the same sets whatever the timing.
 * OUTPUTS: d_agg[m] = the aggregate of every row.  d_agg_rows[m] = the rows in ascending (aggregate, row), a stable sort.  d_agg_ptr[m + 1]:
 * d_agg_ptr[a] = the first position of aggregate a in d_agg_rows for a <= naggs, and m for naggs < a <= m.  *h_naggs.  (d_agg_ptr[0 ..
 * naggs], d_agg_rows) is the structure of R with ascending rows; (0, 1, .. m, d_agg) is that of P.
 * CHECKS.  On the host, before the device is touched: negative m or nnz, null pointers where data is needed: SPMV_ACC_ERR_BAD_ARGUMENT; m or
 * nnz beyond INT_MAX - 2^16: SPMV_ACC_ERR_TOO_LARGE.  On the device the colouring's ONE CENSUS, counting (a) rowptr[0] != 0 or rowptr[m] !=
 * nnz, (b) rows whose rowptr extent descends or leaves [0, nnz], (c) columns outside [0, m), (d) positions where a row does not strictly
 * ascend, (e) off-diagonal entries (i, j) whose mirror (j, i) is not stored: if any count is non-zero, SPMV_ACC_ERR_BAD_ARGUMENT, nothing was
 * written and the error string holds the counts.  Rows are read clamped and a bad index is never turned into an address.  A group of rounds that
 * decides no row while some remain, or a row without an aggregate after B (both impossible on a pattern that passed the census), ends the call
 * with SPMV_ACC_ERR_HIP instead of another round.  CANNOT CHECK: that the pattern is the strength graph the caller meant.
 * Runs on the calling thread's library stream and has finished when it returns.  No atomic, no kernel that waits on another workgroup: two
 * calls on the same pattern give the same arrays.  WORKSPACE, one allocation, freed on every path: 28 B per row, 96 KiB of counts and the
 * scratch of the scan and the radix sort.  Inside a stream capture it enqueues nothing and returns SPMV_ACC_ERR_BAD_ARGUMENT.  Makes and
 * touches no plan.  Returns 0 or an spmv_acc_error code (also left in spmv_acc_last_error).
 * COST: the census, then per round two passes over rowptr and colindex with one 8-byte gather per entry (the second pass only for the rows
 * still undecided), one row per lane, one synchronising read per 4 rounds; one scan, two assignment passes, one radix sort of m keys.
 * As measured (MI355X, tools/agg_bench.py, profiles/agg_bench.md): a 9-point FEM-quads matrix of 4.0 M rows and 36.0 M entries 3.00 ms = 40
 * settled SpMVs = 1.28 x spmv_acc_csr_color on the same matrix (13 rounds, 302 683 aggregates of 13 rows); a 27-point grid of 3.4 M rows and
 * 89.9 M entries 9.37 ms = 51 SpMVs = 0.68 x the colouring (16 rounds, 71 946 aggregates of 47 rows).  A lane group per row was measured
 * and not kept: four lanes gain 3 % on the grid and lose 38 % on the mesh. */
int spmv_acc_csr_aggregate(int m, int nnz, const int *d_rowptr, const int *d_colindex,
                           int *d_agg, int *d_agg_rows, int *d_agg_ptr, int *h_naggs);

/* ---- aggregation coarsening, 2: the tentative prolongator's values (new; the per-step values pass) ------------------------------------------
 * replaces: nothing in the reference.  The one-vector QR of smoothed aggregation on the aggregates of spmv_acc_csr_aggregate: d_b is the fine
 * near-nullspace vector (NULL: all ones), and with s[a] = the sum of d_b[i]^2 over the rows i of aggregate a,
 *   d_bc[a] = sqrt(s[a]) (naggs doubles: the coarse near-nullspace vector),  d_p_value[i] = d_b[i] / d_bc[d_agg[i]] (m doubles: the values of
 *   P in its CSR order),  d_r_value[p] = d_p_value[d_agg_rows[p]] (m doubles, or NULL: the values of R = P^T in its CSR order).
 * The columns of P are orthonormal: P^T P = I to rounding.  With d_b == NULL every value is 1 / sqrt(the aggregate's size).
 * BIT FOR BIT a pure function of the arrays: every square is rounded on its own (no fused multiply-add) and an aggregate's squares are added
 * in the summation order of spmv_acc_coo_to_csr_values over the run [d_agg_ptr[a], d_agg_ptr[a + 1]) of d_agg_rows; the square root and the
 * division are correctly rounded; a zero norm gives +0.0 in P, not a division by zero.
 * The maps are the caller's arrays: runs are clamped to [0, m]; a d_agg[i] outside [0, naggs) gives d_p_value[i] = +0.0; a d_agg_rows[p]
 * outside [0, m) contributes +0.0 to its norm and gives d_r_value[p] = +0.0: crafted arrays cannot make it read or write outside the caller's
 * arrays.  CANNOT CHECK that d_agg, d_agg_ptr and d_agg_rows describe the same aggregates: pass them as spmv_acc_csr_aggregate left them
 * (d_agg_ptr must hold naggs + 1 ints).
 * Two launches on the calling thread's library stream, the norms and then the values: asynchronous, no allocation, no synchronisation, no
 * copy, no plan; may be captured into a hipGraph.  CHECKS, on the host, nothing launched: negative sizes, null pointers where data is needed,
 * d_b or d_bc overlapping an output, outputs overlapping each other: SPMV_ACC_ERR_BAD_ARGUMENT; a size beyond INT_MAX - 2^16:
 * SPMV_ACC_ERR_TOO_LARGE.  Returns 0 or an spmv_acc_error code.
 * COST: at least 36 B per row with d_r_value and d_b (d_agg, d_agg_rows twice, b, two outputs) and 20 B per aggregate; one lane adds an
 * aggregate's squares one after the other.  As measured (the same tool, file and matrices): 0.105 ms on the FEM-quads aggregates = 4.8 x a
 * device copy of those bytes, 0.125 ms on the grid's = 6.9 x; replayed from a graph: the same times.  Supposed, not checked: the norms are
 * bound by the latency of their dependent gathers, R's values by three dependent gathers per entry. */
int spmv_acc_csr_tentative_values(int m, int naggs, const int *d_agg, const int *d_agg_ptr, const int *d_agg_rows,
                                  const double *d_b, double *d_p_value, double *d_r_value, double *d_bc);

/* ---- strength of connection, 1: the kept pattern of a value threshold and the partition of A's positions (new; analysis) ---------------------
 * replaces: nothing in the reference.  The filter of an aggregation algebraic-multigrid setup on the device: it drops the WEAK couplings of a
 * square matrix by the classical symmetric criterion and returns the kept pattern S -- the strength graph spmv_acc_csr_aggregate takes -- and
 * a stable partition of A's positions into kept and dropped, from which spmv_acc_csr_strength_values forms the filtered matrix and the
 * prolongator smoother per step.
 * INPUTS: A, m x m, CSR, int32 / fp64, rebased (rowptr[0] == 0, rowptr[m] == nnz); its rows STRICTLY ascend and its PATTERN is symmetric (the
 * contract of spmv_acc_csr_color); the values may be unsymmetric.  theta: finite, >= 0 (0.25 is customary; 0 keeps every finite entry).
 * THE RESULT IS UNIQUE TO THE BIT, a pure function of the arrays and theta.  sd[i] = sqrt(|a_ii|), correctly rounded, +0.0 for a row without a
 * stored diagonal.  For an off-diagonal entry (i, j): rhs = fl(fl(sd[i] * sd[j]) * theta) -- the same bits at both ends of the edge, no square
 * root per entry, and no a_ii * a_jj that could overflow --; the entry is KEPT iff |a_ij| >= rhs or |a_ji| >= rhs, a_ji the value at the
 * mirror position (a binary search of row j).  IEEE comparisons: a NaN on either side is false.  A stored diagonal entry is always kept.  The
 * kept pattern is therefore symmetric whatever the values; a row whose diagonal is zero or missing keeps its finite couplings.
 * OUTPUTS: S = the kept entries in A's order (a stable compaction: rows still strictly ascend, nothing is sorted): d_s_rowptr[m + 1],
 * d_s_colindex (nnz ints of room, written in [0, nnz_s)).  d_map[nnz]: a stable partition of A's positions, d_map[0 .. nnz_s) the kept
 * positions ascending (d_map[k] = the position in A of S's entry k), d_map[nnz_s .. nnz) the dropped positions ascending.  d_drop_ptr[m + 1]:
 * d_drop_ptr[i] = the first place of row i's dropped positions in d_map, in [nnz_s, nnz]; d_drop_ptr[m] = nnz.  *h_nnz_s, and *h_no_diag =
 * the number of rows without a stored diagonal (not an error); both are written last.
 * CHECKS.  On the host, before the device is touched: negative m or nnz, null pointers where data is needed, a theta that is negative, NaN or
 * infinite: SPMV_ACC_ERR_BAD_ARGUMENT; m or nnz beyond INT_MAX - 2^16: SPMV_ACC_ERR_TOO_LARGE.  On the device the colouring's ONE CENSUS,
 * counting (a) rowptr[0] != 0 or rowptr[m] != nnz, (b) rows whose rowptr extent descends or leaves [0, nnz], (c) columns outside [0, m),
 * (d) positions where a row does not strictly ascend, (e) off-diagonal entries (i, j) whose mirror (j, i) is not stored: if any count is
 * non-zero, SPMV_ACC_ERR_BAD_ARGUMENT, nothing was written and the error string holds the counts.  Rows are read clamped and a bad index is
 * never turned into an address.  m == 0 touches nothing and returns 0 with *h_nnz_s = 0.  CANNOT CHECK: that theta suits the problem (with
 * M-matrix-like values 0.25 separates a grid's strong direction from a coupling 0.01 times as large; with positive off-diagonals the
 * criterion by magnitude may keep what a signed criterion would drop).
 * Runs on the calling thread's library stream and has finished when it returns.  No atomic, no kernel that waits on another workgroup: two
 * calls on the same arrays give the same arrays.  WORKSPACE, one allocation, freed on every path: 8 B per row, 8 B per entry, 96 KiB of counts
 * and the scan's scratch.  Inside a stream capture it enqueues nothing and returns SPMV_ACC_ERR_BAD_ARGUMENT.  Makes and touches no plan.
 * Returns 0 or an spmv_acc_error code (also left in spmv_acc_last_error).
 * COST: the census (one binary search per entry); one row-per-lane pass for the roots; the flags pass, one entry per lane: 12 B streamed per
 * entry, two gathers of sd, one binary search of the mirror row and one gather of the mirror's value; a scan of nnz + 1 ints; a row-pointer
 * pass; the scatter, 12 B read and 4 or 8 B written per entry; one synchronising read each for the census and for nnz_s.  As measured (MI355X,
 * tools/strength_bench.py, profiles/strength_bench.md; anisotropic values of which 44 % drop at theta = 0.05): a 9-point FEM-quads matrix of
 * 4.0 M rows and 36.0 M entries 3.09 ms = 41 settled SpMVs (spmv_acc_csr_aggregate on that pattern: 3.00 ms); a 27-point grid of 3.4 M rows and
 * 89.9 M entries 9.34 ms = 49 SpMVs; 23 and 30 x a device copy of the inputs and outputs alone.  From a kernel trace: the flags pass 1.50 and
 * 3.51 ms, the census 0.30 and 2.56 ms, the scatter 0.14 and 0.36 ms.  A flags pass with one row per lane was measured and not kept: 0.92 ms
 * on the mesh, 7.52 ms on the grid. */
int spmv_acc_csr_strength(int m, int nnz, const int *d_rowptr, const int *d_colindex, const double *d_value, double theta,
                          int *d_s_rowptr, int *d_s_colindex, int *d_map, int *d_drop_ptr, int *h_nnz_s, int *h_no_diag);

/* ---- strength of connection, 2: the lumped diagonal, the filtered matrix and the prolongator smoother (new; the per-step values pass) --------
 * replaces: nothing in the reference.  On the arrays of spmv_acc_csr_strength and the CURRENT values of A (nnz doubles, A's order):
 * LAUNCH 1, per row i: the lump s_i = the sum of d_value[d_map[p]] over the run [d_drop_ptr[i], d_drop_ptr[i + 1]) in the summation order of
 *   spmv_acc_coo_to_csr_values;  d_diag[i] = a_ii with its bits copied if the run is empty, fl(a_ii + s_i) otherwise, and +0.0 if S's row holds no
 *   diagonal (THE LUMP OF SUCH A ROW IS DISCARDED: S has no entry to carry it).  m doubles: the diagonal D_F of the filtered matrix.
 * LAUNCH 2, per entry j of S in row i, v = d_value[d_map[j]]:
 *   omega == 0.0: the FILTERED MATRIX A_F on S's structure: the diagonal gets d_diag[i], an off-diagonal v with its bits copied.  The row sums
 *     of A_F are those of A up to rounding (rows with a stored diagonal).
 *   omega != 0.0: M = I - omega D_F^-1 A_F on S's structure, so that the smoothed prolongator (I - omega D_F^-1 A_F) T is ONE
 *     spmv_acc_csr_spgemm(M, T):  the diagonal gets d_diag[i] == 0.0 ? 1.0 : fl(1.0 - omega);  an off-diagonal gets
 *     d_diag[i] == 0.0 ? +0.0 : fl(fl(-omega * v) / d_diag[i]).  A row with a zero d_diag is an identity row.
 * d_s_value: nnz_s doubles.  BIT FOR BIT a pure function of the arrays and omega: no fused multiply-add, every operation rounded on its own.
 * The maps are the caller's arrays: every run and row is clamped ([0, nnz] and [0, nnz_s]); a d_map index outside [0, nnz) gives +0.0; the row
 * of an entry is searched inside [0, m) whatever d_s_rowptr holds: crafted arrays cannot make it read or write outside the caller's arrays.
 * Nothing is written outside d_s_value[0 .. nnz_s) and d_diag[0 .. m).  CANNOT CHECK that the four arrays describe the same partition: pass
 * them as spmv_acc_csr_strength left them.
 * Two launches on the calling thread's library stream, the diagonal and then the values: asynchronous, no allocation, no synchronisation, no
 * copy, no plan; may be captured into a hipGraph.  CHECKS, on the host, nothing launched: negative sizes, nnz_s > nnz, null pointers where data
 * is needed, an omega that is NaN or infinite, d_value or d_diag overlapping d_s_value, d_diag overlapping d_value:
 * SPMV_ACC_ERR_BAD_ARGUMENT; m or nnz beyond INT_MAX - 2^16: SPMV_ACC_ERR_TOO_LARGE.  Returns 0 or an spmv_acc_error code.
 * omega = 4 / (3 rho(D_F^-1 A_F)) is the caller's to estimate (d_diag and a few SpMVs with A_F); 2/3 suits a diagonally dominant A_F.
 * COST: launch 1 reads 8 B per row of pointers, 12 B per dropped entry and a short search per row, and writes 8 B per row; launch 2 streams
 * 8 B, gathers 8 B, searches its row and stores 8 B per entry of S, four entries per lane.  As measured (the same tool, file and matrices),
 * both launches together: 0.52 ms on the FEM-quads matrix (20.0 M kept entries) = 6.9 SpMVs = 3.4 x a device copy of those bytes, 1.80 ms on
 * the grid (50.1 M kept) = 9.4 SpMVs = 5.3 x; omega != 0 costs the same within 1 %; replayed from a graph: the same times.  From a kernel
 * trace: launch 1 0.21 and 1.13 ms (twelve dropped entries a row on the grid: a chain of dependent gathers per lane), launch 2 0.31 and
 * 0.71 ms.  Supposed, not checked with counters: the searches of the wavefront's two end rows over all of d_s_rowptr bound launch 2. */
int spmv_acc_csr_strength_values(int m, int nnz, int nnz_s, const int *d_s_rowptr, const int *d_s_colindex, const int *d_map,
                                 const int *d_drop_ptr, const double *d_value, double omega, double *d_s_value, double *d_diag);

/* ---- dense coarse-level solve, 1: the inverse of a small CSR by Gauss-Jordan elimination (new; analysis) -------------------------------------
 * replaces: nothing in the reference.  The solve on the coarsest level of a multigrid hierarchy, on the device: d_inv = A^-1 as a dense
 * row-major m x m array, which spmv_acc_dense_apply multiplies by a right-hand side per cycle.
 * INPUTS: A, m x m, CSR, int32 / fp64, rebased (rowptr[0] == 0, rowptr[m] == nnz); its rows STRICTLY ascend, its columns lie in [0, m); the
 * pattern need not be symmetric.  m <= 4096.  d_inv: caller-owned, m * m doubles.
 * THE RESULT IS UNIQUE TO THE BIT (-0.0 and +0.0 count as equal, NaNs by position), a pure function of the arrays: E = [A | I], m x 2m,
 * positions not stored +0.0; for k = 0 .. m - 1: the pivot row p = the smallest i in [k, m) whose |E[i, k]| equals the maximum over the non-NaN
 * magnitudes of E[k .. m - 1, k] (all NaN: p = k); rows k and p are swapped; piv = E[k, k]; E[k, j] = E[k, j] / piv for every j (an IEEE
 * division, not a reciprocal multiply); every row i != k, with f = E[i, k] taken before the row changes: E[i, j] = fl(E[i, j] - fl(f * E[k, j]))
 * (no fused multiply-add).  d_inv = the right half of E.  The elimination is NOT blocked: the unblocked order is the definition
 * (spmv_acc_amd/csrc/dense.hpp spells it out, tests/test_dense_host.py host_dense_inverse restates it in numpy).
 * *h_info = 0: the inverse is valid.  *h_info = k + 1: the pivot of step k, the first such, was zero, NaN or infinite -- A is singular to
 * working precision, or holds a non-finite value --; the elimination is carried out all the same and the contents of d_inv are unspecified.
 * CHECKS.  On the host, before the device is touched: negative m or nnz, null pointers where data is needed: SPMV_ACC_ERR_BAD_ARGUMENT;
 * m > 4096 or nnz beyond INT_MAX - 2^16: SPMV_ACC_ERR_TOO_LARGE.  On the device the colouring's ONE CENSUS, counting (a) rowptr[0] != 0 or
 * rowptr[m] != nnz, (b) rows whose rowptr extent descends or leaves [0, nnz], (c) columns outside [0, m), (d) positions where a row does not
 * strictly ascend: if any count is non-zero, SPMV_ACC_ERR_BAD_ARGUMENT, nothing was written and the error string holds the counts.  Rows are
 * read clamped and a bad index is never turned into an address.  m == 0 reads nothing, writes nothing and sets *h_info = 0.
 * CANNOT CHECK: that the inverse is accurate.  Partial pivoting bounds the growth in practice, not in theory, and an ill-conditioned A gives
 * an inverse with few correct digits and *h_info = 0: max |A inv - I| is of the order m cond(A) 2^-52.
 * Runs on the calling thread's library stream and has finished when it returns.  No atomic, no kernel that waits on another workgroup: two
 * calls on the same arrays give the same bits.  WORKSPACE, one allocation, freed on every path: 16 m B per row (E), 24 B per row and 96 KiB of
 * counts: 256 MiB at 4096 rows.  Inside a stream capture it enqueues nothing and returns SPMV_ACC_ERR_BAD_ARGUMENT.  Makes and touches no
 * plan.  Returns 0 or an spmv_acc_error code (also left in spmv_acc_last_error).
 * COST: 3 m + 4 launches -- per step the pivot search (one workgroup), the row pass and the rank-1 update, which reads and writes all of E:
 * 32 m^3 B of traffic in all, and below a few hundred rows nothing but launches.  As measured (MI355X,
 * tools/amg_bench.py, profiles/amg_bench.md; the five-point Laplacian): 64 rows 0.7 ms, 256 rows 2.2 to 2.5 ms, 1024 rows 12.5 ms -- 9 to 12 us per
 * step, three launches, at all three sizes: launches, not bytes.  The cap of 4096 rows is reasoned from memory, not timed. */
int spmv_acc_csr_dense_inverse(int m, int nnz, const int *d_rowptr, const int *d_colindex, const double *d_value, double *d_inv, int *h_info);

/* ---- dense coarse-level solve, 2: the apply (new; the per-step hot path) ---------------------------------------------------------------------
 * replaces: nothing in the reference.  d_x = d_inv d_b with the row-major m x m array of spmv_acc_csr_dense_inverse (or any other).
 * BIT FOR BIT a pure function of the arrays: x[i] is the sum of the terms inv[i, j] * b[j], each product rounded on its own (no fused
 * multiply-add), added by the 64 lanes of one wavefront: lane l the terms l, l + 64, ... in order from its first (a lane without a term
 * holds +0.0), the 64 partial sums as a balanced tree over neighbouring lanes -- the order of spmv_acc_csr_gs_sweep with G = 64.  It does not
 * depend on the grid or on timing.
 * One launch on the calling thread's library stream: asynchronous, no allocation, no synchronisation, no copy, no plan; may be captured
 * into a hipGraph.  m == 0 launches nothing.  CHECKS, on the host, nothing launched: a negative m, null pointers where data is needed, d_b
 * overlapping d_x, either overlapping d_inv: SPMV_ACC_ERR_BAD_ARGUMENT; m beyond INT_MAX - 2^16: SPMV_ACC_ERR_TOO_LARGE.  Returns 0 or an
 * spmv_acc_error code.  CANNOT CHECK: that d_inv holds m * m doubles, or the inverse of the matrix the caller means.
 * COST: 8 m^2 B of inv read once, one wavefront per row in 512-B lines; b (8 m B) is read by every wavefront and served by the cache.
 * As measured (the same tool and file): 0.009 ms at 64, 256 and 1024 rows alike, plain or replayed from a graph (0.010 ms) -- one launch --,
 * 2.3 to 2.7 x torch's device copy of as many bytes, which is one launch as well (0.004 ms).  Larger inverses were not measured. */
int spmv_acc_dense_apply(int m, const double *d_inv, const double *d_b, double *d_x);

/* ---- conjugate-gradient vector passes, 1: the size of the partials buffer (new; host arithmetic) ------------------------------------------------
 * replaces: nothing in the reference.  *h_count = the doubles the caller's d_partials must hold for vectors of n entries: 3 * ceil(n / 1024),
 * three dot products' worth of one partial per 1024 terms (0 for n == 0).  Touches no device.
 * COST: none.  CHECKS: a negative n, a null h_count: SPMV_ACC_ERR_BAD_ARGUMENT; n beyond INT_MAX - 2^16: SPMV_ACC_ERR_TOO_LARGE.
 * CANNOT CHECK: that the buffer handed to the other three entries is that large. */
int spmv_acc_cg_partials(int n, size_t *h_count);

/* ---- conjugate-gradient vector passes, 2: the start (new; launch-only) ---------------------------------------------------------------------------
 * replaces: nothing in the reference.  The three entries below are what preconditioned conjugate gradients need beside the SpMV q = A p and
 * the preconditioner z = M r, which stay the caller's calls: every dot product, every scalar that depends on one, and every vector update
 * stay on the device, so that iterations can be enqueued in batches without a host read.  The sequence for A x = b, A symmetric positive
 * definite, M symmetric positive definite:
 *     r = b - A x;  z = M r;  spmv_acc_cg_start;
 *     repeat:  q = A p;  spmv_acc_cg_update;  z = M r;  spmv_acc_cg_direction;        (read d_state now and then: status != 0 ends the solve)
 * The caller owns every array: the vectors (n doubles each), d_partials (spmv_acc_cg_partials doubles), the state block d_state (9 words of
 * 8 bytes) and the optional history d_hist (hist_cap doubles; hist_cap == 0: none, d_hist may be NULL).
 * THE DOT PRODUCT IS A PURE FUNCTION OF ITS TWO ARRAYS, bit for bit -- not of the grid, not of timing; no atomic, no kernel waits on another
 * workgroup: term i = fl(u[i] * v[i]) (no fused multiply-add); partial c = the sum of the terms [1024 c, min(n, 1024 (c + 1))) by the 64 lanes
 * of one wavefront in the order of spmv_acc_csr_gs_sweep with G = 64 (lane l the terms l, l + 64, ... in order from its first, a lane without
 * a term holds +0.0; the 64 sums as a balanced tree over neighbouring lanes); the dot = the partials added the same way by the 256 lanes of
 * ONE workgroup in a launch of its own (lane l the partials l, l + 256, ...; then the balanced tree over neighbouring lanes).  n == 0: +0.0.
 * THE STATE BLOCK, written only by those finish workgroups, with ordinary stores (integer words are unsigned 64-bit, the others doubles):
 *   [0] status: 0 running, 1 converged (rr <= tol2), 2 breakdown with p.q not finite or <= 0, 3 breakdown with r.z not finite or < 0
 *   [1] iterations done   [2] bb = b.b   [3] rr = r.r   [4] rz = r.z   [5] pq = p.q   [6] alpha = rz / pq   [7] beta = rz_new / rz
 *   [8] tol2 = fl(fl(rtol * rtol) * bb): rtol is squared first.  Both quotients are IEEE divisions.
 * THIS ENTRY: the caller has computed r = b - A x and z = M r (d_z == d_r: no preconditioner).  Launch 1, one pass: the partials of b.b, r.r
 * and r.z off the same loads, and p = z.  Launch 2, the finish: bb, rr, rz, tol2; iterations = 0; pq = alpha = beta = +0.0; hist[0] = rr;
 * status = 3 if rz is not finite, else 1 if rr <= tol2 (b = 0, or an exact x0: no iteration is needed), else 3 if rz <= 0, else 0.
 * Two launches on the calling thread's library stream: asynchronous, no allocation, no synchronisation, no copy, no host read, no plan; may be
 * captured into a hipGraph.  n == 0 launches the finish alone (status 1).  CHECKS, on the host, nothing launched: a negative n or hist_cap,
 * null pointers where data is needed, an rtol that is not finite or < 0, d_p, d_partials, d_state or d_hist overlapping each other or d_b,
 * d_r or d_z (the single allowed alias is d_z == d_r): SPMV_ACC_ERR_BAD_ARGUMENT; n beyond INT_MAX - 2^16: SPMV_ACC_ERR_TOO_LARGE.  Returns 0
 * or an spmv_acc_error code.  CANNOT CHECK: that r and z are what the caller says, that A and M are symmetric positive definite (a breakdown
 * status is the only sign), or that the buffers are as large as stated.
 * COST: the pass reads 3 n doubles (2 n with d_z == d_r) and writes n; the finish reads 3 n / 1024.  As measured (MI355X, tools/cg_bench.py,
 * profiles/cg_bench.md; 4.0 M rows, vectors warm in the Infinity Cache): 0.027 ms, 1.4 x torch's device copy of as many bytes. */
int spmv_acc_cg_start(int n, double rtol, const double *d_b, const double *d_r, const double *d_z, double *d_p, double *d_partials,
                      unsigned long long *d_state, double *d_hist, int hist_cap);

/* ---- conjugate-gradient vector passes, 3: the update of x and r (new; the per-iteration hot path) -----------------------------------------------
 * replaces: nothing in the reference.  The caller has computed q = A p.  Four launches: (1) the partials of p.q; (2) the finish: pq, and
 * alpha = rz / pq if pq is finite and > 0, else status = 2; (3) the fused pass x[i] = x[i] + fl(alpha * p[i]), r[i] = r[i] - fl(alpha * q[i])
 * and the partials of the new r.r, every product and sum rounded on its own; (4) the finish: rr, iterations += 1, hist[iterations] = rr while
 * iterations < hist_cap, status = 1 if rr <= tol2.
 * FROZEN MEANS FROZEN: every kernel of this entry and of spmv_acc_cg_direction reads the status first and, when it is not 0, returns before it
 * writes anything: x, r, p, z, the partials, the state and the history keep their bits.  Iterations enqueued past the end of a solve change
 * nothing, and the solution's bits do not depend on how often the host reads the state.
 * On the calling thread's library stream: asynchronous, no allocation, no synchronisation, no copy, no host read, no plan; may be captured.
 * CHECKS, on the host, nothing launched: a negative n or hist_cap, null pointers where data is needed, d_x, d_r, d_partials, d_state or d_hist
 * overlapping each other or d_p or d_q: SPMV_ACC_ERR_BAD_ARGUMENT; n beyond INT_MAX - 2^16: SPMV_ACC_ERR_TOO_LARGE.  Returns 0 or an
 * spmv_acc_error code.  CANNOT CHECK: that q is A p, or that d_state and d_partials are those of the spmv_acc_cg_start of this solve.
 * COST: 4 reads + 2 writes + 2 reads of n doubles (p, q; p, q, x, r, and x, r back), two finishes of n / 1024 doubles.  As measured (the
 * same tool and file; 4.0 M rows, cache-warm): 0.047 ms for the four launches, 1.3 x a device copy of those bytes (1.6 x at 3.4 M rows). */
int spmv_acc_cg_update(int n, const double *d_p, const double *d_q, double *d_x, double *d_r, double *d_partials, unsigned long long *d_state,
                       double *d_hist, int hist_cap);

/* ---- conjugate-gradient vector passes, 4: the new direction (new; the per-iteration hot path) ----------------------------------------------------
 * replaces: nothing in the reference.  Three launches: (1) with d_dinv non-NULL the pass first writes z[i] = fl(dinv[i] * r[i]) -- the Jacobi
 * preconditioner fused, no sweep of its own over r -- and takes the partials of r.z from it; with d_dinv == NULL it reads the caller's z = M r
 * (d_z == d_r: no preconditioner); (2) the finish: rz_new; if it is finite and >= 0, beta = rz_new / rz and rz = rz_new, else status = 3 and
 * both are kept; (3) p[i] = z[i] + fl(beta * p[i]).  Frozen as spmv_acc_cg_update is: with a status other than 0 nothing is written.
 * THE ONE CALL THAT FINDS STATUS 3 has, with d_dinv, already written z = dinv r in its launch 1 (and the partials of r.z): that z is left as
 * written, p is kept.  Likewise the update that finds status 2 has written the partials of p.q, and x and r are kept.
 * On the calling thread's library stream: asynchronous, no allocation, no synchronisation, no copy, no host read, no plan; may be captured.
 * CHECKS, on the host, nothing launched: a negative n, null pointers where data is needed, d_p, d_partials or d_state overlapping each other
 * or d_r or d_z, and with d_dinv also d_z overlapping d_r, d_dinv or any of them (d_z == d_r is allowed only without d_dinv):
 * SPMV_ACC_ERR_BAD_ARGUMENT; n beyond INT_MAX - 2^16: SPMV_ACC_ERR_TOO_LARGE.  Returns 0 or an spmv_acc_error code.  CANNOT CHECK: that z is
 * M r for a symmetric positive definite M -- a V-cycle is one only from a zero start with symmetric sweeps --, or that dinv is positive.
 * COST: 2 reads (3 and a write with d_dinv), then 2 reads + 1 write of n doubles, one finish.  As measured (the same tool and file; 4.0 M
 * rows, cache-warm): 0.029 ms, with d_dinv 0.034 ms: 1.3 and 1.1 x a device copy of those bytes. */
int spmv_acc_cg_direction(int n, const double *d_r, double *d_z, const double *d_dinv, double *d_p, double *d_partials,
                          unsigned long long *d_state);

/* ---- row sub-ranges of one matrix as consecutive launches over two streams (new) ------------------------------------------
 * replaces: nothing in the reference (one kernel per SpMV on the NULL stream).  The compute side of the pipelined row-sharded step
 * (spmv_acc_shard_step with pipeline > 1, spmv_acc_amd/dist.py): rows [row_cuts[k], row_cuts[k + 1]) of the matrix are chunk k,
 * handed to the kernels as an un-rebased row sub-range (d_rowptr + row_cuts[k], the whole colindex / value arrays; nnz_ends[k] =
 * rowptr[row_cuts[k + 1]], which the caller reads once); chunk k's kernels go to streams[k & 1] -- consecutive chunks are
 * independent, on one stream each would wait for its predecessor's last wavefront -- and events[k] (a hipEvent_t the caller
 * made; may be NULL) is recorded behind them, so that the caller can send chunk k on its way while chunk k + 1 computes.  ONE
 * host call instead of one per chunk (each costs microseconds of a step that lasts tens).  y_out / y_in as spmv_acc_csr_spmv_oop,
 * indexed by the matrix' rows.  The calling thread's library stream is left as it was.  Returns 0 or the first error. */
int spmv_acc_csr_spmv_chunks(int strategy, double alpha, double beta, int n, int nchunks, const int *row_cuts, const int *nnz_ends,
                             const int *d_rowptr, const int *d_colindex, const double *d_value, const double *dx,
                             const double *dy_in, double *dy_out, void *const *streams, void *const *events);

/* ---- row-block preprocessing pass, device form ---------------------------------------------------------
 * replaces: pre_calc_break_point<STRIDE, BLOCKS, int><<<1024,512>>>(row_ptr, m, break_points, bp_len)
 *           -- src/acc/hip-flat/flat_imp.inl:108-131, launched from flat.cpp:25,43.
 * d_break_points (device, bp_len ints) receives bit-identical values; no pre-zeroing needed.
 * Returns 0, or an error code. */
int spmv_acc_break_points(const int *d_rowptr, int m, int nnz, int stride, int *d_break_points, int bp_len);
int spmv_acc_break_points_len(int nnz, int stride); /* flat.cpp:35-38: ceil(nnz/stride) + 1 */

/* ---- row-block preprocessing pass, host form --------------------------------------------------------------
 * replaces: csr_adaptive_plus_analyze_imp<int, THREADS, VEC>(m, nnz, MIN_NNZ_PER_BLOCK, break_points,
 *           first_block_of_row, host_row_ptr, dev_row_ptr) -- hip-csr-adaptive-plus/csr_adaptive_plus_analyze.cpp:13-98.
 * h_break_points: host, capacity bp_cap (m + 2 + nnz / (2 * min_nnz_per_block) is always enough); h_first_block_of_row: host, m + 1 ints.
 * Returns the number of row blocks, -1 if bp_cap is too small. */
int spmv_acc_adaptive_plus_analyze(int m, int min_nnz_per_block, int threads_per_block, int vec_size,
                                   const int *h_rowptr, int *h_break_points, int bp_cap,
                                   int *h_first_block_of_row);
/* The same analysis on the DEVICE (new): next-block search per row + pointer jumping + scan; bit-identical tables,
 * no host rowptr and no PCIe traffic.  d_break_points: device, bp_cap ints; d_first_block_of_row: device, m + 1 ints.
 * Returns the number of row blocks, -1 if bp_cap is too small, -2 on error.  Synchronises the library stream. */
int spmv_acc_adaptive_plus_analyze_device(int m, int min_nnz_per_block, int threads_per_block, int vec_size,
                                          const int *d_rowptr, int *d_break_points, int bp_cap,
                                          int *d_first_block_of_row);
int spmv_acc_adaptive_plus_vec(int m, int nnz); /* csr_adaptive_plus_spmv.cpp:139-165 */

/* ---- strategy pickers (host logic, no GPU needed) --------------------------------------------------------------
 * replaces: the decision tree of adaptive_sparse_spmv, hip-adaptive/adaptive.cpp:24-66, on the same four
 * inputs rowptr[m/4], rowptr[m/2], rowptr[3m/4], rowptr[m].  Returns 1 vector-row split, 2 adaptive line,
 * 3 adaptive line-enhance, 4 adaptive flat, 5 line-enhance. */
int spmv_acc_adaptive_branch(int m, int rp_quarter, int rp_half, int rp_three_quarter, int rp_last);

/* ---- multi-GPU row-range partition (new; the reference is single-GPU) -----------------------------------------------
 * Contiguous row ranges for `parts` ranks.  mode 0: equal row counts (what an allgather of equal-sized
 * y shards needs); mode 1: nnz-balanced boundaries found by binary search on rowptr.
 * h_rowptr: host rowptr (may be NULL for mode 0).  row_begin: out, parts + 1 entries. */
int spmv_acc_partition_rows(int m, int parts, int mode, const int *h_rowptr, int *row_begin);

/* ---- one rank's step of the row-sharded SpMV, behind the C boundary (new) ---------------------------------------------------
 * replaces: nothing in the reference (single GPU: hipSetDevice(0) at cli/main.cpp:89, no collective anywhere); BASELINE's
 * north_star adds the row-range partition with an RCCL allgather of the y sub-vectors.  spmv_acc_amd/dist.py does this with
 * torch.distributed; this entry gives C / C++ consumers (one process or one thread per GPU) the same step:
 *     y_local[0 .. m_local) = alpha * A_local * x + beta * y_local          (this rank's rows, any strategy)
 *     ncclAllGather(y_local, y_full, m_pad doubles, comm, library stream)   (ONE collective per SpMV, behind the kernels)
 * nccl_comm: the caller's ncclComm_t.  The library resolves ncclAllGather at run time from the RCCL the process already has
 * (dlopen RTLD_NOLOAD of librccl.so.1 / librccl.so, else a fresh dlopen; environment variable SPMV_ACC_RCCL_LIB names a
 * particular file), so libspmv_acc.so keeps linking only the HIP runtime.  y_local holds m_pad >= m_local doubles (every rank
 * the same m_pad: RCCL has no allgatherv; rows past m_local are padding the caller zeroes once), y_full holds
 * world * m_pad doubles; rank r's rows land at y_full + r * m_pad.  Returns 0 or an error code (SPMV_ACC_ERR_NO_DEVICE when
 * no RCCL can be found, SPMV_ACC_ERR_HIP when the collective fails). */
int spmv_acc_sharded_spmv(void *nccl_comm, int strategy, double alpha, double beta, int m_local, int m_pad, int n, int nnz_local,
                          const int *h_rowptr, const int *d_rowptr, const int *d_colindex, const double *d_value, const double *dx,
                          double *dy_local, double *dy_full);

/* ---- the same step with a per-rank handle: in place, out of place, pipelined (new) ---------------------------------------------
 * replaces: nothing in the reference (single GPU).  One handle per rank and matrix, made by the host thread that drives the GPU
 * (hipSetDevice first; the library stream is per host thread).  A step
 *     y_full[rank * m_pad + i] = alpha * (A_local * x)[i] + beta * y_in_local[i]      i in [0, m_local)
 * computes this rank's rows straight into their place in the gathered vector -- dy_in_local (m_local doubles; NULL = that place
 * itself, i.e. in place) is read by the out-of-place kernels, so no slice is ever copied -- and then every rank receives every
 * slice, in place:
 *   pipeline <= 1: ONE ncclAllGather (send buffer = this rank's slice of dy_full) on the library stream, behind the kernels;
 *   pipeline  = C: the local rows are cut into C chunks -- row sub-ranges of the caller's own arrays, nothing is copied or rebased; their
 *                  kernels alternate over two streams of the shard's own (consecutive chunks are independent);
 *                  chunk c's slice travels -- grouped ncclSend / ncclRecv with every peer, straight to its place in their
 *                  vectors, on a second stream -- as soon as its kernels have finished, while chunk c+1 computes.  This is the
 *                  overlap that survives when the next x depends on the gathered y.  The library stream waits for the last
 *                  arrival, so work enqueued after the step sees the whole vector.
 * Rows [m_local, m_pad) of a slice are padding: zero dy_full once.  dy_full holds world * m_pad doubles (world and rank are
 * the communicator's).  RCCL is resolved at run time as in spmv_acc_sharded_spmv.  Returns 0 or an error code.
 * spmv_acc_rccl_comm_init_all / _destroy: ncclCommInitAll / ncclCommDestroy through the same run-time binding, for a
 * one-process driver that must not link RCCL either (spmv-cli --gpus N); devices may be NULL (0 .. ndev-1). */
typedef struct spmv_acc_shard *spmv_acc_shard_t;
int spmv_acc_shard_create(spmv_acc_shard_t *out, void *nccl_comm, int strategy, int m_local, int m_pad, int n, int nnz_local,
                          const int *d_rowptr, const int *d_colindex, const double *d_value, int pipeline);
int spmv_acc_shard_step(spmv_acc_shard_t shard, double alpha, double beta, const double *dx, const double *dy_in_local,
                        double *dy_full);
/* Builds and tunes every chunk's plan for the beta class of `beta` (beta == 0 / beta != 0) with x = dx, so that the steps only enqueue: plan
 * building allocates, frees and synchronises, which must not fall between the exchanges of a step the peers are already in.  No collective
 * inside; every rank calls it once before its first step (spmv-cli --gpus N does).  A rank whose local SpMV fails inside a step still takes
 * part in all of that step's exchanges and reports its error afterwards: the peers are never left waiting in a collective. */
int spmv_acc_shard_prepare(spmv_acc_shard_t shard, double beta, const double *dx);
int spmv_acc_shard_pipeline(spmv_acc_shard_t shard); /* chunks per step actually in use */
int spmv_acc_shard_destroy(spmv_acc_shard_t shard);
int spmv_acc_rccl_comm_init_all(void **comms, int ndev, const int *devices);
int spmv_acc_rccl_comm_destroy(void *comm);

/* ---- host staging (new; replaces the pageable blocking hipMemcpy of cli/utils.hpp:94-117) ----------------------------
 * Copies host CSR arrays + vectors to freshly hipMalloc'ed device buffers: the caller's arrays are pinned in place
 * (hipHostRegister) and sent with hipMemcpyAsync on a private copy stream, all transfers in flight together; an
 * array that cannot be pinned goes through a pinned double buffer.  Any of the host pointers
 * may be NULL to skip that array.  Free with spmv_acc_free_device. */
int spmv_acc_stage_csr(int m, int n, int nnz, const int *h_rowptr, const int *h_colindex, const double *h_value,
                       const double *h_x, const double *h_y, int **d_rowptr, int **d_colindex, double **d_value,
                       double **d_x, double **d_y);
int spmv_acc_free_device(void *p);

/* ---- explicit preprocessing (new) ---------------------------------------------------------------------------------------
 * Builds everything the FIRST call on a matrix would build for `strategy` -- the structural passes (break points, row-block
 * analysis, balance probe) and the per-matrix timings (cache policy, flat's cut-row form, adaptive-plus block size) -- by
 * running that first call into a zeroed scratch y (alpha = beta = 1, the reference's protocol), then synchronises.  The caller's y is not touched; x is read.
 * After it every spmv call on the matrix is kernel launches only (capturable into a hipGraph).  ms_out (may be NULL):
 * device time of the preparation, the figure the reference's benchmark reports as `pre` (benchmark_time.cpp:23-43;
 * there it is the per-call break-point / analysis cost, here it is paid once).
 * replaces: nothing callable in the reference (its preprocessing is re-done inside every SpMV call, flat.cpp:35-45,
 * csr_adaptive_plus_spmv.cpp:104-125). */
int spmv_acc_prepare(int strategy, int m, int n, int nnz, const int *h_rowptr, const int *d_rowptr, const int *d_colindex,
                     const double *d_value, const double *dx, float *ms_out);
/* The same for the beta class the caller will run in: the choices that depend on whether y is read (stream cache policy,
 * adaptive's kernel family, flat's cut-row form) are timed and kept PER CLASS (beta == 0: y only written; beta != 0: read too).
 * spmv_acc_prepare is the beta != 0 class (the reference's protocol, alpha = beta = 1).  A class that was never prepared is
 * timed by its first call -- or, inside a stream capture, runs with the other class' choices. */
int spmv_acc_prepare_beta(int strategy, double beta, int m, int n, int nnz, const int *h_rowptr, const int *d_rowptr,
                          const int *d_colindex, const double *d_value, const double *dx, float *ms_out);

/* ---- persistent choices + the deterministic switch (new) -------------------------------------------------------------------
 * The reference's strategy choice is a pure function of its inputs (strategy_picker.cpp:19-65, adaptive.cpp:24-66) and costs
 * nothing; this library times a handful of choices on each matrix' first call (cache policy, kernel family, tile geometry: up
 * to 13 ms on the headline matrix), per process.  Two opt-in ways out:
 *   spmv_acc_set_tune_cache(path) / environment SPMV_ACC_TUNE_CACHE=<file>: the choices are appended to a text file, one line per
 *     matrix, keyed by a digest of (library version, device name, m, n, nnz, 64 rowptr samples); a later process that meets the
 *     same matrix on the same device adopts them and only runs the structural passes (NULL or "" switches it off);
 *   tunable "deterministic" = 1 / environment SPMV_ACC_DETERMINISTIC=1: nothing is timed at all, every choice follows a fixed
 *     rule on the matrix' shape -- y is then bitwise equal across processes and runs (the kernels never use atomics; the one
 *     exception, spmv_acc_csr_spmv_t, adds with fp64 atomics and is therefore refused under this switch).
 * Round 6: with the default ("deterministic" = 0) the calls made BEFORE a plan is settled are answered by that same rule (the plan's rule twin)
 * while the timings advance beside them against a scratch y; from the first settled call on the timed choices serve.  y changes its last bits at
 * most once per (matrix, strategy, beta class), at a call spmv_acc_query_plan_settled shows.  "deterministic" = -1: as rounds 2-5 (the timed
 * choices as far as they have come serve from the first call on). */
void spmv_acc_set_tune_cache(const char *path);

/* ---- values changed in place, with the opt-in column slabs in use (new) ---------------------------------------------------------
 * Every plan survives in-place edits of `value` (the reference keeps nothing between calls) -- except the one opt-in mode whose plan
 * holds a re-ordered COPY of the matrix (tunable col_slabs).  After changing values in place, call this instead of dropping the plan:
 * one scatter pass re-copies the values into the slabs (enqueued on the calling thread's library stream, ordered before later
 * SpMVs on it); the slabs' structure, plans and timed choices stay.  Returns the number of plans refreshed (0: the matrix has no
 * slabs, nothing to do).  A changed STRUCTURE (rowptr / colindex) still needs spmv_acc_release_plans. */
int spmv_acc_refresh_values(const int *d_rowptr);

/* Host microseconds the calling thread's most recent SpMV call spent preparing its matrix (structural passes + per-matrix
 * timings of the FIRST call on a matrix); 0 when the plan already existed.
 * replaces: BenchmarkTime::pre of the reference's harness (benchmark/utils/benchmark_time.cpp:23-43,
 * benchmark/flat/spmv_acc_flat.cpp:20-71: the break-point pass timed on EVERY call there) and
 * SpMVAccHanele::profile_analyze_time (csr_adaptive_plus_spmv.cpp:98-128). */
double spmv_acc_last_prepare_us(void);

/* ---- plan cache, stream, errors ------------------------------------------------------------------------------------------
 * Preprocessing results (break points, row blocks, carries) are cached per matrix, keyed by
 * (device, rowptr, colindex, value, m, n).  Release when a matrix' structure changes in place or its
 * buffers are freed; NULL releases everything.
 * Stale-plan guard: the reference recomputes its preprocessing on every call (hip-flat/flat.cpp:39-44), so its callers
 * never announce a change.  Every plan therefore records 64 strided rowptr entries (rowptr[0] .. rowptr[m] = nnz);
 * the first wavefront of every SpMV kernel re-reads them and raises a sticky flag (pinned host memory, no
 * synchronisation) when the matrix behind the pointers is no longer the one the plan was built for -- buffers freed
 * and re-allocated at the same addresses for another matrix of the same shape, or a structure rewritten in place.
 * spmv_acc_last_error() (after the caller's synchronisation) and the next call on those pointers then report
 * SPMV_ACC_ERR_BAD_ARGUMENT ("... changed ..."): the y of the call that ran on the stale plan is invalid, the plan
 * is dropped and the next call builds a fresh one before it runs.  Values edited in place never trip the guard
 * (plans hold no copy of colindex or values).  A change that leaves all 64 samples untouched is not seen: callers
 * that permute a few rows in place still have to call spmv_acc_release_plans. */
void spmv_acc_release_plans(const int *d_rowptr);
int spmv_acc_cached_plans(void);
/* spmv_acc_last_error() asks the plan the CALLING THREAD used last (one load, no lock).  This one looks at every cached plan,
 * any thread's: drops the stale ones, returns how many there were (and records SPMV_ACC_ERR_BAD_ARGUMENT if any).  Call after a
 * device synchronisation. */
int spmv_acc_check_plans(void);
/* plan introspection: fills out[9] = {nnz, adaptive_branch, vec, flat_tiles, plus_blocks, aligned16, stream_policy,
 * flat_fixup, adaptive_family};
 * stream_policy: cache policy of the stream loads chosen by timing at plan time (0 nt, 1 default, 3 values default,
 * -1 not tuned yet); flat_fixup: 1 the flat plan folds cut rows with its fix-up kernel, 0 tiles finish them, -1 no flat
 * plan yet; adaptive_family: the kernel family adaptive settled on by timing (0 fixed row blocks, 1 row-block-plus, 2 flat,
 * -1 not timed); returns 1 if a plan exists */
int spmv_acc_query_plan(const int *d_rowptr, int m, int *out);
/* adaptive's timed kernel family for the beta == 0 class alone (out[8] above reports the beta != 0 class when it has been
 * timed): the families are timed per class because the ranking changes with the y read; -2 = no such plan */
int spmv_acc_query_plan_beta0(const int *d_rowptr, int m);
/* number of column slabs whose run lists the plan holds and its SpMVs pass over (tunable slab_segments, k_segment.hip: column-slab
 * blocking without a copy of the matrix -- chosen by a plan-time timing on matrices whose column census finds a hot set, or forced);
 * 0 = the plan runs the named strategy's own kernel; -2 = no such plan.  No reference counterpart: the reference has one path per
 * strategy (strategy_picker.cpp:19-65). */
int spmv_acc_query_plan_slab_passes(const int *d_rowptr, int m);
/* 1: the latest call on this plan left none of its per-matrix timings open -- the plan is settled, calls are launches only and bitwise stable;
 * 0: the first-call budget (tunable first_call_budget) deferred some, the next calls resume them (or call spmv_acc_prepare); that call was answered
 * by the plan's rule twin (round 6), as the following ones are until one returns 1 here; -2 = no such plan.
 * No reference counterpart (the reference times nothing). */
int spmv_acc_query_plan_settled(const int *d_rowptr, int m);
/* Did the plan's LATEST SpMV read the plan's 16-bit column encoding instead of colindex (round 6; tunable col16, default: timed per matrix and
 * kernel family)?  16 / 32 / 64 = yes, with that many ints per 256-non-zero chunk record; 0 = no (the caller's colindex was streamed);
 * -1 = no SpMV yet; -2 = no such plan.  A plan that uses the encoding holds structure derived from colindex: after editing column indices in
 * place (same rowptr) call spmv_acc_release_plans (64 samples of colindex are re-checked by every launch, like rowptr's).  No reference counterpart:
 * the reference streams one 4-byte column per non-zero (hip-flat/flat_imp_one_pass.hpp:35-39, hip-line-enhance/line_enhance_spmv_imp.inl:55-62). */
int spmv_acc_query_plan_col16(const int *d_rowptr, int m);
/* The code width of that encoding (round 7): 16 or 8 bits per non-zero (8: where a chunk's near columns lie within 255 of each other -- the plan
 * picks the width by rule from its escape statistics, tunable col16 = 8 / 2 pins 8- / 16-bit codes); 0 = the caller's colindex was streamed;
 * -1 = no SpMV yet; -2 = no such plan. */
int spmv_acc_query_plan_col_bits(const int *d_rowptr, int m);
/* Which kernel ran the plan's LATEST SpMV (round 5).  The reference's strategy name IS its kernel (strategy_picker.cpp:19-65); here a name selects a
 * policy by default (`flat` may run the row-block kernel where it timed faster, `line_enhance` the column-slab passes on power-law columns) and
 * tunable strict_strategy = 1 (SPMV_ACC_TUNABLES=strict_strategy=1) binds the name to its algorithm.  -1 = no SpMV yet, -2 = no such plan. */
enum spmv_acc_kernel {
  SPMV_ACC_KERNEL_ROWBLOCK = 0,    /* rowblock_stream_kernel: line_enhance / line / thread_row / default (line_enhance_spmv_imp.inl:12-95) */
  SPMV_ACC_KERNEL_ROWBLOCK_PLUS = 1, /* plus_kernel: adaptive_plus, and the row-block family's rescue of unbalanced rows (csr_adaptive_plus_spmv_imp.inl:31-205) */
  SPMV_ACC_KERNEL_FLAT_TILE = 2,   /* flat_tile_kernel (+ fix-up): flat (flat_imp_one_pass.hpp:16-77) */
  SPMV_ACC_KERNEL_SLAB_PASSES = 3, /* segment_tile_kernel passes over the plan's run lists (no reference counterpart) */
  SPMV_ACC_KERNEL_VECTOR_TILE = 4, SPMV_ACC_KERNEL_VECTOR_ROW = 5, SPMV_ACC_KERNEL_WAVE_ROW = 6, SPMV_ACC_KERNEL_LIGHT = 7,
  SPMV_ACC_KERNEL_BLOCK_ROW = 8, SPMV_ACC_KERNEL_COL_SLABS = 9, SPMV_ACC_KERNEL_SCALE_ONLY = 10
};
int spmv_acc_query_plan_last_kernel(const int *d_rowptr, int m);

void spmv_acc_set_stream(void *hip_stream); /* hipStream_t; NULL = the NULL stream (reference behaviour).  The stream belongs to the
                                             * CALLING HOST THREAD, like HIP's current device: N threads driving N GPUs each set
                                             * their own and cannot redirect one another.  Steady-state calls are
                                             * launches only and may be captured into a hipGraph; the first call on a matrix
                                             * (plan: allocations, synchronisation, timings) must run outside a capture: a call that
                                             * would need such work inside a capture enqueues nothing and reports
                                             * SPMV_ACC_ERR_BAD_ARGUMENT (timed choices that are merely missing are skipped instead).
                                             * A thread that never set a stream launches on the NULL stream; if another thread HAS set
                                             * one, the first such launch prints a one-time note on stderr (SPMV_ACC_QUIET=1: none).
                                             * A plan remembers the stream of its latest call to order a call on another stream behind
                                             * it: before destroying a stream, synchronise it or release the plans used on it.
                                             * Captured graphs bypass that ordering: a plan owns scratch its kernels write (flat's
                                             * carries, the slab passes' partial sums, LIGHT's row counter), so two graphs that hold
                                             * SpMVs of ONE matrix must not be replayed concurrently on two streams.
                                             * The first call on a matrix spends at most ~20 SpMV-equivalents on per-matrix timings
                                             * (tunable first_call_budget) and the following calls finish them; until they have, two
                                             * calls may run different kernels, i.e. sum in a different order -- spmv_acc_prepare
                                             * settles everything up front, tunable deterministic times nothing at all. */
void *spmv_acc_get_stream(void);

int spmv_acc_last_error(void); /* 0 = ok; see enum below.  Per host thread, like errno. */
const char *spmv_acc_last_error_string(void);
void spmv_acc_clear_error(void);
enum spmv_acc_error {
  SPMV_ACC_OK = 0,
  SPMV_ACC_ERR_UNSUPPORTED_TRANS = 1,
  SPMV_ACC_ERR_BAD_ARGUMENT = 2,
  SPMV_ACC_ERR_HIP = 3,
  SPMV_ACC_ERR_TOO_LARGE = 4,
  SPMV_ACC_ERR_UNKNOWN_STRATEGY = 5,
  SPMV_ACC_ERR_NO_DEVICE = 6
};

/* ---- measurement helper ----------------------------------------------------------------------------------------------------
 * replaces: hip::timer::event_timer around the L1 call (benchmark/utils/timer_utils.h:16-51,
 * benchmark/csr_spmv.hpp:67-74).  Runs `iters` SpMVs with `strategy`; each is bracketed by hipEvents on
 * the library stream, y is restored from d_y0 (device, m doubles, may be NULL) outside the timed region -- by a non-temporal copy kernel
 * (round 5: like the DMA write of the reference's hipMemcpy reset, csr_spmv.hpp:68, it parks nothing in the L2s; env SPMV_ACC_RESET_NT=0: the
 * default-policy copy of rounds 1-4, SPMV_ACC_RESET_MEMCPY=1: hipMemcpyAsync device -> device).
 * ms_out receives iters per-launch durations in milliseconds.  Returns 0 or an error code.  What is timed is a SETTLED plan: the helpers
 * first finish whatever per-matrix timings the first-call budget left open (spmv_acc_prepare_beta: at least one untimed SpMV into a scratch y).
 * d_y0 == NULL: no reset, the launches accumulate into y (as the launches of spmv_acc_time_spmv_total / _region do).  The reset writes dy[0 .. m) and
 * nothing else, whatever the alignment of dy and d_y0 (both on a 16-byte line: the copy kernel, with a one-workgroup tail for the last double of an
 * odd m; else hipMemcpyAsync).
 * REFUSALS, the same for every spmv_acc_time_* entry below: iters <= 0 or a NULL result pointer (ms_out / total_ms_out / kernel_ms_out):
 * SPMV_ACC_ERR_BAD_ARGUMENT; a strategy id no strategy has (e.g. the -1 of spmv_acc_parse_strategy): SPMV_ACC_ERR_UNKNOWN_STRATEGY.  Either way
 * nothing is launched and nothing is written, neither to y nor to a result.  m == 0: returns 0 and launches no SpMV; y is not touched and the
 * times are those of the empty protocol (finite, >= 0). */
int spmv_acc_time_spmv(int strategy, int iters, double alpha, double beta, int m, int n, int nnz,
                       const int *h_rowptr, const int *d_rowptr, const int *d_colindex, const double *d_value,
                       const double *dx, double *dy, const double *d_y0, float *ms_out);

/* The same with the events' creation flags chosen by the caller (hipEventCreateWithFlags): 0 = hipEventDefault, what
 * benchmark/utils/timer_utils.h:16-51 creates and what every gate of this repository is quoted on.  hipEventDisableSystemFence
 * (0x20000000) takes the system-scope fence -- a cache write-back and invalidation -- out of the event, which HIP documents as the
 * more accurate form for events that only measure time; on MI355X it is 1.2 us of the ~6.7 us an almost empty launch takes between
 * default events, and it leaves the L2s warm for the timed launch.  Reported beside the default figure, never instead of it. */
int spmv_acc_time_spmv_events(int strategy, int iters, double alpha, double beta, int m, int n, int nnz,
                              const int *h_rowptr, const int *d_rowptr, const int *d_colindex, const double *d_value,
                              const double *dx, double *dy, const double *d_y0, float *ms_out, unsigned event_flags);

/* The per-launch protocol with a COLD cache hierarchy (round 6; context for every fraction, never a gate): after y has been restored and before the
 * start event, flush_bytes of scratch traffic under the default cache policy (the copy kernel: second half of d_flush overwritten with the first)
 * displace what the previous launch left in the L2s and the 256 MB Infinity Cache.  The reference's protocol (benchmark/csr_spmv.hpp:49-74) repeats
 * one SpMV on one matrix, so its launches start in whatever the previous one left; this entry says how much of a figure that is.  d_flush: device
 * memory, 16-byte aligned, flush_bytes >= 2 x the Infinity Cache (the bench passes 1 GiB).  With half = flush_bytes / 2 / 16 * 16 the copy writes
 * bytes [half, 2 * half) of d_flush from bytes [0, half) and touches no other byte.  d_flush == NULL, flush_bytes < 32 or a d_flush off a 16-byte
 * line: SPMV_ACC_ERR_BAD_ARGUMENT ("... 16-byte aligned ..."), nothing is launched or written.  No reference counterpart. */
int spmv_acc_time_spmv_cold(int strategy, int iters, double alpha, double beta, int m, int n, int nnz,
                            const int *h_rowptr, const int *d_rowptr, const int *d_colindex, const double *d_value,
                            const double *dx, double *dy, const double *d_y0, void *d_flush, long long flush_bytes, float *ms_out);

/* One event pair around all `iters` back-to-back launches (no per-launch markers): *total_ms_out / iters is
 * the average launch duration a solver loop sees. */
int spmv_acc_time_spmv_total(int strategy, int iters, double alpha, double beta, int m, int n, int nnz,
                             const int *h_rowptr, const int *d_rowptr, const int *d_colindex, const double *d_value,
                             const double *dx, double *dy, float *total_ms_out);
/* The per-launch protocol once more, with the library's KERNEL CLOCK on (round 5): event_ms_out[i] (may be NULL) is the event pair around call i as
 * above -- the reference harness's figure, which also holds the protocol's floor (two marker packets and the dispatch latency: ~4-7 us on MI355X) --
 * and kernel_ms_out[i] the sum of the durations of the kernels call i launched, each read from the dispatch's own begin / end timestamps
 * (hipExtLaunchKernelGGL start / stop events: what rocprofv3 --kernel-trace reports).  launches_out[i] (may be NULL): kernels per call.
 * replaces: nothing in the reference (its harness has the event pair only, benchmark/utils/timer_utils.h:16-51). */
int spmv_acc_time_spmv_kernels(int strategy, int iters, double alpha, double beta, int m, int n, int nnz,
                               const int *h_rowptr, const int *d_rowptr, const int *d_colindex, const double *d_value,
                               const double *dx, double *dy, const double *d_y0, float *event_ms_out, float *kernel_ms_out, int *launches_out);
/* The same region and NOTHING else (round 5): no plan work -- the caller settles the plan first (spmv_acc_prepare_beta) --, no allocation, the
 * event pair is made once per host thread.  A wall clock around this call, between two device synchronisations, reads the K launches' own time
 * (bench.py's `value` / `ms_per_step`: median over repeated regions, the reference's median rule, benchmark/utils/benchmark_time.cpp:23-43).
 * A region that did plan work after all (no spmv_acc_prepare_beta in the call's beta class since the plan was made or released) returns
 * SPMV_ACC_ERR_BAD_ARGUMENT ("... the plan was not settled ..."): y holds the `iters` launches' result and *total_ms_out is written, but it
 * holds the plan work too. */
int spmv_acc_time_spmv_region(int strategy, int iters, double alpha, double beta, int m, int n, int nnz,
                              const int *h_rowptr, const int *d_rowptr, const int *d_colindex, const double *d_value,
                              const double *dx, double *dy, float *total_ms_out);
/* Streaming-copy ceiling (GB/s, read + write bytes) with the kernels' 16-B non-temporal access shape;
 * replaces: the WITH_MEM_BANDWIDTH macros of src/acc/common/mem_bandwidth.hpp:13-38 as the yardstick.
 * Copies bytes / 16 * 16 bytes from d_src to d_dst (both 16-byte aligned, not overlapping) and writes nothing beyond; best of `reps` after one
 * warm-up.  A NULL pointer, bytes < 16 or reps <= 0: returns -1.0 and launches nothing (also -1.0 when a HIP call fails). */
double spmv_acc_copy_ceiling_gbs(void *d_dst, const void *d_src, long long bytes, int reps);

/* ---- switches (new) -------------------------------------------------------------------------------------------------
 * A/B knobs for tools/kbench.py ("xcd_chunk", "rowblock_target", "stream_plain", "flat_finish", "flat_npt", ...; the table
 * with every default is in spmv_acc_amd/csrc/config.cpp) and one behavioural switch:
 *   "validate" (0): 1 = check rowptr / colindex of every new matrix on the device before the first launch (rowptr
 *   monotone and non-negative, rowptr[m] == nnz, 0 <= colindex < n); a matrix that fails is refused with
 *   SPMV_ACC_ERR_BAD_ARGUMENT on this and every later call and y is left untouched.  One pass over the indices per
 *   matrix; the reference has no counterpart (its kernels read through whatever the caller passes).
 * Defaults are the shipped configuration; unknown names return -1.  The environment variable
 * SPMV_ACC_TUNABLES="name=value,name=value" seeds the defaults at load time, for executables that cannot call the setter
 * (the reference's spmv-cli / benchmark linked against this library). */
int spmv_acc_set_tunable(const char *name, int value);
int spmv_acc_get_tunable(const char *name);
void spmv_acc_reset_tunables(void);

const char *spmv_acc_version(void);

#ifdef __cplusplus
}
#endif

#endif /* SPMV_ACC_C_ABI_H */
