// k_spgemm.hip -- the kernels of the device CSR SpGEMM C = A * B (size rules, the expansion and summation orders and launcher declarations
// in spgemm.hpp, engine in spgemm.cpp).
//
// No reference counterpart: hpcde/spmv-acc multiplies a matrix by a vector.
//
// Expand - sort - compress.  The scalar products a_ik * b_kj are listed as (i, j) keys in a fixed order, and from there the product IS the
// assembly of k_coo.hip: its stable sort, run heads, scan, entries and row pointer run unchanged on these keys.  New here:
//
// 1. Counts (spgemm_counts_kernel): per non-zero q of A the length of B's row a_colindex[q] (64-bit, so that a total past 2^31 is still a
//    number) and the row of A that holds q.  rocPRIM then reduces (the count entry) or scans (the main entry) them.
//
// 2. Expansion (spgemm_expand_kernel), PRODUCT-parallel: the stream of products is cut into tiles of kSpgemmExpandTile, a wavefront owns
//    kSpgemmExpandChunk consecutive products, finds the non-zeros of A that hold its first and last product by binary search in the scan, and
//    each lane finds its own between the two.  A wavefront inside one long row of B searches nothing further; a row of 10^5 entries is 391
//    wavefronts, not 10^5 steps of a lane.  Writes the packed key of every product; no factor position is kept (8 B per product).
//
// 3. Map (spgemm_map_kernel), after the sort: sorted position p holds product e = order[p]; its non-zero q of A is found again by binary search
//    in the scan -- inside row i of A, which the sorted key names, so a handful of steps in lines the neighbours share -- and t follows.  The
//    pass rewrites the sort's order array in place as pa and writes pb.
//
// 4. Values (spgemm_values_kernel, the per-step hot path and the first call's last launch): the body coo_values_kernel runs (structure_passes.hpp
//    sum_runs: its tiling and summation order) on SpgemmTerms, the gather replaced by two index loads, two gathers and a product rounded on its
//    own (fp contraction is off in the product and in the shared sums: a fused multiply-add would round once where the definition rounds twice).  Streams start, pa and pb (4 B per entry, 8 B per product), gathers 16 B
//    per product, writes 8 B per entry.  Four entries per lane: spgemm.hpp kSpgemmPerLane.  The sums depend on the map and the values alone (no
//    atomics), so the same values give the same bits.
#include "spgemm.hpp"
#include "structure_passes.hpp"

#include <rocprim/device/device_reduce.hpp>
#include <rocprim/device/device_scan.hpp>

namespace spmv_acc {
namespace {

using namespace dev;
using namespace passes;

typedef unsigned long long u64;

// (last_at_most in the scan `off`: the non-zero of A whose products include e; non-zeros without products, off[q] == off[q + 1], are passed over.
// A column of A names a row of B: it has passed the census, 0 <= c < k, and row_extent holds the row inside B's arrays)

__global__ __launch_bounds__(kThreads) void spgemm_counts_kernel(int m, int nnz_a, const int *__restrict__ a_rowptr,
                                                                 const int *__restrict__ a_colindex, const int *__restrict__ b_rowptr, int nnz_b,
                                                                 long long *__restrict__ count, int *__restrict__ arow) {
  const long long stride = static_cast<long long>(gridDim.x) * kThreads;
  for (long long q = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; q <= nnz_a; q += stride) {
    if (q == nnz_a) {
      count[q] = 0; // (the scan's closing element)
      continue;
    }
    int hi;
    const int lo = row_extent(b_rowptr, nnz_b, a_colindex[q], &hi);
    count[q] = hi - lo;
    if (arow != nullptr) arow[q] = last_at_most(a_rowptr, 0, m - 1, q); // (stays inside a_rowptr[0 .. m) whatever it holds)
  }
}

// One workgroup per tile of kSpgemmExpandTile products, blocks stride over the tiles beyond the grid.  nnz_a > 0, 0 < nprod == off[nnz_a].
__global__ __launch_bounds__(kThreads) void spgemm_expand_kernel(int nnz_a, int nprod, const long long *__restrict__ off,
                                                                 const int *__restrict__ arow, const int *__restrict__ a_colindex,
                                                                 const int *__restrict__ b_rowptr, int nnz_b, const int *__restrict__ b_colindex,
                                                                 int col_bits, u64 *__restrict__ keys) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const long long ntiles = (static_cast<long long>(nprod) + kSpgemmExpandTile - 1) / kSpgemmExpandTile;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) { // (block-uniform)
    const long long base = tile * kSpgemmExpandTile + static_cast<long long>(wave) * kSpgemmExpandChunk;
    if (base >= nprod) continue; // (wave-uniform)
    const long long last = (base + kSpgemmExpandChunk < nprod ? base + kSpgemmExpandChunk : nprod) - 1;
    // the non-zeros of A that hold the wavefront's first and last product (every lane the same search), then each lane's between them
    int q_last;
    const int q_first = wave_end_rows(off, nnz_a, base, last, &q_last);
#pragma unroll
    for (int k = 0; k < kSpgemmExpandPerLane; ++k) {
      const long long e = base + k * kWave + lane;
      if (e > last) continue;
      const int q = last_at_most(off, q_first, q_last, e);
      int hi;
      const int lo = row_extent(b_rowptr, nnz_b, a_colindex[q], &hi);
      const int len = hi - lo;
      long long step = e - off[q]; // (0 <= step < len by the scan; held to it so that no array content can move t outside B's arrays)
      step = step >= len ? len - 1 : step;
      const int t = lo + static_cast<int>(step < 0 ? 0 : step);
      keys[e] = static_cast<u64>(static_cast<unsigned>(arow[q])) << col_bits | static_cast<unsigned>(b_colindex[t < nnz_b ? t : nnz_b - 1]);
    }
  }
}

// pa holds the sort's order on entry.  nnz_a > 0, nnz_b > 0, nprod == off[nnz_a] > 0; the keys' rows are arow values: inside [0, m)
__global__ __launch_bounds__(kThreads) void spgemm_map_kernel(int m, int nnz_a, int nprod, const u64 *__restrict__ keys, int col_bits,
                                                              const long long *__restrict__ off, const int *__restrict__ a_rowptr,
                                                              const int *__restrict__ a_colindex, const int *__restrict__ b_rowptr, int nnz_b,
                                                              int *__restrict__ pa, int *__restrict__ pb) {
  const long long stride = static_cast<long long>(gridDim.x) * kThreads;
  for (long long p = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; p < nprod; p += stride) {
    long long e = pa[p]; // (written by the sort from a counting iterator: 0 <= e < nprod)
    e = e < 0 ? 0 : (e >= nprod ? nprod - 1 : e);
    int i = static_cast<int>(keys[p] >> col_bits);
    i = i < 0 ? 0 : (i >= m ? m - 1 : i);
    int lo = a_rowptr[i], hi = a_rowptr[i + 1] - 1; // row i of A, held inside A's arrays
    lo = lo < 0 ? 0 : (lo > nnz_a - 1 ? nnz_a - 1 : lo);
    hi = hi < lo ? lo : (hi > nnz_a - 1 ? nnz_a - 1 : hi);
    const int q = last_at_most(off, lo, hi, e); // (with an a_rowptr that does not ascend: some non-zero of A, and t below is held inside B)
    int b_hi;
    const int b_lo = row_extent(b_rowptr, nnz_b, a_colindex[q], &b_hi);
    const int len = b_hi - b_lo;
    long long step = e - off[q];
    step = step >= len ? len - 1 : step;
    const int t = b_lo + static_cast<int>(step < 0 ? 0 : step);
    pa[p] = q;
    pb[p] = t < nnz_b ? t : nnz_b - 1;
  }
}

// the terms of the product's runs: the rounded product of sorted position p (0 <= p < nprod).  The map is the caller's and carries no lengths:
// pa / pb are not checked
struct SpgemmTerms {
  struct Pair {
    int a, b;
  };
  struct Factors {
    double a, b;
  };
  const int *__restrict__ pa;
  const int *__restrict__ pb;
  const double *__restrict__ a_value;
  const double *__restrict__ b_value;
  __device__ __forceinline__ Pair index(int p) const { return {pa[p], pb[p]}; }
  __device__ __forceinline__ Factors load(Pair u) const { return {a_value[u.a], b_value[u.b]}; }
  __device__ __forceinline__ double term(Pair, Factors v) const {
#pragma clang fp contract(off)
    const double prod = v.a * v.b; // rounded here, added by the caller
    return prod;
  }
  __device__ __forceinline__ double fetch(int p) const {
    const Pair u = index(p);
    return term(u, load(u));
  }
};

static_assert(kSpgemmWaveChunk == kWave * kSpgemmPerLane && kSpgemmTile == (kThreads / kWave) * kSpgemmWaveChunk,
              "sum_runs derives its tile from kSpgemmPerLane");

// One workgroup per tile of kSpgemmTile C entries, blocks stride over the tiles beyond the grid.  nprod > 0 (the launcher checks).
// (waves_per_eu: the kernel asks for the eighth wave per SIMD; the compiler then orders the loads to fit 64 VGPRs without scratch)
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(8, 8))) void spgemm_values_kernel(int nprod, int nnz_c, const int *__restrict__ pa, const int *__restrict__ pb,
                                                                 const int *__restrict__ start, const double *__restrict__ a_value,
                                                                 const double *__restrict__ b_value, double *__restrict__ value) {
  sum_runs<kSpgemmPerLane>(nprod, nnz_c, start, SpgemmTerms{pa, pb, a_value, b_value}, value);
}

} // namespace

void launch_spgemm_counts(hipStream_t stream, int m, int nnz_a, const int *a_rowptr, const int *a_colindex, const int *b_rowptr, int nnz_b,
                          long long *count, int *arow) {
  if (nnz_a <= 0 || m <= 0) return;
  SPMV_ACC_LAUNCH(spgemm_counts_kernel, dim3(grid_for(static_cast<long long>(nnz_a) + 1, kThreads)), dim3(kThreads), 0, stream, m, nnz_a,
                  a_rowptr, a_colindex, b_rowptr, nnz_b, count, arow);
}

bool launch_spgemm_reduce(hipStream_t stream, const long long *count, int nnz_a, long long *total, void *tmp, size_t *tmp_bytes) {
  return rocprim::reduce(tmp, *tmp_bytes, count, total, 0LL, static_cast<size_t>(nnz_a), rocprim::plus<long long>(), stream) == hipSuccess;
}

bool launch_spgemm_scan(hipStream_t stream, const long long *count, int nnz_a, long long *off, void *tmp, size_t *tmp_bytes) {
  return rocprim::exclusive_scan(tmp, *tmp_bytes, count, off, 0LL, static_cast<size_t>(nnz_a) + 1, rocprim::plus<long long>(), stream) ==
         hipSuccess;
}

void launch_spgemm_expand(hipStream_t stream, int nnz_a, int nprod, const long long *off, const int *arow, const int *a_colindex,
                          const int *b_rowptr, int nnz_b, const int *b_colindex, int col_bits, unsigned long long *keys) {
  if (nnz_a <= 0 || nnz_b <= 0 || nprod <= 0) return;
  SPMV_ACC_LAUNCH(spgemm_expand_kernel, dim3(grid_for(nprod, kSpgemmExpandTile)), dim3(kThreads), 0, stream, nnz_a, nprod, off, arow,
                  a_colindex, b_rowptr, nnz_b, b_colindex, col_bits, keys);
}

void launch_spgemm_map(hipStream_t stream, int m, int nnz_a, int nprod, const unsigned long long *keys, int col_bits, const long long *off,
                       const int *a_rowptr, const int *a_colindex, const int *b_rowptr, int nnz_b, int *pa, int *pb) {
  if (m <= 0 || nnz_a <= 0 || nnz_b <= 0 || nprod <= 0) return;
  SPMV_ACC_LAUNCH(spgemm_map_kernel, dim3(grid_for(nprod, kThreads)), dim3(kThreads), 0, stream, m, nnz_a, nprod, keys, col_bits, off,
                  a_rowptr, a_colindex, b_rowptr, nnz_b, pa, pb);
}

void launch_spgemm_values(hipStream_t stream, int nprod, int nnz_c, const int *pa, const int *pb, const int *start, const double *a_value,
                          const double *b_value, double *value) {
  if (nnz_c <= 0 || nprod <= 0) return;
  SPMV_ACC_LAUNCH(spgemm_values_kernel, dim3(grid_for(nnz_c, kSpgemmTile)), dim3(kThreads), 0, stream, nprod, nnz_c, pa, pb, start, a_value,
                  b_value, value);
}

} // namespace spmv_acc
