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
// 4. Values (spgemm_values_kernel, the per-step hot path and the first call's last launch): coo_values_kernel's tiling and summation order, the
//    gather replaced by two index loads, two gathers and a product rounded on its own (fp contraction is off in this file's sums: a fused
//    multiply-add would round once where the definition rounds twice).  Streams start, pa and pb (4 B per entry, 8 B per product), gathers 16 B
//    per product, writes 8 B per entry.  Four entries per lane: spgemm.hpp kSpgemmPerLane.  The sums depend on the map and the values alone (no
//    atomics), so the same values give the same bits.
#include "spgemm.hpp"
#include "device_utils.hpp"
#include "kernels.hpp"

#include <rocprim/device/device_reduce.hpp>
#include <rocprim/device/device_scan.hpp>

namespace spmv_acc {
namespace {

using namespace dev;

typedef unsigned long long u64;

unsigned spgemm_grid(long long items, int per_block) {
  long long b = (items + per_block - 1) / per_block;
  const long long cap = max_grid_blocks();
  return static_cast<unsigned>(b < 1 ? 1 : (b > cap ? cap : b));
}

// B's row c as positions [lo, lo + len) inside B's arrays, whatever b_rowptr holds (c has passed the census: 0 <= c < k)
__device__ __forceinline__ int spgemm_b_row(const int *__restrict__ b_rowptr, int nnz_b, int c, int *len) {
  int lo = b_rowptr[c], hi = b_rowptr[c + 1];
  lo = lo < 0 ? 0 : (lo > nnz_b ? nnz_b : lo);
  hi = hi < lo ? lo : (hi > nnz_b ? nnz_b : hi);
  *len = hi - lo;
  return lo;
}

// the largest q in [lo, hi] with off[q] <= e (lo itself if there is none).  off ascends; with off[lo] <= e < off[hi + 1] this is the non-zero of
// A whose products include e: non-zeros without products (off[q] == off[q + 1]) are passed over
__device__ __forceinline__ int spgemm_holder(const long long *__restrict__ off, int lo, int hi, long long e) {
  while (lo < hi) {
    const int mid = lo + (hi - lo + 1) / 2;
    if (off[mid] <= e) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(kThreads) void spgemm_counts_kernel(int m, int nnz_a, const int *__restrict__ a_rowptr,
                                                                 const int *__restrict__ a_colindex, const int *__restrict__ b_rowptr, int nnz_b,
                                                                 long long *__restrict__ count, int *__restrict__ arow) {
  const long long stride = static_cast<long long>(gridDim.x) * kThreads;
  for (long long q = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; q <= nnz_a; q += stride) {
    if (q == nnz_a) {
      count[q] = 0; // (the scan's closing element)
      continue;
    }
    int len;
    (void)spgemm_b_row(b_rowptr, nnz_b, a_colindex[q], &len);
    count[q] = len;
    if (arow != nullptr) { // the last row r in [0, m) with a_rowptr[r] <= q: the search stays inside a_rowptr[0 .. m) whatever it holds
      int lo = 0, hi = m - 1;
      while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (a_rowptr[mid] <= q) lo = mid;
        else hi = mid - 1;
      }
      arow[q] = lo;
    }
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
    const int q_first = spgemm_holder(off, 0, nnz_a - 1, base);
    const int q_last = spgemm_holder(off, q_first, nnz_a - 1, last);
#pragma unroll
    for (int k = 0; k < kSpgemmExpandPerLane; ++k) {
      const long long e = base + k * kWave + lane;
      if (e > last) continue;
      const int q = spgemm_holder(off, q_first, q_last, e);
      int len;
      const int lo = spgemm_b_row(b_rowptr, nnz_b, a_colindex[q], &len);
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
    const int q = spgemm_holder(off, lo, hi, e); // (with an a_rowptr that does not ascend: some non-zero of A, and t below is held inside B)
    int len;
    const int b_lo = spgemm_b_row(b_rowptr, nnz_b, a_colindex[q], &len);
    long long step = e - off[q];
    step = step >= len ? len - 1 : step;
    const int t = b_lo + static_cast<int>(step < 0 ? 0 : step);
    pa[p] = q;
    pb[p] = t < nnz_b ? t : nnz_b - 1;
  }
}

// the rounded product of sorted position p (0 <= p < nprod).  The map is the caller's and carries no lengths: pa / pb are not checked
__device__ __forceinline__ double spgemm_fetch(const int *__restrict__ pa, const int *__restrict__ pb, const double *__restrict__ a,
                                               const double *__restrict__ b, int p) {
#pragma clang fp contract(off)
  const double prod = a[pa[p]] * b[pb[p]];
  return prod;
}

// the wavefront form of coo.hpp's order for the run [s, end), end - s > 64.  All 64 lanes must call it; every lane returns the sum.
__device__ __forceinline__ double spgemm_wave_run_sum(const int *__restrict__ pa, const int *__restrict__ pb, const double *__restrict__ a,
                                                      const double *__restrict__ b, int s, int end, int lane) {
#pragma clang fp contract(off)
  int p = s + lane;
  double part = spgemm_fetch(pa, pb, a, b, p);
  p += kWave;
  for (; p + 3 * kWave < end; p += 4 * kWave) { // four independent products in flight, added in order
    const double v0 = spgemm_fetch(pa, pb, a, b, p), v1 = spgemm_fetch(pa, pb, a, b, p + kWave);
    const double v2 = spgemm_fetch(pa, pb, a, b, p + 2 * kWave), v3 = spgemm_fetch(pa, pb, a, b, p + 3 * kWave);
    part += v0;
    part += v1;
    part += v2;
    part += v3;
  }
  for (; p < end; p += kWave) part += spgemm_fetch(pa, pb, a, b, p);
  return group_sum<64>(part);
}

// One workgroup per tile of kSpgemmTile C entries, blocks stride over the tiles beyond the grid.  nprod > 0 (the launcher checks).
// (waves_per_eu: the kernel asks for the eighth wave per SIMD; the compiler then orders the loads to fit 64 VGPRs without scratch)
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(8, 8))) void spgemm_values_kernel(int nprod, int nnz_c, const int *__restrict__ pa, const int *__restrict__ pb,
                                                                 const int *__restrict__ start, const double *__restrict__ a_value,
                                                                 const double *__restrict__ b_value, double *__restrict__ value) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const long long ntiles = (static_cast<long long>(nnz_c) + kSpgemmTile - 1) / kSpgemmTile;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) { // (block-uniform)
    const long long base = tile * kSpgemmTile + static_cast<long long>(wave) * kSpgemmWaveChunk;
    if (base >= nnz_c) continue; // (wave-uniform)
    int s[kSpgemmPerLane];
    int len[kSpgemmPerLane]; // the run's length; NEGATED where it is longer than kCooLongRun (such a run sits the lane pass out)
    double acc[kSpgemmPerLane];
    int rounds = 0;
    bool any_long = false;
#pragma unroll
    for (int k = 0; k < kSpgemmPerLane; ++k) {
      const long long j = base + k * kWave + lane;
      int a = 0, b = 0;
      if (j < nnz_c) {
        a = load_stream(start + j);
        b = load_stream(start + j + 1);
      }
      a = a < 0 ? 0 : (a > nprod ? nprod : a); // the map is the CALLER's array here: every run is clamped to [0, nprod]
      b = b < a ? a : (b > nprod ? nprod : b);
      s[k] = a;
      const int l = b - a;
      len[k] = l > kCooLongRun ? -l : l;
      any_long |= l > kCooLongRun;
      rounds = l <= kCooLongRun && l > rounds ? l : rounds;
      acc[k] = 0.0; // (an empty run -- a crafted map -- sums to 0.0)
    }
    for (int t = 0; t < rounds; ++t) {
      int ua[kSpgemmPerLane], ub[kSpgemmPerLane];
      double va[kSpgemmPerLane], vb[kSpgemmPerLane];
#pragma unroll
      for (int k = 0; k < kSpgemmPerLane; ++k) {
        const int p = t < len[k] ? s[k] + t : 0;
        ua[k] = pa[p];
        ub[k] = pb[p];
      }
#pragma unroll
      for (int k = 0; k < kSpgemmPerLane; ++k) {
        va[k] = a_value[ua[k]];
        vb[k] = b_value[ub[k]];
      }
#pragma unroll
      for (int k = 0; k < kSpgemmPerLane; ++k) {
        const double vk = va[k] * vb[k]; // rounded here, added below
        acc[k] = t < len[k] ? (t == 0 ? vk : acc[k] + vk) : acc[k];
      }
    }
    if (__ballot(any_long)) { // (wave-uniform; never taken on a mesh)
#pragma unroll
      for (int k = 0; k < kSpgemmPerLane; ++k) {
        unsigned long long todo = __ballot(len[k] < 0);
        while (todo) { // the wavefront takes its long runs one at a time, in lane order
          const int owner = __ffsll(static_cast<long long>(todo)) - 1;
          todo &= todo - 1;
          const int a = __shfl(s[k], owner, kWave);
          const int l = -__shfl(len[k], owner, kWave);
          const double sum = spgemm_wave_run_sum(pa, pb, a_value, b_value, a, a + l, lane);
          if (lane == owner) acc[k] = sum;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kSpgemmPerLane; ++k) {
      const long long j = base + k * kWave + lane;
      if (j < nnz_c) value[j] = acc[k];
    }
  }
}

} // namespace

void launch_spgemm_counts(hipStream_t stream, int m, int nnz_a, const int *a_rowptr, const int *a_colindex, const int *b_rowptr, int nnz_b,
                          long long *count, int *arow) {
  if (nnz_a <= 0 || m <= 0) return;
  SPMV_ACC_LAUNCH(spgemm_counts_kernel, dim3(spgemm_grid(static_cast<long long>(nnz_a) + 1, kThreads)), dim3(kThreads), 0, stream, m, nnz_a,
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
  SPMV_ACC_LAUNCH(spgemm_expand_kernel, dim3(spgemm_grid(nprod, kSpgemmExpandTile)), dim3(kThreads), 0, stream, nnz_a, nprod, off, arow,
                  a_colindex, b_rowptr, nnz_b, b_colindex, col_bits, keys);
}

void launch_spgemm_map(hipStream_t stream, int m, int nnz_a, int nprod, const unsigned long long *keys, int col_bits, const long long *off,
                       const int *a_rowptr, const int *a_colindex, const int *b_rowptr, int nnz_b, int *pa, int *pb) {
  if (m <= 0 || nnz_a <= 0 || nnz_b <= 0 || nprod <= 0) return;
  SPMV_ACC_LAUNCH(spgemm_map_kernel, dim3(spgemm_grid(nprod, kThreads)), dim3(kThreads), 0, stream, m, nnz_a, nprod, keys, col_bits, off,
                  a_rowptr, a_colindex, b_rowptr, nnz_b, pa, pb);
}

void launch_spgemm_values(hipStream_t stream, int nprod, int nnz_c, const int *pa, const int *pb, const int *start, const double *a_value,
                          const double *b_value, double *value) {
  if (nnz_c <= 0 || nprod <= 0) return;
  SPMV_ACC_LAUNCH(spgemm_values_kernel, dim3(spgemm_grid(nnz_c, kSpgemmTile)), dim3(kThreads), 0, stream, nprod, nnz_c, pa, pb, start, a_value,
                  b_value, value);
}

} // namespace spmv_acc
