// k_cg.hip -- the kernels of the conjugate-gradient vector passes (the dot product's definition, the state block, size rules and launcher
// declarations in cg.hpp, engine in cg.cpp).
//
// No reference counterpart: hpcde/spmv-acc multiplies a matrix by a vector.
//
// No atomics and no waiting on another workgroup anywhere: a pass stores one partial per wavefront and chunk, a finish is ONE workgroup that
// reads them behind the kernel boundary and combines its four wavefronts in LDS behind its own barrier; the state block is written by a
// finish workgroup's first lane alone, with ordinary stores.  Every kernel of the update and the direction reads the status word before
// anything else and returns when it is not 0 (cg.hpp FROZEN MEANS FROZEN).  VGPRs as compiled for gfx950 (wave64; no scratch, no AGPR, 8 waves
// per SIMD in all):
// 1. Passes: a workgroup's four wavefronts take a chunk of kCgPartial consecutive terms each and stride over the chunks beyond the grid.  A
//    lane owns the chunk's terms lane, lane + 64, ...: a step of the wavefront is one coalesced 512-B line of every operand, kCgBatch steps are
//    loaded before their arithmetic.  A full chunk tests no index; the last chunk of a vector may be ragged.  The 64 lane sums go through the
//    DPP butterfly (neighbouring lanes first: the balanced tree of gs.hpp).  Operands are read with the default cache policy: every vector of
//    an iteration is read again by the next pass.
//      cg_start_pass_kernel, 58: three dots off the same loads, p = z.        cg_pq_pass_kernel, 34: p.q.
//      cg_update_pass_kernel, 62: x += alpha p, r -= alpha q, the new r.r.    cg_rz_pass_kernel, 40: z = dinv r (template: with or without), r.z.
//      cg_direction_pass_kernel, 28: p = z + beta p, no dot.
// 2. Finishes (one workgroup of kCgFinishThreads): lane t adds the partials t, t + 256, ... from its first, four loads ahead; butterfly; LDS.
//      cg_start_finish_kernel, 24: bb, rr, rz, tol2, the first status.        cg_pq_finish_kernel, 18: pq, alpha or status 2.
//      cg_rr_finish_kernel, 18: rr, the history, the count, status 1.         cg_rz_finish_kernel, 18: beta and rz, or status 3.
#include "cg.hpp"
#include "structure_passes.hpp"

namespace spmv_acc {
namespace {

using namespace dev;
using namespace passes;
using u64 = unsigned long long;

constexpr int kWavesPerBlock = kThreads / kWave; // chunks a workgroup takes per stride, one per wavefront

static_assert(kCgFinishThreads == kThreads && kWavesPerBlock == 4, "the finish combines four wavefronts as (w0 + w1) + (w2 + w3)");
static_assert(kCgPartial % (kWave * kCgBatch) == 0, "a full chunk is a whole number of batches");

__device__ __forceinline__ double word_as_double(u64 w) { return __longlong_as_double(static_cast<long long>(w)); }
__device__ __forceinline__ u64 double_as_word(double v) { return static_cast<u64>(__double_as_longlong(v)); }
__device__ __forceinline__ bool finite(double v) { return fabs(v) < __builtin_huge_val(); } // (false for a NaN)

// The body of a pass.  An item names element i in two phases, so that a batch issues all its loads before any arithmetic or store:
// load(i) = the element's operands, apply(i, operands, t) = its arithmetic and stores, leaving its DOTS terms in t.  partials: dot d owns
// [d * nchunks, (d + 1) * nchunks); DOTS == 0: no dot, nothing is stored here.  All 64 lanes of a wavefront run the same chunks.
template <int DOTS, typename Item> __device__ __forceinline__ void chunk_pass(int n, double *__restrict__ partials, const Item &item) {
#pragma clang fp contract(off)
  constexpr int slots = DOTS > 0 ? DOTS : 1;
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const long long nchunks = (static_cast<long long>(n) + kCgPartial - 1) / kCgPartial;
  const long long stride = static_cast<long long>(gridDim.x) * kWavesPerBlock;
  for (long long c = static_cast<long long>(blockIdx.x) * kWavesPerBlock + wave; c < nchunks; c += stride) { // (wave-uniform)
    const long long base = c * kCgPartial;
    const long long left = n - base;
    double part[slots];
#pragma unroll
    for (int d = 0; d < slots; ++d) part[d] = 0.0; // a lane without a term holds +0.0
    if (left >= kCgPartial) { // (wave-uniform) a full chunk: no lane tests its index
#pragma unroll 1
      for (int k0 = 0; k0 < kCgPartial / kWave; k0 += kCgBatch) {
        typename Item::Operands o[kCgBatch];
        double t[kCgBatch][slots];
#pragma unroll
        for (int k = 0; k < kCgBatch; ++k) o[k] = item.load(base + (k0 + k) * kWave + lane);
#pragma unroll
        for (int k = 0; k < kCgBatch; ++k) item.apply(base + (k0 + k) * kWave + lane, o[k], t[k]);
#pragma unroll
        for (int k = 0; k < kCgBatch; ++k)
#pragma unroll
          for (int d = 0; d < DOTS; ++d) part[d] = k0 + k == 0 ? t[k][d] : part[d] + t[k][d]; // the sum starts from the lane's first term, not from 0.0
      }
    } else { // the ragged last chunk
      bool first = true;
      for (long long i = base + lane; i < n; i += kWave) {
        double t[slots];
        item.apply(i, item.load(i), t);
#pragma unroll
        for (int d = 0; d < DOTS; ++d) part[d] = first ? t[d] : part[d] + t[d];
        first = false;
      }
    }
#pragma unroll
    for (int d = 0; d < DOTS; ++d) {
      const double s = group_sum<64>(part[d]);
      if (lane == 0) partials[d * nchunks + c] = s;
    }
  }
}

// The finish of DOTS dots by one workgroup: dot[d] = row_sum(partials[d * nchunks ..], kCgFinishThreads), the same value in every lane.
template <int DOTS> __device__ __forceinline__ void finish_dots(int n, const double *__restrict__ partials, double (&dot)[DOTS]) {
#pragma clang fp contract(off)
  __shared__ double s_wave[DOTS][kWavesPerBlock];
  const int t = threadIdx.x;
  const long long nchunks = (static_cast<long long>(n) + kCgPartial - 1) / kCgPartial;
#pragma unroll
  for (int d = 0; d < DOTS; ++d) {
    const double *__restrict__ mine = partials + d * nchunks;
    double part = 0.0; // a lane without a partial holds +0.0
    long long c = t;
    if (c < nchunks) {
      part = mine[c]; // the sum starts from the lane's first partial
      c += kCgFinishThreads;
      for (; c + 3 * kCgFinishThreads < nchunks; c += 4 * kCgFinishThreads) { // four independent loads in flight, added in order
        const double v0 = mine[c], v1 = mine[c + kCgFinishThreads], v2 = mine[c + 2 * kCgFinishThreads], v3 = mine[c + 3 * kCgFinishThreads];
        part += v0;
        part += v1;
        part += v2;
        part += v3;
      }
      for (; c < nchunks; c += kCgFinishThreads) part += mine[c];
    }
    part = group_sum<64>(part);
    if ((t & (kWave - 1)) == 0) s_wave[d][t / kWave] = part;
  }
  __syncthreads();
#pragma unroll
  for (int d = 0; d < DOTS; ++d) dot[d] = (s_wave[d][0] + s_wave[d][1]) + (s_wave[d][2] + s_wave[d][3]);
}

// ---- the items of the five passes (chunk_pass) ----------------------------------------------------------------------------------------------
struct Two {
  double a, b;
};
struct Three {
  double a, b, c;
};
struct Four {
  double a, b, c, d;
};

// the start: b.b, r.r, r.z; p = z
struct StartItem {
  using Operands = Three;
  const double *b, *r, *z;
  double *p;
  __device__ __forceinline__ Three load(long long i) const { return {b[i], r[i], z[i]}; }
  __device__ __forceinline__ void apply(long long i, const Three &o, double *t) const {
#pragma clang fp contract(off)
    p[i] = o.c;
    t[0] = o.a * o.a;
    t[1] = o.b * o.b;
    t[2] = o.b * o.c;
  }
};

// p.q
struct PqItem {
  using Operands = Two;
  const double *p, *q;
  __device__ __forceinline__ Two load(long long i) const { return {p[i], q[i]}; }
  __device__ __forceinline__ void apply(long long, const Two &o, double *t) const {
#pragma clang fp contract(off)
    t[0] = o.a * o.b;
  }
};

// x += alpha p, r -= alpha q, the new r.r
struct UpdateItem {
  using Operands = Four;
  const double *p, *q;
  double *x, *r;
  double alpha;
  __device__ __forceinline__ Four load(long long i) const { return {p[i], q[i], x[i], r[i]}; }
  __device__ __forceinline__ void apply(long long i, const Four &o, double *t) const {
#pragma clang fp contract(off)
    const double ap = alpha * o.a, aq = alpha * o.b;
    const double rn = o.d - aq;
    x[i] = o.c + ap;
    r[i] = rn;
    t[0] = rn * rn;
  }
};

// JACOBI: z = dinv r, written; r.z
template <bool JACOBI> struct RzItem {
  using Operands = Two;
  const double *r;
  double *z;
  const double *dinv;
  __device__ __forceinline__ Two load(long long i) const { return {r[i], JACOBI ? dinv[i] : z[i]}; }
  __device__ __forceinline__ void apply(long long i, const Two &o, double *t) const {
#pragma clang fp contract(off)
    double zi = o.b;
    if (JACOBI) {
      zi = o.b * o.a;
      z[i] = zi;
    }
    t[0] = o.a * zi;
  }
};

// p = z + beta p
struct DirectionItem {
  using Operands = Two;
  const double *z;
  double *p;
  double beta;
  __device__ __forceinline__ Two load(long long i) const { return {z[i], p[i]}; }
  __device__ __forceinline__ void apply(long long i, const Two &o, double *) const {
#pragma clang fp contract(off)
    const double bp = beta * o.b;
    p[i] = o.a + bp;
  }
};

// ---- the start ------------------------------------------------------------------------------------------------------------------------------
// b, r and z are only read (z may be r); p overlaps none of them
__global__ __launch_bounds__(kThreads) void cg_start_pass_kernel(int n, const double *__restrict__ b, const double *__restrict__ r,
                                                                 const double *__restrict__ z, double *__restrict__ p,
                                                                 double *__restrict__ partials) {
#pragma clang fp contract(off)
  chunk_pass<kCgDots>(n, partials, StartItem{b, r, z, p});
}

// ONE workgroup.  cg.hpp THE START's finish
__global__ __launch_bounds__(kThreads) void cg_start_finish_kernel(int n, double rtol, const double *__restrict__ partials, u64 *__restrict__ state,
                                                                   double *__restrict__ hist, int hist_cap) {
#pragma clang fp contract(off)
  double dot[kCgDots];
  finish_dots<kCgDots>(n, partials, dot);
  if (threadIdx.x != 0) return;
  const double bb = dot[0], rr = dot[1], rz = dot[2];
  const double rtol2 = rtol * rtol;
  const double tol2 = rtol2 * bb; // rtol is squared first, the product with bb is rounded second
  const u64 status = !finite(rz) ? 3 : (rr <= tol2 ? 1 : (rz <= 0.0 ? 3 : 0));
  state[kCgStatus] = status;
  state[kCgIterations] = 0;
  state[kCgBb] = double_as_word(bb);
  state[kCgRr] = double_as_word(rr);
  state[kCgRz] = double_as_word(rz);
  state[kCgPq] = double_as_word(0.0);
  state[kCgAlpha] = double_as_word(0.0);
  state[kCgBeta] = double_as_word(0.0);
  state[kCgTol2] = double_as_word(tol2);
  if (hist_cap > 0) hist[0] = rr;
}

// ---- the update -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void cg_pq_pass_kernel(int n, const double *__restrict__ p, const double *__restrict__ q,
                                                              const u64 *__restrict__ state, double *__restrict__ partials) {
#pragma clang fp contract(off)
  if (state[kCgStatus] != 0) return; // frozen: nothing is written
  chunk_pass<1>(n, partials, PqItem{p, q});
}

// ONE workgroup.  Finish (a) of cg.hpp THE UPDATE's finishes
__global__ __launch_bounds__(kThreads) void cg_pq_finish_kernel(int n, const double *__restrict__ partials, u64 *__restrict__ state) {
#pragma clang fp contract(off)
  if (state[kCgStatus] != 0) return; // frozen (every lane reads the same word: the barrier below is passed by all or by none)
  double dot[1];
  finish_dots<1>(n, partials, dot);
  if (threadIdx.x != 0) return;
  const double pq = dot[0];
  state[kCgPq] = double_as_word(pq);
  if (finite(pq) && pq > 0.0) state[kCgAlpha] = double_as_word(word_as_double(state[kCgRz]) / pq);
  else state[kCgStatus] = 2;
}

// x and r are read and written in place (a lane its own elements only); p and q overlap neither
__global__ __launch_bounds__(kThreads) void cg_update_pass_kernel(int n, const double *__restrict__ p, const double *__restrict__ q,
                                                                  double *__restrict__ x, double *__restrict__ r, const u64 *__restrict__ state,
                                                                  double *__restrict__ partials) {
#pragma clang fp contract(off)
  if (state[kCgStatus] != 0) return; // frozen, or finish (a) has just found the breakdown
  const double alpha = word_as_double(state[kCgAlpha]);
  chunk_pass<1>(n, partials, UpdateItem{p, q, x, r, alpha});
}

// ONE workgroup.  Finish (b) of cg.hpp THE UPDATE's finishes
__global__ __launch_bounds__(kThreads) void cg_rr_finish_kernel(int n, const double *__restrict__ partials, u64 *__restrict__ state,
                                                                double *__restrict__ hist, int hist_cap) {
#pragma clang fp contract(off)
  if (state[kCgStatus] != 0) return;
  double dot[1];
  finish_dots<1>(n, partials, dot);
  if (threadIdx.x != 0) return;
  const double rr = dot[0];
  const u64 done = state[kCgIterations] + 1;
  state[kCgRr] = double_as_word(rr);
  state[kCgIterations] = done;
  if (done < static_cast<u64>(hist_cap > 0 ? hist_cap : 0)) hist[done] = rr;
  if (rr <= word_as_double(state[kCgTol2])) state[kCgStatus] = 1;
}

// ---- the direction --------------------------------------------------------------------------------------------------------------------------
// JACOBI: z = dinv r is written (z overlaps neither r nor dinv); otherwise z is only read and may be r
template <bool JACOBI>
__global__ __launch_bounds__(kThreads) void cg_rz_pass_kernel(int n, const double *__restrict__ r, double *z, const double *__restrict__ dinv,
                                                              const u64 *__restrict__ state, double *__restrict__ partials) {
#pragma clang fp contract(off)
  if (state[kCgStatus] != 0) return;
  chunk_pass<1>(n, partials, RzItem<JACOBI>{r, z, dinv});
}

// ONE workgroup.  cg.hpp THE DIRECTION's finish
__global__ __launch_bounds__(kThreads) void cg_rz_finish_kernel(int n, const double *__restrict__ partials, u64 *__restrict__ state) {
#pragma clang fp contract(off)
  if (state[kCgStatus] != 0) return;
  double dot[1];
  finish_dots<1>(n, partials, dot);
  if (threadIdx.x != 0) return;
  const double rz_new = dot[0];
  if (finite(rz_new) && rz_new >= 0.0) {
    state[kCgBeta] = double_as_word(rz_new / word_as_double(state[kCgRz]));
    state[kCgRz] = double_as_word(rz_new);
  } else {
    state[kCgStatus] = 3;
  }
}

// z is only read (it may be r); p is read and written in place
__global__ __launch_bounds__(kThreads) void cg_direction_pass_kernel(int n, const double *__restrict__ z, double *__restrict__ p,
                                                                     const u64 *__restrict__ state) {
#pragma clang fp contract(off)
  if (state[kCgStatus] != 0) return; // frozen, or the finish has just found the breakdown: p keeps its bits
  const double beta = word_as_double(state[kCgBeta]);
  chunk_pass<0>(n, nullptr, DirectionItem{z, p, beta});
}

inline unsigned pass_grid(int n) { return grid_for(cg_chunks(n), kWavesPerBlock); }

} // namespace

void launch_cg_start_pass(hipStream_t stream, int n, const double *b, const double *r, const double *z, double *p, double *partials) {
  if (n <= 0) return;
  SPMV_ACC_LAUNCH(cg_start_pass_kernel, dim3(pass_grid(n)), dim3(kThreads), 0, stream, n, b, r, z, p, partials);
}

void launch_cg_start_finish(hipStream_t stream, int n, double rtol, const double *partials, unsigned long long *state, double *hist, int hist_cap) {
  if (n < 0) return;
  SPMV_ACC_LAUNCH(cg_start_finish_kernel, dim3(1), dim3(kThreads), 0, stream, n, rtol, partials, state, hist, hist_cap);
}

void launch_cg_pq_pass(hipStream_t stream, int n, const double *p, const double *q, const unsigned long long *state, double *partials) {
  if (n <= 0) return;
  SPMV_ACC_LAUNCH(cg_pq_pass_kernel, dim3(pass_grid(n)), dim3(kThreads), 0, stream, n, p, q, state, partials);
}

void launch_cg_pq_finish(hipStream_t stream, int n, const double *partials, unsigned long long *state) {
  if (n < 0) return;
  SPMV_ACC_LAUNCH(cg_pq_finish_kernel, dim3(1), dim3(kThreads), 0, stream, n, partials, state);
}

void launch_cg_update_pass(hipStream_t stream, int n, const double *p, const double *q, double *x, double *r, const unsigned long long *state,
                           double *partials) {
  if (n <= 0) return;
  SPMV_ACC_LAUNCH(cg_update_pass_kernel, dim3(pass_grid(n)), dim3(kThreads), 0, stream, n, p, q, x, r, state, partials);
}

void launch_cg_rr_finish(hipStream_t stream, int n, const double *partials, unsigned long long *state, double *hist, int hist_cap) {
  if (n < 0) return;
  SPMV_ACC_LAUNCH(cg_rr_finish_kernel, dim3(1), dim3(kThreads), 0, stream, n, partials, state, hist, hist_cap);
}

void launch_cg_rz_pass(hipStream_t stream, int n, const double *r, double *z, const double *dinv, const unsigned long long *state, double *partials) {
  if (n <= 0) return;
  if (dinv) SPMV_ACC_LAUNCH(cg_rz_pass_kernel<true>, dim3(pass_grid(n)), dim3(kThreads), 0, stream, n, r, z, dinv, state, partials);
  else SPMV_ACC_LAUNCH(cg_rz_pass_kernel<false>, dim3(pass_grid(n)), dim3(kThreads), 0, stream, n, r, z, dinv, state, partials);
}

void launch_cg_rz_finish(hipStream_t stream, int n, const double *partials, unsigned long long *state) {
  if (n < 0) return;
  SPMV_ACC_LAUNCH(cg_rz_finish_kernel, dim3(1), dim3(kThreads), 0, stream, n, partials, state);
}

void launch_cg_direction_pass(hipStream_t stream, int n, const double *z, double *p, const unsigned long long *state) {
  if (n <= 0) return;
  SPMV_ACC_LAUNCH(cg_direction_pass_kernel, dim3(pass_grid(n)), dim3(kThreads), 0, stream, n, z, p, state);
}

} // namespace spmv_acc
