// cg.hpp -- the vector passes of preconditioned conjugate gradients: the definition of the dot product, the state block, size rules, launchers
// (k_cg.hip) and engine entries (cg.cpp) of
//   spmv_acc_cg_partials   how many doubles the partials buffer must hold (host arithmetic only),
//   spmv_acc_cg_start      b.b, r.r, r.z and p = z in one pass, then the state (two launches),
//   spmv_acc_cg_update     p.q; alpha; x += alpha p, r -= alpha q and the new r.r; rr, the history, the count (four launches),
//   spmv_acc_cg_direction  z = dinv r (optional) and r.z; beta; p = z + beta p (three launches).
// All three are launch-only (the per-iteration hot path): no allocation, no host read, no plan, no cache entry; capturable.  The caller owns
// every array, the state block and the partials buffer included; the SpMV q = A p and the preconditioner z = M r are the caller's calls.
// Constants, no tunables: nothing here is timed per matrix and nothing outlives a call.
// tests/test_cg_host.py CG_SIZE_RULES names each rule and the GPU tests that cross it.
//
// THE DOT PRODUCT (a pure function of the two arrays: not of the grid, not of timing; tests/test_cg_host.py host_cg_dot restates it).
//   1. Term i is u[i] * v[i], rounded on its own (contraction is off).
//   2. Partial c is the sum of the terms [c * kCgPartial, min(n, (c + 1) * kCgPartial)) in THE SUMMATION ORDER of gs.hpp with G = 64: lane l adds
//      the chunk's terms l, l + 64, ... in that order starting from its first (a lane without a term holds +0.0), the 64 lane sums are combined
//      as the balanced tree over neighbouring lanes (tests/test_gs_host.py row_sum(terms, 64)).  One wavefront produces one partial and stores
//      it: partials[c].  There are cg_chunks(n) = ceil(n / kCgPartial) of them.
//   3. The dot is row_sum(partials, kCgFinishThreads), computed by ONE workgroup in the finish launch that follows the pass: lane l adds the
//      partials l, l + kCgFinishThreads, ... from its first (none: +0.0), then the balanced tree over neighbouring lanes -- inside a wavefront
//      across lanes, the four wavefronts' sums through LDS as (w0 + w1) + (w2 + w3).
//   4. n = 0: no partial, the dot is +0.0.
// Several dots taken in one pass share the loads and have their own partials: dot d of a pass owns partials[d * cg_chunks(n) ..).  The start
// takes three (b.b, r.r, r.z), so the buffer holds 3 * cg_chunks(n) doubles; the later passes take one and use the first cg_chunks(n).
// No atomics and no waiting on another workgroup: a pass writes its partials, the kernel boundary orders them before the finish workgroup.
//
// THE STATE BLOCK: kCgState 8-byte words on the device, written only by the finish workgroups, with ordinary stores.
//   [0] status      integer  0 running; 1 converged (rr <= tol2); 2 breakdown, p.q not finite or <= 0; 3 breakdown, r.z not finite or < 0
//   [1] iterations  integer  updates of x done
//   [2] bb          double   b.b (the start)
//   [3] rr          double   r.r of the latest residual
//   [4] rz          double   r.z of the latest residual
//   [5] pq          double   p.q of the latest update
//   [6] alpha       double   rz / pq of the latest update, an IEEE division
//   [7] beta        double   rz_new / rz of the latest direction, an IEEE division
//   [8] tol2        double   fl(fl(rtol * rtol) * bb): rtol is squared first, the product with bb is rounded second
// THE START's finish: bb, rr, rz from the three dots; tol2; iterations = 0; pq = alpha = beta = +0.0; hist[0] = rr if hist_cap > 0;
//   status = 3 if rz is not finite, else 1 if rr <= tol2 (b = 0 or an exact x0), else 3 if rz <= 0, else 0.
// THE UPDATE's finishes: (a) pq = the dot; if pq is finite and > 0: alpha = rz / pq, else status = 2.  (b) rr = the dot; iterations += 1;
//   hist[iterations] = rr while iterations < hist_cap; status = 1 if rr <= tol2.
// THE DIRECTION's finish: rz_new = the dot; if it is finite and >= 0: beta = rz_new / rz, rz = rz_new; else status = 3 (rz and beta are kept).
// The fused passes: x[i] = x[i] + fl(alpha * p[i]); r[i] = r[i] - fl(alpha * q[i]); z[i] = fl(dinv[i] * r[i]); p[i] = z[i] + fl(beta * p[i]) --
// every product and sum rounded on its own.
//
// FROZEN MEANS FROZEN.  Every kernel of the update and the direction reads the status first and, when it is not 0, returns before it writes
// anything: x, r, p, z, the partials, the state and the history keep their bits.  A batch of iterations enqueued without a host check is
// therefore idempotent once the solve has ended, and the solution's bits do not depend on how often the host looks.
//
// Deliberately not done: folding a finish into the prologue of the pass that consumes it would save three launches per iteration, and wants a
// measurement (every workgroup would repeat the finish) and, at very large n, a two-level tree (a finish lane adds cg_chunks(n) / 256 partials
// one after the other: 4 at a million rows, 8 192 at the largest n).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>

namespace spmv_acc {

constexpr int kCgPartial = 1024;       // terms per partial, one wavefront's: 16 per lane in coalesced 512-B steps.  Long enough that the partials are
                                       // a thousandth of a vector (one finish workgroup reads them), short enough that a vector of 100 000 entries
                                       // already gives every CU a wavefront.  Reasoned, not timed
constexpr int kCgFinishThreads = 256;  // the finish is one workgroup of four wavefronts: up to a quarter of a million terms one partial a lane, and
                                       // one workgroup needs no further launch to combine.  Reasoned, not timed
constexpr int kCgState = 9;            // the state block in 8-byte words (THE STATE BLOCK above)
constexpr int kCgDots = 3;             // dots the start takes in one pass: what the partials buffer has room for
constexpr int kCgBatch = 4;            // a lane loads the operands of four of its 16 terms before it adds them in order: the update pass holds
                                       // 4 x (p, q, x, r) = 32 registers of operands and stays at eight waves per SIMD.  Reasoned, not timed

// the words of the state block
enum CgWord { kCgStatus = 0, kCgIterations, kCgBb, kCgRr, kCgRz, kCgPq, kCgAlpha, kCgBeta, kCgTol2 };

// partials of one dot over n terms
inline long long cg_chunks(long long n) { return n <= 0 ? 0 : (n + kCgPartial - 1) / kCgPartial; }

// ---- launchers (k_cg.hip): enqueue only.  state: kCgState words; partials: kCgDots * cg_chunks(n) doubles; n >= 0 (a pass over no terms is
// not launched, a finish always is) -----------------------------------------------------------------------------------------------------------
// the start's pass: partials of b.b, r.r, r.z; p = z (z may be r)
void launch_cg_start_pass(hipStream_t stream, int n, const double *b, const double *r, const double *z, double *p, double *partials);
// the start's finish (THE START's finish)
void launch_cg_start_finish(hipStream_t stream, int n, double rtol, const double *partials, unsigned long long *state, double *hist, int hist_cap);
// the update's first pass: partials of p.q
void launch_cg_pq_pass(hipStream_t stream, int n, const double *p, const double *q, const unsigned long long *state, double *partials);
// finish (a) of the update
void launch_cg_pq_finish(hipStream_t stream, int n, const double *partials, unsigned long long *state);
// the update's fused pass: x += alpha p, r -= alpha q, partials of the new r.r
void launch_cg_update_pass(hipStream_t stream, int n, const double *p, const double *q, double *x, double *r, const unsigned long long *state,
                           double *partials);
// finish (b) of the update
void launch_cg_rr_finish(hipStream_t stream, int n, const double *partials, unsigned long long *state, double *hist, int hist_cap);
// the direction's first pass: with dinv, z = dinv r is written first; partials of r.z (without dinv z is read and may be r)
void launch_cg_rz_pass(hipStream_t stream, int n, const double *r, double *z, const double *dinv, const unsigned long long *state, double *partials);
// the direction's finish
void launch_cg_rz_finish(hipStream_t stream, int n, const double *partials, unsigned long long *state);
// the direction's last pass: p = z + beta p
void launch_cg_direction_pass(hipStream_t stream, int n, const double *z, double *p, const unsigned long long *state);

// ---- engine entries (cg.cpp): return kOk or the error code they also leave in the calling thread's error slot --------------------------------
int run_cg_partials(int n, size_t *h_count);
int run_cg_start(int n, double rtol, const double *d_b, const double *d_r, const double *d_z, double *d_p, double *d_partials,
                 unsigned long long *d_state, double *d_hist, int hist_cap);
int run_cg_update(int n, const double *d_p, const double *d_q, double *d_x, double *d_r, double *d_partials, unsigned long long *d_state,
                  double *d_hist, int hist_cap);
int run_cg_direction(int n, const double *d_r, double *d_z, const double *d_dinv, double *d_p, double *d_partials, unsigned long long *d_state);

} // namespace spmv_acc
