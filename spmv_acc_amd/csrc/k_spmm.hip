// k_spmm.hip -- CSR SpMM: Y = alpha * A * X + beta * Y for k dense vectors in one pass over the matrix per column panel.
//
// No reference counterpart (hpcde/spmv-acc has no multi-vector product).  What binds the single-vector kernels is bytes: the 12 B per
// non-zero of the matrix stream and the 128-B line every far gather costs for 8 useful bytes.  A multi-vector
// product reads the matrix once per panel of up to kSpmmPanel columns, and with row-major X one gather of a team fetches a contiguous
// row segment of X instead of one value per line.
//
// Three kernels, all atomic-free, with sum orders fixed by the matrix alone (never by ldx / ldy, the base alignment of X and Y, the stream or
// timing):
//   * spmm_rows_kernel (row-major X / Y): a workgroup owns consecutive rows; their colindex / values are staged into LDS with coalesced loads,
//     then a TEAM of TS lanes owns one row, each lane two adjacent columns of the panel (one 16-B gather of X[col * ldx + c .. c + 1] per
//     non-zero, through the under-aligned vector type, so odd ldx and 8-B offset views take the same instruction).  The team walks its row in
//     CSR order: no cross-lane reduction.
//   * spmm_rows_cm_kernel (column-major X / Y): one lane per row, the panel's columns in register chunks of kSpmmColChunk; the gathers
//     X[j * ldx + col] and the stores Y[j * ldy + r] are coalesced across the lanes' consecutive rows.
//   * rows longer than kSpmmLongRow (hub rows): the two kernels above skip them.  The plan cuts them into pieces of kSpmmPiece non-zeros
//     (spmm.cpp); spmm_pieces_kernel gives each piece a wavefront that writes the piece's partial k-vector to plan scratch, and
//     spmm_fixup_kernel adds a row's pieces in piece order and applies alpha / beta -- the plus_kernel + plus_fixup_kernel pattern.
#include "spmm.hpp"
#include "structure_passes.hpp"

namespace spmv_acc {
namespace {

using namespace dev;
using passes::grid_for; // (the launchers' clamped grid)

// (the size rules themselves are in spmm.hpp; the constants here are geometry)
constexpr int kSpmmTeamMax = kSpmmPanel / 2; // lanes of the widest team: two columns per lane
constexpr int kSpmmTile = 1024;               // row-major: non-zeros per LDS tile (12 KB: eight workgroups per CU)
constexpr int kSpmmColChunk = 4;              // column-major: columns a lane holds in registers per pass over its row
// XCD-chunked workgroup order (device_utils.hpp xcd_chunked_block), the SpMV kernels' order (tunable xcd_chunk = 16 row blocks): each XCD takes
// this many consecutive ROWS per super-chunk, whatever the rows per workgroup, so that neighbouring rows -- which share X rows on FEM-like
// matrices -- run on one XCD's L2.  (Not measured against the plain order on this kernel: DESIGN.md section 6.)
constexpr int kSpmmXcdRows = 1024;

// 16-B gather / store of two adjacent doubles through the under-aligned vector type: one instruction whatever the alignment of X / Y
__device__ __forceinline__ double2v load_x2(const double *p) { return *reinterpret_cast<const double2v_a8 *>(p); }

// Y[row, c .. c + 1] (row-major) or Y[row, c] alone (pair == false): beta == 0 never reads Y
__device__ __forceinline__ void store_y_pair(double *y, bool pair, double alpha, double beta, double s0, double s1) {
  if (pair) {
    double2v o;
    o.x = alpha * s0;
    o.y = alpha * s1;
    if (beta != 0.0) {
      const double2v old = *reinterpret_cast<const double2v_a8 *>(y);
      o.x += beta * old.x;
      o.y += beta * old.y;
    }
    __builtin_nontemporal_store(o, reinterpret_cast<double2v_a8 *>(y));
  } else {
    const double r = beta == 0.0 ? alpha * s0 : alpha * s0 + beta * y[0];
    __builtin_nontemporal_store(r, y);
  }
}

// Row-major: a workgroup owns 256 / TS consecutive rows, TS lanes per row; lane t of a team owns panel columns 2t, 2t + 1 (kp = the panel's
// width, <= 2 * TS).  The block's colindex / values are staged into LDS in tiles of kSpmmTile non-zeros with coalesced loads (the matrix stream
// read once, line by line), then each team walks its row's part of the tile in CSR order -- no cross-lane reduction.  Every lane gathers 16 B:
// where kp is odd the last lane's pair starts one column to the left and it keeps the upper half (no branch between the loads).  SINGLE (kp == 1):
// 8-B gathers.  x / y point at the panel's first column.  Rows longer than kSpmmLongRow are skipped, and so are the tiles only they cover: each
// round the block's short rows vote (LDS min) where the next tile starts.  Blocks stride over the rows beyond the grid (max_grid_blocks).
// (A first form read colindex / values straight from global memory, every lane of a team at the same address: a wave's 64 / TS rows each took
// 16 B of a line per step, the partly read lines fell out of the caches between steps, and the boneS10 stand-in took 0.27-0.49 ms for k = 1 ... 16,
// up to 9 x one SpMV.)
template <int TS, bool SINGLE>
__global__ __launch_bounds__(kThreads) void spmm_rows_kernel(int m, int kp, int xcd_chunk, long long ldx, long long ldy, double alpha, double beta,
                                                             const int *__restrict__ rp, const int *__restrict__ ci,
                                                             const double *__restrict__ v, const double *__restrict__ x,
                                                             double *__restrict__ y, const int *__restrict__ guard, int *__restrict__ stale) {
  check_plan_guard(rp, m, guard, stale);
  constexpr int kRows = kThreads / TS;
  __shared__ int lci[kSpmmTile];
  __shared__ double lv[kSpmmTile];
  __shared__ int vote[2];
  const int t = threadIdx.x % TS;
  const int c = 2 * t;
  const bool active = c < kp; // (inactive lanes still stage and vote)
  const bool pair = c + 1 < kp;
  const double *xl = x + (SINGLE ? 0 : (pair ? c : (active ? c - 1 : 0)));
  const int nblocks = static_cast<int>((static_cast<long long>(m) + kRows - 1) / kRows);
  for (int blk = xcd_chunked_block(blockIdx.x, gridDim.x, xcd_chunk); blk < nblocks; blk += gridDim.x) { // (block-uniform)
    const long long row_base = static_cast<long long>(blk) * kRows;
    const long long row_end = row_base + kRows < m ? row_base + kRows : m;
    const long long row = row_base + threadIdx.x / TS;
    const int s1 = rp[row_end];
    int r0 = 0, r1 = 0;
    bool mine = false; // a row of this block that this kernel finishes (not a long one)
    if (row < row_end) {
      r0 = rp[row];
      r1 = rp[row + 1];
      mine = r1 - r0 <= kSpmmLongRow;
      if (!mine) r1 = r0; // the pieces and the fix-up own this row
    }
    if (threadIdx.x == 0) vote[0] = vote[1] = INT_MAX;
    __syncthreads();
    if (t == 0 && r1 > r0) atomicMin(&vote[0], r0);
    __syncthreads();
    int off = vote[0];
    double s0 = 0.0, s1v = 0.0;
    for (int round = 1; off != INT_MAX; ++round) { // (block-uniform)
      const int cnt = s1 - off < kSpmmTile ? s1 - off : kSpmmTile;
      for (int i = threadIdx.x; i < cnt; i += kThreads) {
        lci[i] = ci[off + i];
        lv[i] = v[off + i];
      }
      if (threadIdx.x == 0) vote[round & 1] = INT_MAX; // (the slot the previous round's result is not in)
      __syncthreads();
      const int end = off + cnt;
      int j = r0 > off ? r0 : off;
      const int hi = r1 < end ? r1 : end;
      if (active) {
        for (; j + 4 <= hi; j += 4) {
          const int q = j - off;
          const long long c0 = lci[q], c1 = lci[q + 1], c2 = lci[q + 2], c3 = lci[q + 3];
          double2v g0, g1, g2, g3;
          if (SINGLE) { // (the one column in the upper half, where a lane without a pair keeps its column)
            g0.y = xl[c0 * ldx];
            g1.y = xl[c1 * ldx];
            g2.y = xl[c2 * ldx];
            g3.y = xl[c3 * ldx];
            g0.x = g1.x = g2.x = g3.x = 0.0;
          } else {
            g0 = load_x2(xl + c0 * ldx);
            g1 = load_x2(xl + c1 * ldx);
            g2 = load_x2(xl + c2 * ldx);
            g3 = load_x2(xl + c3 * ldx);
          }
          const double a0 = lv[q], a1 = lv[q + 1], a2 = lv[q + 2], a3 = lv[q + 3];
          s0 += a0 * (pair ? g0.x : g0.y);
          s1v += a0 * g0.y;
          s0 += a1 * (pair ? g1.x : g1.y);
          s1v += a1 * g1.y;
          s0 += a2 * (pair ? g2.x : g2.y);
          s1v += a2 * g2.y;
          s0 += a3 * (pair ? g3.x : g3.y);
          s1v += a3 * g3.y;
        }
        for (; j < hi; ++j) {
          const long long col = lci[j - off];
          const double a = lv[j - off];
          if (SINGLE) {
            s0 += a * xl[col * ldx];
          } else {
            const double2v g = load_x2(xl + col * ldx);
            s0 += a * (pair ? g.x : g.y);
            s1v += a * g.y;
          }
        }
      }
      if (t == 0 && r1 > end) atomicMin(&vote[round & 1], r0 > end ? r0 : end); // where this row goes on
      __syncthreads(); // (the vote is in; the tile may be overwritten)
      off = vote[round & 1];
    }
    if (active && mine) store_y_pair(y + row * ldy + c, pair, alpha, beta, s0, s1v);
    __syncthreads(); // (the next block's votes reuse the slots)
  }
}

// Column-major: one lane per row, the panel's kp columns in chunks of kSpmmColChunk (the row's colindex / values are read once per chunk).
__global__ __launch_bounds__(kThreads) void spmm_rows_cm_kernel(int m, int kp, int xcd_chunk, long long ldx, long long ldy, double alpha, double beta,
                                                                const int *__restrict__ rp, const int *__restrict__ ci,
                                                                const double *__restrict__ v, const double *__restrict__ x,
                                                                double *__restrict__ y, const int *__restrict__ guard,
                                                                int *__restrict__ stale) {
  check_plan_guard(rp, m, guard, stale);
  const long long lanes = static_cast<long long>(gridDim.x) * kThreads;
  const int b = xcd_chunked_block(blockIdx.x, gridDim.x, xcd_chunk);
  for (long long row = static_cast<long long>(b) * kThreads + threadIdx.x; row < m; row += lanes) {
    const int r0 = rp[row], r1 = rp[row + 1];
    if (r1 - r0 > kSpmmLongRow) continue;
    for (int c0 = 0; c0 < kp; c0 += kSpmmColChunk) {
      const int w = kp - c0 < kSpmmColChunk ? kp - c0 : kSpmmColChunk;
      const double *xc = x + c0 * ldx;
      double s[kSpmmColChunk] = {0.0, 0.0, 0.0, 0.0};
      int j = r0;
      for (; j + 2 <= r1; j += 2) {
        const int ca = ci[j], cb = ci[j + 1];
        const double va = v[j], vb = v[j + 1];
#pragma unroll
        for (int q = 0; q < kSpmmColChunk; ++q) {
          if (q < w) {
            const double ga = xc[q * ldx + ca], gb = xc[q * ldx + cb];
            s[q] += va * ga;
            s[q] += vb * gb;
          }
        }
      }
      if (j < r1) {
        const int ca = ci[j];
        const double va = v[j];
#pragma unroll
        for (int q = 0; q < kSpmmColChunk; ++q)
          if (q < w) s[q] += va * xc[q * ldx + ca];
      }
#pragma unroll
      for (int q = 0; q < kSpmmColChunk; ++q) {
        if (q < w) {
          double *yq = y + (c0 + q) * ldy + row;
          __builtin_nontemporal_store(beta == 0.0 ? alpha * s[q] : alpha * s[q] + beta * *yq, yq);
        }
      }
    }
  }
}

// Long-row pieces: one wavefront per piece [begin, end) of <= kSpmmPiece non-zeros, four per lane; for each chunk of kSpmmColChunk panel
// columns the lanes' products are added by the DPP butterfly (a fixed tree) and lane 0 writes them to partial[col * npieces + piece] (each
// (row, column) pair's pieces are contiguous there: the fix-up adds them with wave_range_sum).  X(i, j) = x[i * sxi + j * sxj] serves both layouts.
__global__ __launch_bounds__(kThreads) void spmm_pieces_kernel(int m, int npieces, int kp, long long sxi, long long sxj,
                                                               const int *__restrict__ piece, const int *__restrict__ rp,
                                                               const int *__restrict__ ci, const double *__restrict__ v,
                                                               const double *__restrict__ x, double *__restrict__ partial,
                                                               const int *__restrict__ guard, int *__restrict__ stale) {
  check_plan_guard(rp, m, guard, stale);
  constexpr int kPer = kSpmmPiece / kWave;
  const int lane = threadIdx.x & (kWave - 1);
  const long long waves = static_cast<long long>(gridDim.x) * (kThreads / kWave);
  for (long long p = static_cast<long long>(blockIdx.x) * (kThreads / kWave) + threadIdx.x / kWave; p < npieces; p += waves) { // wave-uniform
    const int begin = piece[2 * p], end = piece[2 * p + 1];
    int col[kPer];
    double a[kPer];
    bool in[kPer];
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
      const int j = begin + q * kWave + lane;
      in[q] = j < end;
      col[q] = in[q] ? load_stream(ci + j) : 0;
      a[q] = in[q] ? load_stream(v + j) : 0.0;
    }
    for (int c0 = 0; c0 < kp; c0 += kSpmmColChunk) {
      double s[kSpmmColChunk] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int q = 0; q < kPer; ++q) {
#pragma unroll
        for (int u = 0; u < kSpmmColChunk; ++u)
          if (c0 + u < kp && in[q]) s[u] += a[q] * x[static_cast<long long>(col[q]) * sxi + (c0 + u) * sxj];
      }
#pragma unroll
      for (int u = 0; u < kSpmmColChunk; ++u) {
        const double tot = group_sum<kWave>(s[u]);
        if (lane == 0 && c0 + u < kp) partial[static_cast<long long>(c0 + u) * npieces + p] = tot;
      }
    }
  }
}

// One lane per (long row, panel column): the row's pieces in piece order, then alpha / beta.  long_rows[i] = row, first[i] .. first[i + 1] = its pieces.
__global__ __launch_bounds__(kThreads) void spmm_fixup_kernel(int m, int nlong, int npieces, int kp, long long syi, long long syj,
                                                              double alpha, double beta, const int *__restrict__ long_rows,
                                                              const int *__restrict__ first, const double *__restrict__ partial,
                                                              double *__restrict__ y, const int *__restrict__ rp,
                                                              const int *__restrict__ guard, int *__restrict__ stale) {
  check_plan_guard(rp, m, guard, stale);
  const long long e = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x;
  const bool live = e < static_cast<long long>(nlong) * kp;
  const int i = live ? static_cast<int>(e / kp) : 0, c = live ? static_cast<int>(e % kp) : 0;
  // (wave_range_sum hands a long range to the whole wavefront with the OWNER's offsets: every lane passes the same source pointer, the column's
  // plane is in the offsets -- kSpmmPanel * npieces < 2^31, npieces < 2 * nnz / kSpmmPiece; lanes without a row pass an empty range)
  const int base = c * npieces;
  const double s = wave_range_sum(partial, live ? base + first[i] : 0, live ? base + first[i + 1] : 0);
  if (live) {
    double *yp = y + long_rows[i] * syi + c * syj;
    *yp = beta == 0.0 ? alpha * s : alpha * s + beta * *yp;
  }
}

// Y = beta * Y over the m x k view (nnz == 0 or n == 0); beta == 0 writes zeros without reading Y
__global__ __launch_bounds__(kThreads) void spmm_scale_kernel(long long m, int k, long long syi, long long syj, double beta, double *y) {
  const long long total = m * k;
  const long long stride = static_cast<long long>(gridDim.x) * kThreads;
  for (long long e = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x; e < total; e += stride) {
    const long long r = syj == 1 ? e / k : e % m, c = syj == 1 ? e % k : e / m; // (consecutive lanes walk the contiguous dimension)
    double *yp = y + r * syi + c * syj;
    *yp = beta == 0.0 ? 0.0 : beta * *yp;
  }
}

template <int TS, bool SINGLE = false>
void launch_rows(hipStream_t st, const CsrDev &A, int kp, long long ldx, long long ldy, double alpha, double beta, const double *x, double *y) {
  SPMV_ACC_LAUNCH((spmm_rows_kernel<TS, SINGLE>), dim3(grid_for(A.m, kThreads / TS)), dim3(kThreads), 0, st, A.m, kp, kSpmmXcdRows / (kThreads / TS), ldx,
                  ldy, alpha, beta, A.rp, A.ci, A.v, x, y, A.guard, A.stale);
}

} // namespace

int spmm_team_lanes(int kp) {
  int ts = 1;
  while (2 * ts < kp && ts < kSpmmTeamMax) ts <<= 1;
  return ts;
}

void launch_spmm_rows(hipStream_t st, const CsrDev &A, bool row_major, int kp, long long ldx, long long ldy, double alpha, double beta,
                      const double *x, double *y) {
  if (A.m <= 0 || kp <= 0) return;
  if (!row_major) {
    SPMV_ACC_LAUNCH(spmm_rows_cm_kernel, dim3(grid_for(A.m, kThreads)), dim3(kThreads), 0, st, A.m, kp, kSpmmXcdRows / kThreads, ldx, ldy, alpha, beta,
                    A.rp, A.ci, A.v, x, y, A.guard, A.stale);
    return;
  }
  switch (spmm_team_lanes(kp)) {
  case 1:
    if (kp == 1) launch_rows<1, true>(st, A, kp, ldx, ldy, alpha, beta, x, y);
    else launch_rows<1>(st, A, kp, ldx, ldy, alpha, beta, x, y);
    break;
  case 2: launch_rows<2>(st, A, kp, ldx, ldy, alpha, beta, x, y); break;
  case 4: launch_rows<4>(st, A, kp, ldx, ldy, alpha, beta, x, y); break;
  case 8: launch_rows<8>(st, A, kp, ldx, ldy, alpha, beta, x, y); break;
  default: launch_rows<kSpmmTeamMax>(st, A, kp, ldx, ldy, alpha, beta, x, y); break;
  }
}

void launch_spmm_long(hipStream_t st, const CsrDev &A, const SpmmLong &L, bool row_major, int kp, long long ldx, long long ldy, double alpha,
                      double beta, const double *x, double *y) {
  if (L.nlong <= 0 || kp <= 0) return;
  const long long sxi = row_major ? ldx : 1, sxj = row_major ? 1 : ldx;
  const long long syi = row_major ? ldy : 1, syj = row_major ? 1 : ldy;
  SPMV_ACC_LAUNCH(spmm_pieces_kernel, dim3(grid_for(L.npieces, kThreads / kWave)), dim3(kThreads), 0, st, A.m, L.npieces, kp, sxi, sxj,
                  L.piece, A.rp, A.ci, A.v, x, L.partial, A.guard, A.stale);
  SPMV_ACC_LAUNCH(spmm_fixup_kernel, dim3(grid_for(static_cast<long long>(L.nlong) * kp, kThreads)), dim3(kThreads), 0, st, A.m, L.nlong,
                  L.npieces, kp, syi, syj, alpha, beta, L.rows, L.first, L.partial, y, A.rp, A.guard, A.stale);
}

void launch_spmm_scale(hipStream_t st, int m, int k, bool row_major, long long ldy, double beta, double *y) {
  if (m <= 0 || k <= 0) return;
  const long long syi = row_major ? ldy : 1, syj = row_major ? 1 : ldy;
  SPMV_ACC_LAUNCH(spmm_scale_kernel, dim3(grid_for(static_cast<long long>(m) * k, kThreads)), dim3(kThreads), 0, st, static_cast<long long>(m), k,
                  syi, syj, beta, y);
}

} // namespace spmv_acc
