// agg.hpp -- aggregation coarsening for a square CSR: the definition of the aggregates, the tentative prolongator's values and their summation
// order, size rules, launchers (k_agg.hip) and engine entries (agg.cpp) of
//   spmv_acc_csr_aggregate         the distance-2 independent roots and their aggregates (analysis: synchronises, not capturable), into caller-owned
//                                  arrays that ARE the CSR structures of P and of R = P^T,
//   spmv_acc_csr_tentative_values  the one-vector QR of smoothed aggregation: P's and R's values and the coarse vector (launch-only: per step).
// Constants, no tunables: nothing here is timed per matrix and nothing outlives a call (no plan, no cache entry).
// tests/test_agg_host.py AGG_SIZE_RULES names each rule and the GPU tests that cross it.
//
// THE AGGREGATES (a pure function of the pattern; tests/test_agg_host.py host_csr_aggregate restates it in numpy).  The input is the pattern of the
// STRENGTH GRAPH: square m x m, rebased CSR, rows strictly ascending, pattern symmetric -- the colouring's contract (gs.hpp), checked by the
// colouring's census; a stored diagonal is not required and values are not read.  For the matrix itself that is its own pattern; a filter that
// drops weak entries by a value threshold is OUT OF SCOPE here: spmv_acc_csr_strength (strength.hpp) does it, and its kept pattern is what is passed.
// Row v has the priority gs_priority(v) of gs.hpp.  Distances are counted over off-diagonal entries.
//   ROOTS.  The rows are taken in DESCENDING priority; a row becomes a root if no root already chosen lies within distance 2 of it: the
//           lexicographically first distance-2 maximal independent set.  An isolated row is a root.
//   IDS.    The roots are numbered 0 .. naggs - 1 in ascending row order.
//   A.      A non-root with a root neighbour joins that root's aggregate (two roots are never at distance 2: there is at most one).
//   B.      Every remaining row joins the smallest aggregate id held by a neighbour that was assigned as a root or in A.  B reads only A's
//           results (one buffer is read, another written).  By maximality every row is assigned after B.
//   OUTPUTS.  agg[v];  agg_rows = the rows in ascending (aggregate, row) -- a stable sort by aggregate --;  agg_ptr[a] = the first position of
//           aggregate a in agg_rows for a <= naggs, and m for naggs < a <= m;  *h_naggs.  (agg_ptr[0 .. naggs], agg_rows) is the CSR structure of
//           R = P^T with ascending rows, (0 .. m, agg) that of P: both go to csr_spgemm as they are, without a transpose.
//
// ROUNDS (host_csr_aggregate_rounds).  Every row holds a 64-bit key: kAggRoot (all ones) once it is a root, kAggOut (0) once a root lies within
// distance 2 of it, and gs_priority(v) + 1 while it is undecided -- above kAggOut, below kAggRoot, distinct for distinct rows.  (64 bits: gs_mix32 is
// a bijection on 32 bits, so its 2^32 values leave no room for two more in a 32-bit key; the high word alone orders the rows, the result cannot
// depend on the width.)  A round is two launches of ONE pass, the maximum over the closed neighbourhood N[v] = {v} and its off-diagonal
// neighbours:  T1[v] = max key over N[v],  T2[v] = max T1 over N[v] = the largest key within distance 2.  An undecided v then becomes
//   kAggOut if T2[v] is kAggRoot (a root within distance 2),  a root if T2[v] is its own key (nothing undecided of higher priority within
//   distance 2, and no root), and waits otherwise.
// The second launch writes key[v] in place: it reads T1 of other rows and the key of its own row only.  The undecided row of highest priority is
// decided in every round, a root takes what the sequential order gives it, and so the roots are the sequential ones whatever the timing; the
// number of rounds is a function of the pattern too.  Rounds are enqueued kAggRoundsPerRead at a time; then the host reads how many rows are
// undecided (per-wavefront counts, no atomic).  A group of rounds that decides no row while some remain ends the call with an error: the loop
// cannot spin.  max is exact, so the mapping of lanes to rows (kAggLaneGroup) cannot change a bit of the result.
//
// THE TENTATIVE VALUES (tests/test_agg_host.py host_tentative_values restates them bit for bit).  b is the fine near-nullspace vector (NULL: all
// ones).  For aggregate a, with the run [agg_ptr[a], agg_ptr[a + 1]) of agg_rows clamped to [0, m]:
//   s[a]  = the sum over the run's positions p of  b[agg_rows[p]] * b[agg_rows[p]]  -- every product rounded on its own (contraction is off),
//           +0.0 for an agg_rows[p] outside [0, m) --, added in THE SUMMATION ORDER of coo.hpp (passes::sum_runs: a run of at most kCooLongRun
//           terms by one lane from its first term, a longer one by a wavefront; an empty run gives +0.0);
//   bc[a] = sqrt(s[a]), correctly rounded: the coarse near-nullspace vector of the next level;
//   p_value[i] = b[i] / bc[agg[i]], and +0.0 where bc[agg[i]] is zero or agg[i] lies outside [0, naggs);
//   r_value[p] = p_value[agg_rows[p]] (recomputed, not read back: the same bits), and +0.0 for an agg_rows[p] outside [0, m).
// With b == NULL every p_value is 1 / sqrt(the aggregate's size).  Two launches: the norms, then the values.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>

#include "gs.hpp"

namespace spmv_acc {

constexpr unsigned long long kAggRoot = ~0ull;  // the key of a root: above every priority
constexpr unsigned long long kAggOut = 0ull;    // the key of a row with a root within distance 2: below every priority (an undecided row: gs_priority + 1)
constexpr int kAggRoundsPerRead = 4;   // rounds enqueued between two reads of the undecided count.  Meshes need 8 to 12 rounds: a group of four
                                       // overshoots by one and a half rounds on average (a round = two passes over the pattern) and reads three times;
                                       // a group of eight, as in the colouring, would overshoot by four.  Reasoned from the round counts, not timed
constexpr int kAggLaneGroup = 1;       // lanes per row of the neighbourhood pass (a power of two, 1 .. 64).  MEASURED on an MI355X with 1, 4 and 8
                                       // (tools/agg_bench.py --lib, profiles/agg_bench.md): on the 27-point grid four lanes per row gain 2 to 4 % of
                                       // the whole call and eight lose 8 %; on the 9-point mesh four lose 35 % and eight 120 %.  One row per lane
constexpr int kAggPerLane = 1;         // norms pass: aggregates per lane of passes::sum_runs.  MEASURED with 1, 2 and 4 (the same tool and file): an
                                       // aggregate is tens of rows, so there are few runs and each is a chain of dependent gathers -- what the pass
                                       // lacks is wavefronts, not loads in flight per lane; 4 per lane takes 1.7 x the time of 1 on the 27-point grid
constexpr int kAggWaveChunk = 64 * kAggPerLane;  // ... so one wavefront owns 64 consecutive aggregates,
constexpr int kAggTile = 4 * kAggWaveChunk;      // ... one workgroup a tile of 256

// the key of an undecided row
constexpr unsigned long long agg_key(unsigned v) { return gs_priority(v) + 1ull; }

// ---- launchers (k_agg.hip): enqueue only ---------------------------------------------------------------------------------------------------
// the neighbourhood pass: out[v] = max of in over N[v] (rows read clamped, a column outside [0, m) is skipped).  m > 0
void launch_agg_max(hipStream_t stream, int m, int nnz, const int *rowptr, const int *colindex, const unsigned long long *in,
                    unsigned long long *out);
// ... and the deciding form: t2 = max of t1 over N[v] for every undecided v, key[v] decided in place (agg.hpp ROUNDS);
// slots[0 .. kCooCheckSlots) = per-wavefront counts of the rows still undecided
void launch_agg_decide(hipStream_t stream, int m, int nnz, const int *rowptr, const int *colindex, const unsigned long long *t1,
                       unsigned long long *key, unsigned *slots);
// key[v] = agg_key(v)
void launch_agg_init(hipStream_t stream, int m, unsigned long long *key);
// flag[v] = 1 where key[v] is kAggRoot, v < m; flag[m] = 0
void launch_agg_flags(hipStream_t stream, int m, const unsigned long long *key, int *flag);
// assignment A: first[v] = id[v] for a root (id = the exclusive scan of the flags), id[u] for a non-root with the root neighbour u, else -1
void launch_agg_assign_roots(hipStream_t stream, int m, int nnz, const int *rowptr, const int *colindex, const int *flag, const int *id,
                             int *first);
// assignment B: agg[v] = first[v] where that is assigned, else the smallest assigned first[u] of a neighbour u (-1 if there is none);
// slots[0 .. kCooCheckSlots) = per-wavefront counts of the rows left at -1
void launch_agg_assign_rest(hipStream_t stream, int m, int nnz, const int *rowptr, const int *colindex, const int *first, int *agg,
                            unsigned *slots);
// bc[a] = sqrt(s[a]), a < naggs (agg.hpp THE TENTATIVE VALUES); b == nullptr: all ones.  m > 0, naggs > 0
void launch_agg_norms(hipStream_t stream, int m, int naggs, const int *agg_ptr, const int *agg_rows, const double *b, double *bc);
// p_value[i], i < m, and r_value[p], p < m (nullptr: not wanted).  m > 0
void launch_agg_values(hipStream_t stream, int m, int naggs, const int *agg, const int *agg_rows, const double *b, const double *bc,
                       double *p_value, double *r_value);

// ---- engine entries (agg.cpp): return kOk or the error code they also leave in the calling thread's error slot --------------------------------
int run_csr_aggregate(int m, int nnz, const int *d_rowptr, const int *d_colindex, int *d_agg, int *d_agg_rows, int *d_agg_ptr, int *h_naggs);
int run_csr_tentative_values(int m, int naggs, const int *d_agg, const int *d_agg_ptr, const int *d_agg_rows, const double *d_b,
                             double *d_p_value, double *d_r_value, double *d_bc);

} // namespace spmv_acc
