"""Smoothed-aggregation AMG on the device: the hierarchy (amg_setup) and the V-cycle (amg_cycle), composed on the host from the package's entries.

No new device code lives here.  A level is the recipe of ``csr_smooth_prolongator``'s docstring, unchanged and in its order -- csr_strength,
csr_aggregate on the kept pattern, csr_tentative, csr_smooth_prolongator, csr_transpose, two csr_spgemm for A_c = R (A P) --; the restriction
and the prolongation are csr_spmv calls, whose plans are keyed by each matrix' rowptr; the coarsest level is solved by csr_dense_inverse
once and dense_apply per cycle.  A cycle therefore never leaves the GPU.

The smoother is chosen at setup (amg_setup(smoother=...)):
  "gs" (the default)       the multicolour Gauss-Seidel sweep: csr_color once per level, csr_gs_sweep per cycle -- one launch per colour and
                           direction --, the residual by csr_spmv;
  "jacobi", "l1_jacobi"    the one-launch sweep: csr_jacobi_diagonal once per level (no colouring), csr_jacobi_sweep per cycle, out of place
                           between x and one work vector of the level; the residual by the same entry's r_out form, so that no pass over a
                           level's A needs a plan; the first pre-sweep of every coarse level in the zero-start form, which does not read A.

omega (the prolongator smoother's relaxation) stays the caller's to choose: 2/3 suits a diagonally dominant filtered matrix."""
from __future__ import annotations

import math
from collections import namedtuple

from . import (DENSE_MAX_ROWS, SpmvAccError, csr_aggregate, csr_color, csr_dense_inverse, csr_gs_sweep, csr_jacobi_diagonal, csr_jacobi_sweep,
               csr_smooth_prolongator, csr_spgemm, csr_spmv, csr_strength, csr_tentative, csr_transpose, dense_apply, release_plans,
               _GS_DIRECTIONS, _require_tensors)

# One non-coarsest level: A = (rowptr, colindex, value) of m rows; P (m x mc) and R = P^T (mc x m) likewise; the colouring of A (color_ptr a
# host list; None under a Jacobi smoother, which needs none); the work vectors r (m), bc and xc (mc each), zero-initialised; keep: every other
# array of the level's setup, kept alive; under a Jacobi smoother dinv (m, csr_jacobi_diagonal) and xw (m), the other vector of the
# out-of-place sweeps' ping-pong (None under Gauss-Seidel).
AmgLevel = namedtuple("AmgLevel", "m mc A P R color_ptr color_rows r bc xc keep dinv xw", defaults=(None, None))
# The coarsest level: A of m rows, its dense inverse (m, m), and the rule that ended the hierarchy ("coarse_rows", "max_levels" or "stall").
AmgCoarsest = namedtuple("AmgCoarsest", "m A inv rule")

# smoother -> (the kind of csr_jacobi_diagonal, or None for Gauss-Seidel; the omega that smoother_omega=None stands for)
_SMOOTHERS = {"gs": (None, 1.0), "jacobi": ("jacobi", 2.0 / 3.0), "l1_jacobi": ("l1", 1.0)}

_RULES = {"coarse_rows": "its rows are at most coarse_rows", "max_levels": "it is level max_levels",
          "stall": "the aggregation stalled (2 * naggs > m)"}


class AmgHierarchy:
    """levels: the non-coarsest levels, finest first (AmgLevel tuples); coarsest: an AmgCoarsest tuple.  Holds every array the cycle reads:
    the SpMV plans are keyed by the rowptr arrays, which must stay alive and in place.  release() drops those plans.  smoother ("gs",
    "jacobi" or "l1_jacobi") and smoother_omega: what amg_setup built the levels for and amg_cycle sweeps with."""

    def __init__(self, levels, coarsest, smoother="gs", smoother_omega=1.0):
        self.levels = list(levels)
        self.coarsest = coarsest
        self.smoother = smoother
        self.smoother_omega = float(smoother_omega)

    @property
    def sizes(self):
        """The rows of every level, finest first."""
        return [lv.m for lv in self.levels] + [self.coarsest.m]

    def release(self) -> None:
        """release_plans on every rowptr of the hierarchy (A, P and R of each level)."""
        for lv in self.levels:
            for mat in (lv.A, lv.P, lv.R):
                release_plans(mat[0])
        if self.coarsest.m:
            release_plans(self.coarsest.A[0])


def amg_setup(m: int, rowptr, colindex, value, theta: float = 0.0, omega: float = 2.0 / 3.0, coarse_rows: int = 256, max_levels: int = 16,
              b=None, smoother="gs", smoother_omega=None) -> AmgHierarchy:
    """The hierarchy of a square m x m CSR with strictly ascending rows and a symmetric pattern (the contract of csr_strength).  theta: the
    strength threshold of every level; omega: the prolongator smoother's relaxation; b: the near-nullspace vector of the finest level (None:
    ones), each coarser level takes the bc of csr_tentative.  A level becomes the coarsest when its rows are at most coarse_rows, when it is
    level max_levels (counted from 1), or when its aggregation stalls: 2 * naggs > m.  The coarsest level is inverted densely
    (csr_dense_inverse): more than DENSE_MAX_ROWS rows there, or a singular matrix, raise SpmvAccError.  Synchronises; not capturable.
    smoother: "gs" (multicolour Gauss-Seidel, the default), "jacobi" (dinv = 1 / a_ii) or "l1_jacobi" (the scaled l1 diagonal of
    csr_jacobi_diagonal); the two Jacobi kinds skip csr_color and hold dinv and one more work vector per level.  smoother_omega: the sweeps'
    relaxation, for all three (under "gs" it is csr_gs_sweep's omega: SOR); None is 1.0 for "gs" and "l1_jacobi" -- l1 at omega <= 1
    contracts on every symmetric positive definite matrix and needs no choice -- and 2/3 for "jacobi".  DAMPING PLAIN JACOBI IS THE CALLER'S RESPONSIBILITY: it converges only for omega < 2 / the largest
    eigenvalue of D^-1 A, which 2/3 meets on a diagonally dominant matrix and nothing guarantees elsewhere."""
    if smoother not in _SMOOTHERS:
        raise SpmvAccError(f"smoother {smoother!r}: one of {tuple(_SMOOTHERS)}")
    kind, default_omega = _SMOOTHERS[smoother]
    if smoother_omega is None:
        smoother_omega = default_omega
    if not (isinstance(smoother_omega, (int, float)) and math.isfinite(smoother_omega) and smoother_omega != 0.0):
        raise SpmvAccError(f"smoother_omega = {smoother_omega}: a finite, non-zero relaxation factor is required")
    if m < 0:
        raise SpmvAccError(f"negative shape ({m}, {m})")
    if int(coarse_rows) < 1 or int(max_levels) < 1:
        raise SpmvAccError(f"coarse_rows = {coarse_rows}, max_levels = {max_levels}: both must be at least 1")
    if not (math.isfinite(theta) and theta >= 0.0):
        raise SpmvAccError(f"theta = {theta}: a finite threshold >= 0 is required")
    if not math.isfinite(omega) or omega == 0.0:
        raise SpmvAccError(f"omega = {omega}: a finite, non-zero relaxation factor is required")
    _require_tensors(rowptr=rowptr, colindex=colindex, value=value)
    import torch

    dev = rowptr.device
    levels = []
    A = (rowptr, colindex, value)
    level = 1
    while True:
        rule = "coarse_rows" if m <= coarse_rows else ("max_levels" if level == max_levels else None)
        if rule is None:
            S, smap, drop_ptr, diag, _ = csr_strength(m, *A, theta)
            agg, agg_ptr, agg_rows, naggs = csr_aggregate(m, S[0], S[1])
            if 2 * naggs > m:
                rule = "stall"
        if rule is not None:
            if m > DENSE_MAX_ROWS:
                raise SpmvAccError(f"the coarsest level (level {level}) holds {m} rows, the dense inverse takes at most {DENSE_MAX_ROWS}: the "
                                   f"hierarchy ended there because {_RULES[rule]}")
            inv, info = csr_dense_inverse(m, *A)
            if info != 0:
                raise SpmvAccError(f"the coarsest level (level {level}, {m} rows) is singular: the pivot of step {info - 1} of its dense inverse "
                                   f"was zero or not finite (info = {info})")
            return AmgHierarchy(levels, AmgCoarsest(m, A, inv, rule), smoother=smoother, smoother_omega=smoother_omega)
        T, _, bc = csr_tentative(m, agg, agg_ptr, agg_rows, b)
        P = csr_smooth_prolongator(m, naggs, S[0], S[1], smap, drop_ptr, A[2], T, omega)
        R = csr_transpose(m, naggs, int(P[1].numel()), *P)
        AP = csr_spgemm(m, m, naggs, *A, *P)
        Ac = csr_spgemm(naggs, m, naggs, *R, *AP)
        keep = (S, smap, drop_ptr, diag, agg, agg_ptr, agg_rows, T, bc, AP)
        work = [torch.zeros(n, dtype=torch.float64, device=dev) for n in (m, naggs, naggs)]
        if kind is None:
            _, color_rows, color_ptr, _ = csr_color(m, A[0], A[1])
            levels.append(AmgLevel(m, naggs, A, P, R, color_ptr, color_rows, *work, keep=keep))
        else:
            levels.append(AmgLevel(m, naggs, A, P, R, None, None, *work, keep=keep, dinv=csr_jacobi_diagonal(m, *A, kind=kind),
                                   xw=torch.zeros(m, dtype=torch.float64, device=dev)))
        A, m, b = Ac, naggs, bc
        level += 1


def amg_cycle(h: AmgHierarchy, b, x, pre: int = 1, post: int = 1, direction="symmetric", zero_start: bool = False) -> None:
    """One V-cycle on x towards A x = b, in place, asynchronous on torch's current stream.  On a non-coarsest level: `pre` sweeps of the
    hierarchy's smoother at its smoother_omega; r = b - A x; b_c = R r; x_c = 0; the cycle on the next level; x += P x_c; `post` sweeps.  On
    the coarsest level x = inv b (dense_apply): a hierarchy of one level is a direct solve.  b must not overlap x.  The smoother is the one
    amg_setup built the hierarchy for:
      "gs"                   csr_gs_sweep in `direction` (omega = smoother_omega: SOR where it is not 1), in place; r by csr_spmv;
      "jacobi", "l1_jacobi"  csr_jacobi_sweep, out of place between x and the level's work vector (an odd number of such sweeps is followed
                             by a copy back into x); r from the same entry's r_out form; every coarse level's first pre-sweep starts from
                             zero without reading its matrix; `direction` is validated and otherwise ignored.
    zero_start: the caller's promise that x is zero, so that a Jacobi hierarchy's finest level starts that way too and what x holds is
    never read (for finite values the same bits as zero_start=False from an x of zeros); ignored under Gauss-Seidel."""
    if not isinstance(h, AmgHierarchy):
        raise SpmvAccError("h: the AmgHierarchy of amg_setup is required")
    if int(pre) < 0 or int(post) < 0:
        raise SpmvAccError(f"negative sweeps ({pre}, {post})")
    if direction not in _GS_DIRECTIONS:  # (here, not only in csr_gs_sweep: a hierarchy of one level never sweeps)
        raise SpmvAccError(f"amg_cycle: direction {direction!r}: one of {tuple(_GS_DIRECTIONS)}")
    _require_tensors(b=b, x=x)
    if h.smoother != "gs":
        _cycle_jacobi(h, 0, b, x, int(pre), int(post), bool(zero_start))
        return
    _cycle(h, 0, b, x, int(pre), int(post), direction)


def _cycle(h, depth, b, x, pre, post, direction) -> None:
    if depth == len(h.levels):
        dense_apply(h.coarsest.m, h.coarsest.inv, b, x)
        return
    lv = h.levels[depth]
    n, nc = lv.m, lv.mc
    csr_gs_sweep(n, *lv.A, lv.color_ptr, lv.color_rows, b, x, omega=h.smoother_omega, direction=direction, sweeps=pre)
    csr_spmv(-1.0, 1.0, n, n, int(lv.A[1].numel()), *lv.A, x, lv.r, y_in=b)  # r = b - A x
    csr_spmv(1.0, 0.0, nc, n, int(lv.R[1].numel()), *lv.R, lv.r, lv.bc)  # b_c = R r
    lv.xc.zero_()
    _cycle(h, depth + 1, lv.bc, lv.xc, pre, post, direction)
    csr_spmv(1.0, 1.0, n, nc, int(lv.P[1].numel()), *lv.P, lv.xc, x)  # x += P x_c
    csr_gs_sweep(n, *lv.A, lv.color_ptr, lv.color_rows, b, x, omega=h.smoother_omega, direction=direction, sweeps=post)


def _cycle_jacobi(h, depth, b, x, pre, post, zero) -> None:
    """zero: x counts as zero whatever it holds (a coarse level's x_c, or the caller's promise): it is written before it is read."""
    if depth == len(h.levels):
        dense_apply(h.coarsest.m, h.coarsest.inv, b, x)
        return
    lv = h.levels[depth]
    n, nc = lv.m, lv.mc
    cur, other = x, lv.xw  # cur holds the iterate; every sweep from a non-zero x writes the other vector

    def sweeps(count, cur, other, zero):
        for _ in range(count):
            if zero:  # x_out = omega * dinv * b: A is not read, and nothing is read from cur
                csr_jacobi_sweep(n, *lv.A, lv.dinv, b, None, x_out=cur, omega=h.smoother_omega)
                zero = False
            else:
                csr_jacobi_sweep(n, *lv.A, lv.dinv, b, cur, x_out=other, omega=h.smoother_omega)
                cur, other = other, cur
        return cur, other, zero

    cur, other, zero = sweeps(pre, cur, other, zero)
    if zero:  # (pre == 0)
        cur.zero_()
    csr_jacobi_sweep(n, *lv.A, lv.dinv, b, cur, r_out=lv.r, omega=h.smoother_omega)  # r = b - A x, in the sweep's order: no plan
    csr_spmv(1.0, 0.0, nc, n, int(lv.R[1].numel()), *lv.R, lv.r, lv.bc)  # b_c = R r
    _cycle_jacobi(h, depth + 1, lv.bc, lv.xc, pre, post, True)
    csr_spmv(1.0, 1.0, n, nc, int(lv.P[1].numel()), *lv.P, lv.xc, cur)  # x += P x_c
    cur, other, _ = sweeps(post, cur, other, False)
    if cur is not x:  # an odd number of out-of-place sweeps ended in the work vector
        x.copy_(cur)
