"""Preconditioned conjugate gradients on the device (pcg), composed on the host from the package's entries.

No new device code lives here.  The residual and q = A p are csr_spmv calls; the dot products, the scalars that depend on them and the vector
updates are cg_start, cg_update and cg_direction, whose scalars never leave the GPU; the preconditioner is nothing, the inverse diagonal
(fused into cg_direction), one V-cycle of an AmgHierarchy, or the caller's function.  The host reads the nine-word state block once per
`check_every` iterations; the entries freeze once the status is set, so the solution's bits do not depend on how often it looks."""
from __future__ import annotations

import math
from collections import namedtuple

from . import (CG_STATE, CG_STATUS, SpmvAccError, cg_direction, cg_partials, cg_start, cg_update, csr_extract, csr_spmv, _require_tensors)
from .amg import AmgHierarchy, amg_cycle

# status: the state block's word 0 (0 running -- maxiter was reached --, 1 converged, 2 breakdown with p.q not finite or <= 0, 3 breakdown with
# r.z not finite or < 0; CG_STATUS holds the words); iterations: updates of x done; rr, bb: r.r of the last residual and b.b, so that
# sqrt(rr / bb) is the relative residual of the recurrence; history: r.r of iterations 0 .. iterations as a list, or None.
CgResult = namedtuple("CgResult", "status iterations rr bb history")


def jacobi_inverse(m: int, rowptr, colindex, value):
    """1 / diag(A) as an fp64 GPU tensor of m entries, for pcg(precond=...): the diagonal by csr_extract(..., diag_lo=0, diag_hi=0), the
    reciprocal by torch -- setup, not the hot path.  A row without a stored diagonal entry is refused."""
    import torch

    if m < 0:
        raise SpmvAccError(f"negative shape ({m}, {m})")
    _require_tensors(rowptr=rowptr, colindex=colindex, value=value)
    d_rowptr, _, d_value = csr_extract(m, m, rowptr, colindex, value, diag_lo=0, diag_hi=0)
    if int(d_value.numel()) != m or (m and not bool((d_rowptr[1:] - d_rowptr[:-1] == 1).all())):
        raise SpmvAccError(f"jacobi_inverse: {m - int(d_value.numel())} more rows than stored diagonal entries: every row needs one")
    return torch.reciprocal(d_value)


def pcg(m: int, rowptr, colindex, value, b, x, precond=None, rtol: float = 1e-8, maxiter: int = 1000, check_every: int = 8, history: bool = False,
        pre: int = 1, post: int = 1) -> CgResult:
    """Solve A x = b by preconditioned conjugate gradients, x in place from the x0 it holds, until r.r <= (rtol * rtol) * b.b for the
    recurrence's residual r, a breakdown, or maxiter iterations.  A: square m x m CSR, symmetric positive definite.  precond:
      None             no preconditioner;
      an fp64 tensor   of m entries on the GPU: the inverse diagonal (jacobi_inverse), applied inside cg_direction;
      an AmgHierarchy  of amg_setup whose finest level has m rows: z = 0, then one amg_cycle(h, r, z, pre, post, "symmetric").  THE ZERO START
                       AND THE SYMMETRIC SWEEPS, with pre == post (the caller's to keep), are what make the cycle a symmetric operator
                       z = M r, which conjugate gradients need: a forward-only sweep, a warm start or pre != post would give a
                       preconditioner that is not symmetric, and a breakdown or a stall.  A hierarchy of a Jacobi smoother
                       (amg_setup(smoother=...)) is cycled with zero_start=True instead of z = 0; pre == post keeps M symmetric;
      a callable       precond(r, z) writes z = M r for a symmetric positive definite M, on torch's current stream.
    The order of an iteration: q = A p (csr_spmv); cg_update; z = M r; cg_direction.  The host reads the state block -- one copy of 72 bytes --
    after every check_every iterations and at maxiter, never inside a batch; iterations enqueued past the end of the solve write nothing, so x
    is bit for bit the same for every check_every.  maxiter is exact: no iteration beyond it is enqueued.  A breakdown or an unconverged solve
    is RETURNED (CgResult.status, CG_STATUS), not raised; SpmvAccError is raised for arguments only.  Synchronises at every read."""
    import torch

    if m < 0:
        raise SpmvAccError(f"negative shape ({m}, {m})")
    if not (isinstance(rtol, (int, float)) and math.isfinite(rtol) and rtol >= 0.0):
        raise SpmvAccError(f"rtol = {rtol}: a finite tolerance >= 0 is required")
    if int(maxiter) < 0 or int(check_every) < 1:
        raise SpmvAccError(f"maxiter = {maxiter}, check_every = {check_every}: maxiter must be at least 0 and check_every at least 1")
    if int(pre) < 0 or int(post) < 0:
        raise SpmvAccError(f"negative sweeps ({pre}, {post})")
    _require_tensors(rowptr=rowptr, colindex=colindex, value=value, b=b, x=x)
    for name, t in (("b", b), ("x", x)):
        if int(t.numel()) != m:
            raise SpmvAccError(f"{name} holds {int(t.numel())} elements, a vector of the {m} rows must hold as many")
    dinv = None
    if isinstance(precond, AmgHierarchy):
        if precond.sizes[0] != m:
            raise SpmvAccError(f"precond: the hierarchy's finest level has {precond.sizes[0]} rows, the matrix {m}")
    elif precond is not None and not callable(precond):
        _require_tensors(precond=precond)
        if int(precond.numel()) != m:
            raise SpmvAccError(f"precond holds {int(precond.numel())} elements, the inverse diagonal of the {m} rows must hold as many")
        dinv = precond
    maxiter, check_every = int(maxiter), int(check_every)
    nnz = int(colindex.numel())
    dev = b.device
    r, p, q = (torch.empty(m, dtype=torch.float64, device=dev) for _ in range(3))
    z = r if precond is None else torch.empty(m, dtype=torch.float64, device=dev)
    partials = torch.empty(cg_partials(m), dtype=torch.float64, device=dev)
    state = torch.zeros(CG_STATE, dtype=torch.int64, device=dev)
    hist = torch.zeros(maxiter + 1, dtype=torch.float64, device=dev) if history else None

    def apply_precond():
        if isinstance(precond, AmgHierarchy):
            if precond.smoother == "gs":
                z.zero_()
                amg_cycle(precond, r, z, int(pre), int(post), "symmetric")
            else:  # a Jacobi hierarchy starts from zero itself and never reads what z holds
                amg_cycle(precond, r, z, int(pre), int(post), "symmetric", zero_start=True)
        elif dinv is None and precond is not None:
            precond(r, z)

    def read_state():
        words = state.cpu()
        return int(words[0]), int(words[1]), words.view(torch.float64)

    csr_spmv(-1.0, 1.0, m, m, nnz, rowptr, colindex, value, x, r, y_in=b)  # r = b - A x
    if dinv is not None:
        torch.mul(dinv, r, out=z)  # (the first z; every later one is fused into cg_direction)
    else:
        apply_precond()
    cg_start(m, rtol, b, r, z, p, partials, state, hist)
    enqueued = 0
    status, done, words = read_state()
    while status == 0 and enqueued < maxiter:
        for _ in range(min(check_every, maxiter - enqueued)):
            csr_spmv(1.0, 0.0, m, m, nnz, rowptr, colindex, value, p, q)  # q = A p
            cg_update(m, p, q, x, r, partials, state, hist)
            apply_precond()
            cg_direction(m, r, z, p, partials, state, dinv)
            enqueued += 1
        status, done, words = read_state()
    assert status in range(len(CG_STATUS)) and done <= enqueued
    return CgResult(status, done, float(words[3]), float(words[2]), hist[:done + 1].cpu().tolist() if history else None)
