#!/usr/bin/env python3
"""The conjugate-gradient vector passes (spmv_acc_cg_start, spmv_acc_cg_update, spmv_acc_cg_direction) and the solver composed of them
(spmv_acc_amd.pcg), on tools/amg_bench.py's two matrices (`fem_quads`, 4.0 M rows, 9-point; `grid27`, 3.4 M rows, 27-point; Dirichlet ends,
theta = 0.05, omega = 2/3, coarse_rows = 256).  One JSON line per matrix:
  entries, at n = the matrix' rows, on random vectors with q = w p for a positive w (no SpMV inside the timed region):
    start_ms, update_ms, direction_ms, direction_jacobi_ms
                     one call: median of 7 regions of 20 calls between one event pair.  rtol = 0 and a status that stays 0 (every region
                     begins from the same p, q, x, r, restored outside the event pair; the scalars stay finite over 20 calls because q = w p
                     keeps alpha bounded and r is reset).  CACHE-WARM: a region is about 1 ms of calls on four or five vectors of 32 MB, which stay
                     in the 256 MB Infinity Cache between calls, and so do the copy's buffers; inside a solve a matrix of 0.4 to 1 GB passes
                     between two entries, so the entry / copy ratios are those of the passes themselves, not of an entry inside a solve
    *_bytes          the bytes the entry's passes move, REASONED from the definitions: start 3 reads + 1 write of n doubles; update 2 reads, then
                     4 reads + 2 writes: 8 n doubles; direction 2 reads, then 2 reads + 1 write: 5 n doubles (with dinv one read and one write
                     more: 7 n); the partials (n / 1024 doubles per dot) are not counted
    *_copy_ms        torch's device copy of as many bytes (half read, half written), same protocol; *_over_copy = the entry over it
  solves, b standard normal from seed 5, x0 = 0, rtol = 1e-8, after one throw-away solve in which the SpMV plans settle; every time is the
  MEDIAN OF 3 solves from x0 = 0 (host clock between device synchronisations; *_samples_ms holds the three), the counts and residuals are the last one's:
    amg_pcg_ms, amg_pcg_iterations       pcg with the hierarchy as M (check_every = 8); the call ends in a state read
    jacobi_pcg_ms, jacobi_pcg_iterations pcg with the inverse diagonal, maxiter = 5000; status 0 means it did not converge within them
    stationary_ms, stationary_cycles     amg_cycle repeated, the residual |b - A x| / |b| read every 8 cycles (one SpMV and two norms), until it
                                         is at most 1e-8 or 400 cycles are done
    *_residual       the true relative residual |b - A x| / |b| at the end of each
    setup_ms         amg_setup, one call (tools/amg_bench.py measures it properly)
Every child process measures one matrix under a time limit; after a child that fails or runs out of time nothing more is started.
usage: tools/cg_bench.py OUT.json [--parts fem_quads,grid27] [--md OUT.md] [--limit SECONDS] [--scale 1.0] [--headline FILE]"""
import argparse
import json
import os
import subprocess
import sys
import time

THETA = 0.05
OMEGA = 2.0 / 3.0
RTOL = 1e-8
MAX_CYCLES, MAX_JACOBI = 400, 5000


def child(name, scale):
    import numpy as np
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import spmv_acc_amd

    def stencil(shape, weak_of, weak):
        """tools/amg_bench.py's matrices: the full 3^d stencil on a grid of `shape` points with anisotropic values and Dirichlet ends, rows
        strictly ascending; weak_of(offset) names the couplings that get `weak` instead of 1"""
        m = int(np.prod(shape))
        coords = torch.unravel_index(torch.arange(m, device="cuda"), shape)
        cols, valid, size = [], [], []
        for off in np.ndindex(*([3] * len(shape))):
            rel = tuple(o - 1 for o in off)
            centre = all(o == 0 for o in rel)
            ok = torch.ones(m, dtype=torch.bool, device="cuda")
            col = torch.zeros(m, dtype=torch.int64, device="cuda")
            for c, o, s in zip(coords, rel, shape):
                q = c + o
                ok &= (q >= 0) & (q < s)
                col = col * s + q
            cols.append(col)
            valid.append(ok)
            size.append(0.0 if centre else (weak if weak_of(rel) else 1.0))
        cols, valid = torch.stack(cols, 1), torch.stack(valid, 1)
        lens = valid.sum(1)
        rp = torch.zeros(m + 1, dtype=torch.int32, device="cuda")
        rp[1:] = torch.cumsum(lens, 0).int()
        ci = cols[valid].int()
        row = torch.repeat_interleave(torch.arange(m, device="cuda"), lens)
        gen = torch.Generator(device="cuda").manual_seed(2033)
        base = torch.tensor(size, dtype=torch.float64, device="cuda").expand(m, -1)[valid]
        v = -base * (0.9 + 0.2 * torch.rand(ci.numel(), dtype=torch.float64, device="cuda", generator=gen))
        outside = ((~valid).double() * torch.tensor(size, dtype=torch.float64, device="cuda")).sum(1)
        diag = torch.zeros(m, dtype=torch.float64, device="cuda").index_add_(0, row, v.abs()) + outside
        v = torch.where(ci.long() == row, diag[row], v)
        return m, rp, ci.contiguous(), v.contiguous()

    def median_region(fn, reset=None, reps=20, regions=7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        out = []
        for _ in range(regions):
            if reset:
                reset()
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) / reps)
        return float(np.median(out))

    if name == "fem_quads":
        side = max(8, int(2001 * scale))
        m, rp, ci, v = stencil((side, side), lambda off: all(o != 0 for o in off), 0.05)
    elif name == "grid27":
        side = max(4, int(150 * scale ** (2.0 / 3.0)))
        m, rp, ci, v = stencil((side, side, side), lambda off: sum(o != 0 for o in off) == 3 or (off[2] == 0 and sum(o != 0 for o in off) == 2), 0.02)
    else:
        raise SystemExit(f"unknown part {name}")
    nnz = ci.numel()
    print(f"# {name}: {m} rows, {nnz} non-zeros", file=sys.stderr, flush=True)
    lib = spmv_acc_amd.load_library()
    out = {"part": name, "m": m, "nnz": nnz}

    # ---- the entries alone ------------------------------------------------------------------------------------------------------------------
    gen = torch.Generator(device="cuda").manual_seed(7)
    rand = lambda: torch.randn(m, dtype=torch.float64, device="cuda", generator=gen)  # noqa: E731
    b, r0, x0, p0 = rand(), rand(), rand(), rand()
    w = 0.5 + torch.rand(m, dtype=torch.float64, device="cuda", generator=gen)
    dinv = 1.0 / w
    r, x, p, z = r0.clone(), x0.clone(), p0.clone(), torch.empty_like(r0)
    q = w * p
    partials = torch.empty(spmv_acc_amd.cg_partials(m), dtype=torch.float64, device="cuda")
    state = torch.zeros(spmv_acc_amd.CG_STATE, dtype=torch.int64, device="cuda")

    def reset():
        r.copy_(r0)
        x.copy_(x0)
        p.copy_(p0)
        torch.mul(dinv, r, out=z)
        spmv_acc_amd.cg_start(m, 0.0, b, r, z, p, partials, state)
        torch.mul(w, p, out=q)

    timed = (("start", lambda: spmv_acc_amd.cg_start(m, 0.0, b, r, z, p, partials, state), 4),
             ("update", lambda: spmv_acc_amd.cg_update(m, p, q, x, r, partials, state), 8),
             ("direction", lambda: spmv_acc_amd.cg_direction(m, r, z, p, partials, state), 5),
             ("direction_jacobi", lambda: spmv_acc_amd.cg_direction(m, r, z, p, partials, state, dinv=dinv), 7))
    for label, fn, doubles in timed:
        reset()
        fn()
        ms = median_region(fn, reset)
        torch.cuda.synchronize()
        status = int(state.cpu()[0])
        nbytes = 8 * doubles * m
        src = torch.empty(nbytes // 16, dtype=torch.float64, device="cuda")
        dst = torch.empty_like(src)
        copy_ms = median_region(lambda: dst.copy_(src))
        out.update({label + "_ms": round(ms, 5), label + "_bytes": nbytes, label + "_copy_ms": round(copy_ms, 5), label + "_over_copy": round(ms / copy_ms, 2),
                    label + "_status_after": status})
        del src, dst
    del r, x, p, z, q, r0, x0, p0, w, dinv

    # ---- the solves ---------------------------------------------------------------------------------------------------------------------------
    b = torch.randn(m, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    bnorm = float(b.norm().item())
    res = torch.empty_like(b)

    def residual(x):
        spmv_acc_amd.csr_spmv(-1.0, 1.0, m, m, nnz, rp, ci, v, x, res, y_in=b)
        return float(res.norm().item()) / bnorm

    def wall(fn, calls=1):
        """(the median of `calls` host-clock times in ms, every sample, the last call's result)"""
        ts = []
        for _ in range(calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts)), [round(t, 2) for t in ts], got

    setup_ms, _, h = wall(lambda: spmv_acc_amd.amg_setup(m, rp, ci, v, theta=THETA, omega=OMEGA, coarse_rows=256))
    out["setup_ms"] = round(setup_ms, 1)
    out["sizes"] = h.sizes
    x = torch.zeros(m, dtype=torch.float64, device="cuda")
    spmv_acc_amd.pcg(m, rp, ci, v, b, x, precond=h, rtol=RTOL)  # (throw-away: the plans of the hierarchy and of A settle)

    def amg_pcg():
        x.zero_()
        return spmv_acc_amd.pcg(m, rp, ci, v, b, x, precond=h, rtol=RTOL)

    ms, samples, got = wall(amg_pcg, 3)
    out.update({"amg_pcg_ms": round(ms, 2), "amg_pcg_samples_ms": samples, "amg_pcg_iterations": got.iterations, "amg_pcg_status": got.status, "amg_pcg_residual": residual(x)})

    def stationary():
        x.zero_()
        for k in range(1, MAX_CYCLES + 1):
            spmv_acc_amd.amg_cycle(h, b, x)
            if k % 8 == 0 and residual(x) <= RTOL:
                return k
        return MAX_CYCLES

    ms, samples, cycles = wall(stationary, 3)
    out.update({"stationary_ms": round(ms, 2), "stationary_samples_ms": samples, "stationary_cycles": cycles, "stationary_residual": residual(x)})
    dinv = spmv_acc_amd.jacobi_inverse(m, rp, ci, v)

    def jacobi_pcg():
        x.zero_()
        return spmv_acc_amd.pcg(m, rp, ci, v, b, x, precond=dinv, rtol=RTOL, maxiter=MAX_JACOBI, check_every=64)

    ms, samples, got = wall(jacobi_pcg, 3)
    out.update({"jacobi_pcg_ms": round(ms, 2), "jacobi_pcg_samples_ms": samples, "jacobi_pcg_iterations": got.iterations, "jacobi_pcg_status": got.status, "jacobi_pcg_residual": residual(x)})
    if lib.spmv_acc_last_error() != 0:
        raise SystemExit(lib.spmv_acc_last_error_string().decode())
    h.release()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--parts", default="fem_quads,grid27")
    ap.add_argument("--md", default=None)
    ap.add_argument("--limit", type=int, default=400, help="seconds a part may take")
    ap.add_argument("--scale", type=float, default=1.0, help="rows relative to the documented size (a rehearsal at a small size)")
    ap.add_argument("--headline", default=None, help="JSON file with the headline ms_per_step of this build and of the parent build from the same run")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.scale)
        return
    rows = []
    for name in a.parts.split(","):  # (this process never opens the GPU: one child per part, each under its own limit)
        try:
            done = subprocess.run([sys.executable, os.path.abspath(__file__), a.out, "--child", name, "--scale", str(a.scale)], stdout=subprocess.PIPE,
                                  text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"{name}: no result within {a.limit} s; nothing more is started")
        if done.returncode != 0:
            raise SystemExit(f"{name}: the child ended with {done.returncode}; nothing more is started")
        rows += [json.loads(ln) for ln in done.stdout.splitlines() if ln.startswith("{")]
    headline = json.load(open(a.headline)) if a.headline else None
    with open(a.out, "w") as f:
        json.dump({"scale": a.scale, "rtol": RTOL, "theta": THETA, "omega": OMEGA, "parts": rows, "headline": headline}, f, indent=1)
    if a.md:
        with open(a.md, "w") as f:
            f.write("# Conjugate-gradient vector passes and AMG-PCG: tools/cg_bench.py\n\n")
            f.write("MI355X.  Times in ms (medians of 7 regions for the entries, medians of 3 solves for the solves; see the tool's docstring for each protocol).\n\n")
            f.write("MEASURED: every time, the iteration and cycle counts, the residuals.  REASONED, not measured: the byte counts behind the copies "
                    "(start 4 n doubles, update 8 n: 4 reads + 2 writes + 2 reads, direction 5 n, with dinv 7 n; the partials are not counted); that "
                    "an entry's distance from its copy is its launches (two, four and three against one) and the one-workgroup finishes between "
                    "the passes -- no trace was taken.\n\n")
            f.write("## One call of each entry at n = the matrix' rows\n\n")
            f.write("| n | entry | launches | ms | bytes moved | copy of those bytes | entry / copy |\n|" + "---|" * 7 + "\n")
            for r in rows:
                for label, launches in (("start", 2), ("update", 4), ("direction", 3), ("direction_jacobi", 3)):
                    f.write(f"| {r['m']} ({r['part']}) | {label} | {launches} | {r[label + '_ms']:.4f} | {r[label + '_bytes']} | {r[label + '_copy_ms']:.4f} | "
                            f"{r[label + '_over_copy']:.2f} |\n")
            f.write("\nCACHE-WARM figures: a timed region is about 1 ms of calls on four or five 32 MB vectors, which stay in the 256 MB Infinity Cache "
                    "between calls, as do the copy's buffers.  Inside a solve a matrix of 0.4 to 1 GB passes between two entries: the ratios compare "
                    "a pass with a copy under the same warm cache and say nothing about an entry's share of an iteration.\n")
            f.write(f"\n## Solves to rtol = {RTOL:g} (theta = {THETA}, omega = {OMEGA:.4f}, coarse_rows = 256, pre = post = 1; b standard normal, x0 = 0)\n\n")
            f.write("`residual` = the true |b - A x| / |b| at the end.  Status 1 = converged, 0 = the iteration cap was reached.\n\n")
            f.write("| matrix | rows | nnz | levels | AMG-PCG: iterations | ms | residual | stationary amg_cycle: cycles | ms | residual | Jacobi-PCG: iterations (status) | ms | residual |\n")
            f.write("|" + "---|" * 13 + "\n")
            for r in rows:
                f.write(f"| {r['part']} | {r['m']} | {r['nnz']} | {r['sizes']} | {r['amg_pcg_iterations']} | {r['amg_pcg_ms']:.1f} | {r['amg_pcg_residual']:.1e} | "
                        f"{r['stationary_cycles']} | {r['stationary_ms']:.1f} | {r['stationary_residual']:.1e} | {r['jacobi_pcg_iterations']} ({r['jacobi_pcg_status']}) | "
                        f"{r['jacobi_pcg_ms']:.1f} | {r['jacobi_pcg_residual']:.1e} |\n")
            f.write("\nAll three samples of each solve (ms): " + "; ".join(f"{r['part']}: AMG-PCG {r['amg_pcg_samples_ms']}, stationary {r['stationary_samples_ms']}, "
                                                                       f"Jacobi-PCG {r['jacobi_pcg_samples_ms']}" for r in rows) + ".\n")
            f.write(f"\nThe stationary loop reads its residual every 8 cycles and stops at {MAX_CYCLES}; Jacobi-PCG stops at {MAX_JACOBI} iterations.\n")
            if headline:
                f.write(f"\nHeadline (bench.py --gpus 1, the same run, the same box, alternating): this build {headline['this_ms_per_step']} ms per step, the parent "
                        f"build {headline['parent_ms_per_step']} ms per step.  No speed gate: the parent cannot do this job; the hot SpMV path is untouched.\n")


if __name__ == "__main__":
    main()
