#!/usr/bin/env python3
"""The one-launch Jacobi / l1-Jacobi smoother (spmv_acc_csr_jacobi_diagonal, spmv_acc_csr_jacobi_sweep) and the AMG cycle on it, on
tools/cg_bench.py's two matrices (`fem_quads`, 4.0 M rows, 9-point; `grid27`, 3.4 M rows, 27-point; anisotropic values, Dirichlet ends,
theta = 0.05, omega = 2/3 for the prolongator, coarse_rows = 256).  One JSON line per matrix:
  spmv_ms            the engine's settled SpMV on the matrix (spmv_acc_time_spmv_region, 10 calls per region, median of 7), beta = 1: the
                     yardstick, as in tools/gs_bench.py
  sweep_ms, residual_ms, zero_ms
                     one csr_jacobi_sweep in the x_out-only, the r_out-only and the zero-start form: median of 7 regions of 10 calls between
                     one event pair, after a warm-up.  The sweep ping-pongs between two vectors
  composed_*_ms      the alternative composed from the engine: sweep = csr_spmv(-1, 1, ..., y_in = b) into r, then torch.addcmul(x, w, r)
                     into the other vector (w = omega dinv, made once); residual = that csr_spmv alone; zero = torch.mul(w, b).  The same
                     protocol, after 40 calls in which the SpMV's plan settles.  composed_agrees_rel: the largest difference of the two sweeps'
                     results over the result's largest magnitude (they differ in the order of a row's terms)
  diagonal_*_ms      spmv_acc_csr_jacobi_diagonal, kinds "jacobi" and "l1": the C entry on preallocated dinv and work (no allocation in the
                     timed region), median of 7 regions of 5 calls, and in SpMVs
  grid_*             the sweep and the residual form with the launch grid lowered through the tunable max_grid_blocks (the kernels stride over
                     the chunks beyond the grid; the bits do not change): ms per cap, the same protocol; cap 0 = the default grid, one
                     workgroup per chunk of 64 rows
  per smoother ("gs", "jacobi", "l1_jacobi"):
    setup_ms         amg_setup: the fastest of 3 calls, host clock between device synchronisations (tools/amg_bench.py: the samples are bimodal)
    cycle_ms         one amg_cycle (pre = post = 1): median of 7 regions of 5 cycles, after 10 cycles in which the plans settle; and in SpMVs
    pcg11_*, pcg22_* pcg with the hierarchy to rtol = 1e-8 at pre = post = 1 and 2, b standard normal from seed 5, x0 = 0: iterations, status,
                     the median of 3 solves' host-clock ms after one throw-away solve, the true relative residual |b - A x| / |b|
Every matrix runs in a child process of its own under a time limit; after a child that fails or runs out of time nothing more is started.
usage: tools/jacobi_bench.py OUT.json [--parts fem_quads,grid27] [--md OUT.md] [--limit SECONDS] [--scale 1.0] [--headline FILE]"""
import argparse
import json
import os
import subprocess
import sys
import time

THETA = 0.05
OMEGA = 2.0 / 3.0
RTOL = 1e-8
SMOOTHERS = ("gs", "jacobi", "l1_jacobi")
GRID_CAPS = (0, 16384, 4096, 2048, 512)  # max_grid_blocks; 0: the default


def child(name, scale):
    import numpy as np
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import spmv_acc_amd

    def stencil(shape, weak_of, weak):
        """tools/cg_bench.py's matrices: the full 3^d stencil on a grid of `shape` points with anisotropic values and Dirichlet ends, rows
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

    def median_region(fn, reps=10, regions=7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        out = []
        for _ in range(regions):
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) / reps)
        return float(np.median(out))

    def wall(fn, calls=1):
        """(every host-clock time in ms, the last call's result)"""
        ts = []
        for _ in range(calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return [round(t, 2) for t in ts], got

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
    lib.spmv_acc_set_stream(torch.cuda.current_stream().cuda_stream)
    out = {"part": name, "m": m, "nnz": nnz}

    def check():
        if lib.spmv_acc_last_error() != 0:
            raise SystemExit(lib.spmv_acc_last_error_string().decode())

    # ---- the yardstick first, on the untouched SpMV path (tools/gs_bench.py's protocol) -------------------------------------------------------
    gen = torch.Generator(device="cuda").manual_seed(7)
    rand = lambda: torch.randn(m, dtype=torch.float64, device="cuda", generator=gen)  # noqa: E731
    x, y = rand(), rand()
    spmv_acc_amd.prepare(m, m, nnz, rp, ci, v, x, beta=1.0)
    region = spmv_acc_amd.time_spmv_region(spmv_acc_amd.get_strategy(), 10, 1.0, 1.0, m, m, nnz, rp, ci, v, x, y)
    spmv_ms = float(np.median([region() for _ in range(7)])) / 10
    spmv_acc_amd.release_plans(rp)
    del y
    out["spmv_ms"] = round(spmv_ms, 5)

    # ---- the entries alone, beside the composed alternative -----------------------------------------------------------------------------------
    omega = 0.9
    b, xa, xb, r = rand(), x.clone(), torch.empty_like(x), torch.empty_like(x)
    d_out, d_work = torch.empty_like(x), torch.empty_like(x)
    for code, kind in enumerate(("jacobi", "l1")):

        def fn(code=code):
            if lib.spmv_acc_csr_jacobi_diagonal(m, nnz, rp.data_ptr(), ci.data_ptr(), v.data_ptr(), code, d_out.data_ptr(), d_work.data_ptr()) != 0:
                raise SystemExit(lib.spmv_acc_last_error_string().decode())

        fn()
        ms = median_region(fn, reps=5)
        out[f"diagonal_{kind}_ms"] = round(ms, 5)
        out[f"diagonal_{kind}_spmvs"] = round(ms / spmv_ms, 2)
    dinv = spmv_acc_amd.csr_jacobi_diagonal(m, rp, ci, v, kind="l1")
    w = omega * dinv
    pair = [xa, xb]

    def sweep():
        spmv_acc_amd.csr_jacobi_sweep(m, rp, ci, v, dinv, b, pair[0], x_out=pair[1], omega=omega)
        pair.reverse()

    def composed_sweep():
        spmv_acc_amd.csr_spmv(-1.0, 1.0, m, m, nnz, rp, ci, v, pair[0], r, y_in=b)
        torch.addcmul(pair[0], w, r, out=pair[1])
        pair.reverse()

    forms = (("sweep", sweep, composed_sweep),
             ("residual", lambda: spmv_acc_amd.csr_jacobi_sweep(m, rp, ci, v, dinv, b, xa, r_out=r, omega=omega),
              lambda: spmv_acc_amd.csr_spmv(-1.0, 1.0, m, m, nnz, rp, ci, v, xa, r, y_in=b)),
             ("zero", lambda: spmv_acc_amd.csr_jacobi_sweep(m, rp, ci, v, dinv, b, None, x_out=xb, omega=omega), lambda: torch.mul(w, b, out=xb)))
    # the two sweeps compute the same update up to the order of a row's terms
    xa.copy_(x)
    spmv_acc_amd.csr_jacobi_sweep(m, rp, ci, v, dinv, b, xa, x_out=xb, omega=omega)
    fused = xb.clone()
    spmv_acc_amd.csr_spmv(-1.0, 1.0, m, m, nnz, rp, ci, v, xa, r, y_in=b)
    torch.addcmul(xa, w, r, out=xb)
    out["composed_agrees_rel"] = float(((fused - xb).abs().max() / fused.abs().max()).item())
    del fused
    for label, fn, composed in forms:
        for tag, f in ((label + "_ms", fn), ("composed_" + label + "_ms", composed)):
            pair[:] = [xa, xb]
            xa.copy_(x)
            for _ in range(40):  # (the composed SpMV's plan settles; the entries have nothing to settle)
                f()
            pair[:] = [xa, xb]
            xa.copy_(x)
            out[tag] = round(median_region(f), 5)
        out[label + "_spmvs"] = round(out[label + "_ms"] / spmv_ms, 2)
        out["composed_" + label + "_spmvs"] = round(out["composed_" + label + "_ms"] / spmv_ms, 2)
        check()
    # the launch grid: fewer, longer-lived workgroups through the tunable the stride tests use
    xa.copy_(x)
    grid = {}
    for cap in GRID_CAPS:
        if cap and lib.spmv_acc_set_tunable(b"max_grid_blocks", cap) != 0:
            raise SystemExit("max_grid_blocks was refused")
        row = {}
        for label, fn in (("sweep", lambda: spmv_acc_amd.csr_jacobi_sweep(m, rp, ci, v, dinv, b, xa, x_out=xb, omega=omega)),
                          ("residual", lambda: spmv_acc_amd.csr_jacobi_sweep(m, rp, ci, v, dinv, b, xa, r_out=r, omega=omega))):
            for _ in range(5):
                fn()
            row[label + "_ms"] = round(median_region(fn), 5)
        lib.spmv_acc_reset_tunables()
        row["workgroups"] = min((m + 63) // 64, cap) if cap else (m + 63) // 64
        grid[str(cap)] = row
    out["grid"] = grid
    check()
    spmv_acc_amd.release_plans(rp)
    del xa, xb, r, w, dinv, pair, x, d_out, d_work
    torch.cuda.empty_cache()

    # ---- the hierarchies: setup, one cycle, AMG-PCG -----------------------------------------------------------------------------------------------
    b = torch.randn(m, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    bnorm = float(b.norm().item())
    res = torch.empty_like(b)
    x = torch.zeros(m, dtype=torch.float64, device="cuda")

    def residual(x):
        spmv_acc_amd.csr_spmv(-1.0, 1.0, m, m, nnz, rp, ci, v, x, res, y_in=b)
        return float(res.norm().item()) / bnorm

    for smoother in SMOOTHERS:
        samples, h = wall(lambda: spmv_acc_amd.amg_setup(m, rp, ci, v, theta=THETA, omega=OMEGA, coarse_rows=256, smoother=smoother), 3)
        row = {"setup_ms": min(samples), "setup_samples_ms": samples, "setup_spmvs": round(min(samples) / spmv_ms, 1), "sizes": h.sizes,
               "smoother_omega": h.smoother_omega}
        x.zero_()
        for _ in range(10):
            spmv_acc_amd.amg_cycle(h, b, x)
        x.zero_()
        row["cycle_ms"] = round(median_region(lambda: spmv_acc_amd.amg_cycle(h, b, x), reps=5), 4)
        row["cycle_spmvs"] = round(row["cycle_ms"] / spmv_ms, 1)
        for sweeps in (1, 2):

            def solve():
                x.zero_()
                return spmv_acc_amd.pcg(m, rp, ci, v, b, x, precond=h, rtol=RTOL, pre=sweeps, post=sweeps)

            solve()  # (throw-away: the plans settle)
            samples, got = wall(solve, 3)
            row.update({f"pcg{sweeps}{sweeps}_ms": round(float(np.median(samples)), 2), f"pcg{sweeps}{sweeps}_samples_ms": samples,
                        f"pcg{sweeps}{sweeps}_iterations": got.iterations, f"pcg{sweeps}{sweeps}_status": got.status,
                        f"pcg{sweeps}{sweeps}_residual": residual(x)})
        check()
        h.release()
        spmv_acc_amd.release_plans(rp)
        del h
        torch.cuda.empty_cache()
        out[smoother] = row
    print(json.dumps(out), flush=True)


def write_md(path, rows, headline):
    with open(path, "w") as f:
        f.write("# One-launch Jacobi / l1-Jacobi smoother and the AMG cycle on it: tools/jacobi_bench.py\n\n")
        f.write("MI355X.  Times in ms (medians of 7 regions for the entries and the cycle, the fastest of 3 calls for the setup, medians of 3 solves "
                "for the solves; see the tool's docstring for each protocol).\n\n")
        f.write("MEASURED: every time, the iteration counts, the residuals, the agreement of the fused and the composed sweep.  REASONED, not "
                "measured: that a sweep moves the bytes of one SpMV plus dinv and one more vector (12 B per non-zero, rowptr, b, x_in, dinv, x_out); "
                "that the composed sweep's distance from the fused one is its second launch and the 5 vectors of its torch pass -- no trace was "
                "taken, no counters were collected.\n\n")
        f.write("## One call of each form, beside a settled SpMV of the engine and beside the composed alternative\n\n")
        f.write("`composed` = csr_spmv(-1, 1, ..., y_in = b) plus one torch pass (sweep), that csr_spmv alone (residual), one torch pass (zero start).  "
                "`in SpMVs` = over the settled SpMV (beta = 1) of the same matrix in the same process.\n\n")
        f.write("| matrix | rows | nnz | SpMV | form | fused | in SpMVs | composed | in SpMVs | fused / composed |\n|" + "---|" * 10 + "\n")
        for r in rows:
            for label in ("sweep", "residual", "zero"):
                f.write(f"| {r['part']} | {r['m']} | {r['nnz']} | {r['spmv_ms']:.4f} | {label} | {r[label + '_ms']:.4f} | {r[label + '_spmvs']:.2f} | "
                        f"{r['composed_' + label + '_ms']:.4f} | {r['composed_' + label + '_spmvs']:.2f} | {r[label + '_ms'] / r['composed_' + label + '_ms']:.2f} |\n")
        f.write("\nThe fused and the composed sweep agree to " + ", ".join(f"{r['composed_agrees_rel']:.1e} ({r['part']})" for r in rows) +
                " of the result's largest magnitude: the order of a row's terms.\n\n")
        for r in rows:
            verdict = {label: r[label + "_ms"] < r["composed_" + label + "_ms"] for label in ("sweep", "residual", "zero")}
            f.write(f"{r['part']}: the fused sweep " + ("BEATS" if verdict["sweep"] else "LOSES TO") + " the composed one; the residual-only form " +
                    ("beats" if verdict["residual"] else "loses to") + " the engine's SpMV with y_in; the zero start " +
                    ("beats" if verdict["zero"] else "loses to") + " one torch pass.\n\n")
        f.write("## The launch grid of the sweep\n\nThe same sweep and residual form with the grid lowered through the tunable max_grid_blocks, so that "
                "fewer workgroups each stride over more chunks of 64 rows (the bits do not change).  `against the default` = the time over the default "
                "grid's: above 1 is SLOWER.\n\n")
        f.write("| matrix | max_grid_blocks | workgroups | sweep | against the default | residual | against the default |\n|" + "---|" * 7 + "\n")
        for r in rows:
            base = r["grid"]["0"]
            for cap, g in r["grid"].items():
                f.write(f"| {r['part']} | {'default' if cap == '0' else cap} | {g['workgroups']} | {g['sweep_ms']:.4f} | {g['sweep_ms'] / base['sweep_ms']:.2f} | "
                        f"{g['residual_ms']:.4f} | {g['residual_ms'] / base['residual_ms']:.2f} |\n")
        best = {r["part"]: min(r["grid"].values(), key=lambda g: g["sweep_ms"])["sweep_ms"] / r["grid"]["0"]["sweep_ms"] for r in rows}
        f.write("\nThe best capped grid runs the sweep in " + ", ".join(f"{v:.2f} ({k})" for k, v in best.items()) +
                " of the default grid's time: the launchers keep one workgroup per chunk up to max_grid_blocks().\n\n")
        f.write("## spmv_acc_csr_jacobi_diagonal (the C entry on preallocated arrays)\n\n| matrix | kind | ms | in SpMVs |\n|---|---|---|---|\n")
        for r in rows:
            for kind in ("jacobi", "l1"):
                f.write(f"| {r['part']} | {kind} | {r['diagonal_' + kind + '_ms']:.4f} | {r['diagonal_' + kind + '_spmvs']:.2f} |\n")
        f.write(f"\n## amg_setup and one amg_cycle for the three smoothers (theta = {THETA}, omega = {OMEGA:.4f}, coarse_rows = 256, pre = post = 1)\n\n")
        f.write("| matrix | smoother (omega) | levels | setup | in SpMVs | cycle | in SpMVs |\n|" + "---|" * 7 + "\n")
        for r in rows:
            for s in SMOOTHERS:
                t = r[s]
                f.write(f"| {r['part']} | {s} ({t['smoother_omega']:.4g}) | {t['sizes']} | {t['setup_ms']:.1f} | {t['setup_spmvs']:.0f} | {t['cycle_ms']:.3f} | "
                        f"{t['cycle_spmvs']:.1f} |\n")
        f.write("\nAll three setup samples (ms; bimodal, as profiles/amg_bench.md describes): " +
                "; ".join(f"{r['part']} / {s}: {r[s]['setup_samples_ms']}" for r in rows for s in SMOOTHERS) + ".\n")
        f.write(f"\n## AMG-PCG to rtol = {RTOL:g} (b standard normal, x0 = 0)\n\n`residual` = the true |b - A x| / |b| at the end.  Status 1 = converged.\n\n")
        f.write("| matrix | smoother | pre = post | iterations (status) | ms | residual |\n|" + "---|" * 6 + "\n")
        for r in rows:
            for s in SMOOTHERS:
                for k in ("11", "22"):
                    t = r[s]
                    f.write(f"| {r['part']} | {s} | {k[0]} | {t['pcg' + k + '_iterations']} ({t['pcg' + k + '_status']}) | {t['pcg' + k + '_ms']:.1f} | "
                            f"{t['pcg' + k + '_residual']:.1e} |\n")
        f.write("\nAll three samples of each solve (ms): " +
                "; ".join(f"{r['part']} / {s} / {k[0]}: {r[s]['pcg' + k + '_samples_ms']}" for r in rows for s in SMOOTHERS for k in ("11", "22")) + ".\n\n")
        for r in rows:
            solves = {(s, k): r[s]["pcg" + k + "_ms"] for s in SMOOTHERS for k in ("11", "22") if r[s]["pcg" + k + "_status"] == 1}
            best = min(solves, key=solves.get) if solves else None
            for k in ("11", "22"):
                at = {s: t for (s, kk), t in solves.items() if kk == k}
                if at:
                    win = min(at, key=at.get)
                    f.write(f"{r['part']}, pre = post = {k[0]}: {win} wins ({at[win]:.1f} ms; " + ", ".join(f"{s} {t:.1f}" for s, t in at.items() if s != win) + ").  ")
            if best:
                f.write(f"The fastest solve of all six: {best[0]} at pre = post = {best[1][0]}, {solves[best]:.1f} ms.\n\n")
        f.write("## What won\n\n")
        for r in rows:
            g, l = r["gs"], r["l1_jacobi"]
            best = min(SMOOTHERS, key=lambda s: r[s]["pcg11_ms"])
            f.write(f"{r['part']}: one cycle on l1_jacobi costs {l['cycle_spmvs']:.1f} SpMVs against {g['cycle_spmvs']:.1f} on Gauss-Seidel "
                    f"({g['cycle_ms'] / l['cycle_ms']:.1f} x less); AMG-PCG at pre = post = 1 needs {l['pcg11_iterations']} iterations against "
                    f"{g['pcg11_iterations']} ({l['pcg11_iterations'] / g['pcg11_iterations']:.1f} x more) and {l['pcg11_ms']:.1f} ms against {g['pcg11_ms']:.1f} "
                    f"({g['pcg11_ms'] / l['pcg11_ms']:.1f} x less); the fastest smoother there is {best} ({r[best]['pcg11_ms']:.1f} ms).  The setup without the "
                    f"colouring is {g['setup_ms'] - l['setup_ms']:.1f} ms shorter ({g['setup_ms']:.1f} against {l['setup_ms']:.1f}).  The fused sweep itself, "
                    f"{r['sweep_spmvs']:.2f} SpMVs, " + ("beats" if r["sweep_ms"] < r["composed_sweep_ms"] else "LOSES TO") +
                    f" csr_spmv plus a torch pass, {r['composed_sweep_spmvs']:.2f} SpMVs" +
                    ("" if r["sweep_ms"] < r["composed_sweep_ms"] else ": what it buys is the contract -- no plan, no per-matrix timing, one documented summation "
                     "order, the same bits from the first call on --, not speed; the cycle's gain is supposed to come from the launches and the row "
                     "indirection it no longer has (no trace was taken), not from this kernel") + ".\n\n")
        f.write("The default smoother stays \"gs\": changing it is not part of this work, whatever wins above.\n")
        if headline:
            f.write(f"\nHeadline (bench.py --gpus 1, the same run, the same box, alternating): this build {headline['this_ms_per_step']} ms per step, the parent "
                    f"build {headline['parent_ms_per_step']} ms per step.  No speed gate: the parent cannot do this job; the hot SpMV path is untouched.\n")


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
        write_md(a.md, rows, headline)


if __name__ == "__main__":
    main()
