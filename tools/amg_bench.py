#!/usr/bin/env python3
"""The dense coarse-level solve (spmv_acc_csr_dense_inverse, spmv_acc_dense_apply) and the AMG hierarchy and V-cycle composed on it
(spmv_acc_amd.amg: amg_setup, amg_cycle).  One JSON line per measurement:
  dense, m = 64, 256, 1024 (the five-point Laplacian on 8 x 8, 16 x 16 and 32 x 32 points):
    inverse_ms       csr_dense_inverse: median of 3 calls after one warm-up, host clock between device synchronisations (the entry synchronises)
    apply_*_ms       dense_apply: median of 7 regions of 20 calls between one event pair, plain on the stream and replayed from a graph
    apply_copy_ms    torch's device copy of as many bytes as the apply must move at least (8 m^2 + 24 m, half read and half written), same protocol
    valid            max |A inv - I| (formed with torch)
  amg, on tools/strength_bench.py's two matrices with its anisotropic values (`fem_quads`, 4.0 M rows, 9-point; `grid27`, 3.4 M rows,
  27-point) -- with ONE change: the diagonal also counts the couplings that leave the grid (Dirichlet ends); with the row's own absolute sum
  alone every row sums to zero and the matrix is singular --, theta = 0.05, omega = 2/3, coarse_rows in (64, 256, 1024):
    setup_ms         amg_setup: the FASTEST of 5 calls after one warm-up, host clock (every entry of the setup synchronises); the hierarchy is
                     released after each.  setup_samples_ms holds all five.  The samples are bimodal: a call takes either the fastest call's time within 2 %
                     or 0.3 to 5.4 s, and from one in ten to all five calls, differently from run to run, are slow.  The setup allocates and frees GiBs of workspaces and
                     results call by call (hipMalloc / hipFree in the analysis entries, torch's allocator for the results); that the slow
                     calls are slow there is supposed, not shown: eight setups of a 7-point grid of the same rows, timed entry by entry, had
                     no slow call among them.  The fastest call is the cost of the work; the slow ones are reported, not explained
    cycle_ms         one amg_cycle (pre = post = 1, symmetric sweeps): median of 5 regions of 5 cycles between one event pair, after the ten
                     cycles of `reduction`, in which the SpMV plans of the hierarchy settle
    spmv_ms          the engine's settled SpMV on the fine matrix (spmv_acc_time_spmv_region, 10 calls per region, median of 7), beta = 1;
                     *_spmvs = the time over it
    sizes, rule      the rows of every level and the rule that ended the hierarchy
    reduction        |b - A x| / |b| after 10 cycles from x = 0, b standard normal
Every child process measures one matrix (or the dense part) under a time limit; after a child that fails or runs out of time nothing more is
started.
usage: tools/amg_bench.py OUT.json [--parts dense,fem_quads,grid27] [--md OUT.md] [--limit SECONDS] [--scale 1.0]"""
import argparse
import json
import os
import subprocess
import sys
import time

THETA = 0.05
OMEGA = 2.0 / 3.0
COARSE_ROWS = (64, 256, 1024)
DENSE_ROWS = (64, 256, 1024)


def child(name, scale):
    import numpy as np
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import spmv_acc_amd

    def median_region(fn, reps=20, regions=7):
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

    def median_host(fn, calls=3):
        fn()
        ts = []
        for _ in range(calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    def stencil(shape, weak_of, weak, seeded=True):
        """tools/strength_bench.py's matrices: the full 3^d stencil on a grid of `shape` points with anisotropic values, rows strictly ascending;
        weak_of(offset) names the couplings that get `weak` instead of 1 (None: the coupling is not stored)"""
        m = int(np.prod(shape))
        coords = torch.unravel_index(torch.arange(m, device="cuda"), shape)
        cols, valid, size = [], [], []
        for off in np.ndindex(*([3] * len(shape))):
            rel = tuple(o - 1 for o in off)
            centre = all(o == 0 for o in rel)
            w = False if centre else weak_of(rel)
            if w is None:
                continue
            ok = torch.ones(m, dtype=torch.bool, device="cuda")
            col = torch.zeros(m, dtype=torch.int64, device="cuda")
            for c, o, s in zip(coords, rel, shape):
                q = c + o
                ok &= (q >= 0) & (q < s)
                col = col * s + q
            cols.append(col)
            valid.append(ok)
            size.append(0.0 if centre else (weak if w else 1.0))
        cols, valid = torch.stack(cols, 1), torch.stack(valid, 1)  # (offsets ascend in the flattened column: every row ascends)
        lens = valid.sum(1)
        rp = torch.zeros(m + 1, dtype=torch.int32, device="cuda")
        rp[1:] = torch.cumsum(lens, 0).int()
        ci = cols[valid].int()
        row = torch.repeat_interleave(torch.arange(m, device="cuda"), lens)
        gen = torch.Generator(device="cuda").manual_seed(2033)
        base = torch.tensor(size, dtype=torch.float64, device="cuda").expand(m, -1)[valid]
        factor = 0.9 + 0.2 * torch.rand(ci.numel(), dtype=torch.float64, device="cuda", generator=gen) if seeded else 1.0
        v = -base * factor
        # the diagonal: the row's absolute sum PLUS the couplings that leave the grid (Dirichlet ends).  With the row's own absolute sum alone, as
        # in tools/strength_bench.py, every row sums to zero: the matrix is singular and the coarsest solve of a V-cycle is not defined
        outside = ((~valid).double() * torch.tensor(size, dtype=torch.float64, device="cuda")).sum(1)
        diag = torch.zeros(m, dtype=torch.float64, device="cuda").index_add_(0, row, v.abs()) + outside
        v = torch.where(ci.long() == row, diag[row], v)
        return m, rp, ci.contiguous(), v.contiguous()

    lib = spmv_acc_amd.load_library()
    lib.spmv_acc_set_stream(torch.cuda.current_stream().cuda_stream)

    if name == "dense":
        for rows in DENSE_ROWS:
            side = int(round(rows ** 0.5))
            # the five-point Laplacian with Dirichlet ends: the diagonal 4, not the row's absolute sum
            m, rp, ci, v = stencil((side, side), lambda off: None if all(o != 0 for o in off) else False, 1.0, seeded=False)
            row = torch.repeat_interleave(torch.arange(m, device="cuda"), (rp[1:] - rp[:-1]).long())
            v = torch.where(ci.long() == row, torch.full_like(v, 4.0), v)
            inverse_ms = median_host(lambda: spmv_acc_amd.csr_dense_inverse(m, rp, ci, v))
            inv, info = spmv_acc_amd.csr_dense_inverse(m, rp, ci, v)
            A = torch.zeros((m, m), dtype=torch.float64, device="cuda")
            A[row, ci.long()] = v
            valid = float((A @ inv - torch.eye(m, dtype=torch.float64, device="cuda")).abs().max().item())
            b = torch.randn(m, dtype=torch.float64, device="cuda")
            x = torch.empty_like(b)
            apply = lambda: spmv_acc_amd.dense_apply(m, inv, b, x)
            apply()
            plain = median_region(apply)
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            g = torch.cuda.CUDAGraph()
            with torch.cuda.stream(s):
                torch.cuda.synchronize()
                with torch.cuda.graph(g, stream=s):
                    apply()
            g.replay()
            graph = median_region(g.replay)
            del g
            nbytes = 8 * m * m + 24 * m
            c_src = torch.randn(nbytes // 16, dtype=torch.float64, device="cuda")
            c_dst = torch.empty_like(c_src)
            copy_ms = median_region(lambda: c_dst.copy_(c_src))
            if lib.spmv_acc_last_error() != 0:
                raise SystemExit(lib.spmv_acc_last_error_string().decode())
            print(json.dumps({"part": "dense", "m": m, "nnz": int(ci.numel()), "info": info, "inverse_ms": round(inverse_ms, 3),
                              "inverse_us_per_step": round(1e3 * inverse_ms / m, 2), "apply_plain_ms": round(plain, 5), "apply_graph_ms": round(graph, 5),
                              "apply_bytes": nbytes, "apply_copy_ms": round(copy_ms, 5), "apply_over_copy": round(graph / copy_ms, 2), "valid": valid}),
                  flush=True)
        return

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

    # the yardstick first: the settled SpMV
    x = torch.randn(m, dtype=torch.float64, device="cuda")
    y = torch.randn(m, dtype=torch.float64, device="cuda")
    spmv_acc_amd.prepare(m, m, nnz, rp, ci, v, x, beta=1.0)
    region = spmv_acc_amd.time_spmv_region(spmv_acc_amd.get_strategy(), 10, 1.0, 1.0, m, m, nnz, rp, ci, v, x, y)
    spmv_ms = float(np.median([region() for _ in range(7)])) / 10
    spmv_acc_amd.release_plans(rp)
    del x, y

    b = torch.randn(m, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    for coarse_rows in COARSE_ROWS:
        def setup():
            return spmv_acc_amd.amg_setup(m, rp, ci, v, theta=THETA, omega=OMEGA, coarse_rows=coarse_rows)

        try:
            setup().release()  # (warm-up)
            samples = []
            for _ in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                made = setup()
                torch.cuda.synchronize()
                samples.append((time.perf_counter() - t0) * 1e3)
                made.release()
                del made
            setup_ms = float(np.min(samples))
            h = setup()
        except spmv_acc_amd.SpmvAccError as e:  # (a hierarchy that ends above the dense cap is a result, not a failure of the tool)
            print(json.dumps({"part": name, "m": m, "nnz": nnz, "coarse_rows": coarse_rows, "error": str(e)}), flush=True)
            continue
        x = torch.zeros(m, dtype=torch.float64, device="cuda")
        r = torch.empty_like(x)
        for _ in range(10):
            spmv_acc_amd.amg_cycle(h, b, x)
        spmv_acc_amd.csr_spmv(-1.0, 1.0, m, m, nnz, rp, ci, v, x, r, y_in=b)
        reduction = float((r.norm() / b.norm()).item())
        cycle_ms = median_region(lambda: spmv_acc_amd.amg_cycle(h, b, x), reps=5, regions=5)
        if lib.spmv_acc_last_error() != 0:
            raise SystemExit(lib.spmv_acc_last_error_string().decode())
        nnz_levels = [int(lv.A[1].numel()) for lv in h.levels] + [int(h.coarsest.A[1].numel())]
        print(json.dumps({"part": name, "m": m, "nnz": nnz, "theta": THETA, "omega": OMEGA, "coarse_rows": coarse_rows, "sizes": h.sizes,
                          "nnz_levels": nnz_levels, "operator_complexity": round(sum(nnz_levels) / nnz, 3), "rule": h.coarsest.rule,
                          "setup_ms": round(setup_ms, 2), "setup_samples_ms": [round(t, 1) for t in samples], "cycle_ms": round(cycle_ms, 4), "spmv_ms": round(spmv_ms, 5),
                          "setup_spmvs": round(setup_ms / spmv_ms, 0), "cycle_spmvs": round(cycle_ms / spmv_ms, 1), "reduction": reduction}), flush=True)
        h.release()
        del h, x, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--parts", default="dense,fem_quads,grid27")
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
    dense = [r for r in rows if r["part"] == "dense"]
    amg = [r for r in rows if r["part"] != "dense"]
    # the default coarse_rows: 256 unless another of the three is faster per cycle by more than 10 % on BOTH matrices
    verdict = "coarse_rows = 256 stays the default"
    by = {(r["part"], r["coarse_rows"]): r["cycle_ms"] for r in amg if "cycle_ms" in r}
    parts = sorted({r["part"] for r in amg})
    for other in (c for c in COARSE_ROWS if c != 256):
        if parts and all((p, other) in by and (p, 256) in by and by[(p, other)] < by[(p, 256)] / 1.1 for p in parts):
            verdict = f"coarse_rows = {other} is faster per cycle than 256 by more than 10 % on every matrix"
    doc = {"scale": a.scale, "dense": dense, "amg": amg, "default": verdict, "headline": headline}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    if a.md:
        with open(a.md, "w") as f:
            f.write("# Dense coarse-level solve, AMG setup and V-cycle: tools/amg_bench.py\n\n")
            f.write("MI355X.  Times in ms (medians; see the tool's docstring for each protocol).\n\n")
            f.write("MEASURED: every time, the level sizes, the reductions and max |A inv - I|.  REASONED, not measured: the byte count behind the "
                    "apply's copy (8 m^2 + 24 m: inv and b read, x written); that the inverse below a few hundred rows is bound by its 3 m "
                    "launches (its time per step is flat in m there; no counters were collected).\n\n")
            f.write("## csr_dense_inverse and dense_apply (five-point Laplacian)\n\n")
            f.write("| m | nnz | inverse | per step (us) | apply plain | apply graph | copy of its bytes | apply / copy | max abs(A inv - I) |\n")
            f.write("|" + "---|" * 9 + "\n")
            for r in dense:
                f.write(f"| {r['m']} | {r['nnz']} | {r['inverse_ms']:.2f} | {r['inverse_us_per_step']:.1f} | {r['apply_plain_ms']:.4f} | "
                        f"{r['apply_graph_ms']:.4f} | {r['apply_copy_ms']:.4f} | {r['apply_over_copy']:.2f} | {r['valid']:.1e} |\n")
            f.write(f"\n## amg_setup and one amg_cycle (theta = {THETA}, omega = {OMEGA:.4f}, pre = post = 1, symmetric sweeps)\n\n")
            f.write("`in SpMVs` = over one settled SpMV of the engine on the fine matrix; `complexity` = the non-zeros of all levels over the fine "
                    "matrix'; `reduction` = the relative residual after 10 cycles.\n\n")
            f.write("| matrix | rows | nnz | coarse_rows | levels | ended by | complexity | setup | in SpMVs | cycle | in SpMVs | SpMV | reduction |\n")
            f.write("|" + "---|" * 13 + "\n")
            for r in amg:
                if "error" in r:
                    f.write(f"| {r['part']} | {r['m']} | {r['nnz']} | {r['coarse_rows']} | refused: {r['error']} |" + " |" * 8 + "\n")
                    continue
                f.write(f"| {r['part']} | {r['m']} | {r['nnz']} | {r['coarse_rows']} | {r['sizes']} | {r['rule']} | {r['operator_complexity']:.2f} | "
                        f"{r['setup_ms']:.1f} | {r['setup_spmvs']:.0f} | {r['cycle_ms']:.3f} | {r['cycle_spmvs']:.1f} | {r['spmv_ms']:.4f} | "
                        f"{r['reduction']:.1e} |\n")
            f.write("\n`setup` is the fastest of five calls.  All five (ms): " + "; ".join(f"{r['part']} / {r['coarse_rows']}: {r['setup_samples_ms']}" for r in amg if "setup_samples_ms" in r)
                    + ".  The samples are bimodal: a call takes either the time in the table, within 2 %, or seconds.  The setup allocates and "
                      "frees GiBs call by call, and the slow calls are supposed to be slow there; that is not shown (the tool's docstring).\n")
            f.write(f"\nThe default: {verdict}.\n")
            if headline:
                f.write(f"\nHeadline (bench.py --gpus 1, the same run, the same box): this build {headline['this_ms_per_step']:.5f} ms per step, the parent "
                        f"build {headline['parent_ms_per_step']:.5f} ms per step.  No speed gate: the parent cannot do this job.\n")


if __name__ == "__main__":
    main()
