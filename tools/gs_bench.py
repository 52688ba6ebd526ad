#!/usr/bin/env python3
"""The multicolour Gauss-Seidel smoother (spmv_acc_csr_color, spmv_acc_csr_gs_sweep) on two mesh matrices of a few million rows, made on the
device: `fem_quads`, the 9-point pattern of a bilinear-quad assembly on a 2000 x 2000 element grid (4.0 M rows), and `grid27`, the 27-point
stencil on 150^3 points (3.4 M rows); off-diagonals -1, the diagonal the row's entry count (symmetric, weakly dominant).  One JSON line each:
  color_ms         spmv_acc_csr_color: median of 3 calls after one warm-up, host clock between device synchronisations (the entry synchronises)
  colors, rounds   the colours it returned; the Jones-Plassmann rounds the pattern needs = the longest chain of rows of descending priority,
                   1 + max over the higher-priority neighbours, iterated with torch to its fixed point (the entry enqueues rounds in groups of 8)
  proper           no stored off-diagonal (i, j) has color[i] == color[j] (checked with torch)
  sweep_*_ms       ONE symmetric sweep (omega = 1: 2 x colours launches), median of 7 regions of 5 sweeps between one event pair, after a warm-up:
                   plain   csr_gs_sweep's launches on the stream,          graph   the sweep captured once and replayed,
                   rows    through color_rows on the original matrix,      perm    on the colour-permuted matrix (color_rows = NULL)
  spmv_ms          the engine's settled SpMV on the original matrix (spmv_acc_time_spmv_region, 10 calls per region, median of 7), beta = 1:
                   the yardstick -- a sweep moves one SpMV's bytes per direction, so a symmetric sweep is held against 2 SpMVs
  floor_*_us       the time per launch of the same entry on a path of 3 000 rows (3 colours, 6 launches of a dozen workgroups): what a launch
                   costs when it has nothing to move, plain and replayed
  copy_ceiling_gbs spmv_acc_copy_ceiling_gbs on this box in this run (1 GiB)
Every matrix runs in a child process of its own under a time limit; after a child that fails or runs out of time nothing more is started.
usage: tools/gs_bench.py OUT.json [--matrices fem_quads,grid27] [--md OUT.md] [--limit SECONDS] [--scale 1.0]"""
import argparse
import json
import os
import subprocess
import sys
import time


def child(name, scale):
    import numpy as np
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import spmv_acc_amd

    def median_region(fn, reps=5, regions=7):
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

    def stencil(shape):
        """the full 3^d stencil on a grid of `shape` points: (m, rowptr, colindex, value), rows strictly ascending"""
        m = int(np.prod(shape))
        coords = torch.unravel_index(torch.arange(m, device="cuda"), shape)
        cols, valid = [], []
        for off in np.ndindex(*([3] * len(shape))):
            ok = torch.ones(m, dtype=torch.bool, device="cuda")
            col = torch.zeros(m, dtype=torch.int64, device="cuda")
            for c, o, s in zip(coords, off, shape):
                q = c + (o - 1)
                ok &= (q >= 0) & (q < s)
                col = col * s + q
            cols.append(col)
            valid.append(ok)
        cols, valid = torch.stack(cols, 1), torch.stack(valid, 1)  # (offsets ascend in the flattened column: every row ascends)
        lens = valid.sum(1)
        rp = torch.zeros(m + 1, dtype=torch.int32, device="cuda")
        rp[1:] = torch.cumsum(lens, 0).int()
        ci = cols[valid].int()
        row = torch.repeat_interleave(torch.arange(m, device="cuda"), lens)
        v = torch.where(ci.long() == row, lens[row].double(), torch.full((), -1.0, dtype=torch.float64, device="cuda"))
        return m, rp, ci.contiguous(), v.contiguous(), row

    def rounds_of(m, row, ci):
        """the rounds the pattern needs: the longest chain of descending priority (the definition's mix32, in torch)"""
        x = torch.arange(m, dtype=torch.int64, device="cuda")
        x ^= x >> 16
        x = (x * 0x7FEB352D) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846CA68B) & 0xFFFFFFFF
        x ^= x >> 16
        higher = (x[ci.long()] > x[row]) | ((x[ci.long()] == x[row]) & (ci.long() > row))  # (mix32(v) << 32) | v, compared by its halves
        src, dst = ci.long()[higher], row[higher]
        depth = torch.ones(m, dtype=torch.int64, device="cuda")
        for _ in range(100000):
            new = torch.ones_like(depth).scatter_reduce(0, dst, depth[src] + 1, reduce="amax")
            if torch.equal(new, depth):
                break
            depth = new
        return int(depth.max().item())

    lib = spmv_acc_amd.load_library()
    src = torch.empty(1 << 27, dtype=torch.float64, device="cuda").normal_()
    dst = torch.empty_like(src)
    ceiling = spmv_acc_amd.copy_ceiling_gbs(dst, src, reps=5)
    del src, dst
    if name == "fem_quads":
        side = max(8, int(2001 * scale))
        shape = (side, side)
    elif name == "grid27":
        side = max(4, int(150 * scale ** (2.0 / 3.0)))
        shape = (side, side, side)
    else:
        raise SystemExit(f"unknown matrix {name}")
    m, rp, ci, v, row = stencil(shape)
    nnz = ci.numel()
    print(f"# {name}: {m} rows, {nnz} non-zeros", file=sys.stderr, flush=True)
    lib.spmv_acc_set_stream(torch.cuda.current_stream().cuda_stream)

    # the yardstick first, on the untouched SpMV path
    x = torch.randn(m, dtype=torch.float64, device="cuda")
    y = torch.randn(m, dtype=torch.float64, device="cuda")
    spmv_acc_amd.prepare(m, m, nnz, rp, ci, v, x, beta=1.0)
    region = spmv_acc_amd.time_spmv_region(spmv_acc_amd.get_strategy(), 10, 1.0, 1.0, m, m, nnz, rp, ci, v, x, y)
    spmv_ms = float(np.median([region() for _ in range(7)])) / 10
    spmv_acc_amd.release_plans(rp)
    del y

    color_ms = median_host(lambda: spmv_acc_amd.csr_color(m, rp, ci))
    color, color_rows, color_ptr, no_diag = spmv_acc_amd.csr_color(m, rp, ci)
    off = ci.long() != row
    proper = not bool((color[row[off]] == color[ci.long()[off]]).any().item())
    rounds = rounds_of(m, row, ci)
    del off, row
    torch.cuda.empty_cache()
    launches = 2 * sum(1 for a, b in zip(color_ptr, color_ptr[1:]) if b > a)

    b = torch.randn(m, dtype=torch.float64, device="cuda")
    p_rp, p_ci, p_v = spmv_acc_amd.csr_permute(m, rp, ci, v, color_rows)
    pb, px = b[color_rows.long()].contiguous(), x[color_rows.long()].contiguous()

    def four_forms(mm, A, rows, bb, xx, P, pbb, pxx, ptr):
        out = {}
        for form, args in (("rows", (mm, *A, ptr, rows, bb, xx)), ("perm", (mm, *P, ptr, None, pbb, pxx))):
            sweep = lambda args=args: spmv_acc_amd.csr_gs_sweep(*args, omega=1.0, direction="symmetric")
            sweep()
            out[f"plain_{form}"] = median_region(sweep)
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            g = torch.cuda.CUDAGraph()
            with torch.cuda.stream(s):
                torch.cuda.synchronize()
                with torch.cuda.graph(g, stream=s):
                    sweep()
            g.replay()
            out[f"graph_{form}"] = median_region(g.replay)
            del g
            if lib.spmv_acc_last_error() != 0:
                raise SystemExit(lib.spmv_acc_last_error_string().decode())
        return out

    t = four_forms(m, (rp, ci, v), color_rows, b, x, (p_rp, p_ci, p_v), pb, px, color_ptr)
    # the two forms computed the same sweeps up to the order of a row's terms: they agree to rounding
    agree = float(((x[color_rows.long()] - px).abs().max() / px.abs().max()).item())

    # the launch floor: the same entry on a path of 3 000 rows
    k = 3000
    i = torch.arange(k, device="cuda")
    t_rows = torch.cat([i, i[1:], i[:-1]])
    t_cols = torch.cat([i, i[:-1], i[1:]])
    order = torch.argsort(t_rows * k + t_cols)
    t_ci = t_cols[order].int().contiguous()
    t_rp = torch.zeros(k + 1, dtype=torch.int32, device="cuda")
    t_rp[1:] = torch.cumsum(torch.bincount(t_rows, minlength=k), 0).int()
    t_v = torch.where(t_ci.long() == t_rows[order], 2.0, -1.0).double().contiguous()
    _, t_color_rows, t_ptr, _ = spmv_acc_amd.csr_color(k, t_rp, t_ci)
    t_P = spmv_acc_amd.csr_permute(k, t_rp, t_ci, t_v, t_color_rows)
    tb, tx = torch.randn(k, dtype=torch.float64, device="cuda"), torch.zeros(k, dtype=torch.float64, device="cuda")
    f = four_forms(k, (t_rp, t_ci, t_v), t_color_rows, tb, tx, t_P, tb.clone(), tx.clone(), t_ptr)
    t_launches = 2 * (len(t_ptr) - 1)

    r = {"matrix": name, "m": m, "nnz": nnz, "colors": len(color_ptr) - 1, "rounds": rounds, "proper": proper, "no_diag": no_diag,
         "launches": launches, "color_ms": round(color_ms, 3), "color_spmvs": round(color_ms / spmv_ms, 1),
         "sweep_plain_rows_ms": round(t["plain_rows"], 4), "sweep_graph_rows_ms": round(t["graph_rows"], 4),
         "sweep_plain_perm_ms": round(t["plain_perm"], 4), "sweep_graph_perm_ms": round(t["graph_perm"], 4), "forms_agree_rel": agree,
         "spmv_ms": round(spmv_ms, 5), "floor_plain_us": round(1e3 * f["plain_perm"] / t_launches, 2),
         "floor_graph_us": round(1e3 * f["graph_perm"] / t_launches, 2), "copy_ceiling_gbs": round(ceiling, 1)}
    for form in ("plain_rows", "graph_rows", "plain_perm", "graph_perm"):
        r[f"ratio_{form}"] = round(t[form] / (2 * spmv_ms), 2)  # a symmetric sweep against the two SpMVs whose bytes it moves
    print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--matrices", default="fem_quads,grid27")
    ap.add_argument("--md", default=None)
    ap.add_argument("--limit", type=int, default=420, help="seconds a matrix may take")
    ap.add_argument("--scale", type=float, default=1.0, help="rows relative to the documented size (a rehearsal at a small size)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.scale)
        return
    rows = []
    for name in a.matrices.split(","):  # (this process never opens the GPU: one child per matrix, each under its own limit)
        try:
            done = subprocess.run([sys.executable, os.path.abspath(__file__), a.out, "--child", name, "--scale", str(a.scale)], stdout=subprocess.PIPE,
                                  text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"{name}: no result within {a.limit} s; nothing more is started")
        if done.returncode != 0:
            raise SystemExit(f"{name}: the child ended with {done.returncode}; nothing more is started")
        rows += [json.loads(ln) for ln in done.stdout.splitlines() if ln.startswith("{")]
    doc = {"copy_ceiling_gbs": rows[0]["copy_ceiling_gbs"] if rows else None, "scale": a.scale, "rows": rows}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    if a.md:
        with open(a.md, "w") as f:
            f.write("# Multicolour Gauss-Seidel: tools/gs_bench.py\n\n")
            f.write("MI355X, fp64.  Times in ms (medians; see the tool's docstring for each protocol).  `sweep` = ONE symmetric sweep, omega = 1: "
                    "2 x colours launches.  `plain` = the entry's launches on the stream, `graph` = the sweep captured once and replayed; `rows` = "
                    "through color_rows on the original matrix, `perm` = on the colour-permuted matrix.  `/ 2 SpMV` = the sweep's time over two "
                    "settled SpMVs of the engine on the same matrix in the same process: a sweep moves one SpMV's bytes per direction.  `floor` = "
                    "the time per launch of the same entry on a path of 3 000 rows, plain / replayed, in us.\n\n")
            f.write("| matrix | rows | nnz | csr_color | in SpMVs | colours | rounds | launches | SpMV | sweep plain rows | / 2 SpMV | sweep graph rows | "
                    "/ 2 SpMV | sweep plain perm | / 2 SpMV | sweep graph perm | / 2 SpMV | floor | copy GB/s |\n")
            f.write("|" + "---|" * 19 + "\n")
            for r in rows:
                f.write(f"| {r['matrix']} | {r['m']} | {r['nnz']} | {r['color_ms']:.2f} | {r['color_spmvs']:.0f} | {r['colors']} | {r['rounds']} | "
                        f"{r['launches']} | {r['spmv_ms']:.4f} | {r['sweep_plain_rows_ms']:.4f} | {r['ratio_plain_rows']:.2f} | "
                        f"{r['sweep_graph_rows_ms']:.4f} | {r['ratio_graph_rows']:.2f} | {r['sweep_plain_perm_ms']:.4f} | {r['ratio_plain_perm']:.2f} | "
                        f"{r['sweep_graph_perm_ms']:.4f} | {r['ratio_graph_perm']:.2f} | {r['floor_plain_us']:.1f} / {r['floor_graph_us']:.1f} | "
                        f"{r['copy_ceiling_gbs']:.0f} |\n")
            f.write("\nWhat separates a sweep from two SpMVs, per matrix (ms): `launch term` = launches x the replayed floor; `indirection` = graph "
                    "rows - graph perm (the same launches with and without the row indirection and its scattered rows); `rest` = graph perm - 2 SpMV "
                    "- launch term (the sweep kernel against the engine's tuned SpMV kernels on the same bytes).\n\n")
            f.write("| matrix | graph perm - 2 SpMV | launch term | rest | indirection | host launches: plain perm - graph perm |\n|---|---|---|---|---|---|\n")
            for r in rows:
                gap = r["sweep_graph_perm_ms"] - 2 * r["spmv_ms"]
                launch = r["launches"] * r["floor_graph_us"] * 1e-3
                f.write(f"| {r['matrix']} | {gap:.4f} | {launch:.4f} | {gap - launch:.4f} | {r['sweep_graph_rows_ms'] - r['sweep_graph_perm_ms']:.4f} | "
                        f"{r['sweep_plain_perm_ms'] - r['sweep_graph_perm_ms']:.4f} |\n")


if __name__ == "__main__":
    main()
