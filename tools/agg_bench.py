#!/usr/bin/env python3
"""The aggregation coarsening (spmv_acc_csr_aggregate, spmv_acc_csr_tentative_values) on tools/gs_bench.py's two mesh matrices, made on the
device: `fem_quads`, the 9-point pattern of a bilinear-quad assembly on a 2000 x 2000 element grid (4.0 M rows), and `grid27`, the 27-point
stencil on 150^3 points (3.4 M rows).  One JSON line each:
  agg_ms           spmv_acc_csr_aggregate: median of 3 calls after one warm-up, host clock between device synchronisations (the entry synchronises)
  color_ms         spmv_acc_csr_color on the same matrix in the same process, the same protocol: the yardstick from before this entry existed --
                   the same census, the same round machinery, the same sort
  spmv_ms          the engine's settled SpMV on the same matrix (spmv_acc_time_spmv_region, 10 calls per region, median of 7), beta = 1
  rounds, groups   the rounds the pattern needs, from the key / T1 / T2 form iterated with torch to its end, and the groups of kAggRoundsPerRead
                   rounds the entry therefore enqueues (each ends with one synchronising read)
  naggs, sizes     the aggregates and the distribution of their sizes (min, median, mean, max, and a histogram by size)
  valid            every row has an aggregate in [0, naggs), every aggregate is non-empty, agg_rows is a permutation sorted by aggregate and
                   agg_ptr its pointer (checked with torch)
  values_*_ms      spmv_acc_csr_tentative_values with b and R's values: median of 7 regions of 20 calls between one event pair, after a warm-up:
                   plain = the entry's two launches on the stream, graph = captured once and replayed
  copy_ms          torch's device copy of as many bytes as the values pass must move at least (36 B per row: agg, agg_rows twice, b, P's and
                   R's values; 20 B per aggregate: agg_ptr, bc written and read), half read and half written, the same protocol
  copy_ceiling_gbs spmv_acc_copy_ceiling_gbs on this box in this run (1 GiB)
--lib NAME=PATH measures another build of the library (a different kAggLaneGroup or kAggPerLane) under the label NAME; the default label is `shipped`.
Every matrix and library runs in a child process of its own under a time limit; after a child that fails or runs out of time nothing more is
started.
usage: tools/agg_bench.py OUT.json [--matrices fem_quads,grid27] [--md OUT.md] [--limit SECONDS] [--scale 1.0] [--lib NAME=PATH ...]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROUNDS_PER_READ = 4  # kAggRoundsPerRead


def child(name, scale, label, lib_path):
    import numpy as np
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import spmv_acc_amd

    if lib_path:
        spmv_acc_amd.LIB_PATH = os.path.abspath(lib_path)

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

    def stencil(shape):
        """the full 3^d stencil on a grid of `shape` points: (m, rowptr, colindex, value, row of every entry), rows strictly ascending"""
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
        """the rounds the pattern needs: the key / T1 / T2 form in torch (mix32 alone orders the rows: it is a bijection)"""
        x = torch.arange(m, dtype=torch.int64, device="cuda")
        x ^= x >> 16
        x = (x * 0x7FEB352D) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846CA68B) & 0xFFFFFFFF
        x ^= x >> 16
        root, out = 1 << 40, 0
        key = x + 1
        col = ci.long()
        rounds = 0
        while True:
            undecided = (key != root) & (key != out)
            if not bool(undecided.any()):
                return rounds, key == root
            t1 = key.clone().scatter_reduce(0, row, key[col], reduce="amax")
            t2 = t1.clone().scatter_reduce(0, row, t1[col], reduce="amax")
            key = torch.where(undecided & (t2 == root), torch.full_like(key, out), torch.where(undecided & (t2 == key), torch.full_like(key, root), key))
            rounds += 1

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
    print(f"# {name} [{label}]: {m} rows, {nnz} non-zeros", file=sys.stderr, flush=True)
    lib.spmv_acc_set_stream(torch.cuda.current_stream().cuda_stream)

    # the yardsticks first: the settled SpMV and the colouring
    x = torch.randn(m, dtype=torch.float64, device="cuda")
    y = torch.randn(m, dtype=torch.float64, device="cuda")
    spmv_acc_amd.prepare(m, m, nnz, rp, ci, v, x, beta=1.0)
    region = spmv_acc_amd.time_spmv_region(spmv_acc_amd.get_strategy(), 10, 1.0, 1.0, m, m, nnz, rp, ci, v, x, y)
    spmv_ms = float(np.median([region() for _ in range(7)])) / 10
    spmv_acc_amd.release_plans(rp)
    del x, y, v
    color_ms = median_host(lambda: spmv_acc_amd.csr_color(m, rp, ci))
    colors = len(spmv_acc_amd.csr_color(m, rp, ci)[2]) - 1

    agg_ms = median_host(lambda: spmv_acc_amd.csr_aggregate(m, rp, ci))
    agg, agg_ptr, agg_rows, naggs = spmv_acc_amd.csr_aggregate(m, rp, ci)
    rounds, roots = rounds_of(m, row, ci)
    sizes = torch.bincount(agg.long(), minlength=naggs)
    valid = (0 <= int(agg.min()) and int(agg.max()) == naggs - 1 and int(sizes.min()) >= 1 and int(roots.sum()) == naggs
             and bool((agg[roots.nonzero().squeeze(1)] == torch.arange(naggs, device="cuda")).all())
             and torch.equal(torch.sort(agg_rows.long()).values, torch.arange(m, device="cuda"))
             and torch.equal(agg_rows.long(), torch.sort(agg.long(), stable=True).indices)
             and torch.equal(agg_ptr.long(), torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(sizes, 0)])))
    hist = torch.bincount(sizes).cpu().tolist()
    del row, roots
    torch.cuda.empty_cache()

    b = torch.randn(m, dtype=torch.float64, device="cuda")
    p, r, bc = (torch.empty(n, dtype=torch.float64, device="cuda") for n in (m, m, naggs))
    values = lambda: spmv_acc_amd.csr_tentative_values(m, agg, agg_ptr, agg_rows, b, p, r, bc)
    values()
    plain = median_region(values)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            values()
    g.replay()
    graph = median_region(g.replay)
    del g
    if lib.spmv_acc_last_error() != 0:
        raise SystemExit(lib.spmv_acc_last_error_string().decode())
    gram = torch.zeros(naggs, dtype=torch.float64, device="cuda").index_add_(0, agg.long(), p * p)
    orthonormal = float((gram - 1.0).abs().max().item())
    values_bytes = 36 * m + 20 * naggs
    c_src = torch.randn(values_bytes // 16, dtype=torch.float64, device="cuda")
    c_dst = torch.empty_like(c_src)
    copy_ms = median_region(lambda: c_dst.copy_(c_src))

    out = {"matrix": name, "lib": label, "m": m, "nnz": nnz, "agg_ms": round(agg_ms, 3), "agg_spmvs": round(agg_ms / spmv_ms, 1),
           "color_ms": round(color_ms, 3), "colors": colors, "agg_over_color": round(agg_ms / color_ms, 2), "spmv_ms": round(spmv_ms, 5),
           "rounds": rounds, "groups": -(-rounds // ROUNDS_PER_READ), "naggs": naggs, "rows_per_agg": round(m / naggs, 2), "valid": bool(valid),
           "size_min": int(sizes.min()), "size_median": float(sizes.double().median()), "size_max": int(sizes.max()), "size_hist": hist,
           "values_plain_ms": round(plain, 4), "values_graph_ms": round(graph, 4), "copy_ms": round(copy_ms, 4), "values_bytes": values_bytes,
           "values_over_copy": round(graph / copy_ms, 2), "gram_minus_identity": orthonormal, "copy_ceiling_gbs": round(ceiling, 1)}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--matrices", default="fem_quads,grid27")
    ap.add_argument("--md", default=None)
    ap.add_argument("--limit", type=int, default=420, help="seconds a matrix may take")
    ap.add_argument("--scale", type=float, default=1.0, help="rows relative to the documented size (a rehearsal at a small size)")
    ap.add_argument("--lib", action="append", default=[], help="NAME=PATH: also measure another build of the library")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--label", default="shipped", help=argparse.SUPPRESS)
    ap.add_argument("--lib-path", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.scale, a.label, a.lib_path)
        return
    libs = [("shipped", "")] + [tuple(spec.split("=", 1)) for spec in a.lib]
    rows = []
    for name in a.matrices.split(","):  # (this process never opens the GPU: one child per matrix and library, each under its own limit)
        for label, path in libs:
            try:
                done = subprocess.run([sys.executable, os.path.abspath(__file__), a.out, "--child", name, "--scale", str(a.scale), "--label", label,
                                       "--lib-path", path], stdout=subprocess.PIPE, text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                raise SystemExit(f"{name} [{label}]: no result within {a.limit} s; nothing more is started")
            if done.returncode != 0:
                raise SystemExit(f"{name} [{label}]: the child ended with {done.returncode}; nothing more is started")
            rows += [json.loads(ln) for ln in done.stdout.splitlines() if ln.startswith("{")]
    doc = {"copy_ceiling_gbs": rows[0]["copy_ceiling_gbs"] if rows else None, "scale": a.scale, "rows": rows}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    if a.md:
        with open(a.md, "w") as f:
            f.write("# Aggregation coarsening: tools/agg_bench.py\n\n")
            f.write("MI355X.  Times in ms (medians; see the tool's docstring for each protocol).  `csr_aggregate` and `csr_color` are whole calls on "
                    "the same matrix in the same process, host clock; `in SpMVs` = csr_aggregate over one settled SpMV of the engine on that "
                    "matrix.  `groups` = groups of 4 rounds, each ended by one synchronising read.  `values` = spmv_acc_csr_tentative_values with b "
                    "and R's values, `plain` on the stream and `graph` replayed; `copy` = torch's device copy of the bytes the pass must move.  "
                    "`lib` = the build measured: `shipped` (kAggLaneGroup 1, kAggPerLane 1), `g4` / `g8` = four / eight lanes per row in the neighbourhood pass, `p2` / `p4` = two / four aggregates per lane in the norms pass.\n\n")
            f.write("| matrix | lib | rows | nnz | csr_aggregate | in SpMVs | csr_color | aggregate / color | SpMV | rounds | groups | aggregates | rows / "
                    "aggregate | sizes min / median / max | values plain | values graph | copy | graph / copy | copy GB/s |\n")
            f.write("|" + "---|" * 19 + "\n")
            for r in rows:
                f.write(f"| {r['matrix']} | {r['lib']} | {r['m']} | {r['nnz']} | {r['agg_ms']:.2f} | {r['agg_spmvs']:.0f} | {r['color_ms']:.2f} | "
                        f"{r['agg_over_color']:.2f} | {r['spmv_ms']:.4f} | {r['rounds']} | {r['groups']} | {r['naggs']} | {r['rows_per_agg']:.1f} | "
                        f"{r['size_min']} / {r['size_median']:.0f} / {r['size_max']} | {r['values_plain_ms']:.4f} | {r['values_graph_ms']:.4f} | "
                        f"{r['copy_ms']:.4f} | {r['values_over_copy']:.2f} | {r['copy_ceiling_gbs']:.0f} |\n")
            f.write("\nAggregates by size (rows: count), shipped build:\n\n")
            for r in rows:
                if r["lib"] == "shipped":
                    f.write(f"- {r['matrix']}: " + ", ".join(f"{n}: {c}" for n, c in enumerate(r["size_hist"]) if c) + "\n")
            if not all(r["valid"] for r in rows):
                f.write("\n**A result failed the tool's validity check.**\n")


if __name__ == "__main__":
    main()
