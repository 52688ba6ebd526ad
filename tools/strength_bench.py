#!/usr/bin/env python3
"""The strength-of-connection filter and the prolongator smoother (spmv_acc_csr_strength, spmv_acc_csr_strength_values) on tools/agg_bench.py's
two mesh matrices, made on the device with ANISOTROPIC values: `fem_quads`, the 9-point pattern on 2001 x 2001 nodes (4.0 M rows) with the four
axis couplings strong and the four corner couplings 0.05 of them, and `grid27`, the 27-point stencil on 150^3 points (3.4 M rows) with the six
face couplings and the eight edge couplings that leave the last axis strong, the other twelve 0.02 of them; every coupling carries a seeded
factor in [0.9, 1.1] of its own (the two directions of an edge differ), the diagonal is the row's absolute sum, theta = 0.05: 4 of 9 and 12 of
27 entries of an inner row drop.  One JSON line each:
  strength_ms      spmv_acc_csr_strength: median of 3 calls after one warm-up, host clock between device synchronisations (the entry synchronises)
  spmv_ms          the engine's settled SpMV on the same matrix (spmv_acc_time_spmv_region, 10 calls per region, median of 7), beta = 1
  nnz_s, dropped   the kept entries and the share of A's entries that drop
  valid            the kept flags recomputed with torch from the definition (the same products, the mirror by a sort) give the same s_rowptr,
                   s_colindex, map and drop_ptr; row sums of A_F against those of A (largest difference relative to the row's absolute sum)
  values_*_ms      spmv_acc_csr_strength_values, omega = 0 (A_F) and omega = 2/3 (M): median of 7 regions of 20 calls between one event pair,
                   after a warm-up: plain = the entry's two launches on the stream, graph = captured once and replayed
  *_copy_ms        torch's device copy of as many bytes as the pass must move at least, half read and half written, the same protocol.
                   analysis: rowptr, colindex and value read, the two pointers, s_colindex and map written = 12 (m + 1) + 16 nnz + 4 nnz_s
                   (the census, the flags, their scan and the mirror gathers are NOT counted: what the result needs, not what the passes do);
                   values: 36 B per row (two pointers, the diagonal read, diag written and read), 12 B per dropped entry, 24 B per kept one
  copy_ceiling_gbs spmv_acc_copy_ceiling_gbs on this box in this run (1 GiB)
The flags pass maps lanes to ENTRIES (strength.hpp PASSES).  FLAGS_KERNEL_MS below holds what the flags kernel took in both mappings on the same
matrices, from kernel traces of this tool's child with the shipped build and with a build that walked one row per lane (it returned the same
arrays and is not kept); it is written into the files beside this run's figures.
Every matrix runs in a child process of its own under a time limit; after a child that fails or runs out of time nothing more is started.
usage: tools/strength_bench.py OUT.json [--matrices fem_quads,grid27] [--md OUT.md] [--limit SECONDS] [--scale 1.0]"""
import argparse
import json
import os
import subprocess
import sys
import time

THETA = 0.05
OMEGA = 2.0 / 3.0
# the flags kernel in its two mappings and the census beside it, MI355X, full size, means of 5 launches in a kernel trace of this tool's child
FLAGS_KERNEL_MS = {"fem_quads": {"by_entry": 1.499, "by_row": 0.917, "census": 0.297},
                   "grid27": {"by_entry": 3.511, "by_row": 7.518, "census": 2.562}}


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

    def stencil(shape, weak_of, weak):
        """the full 3^d stencil on a grid of `shape` points with anisotropic values: (m, rowptr, colindex, value, row of every entry); rows
        strictly ascend.  weak_of(offset) names the couplings that get `weak` instead of 1"""
        m = int(np.prod(shape))
        coords = torch.unravel_index(torch.arange(m, device="cuda"), shape)
        cols, valid, size = [], [], []
        for off in np.ndindex(*([3] * len(shape))):
            ok = torch.ones(m, dtype=torch.bool, device="cuda")
            col = torch.zeros(m, dtype=torch.int64, device="cuda")
            for c, o, s in zip(coords, off, shape):
                q = c + (o - 1)
                ok &= (q >= 0) & (q < s)
                col = col * s + q
            cols.append(col)
            valid.append(ok)
            size.append(0.0 if all(o == 1 for o in off) else (weak if weak_of(tuple(o - 1 for o in off)) else 1.0))
        cols, valid = torch.stack(cols, 1), torch.stack(valid, 1)  # (offsets ascend in the flattened column: every row ascends)
        lens = valid.sum(1)
        rp = torch.zeros(m + 1, dtype=torch.int32, device="cuda")
        rp[1:] = torch.cumsum(lens, 0).int()
        ci = cols[valid].int()
        row = torch.repeat_interleave(torch.arange(m, device="cuda"), lens)
        gen = torch.Generator(device="cuda").manual_seed(2033)
        base = torch.tensor(size, dtype=torch.float64, device="cuda").expand(m, -1)[valid]
        v = -base * (0.9 + 0.2 * torch.rand(ci.numel(), dtype=torch.float64, device="cuda", generator=gen))
        v = torch.where(ci.long() == row, torch.zeros(m, dtype=torch.float64, device="cuda").index_add_(0, row, v.abs())[row], v)
        return m, rp, ci.contiguous(), v.contiguous(), row

    lib = spmv_acc_amd.load_library()
    src = torch.empty(1 << 27, dtype=torch.float64, device="cuda").normal_()
    dst = torch.empty_like(src)
    ceiling = spmv_acc_amd.copy_ceiling_gbs(dst, src, reps=5)
    del src, dst
    if name == "fem_quads":
        side = max(8, int(2001 * scale))
        m, rp, ci, v, row = stencil((side, side), lambda off: all(o != 0 for o in off), 0.05)
    elif name == "grid27":
        side = max(4, int(150 * scale ** (2.0 / 3.0)))
        m, rp, ci, v, row = stencil((side, side, side), lambda off: sum(o != 0 for o in off) == 3 or (off[2] == 0 and sum(o != 0 for o in off) == 2), 0.02)
    else:
        raise SystemExit(f"unknown matrix {name}")
    nnz = ci.numel()
    print(f"# {name}: {m} rows, {nnz} non-zeros", file=sys.stderr, flush=True)
    lib.spmv_acc_set_stream(torch.cuda.current_stream().cuda_stream)

    # the yardstick first: the settled SpMV
    x = torch.randn(m, dtype=torch.float64, device="cuda")
    y = torch.randn(m, dtype=torch.float64, device="cuda")
    spmv_acc_amd.prepare(m, m, nnz, rp, ci, v, x, beta=1.0)
    region = spmv_acc_amd.time_spmv_region(spmv_acc_amd.get_strategy(), 10, 1.0, 1.0, m, m, nnz, rp, ci, v, x, y)
    spmv_ms = float(np.median([region() for _ in range(7)])) / 10
    spmv_acc_amd.release_plans(rp)
    del x, y

    strength_ms = median_host(lambda: spmv_acc_amd.csr_strength(m, rp, ci, v, THETA))
    (s_rp, s_ci, a_f), smap, drop_ptr, diag, no_diag = spmv_acc_amd.csr_strength(m, rp, ci, v, THETA)
    nnz_s = s_ci.numel()

    # the definition with torch: the same two products per entry, the mirror's position by a sort of (column, row)
    col = ci.long()
    sd = torch.zeros(m, dtype=torch.float64, device="cuda")
    on_diag = col == row
    sd[row[on_diag]] = v[on_diag].abs().sqrt()
    mirror = torch.sort(col * m + row, stable=True).indices
    rhs = (sd[row] * sd[col]) * THETA
    keep = on_diag | (v.abs() >= rhs) | (v.abs()[mirror] >= rhs)
    pos = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(keep.long(), 0)])
    valid = (int(pos[-1]) == nnz_s and torch.equal(s_rp.long(), pos[rp.long()]) and torch.equal(drop_ptr.long(), nnz_s + rp.long() - pos[rp.long()])
             and torch.equal(smap[:nnz_s].long(), keep.nonzero().squeeze(1)) and torch.equal(smap[nnz_s:].long(), (~keep).nonzero().squeeze(1))
             and torch.equal(s_ci, ci[keep]) and no_diag == 0)
    srow = row[keep]
    sum_a = torch.zeros(m, dtype=torch.float64, device="cuda").index_add_(0, row, v)
    sum_f = torch.zeros(m, dtype=torch.float64, device="cuda").index_add_(0, srow, a_f)
    scale_a = torch.zeros(m, dtype=torch.float64, device="cuda").index_add_(0, row, v.abs())
    rowsum_err = float(((sum_a - sum_f).abs() / scale_a).max().item())
    del col, sd, mirror, rhs, keep, pos, srow, sum_a, sum_f, scale_a, row, on_diag
    torch.cuda.empty_cache()

    out_v = torch.empty(nnz_s, dtype=torch.float64, device="cuda")
    out_d = torch.empty(m, dtype=torch.float64, device="cuda")
    timings = {}
    for label, omega in (("af", 0.0), ("m", OMEGA)):
        values = lambda: spmv_acc_amd.csr_strength_values(m, s_rp, s_ci, smap, drop_ptr, v, out_v, out_d, omega)
        values()
        timings[f"values_{label}_plain_ms"] = median_region(values)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=s):
                values()
        g.replay()
        timings[f"values_{label}_graph_ms"] = median_region(g.replay)
        del g
    if lib.spmv_acc_last_error() != 0:
        raise SystemExit(lib.spmv_acc_last_error_string().decode())
    analysis_bytes = 12 * (m + 1) + 16 * nnz + 4 * nnz_s
    values_bytes = 36 * m + 12 * (nnz - nnz_s) + 24 * nnz_s
    copies = {}
    for label, nbytes in (("analysis", analysis_bytes), ("values", values_bytes)):
        c_src = torch.randn(nbytes // 16, dtype=torch.float64, device="cuda")
        c_dst = torch.empty_like(c_src)
        copies[label] = median_region(lambda: c_dst.copy_(c_src))
        del c_src, c_dst

    out = {"matrix": name, "m": m, "nnz": nnz, "theta": THETA, "omega": OMEGA, "nnz_s": nnz_s, "dropped": round(1.0 - nnz_s / nnz, 4),
           "strength_ms": round(strength_ms, 3), "spmv_ms": round(spmv_ms, 5), "strength_spmvs": round(strength_ms / spmv_ms, 1),
           "analysis_bytes": analysis_bytes, "analysis_copy_ms": round(copies["analysis"], 4), "strength_over_copy": round(strength_ms / copies["analysis"], 2),
           "values_bytes": values_bytes, "values_copy_ms": round(copies["values"], 4), "valid": bool(valid), "rowsum_err": rowsum_err,
           "copy_ceiling_gbs": round(ceiling, 1)}
    for k, t in timings.items():
        out[k] = round(t, 4)
    for label in ("af", "m"):
        out[f"values_{label}_spmvs"] = round(timings[f"values_{label}_graph_ms"] / spmv_ms, 2)
        out[f"values_{label}_over_copy"] = round(timings[f"values_{label}_graph_ms"] / copies["values"], 2)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--matrices", default="fem_quads,grid27")
    ap.add_argument("--md", default=None)
    ap.add_argument("--limit", type=int, default=300, help="seconds a matrix may take")
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
    doc = {"copy_ceiling_gbs": rows[0]["copy_ceiling_gbs"] if rows else None, "scale": a.scale, "rows": rows,
           "flags_kernel_ms_at_full_size": FLAGS_KERNEL_MS}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    if a.md:
        with open(a.md, "w") as f:
            f.write("# Strength-of-connection filter and prolongator smoother: tools/strength_bench.py\n\n")
            f.write(f"MI355X.  Times in ms (medians; see the tool's docstring for each protocol).  theta = {THETA}, anisotropic values (the tool's "
                    "docstring).  `csr_strength` is the whole analysis call, host clock; `in SpMVs` = over one settled SpMV of the engine on that matrix; "
                    "`/ copy` = over torch's device copy of the bytes the result must move at least (inputs read once, outputs written once: the "
                    "census, the flags, their scan and the mirror gathers are not counted).  `A_F` = spmv_acc_csr_strength_values with omega = 0, "
                    f"`M` = with omega = {OMEGA:.4f}; `plain` on the stream, `graph` replayed; their `in SpMVs` and `/ copy` are the replayed times.\n\n")
            f.write("MEASURED: every time, nnz_s, the dropped share, the validity check and the row-sum difference.  REASONED, not measured: the "
                    "byte counts behind the two copies (counted from the arrays' sizes); that the flags pass is bound by the mirror's binary "
                    "search and its dependent gathers (no counters were collected).\n\n")
            if a.scale == 1.0:
                f.write("The flags pass maps lanes to ENTRIES (the row by the wavefront's row search).  A build with one ROW per lane returned the "
                        "same arrays and is not kept; the flags kernel alone in both mappings, from kernel traces taken apart from this run: "
                        + "; ".join(f"{k}: by entry {v['by_entry']:.2f} ms, by row {v['by_row']:.2f} ms, the census beside them {v['census']:.2f} ms"
                                    for k, v in FLAGS_KERNEL_MS.items()) + ".\n\n")
            f.write("| matrix | rows | nnz | kept | dropped | csr_strength | in SpMVs | / copy | SpMV | A_F plain | A_F graph | in SpMVs | / copy | "
                    "M plain | M graph | in SpMVs | / copy | copy (analysis) | copy (values) | copy GB/s |\n")
            f.write("|" + "---|" * 20 + "\n")
            for r in rows:
                f.write(f"| {r['matrix']} | {r['m']} | {r['nnz']} | {r['nnz_s']} | {100 * r['dropped']:.1f} % | {r['strength_ms']:.2f} | "
                        f"{r['strength_spmvs']:.0f} | {r['strength_over_copy']:.1f} | {r['spmv_ms']:.4f} | {r['values_af_plain_ms']:.4f} | "
                        f"{r['values_af_graph_ms']:.4f} | {r['values_af_spmvs']:.2f} | {r['values_af_over_copy']:.2f} | {r['values_m_plain_ms']:.4f} | "
                        f"{r['values_m_graph_ms']:.4f} | {r['values_m_spmvs']:.2f} | {r['values_m_over_copy']:.2f} | {r['analysis_copy_ms']:.4f} | "
                        f"{r['values_copy_ms']:.4f} | {r['copy_ceiling_gbs']:.0f} |\n")
            f.write("\nRow sums of A_F against those of A, largest difference relative to the row's absolute sum: "
                    + ", ".join(f"{r['matrix']} {r['rowsum_err']:.1e}" for r in rows) + ".\n")
            if not all(r["valid"] for r in rows):
                f.write("\n**A result failed the tool's validity check.**\n")


if __name__ == "__main__":
    main()
