#!/usr/bin/env python3
"""The device COO -> CSR assembly on the bench's stand-ins (spmv_acc_coo_to_csr, spmv_acc_coo_to_csr_values).  The triple list of a matrix:
every CSR entry split into 1 ... 4 duplicates with random values, the whole list shuffled.  One JSON line per matrix:
  assemble_ms    spmv_acc_coo_to_csr with values and map: median of 3 calls after one warm-up, host clock between device synchronisations (the
                 entry synchronises itself); assemble_spmvs = that time in settled SpMVs of the assembled matrix
  values_ms      spmv_acc_coo_to_csr_values: median of 7 regions of 5 back-to-back calls between one event pair, after one warm-up
  values_gbs     its moved bytes per second: 4 B (start) + 8 B (value) per entry, 4 B (order) + 8 B (gathered val) per triple -- the bytes the
                 pass NEEDS; after the shuffle every 8-B gather is a 128-B request of its own, so the memory system moves far more
  sorted_values_ms   the same pass on the same triples in the CSR's storage order (row by row): order is the identity, the gathers are contiguous
  coalesce_ms    torch.sparse_coo_tensor(indices, val, (m, n)).coalesce() on the same triples (int64 indices, the only form torch takes), median
                 of 3 after one warm-up: structure and values in one step, torch has no values-only pass
  spmv_ms        a settled spmv_acc_csr_spmv on the assembled CSR (spmv_acc_time_spmv_region, 10 calls per region, median of 7 regions), beta = 1
  copy_ceiling_gbs   spmv_acc_copy_ceiling_gbs on this box in this run (1 GiB)
  check          the assembled values against coalesce()'s, max difference relative to the sum of |val| per entry
usage: tools/coo_bench.py OUT.json [--matrices Hardesty3,boneS10] [--md OUT.md]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spmv_acc_amd  # noqa: E402
from spmv_acc_amd import synth  # noqa: E402


def median_region(fn, reps, regions=7):
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


def triples_of(m, rp, ci, seed):
    """(row, col, val) on the GPU: every entry as 1 ... 4 duplicates, shuffled; and the same list in (row, col) order."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    rows = torch.repeat_interleave(torch.arange(m, dtype=torch.int32, device="cuda"), (rp[1:] - rp[:-1]).long())
    reps = torch.randint(1, 5, (ci.numel(),), device="cuda", generator=g)
    row, col = torch.repeat_interleave(rows, reps), torch.repeat_interleave(ci, reps)
    val = torch.rand(row.numel(), dtype=torch.float64, device="cuda", generator=g) * 2 - 1
    perm = torch.randperm(row.numel(), device="cuda", generator=g)
    return (row[perm].contiguous(), col[perm].contiguous(), val[perm].contiguous()), (row, col, val)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--matrices", default="Hardesty3,boneS10")
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    lib = spmv_acc_amd.load_library()
    src = torch.empty(1 << 27, dtype=torch.float64, device="cuda").normal_()
    dst = torch.empty_like(src)
    ceiling = spmv_acc_amd.copy_ceiling_gbs(dst, src, reps=5)
    del src, dst
    rows = []
    for name in a.matrices.split(","):
        m, n, nnz_in, rp, ci, v = synth.sweep_standin_torch(name)
        (row, col, val), (srow, scol, sval) = triples_of(m, rp, ci, seed=len(name))
        del rp, ci, v
        k = row.numel()
        o_rp = torch.empty(m + 1, dtype=torch.int32, device="cuda")
        o_ci = torch.empty(k, dtype=torch.int32, device="cuda")
        o_v = torch.empty(k, dtype=torch.float64, device="cuda")
        o_or = torch.empty(k, dtype=torch.int32, device="cuda")
        o_st = torch.empty(k + 1, dtype=torch.int32, device="cuda")
        h = ctypes.c_int(0)
        lib.spmv_acc_set_stream(torch.cuda.current_stream().cuda_stream)

        def assemble(r=row, c=col, w=val):
            rc = lib.spmv_acc_coo_to_csr(m, n, k, r.data_ptr(), c.data_ptr(), w.data_ptr(), o_rp.data_ptr(), o_ci.data_ptr(), o_v.data_ptr(),
                                         o_or.data_ptr(), o_st.data_ptr(), ctypes.byref(h))
            if rc != 0:
                raise SystemExit(lib.spmv_acc_last_error_string().decode())

        # the sorted list first (its map is overwritten by the shuffled list's below)
        assemble(srow, scol, sval)
        nnz = int(h.value)
        sargs = (k, nnz, o_or.data_ptr(), o_st.data_ptr(), sval.data_ptr(), o_v.data_ptr())
        lib.spmv_acc_coo_to_csr_values(*sargs)
        sorted_values_ms = median_region(lambda: lib.spmv_acc_coo_to_csr_values(*sargs), reps=5)
        del srow, scol, sval
        assemble_ms = median_host(assemble)
        assert int(h.value) == nnz
        vargs = (k, nnz, o_or.data_ptr(), o_st.data_ptr(), val.data_ptr(), o_v.data_ptr())
        lib.spmv_acc_coo_to_csr_values(*vargs)
        values_ms = median_region(lambda: lib.spmv_acc_coo_to_csr_values(*vargs), reps=5)
        if lib.spmv_acc_last_error() != 0:
            raise SystemExit(lib.spmv_acc_last_error_string().decode())
        moved = 4.0 * (nnz + 1) + 8.0 * nnz + 12.0 * k
        # torch on the same triples
        idx = torch.stack([row.long(), col.long()])
        coalesce_ms = median_host(lambda: torch.sparse_coo_tensor(idx, val, (m, n)).coalesce())
        t = torch.sparse_coo_tensor(idx, val, (m, n)).coalesce()
        scale = torch.sparse_coo_tensor(idx, val.abs(), (m, n)).coalesce().values()
        assert t.values().numel() == nnz
        check = float(((t.values() - o_v[:nnz]).abs() / scale.clamp_min(1e-300)).max().item())
        del idx, t, scale
        # a settled SpMV on the assembled matrix
        a_ci, a_v = o_ci[:nnz].clone(), o_v[:nnz].clone()
        x = torch.randn(n, dtype=torch.float64, device="cuda")
        y = torch.randn(m, dtype=torch.float64, device="cuda")
        spmv_acc_amd.prepare(m, n, nnz, o_rp, a_ci, a_v, x, beta=1.0)
        region = spmv_acc_amd.time_spmv_region(spmv_acc_amd.get_strategy(), 10, 1.0, 1.0, m, n, nnz, o_rp, a_ci, a_v, x, y)
        spmv_ms = float(np.median([region() for _ in range(7)])) / 10
        r = {"matrix": name, "m": m, "n": n, "nnz_coo": k, "nnz": nnz, "assemble_ms": round(assemble_ms, 3),
             "assemble_spmvs": round(assemble_ms / spmv_ms, 1), "values_ms": round(values_ms, 4), "values_gbs": round(moved / (values_ms * 1e-3) / 1e9, 1),
             "values_spmvs": round(values_ms / spmv_ms, 1), "sorted_values_ms": round(sorted_values_ms, 4),
             "sorted_values_gbs": round(moved / (sorted_values_ms * 1e-3) / 1e9, 1), "coalesce_ms": round(coalesce_ms, 3),
             "spmv_ms": round(spmv_ms, 5), "copy_ceiling_gbs": round(ceiling, 1), "check": check}
        print(json.dumps(r), flush=True)
        rows.append(r)
        spmv_acc_amd.release_plans(o_rp)
        del row, col, val, o_rp, o_ci, o_v, o_or, o_st, a_ci, a_v, x, y
        torch.cuda.empty_cache()
    doc = {"device": torch.cuda.get_device_name(0), "strategy": spmv_acc_amd.get_strategy(), "copy_ceiling_gbs": round(ceiling, 1), "rows": rows}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    if a.md:
        with open(a.md, "w") as f:
            f.write("# Device COO -> CSR assembly: tools/coo_bench.py\n\n")
            f.write(f"{doc['device']}, strategy {doc['strategy']}, fp64; streaming-copy ceiling of this box in this run: {doc['copy_ceiling_gbs']} GB/s.  "
                    "Triples: every CSR entry of the stand-in as 1 ... 4 duplicates, shuffled.  Times in ms (medians; see the tool's docstring for each "
                    "protocol).  `GB/s` = the bytes the values pass needs (12 B per triple + 12 B per entry) / its time; `sorted` = the same pass on the "
                    "triples in the CSR's storage order (contiguous gathers).\n\n")
            f.write("| matrix | m | triples | entries | coo_to_csr | in SpMVs | coo_to_csr_values | GB/s | in SpMVs | values, sorted triples | GB/s | "
                    "torch coalesce() | settled SpMV | differs from coalesce by |\n")
            f.write("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                f.write(f"| {r['matrix']} | {r['m']} | {r['nnz_coo']} | {r['nnz']} | {r['assemble_ms']:.2f} | {r['assemble_spmvs']:.0f} | {r['values_ms']:.3f} | "
                        f"{r['values_gbs']:.0f} | {r['values_spmvs']:.1f} | {r['sorted_values_ms']:.3f} | {r['sorted_values_gbs']:.0f} | {r['coalesce_ms']:.2f} | "
                        f"{r['spmv_ms']:.4f} | {r['check']:.1e} |\n")


if __name__ == "__main__":
    main()
