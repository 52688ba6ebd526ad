#!/usr/bin/env python3
"""The device CSR SpGEMM (spmv_acc_csr_spgemm_products, spmv_acc_csr_spgemm, spmv_acc_csr_spgemm_values) on the bench's stand-ins.  Per matrix A
two jobs: A * A (a rectangular stand-in: A^T * A on the device-made transpose), and the Galerkin-shaped R * (A * P) with P a piecewise-constant
aggregation 8 : 1 (P[i, i // 8] = 1, R the same aggregation of the rows, = P^T for a square A; the row reports both products together).  Where a job's product count is beyond what the entry takes (INT_MAX - 2^16, or --max-products), the job multiplies
the leading rows of the left factor that stay under it and says which (rows of C are independent).  One JSON line per job:
  nprod, nnz_c     the product count (spmv_acc_csr_spgemm_products) and nnz(C)
  structure_ms     spmv_acc_csr_spgemm with values and map: median of 3 calls after one warm-up, host clock between device synchronisations (the
                   entry synchronises itself); structure_spmvs = that time in settled SpMVs of A
  values_ms        spmv_acc_csr_spgemm_values: median of 7 regions of 5 back-to-back calls between one event pair, after one warm-up
  values_gbs       the bytes the pass NEEDS per second: 8 B of map and 16 B of gathers per product, 4 B (start) + 8 B (value) per entry
  torch_ms         torch.sparse CSR @ CSR on the same inputs (rocSPARSE underneath; structure and values in one step, no values-only pass), median
                   of 3 after one warm-up; null with the reason where torch refuses
  spmv_ms          a settled spmv_acc_csr_spmv on A (spmv_acc_time_spmv_region, 10 calls per region, median of 7 regions), beta = 1: the unit
  copy_ceiling_gbs spmv_acc_copy_ceiling_gbs on this box in this run (1 GiB)
  check            the values against torch's where it ran, max difference relative to the product of the absolute values, entrywise
usage: tools/spgemm_bench.py OUT.json [--matrices Hardesty3,boneS10] [--md OUT.md] [--max-products N]"""
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

INT_LIMIT = 2 ** 31 - 1 - 2 ** 16


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


def leading_rows(m, a, b_rp, cap):
    """(rows, A restricted to them): the longest leading row range of A whose product count with B stays within cap."""
    rp, ci, v = a
    cum = torch.cumsum((b_rp[1:] - b_rp[:-1])[ci.long()].long(), 0)
    upto = torch.cat([cum.new_zeros(1), cum])[rp.long()]  # products of rows [0, r)
    rows = int(torch.searchsorted(upto, torch.tensor([cap], device=upto.device), right=True).item()) - 1
    rows = max(min(rows, m), 0)
    end = int(rp[rows].item())
    return rows, (rp[:rows + 1].contiguous(), ci[:end].contiguous(), v[:end].contiguous())


class Product:
    """One C = A * B with arrays kept for the values pass."""

    def __init__(self, lib, m, k, n, a, b, cap):
        self.lib, self.k, self.n, self.b = lib, k, n, b
        self.rows, self.a = leading_rows(m, a, b[0], cap)
        self.m = self.rows
        self.nprod = spmv_acc_amd.csr_spgemm_products(self.m, k, self.a[0], self.a[1], b[0]) if self.m else 0
        p = self.nprod
        self.rp = torch.empty(self.m + 1, dtype=torch.int32, device="cuda")
        self.ci = torch.empty(p, dtype=torch.int32, device="cuda")
        self.v = torch.empty(p, dtype=torch.float64, device="cuda")
        self.pa, self.pb = torch.empty(p, dtype=torch.int32, device="cuda"), torch.empty(p, dtype=torch.int32, device="cuda")
        self.st = torch.empty(p + 1, dtype=torch.int32, device="cuda")
        self.h = ctypes.c_int(0)
        self.nnz = 0

    def structure(self):
        a, b = self.a, self.b
        rc = self.lib.spmv_acc_csr_spgemm(self.m, self.k, self.n, a[1].numel(), a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), b[1].numel(),
                                          b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), self.nprod, self.rp.data_ptr(), self.ci.data_ptr(),
                                          self.v.data_ptr(), self.pa.data_ptr(), self.pb.data_ptr(), self.st.data_ptr(), ctypes.byref(self.h))
        if rc != 0:
            raise SystemExit(self.lib.spmv_acc_last_error_string().decode())
        self.nnz = int(self.h.value)

    def values(self):
        self.lib.spmv_acc_csr_spgemm_values(self.nprod, self.nnz, self.pa.data_ptr(), self.pb.data_ptr(), self.st.data_ptr(), self.a[2].data_ptr(),
                                            self.b[2].data_ptr(), self.v.data_ptr())

    def result(self):
        return self.rp, self.ci[:self.nnz].contiguous(), self.v[:self.nnz].contiguous()

    def needed_bytes(self):
        return 24.0 * self.nprod + 12.0 * self.nnz + 4.0


def torch_csr(m, n, a):
    return torch.sparse_csr_tensor(a[0], a[1], a[2], size=(m, n))


def measure(lib, name, job, chain, spmv_ms, ceiling, cap):
    """chain: [(m, k, n, a, b) or a callable taking the previous result], multiplied left to right as (.. (A1 * B1) ..)."""
    structure_ms = values_ms = needed = 0.0
    nprod = nnz = 0
    ranges = []
    prev = None
    for step in chain:
        m, k, n, a, b = step(prev) if callable(step) else step
        p = Product(lib, m, k, n, a, b, cap)
        print(f"# {name}: {job}: {p.m} x {k} times {k} x {n}, {p.nprod} products", file=sys.stderr, flush=True)
        if p.rows != m:
            ranges.append(f"rows [0, {p.rows}) of {m}")
        structure_ms += median_host(p.structure)
        p.values()
        values_ms += median_region(p.values, reps=5)
        if lib.spmv_acc_last_error() != 0:
            raise SystemExit(lib.spmv_acc_last_error_string().decode())
        needed += p.needed_bytes()
        nprod, nnz = nprod + p.nprod, p.nnz
        prev = (p.m, n, p.result(), p.a, b, k)
    # torch on the same inputs; only the single-product job is compared value by value
    torch_ms, check, why = None, None, None
    try:
        m1, n1, c, a, b, k1 = prev
        ta, tb = torch_csr(m1, k1, a), torch_csr(k1, n1, b)
        if len(chain) == 1:
            torch_ms = median_host(lambda: ta @ tb)
            tc = ta @ tb
            ts = torch_csr(m1, k1, (a[0], a[1], a[2].abs())) @ torch_csr(k1, n1, (b[0], b[1], b[2].abs()))
            if tc.values().numel() == c[2].numel():
                check = float(((tc.values() - c[2]).abs() / ts.values().clamp_min(1e-300)).max().item())
            else:
                why = f"torch returns {tc.values().numel()} entries"
        else:
            first = chain[0]
            t1a, t1b = torch_csr(first[0], first[1], first[3]), torch_csr(first[1], first[2], first[4])
            torch_ms = median_host(lambda: ta @ (t1a @ t1b))  # (ta: the last product's left factor, R)
    except Exception as e:  # noqa: BLE001 -- torch refusing the product is a result of the comparison, not an error of the tool
        why = f"{type(e).__name__}: {str(e).splitlines()[0][:160]}"
    r = {"matrix": name, "job": job, "range": "; ".join(ranges) or "whole", "nprod": nprod, "nnz_c": nnz, "structure_ms": round(structure_ms, 3),
         "structure_spmvs": round(structure_ms / spmv_ms, 1), "values_ms": round(values_ms, 4), "values_gbs": round(needed / (values_ms * 1e-3) / 1e9, 1),
         "values_spmvs": round(values_ms / spmv_ms, 1), "torch_ms": None if torch_ms is None else round(torch_ms, 3), "torch_note": why,
         "spmv_ms": round(spmv_ms, 5), "copy_ceiling_gbs": round(ceiling, 1), "check": check}
    print(json.dumps(r), flush=True)
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--matrices", default="Hardesty3,boneS10")
    ap.add_argument("--md", default=None)
    ap.add_argument("--max-products", type=int, default=INT_LIMIT)
    a = ap.parse_args()
    cap = min(a.max_products, INT_LIMIT)
    lib = spmv_acc_amd.load_library()
    src = torch.empty(1 << 27, dtype=torch.float64, device="cuda").normal_()
    dst = torch.empty_like(src)
    ceiling = spmv_acc_amd.copy_ceiling_gbs(dst, src, reps=5)
    del src, dst
    rows = []
    for name in a.matrices.split(","):
        m, n, nnz, rp, ci, v = synth.sweep_standin_torch(name)
        lib.spmv_acc_set_stream(torch.cuda.current_stream().cuda_stream)
        x = torch.randn(n, dtype=torch.float64, device="cuda")
        y = torch.randn(m, dtype=torch.float64, device="cuda")
        spmv_acc_amd.prepare(m, n, nnz, rp, ci, v, x, beta=1.0)
        region = spmv_acc_amd.time_spmv_region(spmv_acc_amd.get_strategy(), 10, 1.0, 1.0, m, n, nnz, rp, ci, v, x, y)
        spmv_ms = float(np.median([region() for _ in range(7)])) / 10
        A = (rp, ci[:nnz].contiguous(), v[:nnz].contiguous())
        if m == n:
            rows.append(measure(lib, name, "A * A", [(m, n, n, A, A)], spmv_ms, ceiling, cap))
        else:  # a rectangular stand-in has no square: the normal-equations product on the device-made transpose instead
            T = spmv_acc_amd.csr_transpose(m, n, nnz, *A)
            rows.append(measure(lib, name, "A^T * A", [(n, m, n, T, A)], spmv_ms, ceiling, cap))
            del T
        # P: n x nc, one entry per row, column i // 8; R: mc x m, the same aggregation of the rows (R = P^T where m == n)
        nc, mc = (n + 7) // 8, (m + 7) // 8
        P = (torch.arange(n + 1, dtype=torch.int32, device="cuda"), (torch.arange(n, device="cuda") // 8).int(), torch.ones(n, dtype=torch.float64, device="cuda"))
        R = (torch.clamp(torch.arange(mc + 1, device="cuda") * 8, max=m).int(), torch.arange(m, dtype=torch.int32, device="cuda"),
             torch.ones(m, dtype=torch.float64, device="cuda"))
        rows.append(measure(lib, name, "R * (A * P), P 8 : 1", [(m, n, nc, A, P), lambda prev: (mc, prev[0], prev[1], R, prev[2])], spmv_ms, ceiling, cap))
        del P, R
        spmv_acc_amd.release_plans(rp)
        del rp, ci, v, x, y, A
        torch.cuda.empty_cache()
    doc = {"device": torch.cuda.get_device_name(0), "strategy": spmv_acc_amd.get_strategy(), "copy_ceiling_gbs": round(ceiling, 1), "rows": rows}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    if a.md:
        with open(a.md, "w") as f:
            f.write("# Device CSR SpGEMM: tools/spgemm_bench.py\n\n")
            f.write(f"{doc['device']}, strategy {doc['strategy']}, fp64; streaming-copy ceiling of this box in this run: {doc['copy_ceiling_gbs']} GB/s.  "
                    "Times in ms (medians; see the tool's docstring for each protocol).  `GB/s` = the bytes the values pass needs (24 B per product + "
                    "12 B per entry) / its time.  `range` = the rows of the left factor that were multiplied where the whole product count is beyond "
                    "the entry's limit.\n\n")
            f.write("| matrix | job | range | products | nnz(C) | csr_spgemm | in SpMVs | csr_spgemm_values | GB/s | in SpMVs | torch CSR @ CSR | "
                    "settled SpMV on A | differs from torch by | note |\n")
            f.write("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                tm = "-" if r["torch_ms"] is None else f"{r['torch_ms']:.2f}"
                ck = "-" if r["check"] is None else f"{r['check']:.1e}"
                f.write(f"| {r['matrix']} | {r['job']} | {r['range']} | {r['nprod']} | {r['nnz_c']} | {r['structure_ms']:.2f} | {r['structure_spmvs']:.0f} | "
                        f"{r['values_ms']:.3f} | {r['values_gbs']:.0f} | {r['values_spmvs']:.1f} | {tm} | {r['spmv_ms']:.4f} | {ck} | {r['torch_note'] or ''} |\n")


if __name__ == "__main__":
    main()
