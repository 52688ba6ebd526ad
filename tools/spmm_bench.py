#!/usr/bin/env python3
"""CSR SpMM against k SpMV calls (spmv_acc_csr_spmm).  One JSON line per (matrix, k, layout, beta class):
  ms         median of 7 regions, each `reps` back-to-back SpMM calls between one event pair (after one warm-up call), per call
  gflops     2 * nnz * k / time
  b_alg      12 nnz + 4 (m + 1) + 8 k n + 16 k m bytes (8 k m at beta = 0): the SpMV's algorithmic bytes with k vectors
  frac       b_alg / time / 8 TB/s
  vs_k_spmv  this time / the time of k SpMV calls on the settled SpMV plan (spmv_acc_time_spmv_region, same process, same region rule)
usage: tools/spmm_bench.py OUT.json [--matrices boneS10,Hardesty3,...,rmat22] [--ks 1,2,4,8,16,32] [--layouts row,col] [--betas 0,1]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spmv_acc_amd  # noqa: E402
from spmv_acc_amd import synth  # noqa: E402

PEAK = 8e12


def matrix(name):
    if name.startswith("rmat"):
        return synth.rmat_torch(int(name[4:]))
    return synth.sweep_standin_torch(name)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--matrices", default="Hardesty3,boneS10,Bump_2911,dielFilterV3real,af_shell10,rmat22")
    ap.add_argument("--ks", default="1,2,4,8,16,32")
    ap.add_argument("--layouts", default="row,col")
    ap.add_argument("--betas", default="0,1")
    a = ap.parse_args()
    lib = spmv_acc_amd.load_library()
    rows = []
    for name in a.matrices.split(","):
        m, n, nnz, rp, ci, v = matrix(name)
        kmax = max(int(k) for k in a.ks.split(","))
        x = torch.randn(n, dtype=torch.float64, device="cuda")
        y = torch.randn(m, dtype=torch.float64, device="cuda")
        spmv_ms = {}
        for beta in (float(b) for b in a.betas.split(",")):
            spmv_acc_amd.prepare(m, n, nnz, rp, ci, v, x, beta=beta)
            region = spmv_acc_amd.time_spmv_region(spmv_acc_amd.get_strategy(), 10, 1.0, beta, m, n, nnz, rp, ci, v, x, y)
            spmv_ms[beta] = float(np.median([region() for _ in range(7)])) / 10
        for layout in a.layouts.split(","):
            Xb = torch.randn((n, kmax) if layout == "row" else (kmax, n), dtype=torch.float64, device="cuda")
            Yb = torch.randn((m, kmax) if layout == "row" else (kmax, m), dtype=torch.float64, device="cuda")
            for k in (int(s) for s in a.ks.split(",")):
                X = Xb[:, :k] if layout == "row" else Xb[:k].t()
                Y = Yb[:, :k] if layout == "row" else Yb[:k].t()
                ldx, ldy = (kmax, kmax) if layout == "row" else (n, m)
                for beta in (float(b) for b in a.betas.split(",")):
                    spmv_acc_amd.csr_spmm(1.0, beta, m, n, nnz, rp, ci, v, X, Y)  # warm-up, builds the SpMM section, sets the stream
                    args = (0 if layout == "row" else 1, k, 1.0, beta, m, n, nnz, None, rp.data_ptr(), ci.data_ptr(), v.data_ptr(), X.data_ptr(),
                            ldx, Y.data_ptr(), ldy)
                    ms = median_region(lambda: lib.spmv_acc_csr_spmm(*args), reps=5)
                    if lib.spmv_acc_last_error() != 0:
                        raise SystemExit(lib.spmv_acc_last_error_string().decode())
                    b_alg = 12 * nnz + 4 * (m + 1) + 8 * k * n + (16 if beta else 8) * k * m
                    row = {"matrix": name, "m": m, "n": n, "nnz": nnz, "k": k, "layout": layout, "beta": beta, "ms": round(ms, 5),
                           "gflops": round(2 * nnz * k / ms / 1e6, 1), "b_alg": b_alg, "frac": round(b_alg / (ms * 1e-3) / PEAK, 3),
                           "spmv_ms": round(spmv_ms[beta], 5), "vs_k_spmv": round(ms / (k * spmv_ms[beta]), 3)}
                    print(json.dumps(row), flush=True)
                    rows.append(row)
        spmv_acc_amd.release_plans(rp)
        del rp, ci, v, Xb, Yb
        torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "strategy": spmv_acc_amd.get_strategy(), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
