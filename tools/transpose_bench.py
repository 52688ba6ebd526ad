#!/usr/bin/env python3
"""The transposed product's three routes on the bench's stand-ins (spmv_acc_csr_transpose, spmv_acc_csr_spmv_t).
One JSON line per matrix:
  transpose_ms   spmv_acc_csr_transpose with values and perm: median of 5 calls after one warm-up, host clock between device synchronisations (the
                 entry synchronises itself); transpose_spmvs = that time in settled SpMVs of the same matrix
  values_ms      spmv_acc_csr_transpose_values (one gather pass)
  spmv_ms        a settled spmv_acc_csr_spmv on A (spmv_acc_time_spmv_region, 10 calls per region, median of 7 regions), beta = 1
  spmv_at_ms     the same on the device-made A^T (an n x m matrix): what a caller who transposed once pays per product
  spmv_t_ms      spmv_acc_csr_spmv_t, beta = 1 (the scatter pass alone) and spmv_t_beta0_ms (scale + scatter): median of 7 regions of `reps`
                 back-to-back calls between one event pair, after one warm-up call
  atomic_tbs     8 B * nnz / spmv_t_ms: the added bytes per second of the atomic pass, beside the 1.3 TB/s MI355X adds at best (256 contiguous
                 bytes per wave instruction); floor_ms = 8 B * nnz / 1.3 TB/s
  breakeven      products after which transposing once is cheaper: transpose_ms / (spmv_t_ms - spmv_at_ms), or null where the atomic pass is not slower
  check          max scaled difference between the two routes' results at this size (relative to sum |a| |x| per output)
usage: tools/transpose_bench.py OUT.json [--matrices Hardesty3,boneS10,rmat22] [--md OUT.md]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spmv_acc_amd  # noqa: E402
from spmv_acc_amd import synth  # noqa: E402

ATOMIC_PEAK = 1.3e12  # bytes of fp adds per second, chip-wide, at the best access shape


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


def settled_spmv_ms(m, n, nnz, rp, ci, v, x, y):
    spmv_acc_amd.prepare(m, n, nnz, rp, ci, v, x, beta=1.0)
    region = spmv_acc_amd.time_spmv_region(spmv_acc_amd.get_strategy(), 10, 1.0, 1.0, m, n, nnz, rp, ci, v, x, y)
    return float(np.median([region() for _ in range(7)])) / 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--matrices", default="Hardesty3,boneS10,rmat22")
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    lib = spmv_acc_amd.load_library()
    rows = []
    for name in a.matrices.split(","):
        m, n, nnz, rp, ci, v = matrix(name)
        x = torch.randn(n, dtype=torch.float64, device="cuda")
        w = torch.randn(m, dtype=torch.float64, device="cuda")
        y = torch.randn(m, dtype=torch.float64, device="cuda")
        z = torch.randn(n, dtype=torch.float64, device="cuda")
        spmv_ms = settled_spmv_ms(m, n, nnz, rp, ci, v, x, y)
        # the transpose: one warm-up (code objects, the sort's first launch), then five timed calls
        t_rp, t_ci, t_v, perm = spmv_acc_amd.csr_transpose(m, n, nnz, rp, ci, v, want_perm=True)
        args = (m, n, nnz, rp.data_ptr(), ci.data_ptr(), v.data_ptr(), t_rp.data_ptr(), t_ci.data_ptr(), t_v.data_ptr(), perm.data_ptr())
        ts = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rc = lib.spmv_acc_csr_transpose(*args)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
            if rc != 0:
                raise SystemExit(lib.spmv_acc_last_error_string().decode())
        transpose_ms = float(np.median(ts))
        spmv_acc_amd.csr_transpose_values(perm, v, t_v)
        vargs = (nnz, perm.data_ptr(), v.data_ptr(), t_v.data_ptr())
        values_ms = median_region(lambda: lib.spmv_acc_csr_transpose_values(*vargs), reps=5)
        spmv_at_ms = settled_spmv_ms(n, m, nnz, t_rp, t_ci, t_v, w, z)
        # the stateless product
        spmv_acc_amd.csr_spmv_t(1.0, 1.0, m, n, nnz, rp, ci, v, w, z)  # warm-up; points the library stream at torch's
        t_ms = {}
        for beta in (1.0, 0.0):
            targs = (1.0, beta, m, n, nnz, rp.data_ptr(), ci.data_ptr(), v.data_ptr(), w.data_ptr(), z.data_ptr())
            t_ms[beta] = median_region(lambda: lib.spmv_acc_csr_spmv_t(*targs), reps=5)
        if lib.spmv_acc_last_error() != 0:
            raise SystemExit(lib.spmv_acc_last_error_string().decode())
        # the two routes agree at this size
        za, zb = torch.zeros_like(z), torch.zeros_like(z)
        spmv_acc_amd.csr_spmv_t(1.0, 0.0, m, n, nnz, rp, ci, v, w, za)
        spmv_acc_amd.csr_spmv(1.0, 0.0, n, m, nnz, t_rp, t_ci, t_v, w, zb)
        scale = torch.zeros_like(z)
        spmv_acc_amd.csr_spmv(1.0, 0.0, n, m, nnz, t_rp, t_ci, t_v.abs(), w.abs(), scale)
        torch.cuda.synchronize()
        live = scale > 0
        check = float(((za - zb).abs()[live] / scale[live]).max().item()) if bool(live.any()) else 0.0
        gap = t_ms[1.0] - spmv_at_ms
        row = {"matrix": name, "m": m, "n": n, "nnz": nnz, "spmv_ms": round(spmv_ms, 5), "spmv_at_ms": round(spmv_at_ms, 5),
               "transpose_ms": round(transpose_ms, 4), "transpose_spmvs": round(transpose_ms / spmv_ms, 1), "values_ms": round(values_ms, 5),
               "spmv_t_ms": round(t_ms[1.0], 5), "spmv_t_beta0_ms": round(t_ms[0.0], 5), "spmv_t_vs_spmv_at": round(t_ms[1.0] / spmv_at_ms, 2),
               "atomic_tbs": round(8.0 * nnz / (t_ms[1.0] * 1e-3) / 1e12, 3), "floor_ms": round(8.0 * nnz / ATOMIC_PEAK * 1e3, 5),
               "breakeven": round(transpose_ms / gap, 1) if gap > 0 else None, "check": check}
        print(json.dumps(row), flush=True)
        rows.append(row)
        spmv_acc_amd.release_plans(rp)
        spmv_acc_amd.release_plans(t_rp)
        del rp, ci, v, t_rp, t_ci, t_v, perm, x, w, y, z, za, zb, scale
        torch.cuda.empty_cache()
    doc = {"device": torch.cuda.get_device_name(0), "strategy": spmv_acc_amd.get_strategy(), "atomic_peak_tbs": ATOMIC_PEAK / 1e12, "rows": rows}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    if a.md:
        with open(a.md, "w") as f:
            f.write("# The transposed product: tools/transpose_bench.py\n\n")
            f.write(f"{doc['device']}, strategy {doc['strategy']}, fp64.  Times in ms (medians; see the tool's docstring for each protocol).  "
                    "`atomic TB/s` = 8 B x nnz / spmv_t time, beside the 1.3 TB/s the chip adds at its best access shape; `floor` = 8 B x nnz / 1.3 TB/s.\n\n")
            f.write("| matrix | m | n | nnz | SpMV A | SpMV on device-made A^T | csr_spmv_t (beta = 1) | csr_spmv_t (beta = 0) | spmv_t / SpMV A^T | atomic TB/s | floor | "
                    "csr_transpose | in SpMVs | transpose_values | break-even products | routes differ by |\n")
            f.write("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                f.write(f"| {r['matrix']} | {r['m']} | {r['n']} | {r['nnz']} | {r['spmv_ms']:.4f} | {r['spmv_at_ms']:.4f} | {r['spmv_t_ms']:.4f} | "
                        f"{r['spmv_t_beta0_ms']:.4f} | {r['spmv_t_vs_spmv_at']:.2f} | {r['atomic_tbs']:.3f} | {r['floor_ms']:.4f} | {r['transpose_ms']:.3f} | "
                        f"{r['transpose_spmvs']:.1f} | {r['values_ms']:.4f} | {r['breakeven']} | {r['check']:.2e} |\n")


if __name__ == "__main__":
    main()
