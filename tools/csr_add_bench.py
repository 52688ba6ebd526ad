#!/usr/bin/env python3
"""The device CSR sparse add (spmv_acc_csr_add, spmv_acc_csr_add_values) on the bench's stand-ins.  Every stand-in is first made canonical
(rows strictly ascending, duplicates merged) by spmv_acc_coo_to_csr, outside every timing.  Per matrix A three jobs, all with alpha = 1:
  A + A^T         the symmetrisation, A^T from spmv_acc_csr_transpose (square stand-ins only): partial overlap
  M + dt K        two matrices on A's pattern with different values, beta = dt = 0.01: every entry matched -- the time-stepping job
  A + sigma I     B = the m x n identity pattern (min(m, n) entries), beta = sigma = 0.5: a shift
One JSON line per job:
  nnz_a, nnz_b, nnz_c
  structure_ms     spmv_acc_csr_add with values and map: median of 3 calls after one warm-up, host clock between device synchronisations (the
                   entry synchronises itself); structure_spmvs = that time in settled SpMVs of A
  values_ms        spmv_acc_csr_add_values: median of 7 regions of 5 back-to-back calls between one event pair, after one warm-up
  values_gbs       the bytes the pass NEEDS per second: 8 B of map per C entry, 8 B per present operand, 8 B stored
  values_of_copy   values_gbs / copy_ceiling_gbs: the yardstick of the values pass
  torch_ms         torch.add on sparse-CSR tensors (structure and values in one step, no kept map), median of 3 after one warm-up; where torch
                   refuses CSR: COO add + coalesce, with the reason in torch_note
  spmv_ms          a settled spmv_acc_csr_spmv on A (spmv_acc_time_spmv_region, 10 calls per region, median of 7 regions), beta = 1: the unit
  copy_ceiling_gbs spmv_acc_copy_ceiling_gbs on this box in this run (1 GiB)
  check            the values against torch's where the patterns agree, max difference relative to |a| + |beta b|, entrywise
usage: tools/csr_add_bench.py OUT.json [--matrices Hardesty3,boneS10,Ga41As41H72] [--md OUT.md]"""
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


class Sum:
    """One C = alpha * A + beta * B with arrays kept for the values pass."""

    def __init__(self, lib, m, n, a, b, alpha, beta):
        self.lib, self.m, self.n, self.a, self.b, self.alpha, self.beta = lib, m, n, a, b, alpha, beta
        cap = a[1].numel() + b[1].numel()
        self.rp = torch.empty(m + 1, dtype=torch.int32, device="cuda")
        self.ci = torch.empty(cap, dtype=torch.int32, device="cuda")
        self.v = torch.empty(cap, dtype=torch.float64, device="cuda")
        self.ia, self.ib = torch.empty(cap, dtype=torch.int32, device="cuda"), torch.empty(cap, dtype=torch.int32, device="cuda")
        self.h = ctypes.c_int(0)
        self.nnz = 0

    def structure(self):
        a, b = self.a, self.b
        rc = self.lib.spmv_acc_csr_add(self.m, self.n, a[1].numel(), a[0].data_ptr(), a[1].data_ptr(), b[1].numel(), b[0].data_ptr(), b[1].data_ptr(),
                                       self.alpha, a[2].data_ptr(), self.beta, b[2].data_ptr(), self.rp.data_ptr(), self.ci.data_ptr(),
                                       self.v.data_ptr(), self.ia.data_ptr(), self.ib.data_ptr(), ctypes.byref(self.h))
        if rc != 0:
            raise SystemExit(self.lib.spmv_acc_last_error_string().decode())
        self.nnz = int(self.h.value)

    def values(self):
        self.lib.spmv_acc_csr_add_values(self.nnz, self.a[2].numel(), self.b[2].numel(), self.ia.data_ptr(), self.ib.data_ptr(), self.alpha,
                                         self.a[2].data_ptr(), self.beta, self.b[2].data_ptr(), self.v.data_ptr())

    def needed_bytes(self):
        return 16.0 * self.nnz + 8.0 * (self.a[1].numel() + self.b[1].numel())  # (every non-zero of A and of B is present in exactly one entry)


def torch_csr(m, n, a):
    return torch.sparse_csr_tensor(a[0], a[1], a[2], size=(m, n))


def measure(lib, name, job, m, n, a, b, beta, spmv_ms, ceiling):
    s = Sum(lib, m, n, a, b, 1.0, beta)
    print(f"# {name}: {job}: {m} x {n}, {a[1].numel()} + {b[1].numel()} non-zeros", file=sys.stderr, flush=True)
    structure_ms = median_host(s.structure)
    s.values()
    values_ms = median_region(s.values, reps=5)
    if lib.spmv_acc_last_error() != 0:
        raise SystemExit(lib.spmv_acc_last_error_string().decode())
    torch_ms, check, why, tv = None, None, None, None
    try:
        ta, tb = torch_csr(m, n, a), torch_csr(m, n, b)
        torch_ms = median_host(lambda: torch.add(ta, tb, alpha=beta))
        tv = torch.add(ta, tb, alpha=beta).values()
    except Exception as e:  # noqa: BLE001 -- torch refusing the CSR sum is a result of the comparison, not an error of the tool
        why = f"CSR refused ({type(e).__name__}: {str(e).splitlines()[0][:120]}); COO add + coalesce instead"
        try:
            ca, cb = torch_csr(m, n, a).to_sparse_coo(), torch_csr(m, n, b).to_sparse_coo()
            torch_ms = median_host(lambda: torch.add(ca, cb, alpha=beta).coalesce())
            tv = torch.add(ca, cb, alpha=beta).coalesce().values()
        except Exception as e2:  # noqa: BLE001
            why += f"; COO refused too ({type(e2).__name__}: {str(e2).splitlines()[0][:120]})"
    if tv is not None:
        if tv.numel() == s.nnz:
            scale = Sum(lib, m, n, (a[0], a[1], a[2].abs()), (b[0], b[1], b[2].abs()), 1.0, abs(beta))
            scale.structure()
            check = float(((tv - s.v[:s.nnz]).abs() / scale.v[:s.nnz].clamp_min(1e-300)).max().item())
        else:
            why = (why + "; " if why else "") + f"torch returns {tv.numel()} entries"
    gbs = s.needed_bytes() / (values_ms * 1e-3) / 1e9
    r = {"matrix": name, "job": job, "nnz_a": a[1].numel(), "nnz_b": b[1].numel(), "nnz_c": s.nnz, "structure_ms": round(structure_ms, 3),
         "structure_spmvs": round(structure_ms / spmv_ms, 1), "values_ms": round(values_ms, 4), "values_gbs": round(gbs, 1),
         "values_of_copy": round(gbs / ceiling, 3), "values_spmvs": round(values_ms / spmv_ms, 1),
         "torch_ms": None if torch_ms is None else round(torch_ms, 3), "torch_note": why, "spmv_ms": round(spmv_ms, 5),
         "copy_ceiling_gbs": round(ceiling, 1), "check": check}
    print(json.dumps(r), flush=True)
    del s
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--matrices", default="Hardesty3,boneS10,Ga41As41H72")
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    lib = spmv_acc_amd.load_library()
    src = torch.empty(1 << 27, dtype=torch.float64, device="cuda").normal_()
    dst = torch.empty_like(src)
    ceiling = spmv_acc_amd.copy_ceiling_gbs(dst, src, reps=5)
    del src, dst
    rows = []
    for name in a.matrices.split(","):
        m, n, nnz, rp, ci, v = synth.sweep_standin_torch(name)
        lib.spmv_acc_set_stream(torch.cuda.current_stream().cuda_stream)
        row = torch.repeat_interleave(torch.arange(m, dtype=torch.int32, device="cuda"), (rp[1:] - rp[:-1]).long())
        A = spmv_acc_amd.coo_to_csr(m, n, row, ci[:nnz].contiguous(), v[:nnz].contiguous())  # canonical: sorted rows, duplicates merged
        del row, rp, ci, v
        nnz = A[1].numel()
        x = torch.randn(n, dtype=torch.float64, device="cuda")
        y = torch.randn(m, dtype=torch.float64, device="cuda")
        spmv_acc_amd.prepare(m, n, nnz, *A, x, beta=1.0)
        region = spmv_acc_amd.time_spmv_region(spmv_acc_amd.get_strategy(), 10, 1.0, 1.0, m, n, nnz, *A, x, y)
        spmv_ms = float(np.median([region() for _ in range(7)])) / 10
        if m == n:
            T = spmv_acc_amd.csr_transpose(m, n, nnz, *A)
            rows.append(measure(lib, name, "A + A^T", m, n, A, T, 1.0, spmv_ms, ceiling))
            del T
        K = (A[0], A[1], torch.randn(nnz, dtype=torch.float64, device="cuda"))
        rows.append(measure(lib, name, "M + dt K", m, n, A, K, 0.01, spmv_ms, ceiling))
        del K
        d = min(m, n)
        eye = (torch.clamp(torch.arange(m + 1, device="cuda"), max=d).int(), torch.arange(d, dtype=torch.int32, device="cuda"),
               torch.ones(d, dtype=torch.float64, device="cuda"))
        rows.append(measure(lib, name, "A + sigma I", m, n, A, eye, 0.5, spmv_ms, ceiling))
        del eye
        spmv_acc_amd.release_plans(A[0])
        del x, y, A
        torch.cuda.empty_cache()
    doc = {"device": torch.cuda.get_device_name(0), "strategy": spmv_acc_amd.get_strategy(), "copy_ceiling_gbs": round(ceiling, 1), "rows": rows}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    if a.md:
        with open(a.md, "w") as f:
            f.write("# Device CSR sparse add: tools/csr_add_bench.py\n\n")
            f.write(f"{doc['device']}, strategy {doc['strategy']}, fp64; streaming-copy ceiling of this box in this run: {doc['copy_ceiling_gbs']} GB/s.  "
                    "Times in ms (medians; see the tool's docstring for each protocol).  `GB/s` = the bytes the values pass needs (8 B of map + 8 B "
                    "stored per entry, 8 B per present operand) / its time; `of copy` = that rate relative to the copy ceiling.  alpha = 1 in every "
                    "job.\n\n")
            f.write("| matrix | job | nnz(A) | nnz(B) | nnz(C) | csr_add | in SpMVs | csr_add_values | GB/s | of copy | in SpMVs | torch add | "
                    "settled SpMV on A | differs from torch by | note |\n")
            f.write("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                tm = "-" if r["torch_ms"] is None else f"{r['torch_ms']:.2f}"
                ck = "-" if r["check"] is None else f"{r['check']:.1e}"
                f.write(f"| {r['matrix']} | {r['job']} | {r['nnz_a']} | {r['nnz_b']} | {r['nnz_c']} | {r['structure_ms']:.2f} | {r['structure_spmvs']:.0f} | "
                        f"{r['values_ms']:.3f} | {r['values_gbs']:.0f} | {r['values_of_copy']:.2f} | {r['values_spmvs']:.1f} | {tm} | {r['spmv_ms']:.4f} | {ck} | "
                        f"{r['torch_note'] or ''} |\n")


if __name__ == "__main__":
    main()
