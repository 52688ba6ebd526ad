#!/usr/bin/env python3
"""The device CSR extraction (spmv_acc_csr_extract, spmv_acc_csr_extract_values) on the bench's stand-ins.  Every stand-in is first made
canonical (rows strictly ascending, duplicates merged) by spmv_acc_coo_to_csr, outside every timing.  Per matrix A three structure jobs:
  permutation     C[i, j] = A[p[i], q[j]] for random permutations p of the rows and q of the columns -- the symmetric P A P^T (q = p) on a
                  square stand-in, two independent ones on a rectangular one: the compaction descends, so the radix sort runs
  strict lower    diag_lo = INT_MIN, diag_hi = -1 on the unmapped matrix: no sort
  block           the contiguous rows [m/4, 3m/4) and columns [n/4, 3n/4), renumbered from 0: no sort
and the values pass on the map of the permutation (a permuted map: every missed gather is a whole memory request) and on the map of the strict
lower triangle (a monotone map).  One JSON line per job:
  nnz_a, nnz_c
  structure_ms     spmv_acc_csr_extract with values and map: median of 3 calls after one warm-up, host clock between device synchronisations
                   (the entry synchronises itself); structure_spmvs = that time in settled SpMVs of A
  sorted           whether the entry took the sort path: the compaction, recomputed with torch, descends inside a row
  torch_ms         the plain torch composition a user would write today -- expand the selected rows, gather and map the columns, mask, one
                   stable sort of row * nc + column, bincount and cumsum for the row pointer, two gathers for values and map -- median of 3
                   after one warm-up; torch_equal = its row pointer, columns, map and value bits equal the entry's
  values_ms        spmv_acc_csr_extract_values: median of 7 regions of 5 back-to-back calls between one event pair, after one warm-up
  values_gbs       the bytes the pass NEEDS per second: 4 B of map, 8 B gathered and 8 B stored per C entry = 20 B
  values_of_copy   values_gbs / copy_ceiling_gbs: the yardstick of the values pass
  index_select_ms  torch.index_select(a_value, 0, map) into a preallocated tensor, same protocol as values_ms
  spmv_ms          a settled spmv_acc_csr_spmv on A (spmv_acc_time_spmv_region, 10 calls per region, median of 7 regions), beta = 1: the unit
  copy_ceiling_gbs spmv_acc_copy_ceiling_gbs on this box in this run (1 GiB)
Every matrix runs in a child process of its own under a time limit; after a child that fails or runs out of time nothing more is started.
usage: tools/extract_bench.py OUT.json [--matrices Hardesty3,boneS10] [--md OUT.md] [--limit SECONDS]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def child(name):
    import numpy as np
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import spmv_acc_amd
    from spmv_acc_amd import synth

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

    lib = spmv_acc_amd.load_library()
    src = torch.empty(1 << 27, dtype=torch.float64, device="cuda").normal_()
    dst = torch.empty_like(src)
    ceiling = spmv_acc_amd.copy_ceiling_gbs(dst, src, reps=5)
    del src, dst
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
    spmv_acc_amd.release_plans(A[0])
    del x, y

    class Extraction:
        """One C = A[rows, colmap] in a band with arrays kept for the values pass."""

        def __init__(self, rows, colmap, nc, lo, hi):
            self.rows, self.colmap, self.nc, self.lo, self.hi = rows, colmap, nc, lo, hi
            self.mc = m if rows is None else rows.numel()
            self.rp = torch.empty(self.mc + 1, dtype=torch.int32, device="cuda")
            self.ci = torch.empty(nnz, dtype=torch.int32, device="cuda")
            self.v = torch.empty(nnz, dtype=torch.float64, device="cuda")
            self.map = torch.empty(nnz, dtype=torch.int32, device="cuda")
            self.h = ctypes.c_int(0)
            self.nnz = 0

        def structure(self):
            rc = lib.spmv_acc_csr_extract(m, n, nnz, A[0].data_ptr(), A[1].data_ptr(), A[2].data_ptr(), self.mc,
                                          None if self.rows is None else self.rows.data_ptr(), self.nc,
                                          None if self.colmap is None else self.colmap.data_ptr(), self.lo, self.hi, self.rp.data_ptr(),
                                          self.ci.data_ptr(), self.v.data_ptr(), self.map.data_ptr(), ctypes.byref(self.h))
            if rc != 0:
                raise SystemExit(lib.spmv_acc_last_error_string().decode())
            self.nnz = int(self.h.value)

        def values(self):
            lib.spmv_acc_csr_extract_values(self.nnz, nnz, self.map.data_ptr(), A[2].data_ptr(), self.v.data_ptr())

        def torch_composition(self):
            """what a user writes today: returns (rowptr, colindex, value, map, descents of the compaction)"""
            rows = torch.arange(m, device="cuda") if self.rows is None else self.rows.long()
            start = A[0][rows].long()
            lens = A[0][rows + 1].long() - start
            i = torch.repeat_interleave(torch.arange(self.mc, device="cuda"), lens)
            first = torch.cumsum(lens, 0) - lens
            q = start[i] + torch.arange(i.numel(), device="cuda") - first[i]
            j = A[1][q].long()
            if self.colmap is not None:
                j = self.colmap[j].long()
            keep = (j >= 0) & (j - i >= self.lo) & (j - i <= self.hi)
            i, q, j = i[keep], q[keep], j[keep]
            order = torch.argsort(i * self.nc + j, stable=True)
            c_rp = torch.zeros(self.mc + 1, dtype=torch.int64, device="cuda")
            torch.cumsum(torch.bincount(i, minlength=self.mc), 0, out=c_rp[1:])
            cmap = q[order]
            down = int(((j[1:] < j[:-1]) & (i[1:] == i[:-1])).sum().item()) if j.numel() > 1 else 0
            return c_rp.int(), j[order].int(), A[2][cmap], cmap.int(), down

    def measure(job, e):
        print(f"# {name}: {job}: {m} x {n}, {nnz} non-zeros", file=sys.stderr, flush=True)
        structure_ms = median_host(e.structure)
        torch_ms = median_host(e.torch_composition)
        t_rp, t_ci, t_v, t_map, down = e.torch_composition()
        k = e.nnz
        equal = bool(t_ci.numel() == k and torch.equal(t_rp, e.rp) and torch.equal(t_ci, e.ci[:k]) and torch.equal(t_map, e.map[:k])
                     and torch.equal(t_v.view(torch.int64), e.v[:k].view(torch.int64)))
        del t_rp, t_ci, t_v, t_map
        torch.cuda.empty_cache()
        r = {"matrix": name, "job": job, "m": m, "n": n, "nnz_a": nnz, "mc": e.mc, "nc": e.nc, "nnz_c": k, "sorted": down > 0,
             "structure_ms": round(structure_ms, 3), "structure_spmvs": round(structure_ms / spmv_ms, 1), "torch_ms": round(torch_ms, 3),
             "torch_equal": equal, "spmv_ms": round(spmv_ms, 5), "copy_ceiling_gbs": round(ceiling, 1)}
        return r

    def measure_values(r, e):
        e.values()
        values_ms = median_region(e.values, reps=5)
        if lib.spmv_acc_last_error() != 0:
            raise SystemExit(lib.spmv_acc_last_error_string().decode())
        cmap, out = e.map[:e.nnz], torch.empty(e.nnz, dtype=torch.float64, device="cuda")
        torch.index_select(A[2], 0, cmap, out=out)
        select_ms = median_region(lambda: torch.index_select(A[2], 0, cmap, out=out), reps=5)
        same = bool(torch.equal(out.view(torch.int64), e.v[:e.nnz].view(torch.int64)))
        gbs = 20.0 * e.nnz / (values_ms * 1e-3) / 1e9
        r.update(values_ms=round(values_ms, 4), values_gbs=round(gbs, 1), values_of_copy=round(gbs / ceiling, 3),
                 values_spmvs=round(values_ms / spmv_ms, 1), index_select_ms=round(select_ms, 4), index_select_equal=same)

    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    p = torch.randperm(m, generator=g, device="cuda").int()
    qperm = p if m == n else torch.randperm(n, generator=g, device="cuda").int()
    inverse = torch.empty(n, dtype=torch.int32, device="cuda")
    inverse[qperm.long()] = torch.arange(n, dtype=torch.int32, device="cuda")
    jobs = (("permutation" + ("" if m == n else " (rows and columns apart)"), Extraction(p, inverse, n, INT_MIN, INT_MAX), True),
            ("strict lower", Extraction(None, None, n, INT_MIN, -1), True),
            ("block", Extraction(torch.arange(m // 4, 3 * m // 4, dtype=torch.int32, device="cuda"),
                                 torch.where((torch.arange(n, device="cuda") >= n // 4) & (torch.arange(n, device="cuda") < 3 * n // 4),
                                             torch.arange(n, device="cuda") - n // 4, -1).int(), 3 * n // 4 - n // 4, INT_MIN, INT_MAX), False))
    for job, e, with_values in jobs:
        r = measure(job, e)
        if with_values:
            measure_values(r, e)
        print(json.dumps(r), flush=True)
        del e
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--matrices", default="Hardesty3,boneS10")
    ap.add_argument("--md", default=None)
    ap.add_argument("--limit", type=int, default=420, help="seconds a matrix may take")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child)
        return
    rows, device = [], None
    for name in a.matrices.split(","):  # (this process never opens the GPU: one child per matrix, each under its own limit)
        try:
            done = subprocess.run([sys.executable, os.path.abspath(__file__), a.out, "--child", name], stdout=subprocess.PIPE, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"{name}: no result within {a.limit} s; nothing more is started")
        if done.returncode != 0:
            raise SystemExit(f"{name}: the child ended with {done.returncode}; nothing more is started")
        rows += [json.loads(ln) for ln in done.stdout.splitlines() if ln.startswith("{")]
    doc = {"copy_ceiling_gbs": rows[0]["copy_ceiling_gbs"] if rows else None, "rows": rows}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    if a.md:
        with open(a.md, "w") as f:
            f.write("# Device CSR extraction: tools/extract_bench.py\n\n")
            f.write("MI355X, fp64; the streaming-copy ceiling of the box is measured in every matrix' run (column `copy`, GB/s).  Times in ms (medians; "
                    "see the tool's docstring for each protocol).  `torch` = the composition a user would write today (expand rows, map, mask, "
                    "stable sort of the keys, bincount); `same` = its result equals the entry's bit for bit.  `GB/s` = 20 B per C entry (4 B of map, "
                    "8 B gathered, 8 B stored) / the time of the values pass; `of copy` = that rate relative to the copy ceiling; `index_select` = "
                    "torch.index_select(a_value, 0, map) into a preallocated tensor.\n\n")
            f.write("| matrix | job | nnz(A) | rows of C | nnz(C) | sort | csr_extract | in SpMVs | torch | same | csr_extract_values | GB/s | of copy | "
                    "in SpMVs | index_select | settled SpMV on A | copy |\n")
            f.write("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                vals = (f"{r['values_ms']:.3f} | {r['values_gbs']:.0f} | {r['values_of_copy']:.2f} | {r['values_spmvs']:.1f} | {r['index_select_ms']:.3f}"
                        if "values_ms" in r else "- | - | - | - | -")
                f.write(f"| {r['matrix']} | {r['job']} | {r['nnz_a']} | {r['mc']} | {r['nnz_c']} | {'yes' if r['sorted'] else 'no'} | "
                        f"{r['structure_ms']:.2f} | {r['structure_spmvs']:.0f} | {r['torch_ms']:.2f} | {'yes' if r['torch_equal'] else 'NO'} | {vals} | "
                        f"{r['spmv_ms']:.4f} | {r['copy_ceiling_gbs']:.0f} |\n")


if __name__ == "__main__":
    main()
