"""CPU check of the row-block kernel's 8-bit column body (round 7; tile_stage.hpp stage_products_c16_all<..., 8>), from hipcc's assembly for gfx950.

test_host_logic.py::test_row_block_kernel_instances_fit_eight_waves_per_simd passes when ANY body of an instance shows the all-steps wait sequence;
an instance that reads the column encoding now holds two such bodies, one per code width.  Here each is found by the stream loads in front of its
first wait -- 8-bit: two record loads and two 4-B code loads (four global_load_dword), 16-bit: two record loads and two 8-B code loads -- and each
must show s_waitcnt vmcnt(5) (first step's record and codes back, five later stream loads in flight), the step's four gathers, then vmcnt(8)."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bodies(lines):
    """(loads in front, wait sequence held) for every s_waitcnt vmcnt(5) of one kernel: the last eight stream loads before it, and whether four
    gathers follow before s_waitcnt vmcnt(8)."""
    out = []
    for i, ln in enumerate(lines):
        if "s_waitcnt vmcnt(5)" not in ln:
            continue
        gathers, ok = 0, False
        for nxt in lines[i + 1:i + 300]:
            if re.search(r"global_load_dwordx2 [^\n]*, s\[", nxt):
                gathers += 1
            elif "s_waitcnt vmcnt(8)" in nxt:
                ok = gathers == 4
                break
            elif "s_waitcnt vmcnt(" in nxt and gathers:
                break
        loads = [re.match(r"\s*global_load_(\w+)", l).group(1) for l in lines[max(0, i - 200):i] if re.match(r"\s*global_load_\w+", l)][-8:]
        out.append((" ".join(loads), ok))
    return out


def test_8_bit_body_keeps_the_all_steps_waits(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_table

    csrc = os.path.join(ROOT, "spmv_acc_amd", "csrc")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-DKERNEL_STRATEGY_ADAPTIVE", "-I" + os.path.join(ROOT, "include"),
                        "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-S", os.path.join(csrc, "k_rowblock.hip"), "-o", str(tmp_path / "k_rowblock.s")],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [k for k in resource_table.parse(r.stderr) if k["name"].startswith("rowblock_stream_kernel<")]
    asm = open(tmp_path / "k_rowblock.s").read()
    eight = "dword dword dword dword dwordx4 dwordx4 dwordx4 dwordx4"
    sixteen = "dword dword dwordx2 dwordx2 dwordx4 dwordx4 dwordx4 dwordx4"
    checked = 0
    for k in rows:
        args = [a.strip() for a in k["name"][len("rowblock_stream_kernel<"):-1].split(",")]
        if args[5] != "true":
            continue  # (instances that read colindex only)
        assert k["vgprs"] <= 64 and k["occupancy"] >= 8 and k["scratch"] == 0, k
        body = asm[asm.index("\n" + k["mangled"] + ":"):]
        body = body[:body.index("s_endpgm")]
        found = _bodies(body.split("\n"))
        for want in (eight, sixteen):
            hits = [ok for loads, ok in found if loads == want]
            assert hits and all(hits), (k["name"], want, found)
        checked += 1
    assert checked >= 30, checked
