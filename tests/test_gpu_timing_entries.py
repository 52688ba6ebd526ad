"""GPU suite (-m gpu): what the TIMING ENTRIES leave behind -- spmv_acc_time_spmv / _events / _cold / _total / _kernels / _region and
spmv_acc_copy_ceiling_gbs (include/spmv_acc.h, "measurement helper"; spmv_acc_amd/csrc/c_api.cpp).  Every published figure is read from them, and a y
reset that did not happen, or a flush copy that writes where it should not, changes a figure without failing anything.  Pinned here:
  * the y each entry leaves: bit for bit what plain calls on the settled plan give, and within the project's gate (scaled error <= 1e-12,
    tests/test_gpu_parity.py) of the CPU oracle -- y is pre-filled with NaN, so a reset that did not happen shows;
  * every form of the reset: the 16-byte copy kernel, its one-workgroup tail for the last double of an odd m (m = 4097, 3, 1), hipMemcpyAsync where
    y or y0 sits at 8 mod 16 (and, in the kernel-clock entry, for every odd m); SPMV_ACC_RESET_MEMCPY / SPMV_ACC_RESET_NT in fresh processes;
  * d_y0 == NULL: the launches accumulate; spmv_acc_time_spmv_total / _region likewise; the region entry's "the plan was not settled" refusal;
  * the cold entry's flush copy, byte by byte, and its refusals; the copy ceiling's copy, byte by byte, and its refusals;
  * bad arguments: nothing is written, neither to y nor to a result;
  * what nobody may touch: y0, x, the matrix, and 8 guard doubles of 7.25 either side of y and y0.
No duration is compared with another or with a constant: times are finite and positive (and the kernel clock reads at most the event pair around
it, as tests/test_gpu_size_rules_and_timing.py already holds); medians are printed for the log.  tests/timing_entries.py is the registry the CPU suite
checks: an entry or a reset form that is rewritten has to re-register the tests that cross it."""
import ctypes
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import spmv_acc_amd
from spmv_acc_amd import synth

pytestmark = pytest.mark.gpu

SCALED_TOL = 1e-12  # tests/test_gpu_parity.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, PAD = 8, 7.25
FENCE = spmv_acc_amd.EVENT_DISABLE_SYSTEM_FENCE
ALPHA_BETA = ((1.0, 1.0), (0.5, -2.0), (1.0, 0.0))
SHIFTS = {"aligned": (0, 0), "y at 8 mod 16": (1, 0), "y0 at 8 mod 16": (0, 1), "both at 8 mod 16": (1, 1)}  # (y, y0) in doubles off a 16-byte line
ROWS = (4097, 4096, 1, 2, 3)  # odd: body + 8-byte tail; no tail; nothing but the tail; exactly one 16-byte unit; one unit + tail
BAD_ARGUMENT, UNKNOWN_STRATEGY = 2, 5  # enum spmv_acc_error

# entry -> C symbol (the per-launch protocol four times, then the two accumulating regions)
ENTRY_SYMBOLS = {"time_spmv": "spmv_acc_time_spmv", "events_fence": "spmv_acc_time_spmv_events", "cold": "spmv_acc_time_spmv_cold",
                 "kernels": "spmv_acc_time_spmv_kernels", "total": "spmv_acc_time_spmv_total", "region": "spmv_acc_time_spmv_region",
                 "copy_ceiling": "spmv_acc_copy_ceiling_gbs"}
PER_LAUNCH = ("time_spmv", "events_fence", "cold", "kernels")
TUNABLES = {"line_enhance": {}, "flat": {"flat_rowblock": 0, "flat_finish": 0}, "adaptive": {}}  # flat: its own tile kernel plus the fix-up


@pytest.fixture(scope="module")
def torch_dev(hiplib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the host arrays are shared among the tests and read-only)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def same_bits(t, a):
    return np.array_equal(t.cpu().numpy().view(np.int64), np.ascontiguousarray(a, dtype=np.float64).view(np.int64))


# ---- inputs, computed once -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_case(m):
    """(rowptr, cols, vals, x, y0) with n = m + 3; the three tiny matrices by hand, one or two non-zeros per row; arrays are never written"""
    n = m + 3
    if m == 1:
        rowptr, cols, vals = [0, 2], [0, 3], [1.5, -0.25]
    elif m == 2:
        rowptr, cols, vals = [0, 1, 3], [4, 0, 2], [-2.0, 0.75, 3.0]
    elif m == 3:
        rowptr, cols, vals = [0, 2, 3, 5], [1, 5, 0, 2, 3], [0.5, -1.25, 2.0, -0.375, 4.0]
    else:
        rowptr, cols, vals = synth.random_csr(m, n, 9, seed=31 + m, kind="uniform")
    rng = np.random.default_rng(1000 + m)
    out = (np.asarray(rowptr, dtype=np.int32), np.asarray(cols, dtype=np.int32), np.asarray(vals, dtype=np.float64), rng.standard_normal(n),
           rng.standard_normal(m))
    for a in out:
        a.setflags(write=False)
    return out


_REFS = {}


def reference(oracle, m, alpha, beta, steps):
    """y after `steps` applications of y <- alpha A x + beta y from y0 (the sequential CPU oracle), and the scale of its error: the magnitude of the
    terms that were added, carried through the steps (s_k = |alpha| |A| |x| + |beta| s_(k-1), s_0 = |y0|) -- one step: oracle.scaled_error's scale"""
    key = (m, alpha, beta, steps)
    if key not in _REFS:
        rowptr, cols, vals, x, y0 = host_case(m)
        mag = oracle.host_spmv(1.0, 0.0, rowptr, cols, np.abs(vals), np.abs(x), np.zeros(m))
        y, scale = y0.copy(), np.abs(y0)
        for _ in range(steps):
            y = oracle.host_spmv(alpha, beta, rowptr, cols, vals, x, y)
            scale = abs(alpha) * mag + abs(beta) * scale
        y.setflags(write=False)
        scale.setflags(write=False)
        _REFS[key] = (y, scale)
    return _REFS[key]


def scaled_error(got, ref, scale):
    diff = np.abs(got - ref)
    zero = scale == 0
    if np.any(diff[zero] != 0) or not np.all(np.isfinite(got)):
        return np.inf
    return float(np.max(diff[~zero] / scale[~zero])) if np.any(~zero) else 0.0


class Case:
    """one matrix and its vectors on the device"""

    def __init__(self, torch, m):
        self.m, self.n = m, m + 3
        self.host = host_case(m)
        self.nnz = int(self.host[0][-1])
        self.rowptr, self.cols, self.vals, self.x, self.y0 = (dev(torch, a) for a in self.host)

    def inputs_unchanged(self):
        rowptr, cols, vals, x, y0 = self.host
        return (np.array_equal(self.rowptr.cpu().numpy(), rowptr) and np.array_equal(self.cols.cpu().numpy(), cols) and same_bits(self.vals, vals)
                and same_bits(self.x, x) and same_bits(self.y0, y0))


class Guarded:
    """`count` doubles inside a buffer with at least GUARD cells of PAD on either side; shift = 1 puts the vector at 8 mod 16"""

    def __init__(self, torch, count, shift, fill):
        self.buf = torch.full((count + 2 * GUARD + 1,), PAD, dtype=torch.float64, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.lo, self.count = GUARD + shift, count
        self.v = self.buf[self.lo:self.lo + count]
        self.address = self.buf.data_ptr() + 8 * self.lo
        assert self.address % 16 == 8 * shift
        self.fill(fill)

    def fill(self, what):
        if isinstance(what, float):
            self.v.fill_(what)
        else:
            self.v.copy_(what)

    def guards_intact(self):
        b = self.buf.cpu().numpy()
        return bool(np.all(b[:self.lo] == PAD) and np.all(b[self.lo + self.count:] == PAD))

    def all_nan(self):
        return bool(np.all(np.isnan(self.v.cpu().numpy())))


class Outputs:
    """result arrays two entries longer than `iters`, pre-filled: what an entry did not write still holds -1"""

    def __init__(self, iters):
        self.cap = max(iters, 0) + 2
        self.ms = (ctypes.c_float * self.cap)(*[-1.0] * self.cap)
        self.event_ms = (ctypes.c_float * self.cap)(*[-1.0] * self.cap)
        self.launches = (ctypes.c_int * self.cap)(*[-1] * self.cap)

    def untouched(self):
        return all(v == -1.0 for v in self.ms) and all(v == -1.0 for v in self.event_ms) and all(v == -1 for v in self.launches)

    def check_written(self, entry, iters, positive=True):
        """exactly `iters` results (one for the two regions), finite and > 0; the kernel clock reads at most the event pair around it"""
        count = 1 if entry in ("total", "region") else iters
        ms = list(self.ms)
        assert all(np.isfinite(v) and (v > 0 if positive else v >= 0) for v in ms[:count]), (entry, ms)
        assert all(v == -1.0 for v in ms[count:]), (entry, ms)
        if entry == "kernels":
            ev, ln = list(self.event_ms), list(self.launches)
            assert all(np.isfinite(v) and (v > 0 if positive else v >= 0) for v in ev[:count]) and all(v == -1.0 for v in ev[count:]), (entry, ev)
            assert all((v >= 1 if positive else v == 0) for v in ln[:count]) and all(v == -1 for v in ln[count:]), (entry, ln)
            assert all(k <= e for k, e in zip(ms[:count], ev[:count])), (entry, ms, ev)
        else:
            assert all(v == -1.0 for v in self.event_ms) and all(v == -1 for v in self.launches)
        return ms[:count]


def flush_buffer(torch, nbytes, shift=0):
    """(whole buffer, first byte of the flush region): a byte pattern of nbytes, 64 guard bytes of 0xA5 either side"""
    buf = torch.full((64 + shift + nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    pattern = ((np.arange(nbytes, dtype=np.int64) * 37 + 11) % 251).astype(np.uint8)
    buf[64 + shift:64 + shift + nbytes] = torch.from_numpy(pattern).cuda()
    return buf, 64 + shift, pattern


def call(lib, entry, sid, iters, alpha, beta, case, y, y0, out, m=None, flush=None, flush_bytes=0, result_null=False):
    """one C entry, raw pointers; y / y0 / flush: device addresses (int or None)"""
    m = case.m if m is None else m
    nnz = case.nnz if m == case.m else 0
    head = (sid, iters, alpha, beta, m, case.n, nnz, None, ptr(case.rowptr), ptr(case.cols), ptr(case.vals), ptr(case.x), y)
    ms = None if result_null else out.ms
    fn = getattr(lib, ENTRY_SYMBOLS[entry])
    if entry == "time_spmv":
        return fn(*head, y0, ms)
    if entry == "events_fence":
        return fn(*head, y0, ms, FENCE)
    if entry == "cold":
        return fn(*head, y0, flush, flush_bytes, ms)
    if entry == "kernels":
        return fn(*head, y0, out.event_ms, ms, out.launches)
    assert entry in ("total", "region")
    return fn(*head, ms)


def use_current_stream(torch, lib):
    lib.spmv_acc_set_stream(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


class Tunables:
    def __init__(self, lib, strat):
        self.lib, self.values = lib, TUNABLES[strat]

    def __enter__(self):
        for k, v in self.values.items():
            assert self.lib.spmv_acc_set_tunable(k.encode(), v) == 0, k

    def __exit__(self, *exc):
        self.lib.spmv_acc_reset_tunables()
        spmv_acc_amd.release_plans()
        self.lib.spmv_acc_set_stream(None)
        self.lib.spmv_acc_clear_error()


_FLUSH = {}


def shared_flush(torch):
    """the flush buffer of the cold entry where the flush itself is not under test (4112 bytes: half = 2048)"""
    if "buf" not in _FLUSH:
        _FLUSH["buf"] = flush_buffer(torch, 4112)
    buf, lo, _ = _FLUSH["buf"]
    return buf.data_ptr() + lo, 4112


def plain_calls(torch, case, strat, alpha, beta, y, steps):
    """`steps` plain csr_spmv calls into the SAME y (same address, same alignment) from y0's values"""
    y.fill(case.y0)
    for _ in range(steps):
        spmv_acc_amd.csr_spmv(alpha, beta, case.m, case.n, case.nnz, case.rowptr, case.cols, case.vals, case.x, y.v, strategy=strat)
    torch.cuda.synchronize()
    return y.v.cpu().numpy()


def check_timed_y(torch, oracle, lib, case, strat, entry, alpha, beta, shift_y=0, shift_y0=0, with_y0=True, flush=None, tag=""):
    """One timing call and everything it must leave.  with_y0: 3 launches, each from a y restored from y0 (y starts as NaN: a reset that did not
    happen shows) -> ONE application; without: 4 launches accumulating from y0's values -> FOUR applications.  Returns y's bytes."""
    m = case.m
    iters, steps = (3, 1) if with_y0 else (4, 4)
    what = (tag, entry, strat, m, alpha, beta, shift_y, shift_y0, with_y0)
    sid = spmv_acc_amd.strategy_id(strat)
    y = Guarded(torch, m, shift_y, float("nan") if with_y0 else case.y0)
    y0 = Guarded(torch, m, shift_y0, case.y0)
    out = Outputs(iters)
    fl, fl_bytes = (None, 0)
    if entry == "cold":
        fl, fl_bytes = flush if flush is not None else shared_flush(torch)
    use_current_stream(torch, lib)
    rc = call(lib, entry, sid, iters, alpha, beta, case, y.address, y0.address if with_y0 else None, out, flush=fl, flush_bytes=fl_bytes)
    torch.cuda.synchronize()
    assert rc == 0, (what, rc, lib.spmv_acc_last_error_string())
    assert lib.spmv_acc_last_error() == 0, (what, lib.spmv_acc_last_error_string())
    ms = out.check_written(entry, iters)
    print(f"{entry:13s} {strat:12s} m={m:5d} alpha={alpha} beta={beta} y+{8 * shift_y} y0+{8 * shift_y0} y0={'yes' if with_y0 else 'no '}: "
          f"median {1e3 * float(np.median(ms)):.2f} us" + (f", launches {list(out.launches)[:iters]}" if entry == "kernels" else ""))
    got = y.v.cpu().numpy()
    assert spmv_acc_amd.query_plan(case.rowptr, m)["settled"], what
    assert case.inputs_unchanged(), what
    assert same_bits(y0.v, case.host[4]), what
    assert y.guards_intact() and y0.guards_intact(), what
    ref, scale = reference(oracle, m, alpha, beta, steps)
    assert scaled_error(got, ref, scale) <= SCALED_TOL, (what, scaled_error(got, ref, scale))
    if steps == 1:
        rowptr, cols, vals, x, hy0 = case.host
        assert oracle.scaled_error(got, ref, alpha, beta, rowptr, cols, vals, x, hy0) <= SCALED_TOL, what
    plain = plain_calls(torch, case, strat, alpha, beta, y, steps)  # afterwards, on the same and now settled plan
    assert np.array_equal(plain.view(np.int64), got.view(np.int64)), (what, int(np.sum(plain.view(np.int64) != got.view(np.int64))))
    assert y.guards_intact() and lib.spmv_acc_last_error() == 0, what
    return got.tobytes()


# ---- (a) the per-launch entries with y0 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", ROWS)
def test_per_launch_entries_restore_y_line_enhance(torch_dev, oracle, hiplib, m):
    """spmv_acc_time_spmv, _events (hipEventDisableSystemFence), _cold and _kernels, three launches each from a y restored from y0: the row-block
    kernel (one launch), every alignment of (y, y0), every (alpha, beta).  Aligned and odd m: the copy kernel's body plus the one-workgroup tail
    (the kernel-clock entry: hipMemcpyAsync); m = 1: nothing but the tail; off a 16-byte line: hipMemcpyAsync."""
    case = Case(torch_dev, m)
    with Tunables(hiplib, "line_enhance"):
        for tag, (sy, sy0) in SHIFTS.items():
            for alpha, beta in ALPHA_BETA:
                for entry in PER_LAUNCH:
                    check_timed_y(torch_dev, oracle, hiplib, case, "line_enhance", entry, alpha, beta, sy, sy0, tag=tag)


@pytest.mark.parametrize("strat", ("flat", "adaptive"))
def test_per_launch_entries_restore_y_flat_and_adaptive(torch_dev, oracle, hiplib, strat):
    """The same through flat (tile kernel plus fix-up) and adaptive (guard check plus the timed family): m = 4097 and 4096, aligned and y at 8 mod 16."""
    with Tunables(hiplib, strat):
        for m in (4097, 4096):
            case = Case(torch_dev, m)
            for tag in ("aligned", "y at 8 mod 16"):
                sy, sy0 = SHIFTS[tag]
                for alpha, beta in ALPHA_BETA:
                    for entry in PER_LAUNCH:
                        check_timed_y(torch_dev, oracle, hiplib, case, strat, entry, alpha, beta, sy, sy0, tag=tag)
            spmv_acc_amd.release_plans(case.rowptr)


# ---- (b) the per-launch entries without y0 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strat", ("line_enhance", "flat", "adaptive"))
def test_per_launch_entries_without_y0_accumulate(torch_dev, oracle, hiplib, strat):
    """d_y0 == NULL: no reset, so four launches leave y0 -> (alpha A x + beta .) applied four times: bit for bit four plain calls on the settled plan,
    and within 1e-12 of the oracle applied four times (reference and scale built step by step on the host)."""
    with Tunables(hiplib, strat):
        for m in ROWS if strat == "line_enhance" else (4097, 4096):
            case = Case(torch_dev, m)
            for sy in (0, 1):
                for alpha, beta in ALPHA_BETA:
                    for entry in PER_LAUNCH:
                        check_timed_y(torch_dev, oracle, hiplib, case, strat, entry, alpha, beta, sy, 0, with_y0=False)
            spmv_acc_amd.release_plans(case.rowptr)


# ---- (c) the two regions ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strat", ("line_enhance", "flat", "adaptive"))
def test_total_and_region_accumulate(torch_dev, oracle, hiplib, strat):
    """spmv_acc_time_spmv_total (settles the plan itself) and spmv_acc_time_spmv_region (after spmv_acc_prepare in the call's beta class: returns 0):
    four back-to-back launches accumulate like (b); a second region on a fresh y gives the same bits."""
    torch = torch_dev
    with Tunables(hiplib, strat):
        for m in (4097, 4096):
            case = Case(torch, m)
            for sy in (0, 1):
                for alpha, beta in ALPHA_BETA:
                    first = check_timed_y(torch, oracle, hiplib, case, strat, "total", alpha, beta, sy, with_y0=False)
                    spmv_acc_amd.release_plans(case.rowptr)
                    spmv_acc_amd.prepare(m, case.n, case.nnz, case.rowptr, case.cols, case.vals, case.x, strategy=strat, beta=beta)
                    second = check_timed_y(torch, oracle, hiplib, case, strat, "region", alpha, beta, sy, with_y0=False)
                    again = check_timed_y(torch, oracle, hiplib, case, strat, "region", alpha, beta, sy, with_y0=False)
                    assert second == again, (strat, m, alpha, beta, sy)
                    assert len(first) == len(second) == 8 * m
            spmv_acc_amd.release_plans(case.rowptr)


@pytest.mark.parametrize("strat", ("line_enhance", "flat", "adaptive"))
def test_region_refuses_a_plan_that_was_not_settled(torch_dev, oracle, hiplib, strat):
    """After spmv_acc_release_plans the first region call without spmv_acc_prepare does plan work between its two events: SPMV_ACC_ERR_BAD_ARGUMENT
    with "the plan was not settled" -- the time is still written, and y is still four applications (by the tolerance only: calls before a plan
    settles are served by the plan's rule twin and may differ in the last bits from the settled plan's).  After spmv_acc_prepare in beta class b a
    region call in class b returns 0."""
    torch = torch_dev
    sid = spmv_acc_amd.strategy_id(strat)
    with Tunables(hiplib, strat):
        for m in (4097, 4096):
            case = Case(torch, m)
            for alpha, beta in ALPHA_BETA:
                spmv_acc_amd.release_plans()
                y = Guarded(torch, m, 0, case.y0)
                out = Outputs(4)
                use_current_stream(torch, hiplib)
                rc = call(hiplib, "region", sid, 4, alpha, beta, case, y.address, None, out)
                torch.cuda.synchronize()
                assert rc == BAD_ARGUMENT and hiplib.spmv_acc_last_error() == BAD_ARGUMENT, (strat, m, rc)
                assert b"the plan was not settled" in hiplib.spmv_acc_last_error_string()
                hiplib.spmv_acc_clear_error()
                out.check_written("region", 4)
                ref, scale = reference(oracle, m, alpha, beta, 4)
                got = y.v.cpu().numpy()
                assert scaled_error(got, ref, scale) <= SCALED_TOL, (strat, m, alpha, beta, scaled_error(got, ref, scale))
                assert y.guards_intact() and case.inputs_unchanged()
                spmv_acc_amd.prepare(m, case.n, case.nnz, case.rowptr, case.cols, case.vals, case.x, strategy=strat, beta=beta)
                check_timed_y(torch, oracle, hiplib, case, strat, "region", alpha, beta, with_y0=False)


# ---- (d) the cold entry's flush buffer ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbytes", (32, 1000, 4112))
def test_cold_flush_overwrites_its_second_half_with_its_first(torch_dev, oracle, hiplib, nbytes):
    """half = flush_bytes / 2 / 16 * 16 (16, 496, 2048): bytes [half, 2 half) <- bytes [0, half); bytes [0, half), bytes [2 half, flush_bytes) and the
    64 guard bytes either side as they were; y as in (a)."""
    torch = torch_dev
    half = nbytes // 2 // 16 * 16
    assert 0 < half and 2 * half <= nbytes
    for m in (4097, 4096):
        case = Case(torch, m)
        with Tunables(hiplib, "line_enhance"):
            for alpha, beta in ALPHA_BETA:
                buf, lo, pattern = flush_buffer(torch, nbytes)
                check_timed_y(torch, oracle, hiplib, case, "line_enhance", "cold", alpha, beta, flush=(buf.data_ptr() + lo, nbytes))
                b = buf.cpu().numpy()
                assert np.all(b[:lo] == 0xA5) and np.all(b[lo + nbytes:] == 0xA5), nbytes
                got = b[lo:lo + nbytes]
                assert np.array_equal(got[:half], pattern[:half]), nbytes
                assert np.array_equal(got[half:2 * half], pattern[:half]), nbytes
                assert np.array_equal(got[2 * half:], pattern[2 * half:]), nbytes
                assert not np.array_equal(pattern[half:2 * half], pattern[:half])  # (the pattern tells the two halves apart)


def test_cold_entry_refuses_a_bad_flush_buffer(torch_dev, hiplib):
    """A NULL flush buffer, fewer than 32 bytes, a base at 8 mod 16: SPMV_ACC_ERR_BAD_ARGUMENT ("... 16-byte aligned ..."), and nothing was touched."""
    torch = torch_dev
    case = Case(torch, 4097)
    sid = spmv_acc_amd.strategy_id("line_enhance")
    with Tunables(hiplib, "line_enhance"):
        for tag, shift, nbytes, null in (("null", 0, 4112, True), ("31 bytes", 0, 31, False), ("base at 8 mod 16", 8, 4112, False)):
            buf, lo, pattern = flush_buffer(torch, max(nbytes, 32), shift)
            before = buf.cpu().numpy().copy()
            y, y0, out = Guarded(torch, case.m, 0, float("nan")), Guarded(torch, case.m, 0, case.y0), Outputs(3)
            use_current_stream(torch, hiplib)
            rc = call(hiplib, "cold", sid, 3, 0.5, -2.0, case, y.address, y0.address, out, flush=None if null else buf.data_ptr() + lo, flush_bytes=nbytes)
            torch.cuda.synchronize()
            assert rc == BAD_ARGUMENT and hiplib.spmv_acc_last_error() == BAD_ARGUMENT, (tag, rc)
            assert b"16-byte aligned" in hiplib.spmv_acc_last_error_string(), tag
            hiplib.spmv_acc_clear_error()
            assert y.all_nan() and y.guards_intact() and y0.guards_intact() and out.untouched(), tag
            assert np.array_equal(buf.cpu().numpy(), before) and case.inputs_unchanged(), tag


# ---- (e) bad arguments, every entry ------------------------------------------------------------------------------------------------------------------
ALL_TIMED = PER_LAUNCH + ("total", "region")


def _refused(torch, lib, case, entry, sid, iters, want, tag, result_null=False):
    y, y0, out = Guarded(torch, case.m, 0, float("nan")), Guarded(torch, case.m, 0, case.y0), Outputs(3)
    fl, fl_bytes = shared_flush(torch)
    use_current_stream(torch, lib)
    rc = call(lib, entry, sid, iters, 0.5, -2.0, case, y.address, y0.address, out, flush=fl, flush_bytes=fl_bytes, result_null=result_null)
    torch.cuda.synchronize()
    code = lib.spmv_acc_last_error()
    lib.spmv_acc_clear_error()
    assert rc == want and code == want, (tag, entry, rc, code)
    assert y.all_nan(), (tag, entry, "y was written")
    assert out.untouched(), (tag, entry, list(out.ms), list(out.event_ms), list(out.launches))
    assert y.guards_intact() and y0.guards_intact() and case.inputs_unchanged(), (tag, entry)


def test_bad_arguments_leave_everything_untouched(torch_dev, hiplib):
    """iters 0 and -1, or a NULL result pointer (the kernel-clock entry: kernel_ms_out; its event_ms_out and launches_out may be NULL):
    SPMV_ACC_ERR_BAD_ARGUMENT, nothing launched -- y still NaN, every result still pre-filled."""
    torch = torch_dev
    case = Case(torch, 4097)
    sid = spmv_acc_amd.strategy_id("line_enhance")
    with Tunables(hiplib, "line_enhance"):
        for entry in ALL_TIMED:
            _refused(torch, hiplib, case, entry, sid, 0, BAD_ARGUMENT, "iters 0")
            _refused(torch, hiplib, case, entry, sid, -1, BAD_ARGUMENT, "iters -1")
            _refused(torch, hiplib, case, entry, sid, 3, BAD_ARGUMENT, "null result", result_null=True)
        assert spmv_acc_amd.query_plan(case.rowptr, case.m) is None  # (refused before any plan work)


def test_unknown_strategy_id_is_refused_before_anything_is_written(torch_dev, hiplib):
    """A strategy id no strategy has -- what spmv_acc_parse_strategy answers to a name it does not know -- is SPMV_ACC_ERR_UNKNOWN_STRATEGY (5), the
    code include/spmv_acc.h documents for it in the measurement helper's comment, from every timing entry; y and the results are untouched."""
    torch = torch_dev
    bad = hiplib.spmv_acc_parse_strategy(b"no-such-strategy")
    assert bad < 0 and hiplib.spmv_acc_strategy_name(bad) == b"unknown"
    assert all(spmv_acc_amd.strategy_id(s) != bad for s in spmv_acc_amd.STRATEGIES)
    hiplib.spmv_acc_clear_error()
    case = Case(torch, 4097)
    with Tunables(hiplib, "line_enhance"):
        for entry in ALL_TIMED:
            _refused(torch, hiplib, case, entry, bad, 3, UNKNOWN_STRATEGY, "unknown strategy")


def test_zero_rows_launch_nothing(torch_dev, hiplib):
    """m = 0: returns 0, writes nothing to y (handed five NaNs it must not touch), and the times are finite and >= 0."""
    torch = torch_dev
    case = Case(torch, 3)
    sid = spmv_acc_amd.strategy_id("line_enhance")
    with Tunables(hiplib, "line_enhance"):
        for entry in ALL_TIMED:
            y, y0, out = Guarded(torch, 5, 0, float("nan")), Guarded(torch, 5, 0, 1.0), Outputs(3)
            fl, fl_bytes = shared_flush(torch)
            use_current_stream(torch, hiplib)
            rc = call(hiplib, entry, sid, 3, 0.5, -2.0, case, y.address, y0.address, out, m=0, flush=fl, flush_bytes=fl_bytes)
            torch.cuda.synchronize()
            assert rc == 0 and hiplib.spmv_acc_last_error() == 0, (entry, rc, hiplib.spmv_acc_last_error_string())
            out.check_written(entry, 3, positive=False)
            assert y.all_nan() and y.guards_intact() and y0.guards_intact() and case.inputs_unchanged(), entry


# ---- (f) the environment switches, each in a fresh process ----------------------------------------------------------------------------------------
def digest_of_the_aligned_line_enhance_cases(torch, oracle, lib):
    """case (a) for line_enhance, m = 4097 and 4096, aligned -- every check of it -- and the SHA-256 of the y's it left"""
    h = hashlib.sha256()
    with Tunables(lib, "line_enhance"):
        for m in (4097, 4096):
            case = Case(torch, m)
            for alpha, beta in ALPHA_BETA:
                for entry in PER_LAUNCH:
                    h.update(check_timed_y(torch, oracle, lib, case, "line_enhance", entry, alpha, beta))
    return h.hexdigest()


_CHILD = r"""
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import torch
import spmv_acc_amd
import oracle_lib
import test_gpu_timing_entries as T
oracle_lib.lib()
print("DIGEST " + T.digest_of_the_aligned_line_enhance_cases(torch, oracle_lib, spmv_acc_amd.load_library()))
"""


def _child(extra_env):
    env = dict(os.environ, **extra_env)
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (extra_env, r.stdout[-2000:], r.stderr[-3000:])
    res = [ln for ln in r.stdout.splitlines() if ln.startswith("DIGEST ")]
    return res[-1][7:]


@pytest.mark.parametrize("switch", ("SPMV_ACC_RESET_MEMCPY=1", "SPMV_ACC_RESET_NT=0"))
def test_reset_switches_in_a_fresh_process(torch_dev, oracle, hiplib, switch):
    """SPMV_ACC_RESET_MEMCPY=1 (hipMemcpyAsync instead of the copy kernel) and SPMV_ACC_RESET_NT=0 (default-policy instead of non-temporal copy) are
    read once per process: a child per switch, one at a time, runs case (a) with all its checks and prints the SHA-256 of y's bytes -- this
    process's, which runs with neither set."""
    assert "SPMV_ACC_RESET_MEMCPY" not in os.environ and "SPMV_ACC_RESET_NT" not in os.environ
    name, value = switch.split("=")
    assert _child({name: value}) == digest_of_the_aligned_line_enhance_cases(torch_dev, oracle, hiplib)


# ---- (g) the copy ceiling and its kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbytes", (16, 16 * 1023, 16 * 1024, 16 * 1025))
def test_copy_ceiling_copies_exactly_its_bytes(torch_dev, hiplib, nbytes):
    """stream_copy_kernel through spmv_acc_copy_ceiling_gbs: one 16-byte unit; one short of a workgroup's 1024 units, exactly one workgroup, one unit
    into the second.  dst's first `nbytes` are src's, the 48 bytes beyond and the guards as they were, src unchanged, the figure > 0."""
    torch = torch_dev
    rng = np.random.default_rng(nbytes)
    dst, lo, pattern = flush_buffer(torch, nbytes + 48)
    src_bytes = rng.integers(0, 256, nbytes + 48, dtype=np.uint8)
    src = torch.full((64 + nbytes + 48 + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    src[64:64 + nbytes + 48] = torch.from_numpy(src_bytes).cuda()
    src_before = src.cpu().numpy().copy()
    use_current_stream(torch, hiplib)
    gbs = hiplib.spmv_acc_copy_ceiling_gbs(ctypes.c_void_p(dst.data_ptr() + lo), ctypes.c_void_p(src.data_ptr() + 64), nbytes, 2)
    torch.cuda.synchronize()
    print(f"copy ceiling at {nbytes} bytes: {gbs:.3f} GB/s")
    assert np.isfinite(gbs) and gbs > 0
    got = dst.cpu().numpy()
    assert np.array_equal(got[lo:lo + nbytes], src_bytes[:nbytes])
    assert np.array_equal(got[lo + nbytes:lo + nbytes + 48], pattern[nbytes:])
    assert np.all(got[:lo] == 0xA5) and np.all(got[lo + nbytes + 48:] == 0xA5)
    assert np.array_equal(src.cpu().numpy(), src_before)


def test_copy_ceiling_refusals_write_nothing(torch_dev, hiplib):
    """fewer than 16 bytes, reps = 0, a NULL pointer: -1.0 and nothing is written"""
    torch = torch_dev
    dst, lo, _ = flush_buffer(torch, 4096)
    src, slo, _ = flush_buffer(torch, 4096)
    src[slo:slo + 4096] = 0x33
    before = dst.cpu().numpy().copy()
    d, s = ctypes.c_void_p(dst.data_ptr() + lo), ctypes.c_void_p(src.data_ptr() + slo)
    use_current_stream(torch, hiplib)
    for tag, args in (("15 bytes", (d, s, 15, 2)), ("reps 0", (d, s, 4096, 0)), ("null dst", (None, s, 4096, 2)), ("null src", (d, None, 4096, 2))):
        assert hiplib.spmv_acc_copy_ceiling_gbs(*args) == -1.0, tag
        torch.cuda.synchronize()
        assert np.array_equal(dst.cpu().numpy(), before), tag


# ---- (h) a side stream ------------------------------------------------------------------------------------------------------------------------------------
def test_per_launch_entries_on_a_side_stream(torch_dev, oracle, hiplib):
    """Case (a), line_enhance, m = 4097, inside torch.cuda.stream(s): x, y0 and y are filled ON s, behind half a gigabyte of other traffic on s and
    with no synchronisation before the call (until then x holds zeros and y0 ones) -- an entry that restored y, flushed or launched anywhere but on
    the library stream would read what was there before.  y must be the default-stream run's, bit for bit.  (The matrix is uploaded and
    synchronised beforehand, as for any first call on a matrix: the plan samples rowptr with blocking copies.)"""
    torch = torch_dev
    m = 4097
    case = Case(torch, m)
    wrappers = {
        "time_spmv": lambda a, b, x, y, y0, fl: spmv_acc_amd.time_spmv("line_enhance", 3, a, b, m, case.n, case.nnz, case.rowptr, case.cols, case.vals, x, y, y0),
        "events_fence": lambda a, b, x, y, y0, fl: spmv_acc_amd.time_spmv("line_enhance", 3, a, b, m, case.n, case.nnz, case.rowptr, case.cols, case.vals, x, y,
                                                                          y0, event_flags=FENCE),
        "cold": lambda a, b, x, y, y0, fl: spmv_acc_amd.time_spmv_cold("line_enhance", 3, a, b, m, case.n, case.nnz, case.rowptr, case.cols, case.vals, x, y,
                                                                       y0, fl),
        "kernels": lambda a, b, x, y, y0, fl: spmv_acc_amd.time_spmv_kernels("line_enhance", 3, a, b, m, case.n, case.nnz, case.rowptr, case.cols, case.vals, x,
                                                                             y, y0)[1],
    }
    with Tunables(hiplib, "line_enhance"):
        want = {(entry, ab): check_timed_y(torch, oracle, hiplib, case, "line_enhance", entry, *ab) for ab in ALPHA_BETA for entry in PER_LAUNCH}
        side = torch.cuda.Stream()
        ballast = torch.zeros(1 << 25, dtype=torch.float64, device="cuda")
        flush = torch.zeros(4112, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for (entry, (alpha, beta)), want_bytes in want.items():
            x = torch.zeros(case.n, dtype=torch.float64, device="cuda")
            y, y0 = Guarded(torch, m, 0, 1.0), Guarded(torch, m, 0, 1.0)
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                ballast.add_(1.0)
                x.copy_(case.x)
                y0.fill(case.y0)
                y.fill(float("nan"))
                ms = wrappers[entry](alpha, beta, x, y.v, y0.v, flush)
            side.synchronize()
            assert len(ms) == 3 and all(np.isfinite(v) and v > 0 for v in ms), (entry, ms)
            assert y.v.cpu().numpy().tobytes() == want_bytes, (entry, alpha, beta)
            assert y.guards_intact() and y0.guards_intact() and same_bits(y0.v, case.host[4]) and same_bits(x, case.host[3]), entry
            assert hiplib.spmv_acc_last_error() == 0
        torch.cuda.synchronize()
