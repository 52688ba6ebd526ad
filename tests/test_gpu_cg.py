"""GPU suite (-m gpu) of the conjugate-gradient vector passes (spmv_acc_cg_start / cg_start, spmv_acc_cg_update / cg_update,
spmv_acc_cg_direction / cg_direction) and of the solver composed of them (spmv_acc_amd.pcg): each entry alone bit for bit against the host
model of tests/test_cg_host.py -- state, history, x, r, p, z and the padding around every written array; -0.0 and +0.0 count as equal, NaNs by
position --, the frozen state after every status, grid striding, a captured and replayed iteration, the contract on the device, AMG-PCG on the
four hierarchies of tests/test_amg_host.py, plain and Jacobi CG, and the independence of check_every.

TOLERANCES, each 100 times a spread measured on the CPU between two host restatements that differ only in the SpMVs' summation order (the
figures are in the docstring of tests/test_cg_host.py, whose test_the_spreads measures them again): the device's SpMVs add in the engine's
order, its dot products and vector updates are the host model's to the bit.
  AMG-PCG: every iterate within 1.2e-13 of its largest magnitude, every history entry within 1e-11 relative; the iteration count is the host's
    (no history entry lies near the threshold); the true residual of the device's x, computed in numpy, below PCG_RESIDUAL_BOUND = 1e-9, ten
    times the host model's largest rounded up to a power of ten.
  Plain and Jacobi CG on grid24: the first 10 history entries within 1e-13 relative; the count within the host's 77 plus or minus 1 (the two
    host orders differ by 0).

  AMG-PCG on the irregular cases of tests/test_amg_host.py, and on fem_weak from a non-zero x0 with pre = post = 2: the host's count exactly
    (tests/test_cg_host.py checks that the entries on either side of the threshold lie farther from it than their tolerance); every iterate
    within 1.2e-13 (7.5e-13 from the non-zero start) of its largest magnitude; every history entry within 100 times that entry's own
    forward-against-reversed spread, at least 100 * 2^-52 -- a converging history's tail is rounding noise relative to itself, so no single
    relative tolerance fits --; the true residual below the same 1e-9.  Nobody has measured the device's spreads on these cases: every
    tolerance comes from the host model alone.

No speed gate: the parent commit cannot do this job (tools/cg_bench.py measures)."""
import ctypes

import numpy as np
import pytest

import spmv_acc_amd
from test_amg_host import OMEGA, TAGS, problem, rhs, rhs_of
from test_cg_host import (CG_COUNT_SPREAD, CG_COUNTS, CG_FIRST, CG_HISTORY_SPREAD, CG_RTOL, IRREGULAR_SOLVES, PARTIAL, PCG_COUNTS, PCG_HISTORY_SPREAD,
                          PCG_ITERATE_SPREAD, PCG_RESIDUAL_BOUND, PCG_RTOL, SIZES, STATE, STRIDE_SIZE, history_tolerances, host_cg_direction, host_cg_start,
                          host_cg_update, inverse_diagonal, iterate_spread, matrix, solve, solve_count, state_words, true_residual, x0_of)
from test_gpu_dense import dev, ptr, same_bits

pytestmark = pytest.mark.gpu

PCG_ITERATE_TOL, PCG_HISTORY_TOL, CG_HISTORY_TOL = 100 * PCG_ITERATE_SPREAD, 100 * PCG_HISTORY_SPREAD, 100 * CG_HISTORY_SPREAD
PAD, FILL = 8, 7.25
FILL_WORD = int(np.array([FILL]).view(np.int64)[0])


@pytest.fixture(scope="module")
def torch_dev(hiplib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


class Arrays:
    """The arrays of one solve on the device, each inside a buffer with PAD entries of 7.25 on either side: vectors by name, the partials
    buffer, the state block (int64 words) and the history."""

    def __init__(self, torch, n, hist_cap, **vectors):
        self.torch, self.n = torch, n
        self.buf = {}
        for name, a in vectors.items():
            self._make(name, n, torch.float64, a)
        self._make("partials", spmv_acc_amd.cg_partials(n), torch.float64, None)
        self._make("hist", hist_cap, torch.float64, np.full(hist_cap, -1.0))
        self.buf["state"] = torch.full((STATE + 2 * PAD,), FILL_WORD, dtype=torch.int64, device="cuda")
        self.state = self.buf["state"][PAD:PAD + STATE]

    def _make(self, name, count, dtype, a):
        self.buf[name] = self.torch.full((count + 2 * PAD,), FILL, dtype=dtype, device="cuda")
        view = self.buf[name][PAD:PAD + count]
        if a is not None and count:
            view.copy_(dev(self.torch, np.asarray(a, dtype=np.float64)))
        setattr(self, name, view)

    def set(self, name, a):
        getattr(self, name).copy_(dev(self.torch, np.asarray(a, dtype=np.float64)))

    def pads_intact(self):
        self.torch.cuda.synchronize()
        for name, b in self.buf.items():
            fill = FILL_WORD if name == "state" else FILL
            if not (bool((b[:PAD] == fill).all()) and bool((b[-PAD:] == fill).all())):
                return False
        return True

    def snapshot(self):
        self.torch.cuda.synchronize()
        return {name: b.view(self.torch.int64).clone() for name, b in self.buf.items()}

    def changed_since(self, snap):
        self.torch.cuda.synchronize()
        return [name for name, b in self.buf.items() if not self.torch.equal(b.view(self.torch.int64), snap[name])]


def same_state(t, want):
    """The device's block against the host's dict: the two integer words exactly, the doubles as same_bits compares."""
    got = t.cpu()
    words = state_words(want)
    import torch

    return [int(got[0]), int(got[1])] == [int(words[0]), int(words[1])] and same_bits(got.view(torch.float64)[2:], words[2:].view(np.float64))


def vectors(n, seed):
    """b, x, r, z and the diagonals w (the matrix A = diag(w), SPD: q = w p needs no SpMV), dinv and minv (two preconditioners), seeded."""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.integers(-3, 4, n)
    return dict(b=rng.standard_normal(n) * scale, x=rng.standard_normal(n), r=rng.standard_normal(n) * scale, w=rng.uniform(0.5, 2.0, n),
                dinv=rng.uniform(0.25, 4.0, n), minv=rng.uniform(0.5, 1.5, n))


@pytest.mark.parametrize("n", SIZES)
def test_each_entry_is_the_host_model(torch_dev, hiplib, n):
    """The start and three iterations on seeded vectors with A = diag(w), each entry's outputs bit for bit against the host model, the padding
    around every written array kept; the direction in its three forms: Jacobi fused (z written), the caller's z, and z == r.  Twice."""
    torch = torch_dev
    v = vectors(n, 700 + n % 1000)
    plans = hiplib.spmv_acc_cached_plans()
    hist_cap = 3  # (room for the iterations 0, 1, 2: the third iteration's entry has no room)
    for _ in range(2):
        z0 = v["minv"] * v["r"]
        a = Arrays(torch, n, hist_cap, b=v["b"], r=v["r"], z=z0, p=np.full(n, 3.0), q=np.zeros(n), x=v["x"], dinv=v["dinv"])
        hist = np.full(hist_cap, -1.0)
        p, st = host_cg_start(1e-6, v["b"], v["r"], z0, hist)
        spmv_acc_amd.cg_start(n, 1e-6, a.b, a.r, a.z, a.p, a.partials, a.state, a.hist)
        assert same_bits(a.p, p) and same_state(a.state, st) and same_bits(a.hist, hist) and a.pads_intact(), n
        assert st["status"] == (1 if n == 0 else 0) and same_bits(a.r, v["r"]) and same_bits(a.z, z0) and same_bits(a.b, v["b"])
        x, r, z = v["x"], v["r"], z0
        for it in range(3):
            q = v["w"] * p
            a.set("q", q)
            x, r, st = host_cg_update(p, q, x, r, st, hist)
            spmv_acc_amd.cg_update(n, a.p, a.q, a.x, a.r, a.partials, a.state, a.hist)
            assert same_bits(a.x, x) and same_bits(a.r, r) and same_state(a.state, st) and same_bits(a.hist, hist) and a.pads_intact(), (n, it)
            assert same_bits(a.p, p) and same_bits(a.q, q)
            if it == 0:  # Jacobi, fused: z = dinv r is written
                z, p, st = host_cg_direction(r, z, p, st, v["dinv"])
                spmv_acc_amd.cg_direction(n, a.r, a.z, a.p, a.partials, a.state, dinv=a.dinv)
            elif it == 1:  # the caller's z = M r
                z = v["minv"] * r
                a.set("z", z)
                z, p, st = host_cg_direction(r, z, p, st)
                spmv_acc_amd.cg_direction(n, a.r, a.z, a.p, a.partials, a.state)
            else:  # no preconditioner: z is r
                _, p, st = host_cg_direction(r, r, p, st)
                spmv_acc_amd.cg_direction(n, a.r, a.r, a.p, a.partials, a.state)
            assert same_bits(a.p, p) and same_bits(a.z, z) and same_bits(a.r, r) and same_state(a.state, st) and a.pads_intact(), (n, it)
        assert n < 63 or (st["status"] == 0 and st["iterations"] == 3 and hist[2] != -1.0)  # (n = 0 converges at the start, n = 1 in one iteration)
    # the start with z == r (no preconditioner) shares its loads
    a = Arrays(torch, n, 0, b=v["b"], r=v["r"], p=np.zeros(n))
    p, st = host_cg_start(0.0, v["b"], v["r"], v["r"])
    spmv_acc_amd.cg_start(n, 0.0, a.b, a.r, a.r, a.p, a.partials, a.state)
    assert same_bits(a.p, p) and same_state(a.state, st) and a.pads_intact() and st["tol2"] == 0.0
    assert hiplib.spmv_acc_cached_plans() == plans and hiplib.spmv_acc_last_error() == 0


def test_frozen_state(torch_dev, hiplib):
    """After status 1 (b = 0 at the start; a converged update), 2 (an inf, a NaN in p; p = 0) and 3 (a negative inverse diagonal; r.z <= 0 at the
    start), five more update + direction calls -- in both forms of the direction -- change no bit of any array, padding included."""
    torch = torch_dev
    n = 2 * PARTIAL + 77
    v = vectors(n, 31)

    def fresh(rtol=1e-8, b=v["b"], r=v["r"], z=None, p_after=None):
        z = v["minv"] * r if z is None else z
        a = Arrays(torch, n, 4, b=b, r=r, z=z, p=np.zeros(n), q=np.zeros(n), x=v["x"], dinv=v["dinv"])
        hist = np.full(4, -1.0)
        p, st = host_cg_start(rtol, b, r, z, hist)
        spmv_acc_amd.cg_start(n, rtol, a.b, a.r, a.z, a.p, a.partials, a.state, a.hist)
        if p_after is not None:
            p = p_after
            a.set("p", p)
        a.set("q", v["w"] * p)
        return a, p, st, hist, z

    def stays_frozen(a, st, tag):
        assert st["status"] != 0 and same_state(a.state, st), tag
        snap = a.snapshot()
        for k in range(5):
            spmv_acc_amd.cg_update(n, a.p, a.q, a.x, a.r, a.partials, a.state, a.hist)
            spmv_acc_amd.cg_direction(n, a.r, a.z, a.p, a.partials, a.state, dinv=a.dinv if k % 2 else None)
        assert a.changed_since(snap) == [], tag

    # status 1 at the start: b = 0 with r = b - A 0 = 0; zero iterations, x untouched
    a, p, st, hist, z = fresh(b=np.zeros(n), r=np.zeros(n))
    assert st["status"] == 1 and st["iterations"] == 0 and same_bits(a.x, v["x"])
    stays_frozen(a, st, "b = 0")
    # status 1 after an update: a tolerance between r.r of the start and of the first iteration
    p, st = host_cg_start(0.0, v["b"], v["r"], v["minv"] * v["r"])
    after = host_cg_update(p, v["w"] * p, v["x"], v["r"], st)[2]
    assert after["rr"] < st["rr"]
    a, p, st, hist, z = fresh(rtol=float(np.sqrt(0.5 * (after["rr"] + st["rr"]) / st["bb"])))
    assert st["status"] == 0
    x, r, st = host_cg_update(p, v["w"] * p, v["x"], v["r"], st, hist)
    spmv_acc_amd.cg_update(n, a.p, a.q, a.x, a.r, a.partials, a.state, a.hist)
    assert st["status"] == 1 and st["iterations"] == 1 and same_bits(a.x, x) and same_bits(a.r, r) and same_bits(a.hist, hist)
    stays_frozen(a, st, "converged")
    # status 2: p.q not finite, or not positive; x and r keep their bits
    for tag, edit in (("inf", np.inf), ("nan", np.nan), ("zero", None)):
        bad = np.zeros(n) if edit is None else host_cg_start(1e-8, v["b"], v["r"], v["minv"] * v["r"])[0]
        if edit is not None:
            bad[n // 2] = edit
        a, p, st, hist, z = fresh(p_after=bad)
        with np.errstate(all="ignore"):
            x, r, st = host_cg_update(p, v["w"] * p, v["x"], v["r"], st, hist)
        spmv_acc_amd.cg_update(n, a.p, a.q, a.x, a.r, a.partials, a.state, a.hist)
        assert st["status"] == 2 and st["iterations"] == 0 and same_bits(a.x, v["x"]) and same_bits(a.r, v["r"]) and same_bits(a.hist, hist), tag
        stays_frozen(a, st, tag)
    # status 3 in the direction: a negative inverse diagonal; z is written, p is kept
    a, p, st, hist, z = fresh()
    x, r, st = host_cg_update(p, v["w"] * p, v["x"], v["r"], st, hist)
    spmv_acc_amd.cg_update(n, a.p, a.q, a.x, a.r, a.partials, a.state, a.hist)
    a.set("dinv", -v["dinv"])
    z, p2, st = host_cg_direction(r, z, p, st, -v["dinv"])
    spmv_acc_amd.cg_direction(n, a.r, a.z, a.p, a.partials, a.state, dinv=a.dinv)
    assert st["status"] == 3 and st["iterations"] == 1 and same_bits(a.z, z) and same_bits(a.p, p) and np.array_equal(p2, p)
    stays_frozen(a, st, "negative dinv")
    # status 3 at the start: r.z <= 0 while r.r > tol2
    a, p, st, hist, z = fresh(z=-v["r"])
    assert st["status"] == 3
    stays_frozen(a, st, "r.z < 0 at the start")
    assert hiplib.spmv_acc_last_error() == 0


def one_iteration(torch, n, v, a, rounds=2):
    """start and `rounds` iterations (Jacobi direction) on the arrays a; returns nothing: the caller compares the buffers."""
    spmv_acc_amd.cg_start(n, 0.0, a.b, a.r, a.z, a.p, a.partials, a.state, a.hist)
    for _ in range(rounds):
        torch.mul(a.w, a.p, out=a.q)
        spmv_acc_amd.cg_update(n, a.p, a.q, a.x, a.r, a.partials, a.state, a.hist)
        spmv_acc_amd.cg_direction(n, a.r, a.z, a.p, a.partials, a.state, dinv=a.dinv)
    torch.cuda.synchronize()


def test_cg_grid_stride_at_test_size(torch_dev, hiplib):
    """max_grid_blocks lowered to 64, the smallest cap the library honours: 258 chunks are 65 workgroups' worth; the same bits as with the
    default grid in every array, and the host model's state."""
    torch = torch_dev
    n = STRIDE_SIZE
    assert (-(-n // PARTIAL) + 3) // 4 > 64
    v = vectors(n, 64)
    z0 = v["minv"] * v["r"]

    def run():
        a = Arrays(torch, n, 3, b=v["b"], r=v["r"], z=z0, p=np.zeros(n), q=np.zeros(n), x=v["x"], dinv=v["dinv"], w=v["w"])
        one_iteration(torch, n, v, a)
        return a

    default = run()
    try:
        assert hiplib.spmv_acc_set_tunable(b"max_grid_blocks", 64) == 0
        strided = run()
    finally:
        hiplib.spmv_acc_reset_tunables()
    for name in default.buf:
        assert torch.equal(default.buf[name].view(torch.int64), strided.buf[name].view(torch.int64)), name
    hist = np.full(3, -1.0)
    p, st = host_cg_start(0.0, v["b"], v["r"], z0, hist)
    x, r, z = v["x"], v["r"], z0
    for _ in range(2):
        x, r, st = host_cg_update(p, v["w"] * p, x, r, st, hist)
        z, p, st = host_cg_direction(r, z, p, st, v["dinv"])
    assert same_state(strided.state, st) and same_bits(strided.x, x) and same_bits(strided.p, p) and same_bits(strided.hist, hist) and strided.pads_intact()
    assert hiplib.spmv_acc_last_error() == 0


def test_update_and_direction_captured_and_replayed(torch_dev, hiplib):
    """One update + direction pair captured after a warm call -- the entries are launch-only and refused in no capture -- and replayed after
    p, q, r and x were edited in place: each replay gives the host model's bits, the state block carrying on from the replay before."""
    torch = torch_dev
    n = 3 * PARTIAL + 5
    v = vectors(n, 9)
    z0 = v["minv"] * v["r"]
    a = Arrays(torch, n, 8, b=v["b"], r=v["r"], z=z0, p=np.zeros(n), q=np.zeros(n), x=v["x"], dinv=v["dinv"], w=v["w"])
    one_iteration(torch, n, v, a, rounds=1)  # (warm: the code objects are loaded outside the capture)
    hist = np.full(8, -1.0)
    p, st = host_cg_start(0.0, v["b"], v["r"], z0, hist)
    x, r, st = host_cg_update(p, v["w"] * p, v["x"], v["r"], st, hist)
    z, p, st = host_cg_direction(r, z0, p, st, v["dinv"])
    assert same_state(a.state, st) and same_bits(a.p, p)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        torch.cuda.synchronize()
        snap = a.snapshot()
        with torch.cuda.graph(g, stream=s):
            spmv_acc_amd.cg_update(n, a.p, a.q, a.x, a.r, a.partials, a.state, a.hist)
            spmv_acc_amd.cg_direction(n, a.r, a.z, a.p, a.partials, a.state, dinv=a.dinv)
    assert hiplib.spmv_acc_last_error() == 0 and a.changed_since(snap) == []  # captured, not run
    rng = np.random.default_rng(77)
    for k in range(2):
        p, x, r = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
        q = v["w"] * p
        for name, arr in (("p", p), ("q", q), ("x", x), ("r", r)):
            a.set(name, arr)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        x, r, st = host_cg_update(p, q, x, r, st, hist)
        z, p, st = host_cg_direction(r, z, p, st, v["dinv"])
        assert st["status"] == 0 and st["iterations"] == 2 + k
        assert same_bits(a.x, x) and same_bits(a.r, r) and same_bits(a.z, z) and same_bits(a.p, p) and same_state(a.state, st) and same_bits(a.hist, hist), k
        assert a.pads_intact()
    del g


def test_cg_contract(torch_dev, hiplib):
    """On real arrays: each overlap and each null pointer is refused with nothing written; adjacent arrays and z == r are accepted."""
    torch = torch_dev
    n = PARTIAL + 9
    v = vectors(n, 5)
    names = ("spare", "b", "r", "z", "p", "q", "x", "dinv", "more")  # (a spare vector at either end: a shifted view stays inside the allocation)
    room = torch.full((len(names) * n,), -3.0, dtype=torch.float64, device="cuda")
    at = {name: room[k * n:(k + 1) * n] for k, name in enumerate(names) if name not in ("spare", "more")}  # adjacent vectors: no two overlap
    small = torch.full((64,), -3.0, dtype=torch.float64, device="cuda")
    at["partials"], at["hist"] = small[:6], small[6:10]
    state = torch.full((STATE,), 5, dtype=torch.int64, device="cuda")
    hiplib.spmv_acc_set_stream(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    def call(entry, **over):
        a = dict(at, state=state)
        a.update(over)
        g = lambda k: ptr(a[k]) if a[k] is not None else None  # noqa: E731
        if entry == "start":
            rc = hiplib.spmv_acc_cg_start(n, 1e-8, g("b"), g("r"), g("z"), g("p"), g("partials"), g("state"), g("hist"), 4)
        elif entry == "update":
            rc = hiplib.spmv_acc_cg_update(n, g("p"), g("q"), g("x"), g("r"), g("partials"), g("state"), g("hist"), 4)
        else:
            rc = hiplib.spmv_acc_cg_direction(n, g("r"), g("z"), g("dinv") if over.pop("jacobi", True) else None, g("p"), g("partials"), g("state"))
        msg = hiplib.spmv_acc_last_error_string().decode()
        hiplib.spmv_acc_clear_error()
        return rc, msg

    def untouched():
        torch.cuda.synchronize()
        return bool((room == -3.0).all()) and bool((small == -3.0).all()) and bool((state == 5).all())

    shifted = lambda name, by: room[names.index(name) * n + by:names.index(name) * n + by + n]  # noqa: E731
    cases = (("start", ("p",), ("b", "r", "z")), ("update", ("x", "r"), ("p", "q")), ("direction", ("z", "p"), ("r", "dinv")))
    for entry, written, read in cases:
        for w in written:
            for other in written + read:
                if other != w:
                    for by in (0, 1, n - 1, -(n - 1)):
                        rc, msg = call(entry, **{w: shifted(other, by)})
                        assert rc == 2 and "overlaps" in msg and f"spmv_acc_cg_{entry}:" in msg, (entry, w, other, by, msg)
            rc, msg = call(entry, **{w: None})
            assert rc == 2 and "null" in msg, (entry, w)
            rc, msg = call(entry, partials=at[w][:6])
            assert rc == 2 and "overlaps" in msg, (entry, w)
        for r_ in read:
            rc, msg = call(entry, **{r_: None} if r_ != "dinv" else dict(r=None))
            assert rc == 2 and "null" in msg, (entry, r_)
        for null in ("partials", "state"):
            assert call(entry, **{null: None})[0] == 2, (entry, null)
    assert call("start", hist=None)[0] == 2 and call("update", hist=None)[0] == 2 and call("start", hist=at["p"][:4])[0] == 2
    with pytest.raises(spmv_acc_amd.SpmvAccError, match="z overlaps r"):
        spmv_acc_amd.cg_direction(n, at["r"], at["r"], at["p"], at["partials"], state, dinv=at["dinv"])
    assert untouched() and hiplib.spmv_acc_last_error() == 0
    # accepted: adjacent vectors (the layout above) and z == r, in the start and in the direction without dinv; the host model's bits
    for name in ("b", "r", "x", "dinv"):
        at[name].copy_(dev(torch, v[name]))
    words = torch.zeros(STATE, dtype=torch.int64, device="cuda")
    spmv_acc_amd.cg_start(n, 1e-8, at["b"], at["r"], at["r"], at["p"], at["partials"], words, at["hist"])
    p, st = host_cg_start(1e-8, v["b"], v["r"], v["r"], None)
    q = v["w"] * p
    at["q"].copy_(dev(torch, q))
    spmv_acc_amd.cg_update(n, at["p"], at["q"], at["x"], at["r"], at["partials"], words, at["hist"])
    x, r, st = host_cg_update(p, q, v["x"], v["r"], st)
    spmv_acc_amd.cg_direction(n, at["r"], at["r"], at["p"], at["partials"], words)
    _, p, st = host_cg_direction(r, r, p, st)
    assert same_bits(at["x"], x) and same_bits(at["r"], r) and same_bits(at["p"], p) and same_state(words, st)
    assert bool((at["z"] == -3.0).all()) and bool((room[:n] == -3.0).all()) and bool((room[8 * n:] == -3.0).all()) and bool((small[10:] == -3.0).all())
    assert hiplib.spmv_acc_last_error() == 0


def device_hierarchy(torch, tag):
    m, (rp, ci, v), theta, coarse_rows, max_levels, near = problem(tag)
    return m, spmv_acc_amd.amg_setup(m, dev(torch, rp), dev(torch, ci), dev(torch, v), theta=theta, omega=OMEGA, coarse_rows=coarse_rows,
                                     max_levels=max_levels, b=None if near is None else dev(torch, near))


@pytest.mark.parametrize("tag", TAGS)
def test_amg_pcg_is_the_host_model(torch_dev, hiplib, tag):
    """pcg with the hierarchy as M at rtol 1e-10: the host's iteration count, every history entry and every iterate -- the solve stopped by
    maxiter = k for each k, which is exact -- within the measured tolerances, the true residual below its bound, and no plan left behind."""
    torch = torch_dev
    want = solve(tag, "amg")
    count = PCG_COUNTS[tag]
    plans = hiplib.spmv_acc_cached_plans()
    m, h = device_hierarchy(torch, tag)
    A = h.levels[0].A
    d_b = dev(torch, rhs(m))
    x = torch.zeros(m, dtype=torch.float64, device="cuda")
    res = spmv_acc_amd.pcg(m, *A, d_b, x, precond=h, rtol=PCG_RTOL, history=True)
    assert res.status == 1 and res.iterations == count == want["iterations"], (tag, res.status, res.iterations)
    assert len(res.history) == count + 1 and res.rr == res.history[-1] and res.bb == float(want["state"]["bb"])  # (b.b has no SpMV in it: the host's bits)
    err = np.max(np.abs(np.array(res.history) - want["history"]) / want["history"])
    assert err <= PCG_HISTORY_TOL, (tag, err)
    true = true_residual(tag, x.cpu().numpy())
    print(f"{tag}: {res.iterations} iterations, true relative residual on the device {true:.3e} (host model {true_residual(tag, want['x']):.3e}), history within {err:.2e}")
    assert true <= PCG_RESIDUAL_BOUND, (tag, true)
    for k in range(1, count + 1):
        x.zero_()
        part = spmv_acc_amd.pcg(m, *A, d_b, x, precond=h, rtol=PCG_RTOL, maxiter=k, check_every=3)
        assert part.iterations == k and part.status == (1 if k == count else 0), (tag, k, part)
        ref = want["iterates"][k - 1]
        err = float(np.max(np.abs(x.cpu().numpy() - ref)) / np.max(np.abs(ref)))
        assert err <= PCG_ITERATE_TOL, (tag, k, err)
    with pytest.raises(spmv_acc_amd.SpmvAccError, match="finest level"):
        spmv_acc_amd.pcg(m - 1, *A, d_b[:m - 1], x[:m - 1], precond=h)
    assert hiplib.spmv_acc_last_error() == 0
    torch.cuda.synchronize()
    assert spmv_acc_amd.check_plans() == 0
    h.release()
    assert hiplib.spmv_acc_cached_plans() == plans and spmv_acc_amd.check_plans() == 0 and hiplib.spmv_acc_last_error() == 0


@pytest.mark.parametrize("tag,kind", IRREGULAR_SOLVES)
def test_amg_pcg_is_the_host_model_on_the_irregular_cases(torch_dev, hiplib, tag, kind):
    """The same on the irregular cases of tests/test_amg_host.py, and (kind "amg22") on fem_weak from a non-zero x0 with pre = post = 2: the
    host's count exactly, every history entry within that entry's own tolerance (history_tolerances), every iterate -- the solve stopped by
    maxiter = k -- within 100 times the host model's spread, the true residual below PCG_RESIDUAL_BOUND, which is also ten times the largest
    of these solves' host figures (7.9e-11) rounded up to a power of ten; no plan left behind."""
    torch = torch_dev
    want = solve(tag, kind)
    count = solve_count(tag, kind)
    options = dict(pre=2, post=2) if kind == "amg22" else {}
    x0 = x0_of(tag) if kind == "amg22" else np.zeros(matrix(tag)[0])
    plans = hiplib.spmv_acc_cached_plans()
    m, h = device_hierarchy(torch, tag)
    A = h.levels[0].A
    d_b = dev(torch, rhs_of(tag))
    x = dev(torch, x0)
    res = spmv_acc_amd.pcg(m, *A, d_b, x, precond=h, rtol=PCG_RTOL, history=True, **options)
    assert res.status == 1 and res.iterations == count == want["iterations"], (tag, kind, res.status, res.iterations)
    assert len(res.history) == count + 1 and res.rr == res.history[-1] and res.bb == float(want["state"]["bb"])
    err = np.abs(np.array(res.history) - want["history"]) / want["history"]
    tols = history_tolerances(tag, kind)
    true = true_residual(tag, x.cpu().numpy())
    print(f"{tag} {kind}: {res.iterations} iterations, true relative residual on the device {true:.3e} (host model {true_residual(tag, want['x']):.3e}), "
          f"history within {err.max():.2e}, at most {np.max(err / tols):.2g} of an entry's tolerance")
    assert np.all(err <= tols), (tag, kind, err, tols)
    assert true <= PCG_RESIDUAL_BOUND, (tag, kind, true)
    worst = 0.0
    for k in range(1, count + 1):
        x.copy_(dev(torch, x0))
        part = spmv_acc_amd.pcg(m, *A, d_b, x, precond=h, rtol=PCG_RTOL, maxiter=k, check_every=3, **options)
        assert part.iterations == k and part.status == (1 if k == count else 0), (tag, kind, k, part)
        ref = want["iterates"][k - 1]
        err = float(np.max(np.abs(x.cpu().numpy() - ref)) / np.max(np.abs(ref)))
        worst = max(worst, err)
        assert err <= 100 * iterate_spread(kind), (tag, kind, k, err)
    print(f"{tag} {kind}: iterates within {worst:.2e}")
    assert hiplib.spmv_acc_last_error() == 0
    torch.cuda.synchronize()
    assert spmv_acc_amd.check_plans() == 0
    h.release()
    assert hiplib.spmv_acc_cached_plans() == plans and spmv_acc_amd.check_plans() == 0 and hiplib.spmv_acc_last_error() == 0


@pytest.fixture(scope="module")
def grid24(torch_dev):
    torch = torch_dev
    m, (rp, ci, v) = matrix("grid24")
    A = (dev(torch, rp), dev(torch, ci), dev(torch, v))
    yield m, A, dev(torch, rhs(m))
    spmv_acc_amd.release_plans(A[0])


def test_plain_and_jacobi_cg_on_grid24(torch_dev, hiplib, grid24):
    torch = torch_dev
    m, A, d_b = grid24
    dinv = spmv_acc_amd.jacobi_inverse(m, *A)
    assert same_bits(dinv, inverse_diagonal("grid24"))
    for kind, precond in (("plain", None), ("jacobi", dinv), ("callable", lambda r, z: torch.mul(dinv, r, out=z))):
        want = solve("grid24", "jacobi" if kind == "callable" else kind)
        x = torch.zeros(m, dtype=torch.float64, device="cuda")
        res = spmv_acc_amd.pcg(m, *A, d_b, x, precond=precond, rtol=CG_RTOL, history=True)
        assert res.status == 1 and abs(res.iterations - CG_COUNTS["jacobi" if kind == "callable" else kind]) <= CG_COUNT_SPREAD + 1, (kind, res.status, res.iterations)
        got, ref = np.array(res.history[:CG_FIRST + 1]), want["history"][:CG_FIRST + 1]
        err = float(np.max(np.abs(got - ref) / ref))
        print(f"{kind}: {res.iterations} iterations (host model {want['iterations']}), first {CG_FIRST} history entries within {err:.2e}")
        assert err <= CG_HISTORY_TOL, (kind, err)
        assert len(res.history) == res.iterations + 1 and res.rr == res.history[-1] and res.rr <= (CG_RTOL * CG_RTOL) * res.bb
    # a row without a diagonal entry is refused
    rp, ci, v = (t.cpu().numpy() for t in A)
    keep = np.ones(ci.size, dtype=bool)
    keep[np.flatnonzero(ci[rp[5]:rp[6]] == 5)[0] + rp[5]] = False
    k_rp = np.concatenate([[0], np.cumsum(np.bincount(np.repeat(np.arange(m), np.diff(rp))[keep], minlength=m))]).astype(np.int32)
    with pytest.raises(spmv_acc_amd.SpmvAccError, match="every row needs one"):
        spmv_acc_amd.jacobi_inverse(m, dev(torch, k_rp), dev(torch, ci[keep]), dev(torch, v[keep]))
    assert hiplib.spmv_acc_last_error() == 0


def test_check_every_independence(torch_dev, hiplib, grid24):
    """On a prepared matrix (both beta classes settled: the engine may change y's last bits once before a plan settles) check_every = 1, 5 and 64
    give the same bits of x and the same count; a maxiter smaller than needed returns status 0 with exactly maxiter iterations."""
    torch = torch_dev
    m, A, d_b = grid24
    nnz = int(A[1].numel())
    dinv = spmv_acc_amd.jacobi_inverse(m, *A)
    x = torch.zeros(m, dtype=torch.float64, device="cuda")
    for beta in (0.0, 1.0):
        spmv_acc_amd.prepare(m, m, nnz, *A, x, beta=beta)
    assert spmv_acc_amd.query_plan(A[0], m)["settled"]
    runs = []
    for check_every in (1, 5, 64):
        x.zero_()
        res = spmv_acc_amd.pcg(m, *A, d_b, x, precond=dinv, rtol=CG_RTOL, check_every=check_every, history=True)
        runs.append((res, x.clone()))
    first, x_first = runs[0]
    assert first.status == 1 and abs(first.iterations - CG_COUNTS["jacobi"]) <= CG_COUNT_SPREAD + 1
    for res, x_k in runs[1:]:
        assert res == first and torch.equal(x_k.view(torch.int64), x_first.view(torch.int64))
    for maxiter in (0, 1, 7, first.iterations - 1):
        x.zero_()
        res = spmv_acc_amd.pcg(m, *A, d_b, x, precond=dinv, rtol=CG_RTOL, maxiter=maxiter, check_every=5, history=True)
        assert res.status == 0 and res.iterations == maxiter and res.history == first.history[:maxiter + 1], (maxiter, res)
    x.zero_()
    res = spmv_acc_amd.pcg(m, *A, d_b, x, precond=dinv, rtol=CG_RTOL, maxiter=first.iterations, check_every=5)
    assert res.status == 1 and res.iterations == first.iterations and torch.equal(x.view(torch.int64), x_first.view(torch.int64))
    assert hiplib.spmv_acc_last_error() == 0
