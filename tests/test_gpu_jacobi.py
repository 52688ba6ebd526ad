"""GPU suite (-m gpu) of the damped Jacobi / l1-Jacobi smoother (spmv_acc_csr_jacobi_diagonal / csr_jacobi_diagonal,
spmv_acc_csr_jacobi_sweep / csr_jacobi_sweep): both inverse diagonals and the sweep in its four modes bit for bit against the definitions
restated in numpy (tests/test_jacobi_host.py host_jacobi_diagonal, host_jacobi_sweep) on the cases of the Gauss-Seidel suite; that nothing
outside the outputs is written; the contract on crafted arrays; a captured and replayed chain; non-finite and subnormal inputs; grid striding;
and that l1 sweeps smooth an SPD system.

No speed gate: the parent commit cannot do this job, so there is no figure to hold (tools/jacobi_bench.py measures)."""
import ctypes
import functools

import numpy as np
import pytest

import spmv_acc_amd
from special_values import BIG_VALUE, BIG_X, POISON, TINY
from test_gs_host import TAGS, cases
from test_jacobi_host import KINDS, dense, host_jacobi_diagonal, host_jacobi_sweep

pytestmark = pytest.mark.gpu

PAD = 64
FILL = 7.25


@pytest.fixture(scope="module")
def torch_dev(hiplib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_csr(torch, csr):
    return tuple(dev(torch, a) for a in csr)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(t, a):
    """the same bits, NaNs by position (a NaN's payload and sign are not part of the contract: the division and the adds may quiet or keep them)"""
    got, want = t.cpu().numpy(), np.asarray(a, dtype=np.float64)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


def padded(torch, m):
    """(buffer, view): m doubles with PAD poisoned doubles on either side"""
    buf = torch.full((m + 2 * PAD,), FILL, dtype=torch.float64, device="cuda")
    return buf, buf[PAD:PAD + m]


def padding_untouched(buf, m):
    return bool((buf[:PAD] == FILL).all()) and bool((buf[PAD + m:] == FILL).all())


@functools.lru_cache(maxsize=None)
def vectors(tag):
    m = cases()[tag][0]
    rng = np.random.default_rng(300 + m)
    return rng.standard_normal(m), rng.standard_normal(m)


@functools.lru_cache(maxsize=None)
def inverse(tag, kind):
    m, (rp, ci, v) = cases()[tag]
    return host_jacobi_diagonal(m, rp, ci, v, kind)


@pytest.mark.parametrize("tag", TAGS)
def test_diagonal_is_the_host_model(torch_dev, hiplib, tag):
    torch = torch_dev
    m, (rp, ci, v) = cases()[tag]
    d_A = dev_csr(torch, (rp, ci, v))
    plans = hiplib.spmv_acc_cached_plans()
    for kind in KINDS:
        want = inverse(tag, kind)
        assert np.all(np.isfinite(want)), (tag, kind)  # (same_bits pairs NaNs by position: these cases hold none, so the compare is strict)
        for _ in range(2):  # twice: the same bits
            got = spmv_acc_amd.csr_jacobi_diagonal(m, *d_A, kind=kind)
            assert got.numel() == m and got.dtype == torch.float64 and same_bits(got, want), (tag, kind)
        # the C entry into the middle of a poisoned buffer: nothing outside dinv (and work) is written
        buf, out = padded(torch, m)
        wbuf, work = padded(torch, m)
        hiplib.spmv_acc_set_stream(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        rc = hiplib.spmv_acc_csr_jacobi_diagonal(m, ci.size, ptr(d_A[0]), ptr(d_A[1]) if ci.size else None, ptr(d_A[2]) if ci.size else None,
                                                 KINDS.index(kind), ptr(out) if m else None, ptr(work) if m and kind == "l1" else None)
        torch.cuda.synchronize()
        assert rc == 0, (rc, hiplib.spmv_acc_last_error_string())
        assert same_bits(out, want) and padding_untouched(buf, m) and padding_untouched(wbuf, m), (tag, kind)
        if kind == "jacobi":
            assert bool((work == FILL).all())  # kind 0 does not use the work vector
    assert hiplib.spmv_acc_cached_plans() == plans and hiplib.spmv_acc_last_error() == 0


@pytest.mark.parametrize("tag", TAGS)
def test_sweep_is_the_host_model(torch_dev, hiplib, tag):
    """omega = 1 and 0.7 in all four modes: x_out only, r_out only, both, and the zero start."""
    torch = torch_dev
    m, (rp, ci, v) = cases()[tag]
    b, x0 = vectors(tag)
    d_A = dev_csr(torch, (rp, ci, v))
    d_b, d_x = dev(torch, b), dev(torch, x0)
    plans = hiplib.spmv_acc_cached_plans()
    for kind, omega in (("l1", 1.0), ("jacobi", 0.7), ("l1", 0.7)):
        dinv = inverse(tag, kind)
        d_dinv = dev(torch, dinv)
        want_x, want_r = host_jacobi_sweep(m, rp, ci, v, dinv, b, x0, omega)
        zero_x, zero_r = host_jacobi_sweep(m, rp, ci, v, dinv, b, None, omega)
        assert all(np.all(np.isfinite(a)) for a in (dinv, want_x, want_r, zero_x, zero_r)), (tag, kind)  # (no NaN: same_bits is strict here)
        for mode in ("x", "r", "both", "zero", "zero both"):
            for _ in range(2):  # twice: the same bits
                xbuf, x_out = padded(torch, m)
                rbuf, r_out = padded(torch, m)
                spmv_acc_amd.csr_jacobi_sweep(m, *d_A, d_dinv, d_b, None if mode.startswith("zero") else d_x,
                                              x_out=None if mode == "r" else x_out, r_out=r_out if mode in ("r", "both", "zero both") else None,
                                              omega=omega)
                torch.cuda.synchronize()
                wx, wr = (zero_x, zero_r) if mode.startswith("zero") else (want_x, want_r)
                if mode != "r":
                    assert same_bits(x_out, wx), (tag, kind, omega, mode)
                else:
                    assert bool((x_out == FILL).all())
                if mode in ("r", "both", "zero both"):
                    assert same_bits(r_out, wr), (tag, kind, omega, mode)
                else:
                    assert bool((r_out == FILL).all())
                assert padding_untouched(xbuf, m) and padding_untouched(rbuf, m), (tag, mode)
        assert same_bits(d_x, x0) and same_bits(d_b, b) and same_bits(d_dinv, dinv)  # the inputs are unchanged
    assert hiplib.spmv_acc_cached_plans() == plans and hiplib.spmv_acc_last_error() == 0


def test_sweep_contract(torch_dev, hiplib):
    """Overlaps are refused with nothing written; columns outside [0, m) and extents that descend or leave the arrays neither fault nor read
    outside (clamped extents, +0.0 terms) and give the host model's bits."""
    torch = torch_dev
    m, (rp, ci, v) = cases()["fem"]
    nnz = ci.size
    b, x0 = vectors("fem")
    dinv = inverse("fem", "l1")
    d_A = dev_csr(torch, (rp, ci, v))
    d_b, d_x, d_dinv = dev(torch, b), dev(torch, x0), dev(torch, dinv)
    xbuf, x_out = padded(torch, m)
    rbuf, r_out = padded(torch, m)
    hiplib.spmv_acc_set_stream(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    def call(mm=m, dv=d_dinv, bb=d_b, xi=d_x, xo=x_out, ro=r_out, omega=1.0):
        rc = hiplib.spmv_acc_csr_jacobi_sweep(mm, nnz, ptr(d_A[0]), ptr(d_A[1]), ptr(d_A[2]), ptr(dv), omega, ptr(bb), ptr(xi), ptr(xo), ptr(ro))
        msg = hiplib.spmv_acc_last_error_string().decode()
        hiplib.spmv_acc_clear_error()
        return rc, msg

    for bad in (dict(xo=d_x), dict(xo=d_b), dict(xo=d_dinv), dict(ro=d_x), dict(ro=d_b), dict(ro=d_dinv), dict(ro=x_out), dict(xi=d_b),
                dict(xo=xbuf[PAD - 1:], ro=x_out), dict(ro=xbuf[PAD + m - 1:]), dict(dv=d_b), dict(dv=d_x)):
        rc, msg = call(**bad)
        assert rc == 2 and "overlaps" in msg and "out of place" in msg, (list(bad), rc, msg)
    assert call(xo=None, ro=None)[0] == 2 and call(omega=float("nan"))[0] == 2 and call(mm=2 ** 29 + 1)[0] == 4 and call(mm=-1)[0] == 2
    torch.cuda.synchronize()
    assert bool((xbuf == FILL).all()) and bool((rbuf == FILL).all()) and same_bits(d_x, x0) and same_bits(d_b, b) and same_bits(d_dinv, dinv)
    with pytest.raises(spmv_acc_amd.SpmvAccError, match="overlaps"):
        spmv_acc_amd.csr_jacobi_sweep(m, *d_A, d_dinv, d_b, d_x, x_out=d_x)
    assert hiplib.spmv_acc_last_error() == 0
    # crafted arrays: columns outside [0, m), a descending extent, extents that leave [0, nnz]
    rng = np.random.default_rng(41)
    bad_ci = ci.copy()
    hit = rng.choice(nnz, 60, replace=False)
    bad_ci[hit] = np.array([-1, m, m + 9, 2 ** 31 - 1, -2 ** 31, -m] * 10, dtype=np.int64).astype(np.int32)
    bad_rp = rp.copy()
    bad_rp[7], bad_rp[200], bad_rp[301] = -5, nnz + 1000, rp[300] - 3
    d_bad = (dev(torch, bad_rp), dev(torch, bad_ci), d_A[2])
    for kind in KINDS:
        want_d = host_jacobi_diagonal(m, bad_rp, bad_ci, v, kind)
        got_d = spmv_acc_amd.csr_jacobi_diagonal(m, *d_bad, kind=kind)
        torch.cuda.synchronize()
        assert same_bits(got_d, want_d), kind
    want_x, want_r = host_jacobi_sweep(m, bad_rp, bad_ci, v, dinv, b, x0, 0.7)
    spmv_acc_amd.csr_jacobi_sweep(m, *d_bad, d_dinv, d_b, d_x, x_out=x_out, r_out=r_out, omega=0.7)
    torch.cuda.synchronize()  # (no device-side fault: the context is alive)
    assert same_bits(x_out, want_x) and same_bits(r_out, want_r) and np.all(np.isfinite(want_x))
    assert padding_untouched(xbuf, m) and padding_untouched(rbuf, m)
    assert np.sum(bits(want_r) != bits(host_jacobi_sweep(m, rp, ci, v, dinv, b, x0, 0.7)[1])) >= 30  # the crafted entries changed their rows


def test_captured_and_replayed(torch_dev, hiplib):
    """The diagonal, three ping-pong sweeps (the first from zero) and a residual captured in one graph (one stream, no parallel branches) and
    replayed twice on a changed b: the same bits as the plain calls, and as the host model."""
    torch = torch_dev
    m, (rp, ci, v) = cases()["grid27"]
    d_A = dev_csr(torch, (rp, ci, v))
    b0 = vectors("grid27")[0]
    d_b = dev(torch, b0)
    xa, xb, r = (torch.zeros(m, dtype=torch.float64, device="cuda") for _ in range(3))
    dinv, work = torch.zeros(m, dtype=torch.float64, device="cuda"), torch.zeros(m, dtype=torch.float64, device="cuda")
    nnz = ci.size

    def chain(stream):
        hiplib.spmv_acc_set_stream(ctypes.c_void_p(stream.cuda_stream))
        assert hiplib.spmv_acc_csr_jacobi_diagonal(m, nnz, ptr(d_A[0]), ptr(d_A[1]), ptr(d_A[2]), 1, ptr(dinv), ptr(work)) == 0
        spmv_acc_amd.csr_jacobi_sweep(m, *d_A, dinv, d_b, None, x_out=xa, omega=0.9)
        spmv_acc_amd.csr_jacobi_sweep(m, *d_A, dinv, d_b, xa, x_out=xb, omega=0.9)
        spmv_acc_amd.csr_jacobi_sweep(m, *d_A, dinv, d_b, xb, x_out=xa, omega=0.9)
        spmv_acc_amd.csr_jacobi_sweep(m, *d_A, dinv, d_b, xa, r_out=r, omega=0.9)

    chain(torch.cuda.current_stream())  # (warm: the code objects are loaded outside the capture)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            chain(s)
    rng = np.random.default_rng(5)
    w_dinv = inverse("grid27", "l1")
    for _ in range(2):
        new_b = rng.standard_normal(m)
        d_b.copy_(dev(torch, new_b))
        for t in (xa, xb, r, dinv):
            t.fill_(FILL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        replayed = [t.clone() for t in (dinv, xa, xb, r)]
        for t in (xa, xb, r, dinv):
            t.fill_(FILL)
        chain(torch.cuda.current_stream())
        torch.cuda.synchronize()
        for got, plain in zip(replayed, (dinv, xa, xb, r)):
            assert np.array_equal(bits(got.cpu().numpy()), bits(plain.cpu().numpy()))
        x = host_jacobi_sweep(m, rp, ci, v, w_dinv, new_b, None, 0.9)[0]
        x1 = host_jacobi_sweep(m, rp, ci, v, w_dinv, new_b, x, 0.9)[0]
        x2 = host_jacobi_sweep(m, rp, ci, v, w_dinv, new_b, x1, 0.9)[0]
        assert same_bits(replayed[0], w_dinv) and same_bits(replayed[2], x1) and same_bits(replayed[1], x2)
        assert same_bits(replayed[3], host_jacobi_sweep(m, rp, ci, v, w_dinv, new_b, x2, 0.9)[1])
    del g


def test_special_values(torch_dev):
    """NaN, +-Inf, overflowing products and subnormals in value, x, b and dinv, and zero, subnormal and infinite diagonals, come out as the
    host models say."""
    torch = torch_dev
    for tag in ("fem", "grid27", "star"):
        m, (rp, ci, v) = cases()[tag]
        row = np.repeat(np.arange(m), np.diff(rp))
        b, x0 = (a.copy() for a in vectors(tag))
        v = v.copy()
        diag = np.flatnonzero(ci == row)
        off = np.flatnonzero(ci != row)
        specials = list(POISON) + [TINY, -TINY, 2.0 ** -1030, 0.0, -0.0]
        for k, s in enumerate(specials):
            v[off[(7 * k + 3) % off.size]] = s
            b[(11 * k + 1) % m] = s
            x0[(13 * k + 2) % m] = s
        v[off[5 % off.size]], x0[ci[off[5 % off.size]]] = BIG_VALUE, BIG_X  # a product that overflows
        v[diag[3]], v[diag[9]], v[diag[20]], v[diag[21]] = 0.0, -0.0, TINY, np.inf  # zero diagonals of either sign, a subnormal and an infinite one
        d_A = dev_csr(torch, (rp, ci, v))
        d_b, d_x = dev(torch, b), dev(torch, x0)
        seen = np.zeros(m, dtype=bool)
        for kind, omega in (("jacobi", 0.7), ("l1", 1.0)):
            dinv = host_jacobi_diagonal(m, rp, ci, v, kind)
            got = spmv_acc_amd.csr_jacobi_diagonal(m, *d_A, kind=kind)
            assert same_bits(got, dinv), (tag, kind)
            assert not np.all(np.isfinite(dinv))  # 1 / 0 and 0 / 0 arrived
            for k, s in enumerate(specials):  # ... and the caller's own dinv may hold anything
                dinv[(17 * k + 5) % m] = s
            want_x, want_r = host_jacobi_sweep(m, rp, ci, v, dinv, b, x0, omega)
            x_out, r_out = torch.empty_like(d_x), torch.empty_like(d_x)
            spmv_acc_amd.csr_jacobi_sweep(m, *d_A, dev(torch, dinv), d_b, d_x, x_out=x_out, r_out=r_out, omega=omega)
            assert same_bits(x_out, want_x) and same_bits(r_out, want_r), (tag, kind)
            zero_x, _ = host_jacobi_sweep(m, rp, ci, v, dinv, b, None, omega)
            spmv_acc_amd.csr_jacobi_sweep(m, *d_A, dev(torch, dinv), d_b, None, x_out=x_out, omega=omega)
            assert same_bits(x_out, zero_x), (tag, kind)
            seen |= ~np.isfinite(want_x)
        assert seen.any() and (tag == "star" or not seen.all()), tag  # the poison arrived and, but through the star's hub, did not take every row


def test_jacobi_grid_stride_at_test_size(torch_dev, hiplib):
    """max_grid_blocks lowered to 64, the smallest cap the library honours, as test_gs_grid_stride_at_test_size: the 7-point stencil on
    44 x 44 x 44 (85 184 rows: 1 331 chunks of the sweep and the l1 diagonal, 333 workgroups of rows in the one-row-per-lane kernels) gives
    the same bits as with the default grid."""
    torch = torch_dev
    rng = np.random.default_rng(77)
    n = 44
    idx = np.arange(n ** 3, dtype=np.int64).reshape(n, n, n)
    pairs_i, pairs_j = [idx.reshape(-1)], [idx.reshape(-1)]
    for axis in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, n - 1), slice(1, n)
        a, c = idx[tuple(lo)].reshape(-1), idx[tuple(hi)].reshape(-1)
        pairs_i += [a, c]
        pairs_j += [c, a]
    i, j = np.concatenate(pairs_i), np.concatenate(pairs_j)
    order = np.lexsort((j, i))
    i, j = i[order], j[order]
    m = n ** 3
    rp = np.zeros(m + 1, dtype=np.int32)
    np.cumsum(np.bincount(i, minlength=m), out=rp[1:])
    ci, v = j.astype(np.int32), rng.uniform(0.5, 2.0, j.size)
    b, x0 = rng.standard_normal(m), rng.standard_normal(m)
    d_A = dev_csr(torch, (rp, ci, v))
    d_b, d_x = dev(torch, b), dev(torch, x0)
    assert m > 64 * 256 and (m + 63) // 64 > 64

    def run():
        out = []
        for kind in KINDS:
            dinv = spmv_acc_amd.csr_jacobi_diagonal(m, *d_A, kind=kind)
            x_out, r_out, z_out = (torch.empty_like(d_x) for _ in range(3))
            spmv_acc_amd.csr_jacobi_sweep(m, *d_A, dinv, d_b, d_x, x_out=x_out, r_out=r_out, omega=0.7)
            spmv_acc_amd.csr_jacobi_sweep(m, *d_A, dinv, d_b, None, x_out=z_out, omega=0.7)
            torch.cuda.synchronize()
            out += [t.cpu().numpy() for t in (dinv, x_out, r_out, z_out)]
        return out

    default = run()
    try:
        assert hiplib.spmv_acc_set_tunable(b"max_grid_blocks", 64) == 0
        strided = run()
    finally:
        hiplib.spmv_acc_reset_tunables()
    for a, c in zip(default, strided):
        assert np.array_equal(bits(a), bits(c))
    # ... and they are the definition's (the host model on 85 184 rows takes a second or two)
    w_dinv = host_jacobi_diagonal(m, rp, ci, v, "l1")
    want_x, want_r = host_jacobi_sweep(m, rp, ci, v, w_dinv, b, x0, 0.7)
    assert np.array_equal(bits(default[4]), bits(w_dinv)) and np.array_equal(bits(default[5]), bits(want_x)) and np.array_equal(bits(default[6]), bits(want_r))


def test_l1_sweeps_smooth(torch_dev, hiplib):
    """The SPD 7-point matrix with b = A x*: each of ten l1 sweeps at omega = 1 reduces the energy norm of the error -- the theorem for
    D >= A -- and is the host model's to the bit."""
    torch = torch_dev
    m, A = cases()["grid7"]
    rp, ci, v = A
    D = dense(m, A)
    star = np.random.default_rng(17).standard_normal(m)
    b = np.asarray(D @ star.astype(np.longdouble), dtype=np.float64)
    d_A = dev_csr(torch, A)
    d_b = dev(torch, b)
    dinv = spmv_acc_amd.csr_jacobi_diagonal(m, *d_A, kind="l1")
    w_dinv = inverse("grid7", "l1")

    def energy(e):
        e = e.astype(np.longdouble)
        return float(np.sqrt(e @ (D @ e)))

    cur, other = torch.zeros(m, dtype=torch.float64, device="cuda"), torch.zeros(m, dtype=torch.float64, device="cuda")
    model = np.zeros(m)
    norms = [energy(-star)]
    for _ in range(10):
        spmv_acc_amd.csr_jacobi_sweep(m, *d_A, dinv, d_b, cur, x_out=other)
        cur, other = other, cur
        model = host_jacobi_sweep(m, rp, ci, v, w_dinv, b, model, 1.0)[0]
        assert same_bits(cur, model)
        norms.append(energy(cur.cpu().numpy() - star))
    print(f"energy norms of the error {['%.6e' % n for n in norms]}")
    assert all(later < earlier for earlier, later in zip(norms, norms[1:])), norms
