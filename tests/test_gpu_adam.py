"""GPU: csrc/adam.hip (adam_seg_kernel, adam_kernel) against the float64 statement of the same step (tests/adam_oracle.py), one step
at a time from a known fp32 state, every element of p, exp_avg and exp_avg_sq inside the error bars derived from adam_update's
operations (adam_oracle.bounds); and the Adam variant of sh_flush_kernel (fdgs_adam_step_sh) bit for bit against fdgs_sh_flush +
fdgs_adam_step at the SH kernels' edge shapes.

Every table runs through both kernels: as it is it tiles [0, n) and takes adam_seg_kernel; with its last segment cut one element
short it does not, and takes adam_kernel (the launcher's rule; tests/test_gpu_loss.py::test_adam_segment_kernel_equals_general_kernel
uses the same device).  The last element then lies in no segment: lr = 0, its moments still update."""
import numpy as np
import pytest
import torch

import adam_oracle as ao
from test_gpu_api import _SH_EDGE_IDS, _SH_EDGE_P, _SH_EDGE_TABLE

pytestmark = pytest.mark.gpu

B1, B2, EPS = 0.9, 0.999, 1e-15
FLT_MIN = 2.0 ** -126
ZERO_EVERY, ZERO_AT = 11, 5   # elements 5, 16, 27 ...: m = v = g = 0

# (begin, end, lr, lr_head, period, head).  Boundaries off the float4 grid (all odd); [3, 5) is shorter than a float4 and crosses
# one; [5, 7) lies inside one float4; periods 21, 2, 1, 3, 144 with heads 3, 1, 1, 2, 3; a negative begin (the phase counts from
# -77); [409, 601) has lr = 0; the last segment ends beyond n.  Clipped to [0, n) the table tiles it for every n >= 1.
def _table(n):
    return [(-77, 3, 1e-3, 5e-2, 21, 3), (3, 5, 2e-3, 1e-1, 2, 1), (5, 7, 3e-3, 3e-3, 0, 0), (7, 201, 4e-3, 2e-1, 1, 1),
            (201, 409, 5e-3, 2.5e-1, 3, 2), (409, 601, 0.0, 0.0, 0, 0), (601, 1001, 1.25e-4, 2.5e-3, 144, 3),
            (1001, max(n, 1001) + 50, 1.6e-4, 3e-2, 21, 3)]


def _cut_short(table, n):
    """The table with the segment that holds element n - 1 ending at n - 1: [0, n) is no longer tiled -> adam_kernel."""
    out = list(table)
    for i, (b, e, *rest) in enumerate(table):
        if max(b, 0) <= n - 1 < min(e, n):
            out[i] = (b, n - 1, *rest)
    assert out != list(table)
    return out


def _native(table):
    from fdgs import _capi
    return (_capi.FdgsAdamSegment * len(table))(*[_capi.FdgsAdamSegment(*s) for s in table])


def _inputs(n, seed, fresh=False):
    """p, g, m, v (float32 numpy).  |g| log-uniform in [1e-15, 1], random signs, a fifth exactly 0; m 0 or +-[1e-16, 1e-2]; v 0 or
    [1e-30, 1e-4]; the elements ZERO_AT + k ZERO_EVERY m = v = g = 0.  ``fresh``: m = v = 0 everywhere (the state a run starts from)."""
    rng = np.random.default_rng(seed)
    sign = lambda: rng.choice([-1.0, 1.0], n)   # noqa: E731
    g = 10.0 ** rng.uniform(-15, 0, n) * sign()
    g[rng.permutation(n)[:n // 5]] = 0.0
    m = np.where(rng.random(n) < 0.3, 0.0, 10.0 ** rng.uniform(-16, -2, n) * sign())
    v = np.where(rng.random(n) < 0.3, 0.0, 10.0 ** rng.uniform(-30, -4, n))
    if fresh:
        m[:], v[:] = 0.0, 0.0
    for a in (g, m, v):
        a[ZERO_AT::ZERO_EVERY] = 0.0
    p = rng.standard_normal(n)
    return tuple(a.astype(np.float32) for a in (p, g, m, v))


def _assert_normal(g, m, v):
    """The float64 reference has no model of fp32 underflow: every non-zero term of the moments is a normal fp32 number."""
    g, m, v = (np.abs(np.asarray(a, np.float64)) for a in (g, m, v))
    c1, c2 = 1.0 - float(np.float32(B1)), 1.0 - float(np.float32(B2))
    for name, x in (("(1-b2) g^2", c2 * g * g), ("b2 v", float(np.float32(B2)) * v), ("(1-b1) g", c1 * g), ("b1 m", float(np.float32(B1)) * m)):
        nz = x[x > 0]
        assert nz.size == 0 or nz.min() >= FLT_MIN, (name, nz.min())


def _launch(dev, p, g, m, v, n, native, nseg, step):
    from fdgs import _capi
    rc = _capi.lib.fdgs_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, native, nseg, B1, B2, EPS, step,
                                  _capi.current_stream_handle(dev))
    assert rc == 0, rc


def _one_step(dev, n, table, step, seed, tag):
    """One kernel step from _inputs(n, seed) against the oracle: all of p, m, v inside the bars; what must not move did not."""
    p, g, m, v = _inputs(n, seed)
    _assert_normal(g, m, v)
    for a in (p, g, m, v):
        assert a.nbytes <= 17 * 2 ** 20
    dp, dg, dm, dv = (torch.from_numpy(a).to(dev) for a in (p, g, m, v))
    assert all(t.data_ptr() % 16 == 0 for t in (dp, dg, dm, dv))
    _launch(dev, dp, dg, dm, dv, n, _native(table), len(table), step)
    torch.cuda.synchronize()
    got = tuple(t.cpu().numpy() for t in (dp, dm, dv))
    want = ao.step(p, g, m, v, table, B1, B2, EPS, step)
    bars = ao.bounds(p, g, m, v, table, B1, B2, EPS, step)
    r = ao.ratios(got, want, bars)
    print("%s n=%d step=%d: max |hip - f64| / bound  p %.3f  m %.3f  v %.3f" % (tag, n, step, *r))
    assert all(np.isfinite(a).all() for a in got)
    assert max(r) <= 1.0, (tag, n, r)
    lr = ao.lr_table(n, table)
    still = (lr == 0) | ((g == 0) & (m == 0) & (v == 0))
    assert np.array_equal(got[0][still].view(np.uint32), p[still].view(np.uint32))    # lr = 0, or nothing to move by: p bit-unchanged
    # (that the moments update under lr = 0 as anywhere else is what their bars say: a moment left alone is off by (1-b) |m - g|)
    return got, still


KERNELS = ["segment", "general"]


def _table_for(kernel, n):
    return _table(n) if kernel == "segment" else _cut_short(_table(n), n)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 1023, 4 * 2503 + 3])
def test_adam_one_step_matches_float64(gpu_device, n, kernel):
    """Sizes below, at and above a float4, 1023 (every segment of the table but the last whole) and 4 * 2503 + 3 (several workgroups,
    a ragged end), step 3."""
    table = _table_for(kernel, n)
    got, still = _one_step(gpu_device, n, table, 3, 100 + n, kernel)
    if n >= 1023:
        assert still[409:601].all() and not still[7:201].all()
    if kernel == "general":
        assert still[n - 1]


def test_adam_segment_kernel_wraps_its_grid(gpu_device):
    """adam_seg_kernel launches min((longest / 4 + 255) / 256 + 1, 256 * 8) workgroups of 256 float4 lanes per segment: a single
    segment of more than 256 * 8 * 256 * 4 = 2,097,152 elements makes its grid-stride loop go round -- here by 300 float4s, and 3
    elements behind the last float4.  The segment has a periodic head (144 / 3), so the phase after the wrap is checked too."""
    n = 2097152 + 4 * 300 + 3
    _one_step(gpu_device, n, [(0, n, 1.25e-4, 2.5e-3, 144, 3)], 2, 7, "segment-wrap")


def test_adam_general_kernel_wraps_its_grid(gpu_device):
    """adam_kernel launches min((n / 4 + 255) / 256 + 1, 256 * 16) workgroups of 256 float4 lanes: n above 256 * 16 * 256 * 4 =
    4,194,304 makes its grid-stride loop go round -- here by 256 float4s, and 3 tail elements.  Four segments, one with a
    periodic head across the wrap, the last one an element short of n (which is what sends the table to this kernel)."""
    n = 4194304 + 1027
    table = [(-5, 1000001, 1e-3, 1e-3, 0, 0), (1000001, 1000003, 0.0, 0.0, 0, 0), (1000003, 3000001, 5e-3, 5e-2, 3, 2),
             (3000001, n - 1, 1.25e-4, 2.5e-3, 144, 3)]
    _one_step(gpu_device, n, table, 2, 8, "general-wrap")


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("steps", [1, 2, 10, 1000, 30000])
def test_adam_step_counts_match_float64_step_by_step(gpu_device, steps, kernel):
    """A run of ``steps`` steps from m = v = 0 with a new gradient each step; every step is compared on its own: the oracle is fed
    the state the kernel itself left, so the one-step bars apply at step 30000 as they do at step 1 (the bias corrections have
    long become 1 there).  The kernel's states are recorded on the device and compared after the run."""
    dev = gpu_device
    n, stride, bank = 37, 40, 64
    table = _table_for(kernel, n)
    native = _native(table)
    p0, _, m0, v0 = _inputs(n, 5, fresh=True)
    gs = np.zeros((bank, stride), np.float32)
    for r in range(bank):
        gs[r, :n] = _inputs(n, 1000 + r)[1]
    dg = torch.from_numpy(gs).to(dev)
    cur = torch.zeros(3, stride, device=dev)
    cur[0, :n] = torch.from_numpy(p0).to(dev)
    hist = torch.empty(steps + 1, 3, stride, device=dev)
    hist[0].copy_(cur)
    ptrs = [cur[i].data_ptr() for i in range(3)]
    gptr = [dg[r].data_ptr() for r in range(bank)]
    assert all(q % 16 == 0 for q in ptrs + gptr)
    from fdgs import _capi
    stream = _capi.current_stream_handle(dev)
    for t in range(1, steps + 1):
        rc = _capi.lib.fdgs_adam_step(ptrs[0], gptr[(t - 1) % bank], ptrs[1], ptrs[2], n, native, len(table), B1, B2, EPS, t, stream)
        assert rc == 0
        hist[t].copy_(cur)
    torch.cuda.synchronize()
    h = hist.cpu().numpy()[:, :, :n]
    g = gs[(np.arange(steps)) % bank, :n]
    p, m, v = h[:-1, 0], h[:-1, 1], h[:-1, 2]
    _assert_normal(g, m, v)
    count = np.arange(1, steps + 1)[:, None]
    want = ao.step(p, g, m, v, table, B1, B2, EPS, count)
    bars = ao.bounds(p, g, m, v, table, B1, B2, EPS, count)
    got = (h[1:, 0], h[1:, 1], h[1:, 2])
    r = ao.ratios(got, want, bars)
    print("%s %d steps: max |hip - f64| / bound  p %.3f  m %.3f  v %.3f" % (kernel, steps, *r))
    assert np.isfinite(h).all()
    assert max(r) <= 1.0, (kernel, steps, r)
    assert (h[:, 1:, ZERO_AT::ZERO_EVERY] == 0).all() and (h[:, 0, ZERO_AT::ZERO_EVERY] == p0[ZERO_AT::ZERO_EVERY]).all()
    fed = (ao.lr_table(n, table) > 0) & (np.arange(n) % ZERO_EVERY != ZERO_AT)
    assert steps < 10 or (h[-1, 0][fed] != p0[fed]).all()


def test_adam_tiny_gradients_stay_finite(gpu_device):
    """|g| down to 1e-30: (1-b2) g^2 underflows in fp32, which the float64 oracle does not model.  This test checks nothing more
    than that p, m and v stay finite and that p moves by no more than lr / (1 - b1^t) * |m'| / eps, for both kernels."""
    n, step = 257, 1
    rng = np.random.default_rng(3)
    g = (10.0 ** rng.uniform(-30, -10, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    g[::5] = 0
    p = rng.standard_normal(n).astype(np.float32)
    for kernel in KERNELS:
        table = _table_for(kernel, n)
        dp, dg = torch.from_numpy(p).to(gpu_device), torch.from_numpy(g).to(gpu_device)
        dm, dv = torch.zeros_like(dp), torch.zeros_like(dp)
        _launch(gpu_device, dp, dg, dm, dv, n, _native(table), len(table), step)
        torch.cuda.synchronize()
        gp, gm, gv = (t.cpu().numpy().astype(np.float64) for t in (dp, dm, dv))
        assert np.isfinite(gp).all() and np.isfinite(gm).all() and np.isfinite(gv).all()
        lr = ao.lr_table(n, table)
        bc1 = 1.0 - float(np.float32(B1)) ** step
        limit = lr / bc1 * np.abs(gm) / float(np.float32(EPS))
        assert (np.abs(gp - p) <= limit * (1 + 1e-6) + 2.0 ** -23 * (np.abs(p) + limit)).all()   # (+ the rounding of p' itself)


_FUSED_P = _SH_EDGE_P + [64, 128, 129]


@pytest.mark.parametrize("P", _FUSED_P)
@pytest.mark.parametrize("D,D_t,M,sh3d,misaligned", _SH_EDGE_TABLE, ids=_SH_EDGE_IDS)
def test_sh_adam_fused_edge_shapes_bitwise(gpu_device, D, D_t, M, sh3d, misaligned, P):
    """fdgs_adam_step_sh against fdgs_sh_flush + fdgs_adam_step on copies, at the shapes the flush is pinned at (plus one wave, two
    waves, one past two) with 1, 2, 5 and 9 staged views, two steps each: gradient, parameters and both moments bit-identical.
    fdgs_adam_step is held to float64 above and the flush is pinned bit for bit in tests/test_gpu_api.py, so this closes the fused
    kernel transitively.  A row the launcher refuses (3 M floats are not whole float4s, or the coefficients are not 16-byte
    aligned) is answered FDGS_ERR_INVALID_ARG with every buffer bit-unchanged."""
    from fdgs import _capi
    dev = gpu_device
    gdim = 3 if sh3d else 4
    lr, lr_dc = 1.25e-4, 2.5e-3
    gen = torch.Generator(device="cpu").manual_seed(7000 + 100 * M + P)
    NV = 9
    stages = torch.randn(NV, P, 8, generator=gen)
    stages[:, :, 3] = torch.rand(NV, P, generator=gen) * 2 - 1
    stages[:, :, 7] = torch.rand(NV, P, generator=gen) * 2 - 1
    stages[:, :, 4:7] = torch.nn.functional.normalize(stages[:, :, 4:7], dim=-1)
    dead = torch.rand(NV, P, generator=gen) < 0.4
    stages[:, :, 0:3][dead] = 0.0
    n = P * M * 3
    off = 1 if misaligned else 0

    def fresh():
        g = torch.Generator(device="cpu").manual_seed(5)
        out = []
        for scale, fn in ((1.0, torch.randn), (0.01, torch.randn), (1e-4, torch.rand)):
            store = torch.zeros(n + 4, device=dev)
            t = store[off:off + n].view(P, M, 3)
            t.copy_((scale * fn(P, M, 3, generator=g)).to(dev))
            out.append(t)
        return out
    refused = (3 * M) % 4 != 0 or misaligned
    for nv in (1, 2, 5, 9):
        st = stages[:nv].to(dev).contiguous()
        pa, ma, va = fresh()
        pf, mf, vf = fresh()
        assert (pf.data_ptr() % 16 != 0) == misaligned
        ga = torch.full((P, M, 3), float("nan"), device=dev)
        gf = torch.full((P, M, 3), float("nan"), device=dev)
        if refused:
            before = [t.clone() for t in (pf, mf, vf)]
            with torch.cuda.device(dev):
                rc = _capi.lib.fdgs_adam_step_sh(pf.data_ptr(), mf.data_ptr(), vf.data_ptr(), gf.data_ptr(), P, D, D_t, M, gdim, int(sh3d), 0, nv,
                                                 st.data_ptr(), lr, lr_dc, B1, B2, EPS, 1, _capi.current_stream_handle(dev))
            assert rc == 1   # FDGS_ERR_INVALID_ARG
            assert not _capi.adam_step_sh(pf, mf, vf, st, D, D_t, gdim, sh3d, False, lr, lr_dc, B1, B2, EPS, 1, dL_dsh=gf)
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(before, (pf, mf, vf))) and bool(torch.isnan(gf).all())
            continue
        seg = _native([(0, n, lr, lr_dc, M * 3, 3)])
        for step in (1, 2):
            _capi.sh_flush(st, ga, D, D_t, gdim, sh3d, False)
            _launch(dev, pa, ga, ma, va, n, seg, 1, step)
            assert _capi.adam_step_sh(pf, mf, vf, st, D, D_t, gdim, sh3d, False, lr, lr_dc, B1, B2, EPS, step, dL_dsh=gf)
            torch.cuda.synchronize()
            assert torch.isfinite(ga).all() and torch.equal(ga, gf), (nv, step)
            assert torch.equal(ma, mf) and torch.equal(va, vf) and torch.equal(pa, pf), (nv, step)
        assert bool((ga != 0).any()) or P == 1
