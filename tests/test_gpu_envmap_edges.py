"""GPU: csrc/envmap.hip through its C ABI (fdgs_env_composite, fdgs_env_composite_backward) on the cases of tests/envmap_cases.py,
element by element against the float64 statement of tests/envmap_oracle.py (reference, atan2 form), at the derived bars of
envmap_oracle.bars: seam and pole pixels included, images below, at and above a tile, maps down to 1 x 1, the LDS-window path up to
its 3072-texel limit and the direct-atomics path beyond it.  No pixel and no texel is exempt (tests/test_envmap_cases_host.py
asserts that no case puts a pixel on the seam itself).  Every output lies between guard bands; the worst error / bar ratios are printed."""
import numpy as np
import pytest
import torch

import envmap_cases as ec
import envmap_oracle as eo
from guarded import Guarded

pytestmark = pytest.mark.gpu

NAMES = [c["name"] for c in ec.CASES]
WORST = {}


def _ratio(tag, got, want, bar, what):
    """Every element of ``got`` within ``bar`` of ``want`` (an error of exactly 0 passes a bar of 0); returns the worst ratio."""
    got = np.asarray(got, np.float64).reshape(want.shape)
    assert np.isfinite(got).all(), "%s: %d non-finite elements" % (what, int((~np.isfinite(got)).sum()))
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bar)
    worst = float(r.max())
    WORST[tag] = max(WORST.get(tag, 0.0), worst)
    at = np.unravel_index(int(np.argmax(r)), r.shape)
    assert worst <= 1.0, "%s: element %s is %.3g from the reference %.9g, bar %.3g (ratio %.3g); %d of %d elements beyond their bar" % (
        what, at, err[at], want[at], bar[at], worst, int((r > 1.0).sum()), r.size)
    return worst


def _bits(x):
    return x.contiguous().view(torch.int32)


class _Device:
    """The case's inputs on the device and the two entry points with raw pointers."""

    def __init__(self, d, dev):
        from fdgs import _capi
        self.capi, self.dev, c = _capi, dev, d["case"]
        self.H, self.W, self.eh, self.ew = c["H"], c["W"], c["eh"], c["ew"]
        cam = d["cam"]
        self.vm = cam.world_view_transform.detach().float().contiguous().to(dev)
        self.cp = cam.camera_center.detach().float().contiguous().to(dev)
        self.intr = (float(cam.fl_x), float(cam.fl_y), float(cam.cx), float(cam.cy))
        self.colour, self.T, self.g, self.env = (torch.from_numpy(d[k]).contiguous().to(dev) for k in ("colour", "T", "g", "env"))
        self.prior_alpha, self.prior_env = torch.from_numpy(d["prior_alpha"]).to(dev), torch.from_numpy(d["prior_env"]).to(dev)

    def forward(self, colour_in_ptr, out_ptr):
        self.capi.call("fdgs_env_composite", self.dev, self.H, self.W, self.vm.data_ptr(), self.cp.data_ptr(), *self.intr, self.env.data_ptr(),
                       self.eh, self.ew, ec.R, self.T.data_ptr(), colour_in_ptr, out_ptr)
        torch.cuda.synchronize()

    def backward(self, ga_ptr, acc_alpha, ge_ptr, acc_env):
        self.capi.call("fdgs_env_composite_backward", self.dev, self.H, self.W, self.vm.data_ptr(), self.cp.data_ptr(), *self.intr,
                       self.env.data_ptr(), self.eh, self.ew, ec.R, self.T.data_ptr(), self.g.data_ptr(), ga_ptr, int(acc_alpha), ge_ptr,
                       int(acc_env))
        torch.cuda.synchronize()


@pytest.mark.parametrize("name", NAMES)
def test_forward_every_pixel_within_its_bar(name, gpu_device):
    """colour_out between guard bands: every element written and finite, every guard element intact, every element within
    8 u (|colour| + T E_c) + 4 delta T max_k |env_ck| of the float64 reference; colour_out aliasing colour_in gives the same bits."""
    d = ec.build(name)
    x = _Device(d, gpu_device)
    out = Guarded(3 * x.H * x.W, gpu_device)
    x.forward(x.colour.data_ptr(), out.ptr)
    got = out.check("colour_out").clone()
    r = _ratio("forward", got.cpu().numpy(), d["out"], d["bar_out"], name + " colour_out")
    inplace = Guarded(3 * x.H * x.W, gpu_device)
    inplace.body().copy_(x.colour.view(-1))
    x.forward(inplace.ptr, inplace.ptr)
    assert torch.equal(_bits(inplace.check("colour_out in place")), _bits(got)), "in place differs from out of place"
    print("%-40s forward worst ratio %.3f" % (name, r))


@pytest.mark.parametrize("name", NAMES)
def test_backward_every_element_within_its_bar(name, gpu_device):
    """g_alpha and g_env between guard bands, both in one launch: written, finite, guards intact, every pixel of d / d alpha within
    8 u sum_c |g_c| E_c + 4 delta sum_c |g_c| max_k |env_ck| and every texel of d / d env within (n + 2) u A + 2 delta B; a texel
    with n = 0 is exactly +0.  d / d alpha is the same bits in a second run, alone (g_env = NULL) and beside g_env; g_env alone
    stays within the bar."""
    d = ec.build(name)
    x = _Device(d, gpu_device)
    HW, ne = x.H * x.W, 3 * x.eh * x.ew
    ga, ge = Guarded(HW, gpu_device), Guarded(ne, gpu_device)
    x.backward(ga.ptr, False, ge.ptr, False)
    a, e = ga.check("g_alpha").clone(), ge.check("g_env").clone()
    ra = _ratio("d_alpha", a.cpu().numpy(), d["ga"], d["bar_ga"], name + " g_alpha")
    re = _ratio("d_env", e.cpu().numpy(), d["ge"], d["bar_ge"], name + " g_env")
    zero = torch.from_numpy(d["n"] == 0).to(gpu_device)
    assert not _bits(e).view(3, x.eh, x.ew)[:, zero].any(), "a texel no pixel contributes to is not exactly +0"
    # again, both: d / d alpha has no atomics
    ga2, ge2 = Guarded(HW, gpu_device), Guarded(ne, gpu_device)
    x.backward(ga2.ptr, False, ge2.ptr, False)
    assert torch.equal(_bits(ga2.check("g_alpha, second run")), _bits(a)), "d / d alpha differs between two runs"
    _ratio("d_env", ge2.check("g_env, second run").cpu().numpy(), d["ge"], d["bar_ge"], name + " g_env, second run")
    # either one alone
    ga3, ge3 = Guarded(HW, gpu_device), Guarded(ne, gpu_device)
    x.backward(ga3.ptr, False, None, False)
    assert torch.equal(_bits(ga3.check("g_alpha alone")), _bits(a)), "d / d alpha alone differs from d / d alpha beside g_env"
    x.backward(None, False, ge3.ptr, False)
    ge3.check("g_env alone")
    ga3.check("g_alpha after the g_env-only launch")
    assert torch.equal(_bits(ga3.body()), _bits(a))
    _ratio("d_env", ge3.body().cpu().numpy(), d["ge"], d["bar_ge"], name + " g_env alone")
    print("%-40s d_alpha worst ratio %.3f   d_env worst ratio %.3f   (%d of %d texels untouched)" % (name, ra, re, int(zero.sum()), x.eh * x.ew))


@pytest.mark.parametrize("name", NAMES)
def test_accumulate_adds_to_the_prior(name, gpu_device):
    """accumulate_alpha: d / d alpha is fl32(prior + ga) bit for bit.  accumulate_env: every texel within (n + 2) u (A + |prior|) +
    2 delta B of prior + d / d env, and a texel with n = 0 keeps exactly its prior's bits.  Guards intact."""
    d = ec.build(name)
    x = _Device(d, gpu_device)
    HW, ne = x.H * x.W, 3 * x.eh * x.ew
    plain = Guarded(HW, gpu_device)
    x.backward(plain.ptr, False, None, False)
    ga, ge = Guarded(HW, gpu_device), Guarded(ne, gpu_device)
    ga.body().copy_(x.prior_alpha.view(-1))
    ge.body().copy_(x.prior_env.view(-1))
    x.backward(ga.ptr, True, ge.ptr, True)
    a, e = ga.check("g_alpha"), ge.check("g_env")
    assert torch.equal(_bits(a), _bits(x.prior_alpha.view(-1) + plain.check("g_alpha, written"))), "accumulate_alpha is not fl32(prior + ga)"
    r = _ratio("d_env accumulate", e.cpu().numpy(), d["ge_acc"], d["bar_ge_acc"], name + " g_env, accumulate")
    zero = torch.from_numpy(d["n"] == 0).to(gpu_device)
    assert torch.equal(_bits(e).view(3, x.eh, x.ew)[:, zero], _bits(x.prior_env)[:, zero]), "accumulate changed a texel no pixel contributes to"
    # accumulate on one output only leaves the other one's rule alone: alpha written, env added
    ga2, ge2 = Guarded(HW, gpu_device), Guarded(ne, gpu_device)
    ge2.body().copy_(x.prior_env.view(-1))
    x.backward(ga2.ptr, False, ge2.ptr, True)
    assert torch.equal(_bits(ga2.check("g_alpha")), _bits(plain.body()))
    _ratio("d_env accumulate", ge2.check("g_env").cpu().numpy(), d["ge_acc"], d["bar_ge_acc"], name + " g_env, accumulate_env only")
    print("%-40s d_env (accumulate) worst ratio %.3f" % (name, r))


def test_autograd_with_non_contiguous_inputs(gpu_device):
    """fdgs.envmap.env_composite on the 17 x 19 seam case: colour, alpha and the upstream gradient as transposed views give the bits
    (image, d / d colour, d / d alpha) and, within the bar, the d / d env of contiguous inputs; all of it within the bars."""
    from fdgs.envmap import env_composite
    d = ec.build("seam-17x19-map40x72-signed")
    c = d["case"]
    H, W = c["H"], c["W"]
    dev = gpu_device
    cam = d["cam"].to(dev)
    colour, env, g = (torch.from_numpy(d[k]).to(dev) for k in ("colour", "env", "g"))
    alpha = (1 - torch.from_numpy(d["T"])).to(dev)
    T = (1 - alpha).cpu().numpy()                               # what the autograd function hands the kernels
    want_out, want_ga, want_ge = eo.reference(d["taps"], d["colour"], T, d["env"], d["g"])
    bar_out, bar_ga, bar_ge, _ = eo.bars(d["taps"], d["colour"], T, d["env"], d["g"], ec.DELTA)

    def view(t):
        v = t.transpose(-1, -2).contiguous().transpose(-1, -2)
        assert not v.is_contiguous() and torch.equal(v, t)
        return v

    runs = []
    for f in (lambda t: t.clone(), view):
        ci, ai, ei = f(colour).requires_grad_(True), f(alpha).requires_grad_(True), env.clone().requires_grad_(True)
        out = env_composite(ci, ai, ei, cam)
        out.backward(gradient=f(g))
        torch.cuda.synchronize()
        runs.append((out.detach(), ci.grad, ai.grad, ei.grad))
        _ratio("forward", out.detach().cpu().numpy(), want_out, bar_out, "autograd image")
        _ratio("d_alpha", ai.grad.cpu().numpy(), want_ga.reshape(1, H, W), bar_ga.reshape(1, H, W), "autograd d / d alpha")
        _ratio("d_env", ei.grad.cpu().numpy(), want_ge, bar_ge, "autograd d / d env")
        assert torch.equal(ci.grad, g)
    for k in range(3):
        assert torch.equal(_bits(runs[0][k]), _bits(runs[1][k])), ("image", "d / d colour", "d / d alpha")[k]


def test_worst_ratios_are_reported():
    """Not a check of its own: prints the worst error / bar ratio per output the tests above observed (DESIGN.md records them)."""
    for k, v in sorted(WORST.items()):
        print("worst ratio %-18s %.3f" % (k, v))
