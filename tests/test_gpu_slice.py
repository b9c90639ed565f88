"""GPU: fdgs.slice.time_slice / render_slice (csrc/time_slice.hip) -- bit for bit against the forward's preprocess, live set and order
against the float64 statement (tests/slice_oracle.py), folded SH rows at a per-element error bar, pixels against the CPU oracle,
the in-kernel eigen-decomposition against numpy's float32 eigh, and the bookkeeping of render_slice."""
import functools

import numpy as np
import pytest
import torch

import slice_oracle as so
import util
from fdgs import synth

pytestmark = pytest.mark.gpu

W, H = 96, 64
SIZES = (1, 63, 64, 65, 257, 4099)
# (prefilter_var, scaling modifier): both values of both, every pairing at P = 257
COMBOS = ((-1.0, 1.0), (0.02, 0.7))
COMBOS_ALL = ((-1.0, 1.0), (0.02, 0.7), (-1.0, 0.7), (0.02, 1.0))
T_FRAC = 0.4


class _Cam:
    def __init__(self, scene, dev):
        self.FoVx, self.FoVy, self.image_height, self.image_width = scene["FoVx"], scene["FoVy"], scene["H"], scene["W"]
        self.world_view_transform = scene["world_view_transform"].to(dev)
        self.full_proj_transform = scene["full_proj_transform"].to(dev)
        self.camera_center = scene["camera_center"].to(dev)
        self.timestamp = scene["timestamp"]


class _Pipe:
    compute_cov3D_python = convert_SHs_python = debug = False
    env_map_res = 0


def make_scene(P, rot_4d, D=0, D_t=0, seed=3, alloc=None, force_sh_3d=False, pose="rig1"):
    """A 4D scene of duration 1 whose temporal extent leaves about half of the Gaussians live at t = 0.4: sigma_t ~ 0.13 with
    rot_4d; without it scales_t IS the variance (the reference's quirk), ~ 0.02."""
    cfg = synth.SceneConfig("slice", P, W, H, D, D_t, 0.03, 1.0, rot_4d, 4, force_sh_3d)
    return synth.make_scene(cfg, seed=seed, bg=(0.1, 0.2, 0.3), pose=pose, alloc=alloc, timestamp_frac=T_FRAC,
                            st_scale=0.3 if rot_4d else 0.05)


def make_model(scene, dev, prefilter_var=-1.0):
    from fdgs.train_host import GaussianParams
    m = GaussianParams(scene, dev)
    m.prefilter_var = prefilter_var
    return m


def raw_numpy(model):
    return {k: v.detach().cpu().numpy() for k, v in model.params.items()}


def oracle_of(model, t, mod=1.0):
    return so.slice_oracle(so.activate(raw_numpy(model)), t, mod=mod, prefilter_var=model.prefilter_var, rot_4d=model.rot_4d,
                           D=model.active_sh_degree, D_t=model.active_sh_degree_t, T=model.time_duration[1] - model.time_duration[0],
                           force_sh_3d=model.force_sh_3d)


def activated_scene(scene, model):
    """``scene`` with the activations the kernels derive in flight from the model's raw fp32 parameters, bit for bit
    (fdgs_debug_activations): what the CPU oracle is fed, so that its bit-exact outputs (radii) stay bit-exact."""
    from fdgs import _capi
    r = {k: v.detach() for k, v in model.params.items()}
    op, sc, sct, rot, rot_r = (t.cpu() for t in _capi.debug_activations(r["_opacity"], r["_scaling"], r["_scaling_t"], r["_rotation"], r["_rotation_r"]))
    out = dict(scene)
    out.update(means3D=r["_xyz"].cpu(), opacities=op, scales=sc, scales_t=sct, rotations=rot, rotations_r=rot_r, ts=r["_t"].cpu(),
               shs=r["_features"].cpu(), prefilter_var=model.prefilter_var)
    return out


@functools.lru_cache(maxsize=None)
def case(P, rot_4d, pv, mod):
    """Scene, model, slice (with decomposition) and oracle of one geometry case, computed once for the tests that share it."""
    from fdgs.slice import time_slice
    dev = torch.device("cuda:0")
    scene = make_scene(P, rot_4d)
    model = make_model(scene, dev, pv)
    sl = time_slice(model, scene["timestamp"], mod, decompose=True)
    return {"scene": scene, "model": model, "slice": sl, "oracle": oracle_of(model, scene["timestamp"], mod), "dev": dev}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


GEOMETRY_CASES = [(P, r, pv, mod) for P in SIZES for r in (True, False) for pv, mod in (COMBOS_ALL if P == 257 else COMBOS)]


@pytest.mark.parametrize("P,rot_4d,pv,mod", GEOMETRY_CASES)
def test_slice_is_the_forwards_preprocess_bit_for_bit(gpu_device, P, rot_4d, pv, mod):
    """1: for every Gaussian the forward keeps (radii > 0), xyz / cov3D / opacity of the slice equal the forward's out_means3D / cov3D /
    conic_opacity[:, 3] bit for bit, and the forward's visible set is inside the live set.  Bar 0: the same operations by construction."""
    from fdgs.fused import raw_forward, raw_settings
    c = case(P, rot_4d, pv, mod)
    scene, model, sl = c["scene"], c["model"], c["slice"]
    rs, (xyz, feats, opacity, ts, scaling, scaling_t, rotation, rotation_r, pvar) = raw_settings(
        _Cam(scene, gpu_device), model, _Pipe(), scene["bg"].to(gpu_device), mod)
    assert pvar == (pv if pv > 0 else -1.0)
    with torch.no_grad():
        res = raw_forward(rs, xyz, feats, opacity, ts, scaling, scaling_t, rotation, rotation_r, pvar)
    hip = util.collect_forward(res, P, W, H)
    vis = np.nonzero(hip["radii"] > 0)[0]
    index = sl.index.cpu().numpy()
    assert index.dtype == np.int32 and sl.n == index.size
    assert np.isin(vis, index).all(), "a Gaussian the forward renders is not in the slice"
    if P >= 63:
        assert vis.size > 0 and index.size < P, "the case should have visible and culled Gaussians"
    row = np.searchsorted(index, vis)
    for got, want, what in ((sl.xyz, hip["out_means3D"], "xyz"), (sl.cov3D, hip["cov3D"], "cov3D"),
                            (sl.opacity, hip["conic_opacity"][:, 3], "opacity")):
        g, w = bits(got.cpu().numpy()[row]), bits(want[vis])
        assert np.array_equal(g, w), "%s differs from the forward's in %d of %d values" % (what, int((g != w).sum()), g.size)


@pytest.mark.parametrize("P,rot_4d,pv,mod", GEOMETRY_CASES)
def test_live_set_and_values_against_the_float64_statement(gpu_device, P, rot_4d, pv, mod):
    """2: the live set is the oracle's off the 0.05 cliff (float64 marginal within 1e-5 relative of it: at most 1 % of the Gaussians),
    ``index`` ascends strictly, and every row is the oracle's row to fp32 accuracy."""
    c = case(P, rot_4d, pv, mod)
    sl, o = c["slice"], c["oracle"]
    assert o["cliff"].sum() <= 0.01 * P, "pick another seed: %d Gaussians on the cull cliff" % int(o["cliff"].sum())
    index = sl.index.cpu().numpy().astype(np.int64)
    assert (np.diff(index) > 0).all() and (index.size == 0 or (index[0] >= 0 and index[-1] < P))
    got = np.zeros(P, bool)
    got[index] = True
    sure = ~o["cliff"]
    assert np.array_equal(got[sure], o["live"][sure])
    for t, want, tol in ((sl.xyz, o["xyz"], 1e-5), (sl.cov3D, o["cov6"], 1e-5), (sl.opacity, o["opacity"], 1e-5)):
        w = want[index]
        assert np.abs(t.cpu().numpy() - w).max(initial=0.0) <= tol * max(1.0, np.abs(w).max(initial=0.0))
    assert sl.P == P and sl.shs.shape == (sl.n, 16, 3) and sl.scales.shape == (sl.n, 3) and sl.rotations.shape == (sl.n, 4)


CHUNK_P = 1024 * 256 + 1   # the scan takes 1024 workgroup counts per chunk: one Gaussian past a scan chunk


def test_live_set_past_a_scan_chunk(gpu_device, rot_4d=True):
    """P = 262 145 at SH degree 0, about half of it live: 1025 workgroup counts, the last one behind the scan's first chunk.  n_live
    and ``index`` against the float64 statement off its cull cliff; the rows' own values at the bar of the smaller cases."""
    from fdgs.slice import time_slice
    scene = make_scene(CHUNK_P, rot_4d)
    model = make_model(scene, gpu_device)
    with torch.no_grad():
        model._t[-1] = scene["timestamp"]          # the one Gaussian of the last workgroup is live: its rank is the scan's carry
    sl = time_slice(model, scene["timestamp"])
    o = oracle_of(model, scene["timestamp"])
    assert o["cliff"].sum() <= 0.01 * CHUNK_P and o["live"][-1] and not o["cliff"][-1]
    index = sl.index.cpu().numpy().astype(np.int64)
    assert sl.n == index.size and 0.25 * CHUNK_P < sl.n < 0.75 * CHUNK_P
    assert (np.diff(index) > 0).all() and index[0] >= 0 and index[-1] < CHUNK_P
    got = np.zeros(CHUNK_P, bool)
    got[index] = True
    sure = ~o["cliff"]
    assert np.array_equal(got[sure], o["live"][sure])
    assert index[-1] == CHUNK_P - 1
    for t, want in ((sl.xyz, o["xyz"]), (sl.cov3D, o["cov6"]), (sl.opacity, o["opacity"])):
        w = want[index]
        assert np.abs(t.cpu().numpy() - w).max() <= 1e-5 * max(1.0, np.abs(w).max())


GUARD = 64
NAN_BITS = 0x7FC00000
SENTINEL = -7


class _Guarded:
    """Output buffers of ``cap`` rows with GUARD rows of NaN (index: a sentinel) on both sides."""

    def __init__(self, cap, dev):
        self.cap = cap
        shapes = {"index": (), "xyz": (3,), "cov3D": (6,), "opacity": (), "shs": (16, 3), "scales": (3,), "rotations": (4,)}
        self.full = {}
        for k, s in shapes.items():
            if k == "index":
                self.full[k] = torch.full((cap + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev)
            else:
                self.full[k] = torch.full((cap + 2 * GUARD,) + s, float("nan"), dtype=torch.float32, device=dev)
        self.n_live = torch.full((1,), SENTINEL, dtype=torch.int32, device=dev)

    def views(self):
        return tuple(self.full[k][GUARD:GUARD + self.cap] for k in ("index", "xyz", "cov3D", "opacity", "shs", "scales", "rotations"))

    def untouched(self, k, lo, hi):
        t = self.full[k][lo:hi]
        if k == "index":
            return bool((t == SENTINEL).all())
        return bool((t.reshape(-1).view(torch.int32) == NAN_BITS).all())

    def check(self, n_written, what):
        for k, t in self.full.items():
            rows = t[GUARD:GUARD + n_written]
            if k == "index":
                assert bool((rows != SENTINEL).all()), "%s: %s has unwritten rows below n" % (what, k)
            else:
                assert bool(torch.isfinite(rows).all()), "%s: %s has unwritten or non-finite rows below n" % (what, k)
            assert self.untouched(k, 0, GUARD), "%s: %s written in front of the buffer" % (what, k)
            assert self.untouched(k, GUARD + n_written, self.cap + 2 * GUARD), "%s: %s written at or beyond row %d" % (what, k, n_written)


def run_guarded(model, t, cap, mod=1.0):
    from fdgs.slice import _enqueue
    dev = model._xyz.device
    g = _Guarded(cap, dev)
    rot_r = model._rotation_r.detach() if model.rot_4d else None
    inputs = (model._xyz.detach(), model.get_features.detach(), model._opacity.detach(), model._t.detach(), model._scaling.detach(),
              model._scaling_t.detach(), model._rotation.detach(), rot_r)
    pv = model.prefilter_var if model.prefilter_var > 0 else -1.0
    _enqueue(inputs, (model.active_sh_degree, model.active_sh_degree_t, mod, pv, t, model.time_duration[1] - model.time_duration[0],
                      model.rot_4d, model.force_sh_3d), cap, g.views(), g.n_live)
    torch.cuda.synchronize()
    return g, int(g.n_live.item())


@pytest.mark.parametrize("rot_4d", (True, False))
@pytest.mark.parametrize("P", (257, 4099))
def test_crafted_patterns_write_exactly_the_live_rows(gpu_device, P, rot_4d):
    """2: none / all / alternating / only the last Gaussian live, into NaN-filled buffers with guards: exactly rows < n are written,
    in index order; with capacity < n_live nothing at or beyond capacity is written, n_live still is, and time_slice raises.
    The empty slice renders as the background."""
    from fdgs.slice import render_slice, time_slice
    scene = make_scene(P, rot_4d, D=1)
    model = make_model(scene, gpu_device)
    t = scene["timestamp"]
    far = t + 100.0
    ar = torch.arange(P, device=gpu_device)
    patterns = {"none": torch.zeros(P, dtype=torch.bool, device=gpu_device), "all": torch.ones(P, dtype=torch.bool, device=gpu_device),
                "alternating": ar % 2 == 1, "last": ar == P - 1}
    for name, live in patterns.items():
        with torch.no_grad():
            model._t.copy_(torch.where(live, torch.tensor(t, device=gpu_device), torch.tensor(far, device=gpu_device)).reshape(P, 1))
        want = torch.nonzero(live).flatten().to(torch.int32)
        g, n = run_guarded(model, t, P)
        assert n == want.numel(), (name, n)
        g.check(n, name)
        assert torch.equal(g.views()[0][:n], want), name
        if n:
            assert torch.equal(g.views()[1][:n], model._xyz.detach()[want.long()]), name   # (dt = 0: no mean shift either way)
        sl = time_slice(model, t, decompose=True)
        assert sl.n == n and torch.equal(sl.index, want)
        if n == 0:   # a sweep that leaves the model's support: the background, nothing visible
            pkg = render_slice(sl, _Cam(scene, gpu_device), scene["bg"].to(gpu_device))
            assert pkg["radii"].shape == (P,) and not bool(pkg["radii"].any()) and not bool(pkg["visibility_filter"].any())
            assert torch.equal(pkg["render"], scene["bg"].to(gpu_device).reshape(3, 1, 1).expand(3, H, W))
            assert not bool(pkg["alpha"].any())
        if n >= 2:
            cap = n // 2
            g2, n2 = run_guarded(model, t, cap)
            assert n2 == n, "n_live must be reported in full when the buffers are too small"
            g2.check(cap, name + " capacity %d" % cap)
            assert torch.equal(g2.views()[0], want[:cap])
            for a, b in zip(g2.views()[1:], g.views()[1:]):
                assert torch.equal(a, b[:cap]), "the first rows do not depend on the capacity"
            with pytest.raises(RuntimeError, match="capacity"):
                time_slice(model, t, capacity=cap)
            assert time_slice(model, t, capacity=n).n == n


SH_CASES = [(0, 0, False), (1, 0, False), (2, 0, False), (3, 0, False), (3, 1, False), (3, 2, False), (3, 2, True)]


@pytest.mark.parametrize("P", (64, 257))   # 64: rows of 16-byte aligned float4s; 257: the float path (the bucket's rows are not aligned)
@pytest.mark.parametrize("D,D_t,force", SH_CASES)
def test_folded_sh_rows(gpu_device, P, D, D_t, force):
    """3: every element of the folded rows within 8 * 2^-24 * (|c0| + |t1 c1| + |t2 c2|) of float64 (three roundings of the sum and
    the fp32 rounding of tk); inactive coefficients exactly 0, whatever the inactive input holds."""
    from fdgs.slice import time_slice
    scene = make_scene(P, True, D=D, D_t=D_t, alloc=(3, 2), force_sh_3d=force, seed=5)
    assert scene["M"] == (16 if force else 48)
    if force:   # the reference allocates 16 coefficients then; give the row its 48 so that blocks 1 and 2 exist and must be ignored
        g = torch.Generator().manual_seed(1)
        scene["shs"] = torch.cat([scene["shs"], torch.randn(P, 32, 3, generator=g)], dim=1).contiguous()
        scene["M"] = 48
    model = make_model(scene, gpu_device)
    vec = model.get_features.data_ptr() % 16 == 0
    assert vec == (P == 64)
    t = scene["timestamp"]
    sl = time_slice(model, t)
    o = oracle_of(model, t)
    index = sl.index.cpu().numpy().astype(np.int64)
    assert 0 < index.size < P
    shs = raw_numpy(model)["_features"].astype(np.float64)[index]
    n0 = (D + 1) ** 2
    nblocks = 1 + min(D_t, 2) if (D > 2 and not force) else 1
    t1, t2 = o["t1"][index, None, None], o["t2"][index, None, None]
    mag = np.zeros((index.size, 16, 3))
    mag[:, :n0] = np.abs(shs[:, :n0])
    if nblocks > 1:
        mag += np.abs(t1 * shs[:, 16:32])
    if nblocks > 2:
        mag += np.abs(t2 * shs[:, 32:48])
    got = sl.shs.cpu().numpy()
    err = np.abs(got.astype(np.float64) - o["shs"][index])
    bound = 8 * 2.0 ** -24 * mag
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print("folded SH D=%d D_t=%d force=%s P=%d: worst error / bound = %.3f" % (D, D_t, force, P, worst))
    assert (err <= bound).all(), "worst error / bound = %g" % worst
    assert not got[:, n0:].any(), "inactive coefficients must be exactly 0"
    # poison everything the active degrees do not read: the rows must not change by a bit
    with torch.no_grad():
        keep = model._features.detach().clone()
        model._features[:, n0:16] = float("nan")
        if nblocks < 2:
            model._features[:, 16:32] = float("nan")
        if nblocks < 3:
            model._features[:, 32:48] = float("inf")
        again = time_slice(model, t).shs.cpu().numpy()
        model._features.copy_(keep)
    assert np.array_equal(bits(again), bits(got))


def _pixels(pkg, ref, label):
    border = ref["border"].astype(bool)
    frac = float(border.mean())
    bound = max(1e-3, 3.0 / border.size)   # check_forward's
    assert frac < bound, "%s: too many cliff pixels %g (bound %g): pick another seed" % (label, frac, bound)
    ok = ~border
    got = {"colour": pkg["render"].cpu().numpy(), "depth": pkg["depth"].cpu().numpy()[0], "alpha": pkg["alpha"].cpu().numpy()[0]}
    want = {"colour": ref["out_color"], "depth": ref["out_depth"], "alpha": 1.0 - ref["out_T"]}
    for k in got:
        d = np.abs(got[k] - want[k])
        d = d[:, ok] if d.ndim == 3 else d[ok]
        print("%s %s: max abs err %.3g off %d cliff pixels" % (label, k, float(d.max()), int(border.sum())))
        assert d.max() <= util.PIX_TOL, "%s: %s max abs err %g" % (label, k, float(d.max()))


PIXEL_P = 4099


@pytest.mark.parametrize("name,rot_4d,D,D_t,seed", [("dim4 sh3 t2", False, 3, 2, 3), ("rot4d sh0", True, 0, 0, 3)])
def test_pixels_where_the_slice_is_the_4d_render(gpu_device, name, rot_4d, D, D_t, seed):
    """4: no rot_4d (no mean shift), or degree 0 (no view dependence): render_slice is the 4D kernel path's image.  Expected: the CPU
    oracle on the 4D scene; colour, depth and alpha off its cliff pixels at PIX_TOL."""
    from fdgs.slice import render_slice, time_slice
    scene = make_scene(PIXEL_P, rot_4d, D=D, D_t=D_t, seed=seed)
    model = make_model(scene, gpu_device)
    scene4 = activated_scene(scene, model)
    ref, _ = util.run_oracle(scene4)
    assert int(ref["border_g"].sum()) == 0, "pick another seed: Gaussians on the temporal-cull cliff"
    sl = time_slice(model, scene["timestamp"])
    assert 0 < sl.n < PIXEL_P
    pkg = render_slice(sl, _Cam(scene, gpu_device), scene["bg"].to(gpu_device))
    _pixels(pkg, ref, name)
    assert np.array_equal(pkg["radii"].cpu().numpy(), ref["radii"]), "radii scattered back to the model's P entries"


def test_pixels_of_a_rot4d_slice_with_view_dependent_colour(gpu_device):
    """5: rot_4d at SH 3 + time 2: expected is the CPU oracle on the 3D scene the float64 statement builds (precomputed covariances,
    folded rows; the view direction from the SHIFTED mean, as any 3D viewer takes it)."""
    from fdgs.slice import render_slice, time_slice
    scene = make_scene(PIXEL_P, True, D=3, D_t=2, seed=3)
    model = make_model(scene, gpu_device)
    o = oracle_of(model, scene["timestamp"])
    assert int(o["cliff"].sum()) == 0
    ref, _ = util.run_oracle(so.sliced_scene(scene, o))
    sl = time_slice(model, scene["timestamp"])
    assert np.array_equal(sl.index.cpu().numpy(), o["index"])
    pkg = render_slice(sl, _Cam(scene, gpu_device), scene["bg"].to(gpu_device))
    _pixels(pkg, ref, "rot4d sh3 t2")
    assert pkg["radii"].shape == (PIXEL_P,) and not pkg["radii"].cpu().numpy()[~o["live"]].any()


def test_decomposition_against_float32_eigh(gpu_device):
    """6: PER GAUSSIAN, e_g = max|R diag(s^2) R^T - cov3D| / trace(cov3D) (R = build_rotation(q) in float64 from the kernel's fp32
    output) is held to 4 x max(e'_g, 2^-23), where e'_g = max|V diag(w) V^T - cov3D| / trace is what numpy.linalg.eigh in float32
    reaches on the same matrix (float64 from its fp32 output).  The two places where the bar is not eigh's raw figure, and why:
    * the floor 2^-23: eigh finds diagonal matrices exactly (e'_g = 0), while scales and quaternion are fp32 numbers -- a scale
      carries 2^-24 relative, its square 2^-23 of an eigenvalue that is at most the trace; a quaternion component 2^-25 absolute;
    * matrices eigh itself finds INDEFINITE (some w <= 0): the cancellation in Sigma_xx - c12 c12^T / cov_t leaves the fp32
      conditional covariance of a needle or near-singular Gaussian with a smallest eigenvalue down to about -2e-6 of the trace.
      R diag(s^2) R^T is positive semi-definite -- the slice's scales are by definition floored square roots -- so no scales come
      closer to such a matrix than |w_min|, while eigh's raw w reproduces it.  For these matrices only, e'_g is taken with eigh's
      eigenvalues through the same map (clipped at 0).  Every positive definite matrix is held to eigh's raw figure.
    Isotropic, needle (1 : 1e3) and near-singular (1 : 1e-6 in scale) Gaussians are planted among random ones; the observed figures
    are printed, DESIGN.md section 4.8 records them."""
    from fdgs.slice import time_slice
    P = 257
    scene = make_scene(P, True, seed=9)
    scene["rotations"] = torch.nn.functional.normalize(torch.randn(P, 4, generator=torch.Generator().manual_seed(2)), dim=1)
    scene["rotations_r"] = torch.nn.functional.normalize(torch.randn(P, 4, generator=torch.Generator().manual_seed(4)), dim=1)
    kinds = np.arange(P) % 4   # 0 random, 1 isotropic, 2 needle, 3 near-singular
    k1, k2, k3 = (torch.from_numpy(kinds == k) for k in (1, 2, 3))
    s = scene["scales"].clone()
    s[k1] = s[k1][:, :1].expand(-1, 3)
    s[k2] = s[k2][:, :1] * torch.tensor([1.0, 1e-3, 1e-3])
    s[k3] = s[k3][:, :1] * torch.tensor([1.0, 0.7, 1e-6])
    scene["scales"] = s
    ident = torch.tensor([1.0, 0.0, 0.0, 0.0])
    scene["rotations"][k1] = ident      # isotropic in space, no space-time mixing: the conditional covariance is s^2 I
    scene["rotations_r"][k1] = ident
    model = make_model(scene, gpu_device)
    with torch.no_grad():
        model._t.fill_(scene["timestamp"])      # everything live
    sl = time_slice(model, scene["timestamp"], decompose=True)
    assert sl.n == P
    cov = so.full3(sl.cov3D.cpu().numpy())
    tr = np.trace(cov, axis1=1, axis2=2)
    q, sc = sl.rotations.cpu().numpy().astype(np.float64), sl.scales.cpu().numpy().astype(np.float64)
    assert np.isfinite(q).all() and np.isfinite(np.log(sc)).all() and (sc > 0).all()
    assert np.abs(np.sqrt((q * q).sum(1)) - 1.0).max() <= 1e-6
    R = so.rotation_matrix(q)
    assert (np.linalg.det(R) > 0).all()
    mine = np.abs((R * (sc ** 2)[:, None, :]) @ R.transpose(0, 2, 1) - cov).max(axis=(1, 2)) / tr
    w, V = np.linalg.eigh(cov.astype(np.float32))
    assert w.dtype == np.float32 and V.dtype == np.float32
    V, w = V.astype(np.float64), w.astype(np.float64)
    raw = np.abs((V * w[:, None, :]) @ V.transpose(0, 2, 1) - cov).max(axis=(1, 2)) / tr
    clipped = np.abs((V * np.maximum(w, 0.0)[:, None, :]) @ V.transpose(0, 2, 1) - cov).max(axis=(1, 2)) / tr
    pd = w.min(axis=1) > 0
    theirs = np.where(pd, raw, clipped)
    bar = 4.0 * np.maximum(theirs, 2.0 ** -23)
    ratio = mine / bar
    for k, name in enumerate(("random", "isotropic", "needle", "near-singular")):
        sel = kinds == k
        print("decomposition %-13s: kernel max %.3g  eigh(float32) max %.3g (raw w: %.3g), %d of %d positive definite, worst e_g / bar_g %.3f" % (
            name, mine[sel].max(), theirs[sel].max(), raw[sel].max(), int(pd[sel].sum()), int(sel.sum()), ratio[sel].max()))
    print("decomposition worst e_g / (4 max(e'_g, 2^-23)) = %.3f; worst e_g / e'_g where e'_g > 2^-23: %.3f" % (
        ratio.max(), (mine / np.maximum(theirs, 1e-300))[theirs > 2.0 ** -23].max(initial=0.0)))
    assert pd[kinds <= 1].all() and (~pd).any(), "random and isotropic matrices are positive definite; the planted kinds include indefinite ones"
    g = int(np.argmax(ratio))
    assert ratio[g] <= 1.0, "Gaussian %d (kind %d): e_g %.3g > 4 max(e'_g %.3g, 2^-23)" % (g, kinds[g], mine[g], theirs[g])
    iso = kinds == 1
    assert np.abs(sc[iso] / sc[iso][:, :1] - 1.0).max() <= 1e-6


def test_render_slice_bookkeeping(gpu_device):
    """7: the P-sized radii are zero off ``index`` and the compact radii on it; visibility_filter is radii > 0."""
    from fdgs.slice import _rasterize, render_slice
    c = case(4099, True, -1.0, 1.0)
    scene, sl = c["scene"], c["slice"]
    cam, bg = _Cam(scene, gpu_device), scene["bg"].to(gpu_device)
    pkg = render_slice(sl, cam, bg)
    assert set(pkg) == {"render", "viewspace_points", "visibility_filter", "radii", "depth", "alpha", "flow"}
    _image, radii, _depth, _alpha, _flow = _rasterize(sl, cam, bg)
    assert radii.shape == (sl.n,) and pkg["radii"].shape == (4099,) and pkg["radii"].dtype == radii.dtype
    idx = sl.index.long()
    assert torch.equal(pkg["radii"][idx], radii) and int((radii > 0).sum()) > 0
    off = torch.ones(4099, dtype=torch.bool, device=gpu_device)
    off[idx] = False
    assert int(off.sum()) > 0 and not bool(pkg["radii"][off].any())
    assert torch.equal(pkg["visibility_filter"], pkg["radii"] > 0)
    assert pkg["render"].shape == (3, H, W) and pkg["depth"].shape == (1, H, W) and pkg["alpha"].shape == (1, H, W)
