"""GPU: csrc/seed.hip (fdgs.seed) against the numpy restatements of tests/seed_oracle.py.

Thinning: keys, counts, first members, order and the count_only total exact; the means bit-equal to the restatement's sequential
float32 sums and within the sequential-sum bound (n - 1) 2^-24 sum|x_i| / n of the float64 mean (derived, not measured); two runs
bit-identical.  Random clouds: Philox words and uniforms bit-equal.  Initial model: every segment bit-equal to the float32 restatement
except ``_scaling`` (a logarithm), which is held to 4 x the error of the reference's own float32 expression evaluated by torch on the
CPU, floor one float32 ulp (the margin of tests/test_gpu_loss_edges.py).  End to end: the example's tiny dataset trains."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import seed_cases
import seed_oracle as so

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = seed_cases.cases()


def _cloud(dev, xyz, rgb, t):
    from fdgs import seed
    return seed.PointCloud(torch.from_numpy(xyz).to(dev), torch.from_numpy(rgb).to(dev), None if t is None else torch.from_numpy(t).to(dev))


def _np(x):
    return None if x is None else x.detach().cpu().numpy()


@pytest.mark.parametrize("timed", [True, False], ids=["t", "no_t"])
@pytest.mark.parametrize("name", list(CASES))
def test_thin_against_the_restatement(gpu_device, name, timed):
    from fdgs import seed
    xyz, rgb, t, cell, cell_t = CASES[name]
    t = t if timed else None
    want = so.thin(xyz, rgb, t, *so.grid_of(xyz, t, cell, cell_t))
    cloud = _cloud(gpu_device, xyz, rgb, t)
    got = seed.thin(cloud, cell, cell_t)
    again = seed.thin(cloud, cell, cell_t)
    M = len(want["key"])
    print(name, "N", len(xyz), "cells", M, "largest", int(want["count"].max()) if M else 0)
    assert len(got.cloud) == M and seed.count_cells(cloud, cell, cell_t) == M
    assert np.array_equal(_np(got.key).view(np.uint64), want["key"])
    assert np.array_equal(_np(got.count), want["count"]) and np.array_equal(_np(got.first), want["first"])
    if name == "big_cells":
        assert (want["count"] >= 300).sum() == 2 and want["count"].max() >= 1100
    if name == "own_cell":
        assert M == len(xyz)
    if name == "one_cell":
        assert M == 1
    cols = [("xyz", got.cloud.xyz, xyz), ("rgb", got.cloud.rgb, rgb)] + ([("t", got.cloud.t, t[:, None])] if timed else [])
    assert (got.cloud.t is None) == (not timed)
    worst = 0.0
    for nm, g, src in cols:
        g = _np(g)
        assert np.array_equal(g.view(np.uint32), want[nm].view(np.uint32)), nm            # bit-equal to the float32 restatement
        for k, idx in enumerate(want["members"]):
            mean, bound = so.mean_bound(src, idx)
            err = np.abs(np.atleast_1d(g[k]).astype(np.float64) - mean)
            assert (err <= bound).all(), (nm, k, len(idx), err, bound)
            if len(idx) > 1:
                worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    print("worst error / bound %.3f" % worst)
    for a, b in zip((got.key, got.count, got.first, got.cloud.xyz, got.cloud.rgb, got.cloud.t),
                    (again.key, again.count, again.first, again.cloud.xyz, again.cloud.rgb, again.cloud.t)):
        assert (a is None and b is None) or torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                        b.view(torch.int32) if b.dtype == torch.float32 else b)


@pytest.mark.parametrize("timed", [True, False], ids=["t", "no_t"])
def test_thin_to_finds_the_finest_rung(gpu_device, timed):
    from fdgs import seed
    xyz, rgb, t, _, _ = CASES["n5000"]
    cloud = _cloud(gpu_device, xyz, rgb, t if timed else None)
    num_pts = 700
    got = seed.thin_to(cloud, num_pts)
    k = seed.ladder_rung(cloud, got.cell)
    assert seed.ladder_cell(cloud, k) == (got.cell, got.cell_t) and 1 < k <= seed.LADDER
    finer = seed.count_cells(cloud, *seed.ladder_cell(cloud, k - 1))
    print("rung", k, "cell", got.cell, got.cell_t, "points", len(got.cloud), "one rung finer", finer)
    assert 1 <= len(got.cloud) <= num_pts < finer
    assert int(got.count.sum()) == len(xyz)
    same = seed.thin_to(cloud, len(xyz))                     # nothing to thin: the cloud itself
    assert same.cloud is cloud and same.key is None


@pytest.mark.parametrize("seed_value", [0, 0x9E3779B97F4A7C15], ids=["seed0", "seed64"])
@pytest.mark.parametrize("N", [1, 64, 65, 1000])
def test_random_words_and_uniforms(gpu_device, N, seed_value):
    from fdgs import seed
    for shape in ("box", "sphere"):
        sid = 0 if shape == "box" else 3
        w, u = so.draws(N, seed_value, sid)
        if shape == "box":
            out, words, uni = seed.random_box(N, seed_value, (-1.3, 0.25, 7.0), (2.6, 0.5, 1e-3), gpu_device, stream_id=sid, debug=True)
            want = u[:, :3] * np.array([2.6, 0.5, 1e-3], np.float32) + np.array([-1.3, 0.25, 7.0], np.float32)
            assert np.array_equal(_np(out).view(np.uint32), want.view(np.uint32))
        else:
            r = 60.0
            out, words, uni = seed.random_sphere(N, seed_value, r, gpu_device, stream_id=sid, debug=True)
            radius = np.sqrt((_np(out).astype(np.float64) ** 2).sum(1))
            # r s cos, r s sin, r c with s = sqrt(1 - c c): a handful of float32 roundings, each a relative 2^-24, on top of
            # sin^2 + cos^2 = 1 to the same order: 16 roundings' worth is generous and still 1e-6 relative
            print("radius error / r: %.3g" % float(np.abs(radius / r - 1.0).max()))
            assert np.abs(radius / r - 1.0).max() <= 16 * 2.0 ** -24
            c = _np(out)[:, 2].astype(np.float64) / r
            assert np.abs(c - (2.0 * u[:, 1].astype(np.float64) - 1.0)).max() <= 4 * 2.0 ** -24
        assert np.array_equal(_np(words).view(np.uint32), w)
        assert np.array_equal(_np(uni).view(np.uint32), u.view(np.uint32))
        assert float(uni.min()) >= 0.0 and float(uni.max()) < 1.0
    cloud = seed.random_cloud(N, seed_value, device=gpu_device)
    assert np.array_equal(_np(cloud.xyz).view(np.uint32), so.box(so.draws(N, seed_value, 0)[1], -1.3, 2.6).view(np.uint32))
    assert np.array_equal(_np(seed.random_times(N, seed_value, (0.5, 10.0), gpu_device)).view(np.uint32),
                          so.times(so.draws(N, seed_value, 2)[1], 0.5, 10.0).view(np.uint32))


CONFIGS = {"dim3": (3, False), "dim4": (4, False), "rot4d": (4, True)}
_ratios = {}


@pytest.mark.parametrize("P", [1, 65, 1000])
@pytest.mark.parametrize("M", [1, 16, 48])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_init_against_the_restatement(gpu_device, config, M, P):
    from fdgs import layout, seed
    from fdgs.train_host import GaussianParams
    dim, rot = CONFIGS[config]
    rng = np.random.default_rng(1000 * P + M)
    xyz = rng.normal(0, 2, (P, 3)).astype(np.float32)
    rgb = rng.uniform(0, 1, (P, 3)).astype(np.float32)
    t = rng.uniform(-1, 11, P).astype(np.float32)
    d2 = np.exp(rng.uniform(np.log(1e-8), np.log(1e4), P)).astype(np.float32)
    d2[::7] = 0.0
    d2[1::7] = 1e-9                                              # below the clamp
    d2[2::7] = 1e6
    td = (0.5, 10.0)
    dev = gpu_device
    cloud = _cloud(dev, xyz, rgb, t)
    kw = dict(sh_degree=3, sh_degree_t=2, gaussian_dim=dim, rot_4d=rot, force_sh_3d=False, time_duration=td, seed=0, M=M)
    model = seed.create_from_pcd(cloud, dist2=torch.from_numpy(d2).to(dev), **kw)
    assert model.P == P and model.M == M and (model.active_sh_degree, model.active_sh_degree_t) == (0, 0)
    assert (model.max_sh_degree, model.max_sh_degree_t, model.gaussian_dim, model.rot_4d) == (3, 2, dim, rot)
    want = so.init_f32(xyz, rgb, t, d2, M, dim, td)
    for name in model.NAMES:
        got = _np(model.params[name])
        assert got.shape == want[name].shape, name
        if name != "_scaling":
            assert np.array_equal(got.view(np.uint32), want[name].view(np.uint32)), name
    # the segments a mode does not read hold layout.placeholder_'s values
    for name in set(model.NAMES) - set(layout.used(dim, rot)):
        ph = torch.empty_like(model.params[name].detach())
        layout.placeholder_(ph, name)
        assert torch.equal(model.params[name].detach(), ph), name
    # _scaling: float64 restatement; bar = 4 x the error of the reference's float32 expression by torch on the CPU, floor one ulp
    exact = so.scaling_f64(d2)
    ref = torch.log(torch.sqrt(torch.clamp_min(torch.from_numpy(d2), 0.0000001))).numpy().astype(np.float64)
    ulp = np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
    bar = np.maximum(4.0 * np.abs(ref - exact), ulp)
    got = _np(model.params["_scaling"]).astype(np.float64)
    assert (got[:, 0] == got[:, 1]).all() and (got[:, 0] == got[:, 2]).all()
    ratio = float((np.abs(got[:, 0] - exact) / bar).max())
    _ratios[(config, M, P)] = ratio
    print("_scaling worst error / bar %.3f" % ratio)
    assert ratio <= 1.0
    # the same model from PyTorch tensors through from_raw
    with torch.no_grad():
        d = torch.from_numpy(d2).to(dev)
        raw = {"_xyz": cloud.xyz, "_opacity": torch.full((P, 1), float(so.init_constants(td)[0]), device=dev),
               "_scaling": torch.log(torch.sqrt(torch.clamp_min(d, 0.0000001)))[..., None].repeat(1, 3),
               "_rotation": torch.tensor([1.0, 0, 0, 0], device=dev).repeat(P, 1),
               "_features": torch.zeros((P, M, 3), device=dev)}
        raw["_features"][:, 0, :] = (cloud.rgb - 0.5) / torch.tensor(so.C0, device=dev)   # a true division: by a Python number it is a product
        if dim == 4:
            raw["_t"] = cloud.t[:, None]
            raw["_scaling_t"] = torch.full((P, 1), float(so.init_constants(td)[1]), device=dev)
        if rot:
            raw[layout.SEGMENTS[6].name] = raw["_rotation"].clone()
    other = GaussianParams.from_raw(raw, dev, **{**model.settings()})
    assert other.settings() == model.settings()
    for name in model.NAMES:
        a, b = model.params[name].detach(), other.params[name].detach()
        if name == "_scaling":
            # the kernel rounds the float64 value once (half an ulp); torch's float32 chain on the device carries the square root's
            # rounding -- a relative 2^-24, the same absolute shift of the logarithm -- and its logarithm's own 1 ulp
            diff = np.abs(_np(a).astype(np.float64) - _np(b).astype(np.float64))[:, 0]
            assert (diff <= 2.0 ** -24 + 2.0 * ulp).all(), float((diff / (2.0 ** -24 + 2.0 * ulp)).max())
        else:
            assert torch.equal(a, b), name


def test_init_draws_times_for_a_cloud_without_them(gpu_device):
    from fdgs import seed
    xyz, rgb, _, _, _ = CASES["n257"]
    cloud = _cloud(gpu_device, xyz, rgb, None)
    model = seed.create_from_pcd(cloud, sh_degree=1, gaussian_dim=4, rot_4d=True, time_duration=(0.0, 2.0), seed=5)
    want = so.times(so.draws(len(xyz), 5, 2)[1], 0.0, 2.0)
    assert np.array_equal(_np(model._t)[:, 0].view(np.uint32), want.view(np.uint32))
    assert float(model._t.detach().min()) >= -0.2 and float(model._t.detach().max()) <= 2.2 and model.M == 6
    assert torch.isfinite(model.flat).all()


def test_worst_scaling_ratio_summary():
    """Not a check of its own: prints the worst ``_scaling`` error / bar the cases above observed (DESIGN.md section 4.7 records it)."""
    if _ratios:
        print("worst _scaling error / bar over %d cases: %.3f" % (len(_ratios), max(_ratios.values())))


def _example():
    spec = importlib.util.spec_from_file_location("train_from_data", os.path.join(ROOT, "examples", "train_from_data.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_end_to_end_on_the_examples_tiny_dataset(gpu_device, tmp_path):
    """examples/train_from_data.py at tiny size, in this process: 8 train views at 64x48, about 600 cloud points with times thinned to at
    most 400, 60 StepPipeline steps."""
    ex = _example()
    out = ex.run(str(tmp_path / "tiny"), gpu_device, views=8, test_views=2, width=64, height=48, cloud_points=600, num_pts=400, steps=60,
                 batch_size=8, log=lambda s: None)   # every step sees all eight views: the first and the last loss are the same sum
    print(out)
    assert out["train_views"] == 8 and out["image_size"] == (64, 48) and 550 <= out["cloud_points"] <= 650
    assert out["model_rows"] == out["thinned_points"] <= 400
    assert out["last_loss"] < out["first_loss"]
    assert out["psnr_trained"] > out["psnr_untrained"]
