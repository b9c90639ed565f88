"""GPU: fdgs.edit.transform (csrc/model_transform.hip) -- the identity bit for bit, means / times / SH rows at per-element error bars
against float64 (tests/edit_oracle.py), covariances against the best an fp32 output can do, in place == out of place, the render
seen through the transformed camera against the CPU oracle's own figure, and the argument errors of the C entry."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import edit_cases as ec
import edit_oracle as eo

pytestmark = pytest.mark.gpu

EPS32 = eo.EPS32
GEOM = ("_xyz", "_t", "_scaling", "_scaling_t", "_rotation", "_rotation_r")
# (mode, transform): without rot_4d one general transform and the half turn; with it the closed form (s == a) and both (s, a) of the
# re-decomposition
CASES = [("3d", "fast"), ("3d", "pi"), ("4d", "fast"), ("4d", "eq"), ("rot4d", "eq"), ("rot4d", "pi"), ("rot4d", "scale_only"),
         ("rot4d", "half"), ("rot4d", "fast")]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def model_of(P, mode, D=3, D_t=2):
    dev = torch.device("cuda:0")
    scene = ec.make_scene(P, mode, D=D, D_t=D_t)
    model = ec.make_model(scene, dev)
    if P >= 63:   # blocks of zeros (a model whose time blocks were never trained), and a negative zero among the parameters
        with torch.no_grad():
            model._features[5:40:3, 16:] = 0.0
            model._features[7, :16] = 0.0
            model._xyz[3, 1] = -0.0
            model._rotation[4, 2] = -0.0
    return scene, model, ec.raw_numpy(model)


@functools.lru_cache(maxsize=None)
def case(P, mode, name):
    """Model, its raw parameters and the raw parameters of its transform: computed once for the tests that share it."""
    from fdgs.edit import transform
    scene, model, raw = model_of(P, mode)
    out = transform(model, ec.similarity(name))
    torch.cuda.synchronize()
    return {"model": model, "raw": raw, "out": out, "raw_out": ec.raw_numpy(out)}


@pytest.mark.parametrize("mode", tuple(ec.MODES))
@pytest.mark.parametrize("P", ec.SIZES)
def test_identity_returns_the_input_bit_for_bit(gpu_device, P, mode):
    """1: every segment, on the closed-form paths, -0 included; degrees, flags, duration and prefilter_var carried."""
    from fdgs.edit import Similarity, transform
    scene, model, raw = model_of(P, mode)
    out = transform(model, Similarity(np.eye(3)))
    assert out is not model and out.P == P and out.M == model.M
    for k in model.NAMES:
        assert np.array_equal(bits(raw[k]), bits(out.params[k].detach().cpu().numpy())), k
        assert out.params[k].data_ptr() != model.params[k].data_ptr()
    for attr in ("active_sh_degree", "active_sh_degree_t", "max_sh_degree", "max_sh_degree_t", "rot_4d", "gaussian_dim", "force_sh_3d",
                 "prefilter_var", "time_duration"):
        assert getattr(out, attr) == getattr(model, attr), attr


@pytest.mark.parametrize("mode,name", CASES)
@pytest.mark.parametrize("P", ec.SIZES)
def test_means_and_times_within_the_rounding_of_their_operations(gpu_device, P, mode, name):
    """2: |x' - float64| <= 4 eps32 (sum_j |s R_ij| |x_j| + |T_i|) per element, likewise t' = a t + b; opacity untouched."""
    c = case(P, mode, name)
    R, T, s, a, b = ec.TRANSFORMS[name]
    xyz, t, bx, bt = eo.transformed_means(c["raw"], R, T, s, a, b)
    ex = np.abs(c["raw_out"]["_xyz"].astype(np.float64) - xyz)
    print("xyz: worst error / bound %.3f" % float((ex / np.maximum(bx, 1e-300)).max()))
    assert (ex <= bx).all()
    if mode != "3d":
        et = np.abs(c["raw_out"]["_t"].astype(np.float64).reshape(-1) - t)
        print("t: worst error / bound %.3f" % float((et / np.maximum(bt, 1e-300)).max()))
        assert (et <= bt).all()
    else:
        assert np.array_equal(bits(c["raw_out"]["_t"]), bits(c["raw"]["_t"]))
        assert np.array_equal(bits(c["raw_out"]["_scaling_t"]), bits(c["raw"]["_scaling_t"]))
    assert np.array_equal(bits(c["raw_out"]["_opacity"]), bits(c["raw"]["_opacity"]))
    out, model = c["out"], c["model"]
    assert out.time_duration == [a * model.time_duration[0] + b, a * model.time_duration[1] + b]


@pytest.mark.parametrize("mode,name", CASES)
@pytest.mark.parametrize("P", ec.SIZES)
def test_covariances_against_the_best_fp32_can_do(gpu_device, P, mode, name):
    """3: the covariance the OUTPUT parameters stand for (re-activated in float64) against A Sigma A^T of the input's, relative in
    Frobenius norm per Gaussian: within 4 x the error of the oracle's own float64 decomposition rounded to fp32 storage on that
    Gaussian, plus 8 eps32.  Covariances, not quaternions or scales: the decomposition is not unique.  No Gaussian is exempt."""
    c = case(P, mode, name)
    R, T, s, a, b = ec.TRANSFORMS[name]
    if mode == "rot4d":
        want = eo.transformed_cov4(c["raw"], R, s, a)
        yard, _ = eo.yardstick4(want)
        err = eo.rel_fro(eo.rebuild4(c["raw_out"]), want)
        print("cov4: worst error %.3g (%.2f eps32), worst error / bar %.3f, yardstick median %.2f eps32"
              % (err.max(), err.max() / EPS32, (err / (4 * yard + 8 * EPS32)).max(), np.median(yard) / EPS32))
        assert (err <= 4 * yard + 8 * EPS32).all()
        q = np.concatenate([c["raw_out"]["_rotation"], c["raw_out"]["_rotation_r"]], 1)
        assert np.isfinite(q).all() and np.isfinite(c["raw_out"]["_scaling"]).all() and np.isfinite(c["raw_out"]["_scaling_t"]).all()
    else:
        raw_in = dict(c["raw"])
        raw_out = dict(c["raw_out"])
        if mode == "3d":
            raw_in["_scaling_t"] = raw_out["_scaling_t"] = None
        want, want_t = eo.transformed_cov3(raw_in, R, s, a)
        yard, yard_t, _ = eo.yardstick3(raw_in, R, s, a)
        got, got_t = eo.rebuild3(raw_out)
        err = eo.rel_fro(got, want)
        print("cov3: worst error %.3g (%.2f eps32), worst error / bar %.3f" % (err.max(), err.max() / EPS32, (err / (4 * yard + 8 * EPS32)).max()))
        assert (err <= 4 * yard + 8 * EPS32).all()
        if mode == "4d":
            err_t = np.abs(got_t - want_t) / want_t
            assert (err_t <= 4 * yard_t + 8 * EPS32).all()
        assert np.array_equal(bits(c["raw_out"]["_rotation_r"]), bits(c["raw"]["_rotation_r"])), "_rotation_r is a placeholder without rot_4d"


def _check_sh(rows_in, rows_out, R, M):
    """4: per element within 4 eps32 sum_j |D_ij| |c_j| + 2^-126 of float64 D c (D from the oracle's fit); DC bit for bit; zero blocks +0."""
    D = eo.sh_rotation_fit(R)
    P = rows_in.shape[0]
    nb, cb = max(M // 16, 1), min(M, 16)
    cin = rows_in.astype(np.float64).reshape(P, nb, cb, 3)
    cout = rows_out.reshape(P, nb, cb, 3)
    want = np.einsum("ij,pbjc->pbic", D[:cb, :cb], cin)
    bar = 4 * EPS32 * np.einsum("ij,pbjc->pbic", np.abs(D[:cb, :cb]), np.abs(cin)) + 2.0 ** -126
    err = np.abs(cout.astype(np.float64) - want)
    print("sh: worst error / bar %.3f" % float((err[:, :, 1:] / bar[:, :, 1:]).max(initial=0.0)))
    assert (err <= bar).all()
    assert np.array_equal(bits(cout[:, :, 0]), bits(rows_in.reshape(P, nb, cb, 3)[:, :, 0])), "DC must be copied bit for bit"
    zero = ~cin.reshape(P, nb, -1).any(axis=2)
    assert not bits(cout)[zero].any(), "a block of zeros must stay +0"
    return int(zero.sum())


@pytest.mark.parametrize("mode,name", [("3d", "fast"), ("rot4d", "eq"), ("rot4d", "half"), ("rot4d", "pi")])
@pytest.mark.parametrize("P", ec.SIZES)
def test_sh_rows_are_rotated_block_by_block(gpu_device, P, mode, name):
    """4: M = 16 (3D) and 48 (4D), the whole allocated row; both the 16-byte path (aligned rows) and the float path."""
    c = case(P, mode, name)
    M = c["model"].M
    assert M == (16 if mode == "3d" else 48)
    nzero = _check_sh(c["raw"]["_features"], c["raw_out"]["_features"], ec.TRANSFORMS[name][0], M)
    if P >= 63:   # (model_of: Gaussian 7's block 0 everywhere; with time blocks, those of twelve Gaussians too)
        assert nzero >= (1 if mode == "3d" else 20)


@pytest.mark.parametrize("mode,name,D,D_t", [("rot4d", "eq", 1, 0), ("rot4d", "eq", 3, 1), ("3d", "fast", 1, 0), ("3d", "fast", 2, 0)])
def test_sh_rotation_does_not_depend_on_the_active_degree(gpu_device, mode, name, D, D_t):
    """4: active degrees below the allocated ones, M = 48 and M = 16: the same rows come out as with every degree active."""
    from fdgs.edit import transform
    scene, model, raw = model_of(257, mode, D, D_t)
    M, max_t = (48, 2) if mode == "rot4d" else (16, 0)
    assert model.M == M and model.active_sh_degree == D and model.active_sh_degree_t == D_t and model.max_sh_degree == 3
    out = transform(model, ec.similarity(name))
    assert (out.active_sh_degree, out.active_sh_degree_t, out.max_sh_degree, out.max_sh_degree_t) == (D, D_t, 3, max_t)
    _check_sh(raw["_features"], out._features.detach().cpu().numpy(), ec.TRANSFORMS[name][0], M)
    full = case(257, mode, name)
    assert np.array_equal(full["raw"]["_features"], raw["_features"])   # (the same seed: the same rows)
    assert np.array_equal(bits(full["raw_out"]["_features"]), bits(out._features.detach().cpu().numpy()))


@pytest.mark.parametrize("P", (63, 64, 65, 257))   # (64: the rows start on 16 bytes)
@pytest.mark.parametrize("M", (1, 4, 9, 32))
def test_short_and_two_block_rows(gpu_device, P, M):
    """4: rows with M < 16 rotate the bands they hold; M = 32 is two blocks."""
    from fdgs.edit import transform
    from fdgs.train_host import GaussianParams
    g = torch.Generator().manual_seed(M)
    dim = 4 if M == 32 else 3
    t = {"_xyz": torch.randn(P, 3, generator=g), "_features": torch.randn(P, M, 3, generator=g), "_opacity": torch.randn(P, 1, generator=g),
         "_scaling": torch.randn(P, 3, generator=g) - 3, "_rotation": torch.randn(P, 4, generator=g), "_t": torch.rand(P, 1, generator=g),
         "_scaling_t": torch.randn(P, 1, generator=g) - 2}
    t["_features"][3] = 0.0
    model = GaussianParams.from_raw(t, gpu_device, max_sh_degree={1: 0, 4: 1, 9: 2, 32: 3}[M], max_sh_degree_t=1 if M == 32 else 0, gaussian_dim=dim)
    out = transform(model, ec.similarity("fast"))
    assert _check_sh(t["_features"].numpy(), out._features.detach().cpu().numpy(), ec.TRANSFORMS["fast"][0], M) >= 1


@pytest.mark.parametrize("mode", ("3d", "rot4d"))
@pytest.mark.parametrize("P", ec.SIZES)
def test_identity_rotation_with_a_scale_leaves_the_rows_alone(gpu_device, P, mode):
    """4: R = I, s != 1: the SH pass is skipped, the rows are copied bit for bit; the geometry still scales."""
    c = case(P, mode, "scale_only")
    assert np.array_equal(bits(c["raw_out"]["_features"]), bits(c["raw"]["_features"]))
    assert np.array_equal(bits(c["raw_out"]["_rotation"]), bits(c["raw"]["_rotation"]))
    assert not np.array_equal(c["raw_out"]["_scaling"], c["raw"]["_scaling"])


@pytest.mark.parametrize("mode,name", [("3d", "fast"), ("4d", "fast"), ("rot4d", "eq"), ("rot4d", "half"), ("rot4d", "scale_only")])
@pytest.mark.parametrize("P", ec.SIZES)
def test_in_place_gives_the_same_bits(gpu_device, P, mode, name):
    """5: inplace=True writes the model's own tensors (every output aliases its input) and returns the model.  P = 64 and 4099 % 4 != 0:
    the SH rows of a flat bucket start on 16 bytes only where P % 4 == 0, so both the 16-byte and the 4-byte path run with in == out."""
    from fdgs.edit import transform
    from fdgs.train_host import GaussianParams
    c = case(P, mode, name)
    scene, _, raw = model_of(P, mode)
    twin = GaussianParams.from_raw({k: v.detach() for k, v in c["model"].params.items()}, gpu_device, max_sh_degree=3,
                                   max_sh_degree_t=c["model"].max_sh_degree_t, time_duration=(0.0, 1.0), rot_4d=c["model"].rot_4d,
                                   gaussian_dim=c["model"].gaussian_dim)
    ptrs = {k: v.data_ptr() for k, v in twin.params.items()}
    assert (twin._features.data_ptr() % 16 == 0) == (P % 4 == 0)
    back = transform(twin, ec.similarity(name), inplace=True)
    assert back is twin and ptrs == {k: v.data_ptr() for k, v in twin.params.items()}
    for k in twin.NAMES:
        assert np.array_equal(bits(twin.params[k].detach().cpu().numpy()), bits(c["raw_out"][k])), k
    assert twin.time_duration == c["out"].time_duration


def test_prefilter_var_scales_with_the_time_axis_and_env_maps_are_refused(gpu_device):
    from fdgs.edit import transform
    scene, model, raw = model_of(64, "rot4d")
    model.prefilter_var = 0.02
    try:
        assert transform(model, ec.similarity("fast")).prefilter_var == pytest.approx(0.02 * 0.25)
    finally:
        model.prefilter_var = -1.0
    assert transform(model, ec.similarity("fast")).prefilter_var == -1.0
    model.env_map = torch.zeros(3, 8, 8, device=gpu_device)
    try:
        with pytest.raises(ValueError, match="environment map"):
            transform(model, ec.similarity("fast"))
    finally:
        model.env_map = None


class _Pipe:
    compute_cov3D_python = convert_SHs_python = debug = False
    env_map_res = 0


@pytest.mark.parametrize("name", ec.RENDER_CASES)
def test_render_is_invariant_under_the_transform(gpu_device, name):
    """6: PSNR of render(transform(model), transform_camera(cam)) against render(model, cam), 96x64, rot_4d, D = 3, D_t = 2, P = 4099:
    no more than 1 dB below the same figure of the CPU oracle (tests/golden/edit_render_psnr.json, made by
    tests/golden/make_golden_edit.py from float64-transformed parameters rounded to fp32); the dB covers alpha = 1/255 and radius
    cliffs that flip differently on the two sides.  Depth / s likewise."""
    from fdgs.edit import transform, transform_camera
    from fdgs.gaussian_renderer import render
    from fdgs.train_host import SyntheticCamera
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", ec.GOLDEN)) as f:
        ref = json.load(f)[name]
    scene = ec.render_scene()
    s = ec.TRANSFORMS[name][2]
    assert ec.near_band_is_empty(scene, s), "the z > 0.2 near cull is not scale-invariant: pick another pose"
    model = ec.make_model(scene, gpu_device)
    sim = ec.similarity(name)
    cam = SyntheticCamera(scene, gpu_device)
    bg = scene["bg"].to(gpu_device)
    with torch.no_grad():
        a = render(cam, model, _Pipe(), bg)
        b = render(transform_camera(cam, sim), transform(model, sim), _Pipe(), bg)
    img_a, img_b = a["render"].cpu().numpy(), b["render"].cpu().numpy()
    dep_a, dep_b = a["depth"].cpu().numpy(), b["depth"].cpu().numpy() / s
    assert int((a["radii"] > 0).sum()) > 500
    p_img, p_dep = ec.psnr(img_a, img_b, 1.0), ec.psnr(dep_a, dep_b, float(ref["depth_peak"]))
    print("%s: image PSNR %.2f dB (oracle %.2f), depth PSNR %.2f dB (oracle %.2f)" % (name, p_img, ref["psnr_image"], p_dep, ref["psnr_depth"]))
    assert p_img >= ref["psnr_image"] - 1.0
    assert p_dep >= ref["psnr_depth"] - 1.0


def test_abi_rejections(gpu_device):
    """7: every argument error returns FDGS_ERR_INVALID_ARG and sets fdgs_last_error, also in a process that has the GPU open."""
    torch.zeros(1, device=gpu_device)
    ec.check_abi_rejections()
