"""CPU: the host side of fdgs.edit -- SH rotation matrices, the isoclinic pair, Similarity, merge / extract, the ABI structs and the
argument checks of fdgs_model_transform (nothing is launched here)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import edit_cases as ec
import edit_oracle as eo
from fdgs import synth

ROTATIONS = [("random0", eo.random_rotation(0)), ("random1", eo.random_rotation(1)), ("pi_x", eo.axis_angle((1, 0, 0), math.pi)),
             ("pi_diag", eo.axis_angle((1, 1, 0), math.pi)), ("pi_gen", eo.axis_angle((0.3, -0.5, 0.8), math.pi)),
             ("z90", eo.axis_angle((0, 0, 1), 0.5 * math.pi)), ("identity", np.eye(3)), ("tiny", eo.axis_angle((0.2, 0.9, -0.4), 1e-9))]
BANDS = ((0, 1), (1, 4), (4, 9), (9, 16))


@pytest.mark.parametrize("name,R", ROTATIONS)
def test_sh_rotation_is_block_orthogonal_and_agrees_with_the_fit(name, R):
    from fdgs.edit import sh_rotation
    D = sh_rotation(R)
    assert D.shape == (16, 16) and D.dtype == np.float64 and D[0, 0] == 1.0
    mask = np.zeros((16, 16), bool)
    for lo, hi in BANDS:
        mask[lo:hi, lo:hi] = True
        B = D[lo:hi, lo:hi]
        assert np.abs(B @ B.T - np.eye(hi - lo)).max() <= 1e-12, name
    assert not D[~mask].any(), "entries outside the band blocks"
    assert np.abs(D - eo.sh_rotation_fit(R)).max() <= 1e-12, name
    if name == "identity":
        assert np.abs(D - np.eye(16)).max() <= 1e-14


def test_sh_rotation_is_a_homomorphism():
    from fdgs.edit import sh_rotation
    R1, R2 = eo.random_rotation(5), eo.random_rotation(6)
    assert np.abs(sh_rotation(R1 @ R2) - sh_rotation(R1) @ sh_rotation(R2)).max() <= 1e-12


@pytest.mark.parametrize("deg", (1, 2, 3))
def test_rotated_coefficients_reproduce_the_colour_through_sh_utils(deg):
    """eval_sh (the package's own torch evaluation) of D c at R d is eval_sh of c at d."""
    from fdgs.edit import sh_rotation
    from fdgs.sh_utils import eval_sh
    R = eo.random_rotation(9)
    g = np.random.default_rng(3)
    n, nc = 50, (deg + 1) ** 2
    c = g.standard_normal((n, 16, 3))
    d = eo.random_directions(n, 4)
    cr = np.einsum("ij,njc->nic", sh_rotation(R), c)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    want = eval_sh(deg, t(c[:, :nc]).permute(0, 2, 1), t(d))
    got = eval_sh(deg, t(cr[:, :nc]).permute(0, 2, 1), t(d @ R.T))
    assert float((got - want).abs().max()) <= 1e-12


@pytest.mark.parametrize("name,R", ROTATIONS)
def test_isoclinic_pair_reproduces_the_embedded_rotation(name, R):
    from fdgs.edit import isoclinic_pair
    u, v = isoclinic_pair(R)
    assert u.dtype == np.float64 and abs(u @ u - 1) <= 1e-14 and abs(v @ v - 1) <= 1e-14
    G = np.eye(4)
    G[:3, :3] = R.T
    assert np.abs(eo.Mr(u) @ eo.Ml(v) - G).max() <= 1e-12, name


def test_isoclinic_families_commute_and_close():
    """What the closed-form rot_4d path rests on: M_r(x) M_l(y) = M_l(y) M_r(x), and each family is closed under the matrix product."""
    g = np.random.default_rng(0)
    x, y = g.standard_normal(4), g.standard_normal(4)
    assert np.abs(eo.Mr(x) @ eo.Ml(y) - eo.Ml(y) @ eo.Mr(x)).max() <= 1e-14
    for M in (eo.Ml, eo.Mr):
        P = M(x) @ M(y)
        e = np.eye(4)
        coef = np.array([(M(e[k]) * P).sum() / 4.0 for k in range(4)])
        assert np.abs(M(coef) - P).max() <= 1e-13


def test_similarity_inverse_compose_and_matrix():
    from fdgs.edit import Similarity
    a = Similarity(eo.random_rotation(1), (0.3, -1.0, 2.0), 0.5, 2.0, 0.25)
    b = Similarity(eo.quat_of(eo.random_rotation(2)), (1.0, 0.5, -0.5), 3.0, 0.5, -1.0)
    x = np.random.default_rng(1).standard_normal((7, 3))
    t = np.random.default_rng(2).standard_normal(7)
    xa, ta = a.apply(x, t)
    assert np.allclose(xa, x @ (0.5 * a.R).T + a.T) and np.allclose(ta, 2.0 * t + 0.25)
    xi, ti = a.inverse().apply(xa, ta)
    assert np.abs(xi - x).max() <= 1e-13 and np.abs(ti - t).max() <= 1e-13
    xc, tc = a.compose(b).apply(x, t)
    xb, tb = b.apply(x, t)
    xab, tab = a.apply(xb, tb)
    assert np.abs(xc - xab).max() <= 1e-12 and np.abs(tc - tab).max() <= 1e-13
    m = a.matrix()
    assert m.shape == (4, 4) and np.allclose(m[:3, :3], 0.5 * a.R) and np.allclose(m[:3, 3], a.T) and np.allclose(m[3], [0, 0, 0, 1])
    ident = a.compose(a.inverse())
    assert np.abs(ident.R - np.eye(3)).max() <= 1e-14 and np.abs(ident.T).max() <= 1e-14 and abs(ident.s - 1) <= 1e-15


def test_similarity_rejects_what_is_not_a_similarity():
    from fdgs.edit import Similarity
    R = eo.random_rotation(3)
    skew = R.copy()
    skew[0, 1] += 1e-4
    bad = [dict(rotation=skew), dict(rotation=np.diag([1.0, 1.0, -1.0])), dict(rotation=R * 1.001), dict(rotation=np.ones((2, 2))),
           dict(rotation=(1.0, 0.1, 0.0, 0.0)), dict(rotation=R, scale=0.0), dict(rotation=R, scale=-1.0), dict(rotation=R, time_scale=0.0),
           dict(rotation=R, time_scale=-2.0), dict(rotation=R, scale=float("nan")), dict(rotation=R, scale=float("inf")),
           dict(rotation=R, time_scale=float("inf")), dict(rotation=R, time_shift=float("nan")),
           dict(rotation=R, translation=(0.0, float("inf"), 0.0)), dict(rotation=np.full((3, 3), np.nan))]
    for kw in bad:
        with pytest.raises(ValueError):
            Similarity(**kw)
    Similarity(R)
    Similarity((1.0, 0.0, 0.0, 0.0))


# ---- merge / extract ----
def _model(P=40, D=3, D_t=0, alloc=(3, 2), rot_4d=True, dim=4, force=False, seed=0, duration=1.0):
    from fdgs.train_host import GaussianParams
    cfg = synth.SceneConfig("edit", P, 32, 32, D, D_t, 0.03, duration, rot_4d, dim, force)
    return GaussianParams(synth.make_scene(cfg, seed=seed, alloc=alloc), "cpu")


def test_extract_and_merge_bookkeeping():
    from fdgs.edit import extract, merge
    a, b = _model(40, D=2, seed=1), _model(25, D=3, D_t=0, seed=2)
    mask = torch.arange(40) % 3 == 0
    sub = extract(a, mask)
    assert sub.P == int(mask.sum()) and sub.M == a.M and sub.active_sh_degree == 2 and sub.max_sh_degree == 3 and sub.max_sh_degree_t == 2
    for n in a.NAMES:
        assert torch.equal(getattr(sub, n).detach(), getattr(a, n).detach()[mask]), n
    idx = torch.tensor([5, 1, 1])
    assert torch.equal(extract(a, idx)._xyz.detach(), a._xyz.detach()[idx])
    m = merge([a, b, sub])
    assert m.P == 40 + 25 + sub.P and m.active_sh_degree == 3 and m.active_sh_degree_t == 0 and m.rot_4d and m.gaussian_dim == 4
    for n in a.NAMES:
        assert torch.equal(getattr(m, n).detach(), torch.cat([getattr(x, n).detach() for x in (a, b, sub)])), n
    assert m.time_duration == [0.0, 1.0] and m.prefilter_var == a.prefilter_var
    # durations may differ as long as no time degree is active: the union of the intervals
    c = _model(10, D=3, seed=3, duration=2.0)
    c.time_duration = [0.5, 2.5]
    assert merge([a, c]).time_duration == [0.0, 2.5]
    # with a time degree the common duration is kept: it is all the renderer reads
    d1, d2 = _model(10, D=3, D_t=1, seed=4), _model(10, D=3, D_t=2, seed=5)
    d2.time_duration = [0.5, 1.5]
    md = merge([d1, d2])
    assert md.active_sh_degree_t == 2 and md.time_duration == [0.0, 1.0]


def test_merge_raises_on_every_mismatch():
    from fdgs.edit import extract, merge
    a = _model(10)
    with pytest.raises(ValueError, match="no models"):
        merge([])
    cases = {"gaussian_dim": _model(10, rot_4d=False, dim=3, alloc=(3, 0)), "rot_4d": _model(10, rot_4d=False),
             "force_sh_3d": _model(10, force=True), "M": _model(10, alloc=(3, 1))}
    cases["M"].max_sh_degree_t = 2   # (a row of 32 coefficients that claims the same maximum degrees)
    for what, other in cases.items():
        with pytest.raises(ValueError, match=what):
            merge([a, other])
    b = _model(10)
    b.max_sh_degree = 2
    with pytest.raises(ValueError, match="max_sh_degree"):
        merge([a, b])
    b = _model(10, alloc=(3, 1))
    with pytest.raises(ValueError, match="max_sh_degree_t"):
        merge([a, b])
    b = _model(10)
    b.prefilter_var = 0.01
    with pytest.raises(ValueError, match="prefilter_var"):
        merge([a, b])
    t1, t2 = _model(10, D=3, D_t=1), _model(10, D=3, D_t=0, duration=2.0)
    with pytest.raises(ValueError, match="time_scale = T_a / T_b = 0.5"):
        merge([t1, t2])
    b = _model(10)
    b.env_map = torch.zeros(3, 4, 4)
    with pytest.raises(ValueError, match="environment map"):
        merge([a, b])
    with pytest.raises(ValueError, match="environment map"):
        extract(b, torch.ones(10, dtype=torch.bool))
    with pytest.raises(ValueError, match="one entry per Gaussian"):
        extract(a, torch.ones(9, dtype=torch.bool))


def test_transform_rejects_on_the_host():
    from fdgs.edit import Similarity, transform
    a = _model(10)
    with pytest.raises(RuntimeError, match="no CPU path"):
        transform(a, Similarity(None))
    a.env_map = torch.zeros(3, 4, 4)
    with pytest.raises(ValueError, match="environment map"):
        transform(a, Similarity(None))


def test_transform_camera_on_the_host():
    """View rotation R_view R^T, centre s R c + T, timestamp a t + b; a point and its image see each other as before, s times as far."""
    from fdgs.edit import Similarity, transform_camera
    from fdgs.train_host import SyntheticCamera
    cfg = synth.SceneConfig("edit", 4, 96, 64, 0, 0, 0.03, 1.0, True, 4, False)
    scene = synth.make_scene(cfg, pose="rig2")
    cam = SyntheticCamera(scene, "cpu")
    sim = Similarity(eo.random_rotation(4), (0.4, -0.2, 1.0), 0.5, 2.0, 0.3)
    cam2 = transform_camera(cam, sim)
    assert type(cam2) is type(cam) and cam2.FoVx == cam.FoVx and cam2.image_width == 96 and cam2.image_height == 64
    assert cam2.timestamp == pytest.approx(2.0 * cam.timestamp + 0.3)
    c = cam.camera_center.numpy().astype(np.float64)
    assert np.abs(cam2.camera_center.numpy() - (0.5 * sim.R @ c + sim.T)).max() <= 1e-6
    assert np.abs(cam2.world_view_transform.numpy()[:3, :3].T - cam.world_view_transform.numpy()[:3, :3].T.astype(np.float64) @ sim.R.T).max() <= 1e-6
    x = np.random.default_rng(0).standard_normal((9, 3))
    h = lambda p: np.concatenate([p, np.ones((p.shape[0], 1))], 1)  # noqa: E731
    v1 = h(x) @ cam.world_view_transform.numpy().astype(np.float64)
    v2 = h(sim.apply(x)) @ cam2.world_view_transform.numpy().astype(np.float64)
    assert np.abs(v2[:, :3] - 0.5 * v1[:, :3]).max() <= 1e-5
    p1 = h(x) @ cam.full_proj_transform.numpy().astype(np.float64)
    p2 = h(sim.apply(x)) @ cam2.full_proj_transform.numpy().astype(np.float64)
    assert np.abs(p1[:, :2] / p1[:, 3:] - p2[:, :2] / p2[:, 3:]).max() <= 1e-5
    assert cam.world_view_transform is not cam2.world_view_transform and cam.timestamp == scene["timestamp"]


# ---- the oracle's own pieces ----
def test_oracle_decomposition_round_trips():
    g = np.random.default_rng(7)
    P = 20
    raw = {"_scaling": g.normal(-3, 0.5, (P, 3)), "_scaling_t": g.normal(-2, 0.5, (P, 1)), "_rotation": g.standard_normal((P, 4)),
           "_rotation_r": g.standard_normal((P, 4))}
    S = eo.transformed_cov4(raw, eo.random_rotation(8), 0.5, 2.0)
    back = eo.rebuild4(eo.decompose4(S))
    assert eo.rel_fro(back, S).max() <= 1e-13
    err, _ = eo.yardstick4(S)
    assert err.max() <= 16 * eo.EPS32 and err.min() > 0


# ---- ABI ----
def test_transform_struct_sizes_are_the_headers():
    """The library compares struct_size with sizeof() of its own header: a call with P = 0 that passes has matching layouts."""
    from fdgs import _capi
    a_in, a_out = ec.args()
    assert a_in.struct_size == C.sizeof(_capi.FdgsTransformIn) and a_out.struct_size == C.sizeof(_capi.FdgsTransformOut)
    assert _capi.FdgsTransformIn._fields_[0][0] == _capi.FdgsTransformOut._fields_[0][0] == "struct_size"
    assert _capi.lib.fdgs_model_transform(C.byref(a_in), C.byref(a_out), None) == 0, _capi.last_error()
    assert "fdgs_model_transform" in _capi.EXPORTED
    for which, name in ((a_in, "fdgs_transform_in"), (a_out, "fdgs_transform_out")):
        which.struct_size -= 4
        assert _capi.lib.fdgs_model_transform(C.byref(a_in), C.byref(a_out), None) == 1
        assert "struct_size" in _capi.last_error() and name in _capi.last_error()
        which.struct_size += 4


def test_c_entry_checks_its_arguments_without_touching_the_gpu():
    ec.check_abi_rejections()


def test_in_place_needs_the_models_own_feature_tensor():
    """A model whose get_features builds the rows on the fly (the reference's _features_dc / _features_rest) cannot be edited in place:
    the rotated rows would be a temporary.  The check comes before anything is launched."""
    from fdgs.edit import Similarity, transform

    class Split:
        gaussian_dim, rot_4d, force_sh_3d, env_map = 3, False, False, None
        active_sh_degree = active_sh_degree_t = 0
        time_duration, prefilter_var = [0.0, 1.0], -1.0
        _xyz = torch.zeros(4, 3)
        get_features = property(lambda self: torch.zeros(4, 16, 3))
    with pytest.raises(ValueError, match="_features"):
        transform(Split(), Similarity(None), inplace=True)
