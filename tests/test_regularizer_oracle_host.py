"""The CPU oracle of the regularisers and the k-NN query (tests/regularizer_oracle.py) against independent statements:
scipy's k-d tree, the model's pinned covariance code, and float64 finite differences.  No GPU."""
import numpy as np
import pytest
import torch

import util  # noqa: F401
import regularizer_oracle as ro
from fdgs import synth
from fdgs.train_host import ReferenceStyleModel


def _model(P, seed):
    cfg = synth.SceneConfig("reg", P, 64, 48, 1, 1, 0.05, 10.0, True, 4, False)
    scene = synth.make_scene(cfg, seed=seed)
    m = ReferenceStyleModel(scene, "cpu")
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():   # raw quaternions of any norm, as the model stores them
        m._rotation.mul_(0.5 + 1.5 * torch.rand(P, 1, generator=g))
        m._rotation_r.mul_(0.5 + 1.5 * torch.rand(P, 1, generator=g))
        m._scaling_t.add_(torch.randn(P, 1, generator=g) * 0.3)
    return m


def _params(m):
    return {n: getattr(m, n).detach() for n in ("_scaling", "_scaling_t", "_rotation", "_rotation_r", "_t")}


@pytest.mark.parametrize("n,m,k", [(300, 500, 20), (200, 200, 1), (150, 90, 64), (50, 7, 20)])
def test_knn_oracle_matches_kdtree(n, m, k):
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(n + m + k)
    x = rng.standard_normal((n, 3)).astype(np.float32)
    src = rng.standard_normal((m, 3)).astype(np.float32)
    idx, d2 = ro.knn(x, src, k)
    kk = min(k, m)
    dd, ii = cKDTree(src.astype(np.float64)).query(x.astype(np.float64), k=kk)
    ii = np.asarray(ii).reshape(n, kk)
    for r in range(n):
        assert set(idx[r, :kk].tolist()) == set(ii[r].tolist())
    np.testing.assert_allclose(d2[:, :kk], np.asarray(dd).reshape(n, kk) ** 2, rtol=1e-5, atol=1e-6)
    assert (np.diff(d2, axis=1) >= 0).all()
    if m < k:
        assert (d2[:, m:] == 1e10).all() and (idx[:, m:] == 0).all()


def test_knn_oracle_ties_go_to_the_lower_index():
    src = np.array([[1, 0, 0], [0, 0, 0], [1, 0, 0], [0, 0, 0], [2, 0, 0]], dtype=np.float32)
    idx, d2 = ro.knn(src[:1], src, 4)
    assert idx[0].tolist() == [0, 2, 1, 3] and d2[0].tolist() == [0, 0, 1, 1]


def test_velocity_matches_the_pinned_model_covariance():
    m = _model(257, 3)
    want = m.get_current_covariance_and_mean_offset(1.0, m.get_t + 0.1)[1]
    got32 = ro.velocity(m._scaling, m._scaling_t, m._rotation, m._rotation_r, m._t, torch.float32)
    torch.testing.assert_close(got32, want, rtol=1e-5, atol=1e-7)
    got64 = ro.velocity(m._scaling, m._scaling_t, m._rotation, m._rotation_r, m._t, torch.float64)
    torch.testing.assert_close(got64.float(), want, rtol=1e-4, atol=1e-6)


def _fd_check(fun, leaves, eps=1e-6, rows=6):
    out = fun(**leaves)
    grads = torch.autograd.grad(out, list(leaves.values()))
    for (name, t), g in zip(leaves.items(), grads):
        for r in range(min(rows, t.shape[0])):
            for c in range(t.shape[1]):
                tp = {n: v.detach().clone() for n, v in leaves.items()}
                tm = {n: v.detach().clone() for n, v in leaves.items()}
                tp[name][r, c] += eps
                tm[name][r, c] -= eps
                fd = (float(fun(**tp)) - float(fun(**tm))) / (2 * eps)
                assert abs(fd - float(g[r, c])) <= 1e-6 * max(1.0, abs(fd)), (name, r, c, fd, float(g[r, c]))


def test_rigid_and_motion_gradients_match_finite_differences():
    m = _model(40, 5)
    p = _params(m)
    xyz = m._xyz.detach().numpy()
    idx, d2 = ro.knn(xyz, xyz, 8)
    idx, d2 = torch.from_numpy(idx), torch.from_numpy(d2) * 1e-3   # O(1) weights
    leaves = {n: p[n].double().clone().requires_grad_(True) for n in ("_scaling", "_scaling_t", "_rotation", "_rotation_r")}

    def fun(_scaling, _scaling_t, _rotation, _rotation_r):
        v = ro.velocity(_scaling, _scaling_t, _rotation, _rotation_r, p["_t"])
        return ro.rigid(v, idx, d2) + 0.7 * ro.motion(v)
    _fd_check(fun, leaves)


def test_norm_gradient_at_a_zero_difference_is_zero():
    v = torch.tensor([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [0.0, 0.0, 0.0]], dtype=torch.float64, requires_grad=True)
    idx = torch.tensor([[0, 1], [1, 0], [2, 0]])
    d2 = torch.zeros(3, 2, dtype=torch.float64)
    (ro.rigid(v, idx, d2) + ro.motion(v)).backward()
    assert torch.isfinite(v.grad).all()
    # the pairs (0, 1) and (1, 0) are exact duplicates: they contribute nothing, only the motion term and the pair (2, 0) do
    w = 1.0 / 3.0 / 2.0
    u = v.detach()[0] / v.detach()[0].norm()
    torch.testing.assert_close(v.grad[0], u / 3 + w * u)
    torch.testing.assert_close(v.grad[2], -w * u)


def test_opa_mask_gradient_matches_finite_differences_and_the_clamp():
    g = torch.Generator().manual_seed(0)
    alpha = torch.rand(1, 6, 7, generator=g, dtype=torch.float64) * 0.98 + 0.01
    mask = (torch.rand(1, 6, 7, generator=g) > 0.5).double()
    a = alpha.clone().requires_grad_(True)
    ro.opa_mask(a, mask).backward()
    sky = 1 - mask
    torch.testing.assert_close(a.grad, sky / (1 - alpha) / alpha.numel())
    _fd_check(lambda alpha: ro.opa_mask(alpha, mask[0]), {"alpha": alpha[0].clone().requires_grad_(True)}, eps=1e-7)
    # clamp bounds: the gradient passes at both bounds (inclusive) and is 0 beyond
    edge = torch.tensor([[[1e-6, 1 - 1e-6, 0.0, 1.0, -0.5, 1.5]]], dtype=torch.float64, requires_grad=True)
    ro.opa_mask(edge, torch.zeros_like(edge)).backward()
    gg = edge.grad[0, 0]
    assert gg[0] > 0 and gg[1] > 0 and (gg[2:] == 0).all()
