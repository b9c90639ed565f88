"""The CPU oracle of the regularisers and the k-NN query (tests/regularizer_oracle.py) against independent statements:
scipy's k-d tree, the model's pinned covariance code, and float64 finite differences; and the proof that the bar the GPU tests hold
the regulariser gradients to (regularizer_oracle.grad_bar) accepts the float32 statement and rejects wrong gradients on every shared
case (tests/regularizer_cases.py).  No GPU."""
import numpy as np
import pytest
import torch

import util  # noqa: F401
import regularizer_cases as rc
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


# ---- the bar of the rigid / motion gradients (regularizer_oracle.grad_bar) discriminates ----

ALL_SPECS = rc.MODEL_SPECS + rc.TABLE_SPECS
WELL = ("_scaling", "_rotation", "_rotation_r")     # float32 reaches ~4e-7 of max|ref| on these; _scaling_t is a cancelling sum


def _wrong_grads(case, w, kind):
    """The float64 gradients of a deliberately wrong statement, by autograd:  no_neighbour / no_query: one side of the rigid pairs
    detached;  no_k: the division by k missing;  dt: dt taken as exactly 0.1 instead of (t + 0.1f) - t."""
    leaves = {n: case.params[n].double().clone().requires_grad_(True) for n in ro.NAMES4}
    v = ro.velocity(*[leaves[n] for n in ro.NAMES4], case.params["_t"], torch.float64, dt=0.1 if kind == "dt" else None)
    mask = torch.ones_like(case.idx, dtype=torch.bool) if case.mask is None else case.mask
    idx = torch.where(mask, case.idx, torch.zeros_like(case.idx))
    vn, vq = v[idx], v[:, None, :]
    if kind == "no_neighbour":
        vn = vn.detach()
    if kind == "no_query":
        vq = vq.detach()
    lr = (torch.exp(-100 * case.d2.double()) * mask.double() * torch.norm(vn - vq, p=2, dim=-1)).sum() / case.k / case.P
    if kind == "no_k":
        lr = lr * case.k
    (w[0] * lr + w[1] * ro.motion(v)).backward()
    return {n: t.grad.detach() for n, t in leaves.items()}


@pytest.mark.parametrize("spec", ALL_SPECS, ids=rc.spec_id)
def test_the_bar_accepts_float32_and_rejects_wrong_gradients(spec):
    case = rc.case_of(spec)      # the builder asserts the case's conditions: finite, median pair weight >= 0.01, L_rigid's share >= 10 %
    for w in rc.WEIGHTS:
        bars = ro.grad_bar(case.params, case.idx, case.d2, w[0], w[1], case.mask)
        g32 = ro.rigid_motion_with_grads(case.params, case.idx, case.d2, torch.float32, w[0], w[1], case.mask)[2]
        g64 = {n: bars[n].ref for n in ro.NAMES4}
        right = _wrong_grads(case, w, "none")
        for n in ro.NAMES4:
            assert bars[n].accepts(g32[n]), (case, w, n)
            assert bars[n].accepts(right[n]), (case, w, n)          # the restatement below is the oracle's when nothing is wrong
            assert bars[n].bar <= 64 * 4e-3 * bars[n].ref_max, (case, w, n, bars[n].bar, bars[n].ref_max)   # never a floor
        live = [n for n in ro.NAMES4 if bars[n].ref_max > 0]
        assert case.zero or w[1] == 0 or len(live) == 4
        # a, b, c: a side of the rigid pairs dropped, the division by k missing
        kinds = ["no_neighbour", "no_query"] + (["no_k"] if case.k > 1 else [])
        if case.rigid and w[0] > 0:
            assert len(live) == 4
            for kind in kinds:
                wrong = _wrong_grads(case, w, kind)
                for n in WELL:
                    assert not bars[n].accepts(wrong[n]), (case, w, kind, n, bars[n].err(wrong[n]), bars[n].bar)
        # e, f: one tensor zeroed, one tensor scaled by 1 + 1e-2
        for n in live:
            assert not bars[n].accepts(torch.zeros_like(g64[n])), (case, w, "zeroed", n)
            if n in WELL:
                assert not bars[n].accepts(g64[n] * (1 + 1e-2)), (case, w, "scaled", n, bars[n].bar / bars[n].ref_max)


@pytest.mark.parametrize("spec", [s for s in rc.MODEL_SPECS if s[0] == "late_t"], ids=rc.spec_id)
def test_the_bar_rejects_dt_taken_as_a_tenth(spec):
    """d: dt = 0.1 where (t + 0.1f) - t is not.  For every t in [32, 64) the float32 dt is 26214 * 2^-18 = 0.0999985, 1.5e-5 below
    0.1, so every gradient element of such a Gaussian is off by 1.5e-5 of itself: 20 to 40 times what float32 resolves on _scaling, _rotation
    and _rotation_r, but inside the float32 error of _scaling_t.  The set of four tensors has to be rejected."""
    case = rc.case_of(spec)
    for w in rc.WEIGHTS:
        bars = ro.grad_bar(case.params, case.idx, case.d2, w[0], w[1], case.mask)
        wrong = _wrong_grads(case, w, "dt")
        caught = [n for n in ro.NAMES4 if not bars[n].accepts(wrong[n])]
        print("%s %s dt = 0.1: error / bar %s" % (case, w, {n: round(bars[n].err(wrong[n]) / bars[n].bar, 2) for n in ro.NAMES4}))
        assert caught, (case, w, "dt", {n: (bars[n].err(wrong[n]), bars[n].bar) for n in ro.NAMES4})


@pytest.mark.parametrize("which", ["synth-P700-k20", "compact-P1025-k20", "thin_time-P255-k20"])
def test_smallest_scale_error_the_bar_detects_on_scaling_t(which):
    """_scaling_t only: its float32 statement is off by e32 (a cancelling sum), so a factor nearer to 1 than 1 + bar / max|ref| passes.
    States that factor; 1 + 1e-2 is rejected wherever it is larger."""
    if which.startswith("synth"):    # the model of tests/test_gpu_regularizers.py::test_rigid_motion_vs_float64_oracle[small]
        m = _model(700, 700)
        xyz = m._xyz.detach().numpy()
        idx, d2 = ro.knn(xyz, xyz, 20)
        params, idx, d2, mask = _params(m), torch.from_numpy(idx), torch.from_numpy(d2), None
    else:
        case = rc.case_of(next(s for s in ALL_SPECS if rc.spec_id(s) == which))
        params, idx, d2, mask = case.params, case.idx, case.d2, case.mask
    bar = ro.grad_bar(params, idx, d2, 1.0, 0.5, mask)["_scaling_t"]
    smallest = bar.bar / bar.ref_max
    print("%s _scaling_t: max|ref| %.2e, e32 / max|ref| %.2e, smallest scale error detected: a factor of 1 + %.2e"
          % (which, bar.ref_max, bar.e32 / bar.ref_max, smallest))
    assert smallest < 0.5          # a zeroed or halved tensor is always caught
    assert not bar.accepts(bar.ref * (1 + 1.01 * smallest)) and bar.accepts(bar.ref * (1 + 0.5 * smallest))
    if smallest < 1e-2:
        assert not bar.accepts(bar.ref * (1 + 1e-2))
