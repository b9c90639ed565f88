"""GPU: fdgs.exposure (csrc/exposure.hip) against the float64 statement of tests/exposure_oracle.py on the shapes, inputs and rows of
tests/exposure_cases.py.  Every bar is derived: float32 operations round to 2^-24 relative each, float64 sums to 2^-53 per addition."""
import numpy as np
import pytest
import torch

import exposure_cases as ec
import exposure_oracle as eo
from fdgs import exposure

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def _t(x, dev):
    return torch.from_numpy(np.array(x)).to(dev)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _table(A, dev):
    """A table of three cameras with ``A`` in the middle: the kernels must read row 1 and nothing else."""
    return _t(np.stack([ec.row("random", seed=9), A, ec.row("offset100", seed=8)]), dev)


@pytest.mark.parametrize("shape", ec.SHAPES, ids=ec.shape_id)
def test_apply_against_the_oracle(shape, gpu_device):
    """|out - oracle| <= 4 * 2^-24 * (sum_j |M_ij| |c_j| + |o_i|) per element: three products and three sums, each rounded once to
    2^-24 relative of a quantity no larger than that magnitude.  In place = out of place, twice the same bits, identity = input."""
    for kind in ec.INPUTS:
        c = ec.image(kind, shape)
        img = _t(c, gpu_device)
        for rk in ec.ROWS:
            A = ec.row(rk)
            tab = _table(A, gpu_device)
            out = exposure.apply_(img, tab, 1, out=torch.empty_like(img))
            assert torch.equal(img, _t(c, gpu_device))      # the input stays
            err = np.abs(out.cpu().numpy().astype(np.float64) - eo.apply(c, A))
            bar = 4 * U * eo.apply_magnitude(c, A)
            print("%s %s %s: worst err / bar %.3f" % (ec.shape_id(shape), kind, rk, float((err / np.maximum(bar, 1e-300)).max())))
            assert (err <= bar).all(), (kind, rk, float((err - bar).max()))
            again = exposure.apply_(img, tab, 1, out=torch.empty_like(img))
            inplace = exposure.apply_(img.clone(), tab, 1)
            assert torch.equal(_bits(again), _bits(out)) and torch.equal(_bits(inplace), _bits(out))
            if rk == "identity":
                assert torch.equal(out, img)     # bit for bit, up to the sign of zero (0 * x + -0 = +0)


@pytest.mark.parametrize("shape", ec.SHAPES, ids=ec.shape_id)
def test_backward_against_the_oracle(shape, gpu_device):
    """Image gradient: the bar of apply with M^T and g'.  The 12 sums: 2^-24 |result| for the one rounding to float32 plus
    H W * 2^-52 * sum |terms| for the float64 additions (at most H W of them per sum, each 2^-53 relative of a partial sum no larger
    than sum |terms|; the products are exact).  In place = out of place, twice the same bits, the add flag adds."""
    H, W = shape
    g_np = ec.upstream(shape)
    g = _t(g_np, gpu_device)
    for kind in ec.INPUTS:
        c = ec.image(kind, shape)
        img = _t(c, gpu_device)
        for rk in ec.ROWS:
            A = ec.row(rk)
            tab = _table(A, gpu_device)
            slot = torch.full((12,), float("nan"), device=gpu_device)
            gi = exposure.backward_(g, img, tab, 1, slot, out=torch.empty_like(g))
            assert torch.equal(g, _t(g_np, gpu_device)) and torch.equal(img, _t(c, gpu_device))
            ref_gi, ref_dA = eo.backward(g_np, c, A)
            mag_gi, mag_dA = eo.backward_magnitudes(g_np, c, A)
            err = np.abs(gi.cpu().numpy().astype(np.float64) - ref_gi)
            bar = 4 * U * mag_gi
            assert (err <= bar).all(), (kind, rk, float((err - bar).max()))
            err_a = np.abs(slot.cpu().numpy().astype(np.float64) - ref_dA)
            bar_a = U * np.abs(ref_dA) + H * W * 2.0 ** -52 * mag_dA
            print("%s %s %s: dA worst err / bar %.3f" % (ec.shape_id(shape), kind, rk, float((err_a / np.maximum(bar_a, 1e-300)).max())))
            assert (err_a <= bar_a).all(), (kind, rk, err_a, bar_a)
            slot2 = torch.full((12,), float("nan"), device=gpu_device)
            g2 = g.clone()
            assert exposure.backward_(g2, img, tab, 1, slot2) is g2
            assert torch.equal(_bits(g2), _bits(gi)) and torch.equal(_bits(slot2), _bits(slot))
            slot3 = torch.full((12,), 7.0, device=gpu_device)
            gi3 = exposure.backward_(g, img, tab, 1, slot3, out=torch.empty_like(g), accumulate=True)
            assert torch.equal(_bits(gi3), _bits(gi)) and torch.equal(_bits(slot3), _bits(slot + 7.0))
            slot4 = torch.zeros(12, device=gpu_device)
            assert exposure.backward_(g, img, tab, 1, slot4, image_grad=False) is None and torch.equal(_bits(slot4), _bits(slot))


def _ulp_bar(ref, n=4):
    return n * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("indices", [[3, 0, 3], [2], [4, 4, 4, 1]], ids=["twice", "one", "thrice"])
def test_adam_step_against_the_oracle(indices, gpu_device):
    """One step from a random state: table, both moments within 4 ulp of the float64 oracle's, the counts exact; rows not named keep
    their bits; a camera named more than once gets the sum of its slots and one count."""
    rng = np.random.default_rng(21)
    N, B = 5, len(indices)
    m = exposure.ExposureModel(N, gpu_device, lr=1e-3)
    state = (rng.normal(0.3, 0.5, (N, 12)).astype(np.float32), rng.normal(0.0, 1e-3, (N, 12)).astype(np.float32),
             (rng.random((N, 12)) * 1e-5).astype(np.float32), rng.integers(0, 50, N).astype(np.int32))
    state[3][0] = 0      # a camera's first step
    slots = rng.normal(0.0, 3e-3, (B, 12)).astype(np.float32)
    for name, a in zip(("table", "exp_avg", "exp_avg_sq", "steps"), state):
        getattr(m, name).copy_(_t(a, gpu_device))
    m.step(indices, _t(slots, gpu_device))
    ref = eo.adam(*state, indices, slots, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-15)
    got = [getattr(m, name).cpu().numpy() for name in ("table", "exp_avg", "exp_avg_sq", "steps")]
    assert np.array_equal(got[3], ref[3]) and [int(ref[3][i] - state[3][i]) for i in range(N)] == [int(i in indices) for i in range(N)]
    others = [i for i in range(N) if i not in indices]
    for k in range(3):
        err = np.abs(got[k].astype(np.float64) - ref[k])
        print("quantity %d: worst err %.3f ulp" % (k, float((err / (_ulp_bar(ref[k]) / 4)).max())))
        assert (err <= _ulp_bar(ref[k])).all(), k
        assert np.array_equal(got[k][others].view(np.int32), state[k][others].view(np.int32)), k
    assert not np.array_equal(got[0][indices[0]], state[0][indices[0]])


def test_model_starts_at_the_identity_and_round_trips_its_state(gpu_device):
    m = exposure.ExposureModel(3, gpu_device, lr=2e-3, betas=(0.8, 0.99), eps=1e-12)
    assert np.array_equal(m.table.cpu().numpy(), np.tile(eo.IDENTITY.astype(np.float32), (3, 1))) and int(m.steps.sum()) == 0
    m.step([1, 2], torch.ones((2, 12), device=gpu_device))
    state = m.state_dict()
    assert all(isinstance(v, (torch.Tensor, float)) for v in state.values()) and not any(v.is_cuda for v in state.values() if isinstance(v, torch.Tensor))
    n = exposure.ExposureModel(3, gpu_device)
    n.load_state_dict(state)
    assert torch.equal(n.table, m.table) and torch.equal(n.exp_avg_sq, m.exp_avg_sq) and n.steps.tolist() == [0, 1, 1]
    assert (n.lr, n.betas, n.eps) == (2e-3, (0.8, 0.99), 1e-12)
    # Adam's first step moves every element by lr against the gradient's sign
    assert np.allclose(m.table.cpu().numpy()[1], eo.IDENTITY - 2e-3, atol=1e-6)

    class Cam:
        uid = 2
    assert m.index_of(Cam()) == 2
    Cam.uid = 3
    with pytest.raises(ValueError):
        m.index_of(Cam())
    with pytest.raises(ValueError, match="outside the table"):
        exposure.apply_(torch.zeros((3, 2, 2), device=gpu_device), m, 3)


def test_fit_affine_against_the_oracle(gpu_device):
    """|A - oracle| <= 2^-23 max(1, max |A|) + cond * H W * 2^-50: the float32 row's rounding, and the float64 moments' summation
    error (H W * 2^-53 relative) through a solve of condition number cond; cond <= 1e4 for every noise case (asserted by the case
    list), so the second term stays below 1e-7 and cannot hide a wrong answer.  The moments themselves: H W * 2^-52 * sum |terms|."""
    for shape, c, gt, A, cond in ec.fit_cases():
        H, W = shape
        got = exposure.fit_affine(_t(c, gpu_device), _t(gt, gpu_device)).cpu().numpy().astype(np.float64)
        bar = 2.0 ** -23 * max(1.0, np.abs(A).max()) + cond * H * W * 2.0 ** -50
        print("%s: cond %.1f err %.3e bar %.3e" % (ec.shape_id(shape), cond, np.abs(got - A).max(), bar))
        assert cond * H * W * 2.0 ** -50 < 1e-7 and np.abs(got - A).max() <= bar
        for clamp, img in ((True, ec.image("wild", shape)), (False, ec.image("wild", shape)), (True, c)):
            mom = exposure.fit_moments(_t(img, gpu_device), _t(gt, gpu_device), clamp=clamp).cpu().numpy()
            M, N, n = eo.fit_moments(img, gt, clamp=clamp)
            Ma, Na, _ = eo.fit_moments(np.abs(np.clip(img, 0, 1) if clamp else img), np.abs(gt), clamp=False)
            ref = np.concatenate([M[np.triu_indices(4)], N.reshape(12)])
            mag = np.concatenate([Ma[np.triu_indices(4)], Na.reshape(12)])
            assert n == H * W and (np.abs(mom - ref) <= H * W * 2.0 ** -52 * mag).all(), (shape, clamp)
            again = exposure.fit_moments(_t(img, gpu_device), _t(gt, gpu_device), clamp=clamp).cpu().numpy()
            assert np.array_equal(again, mom)
    # a clamped image far outside [0, 1]: still a well-conditioned case, against the oracle under the same bar
    shape = (64, 64)
    img, gt = ec.image("wild", shape), ec.fit_pair(shape)[1]
    A, cond = eo.fit_affine(img, gt, 1e-6, clamp=True, return_cond=True)
    assert cond <= ec.COND_MAX
    got = exposure.fit_affine(_t(img, gpu_device), _t(gt, gpu_device)).cpu().numpy().astype(np.float64)
    assert np.abs(got - A).max() <= 2.0 ** -23 * max(1.0, np.abs(A).max()) + cond * 64 * 64 * 2.0 ** -50
    for shape in ((3, 5), (1, 1)):
        const = _t(ec.image("constant", shape), gpu_device)
        row = exposure.fit_affine(const, const)
        assert row.shape == (12,) and row.dtype == torch.float32 and bool(torch.isfinite(row).all())


@pytest.mark.parametrize("shape", [(17, 65), (64, 64)], ids=ec.shape_id)
def test_autograd_gives_the_raw_calls_gradients(shape, gpu_device):
    c, w, A = ec.image("wild", shape), ec.upstream(shape), ec.row("random")
    img = _t(c, gpu_device).requires_grad_(True)
    tab = _table(A, gpu_device).requires_grad_(True)
    out = exposure.apply(img, tab, 1)
    assert torch.equal(_bits(out.detach()), _bits(exposure.apply_(img.detach(), tab, 1, out=torch.empty_like(out))))
    (out * _t(w, gpu_device)).sum().backward()
    slot = torch.empty(12, device=gpu_device)
    gi = exposure.backward_(_t(w, gpu_device), img.detach(), tab, 1, slot, out=torch.empty_like(out))
    assert torch.equal(_bits(img.grad), _bits(gi)) and torch.equal(_bits(tab.grad[1]), _bits(slot))
    assert not tab.grad[0].any() and not tab.grad[2].any()
    # the image alone, and through an ExposureModel
    m = exposure.ExposureModel(3, gpu_device)
    m.table.copy_(tab.detach())
    img2 = _t(c, gpu_device).requires_grad_(True)
    (exposure.apply(img2, m, 1) * _t(w, gpu_device)).sum().backward()
    assert torch.equal(_bits(img2.grad), _bits(gi))
