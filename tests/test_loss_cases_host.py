"""CPU: pins tests/loss_cases.py -- the input classes, the two references and the error bars that tests/test_gpu_loss_edges.py
holds the HIP loss kernels to -- so that the GPU test cannot be quietly emptied: every class is there and deterministic, the
float32 reference stays useful on every class (and tight on the well-conditioned ones: that figure is the floor of every bar),
and the float64 reference reproduces the fixtures the reference's own utils/loss_utils.py produced."""
import glob
import os

import numpy as np
import pytest
import torch

import loss_cases as lc

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ssim_*.npz")))
SHAPE, LAM = (3, 48, 70), 0.2
NAMES = ["noise", "smooth", "white_bg", "white_bg_exact", "const_pair", "identical", "black", "unclamped"]
ZERO_GRADIENT = ("identical", "black")     # img == gt: the true gradient is 0 everywhere


def test_every_class_is_there():
    assert list(lc.CLASSES) == NAMES


@pytest.mark.parametrize("name", NAMES)
def test_float32_reference_is_within_its_cap(name):
    """|g_ref32 - g_ref64|_inf <= 1e-3 max|g_ref64| on every class (measured worst: const_pair, 4.4e-4), <= 1e-5 on noise and smooth
    (measured 1.3e-6 and 2.6e-6).  The two classes whose true gradient is 0 have no scale of their own (max|g_ref64| is 0 for black, 1e-19
    of fp64 rounding for identical): theirs is the noise case's max|g_ref64|, the scale their GPU bar is drawn on as well."""
    c = lc.case(name, SHAPE, LAM)
    scale = lc.case("noise", SHAPE, LAM).grad_max if name in ZERO_GRADIENT else c.grad_max
    print("%-15s ref32 gradient err %.2e = %.2e of max|g| %.2e; value err %.2e; bars %.2e / %.2e"
          % (name, c.err_g, c.err_g / scale, scale, c.err_v, c.bar_g, c.bar_v))
    assert scale > 1e-6
    assert c.err_g <= 1e-3 * scale, (c.err_g, scale)
    if name in ("noise", "smooth"):
        assert c.err_g <= 1e-5 * scale, (c.err_g, scale)
    if name in ZERO_GRADIENT:
        assert c.grad_max <= 1e-12 * scale and abs(c.loss64) <= 1e-12
    # the bars are the formula, from the references alone
    floor = lc.case("noise", SHAPE, LAM)
    assert c.bar_g == 4.0 * max(c.err_g, floor.err_g) and c.bar_g > 0.0
    assert c.bar_v == max(2e-6, 4.0 * max(c.err_v, floor.err_v))


@pytest.mark.parametrize("name", NAMES)
def test_generators_are_deterministic_float32_and_what_they_say(name):
    f = lc.CLASSES[name]
    img, gt = f(SHAPE, 5)
    img2, gt2 = f(SHAPE, 5)
    assert img.dtype == gt.dtype == torch.float32 and tuple(img.shape) == tuple(gt.shape) == SHAPE
    assert torch.equal(img, img2) and torch.equal(gt, gt2)
    assert torch.isfinite(img).all() and torch.isfinite(gt).all()
    if name in ("noise", "smooth", "white_bg", "white_bg_exact", "unclamped"):
        other = f(SHAPE, 6)[0]
        assert not torch.equal(img, other)
    if name == "identical":
        assert torch.equal(img, gt) and float(img.std()) > 0.2
    if name == "black":
        assert not img.any() and not gt.any()
    if name == "const_pair":
        assert (img == 0.7).all() and (gt == 0.701).all()
    if name == "unclamped":
        assert float(img.min()) < -0.4 and float(img.max()) > 3.4 and 0.0 <= float(gt.min()) and float(gt.max()) < 1.0
    if name in ("white_bg", "white_bg_exact"):
        white = gt == 1.0
        assert 0.5 < float(white.float().mean()) < 0.8 and bool(white[:, 0, :].all()) and not bool(white[:, SHAPE[1] // 2, SHAPE[2] // 2].any())
        assert 0.0 <= float(img.min()) and float(img.max()) <= 1.0
        d = (img - gt).abs()
        assert 0.005 < float(d[~white].mean()) < 0.03        # 0.02 N(0, 1) inside the disc
        if name == "white_bg_exact":
            assert torch.equal(img[white], gt[white])
        else:
            assert 0.0 < float(d[white].mean()) < 0.002      # 0.002 N(0, 1) clamped at 1: half of it survives


def test_smooth_is_the_pair_of_the_gpu_loss_test():
    """tests/test_gpu_loss.py::test_fused_l1_ssim_matches_reference_loss drew these inputs inline before they moved to loss_cases: same
    draws from the same generator in the same order."""
    shape = (3, 77, 131)
    g = torch.Generator().manual_seed(5)
    base = torch.rand(shape[0], shape[1] // 4 + 2, shape[2] // 4 + 2, generator=g)
    up = torch.nn.functional.interpolate(base[None], size=shape[1:], mode="bilinear", align_corners=False)[0]
    img = (up + 0.1 * torch.randn(shape, generator=g)).clamp(0, 1)
    gt = (up.flip(-1) * 0.5 + 0.5 * torch.rand(shape, generator=g)).clamp(0, 1)
    a, b = lc.smooth(shape, 5)
    assert torch.equal(a, img) and torch.equal(b, gt)


def test_fixtures_present():
    assert len(GOLDEN) >= 4


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:-4] for p in GOLDEN])
def test_ref64_reproduces_the_reference_fixtures(path):
    f = np.load(path)
    loss, grad = lc.reference(torch.from_numpy(f["img"]), torch.from_numpy(f["gt"]), float(f["lam"]), torch.float64)
    assert abs(loss - float(f["loss"])) <= 1e-12
    assert float(np.abs(grad.numpy() - f["dloss_dimg"]).max()) <= 1e-12
    # ... and the float32 evaluation of the same statement sits where the bars assume it does
    loss32, grad32 = lc.reference(torch.from_numpy(f["img"]), torch.from_numpy(f["gt"]), float(f["lam"]), torch.float32)
    assert abs(loss32 - float(f["loss"])) <= 2e-6
    assert float(np.abs(grad32.double().numpy() - f["dloss_dimg"]).max()) <= 1e-4 * float(np.abs(f["dloss_dimg"]).max())
