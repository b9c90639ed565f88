"""CPU: the float64 statement of the evaluation metrics (tests/metrics_oracle.py) against fixtures made with the reference's own
l1_loss / psnr / ssim (tests/golden/make_golden_metrics.py), and the properties that pin its MS-SSIM definition."""
import glob
import math
import os

import numpy as np
import pytest
import torch

import metrics_oracle as mo

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics", "metrics_*.npz")))


def load(path):
    f = np.load(path)
    return torch.from_numpy(f["img"]), torch.from_numpy(f["gt"]).to(torch.float64) / 255.0, f


def test_fixtures_exist():
    assert len(GOLDEN) == 3


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:-4] for p in GOLDEN])
def test_oracle_reproduces_the_fixtures(path):
    img, gt, f = load(path)
    assert float(img.min()) < 0.0 and float(img.max()) > 1.0   # the clamp matters
    got = mo.metrics(img, gt)
    assert abs(got[0] - float(f["l1"])) <= 1e-12
    assert abs(got[1] - float(f["psnr"])) <= 1e-9
    assert abs(got[2] - float(f["ssim"])) <= 1e-7   # the same float32-rounded window, float64 sums in another order
    assert abs(got[3] - float(f["msssim"])) <= 1e-12


def test_msssim_of_an_image_with_itself_is_one():
    g = torch.Generator().manual_seed(0)
    x = torch.rand(3, 180, 200, generator=g, dtype=torch.float64)
    assert abs(mo.msssim(x, x) - 1.0) <= 1e-12
    assert math.isinf(mo.psnr(x, x))


@pytest.mark.parametrize("path", GOLDEN[:1], ids=["176"])
def test_one_scale_equals_the_interior_of_the_reference_ssim_map(path):
    """beta = (1,): MS-SSIM is the mean of the valid-window SSIM map, i.e. the reference's zero-padded map over [5:-5, 5:-5]."""
    img, gt, f = load(path)
    assert abs(mo.msssim(img, gt, betas=(1.0,)) - float(f["ssim_interior"])) <= 1e-7


def test_negative_coarse_contrast_gives_zero():
    """An image against its negative has CS < 0 at the coarse scales: the relu makes MS-SSIM 0."""
    g = torch.Generator().manual_seed(1)
    base = torch.rand(1, 1, 12, 12, generator=g, dtype=torch.float64)
    x = torch.nn.functional.interpolate(base, size=(192, 192), mode="bilinear", align_corners=False)[0]
    y = 1.0 - x
    terms = mo.msssim_terms(x, y)
    assert any(cs == 0.0 for _, cs in terms[:4])
    assert mo.msssim(x, y) == 0.0


@pytest.mark.parametrize("H,W,side", [(175, 200, "height"), (200, 175, "width")])
def test_sides_below_176_are_rejected(H, W, side):
    x = torch.zeros(3, H, W, dtype=torch.float64)
    with pytest.raises(ValueError, match="the image %s must be larger than 160" % side):
        mo.msssim(x, x)
    mo.msssim(torch.zeros(3, 176, 176, dtype=torch.float64), torch.zeros(3, 176, 176, dtype=torch.float64))


def test_single_channel_and_psnr_per_channel_mean():
    g = torch.Generator().manual_seed(2)
    x = torch.rand(2, 40, 50, generator=g, dtype=torch.float64)
    y = torch.rand(2, 40, 50, generator=g, dtype=torch.float64)
    want = np.mean([20 * math.log10(1.0 / math.sqrt(float(((x[c] - y[c]) ** 2).mean()))) for c in range(2)])
    assert abs(mo.psnr(x, y) - want) <= 1e-12
    assert abs(mo.ssim(x[:1], y[:1]) - mo.ssim(x[:1], y[:1], clamp=False)) <= 1e-15
