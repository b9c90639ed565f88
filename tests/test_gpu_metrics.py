"""GPU: the evaluation metrics kernels (csrc/metrics.hip, fdgs.metrics) against fixtures made with the reference's own l1_loss /
psnr / ssim (tests/golden/make_golden_metrics.py) and against the float64 oracle (tests/metrics_oracle.py) up to C3 size."""
import glob
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_cases as lc
import metrics_oracle as mo

pytestmark = pytest.mark.gpu

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics", "metrics_*.npz")))
BARS = (2e-6, 1e-4, 2e-6, 1e-5)   # l1, psnr (dB), ssim, msssim: absolute
NAMES = ("l1", "psnr", "ssim", "msssim")


def pair(shape, seed):
    """A smooth render-like image partly outside [0, 1] and a correlated ground truth."""
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(shape[0], shape[1] // 8 + 2, shape[2] // 8 + 2, generator=g)
    up = F.interpolate(base[None], size=shape[1:], mode="bilinear", align_corners=False)[0]
    img = 1.2 * up - 0.1 + 0.05 * torch.randn(shape, generator=g)
    gt = (0.8 * up + 0.2 * torch.rand(shape, generator=g)).clamp(0, 1)
    return img, gt


def check(got, want, what):
    errs = [abs(float(got[k]) - want[k]) for k in range(4)]
    print("%s: |err| l1 %.2e psnr %.2e ssim %.2e msssim %.2e" % ((what,) + tuple(errs)))
    for k in range(4):
        if math.isnan(want[k]):
            assert math.isnan(float(got[k])), (what, NAMES[k])
        else:
            assert errs[k] <= BARS[k], (what, NAMES[k], float(got[k]), want[k])


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:-4] for p in GOLDEN])
def test_kernels_match_reference_fixtures(path, gpu_device):
    from fdgs.metrics import image_metrics
    f = np.load(path)
    img = torch.from_numpy(f["img"]).float().to(gpu_device)
    gt = (torch.from_numpy(f["gt"]).float() / 255.0).to(gpu_device)
    got = image_metrics(img, gt).cpu()
    check(got, [float(f[k]) for k in NAMES], os.path.basename(path))


# 176^2: the minimum; 201 x 333: odd sides at every scale; 400^2, 800^2, 1014 x 1352: C1, C2, C3
@pytest.mark.parametrize("shape", [(3, 176, 176), (3, 201, 333), (3, 400, 400), (3, 800, 800), (3, 1014, 1352)])
def test_kernels_match_oracle(shape, gpu_device):
    from fdgs.metrics import image_metrics
    img, gt = pair(shape, sum(shape))
    got = image_metrics(img.to(gpu_device), gt.to(gpu_device)).cpu()
    check(got, mo.metrics(img, gt), "x".join(map(str, shape)))


def test_ssim_equals_the_training_loss_ssim(gpu_device):
    from fdgs.loss import fused_l1_ssim
    from fdgs.metrics import image_metrics, ssim
    img, gt = pair((3, 1014, 1352), 11)
    img, gt = img.to(gpu_device), gt.to(gpu_device)
    row = image_metrics(img, gt)
    train_ssim = 1.0 - float(fused_l1_ssim(img.clamp(0, 1), gt, 1.0))   # lambda = 1: the loss is 1 - SSIM
    assert abs(float(row[2]) - train_ssim) <= 1e-6, (float(row[2]), train_ssim)
    assert abs(float(ssim(img.clamp(0, 1), gt)) - train_ssim) <= 1e-6


def test_rows_are_bitwise_reproducible(gpu_device):
    from fdgs.metrics import image_metrics
    img, gt = pair((3, 1014, 1352), 12)
    img, gt = img.to(gpu_device), gt.to(gpu_device)
    rows = torch.empty((3, 4), dtype=torch.float32, device=gpu_device)
    image_metrics(img, gt, out=rows[0])
    other, other_gt = pair((3, 1014, 1352), 13)
    image_metrics(other.to(gpu_device), other_gt.to(gpu_device), out=rows[1])   # another view in between
    image_metrics(img, gt, out=rows[2])
    r = rows.cpu()
    assert torch.equal(r[0].view(torch.int32), r[2].view(torch.int32)), r


def test_clamp_flag(gpu_device):
    from fdgs.metrics import image_metrics
    img, gt = pair((3, 200, 240), 14)
    assert float(img.min()) < 0 and float(img.max()) > 1
    d_img, d_gt = img.to(gpu_device), gt.to(gpu_device)
    check(image_metrics(d_img, d_gt, clamp=True).cpu(), mo.metrics(img, gt, clamp=True), "clamped")
    check(image_metrics(d_img, d_gt, clamp=False).cpu(), mo.metrics(img, gt, clamp=False), "unclamped")
    assert abs(float(image_metrics(d_img, d_gt, clamp=True)[0]) - float(image_metrics(d_img, d_gt, clamp=False)[0])) > 1e-3


def test_skip_msssim_allows_small_images(gpu_device):
    from fdgs.metrics import image_metrics, psnr, ssim
    img, gt = pair((3, 64, 64), 15)
    d_img, d_gt = img.to(gpu_device), gt.to(gpu_device)
    got = image_metrics(d_img, d_gt, msssim=False).cpu()
    check(got, mo.metrics(img, gt, with_msssim=False), "64x64 without MS-SSIM")
    p, s = psnr(d_img, d_gt), ssim(d_img, d_gt)
    assert p.dim() == 0 and p.is_cuda and s.dim() == 0 and s.is_cuda
    assert abs(float(p) - mo.psnr(img, gt, clamp=False)) <= BARS[1]
    assert abs(float(s) - mo.ssim(img, gt, clamp=False)) <= BARS[2]


@pytest.mark.parametrize("shape", list(lc.EDGE_SHAPES), ids=["x".join(map(str, s)) for s in lc.EDGE_SHAPES])
def test_edge_shapes_match_oracle(shape, gpu_device):
    """L1 / PSNR / SSIM without MS-SSIM on the edge shapes of the loss kernels (loss_cases.EDGE_SHAPES: sides of 1, sides below the
    window, ragged tiles, tile counts around the 8 XCD chunks): the scale kernel shares its halo load and window passes with them.
    Every one of the 17 shapes is run: the float64 oracle is finite on all of them with these inputs (img != gt everywhere: PSNR of
    identical images is +inf), asserted here before the comparison."""
    from fdgs.metrics import image_metrics
    img, gt = pair(shape, 100 + sum(shape))
    want = mo.metrics(img, gt, with_msssim=False)
    assert all(math.isfinite(w) for w in want[:3]) and math.isnan(want[3]), want
    got = image_metrics(img.to(gpu_device), gt.to(gpu_device), msssim=False).cpu()
    check(got, want, "x".join(map(str, shape)))


@pytest.mark.parametrize("H,W,side", [(175, 240, "height"), (240, 175, "width"), (64, 64, "height")])
def test_too_small_for_msssim_raises(H, W, side, gpu_device):
    from fdgs import _capi
    from fdgs.metrics import image_metrics, msssim
    img, gt = pair((3, H, W), 16)
    img, gt = img.to(gpu_device), gt.to(gpu_device)
    with pytest.raises(ValueError, match="For a given number of `betas` parameters 5 and kernel size 11, the image %s must be larger than 160" % side):
        image_metrics(img, gt)
    with pytest.raises(ValueError, match="must be larger than 160"):
        msssim(img, gt)
    # the C entry refuses it too, naming the limit
    out = torch.empty(4, device=gpu_device)
    scratch = torch.empty(max(_capi.lib.fdgs_eval_metrics_scratch_bytes(3, H, W), 256), dtype=torch.uint8, device=gpu_device)
    rc = _capi.lib.fdgs_eval_metrics(img.data_ptr(), gt.data_ptr(), 3, H, W, 1, scratch.data_ptr(), out.data_ptr(),
                                     _capi.current_stream_handle(gpu_device))
    assert rc == 1 and "176" in _capi.last_error()


def test_single_channel(gpu_device):
    from fdgs.metrics import image_metrics, msssim
    img, gt = pair((1, 200, 240), 17)
    got = image_metrics(img.to(gpu_device), gt.to(gpu_device)).cpu()
    check(got, mo.metrics(img, gt), "1x200x240")
    m = msssim(img.clamp(0, 1).to(gpu_device), gt.to(gpu_device))
    assert m.dim() == 0 and abs(float(m) - mo.msssim(img, gt)) <= BARS[3]


def test_identical_images(gpu_device):
    from fdgs.metrics import image_metrics
    _, gt = pair((3, 180, 190), 18)
    row = image_metrics(gt.to(gpu_device), gt.to(gpu_device)).cpu()
    assert float(row[0]) == 0.0 and math.isinf(float(row[1])) and float(row[1]) > 0
    assert abs(float(row[2]) - 1.0) <= 1e-6 and abs(float(row[3]) - 1.0) <= 1e-5
