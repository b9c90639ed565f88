"""Golden fixtures for the evaluation metrics (fdgs.metrics, csrc/metrics.hip).  L1, PSNR and SSIM come from the REFERENCE's own
``utils/loss_utils.l1_loss`` / ``ssim`` and ``utils/image_utils.psnr`` evaluated in float64 on ``clamp(render, 0, 1)`` as
training_report does (train.py:318-326); the reference's missing import (torchmetrics, used by ``msssim`` only) is stubbed, so
MS-SSIM comes from the written definition in tests/metrics_oracle.py.  ``ssim_interior`` is the mean over [5:-5, 5:-5] of the
SSIM map built from the reference's ``create_window`` and the convolutions of ``_ssim`` (which itself returns only means): the
one-scale MS-SSIM of the oracle must equal it.

The ground truth is stored as uint8 (PNG data; gt = u8 / 255), the render as float16 with values outside [0, 1] so that the
clamp matters.

    python tests/golden/make_golden_metrics.py   ->   tests/golden/metrics/*.npz
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import metrics_oracle  # noqa: E402

REF = "/root/reference"
tm = types.ModuleType("torchmetrics")
tm.MultiScaleStructuralSimilarityIndexMeasure = lambda **k: None
sys.modules["torchmetrics"] = tm


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref_loss = _load("ref_loss_utils", os.path.join(REF, "utils", "loss_utils.py"))
ref_image = _load("ref_image_utils", os.path.join(REF, "utils", "image_utils.py"))

CASES = {"metrics_3x176x176": ((3, 176, 176), 1), "metrics_3x201x333": ((3, 201, 333), 2), "metrics_3x256x320": ((3, 256, 320), 3)}


def images(shape, seed):
    """A blocky render-like image in about [-0.15, 1.15] and a correlated ground truth quantised to uint8."""
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(shape[0], shape[1] // 8 + 2, shape[2] // 8 + 2, generator=g)
    # few distinct values (small files): 8 x 8 blocks, the noise of both images in one pixel of four (the render's on a
    # 1/32 grid, the ground truth's on three levels)
    up = F.interpolate(base[None], size=shape[1:], mode="nearest")[0]
    noise = torch.round(0.04 * torch.randn(shape, generator=g) * 32.0) / 32.0 * (torch.rand(shape, generator=g) < 0.25)
    img = (torch.round((1.3 * up - 0.15) * 32.0) / 32.0 + noise).to(torch.float16)
    gt_noise = 0.05 * torch.randint(1, 4, shape, generator=g) * (torch.rand(shape, generator=g) < 0.25)
    gt = ((0.8 * up + gt_noise).clamp(0, 1) * 255.0).round().to(torch.uint8)
    return img, gt


def interior_ssim(x, y):
    """The reference's SSIM map (create_window + the convolutions of _ssim, zero padding 5), averaged over [5:-5, 5:-5]."""
    Cn = x.shape[0]
    w = ref_loss.create_window(11, Cn).type_as(x)
    conv = lambda t: F.conv2d(t[None], w, padding=5, groups=Cn)[0]
    mu1, mu2 = conv(x), conv(y)
    s1 = conv(x * x) - mu1.pow(2)
    s2 = conv(y * y) - mu2.pow(2)
    s12 = conv(x * y) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1.pow(2) + mu2.pow(2) + C1) * (s1 + s2 + C2))
    return float(m[:, 5:-5, 5:-5].mean())


if __name__ == "__main__":
    os.makedirs(os.path.join(HERE, "metrics"), exist_ok=True)
    for name, (shape, seed) in CASES.items():
        img16, gt8 = images(shape, seed)
        x = torch.clamp(img16.double(), 0.0, 1.0)
        y = gt8.double() / 255.0
        l1 = float(ref_loss.l1_loss(x, y).mean())
        ps = float(ref_image.psnr(x, y).mean())
        ss = float(ref_loss.ssim(x, y).mean())
        ms = metrics_oracle.msssim(img16, y)
        np.savez_compressed(os.path.join(HERE, "metrics", name + ".npz"), img=img16.numpy(), gt=gt8.numpy(), l1=np.float64(l1),
                            psnr=np.float64(ps), ssim=np.float64(ss), msssim=np.float64(ms), ssim_interior=np.float64(interior_ssim(x, y)))
        print(name, "l1 %.6f psnr %.4f ssim %.6f msssim %.6f" % (l1, ps, ss, ms))
