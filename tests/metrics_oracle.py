"""Float64 statement of the evaluation metrics of csrc/metrics.hip (fdgs.metrics), on the CPU.  It is the specification:

``img`` is the render, clamped to [0, 1] before every metric (train.py:318: ``torch.clamp(render, 0.0, 1.0)``); ``gt`` is not
clamped.  Images are [C, H, W], C >= 1.

* L1     mean |img - gt| over all elements (utils/loss_utils.py:18).
* PSNR   per channel mse_c = mean over H*W of (img - gt)^2, psnr_c = 20 log10(1 / sqrt(mse_c)) (utils/image_utils.py:17-19);
         the view's PSNR is the mean of the C values (training_report's ``.mean()``); mse_c = 0 gives +inf.
* SSIM   the training loss's SSIM (utils/loss_utils.py:34-66): 11x11 Gaussian window, sigma 1.5, ZERO padding, "same" size,
         C1 = 0.01^2, C2 = 0.03^2, the mean over all pixels and channels.
* MS-SSIM  torchmetrics 0.11.4 ``MultiScaleStructuralSimilarityIndexMeasure(data_range=1.0)``, every other argument at its
         default.  For scales s = 0..4: the per-pixel SSIM map S and the contrast-structure map CS = (2 s_xy + C2) / (s_x^2 +
         s_y^2 + C2) with the same window and constants, on the VALID (H - 10) x (W - 10) window positions only (torchmetrics
         reflect-pads by 5, convolves and crops 5 on each side: exactly the valid positions of the unpadded image, so the
         reflection never reaches the result); sim_s = relu(mean S), cs_s = relu(mean CS) over channels and valid pixels together
         (normalize="relu"); then both images are 2x2 average-pooled (sizes floor: an odd last row / column is dropped).
         MS-SSIM = prod_{s<4} cs_s^beta_s * sim_4^beta_4, beta = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333).  Images with
         H // 16 <= 10 or W // 16 <= 10 (a side below 176) are rejected with torchmetrics' ValueError.

torchmetrics is not a dependency of this project, so no fixture comes from it: this written definition, evaluated in float64, is
the oracle.  The reference's own call runs torchmetrics in float32 on the CPU; the two may differ in the last bits.
"""
import math

import torch
import torch.nn.functional as F

C1, C2 = 0.01 ** 2, 0.03 ** 2
BETAS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
WIN, SIGMA = 11, 1.5


def window(channels: int) -> torch.Tensor:
    """The normalised 11-tap Gaussian (sigma 1.5) as an [C, 1, 11, 11] depthwise kernel, with the reference's rounding
    (utils/loss_utils.py:23-32: taps, normalisation and outer product in float32 -- the window both the reference's SSIM and its
    float32 torchmetrics call convolve with), then widened to float64.  (A float64 window moves SSIM by ~1e-6.)"""
    g = torch.tensor([math.exp(-(x - WIN // 2) ** 2 / float(2 * SIGMA ** 2)) for x in range(WIN)], dtype=torch.float32)
    g = (g / g.sum()).unsqueeze(1)
    return g.mm(g.t()).to(torch.float64).expand(channels, 1, WIN, WIN).contiguous()


def ssim_maps(x: torch.Tensor, y: torch.Tensor, padding: int):
    """(S, CS) maps of [C, H, W] float64 images: zero ``padding`` = 5 gives the "same" maps, 0 the valid window positions."""
    Cn = x.shape[0]
    w = window(Cn)
    conv = lambda t: F.conv2d(t[None], w, padding=padding, groups=Cn)[0]
    mu1, mu2 = conv(x), conv(y)
    s11 = conv(x * x) - mu1 * mu1
    s22 = conv(y * y) - mu2 * mu2
    s12 = conv(x * y) - mu1 * mu2
    cs = (2 * s12 + C2) / (s11 + s22 + C2)
    s = (2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1) * cs
    return s, cs


def _f64(img, gt, clamp):
    x = torch.as_tensor(img).to(torch.float64)
    y = torch.as_tensor(gt).to(torch.float64)
    return (x.clamp(0.0, 1.0) if clamp else x), y


def l1(img, gt, clamp=True) -> float:
    x, y = _f64(img, gt, clamp)
    return float((x - y).abs().mean())


def psnr(img, gt, clamp=True) -> float:
    x, y = _f64(img, gt, clamp)
    mse = ((x - y) ** 2).reshape(x.shape[0], -1).mean(1)
    return float((20.0 * torch.log10(1.0 / torch.sqrt(mse))).mean())


def ssim(img, gt, clamp=True) -> float:
    x, y = _f64(img, gt, clamp)
    return float(ssim_maps(x, y, WIN // 2)[0].mean())


def check_msssim_size(H: int, W: int, betas=BETAS) -> None:
    """torchmetrics 0.11.4's size check (functional/image/ssim.py, _multiscale_ssim_update)."""
    div = max(1, len(betas) - 1) ** 2
    if H // div <= WIN - 1:
        raise ValueError("For a given number of `betas` parameters %d and kernel size %d, the image height must be larger than %d."
                         % (len(betas), WIN, (WIN - 1) * div))
    if W // div <= WIN - 1:
        raise ValueError("For a given number of `betas` parameters %d and kernel size %d, the image width must be larger than %d."
                         % (len(betas), WIN, (WIN - 1) * div))


def msssim_terms(img, gt, clamp=True, betas=BETAS):
    """[(sim_s, cs_s)] per scale, after the relu."""
    x, y = _f64(img, gt, clamp)
    check_msssim_size(x.shape[-2], x.shape[-1], betas)
    out = []
    for s in range(len(betas)):
        S, CS = ssim_maps(x, y, 0)
        out.append((max(float(S.mean()), 0.0), max(float(CS.mean()), 0.0)))
        if s + 1 < len(betas):
            x, y = F.avg_pool2d(x[None], 2)[0], F.avg_pool2d(y[None], 2)[0]
    return out


def msssim(img, gt, clamp=True, betas=BETAS) -> float:
    terms = msssim_terms(img, gt, clamp, betas)
    v = 1.0
    for s, (sim, cs) in enumerate(terms):
        v *= (sim if s == len(terms) - 1 else cs) ** betas[s]
    return v


def metrics(img, gt, clamp=True, with_msssim=True):
    """[l1, psnr, ssim, msssim] (msssim NaN without ``with_msssim``), floats."""
    return [l1(img, gt, clamp), psnr(img, gt, clamp), ssim(img, gt, clamp),
            msssim(img, gt, clamp) if with_msssim else float("nan")]
