"""Inputs, references and error bars for the photometric-loss tests (tests/test_loss_cases_host.py on the CPU,
tests/test_gpu_loss_edges.py and tests/test_gpu_loss.py on the GPU).

Input classes: functions ``(shape, seed) -> (img, gt)``, float32 CPU tensors [C, H, W], deterministic through a
``torch.Generator``.  References: ``fdgs.train_host.photometric_loss`` -- the reference's ``l1_loss`` + ``ssim`` with
``F.conv2d(padding=5, groups=C)`` -- under autograd, in float64 (``ref64``: what the kernels are compared with) and in float32
(``ref32``: the reference's own arithmetic at the kernels' precision; its distance from ``ref64`` says how ill-conditioned a case is).

The error bar of a case comes from the references alone, never from a kernel's output:

    bar_g = MARGIN * max(|g_ref32 - g_ref64|_inf on the case, |g_ref32 - g_ref64|_inf on the noise case of the same shape and lambda)
    bar_v = max(VALUE_FLOOR, the same with |loss_ref32 - loss_ref64|)

The second term of the max is a floor: it keeps cases testable whose true gradient is 0 and whose ref32 error is (near) 0.
MARGIN = 4: the two-kernel path filters u = x + y and u^2 <= 4 max(x^2, y^2), so the absolute rounding of its window sums can be up
to four times that of the reference's E[x^2]; the one-ulp reciprocal and another summation order are small beside that.
Every figure is a maximum over all C*H*W elements: no pixel and no case is excluded."""
import functools

import torch

MARGIN = 4.0
VALUE_FLOOR = 2e-6     # what tests/test_gpu_loss.py asserts for the loss value


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def noise(shape, seed):
    """Independent uniform [0, 1)."""
    g = _gen(seed)
    return torch.rand(shape, generator=g), torch.rand(shape, generator=g)


def smooth(shape, seed):
    """Smooth-ish images in [0, 1] plus noise, like a render against a photo (bilinear-upsampled coarse noise)."""
    g = _gen(seed)
    base = torch.rand(shape[0], shape[1] // 4 + 2, shape[2] // 4 + 2, generator=g)
    up = torch.nn.functional.interpolate(base[None], size=shape[1:], mode="bilinear", align_corners=False)[0]
    img = (up + 0.1 * torch.randn(shape, generator=g)).clamp(0, 1)
    gt = (up.flip(-1) * 0.5 + 0.5 * torch.rand(shape, generator=g)).clamp(0, 1)
    return img, gt


def _disc_scene(shape, g):
    """gt = 1 outside a centred disc (radius 0.35 of the shorter side), smooth texture plus grain inside; the disc as a bool mask."""
    C, H, W = shape
    ys = torch.arange(H, dtype=torch.float32)[:, None] - 0.5 * (H - 1)
    xs = torch.arange(W, dtype=torch.float32)[None, :] - 0.5 * (W - 1)
    disc = (ys * ys + xs * xs <= (0.35 * min(H, W)) ** 2)[None].expand(C, H, W)
    base = torch.rand(C, H // 4 + 2, W // 4 + 2, generator=g)
    tex = torch.nn.functional.interpolate(base[None], size=(H, W), mode="bilinear", align_corners=False)[0]
    tex = (0.1 + 0.8 * tex + 0.05 * torch.randn(shape, generator=g)).clamp(0, 1)
    return torch.where(disc, tex, torch.ones(shape)), disc


def white_bg(shape, seed):
    """A white-background scene near convergence: gt = 1 outside a textured disc; img = gt + 0.02 N(0, 1) inside the disc +
    0.002 N(0, 1) everywhere, clamped to [0, 1]."""
    g = _gen(seed)
    gt, disc = _disc_scene(shape, g)
    img = gt + 0.02 * torch.randn(shape, generator=g) * disc + 0.002 * torch.randn(shape, generator=g)
    return img.clamp(0, 1), gt


def white_bg_exact(shape, seed):
    """As white_bg with img == gt == 1 bit-exactly outside the disc (both noises inside it only)."""
    g = _gen(seed)
    gt, disc = _disc_scene(shape, g)
    img = gt + (0.02 * torch.randn(shape, generator=g) + 0.002 * torch.randn(shape, generator=g)) * disc
    return torch.where(disc, img.clamp(0, 1), torch.ones(shape)), gt


def const_pair(shape, seed):
    return torch.full(shape, 0.7), torch.full(shape, 0.701)


def identical(shape, seed):
    img = torch.rand(shape, generator=_gen(seed))
    return img, img.clone()


def black(shape, seed):
    return torch.zeros(shape), torch.zeros(shape)


def unclamped(shape, seed):
    """The raw render is not clamped: img in [-0.5, 3.5)."""
    g = _gen(seed)
    return 4.0 * torch.rand(shape, generator=g) - 0.5, torch.rand(shape, generator=g)


# The edge shapes of the 32 x 32-tile SSIM kernels (csrc/ssim.hip, csrc/metrics.hip), the smallest that exercise each mechanism.
# shape -> number of 32 x 32 tiles = fdgs_l1_ssim_num_partials = C * ceil(H / 32) * ceil(W / 32).  A launch has ceil(tiles / 8) * 8
# workgroups; workgroup w takes tile (w % 8) * chunk + w / 8 with chunk = ceil(tiles / 8), if that is a tile (tile_of, csrc/ssim_window.h).
EDGE_SHAPES = {
    # the 11-tap window larger than the image: overhanging both borders at once, sides below the radius 5, sides of 1
    (3, 1, 1): 3, (1, 1, 37): 2, (1, 37, 1): 2, (3, 4, 4): 3, (3, 5, 6): 3, (3, 10, 11): 3, (1, 11, 10): 1,
    # tile edges: exact tiles, ragged on either axis and on both
    (3, 32, 32): 3, (3, 33, 31): 6, (2, 65, 64): 12, (3, 31, 97): 12,
    # tile counts: 8 = one tile per XCD chunk; 9 = chunk 2, XCD 4 half idle and three XCDs idle, 7 invalid workgroups; 12 = chunk 2 with
    # 4 tiles per channel: chunks inside a channel and across two; 8 as 2 x 4; 20 = chunk 3, 4 invalid workgroups, a chunk across the
    # channel boundary at tile 10; 36 = chunk 5, 4 invalid workgroups, chunks across both channel boundaries
    (1, 32, 225): 8, (1, 32, 257): 9, (3, 33, 33): 12, (1, 33, 97): 8, (2, 64, 129): 20, (3, 95, 97): 36,
}


CLASSES = {f.__name__: f for f in (noise, smooth, white_bg, white_bg_exact, const_pair, identical, black, unclamped)}
SEED = 5


@functools.lru_cache(maxsize=None)
def inputs(name, shape, seed=SEED):
    img, gt = CLASSES[name](tuple(shape), seed)
    assert img.dtype == torch.float32 and gt.dtype == torch.float32 and tuple(img.shape) == tuple(gt.shape) == tuple(shape)
    return img, gt


def reference(img, gt, lam, dtype):
    """(loss, d loss / d img) of fdgs.train_host.photometric_loss evaluated in ``dtype``; loss a Python float, the gradient in ``dtype``."""
    from fdgs import train_host
    x = img.detach().to(dtype).clone().requires_grad_(True)
    loss = train_host.photometric_loss(x, gt.detach().to(dtype), lam)
    loss.backward()
    return float(loss.item()), x.grad.detach()


class Case:
    """One (class, shape, lambda): inputs, both references, the fp32 reference's own error and the bars.  Computed once, shared, read-only."""

    def __init__(self, name, shape, lam, seed=SEED):
        self.name, self.shape, self.lam = name, tuple(shape), float(lam)
        self.img, self.gt = inputs(name, self.shape, seed)
        self.loss64, self.grad64 = reference(self.img, self.gt, self.lam, torch.float64)
        self.loss32, g32 = reference(self.img, self.gt, self.lam, torch.float32)
        self.grad_max = float(self.grad64.abs().max())
        self.err_g = float((g32.double() - self.grad64).abs().max())
        self.err_v = abs(self.loss32 - self.loss64)
        floor = self if name == "noise" else case("noise", self.shape, self.lam, seed)
        self.bar_g = MARGIN * max(self.err_g, floor.err_g)
        self.bar_v = max(VALUE_FLOOR, MARGIN * max(self.err_v, floor.err_v))


@functools.lru_cache(maxsize=None)
def case(name, shape, lam, seed=SEED):
    return Case(name, tuple(shape), lam, seed)
