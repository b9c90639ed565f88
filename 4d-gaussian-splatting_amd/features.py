"""Per-Gaussian feature channels rendered with the weights of the image: segmentation labels, distilled 2D embeddings, diagnostics.

A user's own per-Gaussian data ``F`` [P,C] is blended with the weights ``w = alpha * T`` the rendered image is made of,
``out[c, y, x] = sum over the pixel's contributions of w * F[id, c]``, by one pass over the buffers a forward leaves behind
(csrc/features.hip, ``fdgs_feature_blend``); its adjoint ``dF[id, c] += sum over pixels of w * g[c, y, x]``
(``fdgs_feature_blend_backward``) makes ``F`` trainable.  The decisions and the arithmetic of the weights are the forward blend's
own.  GEOMETRY IS HELD CONSTANT: the weights are numbers here, no gradient reaches alpha, the positions or the covariances -- a
loss on a feature image trains the features and nothing else.  Nothing is composited behind the features.

* ``blend_pass`` / ``blend_backward_pass`` -- the two library calls on the three scratch buffers of a forward, on the current stream.
* ``render_features``                      -- one forward of a model + the feature image of it; autograd reaches the features only.
* ``fit_features``                         -- distils per-view target maps into a [P,C] feature tensor with Adam.

There is no CPU path.
"""
import ctypes as C
from typing import Callable, List, Optional, Sequence, Tuple

import torch

from . import _capi

MAX_CHANNELS = _capi.FDGS_FEATURE_MAX_CHANNELS


def as_feature_matrix(features: torch.Tensor, P: int) -> torch.Tensor:
    """``features`` as [P,C]: a [P] vector is one channel; ValueError for any other shape or a C outside [1, MAX_CHANNELS]."""
    if features.dim() == 1:
        features = features.unsqueeze(1)
    if features.dim() != 2 or int(features.shape[0]) != int(P):
        raise ValueError("fdgs.features: features must be [P] or [P,C] with P = %d, got %s" % (P, tuple(features.shape)))
    _check_channels(int(features.shape[1]))
    return features


def _check_channels(Cn: int) -> None:
    if not (1 <= Cn <= MAX_CHANNELS):
        raise ValueError("fdgs.features: %d channels, 1 .. %d are supported" % (Cn, MAX_CHANNELS))


def _check_f32(t: torch.Tensor, name: str, shape) -> None:
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError("fdgs.features: %s must be a contiguous float32 tensor of shape %s, got %s %s" % (name, tuple(shape), t.dtype, tuple(t.shape)))


def blend_pass(P: int, W: int, H: int, geom, binb, img, num_rendered: int, features: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``fdgs_feature_blend`` on the three scratch buffers of a forward (the binding's ``geomBuffer, binningBuffer, imgBuffer`` and
    ``num_rendered``), enqueued on the current stream of the buffers' device: ``features`` [P,C] (or [P]) float32 -> [C,H,W],
    overwritten (``out``: written into when given).  A pixel without a contributor is exactly 0; no background.  The weights are
    constants: this call is not recorded by autograd (``render_features`` is)."""
    named = [("geom", geom), ("binb", binb), ("img", img), ("features", features), ("out", out)]
    for name, t in named:   # the device check comes first: nothing here runs on the CPU (an empty model leaves scratch buffers out)
        if t is not None and (t.numel() > 0 or name in ("features", "out")):
            _capi.need_gpu(t, name)
    features = as_feature_matrix(features.detach(), P)
    Cn = int(features.shape[1])
    _check_f32(features, "features", (P, Cn))
    dev = _capi._common_device(named[:3] + [("out", out)]) or features.device
    if features.device != dev:
        raise RuntimeError("fdgs: 'features' lives on %s, the forward's buffers on %s" % (features.device, dev))
    if out is None:
        out = torch.empty((Cn, H, W), dtype=torch.float32, device=dev)
    else:
        _check_f32(out, "out", (Cn, H, W))
    cin = _capi.FdgsFeatureIn(int(P), int(W), int(H), Cn, _capi._ptr(geom), _capi._ptr(binb), _capi._ptr(img), int(num_rendered),
                              features.data_ptr() if P > 0 else out.data_ptr())   # (P == 0: no row is read; the library wants a pointer)
    _capi.call("fdgs_feature_blend", dev, C.byref(cin), out.data_ptr())
    return out


def blend_backward_pass(P: int, W: int, H: int, geom, binb, img, num_rendered: int, dL_dout: torch.Tensor, d_features: torch.Tensor) -> torch.Tensor:
    """``fdgs_feature_blend_backward``: the adjoint of ``blend_pass`` for the same forward, on the current stream.  ``dL_dout``
    [C,H,W] float32; ``d_features`` [P,C] float32 is ACCUMULATED into (zero-fill it once, further views add to it) and returned.
    Geometry is held constant: this is the whole gradient of a feature image, and it reaches the features only."""
    named = [("geom", geom), ("binb", binb), ("img", img), ("dL_dout", dL_dout), ("d_features", d_features)]
    for name, t in named:
        if t is not None and (t.numel() > 0 or name in ("dL_dout", "d_features")):
            _capi.need_gpu(t, name)
    if d_features.dim() != 2 or int(d_features.shape[0]) != int(P):
        raise ValueError("fdgs.features: d_features must be [P,C] with P = %d, got %s" % (P, tuple(d_features.shape)))
    Cn = int(d_features.shape[1])
    _check_channels(Cn)
    _check_f32(d_features, "d_features", (P, Cn))
    _check_f32(dL_dout, "dL_dout", (Cn, H, W))
    dev = _capi._common_device(named)
    if P == 0:
        return d_features   # an empty model: nothing to add to
    cin = _capi.FdgsFeatureIn(int(P), int(W), int(H), Cn, _capi._ptr(geom), _capi._ptr(binb), _capi._ptr(img), int(num_rendered), None)
    _capi.call("fdgs_feature_blend_backward", dev, C.byref(cin), dL_dout.data_ptr(), d_features.data_ptr())
    return d_features


class _FeatureBlend(torch.autograd.Function):
    """features [P,C] -> [C,H,W] behind a finished forward; saves the forward's three buffers for the adjoint."""

    @staticmethod
    def forward(ctx, features, geom, binb, img, P, W, H, num_rendered):
        ctx.dims = (int(P), int(W), int(H), int(num_rendered))
        ctx.save_for_backward(geom, binb, img)
        return blend_pass(P, W, H, geom, binb, img, num_rendered, features.contiguous())

    @staticmethod
    def backward(ctx, g):
        P, W, H, R = ctx.dims
        geom, binb, img = ctx.saved_tensors
        d = torch.zeros((P, int(g.shape[0])), dtype=torch.float32, device=g.device)
        blend_backward_pass(P, W, H, geom, binb, img, R, g.contiguous(), d)
        return d, None, None, None, None, None, None, None


def render_features(camera, model, pipe, features: torch.Tensor, *, bg_color: Optional[torch.Tensor] = None, scaling_modifier: float = 1.0,
                    tile_cull: bool = False) -> dict:
    """One waiting forward of ``model`` seen from ``camera`` (at the camera's timestamp) and the feature image of that forward.
    ``features``: [P,C] or [P] (one channel) float32 on the model's device.  Returns {"features": [C,H,W], "render": [3,H,W],
    "alpha": [1,H,W], "depth": [1,H,W], "radii": [P]}: the last four are that same forward's, detached.

    Autograd reaches ``features`` ONLY: the blending weights are constants (geometry is held constant), the model's parameters get
    no gradient from this call -- not through "features" and not through "render", "alpha" or "depth".  Nothing is composited behind
    the features (use ``"alpha"`` for that); ``bg_color`` (default: black) is the background of ``"render"``.  Both model styles work:
    raw parameters (``fdgs.train_host.GaussianParams``) and the reference's post-activation getters."""
    from .importance import _forward
    P = int(model.get_xyz.shape[0])
    dev = model.get_xyz.device
    _capi.need_gpu(features, "features")
    F = as_feature_matrix(features, P)
    if F.dtype != torch.float32:
        raise ValueError("fdgs.features: features must be float32, got %s" % (F.dtype,))
    W, H = int(camera.image_width), int(camera.image_height)
    if bg_color is None:
        bg_color = torch.zeros(3, dtype=torch.float32, device=dev)
    with torch.no_grad():
        (R, color, _flow, depth, T, radii, geom, binb, img, _covs, _om) = _forward(model, camera, pipe, bg_color, tile_cull, scaling_modifier)
    fmap = _FeatureBlend.apply(F, geom, binb, img, P, W, H, R)
    return {"features": fmap, "render": color.detach(), "alpha": (1 - T).detach(), "depth": depth.detach(), "radii": radii.detach()}


def _loss(kind: str, out: dict, target: torch.Tensor) -> torch.Tensor:
    f = out["features"]
    if kind == "l2":
        return ((f - target) ** 2).mean()
    if kind == "l1":
        return (f - target).abs().mean()
    # cosine: between features / alpha and the target where something was rendered
    a = out["alpha"]
    seen = (a > 0).expand_as(f)
    fn = torch.where(seen, f / a.clamp_min(1e-12), torch.zeros_like(f))
    cos = torch.nn.functional.cosine_similarity(fn, target, dim=0, eps=1e-8)
    m = (a[0] > 0).to(f.dtype)
    return ((1.0 - cos) * m).sum() / m.sum().clamp_min(1.0)


def fit_features(model, cameras: Sequence, targets: Sequence[torch.Tensor], pipe, *, iterations: int, lr: float = 0.05, loss: str = "l2",
                 features: Optional[torch.Tensor] = None, on_step: Optional[Callable[[int, float], None]] = None) -> Tuple[torch.Tensor, List[float]]:
    """Distils the per-view target maps ``targets`` (a sequence indexed like ``cameras``, each [C,H,W] on the model's device; every
    camera carries its own timestamp) into a per-Gaussian feature tensor [P,C]: ``iterations`` steps of ``torch.optim.Adam`` (``lr``),
    one view per step in turn, on ``loss`` = "l2" or "l1" between ``render_features(...)["features"]`` and the target, or "cosine"
    between ``features / alpha`` and the target on the pixels with alpha > 0.  ``features``: the start value (zeros when None; not
    modified).  ``on_step(iteration, loss)`` is called after every step.  The model is not touched: its geometry is held constant.
    Returns (features [P,C], detached; the loss of every step)."""
    if loss not in ("l2", "l1", "cosine"):
        raise ValueError("fdgs.features.fit_features: loss must be 'l2', 'l1' or 'cosine', got %r" % (loss,))
    if len(cameras) == 0 or len(cameras) != len(targets):
        raise ValueError("fdgs.features.fit_features: need one target per camera (%d cameras, %d targets)" % (len(cameras), len(targets)))
    P = int(model.get_xyz.shape[0])
    dev = model.get_xyz.device
    Cn = int(targets[0].shape[0])
    _check_channels(Cn)
    if features is None:
        start = torch.zeros((P, Cn), dtype=torch.float32, device=dev)
    else:
        start = as_feature_matrix(features.detach(), P).to(dev, torch.float32).clone()
        if int(start.shape[1]) != Cn:
            raise ValueError("fdgs.features.fit_features: the start value has %d channels, the targets %d" % (int(start.shape[1]), Cn))
    F = start.requires_grad_(True)
    opt = torch.optim.Adam([F], lr=lr)
    history: List[float] = []
    for it in range(int(iterations)):
        v = it % len(cameras)
        out = render_features(cameras[v], model, pipe, F)
        value = _loss(loss, out, targets[v])
        opt.zero_grad(set_to_none=True)
        value.backward()
        opt.step()
        history.append(float(value.detach()))
        if on_step is not None:
            on_step(it, history[-1])
    return F.detach(), history
