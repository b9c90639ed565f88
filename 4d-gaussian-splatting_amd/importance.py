"""Which Gaussians a model actually uses: per-Gaussian contribution statistics, the per-pixel ID map, pruning by them.

Everything here reduces to one quantity, the blending weight ``w = alpha * T`` a Gaussian gets at a pixel, summarised per Gaussian
over pixels, views and timestamps by one pass over the buffers a forward leaves behind (csrc/contribution.hip,
``fdgs_contribution``): its sum, its maximum, the number of pixels it contributes to (``hits``) and the number of pixels it
dominates (``dominant``: it is the pixel's largest-``w`` contributor), plus the map of the dominant Gaussian per pixel.  The
decisions and the arithmetic are the forward blend's own, so what is counted is exactly what the rendered images are made of.

* ``ContributionStats``      -- the four per-Gaussian tensors, accumulated over any number of views; ``score()``, ``keep_mask()``.
* ``accumulate``             -- forward + statistics pass per camera (each camera carries its own timestamp).
* ``id_map``                 -- index of the dominant Gaussian under every pixel of one view (-1: none): picking, masking.
* ``prune_by_contribution``  -- cuts the flat-bucket model (and its Adam moments) down to the Gaussians the statistics select.

There is no CPU path for the statistics themselves; ``ContributionStats`` and the selection are plain tensor code and run anywhere.
"""
import ctypes as C
import math
from typing import Dict, Optional, Sequence

import torch

from . import _capi
from .train_host import relayout


class ContributionStats:
    """``weight_sum`` / ``weight_max`` (float32 [P]), ``hits`` / ``dominant`` (int32 [P]: the library's uint32 counters) and
    ``views``, the number of views accumulated.  ``scales``: the activated spatial scales [P,3] of the model the statistics were
    taken from (set by ``accumulate``; only ``score(volume_power != 0)`` reads them)."""

    def __init__(self, P: int, device):
        self.P = int(P)
        self.weight_sum = torch.zeros(self.P, dtype=torch.float32, device=device)
        self.weight_max = torch.zeros(self.P, dtype=torch.float32, device=device)
        self.hits = torch.zeros(self.P, dtype=torch.int32, device=device)
        self.dominant = torch.zeros(self.P, dtype=torch.int32, device=device)
        self.scales: Optional[torch.Tensor] = None
        self.views = 0

    def zero_(self) -> "ContributionStats":
        for t in (self.weight_sum, self.weight_max, self.hits, self.dominant):
            t.zero_()
        self.views = 0
        return self

    def score(self, kind: str = "sum", volume_power: float = 0.0) -> torch.Tensor:
        """float32 [P]: ``weight_sum`` ("sum"), ``weight_max`` ("max") or ``dominant`` ("dominant"), times
        (product of the activated spatial scales) ** ``volume_power`` when that is non-zero (a large Gaussian that contributes
        little is worth more than a small one: volume_power > 0; the opposite: < 0)."""
        if kind == "sum":
            s = self.weight_sum.clone()
        elif kind == "max":
            s = self.weight_max.clone()
        elif kind == "dominant":
            s = self.dominant.to(torch.float32)
        else:
            raise ValueError("ContributionStats.score: kind must be 'sum', 'max' or 'dominant', got %r" % (kind,))
        if volume_power != 0.0:
            if self.scales is None or int(self.scales.shape[0]) != self.P:
                raise ValueError("ContributionStats.score: volume_power needs .scales = the model's activated spatial scales [P,3]")
            s = s * self.scales.detach().to(s.device, torch.float32).prod(dim=1).pow(float(volume_power))
        return s

    def keep_mask(self, *, keep_fraction: Optional[float] = None, min_weight_max: Optional[float] = None, min_hits: Optional[int] = None,
                  min_dominant: Optional[int] = None) -> torch.Tensor:
        """bool [P]: the Gaussians that pass EVERY criterion given.  ``keep_fraction``: the top ceil(keep_fraction * P) by
        ``score("sum")`` -- everything that ties with the last one kept is kept too; ``min_*``: at least that value.  At least one
        Gaussian survives (the best by ``score("sum")``) whatever the criteria say."""
        keep = torch.ones(self.P, dtype=torch.bool, device=self.weight_sum.device)
        if self.P == 0:
            return keep
        s = self.score("sum")
        if keep_fraction is not None:
            if not (0.0 < float(keep_fraction) <= 1.0):
                raise ValueError("keep_fraction must be in (0, 1], got %r" % (keep_fraction,))
            k = min(self.P, max(1, int(math.ceil(float(keep_fraction) * self.P))))
            keep &= s >= torch.topk(s, k, largest=True, sorted=True).values[k - 1]
        if min_weight_max is not None:
            keep &= self.weight_max >= float(min_weight_max)
        if min_hits is not None:
            keep &= self.hits >= int(min_hits)
        if min_dominant is not None:
            keep &= self.dominant >= int(min_dominant)
        if not bool(keep.any()):
            keep[torch.argmax(s)] = True
        return keep

    def broadcast_(self, src: int = 0) -> "ContributionStats":
        """Replaces ``weight_sum`` by rank ``src``'s (torch.distributed, the default group).  ``weight_sum`` is a float atomic sum:
        its last bits depend on the order the adds arrive in, so replicas that each accumulated the same views hold sums that differ
        by rounding, and a cut at the k-th largest of them could keep different rows on different ranks.  ``weight_max``, ``hits``
        and ``dominant`` are reproducible and stay as they are."""
        import torch.distributed as dist
        dist.broadcast(self.weight_sum, src=src)
        return self

    def select_(self, index: torch.Tensor) -> "ContributionStats":
        """Keeps the rows ``index`` (int64, ascending for a prune): the statistics follow a model whose rows were gathered alike."""
        index = index.to(self.weight_sum.device)
        self.weight_sum, self.weight_max = self.weight_sum[index], self.weight_max[index]
        self.hits, self.dominant = self.hits[index], self.dominant[index]
        if self.scales is not None:
            self.scales = self.scales[index]
        self.P = int(self.weight_sum.shape[0])
        return self


_RAW_ATTRS = ("_xyz", "_opacity", "_scaling", "_rotation")


def _forward(model, camera, pipe, bg, tile_cull, scaling_modifier=1.0):
    """A waiting (non-lazy) forward of ``model`` seen from ``camera``; the native binding's 11-tuple."""
    from .fused import raw_forward, raw_settings
    if all(isinstance(getattr(model, a, None), torch.Tensor) for a in _RAW_ATTRS):
        rs, tensors = raw_settings(camera, model, pipe, bg, scaling_modifier)
        return raw_forward(rs, *tensors, tile_cull=tile_cull)
    # a model that only has the reference's post-activation getters
    from .gaussian_renderer.diff_gaussian_rasterization import _C, forward_args, time_inputs, view_settings
    if pipe.compute_cov3D_python or pipe.convert_SHs_python:
        raise ValueError("fdgs.importance covers the default pipeline only (in-kernel covariance and SH)")
    rs, _timestamp_tensor = view_settings(camera, model, pipe, bg, scaling_modifier)
    ts, scaling_t, rotation_r, prefilter_var = time_inputs(model, lambda name: getattr(model, "get_" + name))
    return _C.rasterize_gaussians(*forward_args(rs, model.get_xyz, model.get_features, model.get_opacity, ts, model.get_scaling, scaling_t,
                                                model.get_rotation, rotation_r, prefilter_var), tile_cull=tile_cull)


def contribution_pass(P: int, W: int, H: int, geom, binb, img, num_rendered: int, *, pix_weight=None, weight_sum=None, weight_max=None,
                      hits=None, dominant=None, dominant_id=None) -> None:
    """``fdgs_contribution`` on the three scratch buffers of a forward (the binding's ``geomBuffer, binningBuffer, imgBuffer`` and
    ``num_rendered``), enqueued on the current stream of the buffers' device.  The per-Gaussian tensors are accumulated into,
    ``dominant_id`` (int32 [H,W]) is overwritten; any may be None, not all."""
    dev = _capi._common_device((("geom", geom), ("binb", binb), ("img", img)))
    outs = {"weight_sum": (weight_sum, torch.float32, P), "weight_max": (weight_max, torch.float32, P), "hits": (hits, torch.int32, P),
            "dominant": (dominant, torch.int32, P), "dominant_id": (dominant_id, torch.int32, W * H)}
    for name, (t, dtype, n) in outs.items():
        if t is None:
            continue
        _capi.need_gpu(t, name)
        if t.dtype != dtype or t.numel() != n or not t.is_contiguous():
            raise RuntimeError("fdgs: %s must be a contiguous %s tensor with %d elements" % (name, dtype, n))
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError("fdgs: %s lives on %s, the forward's buffers on %s" % (name, t.device, dev))
    if dev is None:
        raise RuntimeError("fdgs: contribution_pass needs at least one output")
    pw = None
    if pix_weight is not None:
        pw = _capi._dev_f32(pix_weight, "pix_weight")
        if pw.numel() != W * H or pw.device != dev:
            raise RuntimeError("fdgs: pix_weight must have %d x %d elements on %s" % (H, W, dev))
    cin = _capi.FdgsContributionIn(int(P), int(W), int(H), _capi._ptr(geom), _capi._ptr(binb), _capi._ptr(img), int(num_rendered),
                                   _capi._ptr(pw))
    ptrs = [_capi._ptr(outs[k][0]) for k in ("weight_sum", "weight_max", "hits", "dominant", "dominant_id")]
    cout = _capi.FdgsContributionOut(*ptrs)
    if P == 0 and ptrs[4] is None:
        return   # an empty model: nothing to accumulate into and no map to fill
    _capi.call("fdgs_contribution", dev, C.byref(cin), C.byref(cout))


@torch.no_grad()
def accumulate(model, cameras: Sequence, pipe, bg: torch.Tensor, *, masks: Optional[Sequence[Optional[torch.Tensor]]] = None,
               stats: Optional[ContributionStats] = None, tile_cull: bool = True) -> ContributionStats:
    """Adds the views ``cameras`` (each with its own ``timestamp``) to ``stats`` (a fresh ``ContributionStats`` when None) and returns
    it: per camera one waiting forward and the statistics pass behind it on the same stream -- no host synchronisation beyond the
    forward's own.  ``masks``: per view an [H,W] weight map or None: ``weight_sum`` takes ``weight * w``, pixels with weight <= 0 are
    left out of every statistic.  ``tile_cull``: the forward lists a Gaussian only in the tiles it can reach (shorter lists, the same
    contributions)."""
    P = int(model.get_xyz.shape[0])
    dev = model.get_xyz.device
    if stats is None:
        stats = ContributionStats(P, dev)
    elif stats.P != P:
        raise ValueError("fdgs.importance.accumulate: stats are for %d Gaussians, the model has %d" % (stats.P, P))
    if masks is not None and len(masks) != len(cameras):
        raise ValueError("fdgs.importance.accumulate: need one mask (or None) per camera")
    for v, cam in enumerate(cameras):
        (R, _c, _f, _d, _T, _radii, geom, binb, img, _covs, _om) = _forward(model, cam, pipe, bg, tile_cull)
        contribution_pass(P, int(cam.image_width), int(cam.image_height), geom, binb, img, R, pix_weight=None if masks is None else masks[v],
                          weight_sum=stats.weight_sum, weight_max=stats.weight_max, hits=stats.hits, dominant=stats.dominant)
        stats.views += 1
    stats.scales = model.get_scaling.detach()
    return stats


@torch.no_grad()
def id_map(model, camera, pipe, bg: torch.Tensor) -> torch.Tensor:
    """int32 [H,W]: the index of the Gaussian with the largest blending weight under every pixel of ``camera``'s view (the earliest in
    depth order on a tie), -1 where nothing contributes."""
    P = int(model.get_xyz.shape[0])
    W, H = int(camera.image_width), int(camera.image_height)
    (R, _c, _f, _d, _T, _radii, geom, binb, img, _covs, _om) = _forward(model, camera, pipe, bg, True)
    ids = torch.empty((H, W), dtype=torch.int32, device=model.get_xyz.device)
    contribution_pass(P, W, H, geom, binb, img, R, dominant_id=ids)
    return ids


@torch.no_grad()
def prune_by_contribution(model, optimizer, stats: ContributionStats, *, keep_fraction: Optional[float] = None,
                          min_weight_max: Optional[float] = None, min_hits: Optional[int] = None, min_dominant: Optional[int] = None,
                          dens_stats=None) -> Dict[str, int]:
    """In place on ``model`` (fdgs.train_host.GaussianParams), ``optimizer`` (FlatAdam, or None for a finished model) and, when
    given, ``dens_stats`` (DensificationStats): only the Gaussians ``stats.keep_mask(...)`` selects survive, in their old order,
    with their Adam moments (``fdgs_densify_gather`` with kind 0), rebound exactly as ``densify_and_prune(prune_only=True)``
    rebinds.  ``stats`` itself is cut down alike, so it stays aligned with the model.  Returns {"P_old", "P_new"}."""
    if not model.flat.is_cuda:
        raise RuntimeError("fdgs: prune_by_contribution needs the model on the GPU; there is no CPU path")
    P = model.P
    if stats.P != P:
        raise ValueError("fdgs.importance.prune_by_contribution: stats are for %d Gaussians, the model has %d" % (stats.P, P))
    dev = model.flat.device
    keep = stats.keep_mask(keep_fraction=keep_fraction, min_weight_max=min_weight_max, min_hits=min_hits, min_dominant=min_dominant)
    sel = torch.nonzero(keep.to(dev)).flatten()
    P_new = int(sel.numel())
    if P_new == P:
        return {"P_old": P, "P_new": P}
    relayout(model, optimizer, sel, stats=(stats,) if dens_stats is None else (stats, dens_stats))
    return {"P_old": P, "P_new": P_new}
