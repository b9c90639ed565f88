"""Densification as Markov chain Monte Carlo (Kheradmand et al., "3D Gaussian Splatting as Markov Chain Monte Carlo", NeurIPS 2024)
on the flat-bucket model; csrc/mcmc.hip, include/fdgs_mcmc.h.

The alternative to ``fdgs.densify``: no gradient statistics, no opacity reset, a model size known in advance.

* ``relocate``    -- dead Gaussians (opacity <= ``min_opacity``) become copies of live ones drawn with probability proportional to
  opacity; a Gaussian that now exists N times gets the opacity and scales that leave the rendered result (nearly) unchanged.  In
  place: the bucket, the optimizer's buffers and ``P`` stay.
* ``grow``        -- 5 % more Gaussians per call, drawn the same way, up to a hard ``cap``; at the cap nothing is touched any more.
* ``noise_step``  -- after every optimizer step the means move by ``Sigma xi`` (xi ~ N(0, I)), scaled by the learning rate and gated
  to Gaussians of low opacity.
* ``regularize``  -- the L1 terms on opacity and scale that make Gaussians die so that they can be relocated.

The sampling is integer arithmetic on 24-bit weights and counter-based random numbers (Philox4x32-10): ``seed``, a stream id and a
call number determine every draw, on every run and every rank whose opacities agree.  ``MCMCStrategy`` keeps the call number.

There is no CPU path.
"""
from typing import Dict, Optional

import torch

from . import _capi, _mcmc_capi
from .train_host import relayout

STREAM_RELOCATE, STREAM_GROW, STREAM_NOISE = 0, 1, 2     # the Philox stream ids of the three users of random numbers
GROW_PERCENT = 5
_p = _capi._ptr


def _need(t, name):
    _capi.need_gpu(t, name)
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError("fdgs.mcmc: '%s' must be a contiguous float32 tensor" % name)
    return t


def _touched(model):
    """The kernels wrote the bucket through raw pointers: move its version counter, which ``StepPipeline(overlap_steps=True)`` reads
    to notice that the model changed between two steps (an in-place operation on an empty slice: no launch)."""
    model.flat[:0].zero_()


@torch.no_grad()
def weights(opacity_raw: torch.Tensor, min_opacity: float = 0.005):
    """(alive uint8 [P], wq int32 [P] holding the uint32 weights, prefix int64 [P] holding their inclusive uint64 sums)."""
    op = _need(opacity_raw.detach(), "opacity_raw")
    P, dev = int(op.numel()), op.device
    alive = torch.empty(P, dtype=torch.uint8, device=dev)
    wq = torch.empty(P, dtype=torch.int32, device=dev)
    prefix = torch.empty(P, dtype=torch.int64, device=dev)
    if P:
        scratch = _capi.scratch(_mcmc_capi.lib.fdgs_mcmc_weights_scratch_bytes(P), dev, floor=8)
        _mcmc_capi.call("fdgs_mcmc_weights", dev, P, _p(op), float(min_opacity), _p(alive), _p(wq), _p(prefix), _p(scratch), arg_error=ValueError)
    return alive, wq, prefix


@torch.no_grad()
def draw(prefix: torch.Tensor, n_draws: int, seed: int, stream_id: int, call: int, return_words: bool = False):
    """``n_draws`` sources from the prefix sums of ``weights``: (source int32 [n_draws], counts int32 [P][, words int32 [n_draws, 4]])."""
    _capi.need_gpu(prefix, "prefix")
    P, dev, n = int(prefix.numel()), prefix.device, int(n_draws)
    source = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.empty(P, dtype=torch.int32, device=dev)
    words = torch.empty((n, 4), dtype=torch.int32, device=dev) if return_words else None
    _mcmc_capi.call("fdgs_mcmc_draw", dev, P, n, _p(prefix), int(seed) & (2 ** 64 - 1), int(stream_id), int(call), _p(source), _p(counts), _p(words),
                    arg_error=ValueError)
    return (source, counts, words) if return_words else (source, counts)


def sample(opacity_raw: torch.Tensor, n_draws: int, seed: int = 0, stream_id: int = 0, call: int = 0, min_opacity: float = 0.005,
           return_words: bool = False) -> Dict[str, torch.Tensor]:
    """``weights`` + ``draw``: dict(alive, wq, prefix, source, counts[, words])."""
    alive, wq, prefix = weights(opacity_raw, min_opacity)
    out = draw(prefix, n_draws, seed, stream_id, call, return_words)
    return dict(zip(("alive", "wq", "prefix", "source", "counts", "words"), (alive, wq, prefix) + tuple(out)))


def _rows(model):
    rows = model.row_floats()
    return len(rows), _mcmc_capi.host_ints(rows)


def _update(model, optimizer, source, counts, copies):
    """The sources drawn at least once and their ``copies`` (rows, in the order of ``source``) get the opacity and scales of a
    Gaussian that exists N times; the sources' Adam moments start from zero (the copies' are the caller's).  Returns the sources."""
    dev = model.flat.device
    srcs = torch.nonzero(counts > 0).flatten().to(torch.int32)
    rows = torch.cat([srcs, copies]).contiguous()
    count_of = torch.cat([srcs, source]).contiguous()
    _mcmc_capi.call("fdgs_mcmc_update", dev, int(rows.numel()), int(model.gaussian_dim), _p(rows), _p(count_of), _p(counts), _p(model._opacity),
                    _p(model._scaling), _p(model._scaling_t))
    return srcs


def _zero_moments(model, optimizer, rows):
    if optimizer is None or rows.numel() == 0:
        return
    n, host_rows = _rows(model)
    _mcmc_capi.call("fdgs_mcmc_zero_rows", model.flat.device, n, host_rows, model.P, int(rows.numel()), _p(rows.contiguous()), _p(optimizer.exp_avg),
                    _p(optimizer.exp_avg_sq))


@torch.no_grad()
def relocate(model, optimizer, seed: int = 0, call: int = 0, min_opacity: float = 0.005, stream_id: int = STREAM_RELOCATE) -> Dict[str, int]:
    """In place on ``model`` (GaussianParams) and ``optimizer`` (FlatAdam or None); ``P`` does not change.  Dead row d_j (ascending)
    becomes a copy of every segment of source s_j, SH rows included; sources and copies then share the opacity and scales of N
    copies, and the Adam moments of both start from zero.  With no dead or no live Gaussian nothing is touched and nothing is drawn.
    Returns dict(P, dead, alive, relocated, sources, drew)."""
    _capi.need_gpu(model.flat, "model.flat")
    P, dev = model.P, model.flat.device
    out = {"P": P, "dead": 0, "alive": P, "relocated": 0, "sources": 0, "drew": False}
    if P == 0:
        return out
    alive, _wq, prefix = weights(model._opacity, min_opacity)
    dead = torch.nonzero(alive == 0).flatten().to(torch.int32)
    n_dead = int(dead.numel())
    out["dead"], out["alive"] = n_dead, P - n_dead
    if n_dead == 0 or n_dead == P or int(prefix[-1]) == 0:
        return out
    source, counts = draw(prefix, n_dead, seed, stream_id, call)
    n, host_rows = _rows(model)
    _mcmc_capi.call("fdgs_mcmc_copy_rows", dev, n, host_rows, P, n_dead, _p(dead), _p(source), _p(model.flat))
    srcs = _update(model, optimizer, source, counts, dead)
    _zero_moments(model, optimizer, torch.cat([srcs, dead]))
    _touched(model)
    out.update(relocated=n_dead, sources=int(srcs.numel()), drew=True)
    return out


def grown_size(P: int, cap: int) -> int:
    """min(cap, floor(1.05 P)), never below P."""
    return max(int(P), min(int(cap), (100 + GROW_PERCENT) * int(P) // 100))


@torch.no_grad()
def grow(model, optimizer, cap: int, seed: int = 0, call: int = 0, min_opacity: float = 0.005, stream_id: int = STREAM_GROW) -> Dict[str, int]:
    """``grown_size(P, cap) - P`` new Gaussians, appended behind the old rows through ``train_host.relayout`` (new buffers, the
    optimizer rebound; the old rows keep their Adam moments, the new ones start from zero), each a copy of a source drawn like
    ``relocate``'s; sources and copies get the same update, the sources' moments start from zero.  At the cap -- and with no live
    Gaussian -- nothing is touched: the bucket is not rebuilt.  Returns dict(P_old, P_new, added, sources, drew)."""
    _capi.need_gpu(model.flat, "model.flat")
    P, dev = model.P, model.flat.device
    n_new = grown_size(P, cap) - P
    out = {"P_old": P, "P_new": P, "added": 0, "sources": 0, "drew": False}
    if n_new <= 0 or P == 0:
        return out
    _alive, _wq, prefix = weights(model._opacity, min_opacity)
    if int(prefix[-1]) == 0:
        return out
    source, counts = draw(prefix, n_new, seed, stream_id, call)
    src = torch.cat([torch.arange(P, dtype=torch.int32, device=dev), source])
    kind = torch.cat([torch.zeros(P, dtype=torch.uint8, device=dev), torch.ones(n_new, dtype=torch.uint8, device=dev)])
    relayout(model, optimizer, src, kind)
    srcs = _update(model, optimizer, source, counts, torch.arange(P, P + n_new, dtype=torch.int32, device=dev))
    _zero_moments(model, optimizer, srcs)
    _touched(model)
    out.update(P_new=model.P, added=n_new, sources=int(srcs.numel()), drew=True)
    return out


@torch.no_grad()
def noise_step(model, lr_xyz: float, noise_lr: float = 5e5, seed: int = 0, call: int = 0, xi: Optional[torch.Tensor] = None,
               stream_id: int = STREAM_NOISE, return_xi: bool = False, return_words: bool = False):
    """``_xyz`` (and ``_t`` with gaussian_dim == 4) += Sigma xi g(o) noise_lr lr_xyz, one launch.  Sigma: each Gaussian's own
    covariance from its raw parameters (the covariance itself, not its square root), g(o) = 1 / (1 + exp(-100 ((1 - o) - 0.995))).
    ``xi`` [P, 3] or [P, 4]: the normals to use (as ``densify_and_prune`` takes ``samples``); without it they come from Philox through
    Box-Muller, a function of (seed, stream_id, call, Gaussian index).  Returns None, or dict(xi [P, 4], words int32 [P, 4]) of what
    was asked for (``words`` only without ``xi``)."""
    _capi.need_gpu(model.flat, "model.flat")
    P, dev = model.P, model.flat.device
    four = int(model.gaussian_dim) == 4
    if xi is not None:
        _capi.need_gpu(xi, "xi")
        if xi.dim() != 2 or xi.shape[0] != P or xi.shape[1] not in (3, 4):
            raise ValueError("fdgs.mcmc.noise_step: xi must be [%d, 3] or [%d, 4], got %s" % (P, P, tuple(xi.shape)))
        xi = xi.detach().to(torch.float32)
        xi = (torch.cat([xi, torch.zeros((P, 1), dtype=torch.float32, device=dev)], 1) if xi.shape[1] == 3 else xi).contiguous()
    xi_out = torch.empty((P, 4), dtype=torch.float32, device=dev) if return_xi else None
    words = torch.empty((P, 4), dtype=torch.int32, device=dev) if return_words and xi is None else None
    _mcmc_capi.call("fdgs_mcmc_noise", dev, P, int(model.gaussian_dim), int(bool(model.rot_4d)), _p(model._xyz), _p(model._t) if four else None,
                    _p(model._opacity), _p(model._scaling), _p(model._scaling_t) if four else None, _p(model._rotation),
                    _p(model._rotation_r) if model.rot_4d else None, float(noise_lr) * float(lr_xyz), _p(xi), int(seed) & (2 ** 64 - 1),
                    int(stream_id), int(call), _p(xi_out), _p(words), arg_error=ValueError)
    _touched(model)
    if return_xi or return_words:
        return {"xi": xi_out, "words": words}
    return None


@torch.no_grad()
def regularize(model, sink: Dict[str, torch.Tensor], lambda_opacity: float = 0.01, lambda_scale: float = 0.01, lambda_scale_t: float = 0.0,
               partials: Optional[torch.Tensor] = None, terms: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ADDS the gradients of lambda_opacity mean(o) + lambda_scale mean(exp(_scaling)) + lambda_scale_t mean(exp(_scaling_t)) into
    ``sink["dL_dopacity"]`` / ``["dL_dscales"]`` / ``["dL_dscales_t"]`` (GaussianParams.grad_sink()'s names; the last only with
    lambda_scale_t > 0) and returns the three terms' values, a float64 [3] device tensor.  ``model``: anything with raw ``_opacity``,
    ``_scaling`` (and ``_scaling_t``).  ``partials`` / ``terms``: buffers of an earlier call with the same P, to allocate nothing."""
    op, sc = _need(model._opacity.detach(), "_opacity"), _need(model._scaling.detach(), "_scaling")
    P, dev = int(op.shape[0]), op.device
    if terms is None:
        terms = torch.zeros(3, dtype=torch.float64, device=dev)
    if P == 0:
        return terms
    g_op, g_sc = _need(sink["dL_dopacity"], "dL_dopacity"), _need(sink["dL_dscales"], "dL_dscales")
    if g_op.numel() != P or g_sc.numel() != 3 * P:
        raise ValueError("fdgs.mcmc.regularize: the sink is not that of a model of %d Gaussians" % P)
    sct = g_sct = None
    if lambda_scale_t > 0:
        sct, g_sct = _need(model._scaling_t.detach(), "_scaling_t"), _need(sink["dL_dscales_t"], "dL_dscales_t")
        if sct.numel() != P or g_sct.numel() != P:
            raise ValueError("fdgs.mcmc.regularize: _scaling_t / dL_dscales_t are not [%d, 1]" % P)
    n = int(_mcmc_capi.lib.fdgs_mcmc_regularize_num_partials(P))
    if partials is None or partials.numel() < n:
        partials = torch.empty(n, dtype=torch.float64, device=dev)
    _mcmc_capi.call("fdgs_mcmc_regularize", dev, P, _p(op), _p(sc), _p(sct), float(lambda_opacity), float(lambda_scale), float(lambda_scale_t),
                    _p(g_op), _p(g_sc), _p(g_sct), _p(partials), _p(terms), arg_error=ValueError)
    return terms


class MCMCStrategy:
    """The three operations with their settings and the call counter, around one model and its optimizer:

        strategy = MCMCStrategy(model, optimizer, cap=200_000)
        pipeline = StepPipeline(model, optimizer, grad_terms=[strategy.add_regularizer_grads])
        for it in range(iterations):
            pipeline.step(...)
            strategy.after_step(lr_xyz)            # the noise on the means
            if it % 100 == 0: strategy.refine()    # relocate the dead, grow towards the cap

    ``after_step`` and ``refine`` write the model outside the step, on the caller's stream: with
    ``StepPipeline(overlap_steps=True)`` call ``pipeline.barrier()`` before the next step.  Single rank (replicas whose opacities agree
    bit for bit make the same draws, but nothing here exchanges anything)."""

    def __init__(self, model, optimizer, cap: int, seed: int = 0, min_opacity: float = 0.005, noise_lr: float = 5e5,
                 lambda_opacity: float = 0.01, lambda_scale: float = 0.01, lambda_scale_t: float = 0.0):
        if int(cap) < 1:
            raise ValueError("MCMCStrategy: cap must be at least 1, got %r" % (cap,))
        self.model, self.optimizer, self.cap, self.seed = model, optimizer, int(cap), int(seed)
        self.min_opacity, self.noise_lr = float(min_opacity), float(noise_lr)
        self.lambda_opacity, self.lambda_scale, self.lambda_scale_t = float(lambda_opacity), float(lambda_scale), float(lambda_scale_t)
        self.call = 0            # the number of the next kernel call that draws
        self.last_terms = None   # float64 [3] on the device: the regularisers' values of the last add_regularizer_grads
        self._partials = None

    def _next_call(self, drew: bool) -> None:
        if drew:
            self.call += 1

    def refine(self) -> Dict[str, int]:
        """relocate, then grow.  Returns both count dicts merged (``P_old`` / ``P_new``: before and after)."""
        m, opt = self.model, self.optimizer
        moved = relocate(m, opt, self.seed, self.call, self.min_opacity)
        self._next_call(moved["drew"])
        grown = grow(m, opt, self.cap, self.seed, self.call, self.min_opacity)
        self._next_call(grown["drew"])
        return {"P_old": grown["P_old"], "P_new": grown["P_new"], "dead": moved["dead"], "relocated": moved["relocated"], "added": grown["added"],
                "sources": moved["sources"] + grown["sources"]}

    def after_step(self, lr_xyz: Optional[float] = None, xi: Optional[torch.Tensor] = None) -> None:
        """The noise step, once after each optimizer step.  ``lr_xyz``: the current learning rate of the means (None: what the
        optimizer's ``_xyz`` segment holds)."""
        if lr_xyz is None:
            lr_xyz = next(s["lr"] for s in self.optimizer.named_segments() if s["name"] == "_xyz")
        noise_step(self.model, lr_xyz, self.noise_lr, self.seed, self.call, xi=xi)
        self._next_call(xi is None)

    def add_regularizer_grads(self, sink: Optional[Dict[str, torch.Tensor]] = None) -> torch.Tensor:
        """Adds the regularisers' gradients into ``sink`` (default: the model's gradient bucket) on the current stream; the signature
        of a ``StepPipeline(grad_terms=...)`` callable.  In a ``render()`` + ``loss.backward()`` + ``fdgs.optim.Adam`` loop: call it
        after ``backward()`` with dict(dL_dopacity=model._opacity.grad, dL_dscales=model._scaling.grad[, dL_dscales_t=...])."""
        if sink is None:
            sink = self.model.grad_sink()
        P = int(self.model._opacity.shape[0])
        n = int(_mcmc_capi.lib.fdgs_mcmc_regularize_num_partials(max(P, 1)))
        if self._partials is None or self._partials.numel() != n or self._partials.device != self.model._opacity.device:
            self._partials = torch.empty(n, dtype=torch.float64, device=self.model._opacity.device)
            self.last_terms = torch.zeros(3, dtype=torch.float64, device=self.model._opacity.device)
        return regularize(self.model, sink, self.lambda_opacity, self.lambda_scale, self.lambda_scale_t, self._partials, self.last_terms)

    def state_dict(self) -> Dict[str, int]:
        return {"seed": self.seed, "call": self.call}

    def load_state_dict(self, state: Dict[str, int]) -> None:
        self.seed, self.call = int(state["seed"]), int(state["call"])


__all__ = ["MCMCStrategy", "weights", "draw", "sample", "relocate", "grow", "grown_size", "noise_step", "regularize"]
