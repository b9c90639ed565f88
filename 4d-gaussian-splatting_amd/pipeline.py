"""One optimizer step = the B views of a batch on two HIP streams (MI355X: overlap instead of a longer queue).

Within one optimizer step the parameters are constant, so the forward of view b+1 does not depend on the backward
of view b (reference train.py:104-170 runs them strictly one after the other through autograd).  The forward front
end is a chain of short latency-bound kernels (preprocess, two radix sorts, scans: HBM / launch latency) while the
backward is dominated by the VALU-bound blend kernel: run on two streams they fill each other's gaps.

    stream F : fwd(0)         fwd(1)         fwd(2) ...
    stream B :        loss+bwd(0)    loss+bwd(1)    ...   all-reduce, Adam

No autograd: forward, fused L1+SSIM (value and gradient) and backward are called explicitly; parameter gradients
are written (view 0) / added (views 1..) straight into the flat bucket (``GaussianParams.grad_sink``), the loss is
pre-scaled by 1 / (B * world) so that the all-reduce SUM is already the mean.  Same arithmetic as
``render_raw`` + ``fused_l1_ssim`` + ``backward()`` per view (tests/test_gpu_api.py compares the two).
"""
import weakref
from functools import partial
from typing import Sequence

import torch

from . import _capi
from .fused import raw_backward, raw_forward, raw_preprocess_batch, raw_settings
from .gaussian_renderer import diff_gaussian_rasterization as _dgr
from .loss import l1_ssim_grad, l1_ssim_loss, l1_ssim_loss_batch
from .train_host import allreduce_and_step, allreduce_sh_begin, gather_view_stage_begin, timed_wait


_LAST_STEPPER = {}    # id(model) -> weak reference to the pipeline whose step() touched the model last (overlap_steps: see _model_token)


class StepPipeline:
    def __init__(self, model, optimizer, world_size: int = 1, lambda_dssim: float = 0.2, overlap: bool = True,
                 fuse_sh_adam: bool = True, gather_max_views: int = 32, split_colour: bool = False, batch_views: bool = False,
                 sh_group: int = 1, tile_cull: bool = True, lazy: bool = True, sparse_lists: bool = True, overlap_steps: bool = False,
                 lambda_rigid: float = 0.0, lambda_motion: float = 0.0, lambda_opa_mask: float = 0.0, rigid_k: int = 20,
                 env_optimizer=None, grad_terms=None, exposure=None):
        """``fuse_sh_adam``: on one rank the SH coefficients are updated straight from the views'
        staged SH gradients (FlatAdam.step_sh_staged) and ``_features.grad`` is NOT materialised for the step; False keeps
        the flush into the gradient bucket followed by the plain Adam step (always the case on several ranks, where the
        bucket is what the all-reduce sums).
        ``lambda_rigid`` / ``lambda_motion`` / ``lambda_opa_mask``: the reference trainer's other loss terms (train.py:119-159), added
        to every view's loss with these weights (0: the term is not computed at all, the step is exactly the plain one); step() then
        needs ``alpha_masks`` for the opacity mask, and the terms' values are in ``last_terms`` after each step.
        ``env_optimizer``: the ``fdgs.envmap.EnvMapAdam`` of ``model.env_map``, used by the steps whose ``pipe.env_map_res`` > 0 (None: one
        with the reference's defaults is made at the first such step).  Such a step rasterizes over black, composites the map behind
        every view on stream F right behind the view's forward (``results[b]["render"]`` is the composited image), takes the
        composite's backward on stream B between the loss gradient and the rasterizer backward (the alpha gradient; the map's gradient
        is written by view 0 and added by the others) and steps the map's Adam in the tail (``step(..., optimize_env=)``).
        ``grad_terms``: callables that add further loss terms' gradients into the gradient bucket (one rank only), each called once per
        step with the sink dict (``GaussianParams.grad_sink()``'s names) while stream B is current, where the rigid / motion terms add
        theirs: right after view 0's backward has written the bucket and before anything reads the geometry gradient
        (``fdgs.mcmc.MCMCStrategy.add_regularizer_grads`` is one).  None: the step's launch sequence is exactly the plain one.
        ``exposure``: a ``fdgs.exposure.ExposureModel`` (one rank only), a learned affine colour transform per training camera.  Every
        view's image goes through its camera's row on stream F behind the forward (and the environment-map composite) into a second
        buffer: ``results[b]["render"]`` is the corrected image the loss is taken on, ``results[b]["render_uncorrected"]`` the
        rasterizer's.  On stream B the transform's backward runs between the loss gradient and the composite's backward: it turns the
        colour gradient into that of the uncorrected image in place and WRITES the view's 12 sums into its slot of a [B, 12] buffer;
        the table's Adam (its own: ``step(..., optimize_exposure=)``) is one launch in the tail.  None: the step's launch sequence is
        exactly the plain one."""
        if int(world_size) > 1 and exposure is not None:
            raise NotImplementedError("StepPipeline: the exposure model runs on one rank only")
        self.exposure = exposure
        self._exp_idx = None    # this step's row of the exposure table per view, and whether the table's Adam runs
        self._optimize_exposure = False
        # recorded on stream B behind the table's Adam; the next step's first apply (stream F) waits for it (see _env_ev)
        self._exp_ev = None
        if int(world_size) > 1 and (lambda_rigid > 0 or lambda_motion > 0 or lambda_opa_mask > 0):
            raise NotImplementedError("StepPipeline: the rigid / motion / opacity-mask terms run on one rank only")
        self.grad_terms = tuple(grad_terms) if grad_terms else ()
        if int(world_size) > 1 and self.grad_terms:
            raise NotImplementedError("StepPipeline: grad_terms run on one rank only")
        self.lam_rigid, self.lam_motion, self.lam_opa = float(lambda_rigid), float(lambda_motion), float(lambda_opa_mask)
        self.rigid_k = int(rigid_k)
        self.regularize = self.lam_rigid > 0 or self.lam_motion > 0
        self.last_terms = {}
        self.env_opt = env_optimizer
        self._env = None        # this step's environment map (None: pipe.env_map_res == 0) and whether its Adam runs
        self._optimize_env = False
        # overlap_steps: recorded on stream B behind the map's Adam; the next step's first composite (stream F) waits for it
        self._env_ev = None
        self.model, self.opt, self.world, self.lam = model, optimizer, int(world_size), float(lambda_dssim)
        self.fuse_sh_adam = bool(fuse_sh_adam)
        # several ranks, up to this many views per step over all ranks: the ranks exchange the views' SH stages (32 B per
        # Gaussian and view, all-gather) instead of all-reducing the dense SH gradient (12 M B per Gaussian), and every rank
        # runs the fused update on all of them.  A view's stage is final when ITS SH backward has run, so its all-gather is
        # started right there (train_host.gather_view_stage_begin) and travels while the following views are rendered -- the
        # dense gradient is a sum over the step's views and can only leave at the end.  8 GPUs x 4 views: 4 x 67 MB received
        # per GPU, three of the four hidden, against a 2 x 7/8 x 171 MB ring all-reduce after the last view; beyond 32 views
        # the stages outweigh the dense gradient
        self.gather_max_views = int(gather_max_views)
        # fdgs_forward_out.tile_cull: the tile lists hold a Gaussian only where it can reach alpha >= 1/255 (same pixels and
        # gradients as with the reference's lists, a quarter fewer instances at C3)
        self.tile_cull = bool(tile_cull)
        # fdgs_forward_out.lazy (one rank): no forward of the step waits for its num_rendered -- the host enqueues all B views without
        # touching the device (the reference stops in the middle of every forward, rasterizer_impl.cu:302) and reads the views' reports
        # ONCE, before the last view's backward, i.e. before anything of the optimizer step is enqueued; a view whose run-ahead buffers
        # turned out too small (its image is invalid) sends the whole step through the waiting path again -- nothing irreversible has
        # happened by then: the gradient bucket and the SH stages are simply overwritten.  ``lazy_redone`` counts those steps.
        # Several ranks: off (the decision to start over would have to be collective).
        self.lazy = bool(lazy)
        self.lazy_redone = 0
        # fdgs_forward_out.sparse_lists (with lazy): every tile's list at a fixed offset of the binning buffer -- the count and scan launches
        # leave the forward's critical chain
        self.sparse_lists = bool(sparse_lists)
        # ``overlap_steps`` (one rank, two streams, fused SH update; opt-in because it is a promise of the caller's): the head of step
        # k + 1 under the tail of step k.  89 % of the parameters are SH coefficients and their update (HBM-bound, 1.08 GB at C3: ~216 us)
        # is the last thing of a step -- but geometry, binning and sort of the next step's first view read no SH coefficient.  The SH
        # update goes onto a third stream A; the first view of the next step is a split_colour forward whose colour launch goes onto A
        # as well (fdgs_forward_out.colour_stream: in order behind the update, no event), while its geometry + binning + sort run on
        # stream F as soon as the GEOMETRY parameters' Adam step (23 us, stream B) is through.  Same kernels on the same numbers: losses and
        # parameters follow the plain pipeline's to the float-atomics noise two runs of ONE pipeline differ by (tests/test_gpu_api.py).
        # The promise: between two step() calls the caller enqueues nothing on ITS stream that writes the model / optimizer state or
        # that the next forwards depend on, and is done with the previous step's result tensors -- or it calls barrier() first (stream F
        # does not wait for the caller's stream at the start of such a step).  A model whose flat tensor was replaced or modified
        # through torch (densification, reset_opacity: the version counter moves) is noticed and treated like barrier().
        self.overlap_steps = bool(overlap_steps) and bool(overlap) and int(world_size) == 1 and bool(fuse_sh_adam)
        # two streams: the small reductions of the loss VALUES on stream F behind its last forward, all views' in ONE launch
        # (fdgs_l1_ssim_loss_batch) -- stream B's chain is the step's critical path, and 4 x ~6 us of a one-workgroup kernel were part
        # of it.  One stream: each view's reduction behind its backward.
        self.finish_on_F = bool(overlap)
        self._carry = None    # what the model looked like when the last step left its SH update running on stream A
        self.steps_carried = 0
        # several ranks, measurement aid: with ``exchange_pairs`` a list, every wait of stream B for a collective at the end of the step
        # is bracketed by two timing events appended to it (train_host.timed_wait): the exchange time nothing overlapped
        self.exchange_pairs = None
        self.split_colour = bool(split_colour)   # fdgs_forward_out.split_colour for the views' forwards (A/B; off: see DESIGN)
        # View batching (opt-in, B > 1): the SH coefficients -- 12 M bytes per Gaussian, most of what preprocess and SH backward
        # read -- are the same for every view of the step.  ``batch_views``: the views' geometry still runs per view, but their SH
        # colours come from ONE pass over the coefficients before the first view's binning (fdgs_preprocess_batch).  ``sh_group``
        # (below): the SH backward of groups of views from ONE pass (fdgs_sh_backward_batch).
        # Measured at C3, 4 views per step: 120 us less kernel time per step, 3.66 -> 3.56 ms on one stream; with the two
        # streams it is a wash (3.04 -> 3.04-3.10 ms): the batched head and tail of the step have nothing to overlap with.  Off by
        # default.
        self.batch_views = bool(batch_views)
        # SH backward of ``sh_group`` consecutive views in one pass over the coefficients (fdgs_sh_backward_batch) on stream B, with
        # the forwards left per view: the batch kernel takes two views in 66 us against 2 x 50 us for the per-view kernel (its lanes
        # pair up on a Gaussian, one view each), four in 120-135 us.  1 (default): the per-view SH backward inside
        # fdgs_rasterize_backward -- in the two-stream step the grouping is a loss (pairs: 1330 -> 1308 images/s at C3, all four: 1278),
        # because a group's SH + geometry backward waits for the group's last blend backward.
        self.sh_group = int(sh_group)
        dev = model.flat.device
        self.dev = dev
        # (Tried and dropped, with measurements on MI355X: a high-priority F stream and a CU-masked B stream change
        # nothing or hurt; persistent blend kernels that leave wave slots free for the other stream lose more to
        # load imbalance / ~100 ns same-address atomics than the overlap returns.  See DESIGN.md.)
        self.sF = torch.cuda.Stream(dev)
        self.sB = torch.cuda.Stream(dev) if overlap else self.sF
        self.sA = torch.cuda.Stream(dev) if self.overlap_steps else None
        # the model's gradient bucket; rebuilt by step() when the model was re-laid out (densification binds a new flat_grad)
        self.sink, self._sink_of = model.grad_sink(), model.flat_grad
        self._up = {}
        # persistent buffers (_buffer): gacc [P, 16] / gacc_b [B, P, 16] always-zero blend-backward accumulators (no memset per view;
        # one per view for the batched SH backward), parts [B, 2, n] the views' partial loss sums, sh_stage [B, P, 8] the deferred SH
        # gradient (fdgs_backward_out.sh_stage), gathered [B, world, P, 8] the stages of all ranks (several ranks, gather mode)
        self._bufs = {}

    def _upstream(self, B):
        if B not in self._up:
            # filled on the stream that reads it (B): created on the caller's stream AFTER sB.wait_stream(main) had been recorded, the
            # fill raced with the first step's loss backward
            with torch.cuda.stream(self.sB):
                self._up[B] = torch.full((1,), 1.0 / (B * self.world), dtype=torch.float32, device=self.dev)
        return self._up[B]

    def _buffer(self, name, shape, fill=torch.empty):
        """The persistent float32 buffer ``name`` (see __init__): made anew on the stream that uses it (B) when its shape changes."""
        buf = self._bufs.get(name)
        if buf is None or buf.shape != shape:
            with torch.cuda.stream(self.sB):
                buf = self._bufs[name] = fill(shape, dtype=torch.float32, device=self.dev)
        return buf

    def barrier(self):
        """overlap_steps: the caller has touched the model, the optimizer state or anything else the next step reads on its stream --
        the next step() waits for that stream before its first launch (as every step does without overlap_steps)."""
        self._carry = None

    def _model_token(self):
        m = self.model
        last = _LAST_STEPPER.get(id(m))
        # (another pipeline that stepped the same model in between counts as the caller having touched it)
        return (id(m.flat), m.flat._version, m.P, m.flat.data_ptr(), last is not None and last() is self)

    def _batched(self, B):
        """The step takes the SH backward of its views in groups (``sh_group``, see __init__): _step_batched."""
        return self.sh_group > 1 and B > 1

    def step(self, cams: Sequence, gts: Sequence[torch.Tensor], pipe, bg: torch.Tensor, scaling_modifier: float = 1.0,
             alpha_masks: Sequence[torch.Tensor] = None, optimize_env: bool = True, camera_indices: Sequence[int] = None,
             optimize_exposure: bool = True):
        """Runs forward + loss + backward of every view, the gradient all-reduce and the optimizer step.
        Returns (list of per-view results dict(render, radii, depth, alpha_T, flow, viewspace_grad, num_rendered), list
        of losses); the tensors may be used on the caller's stream until the next call of step().  ``losses`` are the views'
        L1 + SSIM values; the other terms (lambda_* > 0) are in ``last_terms``: "rigid", "motion" (device scalars) and "opa_mask"
        (device [B]), unweighted.  ``alpha_masks``: each view's ``gt_alpha_mask`` [1, H, W] (needed with lambda_opa_mask > 0).
        ``optimize_env`` (``pipe.env_map_res`` > 0): whether the environment map's Adam runs this step (train.py:250: iteration <
        env_optimize_until); without it the map's gradient is not computed, the Gaussians still see the map through alpha.
        ``camera_indices`` (with an exposure model): each view's row of the exposure table (default: ``exposure.index_of(cam)``);
        ``optimize_exposure``: whether the table's Adam runs this step (the images are corrected either way)."""
        m, ctx = self.model, (pipe, bg, scaling_modifier)
        self._exposure_begin(cams, camera_indices, optimize_exposure)
        if self.lam_opa > 0 and (alpha_masks is None or len(alpha_masks) != len(cams)):
            raise ValueError("StepPipeline: lambda_opa_mask > 0 needs one alpha mask per view (step(..., alpha_masks=))")
        if self.regularize and not (m.rot_4d and m.gaussian_dim == 4):
            raise ValueError("StepPipeline: lambda_rigid / lambda_motion need a rot_4d model with gaussian_dim == 4")
        self._masks = alpha_masks if self.lam_opa > 0 else None
        self._env_begin(pipe, optimize_env)
        if m.flat_grad is not self._sink_of:
            self.sink, self._sink_of = m.grad_sink(), m.flat_grad
        if self._batched(len(cams)):
            return self._step_batched(cams, gts, ctx)
        if self.lazy and self.world == 1:
            out = self._step_views(cams, gts, ctx, True)
            if out is not None:
                return out
            self.lazy_redone += 1
        return self._step_views(cams, gts, ctx, False)

    def _env_begin(self, pipe, optimize_env):
        """The environment map of this step (pipe.env_map_res > 0), and its optimizer."""
        self._env = None
        if not getattr(pipe, "env_map_res", 0):
            return
        if self.world > 1:
            raise NotImplementedError("StepPipeline: the environment map runs on one rank only")
        from .envmap import EnvMapAdam, _check_env
        env = getattr(self.model, "env_map", None)
        _check_env(env)
        if self.env_opt is None:
            self.env_opt = EnvMapAdam(env)
        elif self.env_opt.env_map is not env:
            raise ValueError("StepPipeline: env_optimizer steps another tensor than model.env_map")
        self._env, self._optimize_env = env.detach(), bool(optimize_env)

    def _env_composite(self, cam, color, T):
        """Stream F is current, right behind the view's forward: the map behind the view's colours, in place.  The first composite
        after a step whose map Adam ran waits for it (overlap_steps: stream F need not have waited for stream B)."""
        from .envmap import composite_
        if self._env_ev is not None:
            self.sF.wait_event(self._env_ev)
            self._env_ev = None
        composite_(color, T, self._env, cam)

    def _env_backward(self, st, b, cam, T, g_color, g_alpha):
        """Stream B is current, between the view's loss gradient and its rasterizer backward: d / d alpha (written, or added to the
        opacity-mask term's) and, with optimize_env, the map's gradient (view 0 writes, the others add).  Returns the alpha gradient."""
        if self._env is None:
            return g_alpha
        from .envmap import composite_backward
        acc = g_alpha is not None
        if not acc:
            g_alpha = torch.empty((1, int(T.shape[-2]), int(T.shape[-1])), dtype=torch.float32, device=self.dev)
            st.keep_masks.append(g_alpha)
        composite_backward(T, g_color, self._env, cam, g_alpha, acc, self.env_opt.grad if self._optimize_env else None, b > 0)
        return g_alpha

    def _exposure_begin(self, cams, camera_indices, optimize_exposure):
        """The rows of the exposure table this step's views go through, checked on the host."""
        self._exp_idx = None
        if self.exposure is None:
            return
        ex = self.exposure
        idx = [ex.index_of(c) for c in cams] if camera_indices is None else [int(i) for i in camera_indices]
        if len(idx) != len(cams) or any(not 0 <= i < ex.num_cameras for i in idx):
            raise ValueError("StepPipeline: camera_indices must name one row of the exposure table's %d per view; got %s for %d views"
                             % (ex.num_cameras, idx, len(cams)))
        self._exp_idx, self._optimize_exposure = idx, bool(optimize_exposure)

    def _exposure_apply(self, b, color):
        """Stream F is current, behind the view's forward and its composite: the corrected image, in a buffer of its own (the backward
        reads the uncorrected one).  The first apply after a step whose table Adam ran waits for it (see _env_composite)."""
        from .exposure import apply_
        if self._exp_ev is not None:
            self.sF.wait_event(self._exp_ev)
            self._exp_ev = None
        return apply_(color, self.exposure.table, self._exp_idx[b], out=torch.empty_like(color))

    def _exposure_backward(self, st, b, color, g_color):
        """Stream B is current, right behind the view's loss gradient: ``g_color`` becomes the gradient of the uncorrected image
        ``color`` in place, the view's 12 sums are written (never added: a lazy step that is given up and redone overwrites them)
        into slot b."""
        if self._exp_idx is None:
            return
        from .exposure import backward_
        backward_(g_color, color, self.exposure.table, self._exp_idx[b], self._buffer("exp_slots", (st.B, 12))[b])

    def _begin(self, B):
        """Head of every step: the streams wait for the caller's (overlap_steps: see __init__), the step's state and buffers."""
        m = self.model
        main = torch.cuda.current_stream(self.dev)
        # overlap_steps: stream F has waited for stream B (the geometry parameters' Adam step included) at the end of the previous step;
        # the caller's stream has nothing new for the forwards (the promise) but waits for the SH update on stream A -- so F must not
        # wait for it.  B does: its first launch of the step is the first view's loss, behind that view's colours anyway
        carried = self.overlap_steps and self._carry is not None and self._carry == self._model_token()
        self._carry = None
        _LAST_STEPPER[id(m)] = weakref.ref(self)
        # A carried step is only in order when its FIRST forward is a split_colour forward whose colour launch goes onto stream A, behind
        # the previous step's SH update.  The view-batched colour pass (batch_views, B > 1) and the batched step (sh_group > 1) evaluate SH
        # colours on stream F: they must not start before that update is through (nondeterministic colours otherwise, with no error)
        if carried and ((self.batch_views and B > 1) or self._batched(B)):
            self.sF.wait_stream(self.sA)
            carried = False
        if carried:
            self.steps_carried += 1
        else:
            self.sF.wait_stream(main)
        if self.sB is not self.sF:
            self.sB.wait_stream(main)
        st = _Step(self, B, main)
        st.up = self._upstream(B)
        if st.defer_sh:
            st.stage = self._buffer("sh_stage", (B, m.P, 8))
        if st.gather:
            st.gathered = self._buffer("gathered", (B, self.world, m.P, 8))
        return st

    def _terms_begin(self, st):
        """Head of a step with the rigid / motion terms: the k-NN of the means (constant within the step) and the terms' forward on
        stream F, ahead of the first forward -- stream B waits for F after every forward, so the backward below finds them done."""
        if not self.regularize:
            return
        m = self.model
        P, k = m.P, self.rigid_k
        with torch.cuda.stream(self.sF):
            from .knn import knn
            st.reg_idx, st.reg_d2 = knn(m._xyz.detach()[None], m._xyz.detach()[None], k)
            st.reg_vel = torch.empty((P, 3), dtype=torch.float32, device=self.dev)
            st.reg_losses = torch.empty(2, dtype=torch.float32, device=self.dev)
            st.reg_scratch = _capi.scratch(_capi.lib.fdgs_rigid_motion_scratch_bytes(P, k), self.dev)
            st.reg_w = torch.tensor([self.lam_rigid, self.lam_motion], dtype=torch.float32, device=self.dev)
            _capi.call("fdgs_rigid_motion_forward", self.dev, P, k, m._scaling.data_ptr(), m._scaling_t.data_ptr(), m._rotation.data_ptr(),
                       m._rotation_r.data_ptr(), m._t.data_ptr(), st.reg_idx.data_ptr(), st.reg_d2.data_ptr(), st.reg_vel.data_ptr(),
                       st.reg_losses.data_ptr(), st.reg_scratch.data_ptr(), guard=False)   # (the stream block has made the device current)
        self.last_terms["rigid"], self.last_terms["motion"] = st.reg_losses[0], st.reg_losses[1]

    def _terms_backward(self, st):
        """Adds lambda_rigid dL_rigid + lambda_motion dL_motion into the bucket, on stream B right after view 0's backward (which
        WRITES the bucket) and before anything reads the geometry gradient (the last view's fused geometry Adam, the tail).  Once per
        step: the reference adds the terms to each of the B views' losses and divides by B (train.py:159-162)."""
        if not self.regularize or st.reg_done:
            return
        m, g = self.model, self.sink
        with torch.cuda.stream(self.sB):
            _capi.call("fdgs_rigid_motion_backward", self.dev, m.P, self.rigid_k, m._scaling.data_ptr(), m._scaling_t.data_ptr(),
                       m._rotation.data_ptr(), m._rotation_r.data_ptr(), m._t.data_ptr(), st.reg_idx.data_ptr(), st.reg_d2.data_ptr(),
                       st.reg_vel.data_ptr(), st.reg_w.data_ptr(), 1.0, g["dL_dscales"].data_ptr(), g["dL_dscales_t"].data_ptr(),
                       g["dL_drotations"].data_ptr(), g["dL_drotations_r"].data_ptr(), st.reg_scratch.data_ptr(), guard=False)
        st.reg_done = True

    def _grad_terms(self, st):
        """The caller's gradient terms (``grad_terms``), at the same point of the step as ``_terms_backward`` and like it once per step."""
        if not self.grad_terms or st.terms_done:
            return
        with torch.cuda.stream(self.sB):
            for term in self.grad_terms:
                term(self.sink)
        st.terms_done = True

    def _opa_grad(self, st, b, T):
        """The opacity-mask term of view b (stream B is current): its value into last_terms["opa_mask"][b] and
        d (lambda_opa_mask L_opa / B) / d alpha, the upstream alpha gradient of the view's backward (None without the term)."""
        if self._masks is None:
            return None
        H, W = int(T.shape[-2]), int(T.shape[-1])
        if b == 0:
            st.opa_vals = torch.empty(st.B, dtype=torch.float32, device=self.dev)
            st.opa_parts = torch.empty(max(1, _capi.lib.fdgs_opa_mask_num_partials(H, W)), dtype=torch.float32, device=self.dev)
            self.last_terms["opa_mask"] = st.opa_vals
        mask = self._masks[b].to(self.dev, torch.float32).contiguous()
        g_alpha = torch.empty((1, H, W), dtype=torch.float32, device=self.dev)
        _capi.call("fdgs_opa_mask_loss", self.dev, H, W, T.data_ptr(), 1, mask.data_ptr(), st.up.data_ptr(), self.lam_opa, g_alpha.data_ptr(), 0,
                   st.opa_parts.data_ptr(), st.opa_vals[b:].data_ptr(), guard=False)   # (stream B's block is open around the caller)
        st.keep_masks.append((mask, g_alpha))
        return g_alpha

    def _colour_pass(self, cams, ctx):
        """batch_views: the SH colours of all views in one pass over the coefficients (stream F), ahead of the first view's binning."""
        with torch.cuda.stream(self.sF):
            sets = [raw_settings(c, self.model, *ctx) for c in cams]
            return raw_preprocess_batch([s[0] for s in sets], *sets[0][1], tile_cull=self.tile_cull)

    def _forward(self, cam, ctx, view=0, **kw):
        """Forward of view ``view`` on stream F (raw_forward options ``kw``; with the environment map its composite behind, with an
        exposure model the corrected image behind that), which stream B then waits for: (settings, tensors, outputs, the image the
        loss is taken on)."""
        with torch.cuda.stream(self.sF):
            rs, tens = raw_settings(cam, self.model, *ctx)
            out = raw_forward(rs, *tens, tile_cull=self.tile_cull, **kw)
            if self._env is not None:
                self._env_composite(cam, out[1], out[4])
            shown = out[1] if self._exp_idx is None else self._exposure_apply(view, out[1])
            ev = torch.cuda.Event()
            ev.record(self.sF)
        self.sB.wait_event(ev)
        return rs, tens, out, shown

    def _step_views(self, cams, gts, ctx, lazy):
        """step(); ``lazy``: see __init__ -- returns None when a view did not fit its run-ahead buffers (nothing of the optimizer step
        has been enqueued then)."""
        st = self._begin(len(cams))
        B, m = st.B, self.model
        gacc = self._buffer("gacc", (m.P, 16), torch.zeros)
        self._terms_begin(st)
        handles = self._colour_pass(cams, ctx) if self.batch_views and B > 1 else [None] * B
        # the fused SH update behind the last view's SH backward: next to stream B's geometry backward on the idle F stream -- with
        # overlap_steps on stream A, which the next step's first view puts its colour launch on
        s_up = self.sA if self.sA is not None else self.sF
        results, losses, keep, pend_loss = [], [], [], []
        R_last = -1
        for b in range(B):
            last, plain = b == B - 1, handles[b] is None
            first_on_A = b == 0 and self.sA is not None and st.fuse and plain
            rs, tens, (R, color, flow, depth, T, radii, geom, binb, img, _covs, out_means3D), shown = self._forward(
                cams[b], ctx, b, preprocessed=handles[b], split_colour=(self.split_colour or first_on_A) and plain,
                colour_stream=self.sA if first_on_A else None, lazy=lazy and plain, sparse_lists=self.sparse_lists and lazy and plain)
            st.rs = rs
            with torch.cuda.stream(self.sB):
                if self.finish_on_F and b == 0:   # (see __init__; the views of a step share one image size)
                    parts = self._buffer("parts", (B, 2, _capi.lib.fdgs_l1_ssim_num_partials(*color.shape)))
                g_color, loss_handle = l1_ssim_grad(shown, gts[b], self.lam, st.up, parts=parts[b] if self.finish_on_F else None)
                self._exposure_backward(st, b, color, g_color)
                if self.finish_on_F and last:
                    ev_parts = torch.cuda.Event()
                    ev_parts.record(self.sB)   # every view's partial sums are there
                if lazy and last:
                    # the one look at the device per step: did every view's lists fit?  (the last forward's tile scan has usually run
                    # by now -- the host is about one view ahead of the device here, not inside every forward)
                    with torch.cuda.stream(self.sF):
                        _pend, failed, reported = _capi.forward_lazy_status(self.dev, wait=True)
                    if failed:
                        self._join(st)
                        return None
                    lazy_ix = [i for i, r_ in enumerate(results) if r_["num_rendered"] < 0] + ([b] if R < 0 else [])
                    for i, r_val in zip(lazy_ix, reported[-len(lazy_ix):] if lazy_ix else []):
                        if i < b:
                            results[i]["num_rendered"] = r_val
                        else:
                            R_last = r_val
                after_sh = partial(self._stages_final, st, [b], s_up) if st.final == "gather" or (last and st.final) else None
                geo_adam = None
                # (B = 1 with the rigid / motion terms or grad_terms: their gradient comes after the only view's backward, so the geometry
                # Adam is the tail's for that step)
                if last and st.final == "sh_update" and m.rot_4d and m.gaussian_dim == 4 and not ((self.regularize or self.grad_terms) and B == 1):
                    # the Adam step of the 17 geometry parameters per Gaussian INSIDE the last view's geometry backward (fdgs_backward_out.adam:
                    # the kernel has just completed their gradient) instead of by a launch of its own in the tail; bit-identical
                    def geo_adam():
                        # (called after after_sh: the step count is this step's, and it is known whether the fused SH update ran --
                        # the tail's fall-back, flush + one Adam over the whole bucket, must not meet parameters already stepped)
                        if not st.sh_stepped:
                            return None
                        st.geo_adam_done = True
                        return self.opt.geometry_adam()
                g_alpha = self._env_backward(st, b, cams[b], T, g_color, self._opa_grad(st, b, T))
                grads = raw_backward(rs, tens[0], out_means3D, radii, *tens[1:], geom, R, binb, img, g_color, None, g_alpha, None,
                                     self.sink, b > 0, grad_accum=gacc, after_sh=after_sh,
                                     sh_stage=st.stage[b] if st.defer_sh else None, per_view_outputs=False, geometry_adam=geo_adam)
                if b == 0:
                    self._terms_backward(st)
                    self._grad_terms(st)
                loss = None if self.finish_on_F else l1_ssim_loss(loss_handle)
                pend_loss.append(loss_handle)
            # buffers allocated on F are read on B: keep them alive until F has waited for B (end of the step)
            keep.append((geom, binb, img, out_means3D, g_color, T, shown))
            results.append({"render": shown, "radii": radii, "depth": depth, "alpha_T": T, "flow": flow,
                            "viewspace_grad": grads[0], "num_rendered": R_last if (lazy and last and R < 0) else R})
            if shown is not color:
                results[-1]["render_uncorrected"] = color
            losses.append(loss)
        if self.finish_on_F:
            with torch.cuda.stream(self.sF):
                self.sF.wait_event(ev_parts)
                losses = l1_ssim_loss_batch(parts, pend_loss)
        self._optimizer_tail(st)
        self._join(st)
        return results, losses

    def _step_batched(self, cams, gts, ctx):
        """step() with the SH backward of ``sh_group`` consecutive views done in one pass over the coefficients (see __init__):
        stream B runs loss + blend backward per view and, after every ``sh_group`` views, ONE SH backward pass for the group
        followed by the group's geometry backward.  (``batch_views``: stream F starts with the geometry of every view and ONE
        colour pass, then per view binning + blend.)  Same arithmetic per view as
        the unbatched step (forward bit-identical; tests/test_gpu_api.py)."""
        st = self._begin(len(cams))
        B, m = st.B, self.model
        G = min(self.sh_group, B)
        gacc = self._buffer("gacc_b", (B, m.P, 16), torch.zeros)
        self._terms_begin(st)
        handles = self._colour_pass(cams, ctx) if self.batch_views else [None] * B
        results, losses, keep, pend = [], [], [], []
        for b in range(B):
            rs, tens, (R, color, flow, depth, T, radii, geom, binb, img, _covs, out_means3D), shown = self._forward(
                cams[b], ctx, b, preprocessed=handles[b], split_colour=self.split_colour and handles[b] is None)
            st.rs = rs
            results.append({"render": shown, "radii": radii, "depth": depth, "alpha_T": T, "flow": flow, "num_rendered": R})
            if shown is not color:
                results[-1]["render_uncorrected"] = color
            with torch.cuda.stream(self.sB):
                g_color, loss_handle = l1_ssim_grad(shown, gts[b], self.lam, st.up)
                self._exposure_backward(st, b, color, g_color)
                g_alpha = self._env_backward(st, b, cams[b], T, g_color, self._opa_grad(st, b, T))
                pend.append(raw_backward(rs, tens[0], out_means3D, radii, *tens[1:], geom, R, binb, img, g_color, None, g_alpha, None,
                                         self.sink, b > 0, grad_accum=gacc[b], sh_stage=st.stage[b], begin_only=True, per_view_outputs=False))
                losses.append(l1_ssim_loss(loss_handle))
                if (b + 1) % G == 0 or b == B - 1:
                    first = b - (b % G)
                    _dgr._C.sh_backward_batch(pend[first:b + 1])
                    if b == B - 1:   # the stages of the step are complete
                        self._stages_final(st, range(B), self.sF)
                    for v in range(first, b + 1):
                        keep.append(_dgr._C.backward_finish(pend[v]))
                        results[v]["viewspace_grad"] = keep[-1][0]
                    self._terms_backward(st)   # (view 0's geometry backward has written the bucket by now)
                    self._grad_terms(st)
            keep.append((geom, binb, img, out_means3D, g_color, T, shown))
        self._optimizer_tail(st)
        self._join(st)
        return results, losses

    def _stages_final(self, st, views, s_up):
        """The SH stages of ``views`` are final (stream B is current, right behind their SH backward): start what waits for them --
        gather: each view's exchange, which travels while the following views are rendered; else (called once, with the step's last
        view among ``views``) the fused SH update on ``s_up``, next to stream B's geometry backward, or the flush of the stages into the
        bucket and the all-reduce of its SH part (several ranks: 88 % of the bucket, it travels while the geometry backward runs)."""
        if st.final == "gather":
            for v in views:
                st.gathers.append(gather_view_stage_begin(st.stage[v], st.gathered[v]))
        elif st.final == "sh_update":
            done = torch.cuda.Event()
            done.record(self.sB)
            with torch.cuda.stream(s_up):
                s_up.wait_event(done)
                self.opt.step_count += 1
                st.sh_stepped = self.opt.step_sh_staged(st.stage, st.rs, _dgr.analytic_sh_gradients())
            st.sh_on_A = s_up is self.sA
        elif st.final == "flush":
            if st.defer_sh:
                self._flush(st, st.stage)
            if self.world > 1:
                st.sh_handle = allreduce_sh_begin(self.model, self.world)

    def _flush(self, st, stages):
        rs = st.rs
        _capi.sh_flush(stages, self.sink["dL_dsh"], rs.sh_degree, rs.sh_degree_t, rs.gaussian_dim, rs.force_sh_3d, _dgr.analytic_sh_gradients())

    def _optimizer_tail(self, st):
        """Exchange (several ranks) + optimizer step on stream B, after the last view's backward."""
        m = self.model
        feat = m.offsets["_features"][0]
        with torch.cuda.stream(self.sB):
            if self._env is not None and self._optimize_env:   # (the map's gradient is complete: every view's composite backward is behind)
                self.env_opt.step()
                self._env_ev = torch.cuda.Event()
                self._env_ev.record(self.sB)
            if self._exp_idx is not None and self._optimize_exposure:   # (every view's slot is written: its exposure backward is behind)
                self.exposure.step(self._exp_idx, self._buffer("exp_slots", (st.B, 12)))
                self._exp_ev = torch.cuda.Event()
                self._exp_ev.record(self.sB)
            # the losses were scaled by 1 / (B * world): SUM = mean; Adam on chunk k overlaps the all-reduce of chunk k+1
            if not (st.fuse or st.gather):
                allreduce_and_step(m, self.opt, self.world, chunks=4, average=False, sh_handle=st.sh_handle, wait_pairs=self.exchange_pairs)
                return
            stages = st.stage
            if st.gather:
                import torch.distributed as dist
                geo = dist.all_reduce(m.flat_grad[:feat], op=dist.ReduceOp.SUM, async_op=True)   # 17 floats per Gaussian
                for work in st.gathers:
                    timed_wait(work, self.exchange_pairs)
                stages = st.gathered.view(-1, m.P, 8)   # [B x world] views: view-major, rank-minor, the same on every rank
            if st.sh_stepped is None:   # (not launched behind the last SH backward: one stream, or several ranks)
                self.opt.step_count += 1
                st.sh_stepped = self.opt.step_sh_staged(stages, st.rs, _dgr.analytic_sh_gradients())
            if not st.sh_stepped:   # layout the fused kernel does not take: the two passes (every rank builds the same summed dL_dsh)
                self._flush(st, stages)
            if st.gather:
                timed_wait(geo, self.exchange_pairs)
            if not st.geo_adam_done:     # (else: taken inside the last view's geometry backward)
                self.opt.step_range(0, feat if st.sh_stepped else m.flat.numel())

    def _join(self, st):
        """End of a step (or of a lazy attempt given up): the caller's stream waits for every stream, F for B -- and for A, unless the
        next step may start under this step's SH update there (overlap_steps).  The returned tensors live in the F / B streams' pools
        and are safe to read on `main` until the next step() makes both streams wait for it (no record_stream: it would defer every
        free by an event query and grow the pools)."""
        main = st.main
        main.wait_stream(self.sB)
        main.wait_stream(self.sF)
        self.sF.wait_stream(self.sB)
        if self.sA is not None:
            main.wait_stream(self.sA)
            if st.sh_on_A and st.sh_stepped:
                self._carry = self._model_token()
            else:
                self.sF.wait_stream(self.sA)


class _Step:
    """One step()'s decisions and what it collects on the way: made at the top of every step, so that nothing of it reaches the next."""

    def __init__(self, sp, B, main):
        self.B, self.main = B, main
        self.fuse = sp.fuse_sh_adam and sp.world == 1
        self.gather = sp.fuse_sh_adam and sp.world > 1 and sp.world * B <= sp.gather_max_views
        # deferred SH gradient: with B > 1 views per step every view stages the 8 numbers it contributes to dL_dsh and ONE flush per
        # step writes the 3 M floats per Gaussian (on one rank also for B = 1: the stage then feeds the fused SH flush + Adam kernel)
        self.defer_sh = B > 1 or self.fuse or self.gather
        # what StepPipeline._stages_final starts (one rank on one stream: nothing, the tail takes the SH update)
        if self.gather:
            self.final = "gather"
        elif self.fuse:
            self.final = "sh_update" if sp.sB is not sp.sF else None
        else:
            self.final = "flush" if self.defer_sh or sp.world > 1 else None
        self.up = self.stage = self.gathered = None   # loss scale, stages [B, P, 8], gathered stages [B, world, P, 8]
        self.rs = None              # the last view's raster settings so far (SH degrees and layout for the SH update / flush)
        self.sh_stepped = None      # fuse: did the fused SH update run (None: not launched yet; False: a layout the kernel refuses)
        self.sh_on_A = False        # ... on stream A (overlap_steps: the next step may start under it)
        self.geo_adam_done = False  # the geometry parameters' Adam step was taken inside the last view's backward
        self.sh_handle = None       # several ranks, dense: the all-reduce of the SH part of the bucket
        self.gathers = []           # gather: the work handles of the views' stage exchanges
        self.reg_done = False       # the rigid / motion gradient has been added to the bucket this step
        self.terms_done = False     # the caller's grad_terms have been added to the bucket this step
        self.keep_masks = []        # the views' alpha masks and alpha gradients, alive until the step's end
