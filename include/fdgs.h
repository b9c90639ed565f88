/* fdgs.h -- C ABI of libfdgs.so, the MI355X-native differentiable 4D Gaussian rasterizer.
 *
 * This is the drop-in boundary for the reference's native extension
 * `diff_gaussian_rasterization._C` (diff-gaussian-rasterization/ext.cpp:15-19):
 *
 *   fdgs_rasterize_forward   replaces  rasterize_gaussians           (rasterize_points.h:18-49,
 *                                                                     RasterizeGaussiansCUDA rasterize_points.cu:36-149)
 *   fdgs_rasterize_backward  replaces  rasterize_gaussians_backward  (rasterize_points.h:51-89,
 *                                                                     RasterizeGaussiansBackwardCUDA rasterize_points.cu:151-270)
 *   fdgs_mark_visible        replaces  mark_visible                  (rasterize_points.h:91-94, rasterize_points.cu:272-291)
 *
 * Plain C: raw DEVICE pointers, sizes, scalars, an explicit HIP stream and int
 * error codes.  No torch / pybind types.  The host binding (ctypes in
 * 4d-gaussian-splatting_amd/_capi.py; any other FFI would look the same, see
 * INTEGRATION.md) owns every tensor, exactly like the reference where torch owns all
 * memory and the rasterizer only borrows pointers.
 *
 * Conventions carried over from the reference:
 *  - an absent optional tensor is a NULL pointer (the reference passes empty
 *    tensors, i.e. data_ptr()==nullptr, gaussian_renderer/diff_gaussian_rasterization.py:282-300);
 *    precedence: cov3D_precomp > rot_4d (4D conditional) > 3D (+1-D temporal marginal);
 *  - viewmatrix / projmatrix are the transposed ("row-vector") matrices of
 *    scene/cameras.py:65-70, read flat as column-major (auxiliary.h:59-78);
 *  - quaternions are (w,x,y,z) and already normalised; scales are post-exp;
 *    opacities post-sigmoid; shs is [P, M, 3];
 *  - the three scratch buffers (geometry / binning / image) are opaque byte
 *    buffers obtained through a resize callback (the reference's
 *    resizeFunctional, rasterize_points.cu:28-34) and must be handed back
 *    unchanged to fdgs_rasterize_backward;
 *  - gradients are bug-compatible with the reference backward (SURVEY.md
 *    Appendix A, Q1-Q13).
 *
 * Threading contract.  All work is enqueued on the caller's `stream`; fdgs_rasterize_forward waits for the device once
 * (for num_rendered, as the reference does at rasterizer_impl.cu:302; not at all with fdgs_forward_out.lazy): it spins on a pinned
 * mailbox the tile-scan kernel writes.  The library keeps, PER HOST THREAD AND DEVICE: the last-error string, that pinned mailbox
 * (a ring of 64 slots: at most 64 lazy forwards of a thread are unreported at a time; the 65th waits for the oldest), a second stream with
 * two events (fdgs_forward_out.split_colour) and the run-ahead guesses (sizes of the thread's previous forward calls per
 * (device, W, H, P)).  Consequence: any number of host threads may call concurrently (each with its own stream), and one
 * thread may drive several devices (hipSetDevice before the call); within ONE thread a forward call has returned before the
 * next one starts, so there is never more than one forward of a thread in flight on the host side.  Process-wide state:
 * the profiling accumulators (fdgs_profile_*, mutex-guarded), the test hooks fdgs_debug_tile_sort_limits /
 * fdgs_set_run_ahead, and the counters of fdgs_debug_run_ahead_stats.
 * Limits: P < 2^26 Gaussians per call (the blend kernels address the 48- / 64-byte per-Gaussian records with 32-bit byte
 * offsets; FDGS_ERR_HIP "invalid value" beyond), num_rendered < 2^31, image sides below 16 * 65535 pixels.
 */
#ifndef FDGS_H
#define FDGS_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FDGS_VERSION 502 /* 0.5.2 (round 6: fdgs_set_sparse_lists_budget; round 5: fdgs_forward_out.sparse_lists, .colour_stream).  Every struct below starts with `struct_size` = sizeof(the struct) as THIS header defines it
                            (the library answers FDGS_ERR_INVALID_ARG to any other value), and fdgs_version() must equal
                            FDGS_VERSION: a binding built against another revision of this header is turned away instead of
                            having the library read past the end of a shorter struct. */

/* error codes */
#define FDGS_OK 0
#define FDGS_ERR_INVALID_ARG 1   /* bad sizes / missing required pointers          */
#define FDGS_ERR_HIP 2           /* a HIP runtime call or kernel launch failed     */
#define FDGS_ERR_ALLOC 3         /* the scratch allocator callback returned NULL   */
#define FDGS_ERR_UNSUPPORTED 4   /* e.g. no gfx950 device                          */

/* which scratch buffer the allocator is asked for */
#define FDGS_BUF_GEOMETRY 0
#define FDGS_BUF_BINNING 1
#define FDGS_BUF_IMAGE 2

/* Resize callback: must return a DEVICE pointer to at least `bytes` bytes,
 * 256-byte aligned, valid until the matching backward has finished.
 * Mirrors std::function<char*(size_t)> in CudaRasterizer::Rasterizer::forward
 * (rasterizer.h:28-31).  Like the reference's resize lambdas it may be called more than once for the same buffer
 * within one forward call (FDGS_BUF_BINNING: the forward sizes it from the previous call before num_rendered is known and
 * asks again if that was too small); the latest answer is the buffer, an earlier one may be released in stream order
 * (work already enqueued on `stream` may still touch it). */
typedef void* (*fdgs_alloc_fn)(void* user, int which, size_t bytes);

/* Everything that describes one view; shared by forward and backward
 * (GaussianRasterizationSettings, gaussian_renderer/diff_gaussian_rasterization.py:227-245,
 * plus the per-call tensors). */
typedef struct fdgs_scene
{
	uint32_t struct_size; /* sizeof(fdgs_scene)                                    */
	int32_t P;            /* number of Gaussians                                   */
	int32_t D, D_t, M;    /* active SH degree, active time degree, SH coeffs/pt    */
	int32_t W, H;         /* image_width, image_height                             */
	const float* bg;              /* [3]                                           */
	const float* means3D;         /* [P,3]                                         */
	const float* shs;             /* [P,M,3] or NULL                               */
	const float* colors_precomp;  /* [P,3]  or NULL (exactly one of shs/colors)    */
	const float* flows;           /* [P,2]  or NULL (NULL == all zero)             */
	const float* opacities;       /* [P]                                           */
	const float* ts;              /* [P]    or NULL                                */
	const float* scales;          /* [P,3]  or NULL                                */
	const float* scales_t;        /* [P]    or NULL                                */
	const float* rotations;       /* [P,4]  or NULL                                */
	const float* rotations_r;     /* [P,4]  or NULL                                */
	const float* cov3D_precomp;   /* [P,6]  or NULL                                */
	const float* viewmatrix;      /* [16]                                          */
	const float* projmatrix;      /* [16]                                          */
	const float* campos;          /* [3]                                           */
	float scale_modifier;
	float prefilter_var;
	float tan_fovx, tan_fovy;
	float timestamp, time_duration;
	int32_t rot_4d, gaussian_dim, force_sh_3d;
	int32_t prefiltered;
	int32_t debug;        /* != 0: synchronise + check after every stage (CHECK_CUDA, auxiliary.h:165-172) */
	int32_t raw_params;   /* 0 (reference semantics): scales / scales_t / opacities / rotations / rotations_r are
	                         post-activation, as the reference passes them.
	                         1 (fused activations): they are the model's RAW parameters and
	                         the kernels apply the reference's activations themselves (scene/gaussian_model.py:179-219:
	                         exp, exp, sigmoid, x / max(|x|, 1e-12) twice); backward then returns gradients w.r.t. the
	                         raw parameters. */
	int32_t analytic_sh_grad; /* 0 (default): the 4D-SH backward reproduces the reference's three deviations from the analytic
	                         gradient (backward.cu:190, 303 / 384, 403): Q1 dL_dsh[1] uses the l = 0
	                         basis value, Q2 the derivative of cos(2 pi k dt / T) has the wrong sign, Q3 the k = 2 time term
	                         overwrites the k = 1 term in dRGB/dt.  1 (opt-in): the analytic gradient of the forward pass.
	                         Forward results do not depend on it.  (3D SH is analytic in the reference already.) */
} fdgs_scene;

/* Forward outputs; every array is fully written by the call (no pre-zeroing needed). */
typedef struct fdgs_forward_out
{
	uint32_t struct_size; /* sizeof(fdgs_forward_out)                              */
	float* out_color;     /* [3,H,W]                                               */
	float* out_flow;      /* [2,H,W]                                               */
	float* out_depth;     /* [1,H,W]                                               */
	float* out_T;         /* [1,H,W]  final transmittance (Python returns 1 - T)   */
	int32_t* radii;       /* [P]                                                   */
	float* out_means3D;   /* [P,3]    means3D, shifted by the conditional mean where rot_4d */
	float* covs_com;      /* [P,6] or NULL: owning copy of the computed 3D covariances
	                         (zero for culled Gaussians; the reference returns uninitialised memory there) */
	int32_t preprocessed; /* 0: the call runs the whole forward.  1: the per-Gaussian preprocess of this view was enqueued on the same
	                         stream by fdgs_preprocess_batch (which obtained the view's geometry and image buffers from the
	                         allocator): the call asks the allocator for the same two buffers again -- the allocator must answer
	                         with the SAME pointers -- and continues with the tile binning and the blend */
	int32_t split_colour; /* 0: one preprocess launch.  1: geometry first, the SH -> RGB evaluation (the bulk of the preprocess'
	                         memory traffic, which only the blend needs) on an internal second stream next to the tile binning
	                         (events in and out): shortens the forward's critical path by ~30 us at C3 for forward-only
	                         rendering; same arithmetic, bit-identical outputs */
	int32_t tile_cull;    /* 0: the tile lists are the reference's -- every tile of the square of 3 sigma_max around the projected
	                         mean (auxiliary.h:46-57), bit-identical point_list / ranges / n_contrib.  1: a Gaussian is only listed
	                         in the tiles of the axis-aligned bounding box of the region where it can reach alpha >= 1/255 (the
	                         forward blend's own per-pixel test, forward.cu:590), intersected with the reference's square; a
	                         Gaussian whose opacity is below 1/255 is listed nowhere.  Every (Gaussian, tile) instance left out
	                         fails that test on every pixel of the tile, so the pixels, radii and gradients are the reference's
	                         (to fp32 rounding: the blend kernels pair the list entries differently); num_rendered, the
	                         lists and n_contrib (a list position) are not: a quarter fewer instances at C3.  The backward takes
	                         whatever lists the forward left */
	int32_t lazy;         /* 0: the call returns num_rendered (it waits for the tile scan, as the reference does at
	                         rasterizer_impl.cu:302, and starts over from the scatter pass when its run-ahead guess was too small).
	                         1: when the call can run ahead (the thread has rendered this (device, W, H, P) before, no debug mode) it
	                         enqueues the whole forward with generous buffers -- 1.5 x the largest num_rendered / longest list of the
	                         thread's last four reports -- and returns WITHOUT waiting: *num_rendered = -1 ("not known yet"; the backward
	                         accepts -1: the tile ranges carry everything the kernels need) and the host never blocks on the device.  If
	                         the lists turn out not to fit, scatter and sort leave everything alone ON THE DEVICE and the forward's outputs
	                         are INVALID (background only): fdgs_forward_lazy_status reports it, and the caller renders that view again
	                         with lazy = 0 BEFORE anything irreversible depends on it (fdgs.pipeline.StepPipeline: before the optimizer
	                         step of the views' batch).  Where it cannot run ahead (first call for a configuration, debug mode,
	                         fdgs_set_run_ahead(0)) the call behaves as with 0 and returns num_rendered >= 0. */
	int32_t sparse_lists; /* with lazy = 1 only (ignored otherwise).  1: the tile lists are NOT packed back to back: tile t's list occupies the
	                         fixed slots [t * cap, t * cap + n_t) of the binning buffer, cap = the longest list the run-ahead guess provides for
	                         (rounded up to 64).  Nothing has to know the lists' starts before the scatter pass then: the count and scan
	                         launches disappear from the forward (4 launches in front of the blend instead of 6), the scatter counts as it goes.
	                         The lists themselves -- which instances, in which order -- are what they are without the flag; `ranges` holds
	                         (t * cap, t * cap + n_t) instead of the reference's prefix sums (identifyTileRanges), num_rendered (reported
	                         lazily) is the same sum.  A list that outgrows cap is cut and the forward reported as failed, like any lazy
	                         forward that does not fit.  Costs address space: T * cap entries of 12.5 bytes instead of num_rendered --
	                         within a BUDGET: when T * cap entries would take more than max(1 GiB, 4 x the compact buffer the same guess
	                         gets) the forward keeps compact lists (count + scan launches, prefix-sum `ranges`), so one hot tile of a real
	                         capture cannot turn a 200 MB buffer into gigabytes (fdgs_set_sparse_lists_budget). */
	void* colour_stream;  /* with split_colour = 1: NULL = the library's own second stream; otherwise the hipStream_t the SH -> RGB
	                         launch goes onto (after an event of the geometry launch; the caller's stream waits for its event before the
	                         blend).  Everything already enqueued on that stream comes first -- so a caller whose optimizer updates the
	                         SH coefficients on it gets: geometry, binning and sort of the next view (which read no SH coefficient) next
	                         to that update on the call's stream, the colours right behind it (fdgs.pipeline.StepPipeline, the first view
	                         of a step).  Same device as the call's stream */
} fdgs_forward_out;

/* fdgs_backward_out.adam: the scene's geometry tensors are slices of ONE flat parameter buffer `flat`; exp_avg / exp_avg_sq are
   torch.optim.Adam's moments in the same layout (a parameter at flat + k has its moments at exp_avg + k, exp_avg_sq + k).  Learning
   rates per tensor (arguments/__init__.py:84-92), `step` >= 1 = the step being taken (bias corrections as fdgs_adam_step). */
typedef struct fdgs_geometry_adam
{
	uint32_t struct_size;
	float* flat; float* exp_avg; float* exp_avg_sq;
	float lr_means3D, lr_opacities, lr_ts, lr_scales, lr_scales_t, lr_rotations, lr_rotations_r;
	float beta1, beta2, eps;
	int32_t step;
} fdgs_geometry_adam;

/* Upstream gradients (d loss / d forward outputs).  Any of the four image gradients may be NULL = "this output
   has no upstream gradient" (treated as zero; at least one must be given).  With only dL_dout_color given the
   backward blend runs its colour-only variant. */
typedef struct fdgs_backward_in
{
	uint32_t struct_size;        /* sizeof(fdgs_backward_in)                       */
	const float* dL_dout_color;  /* [3,H,W]                                        */
	const float* dL_dout_depth;  /* [1,H,W]                                        */
	const float* dL_dout_alpha;  /* [1,H,W]  gradient w.r.t. alpha = 1 - T         */
	const float* dL_dout_flow;   /* [2,H,W]                                        */
	const int32_t* radii;        /* [P]  as returned by forward                    */
	const float* out_means3D;    /* [P,3] as returned by forward                   */
	const void* geom_buffer;     /* the three scratch buffers of the forward call  */
	const void* binning_buffer;
	const void* image_buffer;
	int32_t num_rendered;        /* R returned by forward (-1 from a lazy forward: fine) */
} fdgs_backward_in;

/* Gradients; every non-NULL array is fully written by the call (no pre-zeroing
 * needed).  dL_dsh may be NULL when M == 0; the 4D-only ones may be NULL when
 * the corresponding input is absent. */
typedef struct fdgs_backward_out
{
	uint32_t struct_size;   /* sizeof(fdgs_backward_out)                           */
	float* dL_dmeans2D;     /* [P,3]  (x,y in NDC-scaled units, z = depth carrier, Q10) */
	float* dL_dcolors;      /* [P,3]   or NULL: not wanted (as dL_dcov3D, dL_dflows: per-view outputs of the reference's binding that no
	                           parameter gradient is read from -- a training step saves their 44 bytes per Gaussian and view) */
	float* dL_dopacity;     /* [P]                                                 */
	float* dL_dmeans3D;     /* [P,3]                                               */
	float* dL_dcov3D;       /* [P,6]   or NULL                                     */
	float* dL_dsh;          /* [P,M,3]                                             */
	float* dL_dflows;       /* [P,2]   or NULL                                     */
	float* dL_dts;          /* [P]                                                 */
	float* dL_dscales;      /* [P,3]                                               */
	float* dL_dscales_t;    /* [P]                                                 */
	float* dL_drotations;   /* [P,4]                                               */
	float* dL_drotations_r; /* [P,4]                                               */
	int32_t accumulate;     /* 0: the parameter gradients (dL_dmeans3D, dL_dsh, dL_dopacity, dL_dts, dL_dscales,
	                           dL_dscales_t, dL_drotations, dL_drotations_r) are overwritten; 1: the kernels ADD into
	                           them (gradient accumulation over the views of one optimizer step, reference
	                           train.py:104-166).  The per-view outputs (dL_dmeans2D, dL_dcolors, dL_dflows,
	                           dL_dcov3D) are always overwritten. */
	float* grad_accum;      /* [P,16] scratch: packed per-Gaussian accumulators of the blend backward
	                           (colour 3, depth 1, flow 2, mean2D 2, conic xx/yy/xy 3 (Q12 convention), opacity 1,
	                           SH-backward mean / time 4) */
	int32_t grad_accum_clean; /* 0: the call clears grad_accum itself (one memset per backward).
	                             1: the caller guarantees it is all zero on entry (a persistent buffer, zeroed once) and
	                                the call leaves it all zero on exit: the last kernel re-zeroes what it has read */
	float* sh_stage;          /* NULL: dL_dsh is written / accumulated by this call.  Otherwise [P,8] floats of scratch owned by the
	                             caller: DEFERRED SH gradient -- the call leaves dL_dsh alone and stores, per Gaussian, the 8
	                             numbers this view contributes through (its dL_dRGB, the view direction, the cosine factors of
	                             the two time blocks);
	                             fdgs_sh_flush turns the stages of all views of an optimizer step into dL_dsh in one pass. */
	int32_t stage_mask;       /* 0 (or 3): the whole backward.  1: blend backward + SH backward only -- dL_dsh is final when
	                             they have run; 2: the geometry backward only (must follow a call with 1 on the same
	                             stream, same arguments).  Lets a data-parallel caller start the all-reduce of the SH
	                             gradients (88 % of the bytes at M = 48) while the geometry backward still runs.
	                             + 4 (5 = blend backward only): the SH backward of this view is left to fdgs_sh_backward_batch, which
	                             does it for all views of the optimizer step in one pass over the coefficients; the view's
	                             geometry backward (2) follows after that call.  Needs sh_stage and a grad_accum of the view's own. */
	const struct fdgs_geometry_adam* adam; /* NULL, or (raw_params scenes with all seven geometry tensors, i.e. rot_4d; the LAST view of an optimizer step): the geometry backward also TAKES the
	                             Adam step of the 17 geometry parameters of every Gaussian -- means3D, opacities, ts, scales, scales_t, rotations,
	                             rotations_r as the scene points at them -- with the gradient it has just completed (this view's, added to what
	                             the gradient arrays hold when accumulate = 1; the arrays still receive the sum).  Bit-identical to
	                             fdgs_adam_step over those tensors afterwards; saves that launch and its 28 bytes per parameter. */
} fdgs_backward_out;

/* Forward pass: preprocess -> tile count -> tile scan -> tile scatter -> per-tile local sort (+ ranges) -> per-tile
 * blend: 6 kernel launches, all enqueued before the host waits for num_rendered (the scan kernel writes it into a pinned
 * mailbox; scatter / sort check on the device that the binning buffer, sized from the calling thread's previous forward, is
 * large enough, and the call starts over from the scatter pass if not).  *num_rendered receives R when the call returns.
 * `stream` is a hipStream_t passed as void* so that this header needs no HIP include. */
int fdgs_rasterize_forward(const fdgs_scene* scene, const fdgs_forward_out* out,
                           fdgs_alloc_fn alloc, void* alloc_user, void* stream,
                           int32_t* num_rendered);

/* The lazy forwards (fdgs_forward_out.lazy) of the CALLING THREAD on the current device, since the previous call of this function:
 * *pending = how many have not reported yet (always 0 with wait != 0: the call then blocks until the tile scan of the most recent one
 * has run -- every pending forward is waited for on the stream IT was enqueued on, whatever stream this call is made from: once that
 * stream has drained or failed the report is in or the call fails; `stream` is accepted for compatibility and not used); *failed = how many turned out not to fit
 * their buffers: the outputs of those forwards are invalid and must be rendered again with lazy = 0; num_rendered[0 .. *n_out) = the
 * num_rendered of the reported ones, oldest first (at most max_out, at most 64).  Every pointer may be NULL. */
int fdgs_forward_lazy_status(int32_t wait, void* stream, int32_t* pending, int32_t* failed,
                             int32_t* num_rendered, int32_t max_out, int32_t* n_out);

/* 1 (default): the forward enqueues scatter / sort / blend before num_rendered is back, with a binning buffer sized from the
 * calling thread's previous call; 0: it always waits and asks the allocator for exactly fdgs_binning_bytes(num_rendered)
 * (+ the long-list scratch), as the reference does.  Process-wide. */
void fdgs_set_run_ahead(int32_t enable);

/* Budget of fdgs_forward_out.sparse_lists: a forward takes the sparse layout only while its binning buffer stays within
 * max(min_bytes, factor x the bytes of the compact buffer sized from the same run-ahead guess).  Defaults: 1 GiB (environment:
 * FDGS_SPARSE_BUDGET_MB), 4.  min_bytes = 0, factor = 1: never more than the compact buffer, i.e. practically always compact.
 * Process-wide.  Returns FDGS_ERR_INVALID_ARG for min_bytes < 0 or factor < 1. */
int fdgs_set_sparse_lists_budget(int64_t min_bytes, int32_t factor);
/* Introspection: counts3[0] forwards that ran with sparse lists, [1] forwards that asked for them and kept compact lists because of the
 * budget, [2] bytes of the binning buffer the last run-ahead forward asked its allocator for. */
void fdgs_debug_sparse_lists_stats(int64_t* counts3);

/* View-batched preprocess (the views of ONE optimizer step: same Gaussian tensors, same P / M / degrees / flags; cameras and
 * timestamps differ).  The 12 M bytes of SH coefficients per Gaussian are most of what the preprocess reads, and they are
 * the same for every view: the geometry part runs per view, the SH colours of all views in ONE pass over the coefficients
 * (colours and clamp bits bit-identical to the per-view forward: test_preprocess_batch_forward_is_bit_identical,
 * test_colour_batch_edge_shapes_bitwise).  For each view v the call obtains the geometry and the image buffer through
 * alloc(alloc_users[v], ...) and fills outs[v]->radii / out_means3D / covs_com; the views' forwards are then completed one by
 * one with fdgs_rasterize_forward(scenes[v], outs[v] with preprocessed = 1, alloc, alloc_users[v], the same stream, ...).
 * The reference has no counterpart (train.py:104-166 renders the views of a batch strictly one after the other). */
int fdgs_preprocess_batch(int32_t num_views, const fdgs_scene* const* scenes, const fdgs_forward_out* const* outs,
                          fdgs_alloc_fn alloc, void* const* alloc_users, void* stream);

/* View-batched SH backward (deferred mode), the counterpart of fdgs_preprocess_batch: after the blend backward of every
 * view (fdgs_rasterize_backward with stage_mask = 5, a grad_accum and an sh_stage of the view's own), ONE pass over the SH
 * coefficients produces every view's stage record and its mean / time gradient (words 12..15 of the view's accumulator
 * records); the views' geometry backward (stage_mask = 2) and fdgs_sh_flush / fdgs_adam_step_sh follow.  Given the same accumulator records,
 * bit-identical to the per-view SH backward (test_sh_backward_paths_bitwise).  ins[v] / outs[v]: the structs of the views' backward calls. */
int fdgs_sh_backward_batch(int32_t num_views, const fdgs_scene* const* scenes, const fdgs_backward_in* const* ins,
                           const fdgs_backward_out* const* outs, void* stream);

/* Introspection for tests: how the forward calls of this process went -- counts3[0] scatter / sort / blend enqueued before
 * num_rendered was back and kept, [1] enqueued ahead but sorted again (longer tile lists than the previous call suggested),
 * [2] sized exactly after the wait (first call of a thread, debug mode, more instances than the previous call suggested). */
void fdgs_debug_run_ahead_stats(int64_t* counts3);

/* Backward pass: blend backward -> fused cov2D / projection / SH / covariance backward. */
int fdgs_rasterize_backward(const fdgs_scene* scene, const fdgs_backward_in* in,
                            const fdgs_backward_out* out, void* stream);

/* Deferred SH gradient, second half (see fdgs_backward_out.sh_stage): dL_dsh [P,M,3] = sum over the num_views staged views,
 * in view order, of basis(direction, time) (x) dL_dRGB -- the same additions in the same order as backward calls that
 * accumulate into dL_dsh view after view, with 1/3 of their memory traffic at 4 views.  stages: [num_views,P,8] floats, the
 * sh_stage buffers of the views back to back.  accumulate != 0 adds to dL_dsh instead of overwriting it.
 * D, D_t, M, gaussian_dim, force_sh_3d, analytic_sh_grad as in the fdgs_scene of the staged views (one value for all of them). */
int fdgs_sh_flush(int32_t P, int32_t D, int32_t D_t, int32_t M, int32_t gaussian_dim, int32_t force_sh_3d, int32_t analytic_sh_grad,
                  int32_t num_views, const float* stages, float* dL_dsh, int32_t accumulate, void* stream);

/* present[i] = view-space z of means3D[i] > 0.2 (checkFrustum, rasterizer_impl.cu:54-67). */
int fdgs_mark_visible(int32_t P, const float* means3D, const float* viewmatrix,
                      const float* projmatrix, uint8_t* present, void* stream);

/* Sizes of the opaque scratch buffers.  Geometry and image: exactly what the allocator is asked for.  Binning: the allocator
 * is asked for fdgs_binning_bytes(n) with n = num_rendered when the forward sizes the buffer after the wait (first call of a
 * thread for a (device, W, H, P), debug mode, fdgs_set_run_ahead(0)), and with n = 1.25 R' + 4096 <= 2^31 - 1 when it runs
 * ahead (R' = num_rendered of the thread's previous call for the same (device, W, H, P)); a second request in the same call
 * follows if that was too small.  Either request grows by 8 bytes per instance (of n) in the rare case that a single tile's
 * list is longer than the LDS sort takes (16384 entries).  (fdgs_binning_bytes(n) = 12 bytes per instance + 32 bytes per 64
 * instances and per tile: the blend forward's per-block cull decisions, kept for the blend backward.)  A caller that pre-sizes a binning arena either uses that bound
 * or switches the run-ahead off. */
size_t fdgs_geometry_bytes(int32_t P);
size_t fdgs_image_bytes(int32_t W, int32_t H);
size_t fdgs_binning_bytes(int32_t num_rendered, int32_t W, int32_t H);

/* Introspection for parity tests: device pointers into the opaque buffers of a
 * finished forward call.  Arrays are indexed as documented in DESIGN.md. */
typedef struct fdgs_debug_view
{
	uint32_t struct_size;          /* sizeof(fdgs_debug_view)                      */
	const float* depths;           /* [P]   view-space z (0 where culled)          */
	const float* records;          /* [P,12] packed blend record: x,y,conic(3),opacity,r,g,b,depth,flow(2) */
	const float* cov3D;            /* [P,6]                                        */
	const uint32_t* tiles_touched; /* [P]                                          */
	const uint8_t* clamped;        /* [P]   bit c set: colour channel c clamped    */
	const uint32_t* point_list;    /* [R]   Gaussian ids sorted by (tile, depth, id) */
	const uint32_t* ranges;        /* [T,2]                                        */
	const uint32_t* n_contrib;     /* [H*W]                                        */
	const float* final_T;          /* [H*W]                                        */
	const uint32_t* tile_order;    /* [T]   the order in which the blend kernels take the tiles: a permutation of all tiles,
	                                  longest lists first (64 length classes), position p on XCD p % 8; written by one
	                                  workgroup of the tile-scatter (sparse lists: sort) launch, so undefined for P == 0 */
} fdgs_debug_view;
int fdgs_debug_views(int32_t P, int32_t W, int32_t H, int32_t num_rendered,
                     const void* geom_buffer, const void* binning_buffer, const void* image_buffer,
                     fdgs_debug_view* view);

/* Introspection for parity tests of the fused-activation mode (fdgs_scene.raw_params = 1): the activated tensors the
 * kernels derive from the RAW parameters -- sigmoid(opacity), exp(scales), exp(scales_t), v / max(|v|, 1e-12) for the two
 * quaternions (scene/gaussian_model.py:179-219) -- computed by the same device functions, bit-identical to the values
 * preprocess uses in flight.  Any input / output pair may be NULL.  A test feeds them to the oracle, so that the
 * 1e-4 bar applies to the raw_params path as well. */
int fdgs_debug_activations(int32_t P, const float* opacity_raw, const float* scales_raw, const float* scales_t_raw,
                           const float* rotations_raw, const float* rotations_r_raw, float* opacity, float* scales,
                           float* scales_t, float* rotations, float* rotations_r, void* stream);

/* Introspection for the block-cull test: the blend kernels skip a list entry for a whole 8x8 pixel block when a closed-form
 * bound says that no pixel of the block can reach alpha >= 1/255 (csrc/blend_common.h, block_reaches).  tuples [n][10] =
 * mean x, y, conic xx, xy, yy, opacity, rx0, rx1, ry0, ry1 (first / last pixel centre of the block in x and y); out [n][2] =
 * { the bound's verdict, brute force: does any pixel centre of the block pass the blend kernels' own per-pixel test }.
 * The verdict must never be 0 where the brute force says 1. */
int fdgs_debug_block_reaches(int32_t n, const float* tuples, uint8_t* out, void* stream);

/* Measurement aid: a one-wave kernel on `stream` that records, into out5 (DEVICE memory, 5 x uint64), the constant-rate wall
 * clock (s_memrealtime) and the shader-clock counter (s_memtime) at its start and again span_ms later, plus the wall clock's
 * rate in kHz: { wall0, shader0, wall1, shader1, wall_khz }.  (shader1 - shader0) / (wall1 - wall0) * wall_khz = the shader
 * clock in kHz the chip sustained over the interval, under whatever the caller's other streams were running (bench.py:
 * valu_issue_frac at the MEASURED clock).  span_ms in (0, 2000]. */
int fdgs_debug_clock_sample(uint64_t* out5, double span_ms, void* stream);

/* Test hook: lists longer than `lds_cap` entries take the global-scratch sort, tiles whose most crowded depth bucket
 * exceeds `rank_max` the LDS bitonic sort (tilebin.hip); values <= 0 restore the defaults (16384, 96).  Process-wide. */
void fdgs_debug_tile_sort_limits(int32_t lds_cap, int32_t rank_max);

/* Test hook: the tile binning of the forward (csrc/tilebin.hip) on the caller's tile rectangles and depths, without a scene in front of
 * it and a blend behind it.  It runs the launchers the forward runs, with the arguments the forward gives them, and nothing else:
 *   sparse_cap == 0 (compact lists): count -> scan -> scatter -> sort; the sort instances are chosen by the longest list the scan
 *     reported (read back after a stream synchronisation), `max_count` is ignored;
 *   sparse_cap  > 0 (sparse lists: tile t owns the slots [t * sparse_cap, (t + 1) * sparse_cap)): scatter -> sort, the sort's extra
 *     workgroup reporting num_rendered / the longest list and writing the tile order; max_count = the longest list provided for
 *     (<= 0: sparse_cap); capacity >= T * sparse_cap.
 * rect [P] ushort4 (x0, y0, x1, y1: tiles [x0, x1) x [y0, y1) of a grid grid_x tiles wide; x0 == x1 or y0 == y1: none), depths [P]
 * float, both DEVICE memory; the pair of an instance is (bits of the depth, Gaussian index).  `capacity` = the instances `pairs` and
 * `point_list` hold, the number the kernels compare num_rendered with: with more instances than that (compact lists) scatter and
 * sort leave both alone and every range is (0, 0).  Outputs, DEVICE memory owned by the caller, written on `stream`:
 *   counts_out [T]      the tile counters after the count pass (sparse lists: after the scatter pass -- the tiles' true counts)
 *   starts_out [T]      the tile counters after the scan (sparse lists: not written)
 *   ctl_out [2]         { num_rendered, longest list }
 *   pairs [2 capacity]  the scattered (depth bits, index) pairs, in arrival order inside every tile's slice
 *   point_list [capacity], ranges [2 T], order_out [T] (the blend kernels' tile order)
 * pairs, point_list and ranges are written by the kernels themselves, the others are copies out of `scratch`
 * (fdgs_debug_tile_bin_scratch_bytes(T, capacity) bytes of device memory: counters, control words, tile-order area, global sort scratch).
 * FDGS_ERR_INVALID_ARG, with nothing launched: T < 1, T >= 2^24, grid_x < 1, P < 1, capacity < 1, a NULL pointer, a sparse layout that
 * does not fit `capacity`, and a rectangle that leaves the grid (x0 > x1, y0 > y1, x1 > grid_x or y1 * grid_x > T; checked on a host copy
 * of `rect`, after a synchronisation of `stream`: a malformed input becomes an error return, never an atomic out of range).
 * Honours fdgs_debug_tile_sort_limits. */
size_t fdgs_debug_tile_bin_scratch_bytes(int32_t T, int32_t capacity);
int fdgs_debug_tile_bin(int32_t P, const uint16_t* rect, const float* depths, int32_t grid_x, int32_t T, int32_t sparse_cap, int32_t capacity,
                        int32_t max_count, uint32_t* counts_out, uint32_t* starts_out, uint32_t* ctl_out, uint32_t* pairs, uint32_t* point_list,
                        uint32_t* ranges, uint32_t* order_out, void* scratch, void* stream);

/* Test hook: the library's radix sort (csrc/radix_sort.hip, radix_sort_pairs -- the sort behind fdgs_dist2_knn3, fdgs_knn_query and
 * fdgs_rigid_motion_backward; there is no second implementation) run on the caller's n (key, value) pairs of uint32, DEVICE memory.
 * A stable LSD sort by the key bits [bit_lo, bit_hi), RADIX_BITS = 8 bits per pass: pairs with equal selected bits keep their input
 * order.  The pairs are copied into the first of two ping-pong buffer pairs in `scratch` (fdgs_debug_radix_sort_scratch_bytes(n) bytes
 * of device memory, which also holds the histogram area), sorted there, and copied back from whichever pair the result landed in (an odd
 * number of passes leaves it in the second); all on `stream`.  n == 0 and bit_lo == bit_hi are no-ops that return FDGS_OK.
 * FDGS_ERR_INVALID_ARG, with nothing launched: n < 0, a NULL pointer with n > 0, bit ranges outside 0 <= bit_lo <= bit_hi <= 32, and
 * a width bit_hi - bit_lo that is not a multiple of 8.  radix_sort_pairs itself does not check the width: its last pass always takes
 * a whole digit, so a ragged width silently sorts on bits up to the next multiple of 8 above bit_lo (bits beyond 31 read as 0).  The
 * library's own callers pass (0, 32) (knn.hip) and (0, bits of the largest key) (regularize.hip, whose keys have no bits above that). */
size_t fdgs_debug_radix_sort_scratch_bytes(int32_t n);
int fdgs_debug_radix_sort_pairs(int32_t n, int32_t bit_lo, int32_t bit_hi, uint32_t* keys, uint32_t* vals, void* scratch, void* stream);

/* Test hook: where the stages of the two k-NN searches lie in their scratch buffer once fdgs_dist2_knn3(m, ...) (query == 0; n is
 * ignored) or fdgs_knn_query(1, n, m, ...) (query != 0) has run on it: BYTE offsets from the start of `scratch`, computed from the same
 * layout functions the two entries use and from the sort's own rule for which of its two buffers holds the result.  Reads nothing from
 * the device.  offsets[FDGS_KNN_STAGE_*]:
 *   BOUNDS        float[6]          min x, y, z, max x, y, z over the sources, the queries (query search) and the origin
 *   BOXES         float[nboxes][6]  min / max of the sources at positions [b * box, (b + 1) * box) of the sorted order
 *   SRC_CODES     uint32[m]         the sources' 30-bit Morton codes, sorted (stable)
 *   SRC_ORDER     uint32[m]         SRC_ORDER[j] = index of the source at sorted position j
 *   QUERY_CODES, QUERY_ORDER        uint32[n] each, the same for the queries; -1 with query == 0
 *   NBOXES, BOX   not offsets: the number of boxes and the sources per box (1024 / 256)
 * FDGS_ERR_INVALID_ARG: offsets == NULL, n or m < 0. */
#define FDGS_KNN_STAGE_BOUNDS 0
#define FDGS_KNN_STAGE_BOXES 1
#define FDGS_KNN_STAGE_SRC_CODES 2
#define FDGS_KNN_STAGE_SRC_ORDER 3
#define FDGS_KNN_STAGE_QUERY_CODES 4
#define FDGS_KNN_STAGE_QUERY_ORDER 5
#define FDGS_KNN_STAGE_NBOXES 6
#define FDGS_KNN_STAGE_BOX 7
#define FDGS_KNN_NUM_STAGES 8
int fdgs_debug_knn_stage_offsets(int32_t query, int32_t n, int32_t m, int64_t* offsets);

/* Optional per-stage timing with HIP events recorded on the caller's stream (so the
 * numbers are the kernels' own durations on that stream, not host wall time).
 * Disabled by default; when enabled each stage of forward / backward is bracketed
 * by an event pair (non-blocking).  fdgs_profile_read synchronises the pending
 * events and returns the accumulated milliseconds and the number of samples. */
#define FDGS_STAGE_PREPROCESS_FWD 0
#define FDGS_STAGE_TILE_COUNT 1
#define FDGS_STAGE_TILE_SCAN 2
#define FDGS_STAGE_TILE_SCATTER 3
#define FDGS_STAGE_TILE_SORT 4
#define FDGS_STAGE_COLOUR_FWD 5  /* the SH colour half of the preprocess when the forward runs it on its second stream (split_colour) */
#define FDGS_STAGE_BLEND_FWD 6
#define FDGS_STAGE_BLEND_BWD 7
#define FDGS_STAGE_PREPROCESS_BWD 8
#define FDGS_STAGE_GRAD_ZERO 9
#define FDGS_STAGE_SH_BWD 10
#define FDGS_STAGE_CAMERA_BWD 11 /* fdgs_camera_backward: both of its launches */
#define FDGS_NUM_STAGES 12
int fdgs_profile_enable(int stage_mask); /* bit i set: bracket stage i with HIP events; 0 = off, -1 = all stages */
int fdgs_profile_sample_every(int32_t n); /* n >= 1: only every n-th launch of a bracketed stage gets its event pair (default 1: every
                                             launch).  An event pair costs its stream ~13 us of idle time around the launch (measured: a
                                             6-7 us gap in front of and behind every bracketed blend backward in the kernel trace); a caller
                                             that measures a stage INSIDE a timed region samples it -- n coprime to the views per step, so
                                             that the samples rotate through the views */
int fdgs_profile_read(int stage, double* total_ms, int64_t* samples);
int fdgs_profile_reset(void);
const char* fdgs_stage_name(int stage);

/* ---- adjacent row: fused photometric loss ----------------------------
 * (1 - lambda) * mean|img - gt| + lambda * (1 - SSIM(img, gt)), the reference's loss
 * (train.py:115-117, utils/loss_utils.py:17-64: 11x11 Gaussian window, sigma 1.5, zero padding).
 * forward writes three per-pixel derivative maps [C,H,W] (kept for backward) and per-tile partial sums
 * of |img-gt| and ssim (fdgs_l1_ssim_num_partials entries each; the host adds them up).
 * backward writes dL/dimg [C,H,W] given the upstream scalar gradient (device pointer). */
int fdgs_l1_ssim_forward(const float* img, const float* gt, int32_t C, int32_t H, int32_t W,
                         float* dm_dmu1, float* dm_de11, float* dm_de12,
                         float* partial_l1, float* partial_ssim, void* stream);
int fdgs_l1_ssim_backward(const float* img, const float* gt, int32_t C, int32_t H, int32_t W,
                          const float* dm_dmu1, const float* dm_de11, const float* dm_de12,
                          const float* upstream, float lambda_dssim, float* dL_dimg, void* stream);
int fdgs_l1_ssim_num_partials(int32_t C, int32_t H, int32_t W);
/* Value and gradient in ONE pass (what a training step needs; same arithmetic, bit-identical results): dL_dimg = upstream[0] *
 * d loss / d img and the per-tile partial sums for fdgs_l1_ssim_loss, without the three derivative maps of the two-call path
 * travelling through memory (a workgroup rebuilds the derivative maps around its tile from the images: more arithmetic, a third
 * of the HBM traffic).  utils/loss_utils.py:34-64 + its autograd backward. */
int fdgs_l1_ssim_value_and_grad(const float* img, const float* gt, int32_t C, int32_t H, int32_t W,
                                const float* upstream, float lambda_dssim, float* dL_dimg,
                                float* partial_l1, float* partial_ssim, void* stream);
/* Reduces the per-tile partial sums of the forward call (fixed order: deterministic) to
 * loss_l1_ssim[0] = (1 - lambda) * L1 + lambda * (1 - SSIM), [1] = L1, [2] = SSIM   (device memory, 3 floats). */
int fdgs_l1_ssim_loss(const float* partial_l1, const float* partial_ssim, int32_t num_partials, int32_t C, int32_t H, int32_t W,
                      float lambda_dssim, float* loss_l1_ssim, void* stream);
/* The same reduction for every view of an optimizer step in ONE launch (one workgroup per view; bit-identical to num_views calls of
 * fdgs_l1_ssim_loss): partials = [num_views][2][num_partials] -- view v's partial_l1 at partials + v * 2 * num_partials, its
 * partial_ssim num_partials floats behind -- losses = [num_views][3]. */
int fdgs_l1_ssim_loss_batch(const float* partials, int32_t num_views, int32_t num_partials, int32_t C, int32_t H, int32_t W,
                            float lambda_dssim, float* losses, void* stream);

/* ---- adjacent row: fused Adam over a flat parameter bucket ---------
 * torch.optim.Adam arithmetic (no amsgrad / weight decay) in one streaming pass over four flat fp32
 * buffers.  Learning rates come from `segments`: elements [begin, end) use `lr`, except that when
 * period > 0 the first `head` elements of every `period` use `lr_head` (SH DC vs. rest inside one
 * [P, M, 3] tensor).  Elements outside every segment are left with lr = 0 (moments still update). */
typedef struct fdgs_adam_segment
{
	int64_t begin, end;
	float lr, lr_head;
	int32_t period, head;
} fdgs_adam_segment;
int fdgs_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                   const fdgs_adam_segment* segments, int32_t num_segments,
                   float beta1, float beta2, float eps, int32_t step, void* stream);

/* Adam over the SH coefficients [P,M,3] with the gradient taken straight from the staged views of the deferred SH backward
 * (fdgs_backward_out.sh_stage): fdgs_sh_flush + fdgs_adam_step on that segment in one pass, without the 12 M bytes per
 * Gaussian of dL_dsh going out to memory and coming back.  params / exp_avg / exp_avg_sq point at the [P,M,3] segment; the
 * first 3 floats of every row (the DC coefficient, scene/gaussian_model.py:339) use lr_dc, the others lr.  dL_dsh: NULL, or
 * [P,M,3] that also receives the summed gradient (bit-identical to fdgs_sh_flush).  The update is bit-identical to
 * fdgs_sh_flush followed by fdgs_adam_step.  Needs rows of whole float4s (3 M % 4 == 0) and 16-byte aligned arrays:
 * FDGS_ERR_INVALID_ARG otherwise (the caller falls back to the two calls). */
int fdgs_adam_step_sh(float* params, float* exp_avg, float* exp_avg_sq, float* dL_dsh,
                      int32_t P, int32_t D, int32_t D_t, int32_t M, int32_t gaussian_dim, int32_t force_sh_3d,
                      int32_t analytic_sh_grad, int32_t num_views, const float* stages,
                      float lr, float lr_dc, float beta1, float beta2, float eps, int32_t step, void* stream);

/* ---- adjacent row: densification / pruning of the flat-bucket model --------------
 * Replaces the boolean-mask gathers and torch.cat calls of scene/gaussian_model.py:391-610 (densify_and_clone,
 * densify_and_split, prune_points, cat_tensors_to_optimizer, _prune_optimizer) for a model whose parameters,
 * exp_avg and exp_avg_sq are one flat buffer each (segments [P,row_0] [P,row_1] ... back to back). */
#define FDGS_DENSIFY_CLONE 1        /* clone this Gaussian (gaussian_model.py:545-569)                          */
#define FDGS_DENSIFY_SPLIT 2        /* replace it by N samples (:487-543)                                       */
#define FDGS_DENSIFY_PRUNE 4        /* the Gaussian (and its clone) fails the final prune test (:598-603)       */
#define FDGS_DENSIFY_PRUNE_CHILD 8  /* its split children (scaling / (0.8 N)) fail the final prune test         */
/* Densification statistics of one optimizer step (train.py:164-184, 229-236; gaussian_model.py:637-642), two phases so
 * that the per-Gaussian sums can be all-reduced in between (count, pgrad: SUM; radii_max: MAX):
 *   local: this rank's views -> count = #views with radius > 0, pgrad = sum of ||dL/dmean2D.xy||, radii_max (all [P] float);
 *   apply: for Gaussians seen at least once, max_radii2D = max(., radii_max), xyz_gradient_accum += pgrad * batch / count,
 *          denom += 1, t_gradient_accum += t_grad * batch / count (t_grad NULL: skipped).
 * radii / viewspace_grad: HOST arrays of num_views (<= 16) device pointers ([P] int32, [P,3] float). */
int fdgs_densify_stats_local(int32_t P, int32_t num_views, const int32_t* const* radii, const float* const* viewspace_grad,
                             float* count, float* pgrad, float* radii_max, void* stream);
int fdgs_densify_stats_apply(int32_t P, const float* count, const float* pgrad, const float* radii_max, const float* t_grad,
                             float global_batch, float* xyz_gradient_accum, float* t_gradient_accum, float* denom,
                             float* max_radii2D, void* stream);
/* Per-Gaussian decision flags from the densification statistics.  max_screen_size <= 0: no size test
 * (`if max_screen_size:`); percent_dense, extent: as training_setup / cameras_extent; prune_only as in :584. */
int fdgs_densify_classify(int32_t P, const float* xyz_gradient_accum, const float* denom, const float* scaling_raw,
                          const float* opacity_raw, const float* max_radii2D, float max_grad, float min_opacity,
                          float extent, float max_screen_size, float percent_dense, int32_t N, int32_t prune_only,
                          uint8_t* flags, void* stream);
/* Builds the three new flat buffers: row j of every segment is row src[j] of the old one; kind[j] == 0 keeps the
 * Adam moments, anything else zeroes them (new points, gaussian_model.py:441-442). */
int fdgs_densify_gather(int32_t num_segments, const int32_t* row_floats, int64_t P_old, int64_t P_new,
                        const int32_t* src, const uint8_t* kind, const float* old_params, const float* old_exp_avg,
                        const float* old_exp_avg_sq, float* new_params, float* new_exp_avg, float* new_exp_avg_sq, void* stream);
/* Split children (gaussian_model.py:497-524): new_* point at the children's rows of the new arrays; parent[c] indexes
 * the OLD arrays; samples [n,4] (rot_4d) or [n,3] (+ samples_t [n] for 4D without rot_4d) are draws of N(0, std). */
int fdgs_densify_split(int32_t n_children, int32_t N, int32_t rot_4d, int32_t gaussian_dim, const int32_t* parent,
                       const float* samples, const float* samples_t, const float* xyz, const float* t, const float* scaling,
                       const float* scaling_t, const float* rotation, const float* rotation_r,
                       float* new_xyz, float* new_t, float* new_scaling, float* new_scaling_t, void* stream);

/* ---- adjacent row: simple-knn's distCUDA2 (simple-knn/spatial.cu:15-27) ----------
 * mean_dist2[i] = mean of the squared distances from points[i] to its three nearest other points ([P,3] float,
 * device).  scratch: fdgs_knn_scratch_bytes(P) bytes of device memory.  Exact search; bit-exact vs the oracle. */
size_t fdgs_knn_scratch_bytes(int32_t P);
int fdgs_dist2_knn3(int32_t P, const float* points, float* mean_dist2, void* scratch, void* stream);

/* ---- k nearest neighbours: pointops2's knnquery (utils/general_utils.py:170-184) ----------------------------------------
 * For every batch bb < b and query i < n: the k sources of that batch nearest to x[bb][i] ([b,n,3] and [b,m,3] float, device),
 * exact, each row sorted by (d2, source index) ascending, d2 = (dx*dx + dy*dy) + dz*dz in fp32.  idx [b,n,k] (batch-local source
 * indices), dist2 [b,n,k] (SQUARED distances).  Slots no source fills (m < k) hold dist2 = 1e10, idx = 0, as the reference's
 * initial heap; a source at d2 >= 1e10 is never taken.  1 <= k <= FDGS_KNN_MAX_K; m <= 2^24 per batch.
 * scratch: fdgs_knn_query_scratch_bytes(n, m) bytes of device memory (reused from batch to batch). */
#define FDGS_KNN_MAX_K 64
size_t fdgs_knn_query_scratch_bytes(int32_t n, int32_t m);
int fdgs_knn_query(int32_t b, int32_t n, int32_t m, int32_t k, const float* x, const float* src, int64_t* idx, float* dist2,
                   void* scratch, void* stream);

/* ---- the reference trainer's regularisers (train.py:119-159) on a rot_4d model with gaussian_dim == 4 -------------------
 * Inputs: the RAW parameters scaling [P,3], scaling_t [P,1], rotation [P,4], rotation_r [P,4] (quaternions of any norm), t [P,1],
 * and the k-NN of the means (fdgs_knn_query with x = src: knn_idx int64 [P,k], knn_d2 [P,k]).
 * velocity v_i = Sigma[0:3,3] / Sigma[3,3] * dt_i, dt_i = (t_i + 0.1f) - t_i (gaussian_model.py:34-47, 247-251), written to
 * velocity [P,3];  losses[0] = L_rigid = sum_ij exp(-100 d2_ij) |v_nbr(i,j) - v_i| / k / P,  losses[1] = L_motion = mean_i |v_i|
 * (device memory, 2 floats; deterministic: fixed-order sums of per-workgroup partials).
 * scratch: fdgs_rigid_motion_scratch_bytes(P, k) bytes (forward and backward; P * k < 2^31). */
size_t fdgs_rigid_motion_scratch_bytes(int32_t P, int32_t k);
int fdgs_rigid_motion_forward(int32_t P, int32_t k, const float* scaling, const float* scaling_t, const float* rotation,
                              const float* rotation_r, const float* t, const int64_t* knn_idx, const float* knn_d2, float* velocity,
                              float* losses, void* scratch, void* stream);
/* ADDS  scale * (g_losses[0] * dL_rigid/d. + g_losses[1] * dL_motion/d.)  into d_scaling, d_scaling_t, d_rotation, d_rotation_r
 * (g_losses: 2 floats of device memory).  The neighbour side of the rigid term is gathered through a reverse-neighbour list
 * (a stable sort of the (neighbour, pair) table), so the result is bitwise reproducible.  |0|'s gradient is 0 (torch.norm). */
int fdgs_rigid_motion_backward(int32_t P, int32_t k, const float* scaling, const float* scaling_t, const float* rotation,
                               const float* rotation_r, const float* t, const int64_t* knn_idx, const float* knn_d2,
                               const float* velocity, const float* g_losses, float scale, float* d_scaling, float* d_scaling_t,
                               float* d_rotation, float* d_rotation_r, void* scratch, void* stream);

/* ---- the opacity-mask loss (train.py:120-128): o = clamp(alpha, 1e-6, 1 - 1e-6), L = mean(-(1 - mask) log(1 - o)) -------
 * alpha [H,W] (or T with alpha_is_T != 0: alpha = 1 - T), mask [H,W].  partials: fdgs_opa_mask_num_partials(H, W) floats;
 * loss: 1 float; both device memory.  With grad != NULL also d L / d alpha = (1 - mask) / (1 - o) / (H W) where the clamp passes
 * it (lo <= alpha <= hi), else 0, times scale (and times *g_upstream if that is not NULL), written (accumulate = 0) or added. */
int fdgs_opa_mask_num_partials(int32_t H, int32_t W);
int fdgs_opa_mask_loss(int32_t H, int32_t W, const float* alpha, int32_t alpha_is_T, const float* mask, const float* g_upstream,
                       float scale, float* grad, int32_t accumulate, float* partials, float* loss, void* stream);

/* ---- the environment map behind the Gaussians (gaussian_renderer/__init__.py:165-177 of the reference) --------------------
 * Per pixel (i, j): the ray of the pixel centre, d = normalize((inv(viewmatrix^T) ((i + .5 - cx) / fl_x, (j + .5 - cy) / fl_y, 1, 1))[:3]
 * - campos) with origin campos (scene/cameras.py:75-82), meets the sphere of `radius` about the origin at
 * t = -(o.d) + sqrt(delta) / (d.d) (the reference's operator precedence); the point (x, y, z) there is looked up at
 * u = atan2(y, x) / 2pi + 0.5, v = acos(z / radius) / pi by a bilinear grid_sample (align_corners = False, zero padding: the seam
 * at u = 0 / 1 does not wrap) of env [3, env_h, env_w].  One deliberate difference: ray and texture coordinates are computed in
 * float64 and v as atan2(sqrt(x^2 + y^2), z), which is acos(clamp(z / radius, -1, 1)) on the sphere: no NaN looking at the pole (fp32
 * gives z / radius = 1.0000001 there, and the reference's acos a NaN), and no loss of v to fp32's acos near the poles.  The bilinear
 * weights are rounded to fp32.  The camera must lie inside the sphere (the reference
 * asserts delta > 0; the library does not check it).  viewmatrix / campos: the camera's world_view_transform [16] (row-major, as the
 * rasterizer takes it) and camera_center [3]; the 4x4 inverse is taken on the device.  All arrays are device memory; images planar
 * [3, H, W], T [H, W] the rasterizer's final transmittance.
 *
 * colour_out = colour_in + T * env(ray(pixel)); colour_out may alias colour_in. */
int fdgs_env_composite(int32_t H, int32_t W, const float* viewmatrix, const float* campos, float fl_x, float fl_y,
                       float cx, float cy, const float* env, int32_t env_h, int32_t env_w, float radius,
                       const float* T, const float* colour_in, float* colour_out, void* stream);
/* g_alpha (+)= -sum_c g_colour_c * env_c   (the gradient w.r.t. alpha = 1 - T, as fdgs_backward_in.dL_dout_alpha; NULL: not computed)
 * g_env   (+)= sum over pixels of g_colour * T * bilinear weights   (NULL: not computed)
 * "(+)=": written, or added with accumulate_* != 0.  g_env is summed with float atomics (per 16 x 16 pixel tile in LDS first): like
 * the reference's grid_sample backward and fdgs_rasterize_backward, it is reproducible to the order of arrival only. */
int fdgs_env_composite_backward(int32_t H, int32_t W, const float* viewmatrix, const float* campos, float fl_x, float fl_y,
                                float cx, float cy, const float* env, int32_t env_h, int32_t env_w, float radius,
                                const float* T, const float* g_colour, float* g_alpha, int32_t accumulate_alpha,
                                float* g_env, int32_t accumulate_env, void* stream);

/* ---- evaluation metrics of one view (train.py:276-345, training_report) ----------------------------------------------------
 * img (the render) and gt [C, H, W] float, device memory.  out4 (device memory, 4 floats) = [l1, psnr, ssim, msssim]:
 *   l1     mean |img - gt|                                                  (utils/loss_utils.py:18)
 *   psnr   mean over channels of 20 log10(1 / sqrt(mse_c)), +inf where mse_c = 0 (utils/image_utils.py:17-19)
 *   ssim   the training loss's SSIM: 11x11 Gaussian window, sigma 1.5, zero padding, mean over all pixels and channels
 *   msssim torchmetrics' MultiScaleStructuralSimilarityIndexMeasure(data_range = 1): five scales of 2x2 average pooling; per scale
 *          the means of SSIM and CS = (2 s_xy + C2) / (s_x^2 + s_y^2 + C2) over the valid (H - 10) x (W - 10) window positions,
 *          relu'd; prod_{s<4} cs_s^beta_s * sim_4^beta_4, beta = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
 * flags: FDGS_METRICS_CLAMP clamps img to [0, 1] first (the reference's evaluation; gt is never clamped); FDGS_METRICS_NO_MSSSIM
 * skips MS-SSIM (out4[3] = NaN) and allows any size.  Without it both sides must be >= 176 (H // 16 > 10, W // 16 > 10, as
 * torchmetrics), else FDGS_ERR_INVALID_ARG.  Fixed-order sums: the row is bitwise reproducible.  scratch: device memory of
 * fdgs_eval_metrics_scratch_bytes(C, H, W) bytes (-1: invalid sizes), reusable by the next call on the same stream. */
#define FDGS_METRICS_CLAMP 1
#define FDGS_METRICS_NO_MSSSIM 2
int fdgs_eval_metrics_scratch_bytes(int32_t C, int32_t H, int32_t W);
int fdgs_eval_metrics(const float* img, const float* gt, int32_t C, int32_t H, int32_t W, int32_t flags, void* scratch,
                      float* out4, void* stream);

/* ---- ground-truth frames kept as 8-bit images, decoded on the device -----------------------------------------------------------
 * What the reference's loader computes on the host for every image (utils/general_utils.py:22-28 PILtoTorch: np.array(pil) / 255.0,
 * permuted to [C, H, W]; scene/cameras.py:53-57: image *= gt_alpha_mask; utils/data_utils.py:16-34 the same per batch) and then
 * moves to the device as float32 inside the step (train.py:106), done here from the 8-bit data: a quarter of the memory or of the
 * bus traffic.  frames: N images uint8 [H, W, C], interleaved, C = 3 or 4, one behind the other (frame n at n*H*W*C bytes).
 * index: B int32 frame numbers in DEVICE memory (no host-side table, no synchronisation to enqueue the call); the B frames of the
 * batch are decoded by ONE launch.  Image b of the batch goes to out + b * out_stride as float32 [3, H, W] and, with C = 4 and
 * mask_out != NULL, its alpha plane to mask_out + b * mask_stride as [1, H, W] (strides in floats, at least 3 H W and H W).
 * fp32, exactly these IEEE operations in this order, bit for bit what the reference's loader produces:
 *   v = float(u8) / 255.0f  for every channel (a division, not a product with 1/255.f);
 *   C = 4:  mask = a / 255.0f,  rgb = v * mask.
 * No clamp: the values are in [0, 1] by construction.  A frame number outside [0, N) writes nothing for that image of the batch.
 * Shapes: a lane takes 4 consecutive pixels with dword / 16-byte accesses when every frame starts on a dword (H*W*C a multiple of
 * 4: every RGBA shape, RGB with H*W a multiple of 4; the last H*W mod 4 pixels one by one); other RGB shapes, and pointers that are
 * not dword-aligned, take a byte-wise path with one pixel per lane.  FDGS_ERR_INVALID_ARG: C outside {3, 4}, non-positive N, H, W
 * or B, B > 65535, H*W > 2^31 - 4096, a NULL frames / index / out, a stride below the image's size. */
int fdgs_frames_decode(const uint8_t* frames, int32_t N, int32_t H, int32_t W, int32_t C, const int32_t* index, int32_t B,
                       float* out, int64_t out_stride, float* mask_out, int64_t mask_stride, void* stream);

/* ---- float images written out as 8-bit frames: the inverse of fdgs_frames_decode ----------------------------------------------------
 * images: B float32 images [3, H, W], image b at images + b * image_stride (floats, at least 3 H W); with C = 4 also alphas: B planes
 * [1, H, W] at alphas + b * alpha_stride (at least H W) for the fourth byte.  frames: N images uint8 [H, W, C], interleaved, C = 3
 * or 4, one behind the other; index: B int32 frame numbers in DEVICE memory: image b is written to frame index[b]; a number outside
 * [0, N) writes nothing.  ONE launch for the batch.  fp32, exactly these IEEE operations in this order per value (torchvision's
 * save_image: img.mul(255).add_(0.5).clamp_(0, 255).to(uint8)), no fused multiply-add:
 *   t = v * 255.0f;  t = t + 0.5f;  q = (uint8) min(max(t, 0.0f), 255.0f)  (truncating);  NaN -> 0.
 * fdgs_frames_encode(fdgs_frames_decode(q)) == q for all 256 bytes.  Shapes: a lane takes 4 consecutive pixels with 16-byte loads
 * and dword stores when every frame starts on a dword (H*W*C a multiple of 4); other shapes, and pointers that are not
 * dword-aligned, take a byte-wise path with one pixel per lane.  FDGS_ERR_INVALID_ARG: C outside {3, 4}, non-positive N, H, W or B,
 * B > 65535, H*W > 2^31 - 4096, a NULL images / index / frames (or alphas with C = 4), a stride below the image's size. */
int fdgs_frames_encode(const float* images, int64_t image_stride, const float* alphas, int64_t alpha_stride, int32_t B,
                       int32_t H, int32_t W, int32_t C, uint8_t* frames, int32_t N, const int32_t* index, void* stream);

/* The reference's grey depth image (utils/image_utils.py:21-28 easy_cmap, what training_report logs): B float32 planes [H, W] at
 * planes + b * plane_stride -> frames uint8 [N, H, W, 1] (ONE channel; a viewer replicates it), frame index[b] as above.
 *   g = clamp((d - min) / (max - min), 0, 1)  -- one IEEE subtraction, one IEEE division, min / max over the plane (a NaN in the
 * plane makes both NaN, as torch.min / torch.max) -- then the quantisation above.  max == min gives 0 / 0 = NaN -> 0.
 * Two launches on `stream`: a wave64 min / max reduction that leaves one (min, max) pair per workgroup in `scratch`, and the encode,
 * whose workgroups finish the pairs of their plane.  No atomics.  scratch: device memory of fdgs_frames_encode_gray_scratch_bytes(B,
 * H, W) bytes (-1: invalid sizes), dword-aligned, reusable by the next call on the same stream. */
int64_t fdgs_frames_encode_gray_scratch_bytes(int32_t B, int32_t H, int32_t W);
int fdgs_frames_encode_gray(const float* planes, int64_t plane_stride, int32_t B, int32_t H, int32_t W, uint8_t* frames, int32_t N,
                            const int32_t* index, void* scratch, void* stream);

/* ---- 8-bit frames resized on the device: Pillow's Image.resize (BICUBIC), byte for byte -----------------------------------------------
 * What the reference's loader does on the host for every image (utils/camera_utils.py:19-49 loadCam -> PILtoTorch(image, resolution)
 * = pil_image.resize(resolution)), done here from full-size 8-bit frames: dst[b] = resize(src[index[b]]) for the B entries of a
 * DEVICE-side index.  src: N frames uint8 [Hs, Ws, C], dst: M >= B frames [Hd, Wd, C], interleaved, C = 3 or 4, as for
 * fdgs_frames_decode; an index outside [0, N) leaves its destination frame unwritten.  Integer arithmetic only:
 *   one pass:  out = clip(0, 255, (2^21 + sum_x k[x] * in[xmin + x]) >> 22), int32 accumulator, arithmetic shift;
 *   the horizontal pass first, into an intermediate rounded to uint8, the vertical pass over that; a pass whose axis keeps its
 *   length is skipped, and with both skipped the result is a plain copy;
 *   RGBA, whenever a pass runs: premultiplied first, c' = ((t >> 8) + t) >> 8 with t = c a + 128; afterwards, where the new alpha
 *   is neither 0 nor 255, c = min(255, (255 c') / a).
 * kx [Wd, ksize_x] / ky [Hd, ksize_y]: the taps in fixed point (22 fractional bits), bx [Wd, 2] / by [Hd, 2]: (xmin, count) per
 * output index, int32 in device memory, built on the host in float64 (fdgs.resize.coefficients); ksize = ceil(2 max(n_in / n_out,
 * 1)) * 2 + 1 per axis.  The tables of an unchanged axis must be passed and are not read.  Bounds outside the axis are clamped,
 * never followed.  One launch (a fused kernel with the intermediate of an output tile in LDS) whenever the source window of some
 * tile fits LDS; otherwise two launches with the intermediate [B, Hs, Wd, C] in `scratch`:
 * fdgs_frames_resize_scratch_bytes(...) bytes (0 where none is needed: scratch may then be NULL; -1 for invalid sizes).  Enqueued on
 * `stream`, no host synchronisation.  FDGS_ERR_INVALID_ARG with nothing launched: C outside {3, 4}, non-positive sizes, B > 65535,
 * B > M, a frame / result / intermediate of 2^31 - 4096 bytes or more, a NULL src / index / dst / table (or scratch where needed),
 * a ksize that disagrees with the sizes.
 * fdgs_debug_frames_resize_path(1) makes every later call take the two-launch path (tests, A/B timing); 0 restores the choice. */
int fdgs_frames_resize(const uint8_t* src, int32_t N, int32_t Hs, int32_t Ws, int32_t C, const int32_t* index, int32_t B,
                       uint8_t* dst, int32_t M, int32_t Hd, int32_t Wd,
                       const int32_t* kx, const int32_t* bx, int32_t ksize_x,
                       const int32_t* ky, const int32_t* by, int32_t ksize_y,
                       void* scratch, void* stream);
int64_t fdgs_frames_resize_scratch_bytes(int32_t B, int32_t Hs, int32_t Ws, int32_t Hd, int32_t Wd, int32_t C);
void fdgs_debug_frames_resize_path(int32_t path);

/* RGBA frames over a white (white != 0) or black background, the step of the reference's readers before the resize
 * (scene/dataset_readers.py:249-259, utils/data_utils.py:20-23), in float64 with every operation rounded on its own:
 *   out = floor(((c / 255.0) * (a / 255.0) + bg * (1.0 - a / 255.0)) * 255.0)
 * src_rgba: N frames uint8 [H, W, 4]; dst: [N, H, W, 4] with the alpha byte kept (keep_alpha != 0) or [N, H, W, 3].  One launch.
 * FDGS_ERR_INVALID_ARG: non-positive sizes, a frame of 2^31 - 4096 bytes or more, a NULL pointer. */
int fdgs_frames_composite(const uint8_t* src_rgba, int32_t N, int32_t H, int32_t W, int32_t white, int32_t keep_alpha,
                          uint8_t* dst, void* stream);

/* ---- a 4D model at one timestamp as 3D Gaussians ---------------------------------------------------------------------------------
 * At time t a 4D Gaussian is a 3D Gaussian: the conditional mean and covariance (rot_4d: forward.cu:279-352; otherwise the plain mean
 * and R S^2 R^T), the opacity times the temporal marginal, an SH row with the time blocks folded in.  The call computes that for the
 * Gaussians that pass the forward's own temporal cull -- marginal = expf(-0.5 dt^2 / (prefilter_var > 0 ? prefilter_var + cov_t :
 * cov_t)) > 0.05, cov_t = Sigma[3][3] with rot_4d, else scales_t * scale_modifier (not squared: the reference's quirk,
 * forward.cu:431-436) -- and writes them COMPACTED, in ascending original index.  Same expressions, promotions and expf as the forward's
 * preprocess: where the forward keeps a Gaussian, xyz / cov3D / opacity are its out_means3D / cov3D / opacity bit for bit.
 * The inputs are the model's RAW parameters (as fdgs_scene.raw_params = 1): opacities pre-sigmoid, scales / scales_t pre-exp,
 * quaternions of any norm; gaussian_dim == 4 is implied.  shs [n,16,3]: coefficient k < (D + 1)^2 is sh[k] + t1 sh[16 + k] + t2 sh[32 + k],
 * tk = (float)cos(2 pi k (ts - timestamp) / time_duration) as the forward evaluates it, the time terms only where the forward has them
 * (4D SH, D == 3, D_t >= 1 / 2; force_sh_3d: block 0 only); coefficients at or beyond (D + 1)^2 are written as 0.  SH rows of culled
 * Gaussians are not read.  One deliberate difference a slice cannot remove: the forward's 4D path takes the SH view direction from the
 * UNSHIFTED mean (forward.cu:79-81); whoever renders the slice takes it from xyz, the shifted one.
 * Three launches on `stream`, no atomics.  Rows at or beyond `capacity` are never written; *n_live always is (it may exceed capacity:
 * the caller then holds the first `capacity` rows).  scratch: fdgs_time_slice_scratch_bytes(P) bytes of device memory. */
typedef struct fdgs_slice_in
{
	uint32_t struct_size;   /* sizeof(fdgs_slice_in)                                 */
	int32_t P;              /* number of Gaussians                                   */
	int32_t D, D_t, M;      /* active SH degree, active time degree, SH coeffs/pt    */
	const float* means3D;     /* [P,3]                                               */
	const float* shs;         /* [P,M,3]                                             */
	const float* opacities;   /* [P]   raw                                           */
	const float* ts;          /* [P]                                                 */
	const float* scales;      /* [P,3] raw                                           */
	const float* scales_t;    /* [P]   raw                                           */
	const float* rotations;   /* [P,4] raw                                           */
	const float* rotations_r; /* [P,4] raw; NULL without rot_4d                      */
	float scale_modifier;
	float prefilter_var;
	float timestamp, time_duration;
	int32_t rot_4d, force_sh_3d;
} fdgs_slice_in;
typedef struct fdgs_slice_out
{
	uint32_t struct_size;   /* sizeof(fdgs_slice_out)                                */
	int32_t capacity;       /* rows the arrays below hold                            */
	int32_t* index;         /* [capacity]       original index of the row            */
	float* xyz;             /* [capacity,3]                                          */
	float* cov3D;           /* [capacity,6]     xx, xy, xz, yy, yz, zz               */
	float* opacity;         /* [capacity]       sigmoid(raw) * marginal              */
	float* shs;             /* [capacity,16,3]                                       */
	float* scales;          /* [capacity,3] or NULL; with rotations: cov3D = R diag(scales^2) R^T by an in-kernel cyclic Jacobi; */
	float* rotations;       /* [capacity,4] or NULL  scales floored at 1e-15, unit quaternions (w,x,y,z) of a proper rotation    */
	int32_t* n_live;        /* device int: how many Gaussians are live               */
} fdgs_slice_out;
size_t fdgs_time_slice_scratch_bytes(int32_t P);
int fdgs_time_slice(const fdgs_slice_in* in, const fdgs_slice_out* out, void* scratch, void* stream);

/* ---- optical flow: how far every Gaussian moves on the screen between two views ----------------------------------------------------
 *   flows[i] = pix(mu_i(timestamp_to); target camera) - pix(mu_i(timestamp); source camera)        [pixels]
 * mu_i(t): the mean as the forward's preprocess has it at time t -- with rot_4d the conditional mean p + Sigma[0:3,3] / Sigma[3,3] *
 * (t - ts), Sigma built exactly as the forward builds it (same scale_modifier): where the forward keeps the Gaussian, its
 * out_means3D bit for bit -- otherwise the plain mean (the flow is then the camera's alone).  pix: the forward's own mean -> pixel
 * expressions (full projection, 1 / (w + 1e-7f), ndc2Pix in double): the flow of a Gaussian that the forward keeps in both views is
 * the difference of the positions in its two blend records, bit for bit; equal timestamps and one camera give exactly (0, 0).
 * viewmatrix_to / projmatrix_to: the target camera (same image size), both NULL: the source camera.  A Gaussian whose view-space
 * z <= 0.2 (the forward's near cull) at either end gets (0, 0) and no gradient; the temporal cull is NOT applied, every row is
 * written.  This is what fdgs_scene.flows takes: the blend then renders sum_i flows[i] alpha_i T_i into out_flow.
 * The parameter tensors are as in fdgs_scene (raw_params = 1: scales / scales_t before exp, quaternions of any norm); without rot_4d
 * only means3D is read.  gaussian_dim 3 or 4; rot_4d needs 4 and ts / scales / scales_t / rotations / rotations_r.  The quaternions
 * need not be 16-byte aligned.  One launch on `stream`, no atomics; P == 0: nothing is launched.  FDGS_ERR_INVALID_ARG before any
 * launch: a NULL in / viewmatrix / projmatrix / flows / required tensor, only one of the _to matrices, P < 0, W or H <= 0. */
typedef struct fdgs_flow_in
{
	uint32_t struct_size;      /* sizeof(fdgs_flow_in)                                  */
	int32_t P;                 /* number of Gaussians                                   */
	int32_t W, H;              /* image size of both views                              */
	const float* means3D;      /* [P,3]                                                 */
	const float* ts;           /* [P]                      rot_4d only                  */
	const float* scales;       /* [P,3]                    rot_4d only                  */
	const float* scales_t;     /* [P]                      rot_4d only                  */
	const float* rotations;    /* [P,4]                    rot_4d only                  */
	const float* rotations_r;  /* [P,4]                    rot_4d only                  */
	const float* viewmatrix;   /* [16] source camera, as fdgs_scene.viewmatrix          */
	const float* projmatrix;   /* [16] source camera, as fdgs_scene.projmatrix          */
	const float* viewmatrix_to;/* [16] target camera or NULL                            */
	const float* projmatrix_to;/* [16] target camera or NULL                            */
	float timestamp;           /* source time                                           */
	float timestamp_to;        /* target time                                           */
	float scale_modifier;
	int32_t rot_4d, gaussian_dim, raw_params;
} fdgs_flow_in;
int fdgs_gaussian_flow_forward(const fdgs_flow_in* in, float* flows, void* stream);
/* ADDS scale * dL/d(parameter) of L(flows) to every array that is not NULL, given dL_dflows [P,2]: the analytic gradient of the
 * forward above (the cameras and the timestamps are constants), with respect to the tensors AS PASSED: through exp and the
 * quaternion normalisation with raw_params = 1, with respect to the activated values otherwise.  Without rot_4d only d_means3D
 * receives anything.  One launch, one lane per Gaussian, no atomics: bitwise reproducible. */
typedef struct fdgs_flow_grads
{
	uint32_t struct_size;      /* sizeof(fdgs_flow_grads)                               */
	float* d_means3D;          /* [P,3] or NULL                                         */
	float* d_ts;               /* [P]   or NULL                                         */
	float* d_scales;           /* [P,3] or NULL                                         */
	float* d_scales_t;         /* [P]   or NULL                                         */
	float* d_rotations;        /* [P,4] or NULL                                         */
	float* d_rotations_r;      /* [P,4] or NULL                                         */
} fdgs_flow_grads;
int fdgs_gaussian_flow_backward(const fdgs_flow_in* in, const float* dL_dflows, float scale, const fdgs_flow_grads* out, void* stream);

/* ---- contribution statistics: which Gaussians a finished forward actually used ----------------------------------------------------
 * One pass over the three scratch buffers of a forward on the same stream (any list layout: compact or sparse, tile_cull on or off,
 * num_rendered = -1 from a lazy forward; the forward's cull planes are not read).  Per pixel the tile list is walked front to back
 * with the forward blend's own decisions and arithmetic (skip power > 0 and alpha < 1/255; the entry that would take T below 1e-4
 * ends the pixel and does not contribute), so the contributions counted are exactly the rendered image's.  w = alpha * T.
 * pix_weight [H,W] or NULL (all ones): a pixel with weight <= 0 is skipped entirely -- it adds to no output and its ID is -1.
 * Outputs (any may be NULL, not all): ACCUMULATED in place -- the caller zero-fills them once, every further view adds / maxes into
 * them -- except dominant_id, which is overwritten:
 *   weight_sum [P]  += sum over pixels of pix_weight * w          (float atomic adds: the last bits depend on the arrival order)
 *   weight_max [P]   = max(weight_max, max over pixels of w)      (integer max on the float's bits, w >= 0: reproducible)
 *   hits [P]        += pixels the Gaussian contributed to         (reproducible)
 *   dominant [P]    += pixels whose largest-w contributor it is; on equal w the earliest list entry wins   (reproducible)
 *   dominant_id [H,W] = that Gaussian's index, -1 for a pixel without a contributor
 * One launch; at most one atomic request per (8x8 pixel block, Gaussian, output), none for a Gaussian that contributed to no pixel
 * of the block.  P == 0 (and num_rendered == 0): nothing is walked, dominant_id is filled with -1.
 * FDGS_ERR_INVALID_ARG before any launch: NULL in / out, a wrong struct_size, P < 0 or >= 2^26, W or H <= 0, every output NULL,
 * P > 0 with a NULL scratch buffer. */
typedef struct fdgs_contribution_in
{
	uint32_t struct_size;      /* sizeof(fdgs_contribution_in)                          */
	int32_t P, W, H;           /* as the forward's fdgs_scene                           */
	const void* geom_buffer;   /* the forward's three scratch buffers                   */
	const void* binning_buffer;
	const void* image_buffer;
	int32_t num_rendered;      /* as returned by the forward (-1: a lazy forward)       */
	const float* pix_weight;   /* [H,W] or NULL                                         */
} fdgs_contribution_in;
typedef struct fdgs_contribution_out
{
	uint32_t struct_size;      /* sizeof(fdgs_contribution_out)                         */
	float* weight_sum;         /* [P] or NULL                                           */
	float* weight_max;         /* [P] or NULL                                           */
	uint32_t* hits;            /* [P] or NULL                                           */
	uint32_t* dominant;        /* [P] or NULL                                           */
	int32_t* dominant_id;      /* [H,W] or NULL                                         */
} fdgs_contribution_out;
int fdgs_contribution(const fdgs_contribution_in* in, const fdgs_contribution_out* out, void* stream);

/* ---- feature channels: per-Gaussian data blended with the weights of a finished forward, and the adjoint ------------------------------
 * CALL ORDER: after the forward, on the same stream, with its three scratch buffers (any list layout: compact or sparse, tile_cull on
 * or off, num_rendered = -1 from a lazy forward; the forward's cull planes are not read) -- exactly as fdgs_contribution.  Per pixel
 * the tile list is walked front to back with the forward blend's own decisions and arithmetic (skip power > 0 and alpha < 1/255; the
 * entry that would take T below 1e-4 ends the pixel and does not contribute), so the weights w = alpha * T are the rendered image's.
 *   fdgs_feature_blend:           out[c, y, x] = sum over the pixel's contributions of w * features[id, c]
 *       features [P,C] float32, row-major, rows contiguous, finite; out [C,H,W] is OVERWRITTEN; a pixel without a contributor is
 *       exactly 0 and nothing is composited behind the features (the caller does that with the forward's alpha if it wants a
 *       background).  No atomics: bit-identical run to run, and the value of a channel does not depend on C or on the channels
 *       rendered with it.
 *   fdgs_feature_blend_backward:  dL_dfeatures[id, c] += sum over the pixels id contributes to of w * dL_dout[c, y, x]
 *       the adjoint of the above; dL_dfeatures [P,C] is ACCUMULATED in place -- the caller zero-fills it once, further views add to
 *       it -- with float atomic adds (the last bits depend on the arrival order): at most one request per (8x8 pixel block,
 *       Gaussian, channel), none for a Gaussian that contributed to no pixel of the block.  in->features is not read (NULL).
 * GEOMETRY IS HELD CONSTANT: w is a number here; no gradient reaches alpha, the positions or the covariances.
 * 1 <= C <= FDGS_FEATURE_MAX_CHANNELS, any C in that range.  P == 0 (and num_rendered == 0): the forward zero-fills out, the
 * backward does nothing.
 * FDGS_ERR_INVALID_ARG before any launch: NULL in / out / dL_dout / dL_dfeatures, a wrong struct_size, P < 0 or >= 2^26, W or H <= 0,
 * C outside [1, FDGS_FEATURE_MAX_CHANNELS], P > 0 with a NULL scratch buffer, NULL features in the forward. */
#define FDGS_FEATURE_MAX_CHANNELS 256
typedef struct fdgs_feature_in
{
	uint32_t struct_size;      /* sizeof(fdgs_feature_in)                               */
	int32_t P, W, H, C;        /* as the forward's fdgs_scene; C: feature channels      */
	const void* geom_buffer;   /* the forward's three scratch buffers                   */
	const void* binning_buffer;
	const void* image_buffer;
	int32_t num_rendered;      /* as returned by the forward (-1: a lazy forward)       */
	const float* features;     /* [P,C]; NULL for the backward                          */
} fdgs_feature_in;
int fdgs_feature_blend(const fdgs_feature_in* in, float* out /* [C,H,W] */, void* stream);
int fdgs_feature_blend_backward(const fdgs_feature_in* in, const float* dL_dout /* [C,H,W] */, float* dL_dfeatures /* [P,C], accumulated */,
                                void* stream);

/* ---- camera gradients: dL/d(viewmatrix, projmatrix, campos, timestamp) of one view --------------------------------------------------
 * The analytic derivatives of the forward with respect to the four camera inputs of fdgs_scene, every discrete decision held constant
 * (culls, radii, tile lists, n_contrib, the alpha and T cut-offs); not the reference backward's quirks: the camera is no parameter of
 * the reference.  36 sums over the P Gaussians:
 *   dL_dviewmatrix [16], laid out as fdgs_scene.viewmatrix: through the view-space mean t (EWA Jacobian, depth, 1 / tz) and through the
 *                        rotation block W of T = J W.  Entries 3, 7, 11, 15 (the column t does not read) are exactly zero.
 *   dL_dprojmatrix [16]: through p_hom.x, .y, .w into the pixel position.  Entries 2, 6, 10, 14 (the depth column) are exactly zero.
 *   dL_dcampos [3]:      through the SH view direction (from the input mean, as the forward takes it); zero with colors_precomp.
 *   dL_dtimestamp [1]:   through the temporal marginal, the conditional mean shift of rot_4d and the 4D-SH time factors; zero for
 *                        gaussian_dim == 3 (and for cov3D_precomp, where the forward applies neither marginal nor shift, without 4D SH).
 * CALL ORDER: fdgs_rasterize_backward(scene, in, out with stage_mask = 1) first, THIS call on the same stream with the same scene, in
 * and out->grad_accum, then fdgs_rasterize_backward(... stage_mask = 2): the per-Gaussian quantities it needs live in words 0-11 of the
 * accumulator records between those two calls only.  grad_accum is only READ here (also with grad_accum_clean: the geometry backward
 * still finds, and re-zeroes, what the blend backward left), so the per-Gaussian gradients are bit for bit what they are without this call.
 * Each result is scale * the sum, written, or with accumulate != 0 added to what the array holds.  Any output may be NULL, not all four.
 * scratch: fdgs_camera_backward_scratch(P) bytes of device memory the call may overwrite.  Two launches, no atomics: one lane per
 * Gaussian, fixed-order wave / block reduction to one row of partial sums per 256 Gaussians, summed in fixed order in double:
 * bitwise reproducible.  P == 0 or every Gaussian culled: zeros (accumulate: the arrays keep their contents).
 * FDGS_ERR_INVALID_ARG before any launch: a NULL scene / in / grads, a wrong struct_size, every output NULL, scratch NULL or
 * scratch_bytes too small, an invalid scene, P > 0 with a NULL radii / out_means3D / geom_buffer / grad_accum. */
typedef struct fdgs_camera_grads
{
	uint32_t struct_size;      /* sizeof(fdgs_camera_grads)                             */
	float* dL_dviewmatrix;     /* [16] or NULL                                          */
	float* dL_dprojmatrix;     /* [16] or NULL                                          */
	float* dL_dcampos;         /* [3]  or NULL                                          */
	float* dL_dtimestamp;      /* [1]  or NULL                                          */
	float scale;               /* multiplies every result                               */
	int32_t accumulate;        /* 0: overwrite, otherwise add to the arrays' contents   */
} fdgs_camera_grads;
size_t fdgs_camera_backward_scratch(int32_t P);
int fdgs_camera_backward(const fdgs_scene* scene, const fdgs_backward_in* in, const float* grad_accum, const fdgs_camera_grads* grads,
                         void* scratch, size_t scratch_bytes, void* stream);

/* ---- storing a trained model small: k-means codebooks, quantised columns and their decode (compress.hip) ---------------------------
 * k-means over rows x [N,D] with a codebook c [K,D], both row-major float in device memory; 1 <= D <= 192, 1 <= K <= 65536, N >= 1,
 * no multiple of any tile size is assumed.  scratch: fdgs_kmeans_scratch_bytes(N, K) bytes of device memory, shared by both calls.
 *
 * fdgs_kmeans_assign: index[n] = argmin_k |x_n - c_k|^2, ties to the lowest k.  The score compared is |c_k|^2 - 2 x_n . c_k in fp32: the
 * norm a d-ordered sum, the dot product the d-ordered fma chain of the f32-input MFMA (v_mfma_f32_32x32x2_f32); both depend on the values
 * of row k alone, so equal codebook rows score bit-identically and the tie rule is exact.  For every row the chosen centroid is within
 * 4 (D + 4) 2^-24 (|x_n|^2 + max_k |c_k|^2) of the nearest one in squared distance.  dist2 [N] or NULL: the winner's squared distance as
 * the direct sum of (x_d - c_d)^2.  No N x K intermediate touches memory: codebook tiles pass through LDS, the running best stays in
 * registers.
 *
 * fdgs_kmeans_update: c_k = sum_{index[n] = k} w_n x_n / sum w_n (w [N] or NULL: all ones), IN PLACE in c; a cluster without rows or
 * with a total weight of zero keeps its row bit for bit.  counts [K] or NULL: rows per cluster.  The (index, row) pairs go through the
 * stable radix sort and every cluster's rows are summed in ascending row id by one workgroup: no float atomics, bitwise reproducible.
 * An index outside [0, K) belongs to no cluster. */
size_t fdgs_kmeans_scratch_bytes(int32_t N, int32_t K);
int fdgs_kmeans_assign(int32_t N, int32_t K, int32_t D, const float* x, const float* c, int32_t* index, float* dist2, void* scratch,
                       void* stream);
int fdgs_kmeans_update(int32_t N, int32_t K, int32_t D, const float* x, const int32_t* index, const float* w, float* c, int32_t* counts,
                       void* scratch, void* stream);
/* q[p][col] = min(max(rintf((x[p][col] - lo[col]) * inv[col]), 0), qmax) for x [P,C]; lo / inv [C] in device memory; q is uint8 with
 * qmax = 255, uint16 with qmax = 65535 (no other value).  fp32, these IEEE operations in this order, no fused multiply-add. */
int fdgs_quantize_columns(int32_t P, int32_t C, const float* x, const float* lo, const float* inv, int32_t qmax, void* q, void* stream);
/* Row p of out [P, C + D]: first the C stored columns -- bits 8 / 16: lo[col] + (float)q[p][col] * step[col] (one product, one sum, no
 * fused multiply-add), bits 32: q holds floats, copied bit for bit -- then, with D > 0, row index[p] of rows [K,D] (index NULL: row p of
 * rows [P,D]; an index outside [0, K) is clamped into it).  That is a whole segment of a flat parameter bucket (D = 0), or a row of SH
 * coefficients in two parts: the DC triple, then its codebook row.  One launch; a lane produces four consecutive floats and stores them
 * as 16 bytes where out is 16-byte aligned and C + D a multiple of 4. */
int fdgs_compact_decode(int32_t P, int32_t C, int32_t bits, const void* q, const float* lo, const float* step, int32_t D, const float* rows,
                        const int32_t* index, int32_t K, float* out, void* stream);

/* ---- a model under a similarity transform: x' = s R x + T, t' = a t + b (model_transform.hip) -----------------------------------------
 * RAW parameters in (as fdgs_scene.raw_params = 1: scales / scales_t before exp, quaternions of any norm), raw parameters out; opacity is
 * not an argument: it does not change.  Two launches on `stream`, one lane per Gaussian for the geometry, one lane per 16-coefficient
 * block for the SH rows; no atomics, no scratch memory, P == 0: nothing is launched.
 *   means3D' = s * (R x) + T, the row of R times x summed left to right, ts' = a * t + b (fp32).
 *   gaussian_dim == 3, or 4 without rot_4d: rotations' = quat * rotations (Hamilton product, no renormalisation), scales' = scales +
 *     log_scale, and for gaussian_dim == 4 scales_t' = scales_t + 2 log_time_scale (exp(scales_t) is a VARIANCE there).
 *   rot_4d, scale == time_scale: rotations' = rotations * iso_v and rotations_r' = rotations_r * iso_u, the products of the left / right
 *     isoclinic families of build_Ml_Mr (M_r(iso_u) M_l(iso_v) = diag(R, 1)^T), scales' = scales + log_scale, scales_t' = scales_t +
 *     log_time_scale.  The products and sums are formed in double and rounded once.
 *   rot_4d, scale != time_scale: Sigma = R4^T S^2 R4 of the activated parameters, A Sigma A^T with A = diag(s R, a), a cyclic Jacobi on the
 *     symmetric 4x4, all in double; the eigenvector with the largest |time component| becomes axis 3 (scales_t), one eigenvector is
 *     negated where the determinant needs it, R4' is factored into unit (rotations', rotations_r') through its rank-1 coefficient
 *     matrix, and the logarithms of the square roots of the eigenvalues (floored at 1e-15) are stored.
 *   shs [P,M,3], M in {1, 4, 9, 16, 32, 48}: in every block of 16 coefficients the row holds, bands 1-3 are multiplied by the 3x3, 5x5,
 *     7x7 matrices of sh_rot (row-major, 83 entries; c' = D c, each sum pairwise in fp32 starting from +0) for all three channels;
 *     coefficient 0 of a block is copied bit for bit, a block of zeros stays zeros.  Skipped when `rotation` is the identity to 0 ulp
 *     (then the rows are copied unless out aliases in).  shs NULL (both): no SH pass.
 * A transform whose spatial part (or rotation, or time part) is the identity to 0 ulp copies what it would otherwise recompute: the
 * identity returns the input bit for bit on the first three paths.  quat, iso_u, iso_v, log_scale, log_time_scale and sh_rot are
 * functions of rotation / scale / time_scale that the caller computes in double (fdgs.edit); the library does not re-derive them.
 * Every pointer of `out` may alias its counterpart of `in` (in place); other overlaps are not allowed.  Segments the mode does not read
 * (ts / scales_t for gaussian_dim 3, rotations_r without rot_4d) may be NULL and are not written.
 * FDGS_ERR_INVALID_ARG before any launch: NULL in / out, a wrong struct_size, P < 0 or >= 2^26, P > 0 with a NULL required pointer, shs
 * given on one side only, M outside {1, 4, 9, 16, 32, 48} (also without shs), scale or time_scale not positive and finite, gaussian_dim
 * outside {3, 4}, rot_4d with gaussian_dim 3. */
typedef struct fdgs_transform_in
{
	uint32_t struct_size;     /* sizeof(fdgs_transform_in)                             */
	int32_t P;                /* number of Gaussians                                   */
	int32_t M;                /* SH coefficients per Gaussian                          */
	int32_t gaussian_dim, rot_4d;
	const float* means3D;     /* [P,3]                                                 */
	const float* ts;          /* [P]   gaussian_dim 4                                  */
	const float* scales;      /* [P,3] raw                                             */
	const float* scales_t;    /* [P]   raw, gaussian_dim 4                             */
	const float* rotations;   /* [P,4] raw                                             */
	const float* rotations_r; /* [P,4] raw, rot_4d                                     */
	const float* shs;         /* [P,M,3] or NULL                                       */
	double rotation[9];       /* R, row-major                                          */
	double translation[3];    /* T                                                     */
	double scale, time_scale, time_shift;   /* s > 0, a > 0, b                         */
	double quat[4];           /* unit (w,x,y,z) of R                                   */
	double iso_u[4], iso_v[4];/* M_r(iso_u) M_l(iso_v) = diag(R, 1)^T                  */
	double log_scale, log_time_scale;
	float sh_rot[83];         /* bands 1, 2, 3 of the SH rotation, row-major           */
} fdgs_transform_in;
typedef struct fdgs_transform_out
{
	uint32_t struct_size;     /* sizeof(fdgs_transform_out)                            */
	float* means3D;           /* the counterparts of fdgs_transform_in's tensors       */
	float* ts;
	float* scales;
	float* scales_t;
	float* rotations;
	float* rotations_r;
	float* shs;
} fdgs_transform_out;
int fdgs_model_transform(const fdgs_transform_in* in, const fdgs_transform_out* out, void* stream);

/* ---- depth supervision on the rendered depth map (csrc/depth_loss.hip) ---------------------------------------------------
 * The per-pixel depth and its validity, shared by the three calls below:
 *   z = depth / alpha where alpha >= alpha_min (alpha == NULL: z = depth and every pixel passes); a pixel is VALID if it passes
 *   that test, mask == NULL or mask > 0, and -- for fdgs_depth_loss -- the prior is finite and > 0.
 * Invalid pixels contribute nothing and receive exactly 0 gradient.  Gradients go to depth and alpha: dz/dD = 1 / A,
 * dz/dA = -D / A^2.  All on `stream`, no host synchronisation, no atomics: every output is bitwise reproducible.
 * FDGS_ERR_INVALID_ARG before any launch: a NULL struct or required pointer, a wrong struct_size, H or W <= 0, H * W >= 2^30,
 * H >= 16 * 65535, alpha given with alpha_min not positive and finite, d_alpha given without alpha, an unknown mode. */
typedef struct fdgs_depth_in
{
	uint32_t struct_size;     /* sizeof(fdgs_depth_in)                                 */
	int32_t H, W;
	const float* depth;       /* [H,W]  the forward's out_depth = sum z_i alpha_i T_i  */
	const float* alpha;       /* [H,W]  1 - T, or NULL                                 */
	const float* mask;        /* [H,W]  or NULL                                        */
	float alpha_min;          /* the alpha test's threshold (> 0 where alpha is given) */
} fdgs_depth_in;

typedef struct fdgs_depth_grads
{
	uint32_t struct_size;     /* sizeof(fdgs_depth_grads)                              */
	float* d_depth;           /* [H,W] or NULL: not computed                           */
	float* d_alpha;           /* [H,W] or NULL (needs fdgs_depth_in.alpha)             */
	const float* g_upstream;  /* one float of device memory, or NULL: 1                */
	float scale;              /* the gradient is scale * g_upstream * dL/d.            */
	int32_t accumulate;       /* 0: written to every one of the H * W elements; else added */
} fdgs_depth_grads;

#define FDGS_DEPTH_PEARSON 0  /* L = 1 - rho(z, prior) over the valid pixels                                                   */
#define FDGS_DEPTH_SSI 1      /* L = sum |s z + b - prior| / n with (s, b) the least-squares fit, constants for the gradient   */
/* The value in out[0], and with `grads` != NULL its gradient.  out: 4 floats of device memory { L, n, rho, 0 } (pearson) or
 * { L, n, s, b } (ssi).  partials: fdgs_depth_loss_num_partials(H, W) DOUBLES of device memory (the per-workgroup float64 moments
 * n, sum z, sum p, sum z^2, sum z p, sum p^2, the ssi residual sums and the finished statistics).  Degenerate inputs -- n < 2, or a
 * variance of z or of the prior at or below 1e-12 max(1, mean^2) -- give exactly L = 1 (pearson) or 0 (ssi) and an all-zero
 * gradient.  pearson: dL/dz_i = -((p_i - pm) - rho (sigma_p / sigma_z) (z_i - zm)) / (n sigma_z sigma_p); ssi: s sign(r_i) / n. */
int fdgs_depth_loss_num_partials(int32_t H, int32_t W);
int fdgs_depth_loss(const fdgs_depth_in* in, const float* prior, int32_t mode, const fdgs_depth_grads* grads, double* partials,
                    float* out, void* stream);
/* Normals from the depth: pixel centres at +0.5, P(u,v) = ((u+.5-cx)/fl_x z, (v+.5-cy)/fl_y z, z), a = P(u+1,v) - P(u-1,v),
 * b = P(u,v+1) - P(u,v-1), n = (b x a) / |b x a| (towards the camera: n_z < 0 on a fronto-parallel plane).  A normal is valid if
 * the pixel and its four neighbours are inside the image and valid and |b x a|^2 > 1e-20; otherwise n = 0 and valid = 0.
 * normals [3,H,W], valid [H,W] bytes.  viewmatrix != NULL (16 floats of device memory, world_view_transform as the rasterizer
 * takes it): the normal is rotated to world space.  The backward maps dL_dnormals [3,H,W] to d_depth / d_alpha of `grads` as a
 * gather over the four neighbouring normals of every pixel. */
int fdgs_depth_normals(const fdgs_depth_in* in, float fl_x, float fl_y, float cx, float cy, const float* viewmatrix, float* normals,
                       uint8_t* valid, void* stream);
int fdgs_depth_normals_backward(const fdgs_depth_in* in, float fl_x, float fl_y, float cx, float cy, const float* viewmatrix,
                                const float* dL_dnormals, const fdgs_depth_grads* grads, void* stream);

/* ---- a surface from depth maps: TSDF fusion and surface nets (csrc/tsdf.hip) ------------------------------------------------
 * The volume: nx x ny x nz voxels of edge voxel_size; voxel (i, j, k) has its centre at origin + (i + .5, j + .5, k + .5) voxel_size.
 * float32 arrays, x fastest: tsdf [nz,ny,nx], weight [nz,ny,nx], and optionally color [3,nz,ny,nx] with cweight [nz,ny,nx].  A fresh
 * volume is all zeros (weight 0: never seen); resetting it is a memset.  tsdf holds the distance in units of `trunc`, in [-1, 1].
 * FDGS_ERR_INVALID_ARG before any launch (all three calls): a NULL or mis-sized struct, NULL tsdf / weight, a negative size,
 * nx ny nz >= 2^28, voxel_size or trunc not positive and finite, a non-finite origin, color and cweight not given together. */
typedef struct fdgs_tsdf_volume
{
	uint32_t struct_size;     /* sizeof(fdgs_tsdf_volume)                              */
	int32_t nx, ny, nz;
	float origin[3];          /* the corner of voxel (0, 0, 0)                         */
	float voxel_size;         /* s > 0                                                 */
	float trunc;              /* truncation distance > 0                               */
	float* tsdf;
	float* weight;
	float* color;             /* or NULL                                               */
	float* cweight;           /* with color                                            */
} fdgs_tsdf_volume;

typedef struct fdgs_tsdf_view
{
	uint32_t struct_size;     /* sizeof(fdgs_tsdf_view)                                */
	int32_t H, W;
	const float* depth;       /* [H,W]  the forward's out_depth                        */
	const float* alpha;       /* [H,W]  or NULL: the pixel depth is `depth` itself     */
	const float* mask;        /* [H,W]  or NULL                                        */
	const float* image;       /* [3,H,W] or NULL: this view carries no colour          */
	const float* viewmatrix;  /* 16 floats of device memory, as fdgs_depth_normals takes it */
	float alpha_min;          /* > 0 where alpha is given                              */
	float fl_x, fl_y, cx, cy; /* pixel (i, j) covers [i, i + 1) x [j, j + 1)           */
	float view_weight;        /* w > 0                                                 */
} fdgs_tsdf_view;

/* Applies `views[0 .. num_views)` in ascending order to every voxel centre c:
 *   (x, y, z) = c in view space; skip the view if z <= 0.2 (the rasterizer's near plane);
 *   u = fl_x x / z + cx, v = fl_y y / z + cy, the pixel is (floor(u), floor(v)); skip if it is outside the image;
 *   skip unless alpha >= alpha_min and mask > 0 there (each where given); zp = depth / alpha (or depth); skip unless 0 < zp < inf;
 *   sdf = zp - z; skip if sdf < -trunc; d = min(1, sdf / trunc);
 *   tsdf = (weight tsdf + w d) / (weight + w), weight += w;   and, where the volume has colour, the view an image and d < 1, the same
 *   running mean of the pixel's colour with cweight.
 * One thread owns a voxel, no atomics; up to 16 views are applied per pass over the volume with the voxel in registers, and the
 * result is bit-identical to one call per view.  A voxel no view reaches is not written.  Further INVALID_ARG: num_views < 0,
 * NULL views with num_views > 0, and per view a wrong struct_size, H or W <= 0, H W >= 2^30, NULL depth or viewmatrix, alpha with
 * alpha_min not positive and finite, fl_x / fl_y not positive and finite, cx / cy not finite, view_weight not positive and finite. */
int fdgs_tsdf_integrate(const fdgs_tsdf_volume* volume, int32_t num_views, const fdgs_tsdf_view* views, void* stream);

typedef struct fdgs_surface_out
{
	uint32_t struct_size;     /* sizeof(fdgs_surface_out)                              */
	int32_t vertex_capacity;  /* rows of vertices / normals / colors                   */
	int32_t face_capacity;    /* rows of faces                                         */
	float* vertices;          /* [vertex_capacity,3] or NULL                           */
	float* normals;           /* [vertex_capacity,3] or NULL                           */
	float* colors;            /* [vertex_capacity,3] or NULL (0 without volume colour) */
	int32_t* faces;           /* [face_capacity,3] vertex indices, or NULL             */
	int32_t* n_vertices;      /* one int32 of device memory: always the full count     */
	int32_t* n_faces;         /* likewise, in triangles                                */
} fdgs_surface_out;

/* Surface nets.  Cells are the (nx-1)(ny-1)(nz-1) cubes whose corners are voxel centres; a corner is KNOWN if weight >= min_weight
 * and weight > 0, INSIDE if tsdf < 0; a cell is ACTIVE if all eight corners are known and not all on one side.  One vertex per active
 * cell in ascending cell index (x fastest): the mean of the linear crossing points t = a / (a - b) of the cell's sign-changing edges,
 * the mean of the corner colours interpolated at them, and the normalised trilinear gradient of tsdf at the cell centre (0 where its
 * squared length is <= 1e-20).  One quad -- triangles (c0, c1, c2), (c0, c2, c3) -- per grid edge (from voxel index e along axis a)
 * whose two ends are known and differ in sign and whose four surrounding cells exist and are active, in ascending 3 e + a, wound so
 * that the geometric normal points from the inside end to the outside end.
 * With vertices, normals, colors and faces all NULL the call only counts; otherwise rows below the capacities are written and the
 * counts are still the full ones.  scratch: fdgs_surface_extract_scratch_bytes(nx, ny, nz) bytes (a cell-to-vertex int32 map and
 * per-workgroup counts).  A volume with a dimension < 2 gives 0 and 0 without a kernel.  Further INVALID_ARG: NULL out / n_vertices /
 * n_faces / scratch, a wrong struct_size, negative capacities, a min_weight that is NaN. */
size_t fdgs_surface_extract_scratch_bytes(int32_t nx, int32_t ny, int32_t nz);
int fdgs_surface_extract(const fdgs_tsdf_volume* volume, float min_weight, const fdgs_surface_out* out, void* scratch, void* stream);

/* ---- cleaning and smoothing a triangle mesh (csrc/mesh.hip) ------------------------------------------------------------------
 * A mesh is what fdgs_surface_extract leaves on the device: vertices, normals, colors [V,3] float32 and faces [F,3] int32, with
 * 0 <= V, F < 2^28.  A face with any index outside [0, V) is ABSENT: no call reads or writes through it, it joins nothing, it
 * contributes to no sum and compaction drops it.  A face with repeated indices is an ordinary face.  Every integer result is a
 * function of the input, bit for bit.  FDGS_ERR_INVALID_ARG before any launch (all three calls): a NULL or mis-sized struct, a
 * negative count or capacity, V or F >= 2^28, NULL faces with F > 0, a NULL required output or scratch (each where its count is not
 * zero).  Each *_scratch_bytes(V, F) is a multiple of 256, and 0 for a negative (or too large) argument. */
typedef struct fdgs_mesh_in
{
	uint32_t struct_size;     /* sizeof(fdgs_mesh_in)                                  */
	int32_t V, F;
	const float* vertices;    /* [V,3] or NULL where the call does not need it         */
	const float* normals;     /* [V,3] or NULL                                         */
	const float* colors;      /* [V,3] or NULL                                         */
	const int32_t* faces;     /* [F,3]                                                 */
} fdgs_mesh_in;

typedef struct fdgs_mesh_components_out
{
	uint32_t struct_size;         /* sizeof(fdgs_mesh_components_out)                  */
	int32_t capacity;             /* rows of component_vertices / component_faces      */
	int32_t labelled;             /* != 0: vertex_component already holds an earlier call's ids for this mesh; only the two count
	                                 arrays are written (n_components and scratch are not used, nothing synchronises)           */
	int32_t* vertex_component;    /* [V] dense component id of every vertex            */
	int32_t* n_components;        /* one int32 of device memory: always the full count */
	int32_t* component_vertices;  /* [capacity] or NULL                                */
	int32_t* component_faces;     /* [capacity] or NULL                                */
	int32_t* rounds;              /* HOST memory or NULL: hook passes the call took    */
} fdgs_mesh_components_out;

/* Connected components of the graph whose nodes are the V vertices and whose edges are the sides of the present faces.
 * vertex_component: ids 0 .. C-1 in ascending order of each component's smallest vertex index (a vertex in no present face is a
 * component of its own, with zero faces); a face is counted for the component of its first index.  Rows of the two count arrays at
 * or beyond `capacity` are never written; *n_components is always C.
 * A lock-free union-find: every face links its corners by a compare-and-swap of the larger root onto the smaller (a failed swap
 * means another thread lowered that root: the retry starts from a strictly smaller index, no thread waits for another), then every
 * vertex reads its root -- the component's smallest index, whatever the schedule.  A second hook pass that finds every face's
 * corners under one root is the convergence check: the host reads one device flag per pass (THE CALL SYNCHRONISES `stream`); more
 * than 32 passes give FDGS_ERR_HIP.  Dense ids by a flag scan of the roots, counts by integer atomics: exact.
 * scratch: fdgs_mesh_components_scratch_bytes(V, F) bytes. */
size_t fdgs_mesh_components_scratch_bytes(int32_t V, int32_t F);
int fdgs_mesh_components(const fdgs_mesh_in* mesh, const fdgs_mesh_components_out* out, void* scratch, void* stream);

/* Keeps the components c with keep[c] != 0 (keep: n_components bytes of device memory; an id outside [0, n_components) is not
 * kept): a vertex survives if its component is kept, a face if it is present and its first vertex's component is kept; survivors
 * keep their relative order, faces are renumbered through the old-to-new vertex map (-1 for a dropped vertex, which only a
 * vertex_component that contradicts the faces can produce), attribute rows are copied unchanged.  `out` as fdgs_surface_extract
 * takes it: with all four arrays NULL the call only counts, otherwise rows below the capacities are written and the counts are the
 * full ones.  An output array needs its input array.  No host synchronisation.  Further INVALID_ARG: NULL vertex_component with
 * V > 0, NULL keep with n_components > 0, n_components < 0, NULL n_vertices / n_faces. */
size_t fdgs_mesh_compact_scratch_bytes(int32_t V, int32_t F);
int fdgs_mesh_compact(const fdgs_mesh_in* mesh, const int32_t* vertex_component, const uint8_t* keep, int32_t n_components,
                      const fdgs_surface_out* out, void* scratch, void* stream);

typedef struct fdgs_mesh_smooth_out
{
	uint32_t struct_size;     /* sizeof(fdgs_mesh_smooth_out)                          */
	int32_t iterations;       /* >= 0                                                  */
	float lambda, mu;         /* not NaN                                               */
	int32_t pin_boundary;
	float* vertices;          /* [V,3] the smoothed positions (NULL allowed with iterations == 0) */
	float* normals;           /* [V,3] or NULL                                         */
	uint8_t* boundary;        /* [V] 1 for a boundary vertex, or NULL                  */
} fdgs_mesh_smooth_out;

/* Taubin smoothing.  The incidences (vertex, 3 face + corner) of the present faces' corners are sorted by vertex with the
 * library's stable radix sort, so a vertex's row is in ascending 3 face + corner.  For an incidence with corner k of face f, its
 * OTHER corners (o1, o2) are the face's remaining two in ascending corner index.  One pass with factor t, in float32 exactly as
 * written (built with FP contraction off), n = the length of v's row:
 *   S = 0;  for the row in order: S = S + (p[o1] + p[o2]);   m = S / (float)(2 n);   p'(v) = p(v) + t * (m - p(v))
 * per component; n == 0 or a pinned vertex: p'(v) = p(v).  An iteration is a pass with t = lambda, then one with t = mu, each from
 * the previous pass's positions.  v is a BOUNDARY vertex if some index occurs among the other corners of exactly one incidence of
 * its row (an integer decision on the topology, taken once; the cost is quadratic in the row length); with pin_boundary != 0 such
 * vertices never move.  normals: N(v) = sum over the row in order of cross(p[b] - p[a], p[c] - p[a]) of the incidence's face
 * (a, b, c), cross = (u.y w.z - u.z w.y, u.z w.x - u.x w.z, u.x w.y - u.y w.x), from the final positions, divided by
 * sqrt((N.x^2 + N.y^2) + N.z^2) where that is > 0, else (0, 0, 0).  iterations == 0 copies the positions (where `vertices` is given
 * and is not the input) and recomputes normals.  Colours are not touched.  No float atomics, no host synchronisation.
 * Further INVALID_ARG: NULL mesh vertices with V > 0, NULL out vertices with iterations > 0, negative iterations, NaN lambda / mu. */
size_t fdgs_mesh_smooth_scratch_bytes(int32_t V, int32_t F);
int fdgs_mesh_smooth(const fdgs_mesh_in* mesh, const fdgs_mesh_smooth_out* out, void* scratch, void* stream);

/* ---- simplifying a triangle mesh: vertex clustering with quadric placement (csrc/mesh_simplify.hip) ---------------------------- */
#define FDGS_SIMPLIFY_MEAN 0
#define FDGS_SIMPLIFY_QUADRIC 1

typedef struct fdgs_mesh_simplify_params
{
	uint32_t struct_size;     /* sizeof(fdgs_mesh_simplify_params)                     */
	int32_t nx, ny, nz;       /* the grid: >= 1 each, nx ny nz <= 2^30                 */
	float origin[3];          /* finite                                                */
	float cell;               /* the cell edge h: positive and finite                  */
	int32_t placement;        /* FDGS_SIMPLIFY_MEAN or FDGS_SIMPLIFY_QUADRIC           */
	float stabilise;          /* >= 0 (1e-3 is a good value)                           */
	int32_t* vertex_map;      /* [V] the cluster of every input vertex, -1 for none; or NULL */
} fdgs_mesh_simplify_params;

/* All vertices that fall into one cell of the grid become one vertex; faces are mapped through that and the degenerate and repeated
 * ones dropped.  All arithmetic is float32 exactly as written (built with FP contraction off) unless stated otherwise.
 * 1. Cell of a vertex p: per axis f = floorf((p - origin) / h) (IEEE division), i = n - 1 where f >= n, else (int)f where f > 0, else 0
 *    (vertices outside the grid go to its border cells); cell = (k ny + j) nx + i.  A vertex with a non-finite coordinate has no
 *    cell: it joins no cluster and a face that uses it is dropped.  Every other vertex takes part, whether a face refers to it or not.
 * 2. Clusters: the pairs (cell, vertex) sorted by cell with the library's stable radix sort (vertices without a cell carry the key
 *    nx ny nz and end up behind every row).  A cluster is a row: its members are in ascending vertex index.  Clusters are numbered in
 *    ascending cell id by a flag scan; vertex_map[v] is that number, or -1.  The clusters are the output vertices.
 * 3. Attributes of a cluster with n members, every sum S = S + term along the row in order: centre = origin + ((float)i + 0.5f) h per
 *    axis; mean position m = S / (float)n of u = (p - centre) / h (cell units); colour = S / (float)n of the colours; normal = S of the
 *    normals divided by sqrt((S.x^2 + S.y^2) + S.z^2) where that is > 0, else (0, 0, 0).
 * 4. Position = centre + h * clamp(x) per axis, clamp(x) = fmin(fmax(x, -0.5), 0.5).  FDGS_SIMPLIFY_MEAN: x = m.
 *    FDGS_SIMPLIFY_QUADRIC: the incidences (cluster, 3 face + corner) of the corners of present faces whose vertex has a cell are
 *    sorted by cluster (stable: a row is in ascending 3 face + corner).  A face contributes once per corner -- three times to a
 *    cluster that holds all three, which is the sum of per-vertex quadrics.  Per incidence, with the face's corners in the receiving
 *    cell's units a' = (a - centre) / h, b', c':  n = cross(b' - a', c' - a') (as fdgs_mesh_smooth writes it),
 *    l = sqrtf((n.x^2 + n.y^2) + n.z^2), d = -((n.x a'.x + n.y a'.y) + n.z a'.z); where l > 0 and l and d are finite, in FLOAT64 and
 *    with n, l, d converted first: A += (n_i n_j) / l (six numbers), b += (n_i d) / l (three).  (The tenth number of the quadric,
 *    d^2 / l, enters no result and is not summed.)  Then, all in float64: t = (A00 + A11) + A22; t == 0: x = m; else
 *    lambda = ((double)stabilise t) / 3, M = A + lambda I, r = lambda m - b, and x = adj(M) r / det(M) by Cramer's rule:
 *      c00 = M11 M22 - M12 M12, c01 = M02 M12 - M01 M22, c02 = M01 M12 - M02 M11, c11 = M00 M22 - M02 M02, c12 = M01 M02 - M00 M12,
 *      c22 = M00 M11 - M01 M01, det = (M00 c00 + M01 c01) + M02 c02, x_0 = ((c00 r0 + c01 r1) + c02 r2) / det, likewise x_1 (c01,
 *      c11, c12) and x_2 (c02, c12, c22); x = m unless det > 0 (M is positive definite with stabilise > 0; only stabilise = 0 on a
 *      rank-deficient A gets there).
 *    x is clamped in float64 and rounded to float32.  The clamp is continuous: the vertex never leaves its cell.
 * 5. Faces: a present face survives if none of its corners maps to -1, the three mapped indices are pairwise different, and it is
 *    the lowest-indexed input face among those with its canonical triple -- the mapped triple rotated so that its smallest index
 *    comes first.  Orientation is kept: two faces of opposite winding on the same three clusters are different and BOTH survive.
 *    (Found by three stable sorts of the face indices, by the triple's third, second and first index.)  Survivors are emitted in
 *    ascending input face index, as the mapped triple without rotation.
 * `out` as fdgs_surface_extract and fdgs_mesh_compact take it: *n_vertices and *n_faces are always the full counts, rows at or beyond
 * a capacity are never written, and with vertices, normals, colors and faces all NULL the call stops after counting.  vertex_map is
 * written in either mode.  No atomics of any kind: the result is a function of the input, bit for bit.  No host synchronisation.
 * One lane sums a cluster's row: the time of a call grows with its largest cluster.
 * FDGS_ERR_INVALID_ARG before any launch: a NULL or mis-sized struct (mesh, params, out), cell not positive and finite, a non-finite
 * origin, a dimension < 1 or nx ny nz > 2^30, V or F >= 2^28, negative capacities, NaN or negative stabilise, a placement other
 * than 0 or 1, NULL vertices with V > 0, NULL faces with F > 0, an output normals / colors array whose input array is NULL, NULL
 * n_vertices / n_faces, NULL scratch with V > 0.  scratch: fdgs_mesh_simplify_scratch_bytes(V, F) bytes, a multiple of 256; 0 for
 * arguments out of range. */
size_t fdgs_mesh_simplify_scratch_bytes(int32_t V, int32_t F);
int fdgs_mesh_simplify(const fdgs_mesh_in* mesh, const fdgs_mesh_simplify_params* params, const fdgs_surface_out* out, void* scratch,
                       void* stream);

/* Thread-local description of the last error on this thread ("" if none).  Every non-zero return of an entry point writes its
 * own message first: the text belongs to the calling thread's most recent non-zero return.  After a call that returned FDGS_OK it
 * is unspecified (an earlier failure's text may still be there). */
const char* fdgs_last_error(void);
int fdgs_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FDGS_H */
