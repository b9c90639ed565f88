"""The environment map behind the Gaussians (the reference's ``pipe.env_map_res``, gaussian_renderer/__init__.py:165-177,
train.py:71-77, 250-252), on the GPU (csrc/envmap.hip).

* ``env_composite(colour, alpha, env_map, cam)`` -- ``colour + (1 - alpha) * env(ray)``, the environment looked up where the pixel's
  ray leaves the sphere of radius 60 about the origin; one kernel forward, one backward (gradients to colour, alpha and the map).
  The rays come from the camera's ``fl_x / fl_y / cx / cy / world_view_transform / camera_center`` (scene/cameras.py:75-82).
* ``EnvMapAdam`` -- the map's own Adam (``torch.optim.Adam(lr=feature_lr, eps=1e-15)`` of train.py:73): its gradient buffer, both
  moments and its step count; one ``fdgs_adam_step`` launch per step.
* ``composite_`` / ``composite_backward`` -- the raw launches on the current stream (StepPipeline).

One deliberate difference: the ray and texture coordinates are computed in float64, v as atan2(sqrt(x^2 + y^2), z), i.e. the
reference's acos(z / R) with z / R clamped to [-1, 1] (fp32 reaches 1.0000001 looking at the pole, where the reference produces NaN).
There is no CPU path.
"""
import weakref

import torch

from . import _capi

ENV_RADIUS = 60.0   # gaussian_renderer/__init__.py:167

_INSIDE = {}   # id(camera_center) -> (weak reference, version, radius) of a camera found inside the sphere


def check_camera(cam, radius: float = ENV_RADIUS):
    """The reference asserts delta > 0 for every ray, i.e. that the camera sits inside the sphere: checked once per camera-centre
    tensor (one host read) and remembered, so that a training step does not wait for the device.  Raises ValueError."""
    c = cam.camera_center
    key = id(c)
    hit = _INSIDE.get(key)
    if hit is not None and hit[0]() is c and hit[1] == c._version and hit[2] == float(radius):
        return
    r = float(c.detach().double().norm())
    if not r < float(radius):
        raise ValueError("fdgs: the environment map needs the camera inside its sphere (|camera_center| = %g, radius %g)" % (r, radius))
    _INSIDE[key] = (weakref.ref(c, lambda _r, k=key: _INSIDE.pop(k, None)), c._version, float(radius))


def _cam_args(cam, dev):
    vm = cam.world_view_transform.detach().to(dev, torch.float32).contiguous()
    cp = cam.camera_center.detach().to(dev, torch.float32).contiguous()
    return vm, cp, float(cam.fl_x), float(cam.fl_y), float(cam.cx), float(cam.cy)


def _check_env(env_map):
    if env_map is None:
        raise ValueError("fdgs: pipe.env_map_res > 0 needs the model's env_map [3, R, R]")
    if env_map.dim() != 3 or env_map.shape[0] != 3 or env_map.dtype != torch.float32 or not env_map.is_contiguous() or not env_map.is_cuda:
        raise ValueError("fdgs: env_map must be a contiguous float32 GPU tensor [3, H, W]; got %s %s on %s"
                         % (tuple(env_map.shape), env_map.dtype, env_map.device))


def composite_(colour, T, env_map, cam, radius: float = ENV_RADIUS, out=None):
    """colour [3, H, W] + T [.., H, W] * env(ray) into ``out`` (default: in place into ``colour``) on the current stream."""
    _check_env(env_map)
    check_camera(cam, radius)
    H, W, dev = int(colour.shape[-2]), int(colour.shape[-1]), colour.device
    out = colour if out is None else out
    vm, cp, fx, fy, cx, cy = _cam_args(cam, dev)
    _capi.call("fdgs_env_composite", dev, H, W, vm.data_ptr(), cp.data_ptr(), fx, fy, cx, cy, env_map.data_ptr(), int(env_map.shape[1]),
               int(env_map.shape[2]), float(radius), T.data_ptr(), colour.data_ptr(), out.data_ptr())
    return out


def composite_backward(T, g_colour, env_map, cam, g_alpha=None, accumulate_alpha=False, g_env=None, accumulate_env=False,
                       radius: float = ENV_RADIUS):
    """d / d alpha into ``g_alpha`` [.., H, W] and d / d env into ``g_env`` [3, eh, ew] (written, or added with accumulate_*; None:
    not computed) on the current stream."""
    _check_env(env_map)
    H, W, dev = int(g_colour.shape[-2]), int(g_colour.shape[-1]), g_colour.device
    vm, cp, fx, fy, cx, cy = _cam_args(cam, dev)
    _capi.call("fdgs_env_composite_backward", dev, H, W, vm.data_ptr(), cp.data_ptr(), fx, fy, cx, cy, env_map.data_ptr(),
               int(env_map.shape[1]), int(env_map.shape[2]), float(radius), T.data_ptr(), g_colour.data_ptr(),
               None if g_alpha is None else g_alpha.data_ptr(), int(bool(accumulate_alpha)), None if g_env is None else g_env.data_ptr(),
               int(bool(accumulate_env)))


class _EnvComposite(torch.autograd.Function):
    @staticmethod
    def forward(ctx, colour, alpha, env_map, cam, radius):
        if not colour.is_cuda or not alpha.is_cuda:
            raise RuntimeError("fdgs: env_composite needs GPU tensors; there is no CPU path")
        c = colour.detach().contiguous().float()
        T = (1 - alpha.detach().float()).contiguous()
        env = env_map.detach()
        out = composite_(c, T, env, cam, radius, out=torch.empty_like(c))
        ctx.save_for_backward(T, env)
        ctx.cam, ctx.radius, ctx.alpha_shape = cam, float(radius), alpha.shape
        return out

    @staticmethod
    def backward(ctx, g):
        T, env = ctx.saved_tensors
        g = g.contiguous().float()
        need_a, need_e = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        g_alpha = torch.empty(ctx.alpha_shape, dtype=torch.float32, device=g.device) if need_a else None
        g_env = torch.empty_like(env) if need_e else None
        if need_a or need_e:
            composite_backward(T, g, env, ctx.cam, g_alpha, False, g_env, False, ctx.radius)
        return g, g_alpha, g_env, None, None


def env_composite(colour: torch.Tensor, alpha: torch.Tensor, env_map: torch.Tensor, cam, radius: float = ENV_RADIUS) -> torch.Tensor:
    """``colour + (1 - alpha) * env(ray)`` (gaussian_renderer/__init__.py:165-177): colour [3, H, W] rendered over black, alpha
    [1, H, W] = 1 - T, env_map [3, eh, ew].  Differentiable in all three.  Raises ValueError if the camera is outside the sphere."""
    return _EnvComposite.apply(colour, alpha, env_map, cam, float(radius))


class EnvMapAdam:
    """``torch.optim.Adam([env_map], lr, eps=1e-15)`` (train.py:73) over the map's own buffers: ``grad`` (what step() reads; also
    bound as ``env_map.grad``, so that autograd accumulates into it), ``exp_avg``, ``exp_avg_sq`` and ``step_count``.
    step() runs on the current stream."""

    def __init__(self, env_map: torch.Tensor, lr: float = 2.5e-3, eps: float = 1e-15, betas=(0.9, 0.999)):
        _check_env(env_map)
        self.env_map, self.lr, self.eps, self.betas = env_map, float(lr), float(eps), (float(betas[0]), float(betas[1]))
        self.grad = torch.zeros_like(env_map.detach())
        self.exp_avg = torch.zeros_like(self.grad)
        self.exp_avg_sq = torch.zeros_like(self.grad)
        self.step_count = 0
        if env_map.requires_grad:
            env_map.grad = self.grad

    def zero_grad(self):
        self.grad.zero_()

    def step(self):
        p = self.env_map.detach()
        self.step_count += 1
        n = p.numel()
        seg = (_capi.FdgsAdamSegment * 1)(_capi.FdgsAdamSegment(0, n, self.lr, self.lr, 0, 0))
        _capi.call("fdgs_adam_step", p.device, p.data_ptr(), self.grad.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), n, seg, 1,
                   self.betas[0], self.betas[1], self.eps, self.step_count)
