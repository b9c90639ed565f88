"""Inputs of tests/test_gpu_mcmc.py: small random models in the three modes, and the opacity patterns of the sampling tests."""
import numpy as np
import torch

MODES = {"3d": (3, False), "4d": (4, False), "rot4d": (4, True)}
SAMPLE_SIZES = (1, 2, 63, 64, 65, 1000, 5000)      # one lane, one wave +- 1, several workgroups (256 rows each), the scan's second level


def logit(o):
    o = np.asarray(o, np.float64)
    return np.log(o / (1.0 - o))


def raw_model(P, mode, M=16, seed=0, opacity=None, scale_range=(-6.0, 2.0)):
    """Raw float32 tensors (CPU) of P Gaussians: quaternions of any norm (e^-3 .. e^3), log-scales uniform in ``scale_range`` per axis,
    opacities uniform in (0.01, 0.99) unless given (activated values)."""
    rng = np.random.default_rng(seed)
    if opacity is None:
        opacity = rng.uniform(0.01, 0.99, P)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))  # noqa: E731
    quat = lambda: rng.normal(size=(P, 4)) * np.exp(rng.uniform(-3, 3, (P, 1)))  # noqa: E731
    return {"_xyz": f(rng.normal(size=(P, 3))), "_opacity": f(logit(opacity).reshape(P, 1)), "_scaling": f(rng.uniform(*scale_range, (P, 3))),
            "_rotation": f(quat()), "_t": f(rng.uniform(0, 1, (P, 1))), "_scaling_t": f(rng.uniform(*scale_range, (P, 1))),
            "_rotation_r": f(quat()), "_features": f(rng.normal(size=(P, M, 3)))}


def make_model(dev, P, mode, M=16, seed=0, opacity=None, scale_range=(-6.0, 2.0), moments=True):
    """(GaussianParams, FlatAdam with non-zero moments) on ``dev``."""
    from fdgs import train_host
    dim, rot = MODES[mode]
    model = train_host.GaussianParams.from_raw(raw_model(P, mode, M, seed, opacity, scale_range), dev, max_sh_degree=3, gaussian_dim=dim, rot_4d=rot)
    opt = train_host.make_optimizer(model)
    if moments:
        g = torch.Generator(device="cpu").manual_seed(seed + 1)
        opt.exp_avg.copy_(torch.randn(opt.exp_avg.shape, generator=g))
        opt.exp_avg_sq.copy_(torch.rand(opt.exp_avg_sq.shape, generator=g) + 0.1)
    return model, opt


def as_numpy(model):
    out = {n: p.detach().cpu().numpy().copy() for n, p in model.params.items()}
    out["gaussian_dim"], out["rot_4d"] = model.gaussian_dim, model.rot_4d
    return out


def opacity_patterns(P, seed=0):
    """name -> (activated opacities [P], min_opacity)."""
    rng = np.random.default_rng(seed)
    out = {"uniform": (rng.uniform(0.0, 1.0, P).clip(1e-4, 1 - 1e-6), 0.005),
           "near-one": (1.0 - rng.uniform(2.0 ** -23, 2.0 ** -10, P), 0.005)}
    out["uniform"][0][0] = 0.5          # (at least one alive, whatever P)
    lone = np.full(P, 0.001)
    lone[P // 2] = 0.3
    out["one-alive"] = (lone, 0.005)
    # weights from 1 to 2^24 units: alive is o > 0, so the smallest weights survive
    span = 2.0 ** -rng.uniform(0.0, 24.0, P)
    span[0], span[-1] = 2.0 ** -24, 1.0 - 2.0 ** -24
    out["span-2^24"] = (span.clip(2.0 ** -24, 1.0 - 2.0 ** -24), 0.0)
    return out
