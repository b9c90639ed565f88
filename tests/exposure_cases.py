"""The shared cases of the exposure tests: image shapes, inputs and table rows (float32, made once per process)."""
import functools
import os
import re

import numpy as np

import exposure_oracle as eo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _define(name):
    with open(os.path.join(ROOT, "include", "fdgs_exposure.h")) as f:
        return int(re.search(r"#define %s (\d+)" % name, f.read()).group(1))


BLOCK = _define("FDGS_EXPOSURE_BLOCK_PIXELS")     # the pixels of one workgroup's pass
# 1 x 1, one short row, a tiny odd image, odd W (one pixel per access), a multiple of 4 (float4 accesses, exactly four workgroups), and
# three rows that cross several workgroups and end in the middle of one: 2 BLOCK + 1 wide (scalar) and 2 BLOCK + 4 wide (float4)
SHAPES = [(1, 1), (1, 63), (3, 5), (17, 65), (64, 64), (3, 2 * BLOCK + 1), (3, 2 * BLOCK + 4)]
INPUTS = ("noise", "constant", "wild")
ROWS = ("identity", "random", "offset100")
FIT_SHAPES = [s for s in SHAPES if s[0] * s[1] >= 15]     # fewer pixels do not determine 12 numbers
COND_MAX = 1e4


def shape_id(s):
    return "%dx%d" % s


@functools.lru_cache(maxsize=None)
def image(kind, shape, seed=0):
    """float32 [3, H, W]: uniform noise in [0, 1); one constant per channel; values far outside [0, 1], half of them negative."""
    H, W = shape
    rng = np.random.default_rng([seed, H, W, INPUTS.index(kind)])
    if kind == "noise":
        x = rng.random((3, H, W))
    elif kind == "constant":
        x = np.broadcast_to(np.array([0.25, 0.5, 0.75])[:, None, None], (3, H, W))
    else:
        x = rng.normal(0.0, 3.0, (3, H, W))
    x = np.ascontiguousarray(x, np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def upstream(shape, seed=1):
    """float32 [3, H, W] upstream gradient of both signs, of a loss gradient's size."""
    H, W = shape
    x = np.ascontiguousarray(np.random.default_rng([seed, H, W]).normal(0.0, 1e-3, (3, H, W)), np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def row(kind, seed=2):
    """float32 [12]: the identity; a random transform near it; the same with an offset of 100."""
    rng = np.random.default_rng([seed, ROWS.index(kind)])
    if kind == "identity":
        A = eo.IDENTITY.copy()
    else:
        A = (np.eye(3, 4) + np.concatenate([rng.normal(0.0, 0.3, (3, 3)), rng.normal(0.0, 0.1, (3, 1))], axis=1)).reshape(12)
        if kind == "offset100":
            A[3::4] = 100.0
    A = np.ascontiguousarray(A, np.float32)
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def fit_pair(shape):
    """(render, ground truth) of a fit: noise, and a random transform of it plus a little noise of its own."""
    H, W = shape
    c = image("noise", shape, seed=5)
    gt = eo.apply(c, row("random", seed=6)) + np.random.default_rng([7, H, W]).normal(0.0, 0.01, (3, H, W))
    gt = np.ascontiguousarray(gt, np.float32)
    gt.setflags(write=False)
    return c, gt


def fit_cases(ridge=1e-6):
    """[(shape, render, gt, the oracle's row, cond)] of the noise fits; the condition number of every one is at most COND_MAX, so that
    the error bar of the GPU test, which grows with it, cannot swallow a wrong answer."""
    out = []
    for s in FIT_SHAPES:
        c, gt = fit_pair(s)
        A, cond = eo.fit_affine(c, gt, ridge, clamp=True, return_cond=True)
        assert cond <= COND_MAX, (s, cond)
        out.append((s, c, gt, A, cond))
    return out
