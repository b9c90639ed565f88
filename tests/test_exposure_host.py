"""CPU: the companion header's symbols and argument handling of the exposure kernels (nothing is launched here), and the float64
yardstick of tests/exposure_oracle.py against central differences and an exact fit."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import exposure_cases as ec
import exposure_oracle as eo
from fdgs import exposure      # the yardstick below is this module's: without it there is nothing to hold to it

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    with open(os.path.join(ROOT, "include", "fdgs_exposure.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return sorted(set(re.findall(r"\b(fdgs_[a-z_0-9]+)\s*\(", text)))


def test_library_exports_every_symbol_of_the_exposure_header():
    from fdgs import _capi, _exposure_capi
    names = _declared_symbols()
    assert len(names) == 6 and all(n.startswith(("fdgs_exposure_", "fdgs_colour_fit_")) for n in names)
    assert sorted(_exposure_capi.EXPORTED) == names == sorted(_exposure_capi.SIGNATURES)
    for n in names:
        assert hasattr(_capi.lib, n), "libfdgs.so does not export %s" % n
        restype, argtypes = _exposure_capi.SIGNATURES[n]
        fn = getattr(_exposure_capi.lib, n)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), n
    assert not set(names) & set(_capi.EXPORTED) and _exposure_capi.lib is _capi.lib and _exposure_capi.call is _capi.call
    with open(os.path.join(ROOT, "include", "fdgs_exposure.h")) as f:
        defines = dict(re.findall(r"#define (FDGS_EXPOSURE_\w+) (\d+)", f.read()))
    assert (int(defines["FDGS_EXPOSURE_BLOCK_PIXELS"]), int(defines["FDGS_EXPOSURE_MAX_BLOCKS"]), int(defines["FDGS_EXPOSURE_MAX_VIEWS"])) == (
        _exposure_capi.EXPOSURE_BLOCK_PIXELS, _exposure_capi.EXPOSURE_MAX_BLOCKS, _exposure_capi.EXPOSURE_MAX_VIEWS)
    assert ec.BLOCK == _exposure_capi.EXPOSURE_BLOCK_PIXELS and exposure.MAX_VIEWS == _exposure_capi.EXPOSURE_MAX_VIEWS


def test_partial_counts_follow_the_workgroups_of_a_pass():
    from fdgs import _exposure_capi
    lib, blk = _exposure_capi.lib, ec.BLOCK
    for H, W, nb in ((1, 1, 1), (1, blk, 1), (1, blk + 1, 2), (3, 2 * blk + 1, 7), (1014, 1352, (1014 * 1352 + blk - 1) // blk),
                     (4096, 4096, _exposure_capi.EXPOSURE_MAX_BLOCKS), (0, 5, 1), (46341, 46341, 1)):
        assert lib.fdgs_exposure_num_partials(H, W) == 12 * nb, (H, W)
        assert lib.fdgs_colour_fit_num_partials(H, W) == 22 * nb, (H, W)


_N = None
_CAMS = (C.c_int32 * 3)(0, 2, 1)
_CAMS_BAD = (C.c_int32 * 3)(0, 3, 1)
_CAMS_NEG = (C.c_int32 * 3)(0, -1, 1)
_ADAM = (1e-3, 0.9, 0.999, 1e-15, _N)
_REJECTED = [
    ("fdgs_exposure_apply", (0, 4, _N, _N, 3, 0, _N, _N), "fdgs_exposure_apply: bad image size H=0 W=4"),
    ("fdgs_exposure_apply", (4, -1, _N, _N, 3, 0, _N, _N), "fdgs_exposure_apply: bad image size H=4 W=-1"),
    ("fdgs_exposure_apply", (65536, 32768, _N, _N, 3, 0, _N, _N), "fdgs_exposure_apply: bad image size"),
    ("fdgs_exposure_apply", (4, 4, _N, _N, 3, 3, _N, _N), "fdgs_exposure_apply: camera=3 is outside the table's 3 rows"),
    ("fdgs_exposure_apply", (4, 4, _N, _N, 3, -1, _N, _N), "fdgs_exposure_apply: camera=-1 is outside"),
    ("fdgs_exposure_apply", (4, 4, _N, _N, 3, 0, _N, _N), "fdgs_exposure_apply: image / table / out must not be NULL"),
    ("fdgs_exposure_backward", (4, 0, _N, _N, _N, 3, 0, _N, _N, _N, 0, _N), "fdgs_exposure_backward: bad image size H=4 W=0"),
    ("fdgs_exposure_backward", (4, 4, _N, _N, _N, 3, 5, _N, _N, _N, 0, _N), "fdgs_exposure_backward: camera=5 is outside the table's 3 rows"),
    ("fdgs_exposure_backward", (4, 4, _N, _N, _N, 3, 0, _N, _N, _N, 0, _N), "fdgs_exposure_backward: g_out / image / table / partials / dA must not be NULL"),
    ("fdgs_exposure_adam", (0, _N, _N, _N, _N, 3, _N, _CAMS) + _ADAM, "fdgs_exposure_adam: num_cameras=0 is below 1"),
    ("fdgs_exposure_adam", (3, _N, _N, _N, _N, 0, _N, _CAMS) + _ADAM, "fdgs_exposure_adam: B=0 views is below 1"),
    ("fdgs_exposure_adam", (3, _N, _N, _N, _N, -2, _N, _CAMS) + _ADAM, "fdgs_exposure_adam: B=-2 views is below 1"),
    ("fdgs_exposure_adam", (3, _N, _N, _N, _N, 65, _N, _CAMS) + _ADAM, "fdgs_exposure_adam: B=65 views is above 64"),
    ("fdgs_exposure_adam", (3, _N, _N, _N, _N, 3, _N, None) + _ADAM, "fdgs_exposure_adam: the host array cameras must not be NULL"),
    ("fdgs_exposure_adam", (3, _N, _N, _N, _N, 3, _N, _CAMS_BAD) + _ADAM, "fdgs_exposure_adam: cameras[1]=3 is outside the table's 3 rows"),
    ("fdgs_exposure_adam", (3, _N, _N, _N, _N, 3, _N, _CAMS_NEG) + _ADAM, "fdgs_exposure_adam: cameras[1]=-1 is outside the table's 3 rows"),
    ("fdgs_exposure_adam", (3, _N, _N, _N, _N, 3, _N, _CAMS) + _ADAM, "fdgs_exposure_adam: table / exp_avg / exp_avg_sq / steps / slots must not be NULL"),
    ("fdgs_colour_fit_moments", (0, 0, _N, _N, 1, _N, _N, _N), "fdgs_colour_fit_moments: bad image size H=0 W=0"),
    ("fdgs_colour_fit_moments", (4, 4, _N, _N, 1, _N, _N, _N), "fdgs_colour_fit_moments: image / gt / partials / moments must not be NULL"),
]


@pytest.mark.parametrize("row", range(len(_REJECTED)), ids=lambda i: "%s-%d" % (_REJECTED[i][0], i))
def test_every_exposure_rejection_carries_its_own_message(row):
    """fdgs_last_error() describes the call that failed, not an earlier one: after the rasterizer's "bad sizes" failure on the same
    thread, every rejected call leaves its own text.  All of these are turned away before anything touches the GPU."""
    from fdgs import _capi, _exposure_capi
    name, args, text = _REJECTED[row]
    scene, out, R = _capi.FdgsScene(), _capi.FdgsForwardOut(), C.c_int32(0)
    scene.P, scene.W, scene.H = 10, 0, 16
    cb = _capi.ALLOC_FN(lambda u, w, n: None)
    assert _capi.lib.fdgs_rasterize_forward(C.byref(scene), C.byref(out), cb, None, None, C.byref(R)) == 1
    assert "bad sizes" in _capi.last_error()   # the poison
    assert getattr(_exposure_capi.lib, name)(*args) == 1
    err = _capi.last_error()
    print(name, "->", err)
    assert text in err and "bad sizes" not in err


def test_cpu_tensors_are_refused():
    img = torch.zeros((3, 4, 4))
    tab = torch.zeros((2, 12))
    slot = torch.zeros(12)
    for call in (lambda: exposure.apply_(img, tab, 0), lambda: exposure.apply(img, tab, 0), lambda: exposure.backward_(img, img, tab, 0, slot),
                 lambda: exposure.fit_moments(img, img), lambda: exposure.fit_affine(img, img), lambda: exposure.ExposureModel(3, "cpu")):
        with pytest.raises(RuntimeError, match="must live on the GPU.*there is no CPU path"):
            call()
    with pytest.raises(ValueError):
        exposure.ExposureModel(0, "cpu")


def test_two_ranks_are_refused_before_anything_is_built():
    from fdgs.pipeline import StepPipeline
    with pytest.raises(NotImplementedError, match="exposure"):
        StepPipeline(None, None, world_size=2, exposure=object())


@pytest.mark.parametrize("kind", ec.ROWS)
def test_oracle_gradients_agree_with_central_differences(kind):
    """L = sum w * apply(c, A): the oracle's analytic d L / d c and d L / d A against (L(x + h) - L(x - h)) / 2 h in float64.  L is
    linear in c and in A separately, so the central difference is exact up to rounding: 1e-9 of the gradient's scale."""
    shape = (3, 5)
    c = ec.image("wild", shape).astype(np.float64)
    w = ec.upstream(shape).astype(np.float64) * 1e3
    A = ec.row(kind).astype(np.float64)
    g_image, dA = eo.backward(w, c, A)

    def L(cc, AA):
        return float((w * eo.apply(cc, AA)).sum())
    h = 1e-3
    for k in range(12):
        d = np.zeros(12)
        d[k] = h
        num = (L(c, A + d) - L(c, A - d)) / (2 * h)
        assert abs(num - dA[k]) <= 1e-9 * max(1.0, np.abs(dA).max()), (k, num, dA[k])
    for idx in np.ndindex(*c.shape):
        d = np.zeros_like(c)
        d[idx] = h
        num = (L(c + d, A) - L(c - d, A)) / (2 * h)
        assert abs(num - g_image[idx]) <= 1e-9 * max(1.0, np.abs(g_image).max()), (idx, num, g_image[idx])


@pytest.mark.parametrize("shape", ec.FIT_SHAPES, ids=ec.shape_id)
def test_oracle_fit_recovers_an_exact_transform(shape):
    c = ec.image("noise", shape).astype(np.float64)
    for kind in ec.ROWS:
        A = ec.row(kind).astype(np.float64)
        got = eo.fit_affine(c, eo.apply(c, A), ridge=0.0, clamp=True)
        assert np.abs(got - A).max() <= 1e-9 * max(1.0, np.abs(A).max()), (kind, np.abs(got - A).max())


def test_fit_cases_are_well_conditioned_and_the_host_solve_is_the_oracles():
    """The noise fits of the GPU test have cond <= 1e4 (asserted by fit_cases); fdgs.exposure.solve_affine, the host half of
    fit_affine, gives the oracle's row from the oracle's moments; a constant image still has a finite answer."""
    cases = ec.fit_cases()
    assert len(cases) == len(ec.FIT_SHAPES) >= 5
    for shape, c, gt, A, cond in cases:
        print(ec.shape_id(shape), "cond %.1f" % cond)
        M, N, n = eo.fit_moments(c, gt, clamp=True)
        m = np.concatenate([M[np.triu_indices(4)], N.reshape(12)])
        got = exposure.solve_affine(m, n, 1e-6)
        assert np.abs(got - A).max() <= 1e-12 * cond * max(1.0, np.abs(A).max())
    c = ec.image("constant", (3, 5))
    A = eo.fit_affine(c, c, 1e-6)
    assert np.isfinite(A).all()


def test_oracle_adam_matches_torch_and_leaves_other_rows_alone():
    rng = np.random.default_rng(11)
    p = torch.tensor(rng.normal(size=(4, 12)), dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([p], lr=1e-3, betas=(0.9, 0.999), eps=1e-15)
    state = (p.detach().numpy().copy(), np.zeros((4, 12)), np.zeros((4, 12)), np.zeros(4, np.int64))
    for _ in range(3):
        g = rng.normal(size=(4, 12))
        p.grad = torch.tensor(g)
        opt.step()
        state = eo.adam(*state, [0, 1, 2, 3], g)
    assert np.abs(state[0] - p.detach().numpy()).max() <= 1e-14
    slots = rng.normal(size=(3, 12))
    new = eo.adam(*state, [2, 0, 2], slots)
    assert np.array_equal(new[0][[1, 3]], state[0][[1, 3]]) and np.array_equal(new[1][[1, 3]], state[1][[1, 3]])
    assert list(new[3]) == [4, 3, 4, 3]
    one = eo.adam(*state, [2, 0], np.stack([slots[0] + slots[2], slots[1]]))
    assert np.array_equal(one[0], new[0]) and np.array_equal(one[2], new[2])
