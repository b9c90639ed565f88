"""CPU: the frame resize's written definition (tests/resize_oracle.py) against Pillow's own results (tests/golden/resize/*.npz, and
Pillow itself where it imports), the host-side logic of fdgs.resize that needs no device, and the new symbols of the C ABI."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import resize_cases as rc
import resize_oracle as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "resize", "*.npz")))
IDS = [os.path.basename(p)[:-4] for p in FIXTURES]

try:
    from PIL import Image
except ImportError:
    Image = None


def test_fixtures_cover_the_shape_list():
    want = {rc.case_id(s, d, c) for s, d in rc.SHAPES for c in (3, 4)}
    assert set(IDS) == want
    for path in FIXTURES:
        d = np.load(path)
        assert os.path.getsize(path) < (1 << 20)
        assert str(d["pil_version"])
        name = os.path.basename(path)[:-4]
        src, dst, c = next((s, t, c) for s, t in rc.SHAPES for c in (3, 4) if rc.case_id(s, t, c) == name)
        assert np.array_equal(d["u8"], rc.contents(src[0], src[1], c))      # the files hold exactly the generated inputs
        assert tuple(d["size"]) == (dst[1], dst[0]) and d["resized"].shape == (6, dst[0], dst[1], c)


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_oracle_equals_pillow_byte_for_byte(path):
    d = np.load(path)
    size = tuple(int(s) for s in d["size"])
    got = ro.resize(d["u8"], size)
    assert got.dtype == np.uint8 and np.array_equal(got, d["resized"])
    if Image is not None:
        mode = "RGB" if d["u8"].shape[3] == 3 else "RGBA"
        for f, g in zip(d["u8"], got):
            assert np.array_equal(np.array(Image.fromarray(f, mode).resize(size)), g)


def test_the_two_likely_wrong_kernels_differ_from_pillow():
    """float32 accumulation with round-to-nearest and a float intermediate between the passes both differ from Pillow on the golden
    inputs: the inputs tell them from the definition."""
    d = np.load(os.path.join(ROOT, "tests", "golden", "resize", "203x270_to_102x135_c3.npz"))
    size = tuple(int(s) for s in d["size"])
    for wrong in (ro.resize_wrong_float32, ro.resize_wrong_float_intermediate):
        differing = sum(int((wrong(f, size) != g).sum()) for f, g in zip(d["u8"][:2], d["resized"][:2]))
        assert differing > 0, wrong.__name__
        # ... and they are resizes, not noise: most bytes agree
        assert differing < d["resized"][:2].size // 2, wrong.__name__


def test_composite_equals_the_readers_expression_for_every_pair():
    """floor((...) * 255) equals the reference's np.array(arr * 255.0, dtype=np.byte) read as unsigned, for all 65 536 (c, a) pairs."""
    col, al = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    rgba = np.stack([col, col, col, al], -1)
    norm = rgba / 255.0
    for white in (True, False):
        bg = np.array([1, 1, 1]) if white else np.array([0, 0, 0])
        arr = norm[:, :, :3] * norm[:, :, 3:4] + bg * (1 - norm[:, :, 3:4])
        assert arr.min() >= 0.0 and (arr * 255.0).max() < 256.0
        ref = (arr * 255.0).astype(np.int64).astype(np.uint8)     # truncation of a non-negative value = what the byte cast keeps
        assert np.array_equal(ro.composite(rgba, white), ref)
        kept = ro.composite(rgba, white, keep_alpha=True)
        assert np.array_equal(kept[..., :3], ref) and np.array_equal(kept[..., 3], al)


def test_target_resolution_follows_loadcam():
    from fdgs.resize import target_resolution as tr
    assert tr(2704, 2028, 2)[:2] == ((1352, 1014), 2.0)
    assert tr(2704, 2028, 1)[:2] == ((2704, 2028), 1.0)
    # Python's round is half to even: 1011 / 2 = 505.5 -> 506, 1013 / 2 = 506.5 -> 506
    assert tr(1011, 1013, 2)[0] == (506, 506)
    assert tr(1352, 1014, 8)[0] == (169, 127)                      # 126.75 -> 127
    assert tr(1000, 750, 3)[0] == (333, 250)
    # -1: the original size, capped at 1600 px width
    size, scale, _ = tr(1920, 1080, -1)
    assert size == (1600, 900) and scale == 1920 / 1600
    assert tr(1352, 1014, -1)[:2] == ((1352, 1014), 1.0)
    assert tr(2704, 2028, -1)[0] == (1600, int(2028 / (2704 / 1600)))
    # any other number is a target width; the height is truncated
    size, scale, _ = tr(2704, 2028, 800)
    assert size == (800, 600) and scale == 2704 / 800
    assert tr(1000, 777, 300)[0] == (int(1000 / (1000 / 300)), int(777 / (1000 / 300)))
    # resolution_scale multiplies in
    assert tr(2704, 2028, 2, resolution_scale=2.0)[:2] == ((676, 507), 4.0)
    assert tr(2704, 2028, -1, resolution_scale=2.0)[:2] == ((800, 600), 2 * 2704 / 1600)
    # the intrinsics are divided by the scale
    _, scale, k = tr(2704, 2028, 2, cx=1352.0, cy=1014.0, fl_x=1462.6, fl_y=1461.2)
    assert k == {"cx": 676.0, "cy": 507.0, "fl_x": 1462.6 / 2, "fl_y": 1461.2 / 2}
    assert tr(1920, 1080, -1, cx=960.0)[2] == {"cx": 960.0 / (1920 / 1600), "cy": None, "fl_x": None, "fl_y": None}


def test_coefficients_of_the_flagship_axis():
    from fdgs.resize import coefficients
    k, b = coefficients(2704, 1352)
    assert k.dtype == np.int32 and b.dtype == np.int32 and k.shape == (1352, 9) and b.shape == (1352, 2)
    assert b[:, 0].min() >= 0 and (b[:, 0] + b[:, 1]).max() <= 2704 and b[:, 1].min() >= 1 and b[:, 1].max() <= 9
    assert np.all(np.diff(b[:, 0]) >= 0) and np.all(np.diff(b[:, 0] + b[:, 1]) >= 0)      # monotonic windows: the kernel's tiles rely on it
    sums = k.sum(axis=1, dtype=np.int64)
    assert np.all(np.abs(sums - (1 << 22)) <= b[:, 1])                                     # each tap is rounded on its own
    assert np.all(k[np.arange(9)[None, :] >= b[:, 1:2]] == 0)                              # nothing behind a row's count
    assert np.abs(k).max() < (1 << 23)                                                     # 24-bit signed: the kernel's multiply


@pytest.mark.parametrize("n_in,n_out", [(2704, 1352), (2028, 1014), (5, 13), (6, 11), (100, 12), (64, 8), (1, 3), (9, 9), (9, 4), (47, 16),
                                        (270, 135), (203, 102), (20000, 2), (1013, 506)])
def test_coefficients_equal_the_oracle(n_in, n_out):
    from fdgs.resize import coefficients
    ks, bounds, taps = ro.coefficients(n_in, n_out)
    k, b = coefficients(n_in, n_out)
    assert k.shape == (n_out, ks) and np.array_equal(k, taps) and np.array_equal(b, bounds)
    assert np.abs(k).max() < (1 << 23)


def test_wrapper_validation_happens_before_any_device_is_touched():
    import torch
    from fdgs.resize import composite, coefficients, resize_frames, resized_store
    u8 = torch.zeros((2, 4, 4, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="GPU tensor"):
        resize_frames(u8, (2, 2))
    with pytest.raises(ValueError, match="channels"):
        resize_frames(torch.zeros((2, 4, 4, 2), dtype=torch.uint8), (2, 2))
    for bad in ((0, 2), (2,), (2.5, 2), "ab", None):
        with pytest.raises(ValueError, match="size"):
            resize_frames(u8, bad)
    with pytest.raises(ValueError, match="RGBA"):
        composite(u8, True)
    with pytest.raises(ValueError, match="GPU tensor"):
        composite(torch.zeros((2, 4, 4, 4), dtype=torch.uint8), True)
    with pytest.raises(ValueError, match="residency"):
        resized_store(np.zeros((2, 4, 4, 3), np.uint8), (2, 2), residency="disk")
    with pytest.raises(ValueError, match="background"):
        resized_store(np.zeros((2, 4, 4, 4), np.uint8), (2, 2), background="grey")
    with pytest.raises(ValueError, match="RGBA"):
        resized_store(np.zeros((2, 4, 4, 3), np.uint8), (2, 2), background="white")
    with pytest.raises(ValueError, match="chunk"):
        resized_store(np.zeros((2, 4, 4, 3), np.uint8), (2, 2), chunk=0)
    with pytest.raises(ValueError, match="positive"):
        coefficients(0, 4)


def test_library_exports_the_resize_calls_and_keeps_its_version():
    from fdgs import _capi
    for sym in ("fdgs_frames_resize", "fdgs_frames_resize_scratch_bytes", "fdgs_frames_composite"):
        assert sym in _capi.EXPORTED and hasattr(_capi.lib, sym)
    assert _capi.lib.fdgs_version() == 502
    assert len(_capi.lib.fdgs_frames_resize.argtypes) == 19 and _capi.lib.fdgs_frames_resize_scratch_bytes.restype is C.c_int64


def _resize_call(f, p, N=2, Hs=8, Ws=8, Cn=3, B=1, M=1, Hd=4, Wd=4, ksx=9, ksy=9, src=True, index=True, dst=True, tables=(True,) * 4):
    t = [p if x else None for x in tables]
    return f(p if src else None, N, Hs, Ws, Cn, p if index else None, B, p if dst else None, M, Hd, Wd, t[0], t[1], ksx, t[2], t[3], ksy, None, None)


def test_frames_resize_argument_errors_without_a_launch():
    """FDGS_ERR_INVALID_ARG (1), decided on the host side of the call before any launch (this runs on a machine without a GPU)."""
    from fdgs import _capi
    f = _capi.lib.fdgs_frames_resize
    p = C.c_void_p(4096)   # never dereferenced: every call below is refused
    assert _resize_call(f, p, Cn=2) == 1 and "C must be 3" in _capi.last_error()
    assert _resize_call(f, p, Cn=5) == 1
    for kw in (dict(N=0), dict(Hs=0), dict(Ws=-1), dict(Hd=0), dict(Wd=0), dict(B=0), dict(M=0), dict(B=70000, M=70000), dict(B=2, M=1),
               dict(Hs=40000, Ws=40000, ksx=40001, ksy=40001)):
        assert _resize_call(f, p, **kw) == 1 and "bad sizes" in _capi.last_error(), kw
    for kw in (dict(src=False), dict(index=False), dict(dst=False), dict(tables=(False, True, True, True)), dict(tables=(True, False, True, True)),
               dict(tables=(True, True, False, True)), dict(tables=(True, True, True, False))):
        assert _resize_call(f, p, **kw) == 1 and "missing pointer" in _capi.last_error(), kw
    # 8 -> 4 takes ceil(2 * 2) * 2 + 1 = 9 taps, 4 -> 8 takes 5, 100 -> 12 takes ceil(16.67) * 2 + 1 = 35
    assert _resize_call(f, p, ksx=5) == 1 and "ksize" in _capi.last_error()
    assert _resize_call(f, p, ksy=8) == 1 and "ksize" in _capi.last_error()
    assert _resize_call(f, p, Ws=100, Wd=12, ksx=33) == 1 and "ksize" in _capi.last_error()
    s = _capi.lib.fdgs_frames_resize_scratch_bytes
    assert s(1, 8, 8, 4, 4, 2) == -1 and s(0, 8, 8, 4, 4, 3) == -1 and s(1, 8, 0, 4, 4, 3) == -1
    assert s(4, 8, 8, 4, 8, 3) == 0 and s(4, 8, 8, 8, 4, 3) == 0 and s(4, 8, 8, 8, 8, 3) == 0     # at most one pass: no intermediate
    assert s(4, 2028, 2704, 1014, 1352, 3) == 0                                                      # the fused kernel keeps it in LDS
    assert s(3, 4, 20000, 5, 2, 3) == 3 * 4 * 2 * 3                                                  # 40 001 taps: [B, Hs, Wd, C]
    # ... and a two-pass call that needs the intermediate refuses a NULL scratch
    assert f(p, 2, 4, 20000, 3, p, 1, p, 1, 5, 2, p, p, 40001, p, p, 5, None, None) == 1 and "scratch" in _capi.last_error()


def test_frames_composite_argument_errors_without_a_launch():
    from fdgs import _capi
    f = _capi.lib.fdgs_frames_composite
    p = C.c_void_p(4096)
    for N, H, W in ((0, 4, 4), (2, 0, 4), (2, 4, -1), (1, 30000, 30000)):
        assert f(p, N, H, W, 1, 0, p, None) == 1 and "bad sizes" in _capi.last_error()
    assert f(None, 2, 4, 4, 1, 0, p, None) == 1 and "missing pointer" in _capi.last_error()
    assert f(p, 2, 4, 4, 0, 1, None, None) == 1 and "missing pointer" in _capi.last_error()
