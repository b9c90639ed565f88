"""CPU: the frame decode's written definition (tests/frames_oracle.py) against the reference loader's own results
(tests/golden/frames/*.npz), the host-side logic of fdgs.frames that needs no device, and the new symbol of the C ABI."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest
import torch

import frames_oracle as fo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "frames", "*.npz")))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_fixtures_cover_the_shapes_the_kernel_distinguishes():
    assert len(FIXTURES) >= 4
    seen = set()
    for path in FIXTURES:
        d = np.load(path)
        u8 = d["u8"]
        N, H, W, Cn = u8.shape
        assert u8.dtype == np.uint8 and d["image"].shape == (N, 3, H, W) and d["image"].dtype == np.float32
        assert os.path.getsize(path) < 240_000
        assert len(np.unique(u8[..., :3])) == 256                     # every colour byte
        seen.add("rgba" if Cn == 4 else "rgb")
        if (H * W) % 4:
            seen.add("hw%4")
        if W % 4:
            seen.add("w%4")
        if (H * W * Cn) % 4 and N >= 2:
            seen.add("unaligned frames")
        if Cn == 4:
            assert d["mask"].shape == (N, 1, H, W)
            a = np.unique(u8[..., 3])
            assert len(a) == 256 and a[0] == 0 and a[-1] == 255      # 0, 255 and everything between
    assert seen == {"rgb", "rgba", "hw%4", "w%4", "unaligned frames"}, seen


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_oracle_equals_the_reference_loader_bit_for_bit(path):
    d = np.load(path)
    image, mask = fo.decode(d["u8"])
    assert np.array_equal(_bits(image), _bits(d["image"]))
    if d["u8"].shape[3] == 4:
        assert np.array_equal(_bits(mask), _bits(d["mask"]))
    else:
        assert mask is None
    assert image.min() >= 0.0 and image.max() <= 1.0                  # no clamp needed


def test_the_two_likely_wrong_kernels_differ_from_the_definition():
    """x * (1/255.f) differs from x / 255.f for 126 of the 256 bytes, (u * a) / 65025 from (u / 255) * (a / 255) for 37 247 of the
    65 536 pairs: the all-bytes tests on the GPU tell a reciprocal or a fused divide from the definition."""
    u = np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1).repeat(3, axis=3)
    right, _ = fo.decode(u)
    assert int((_bits(right) != _bits(fo.wrong_reciprocal(u))).sum()) == 3 * 126
    col, al = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    rgba = np.stack([col, col, col, al], -1)[None]
    right, _ = fo.decode(rgba)
    assert int((_bits(right[0, 0]) != _bits(fo.wrong_fused(col, al))).sum()) == 37247


def test_ring_arithmetic():
    from fdgs.frames import ring_runs
    assert ring_runs(0, 4, 8) == [(0, 4)] and ring_runs(4, 4, 8) == [(4, 4)] and ring_runs(8, 4, 8) == [(0, 4)]
    assert ring_runs(3, 2, 5) == [(3, 2)] and ring_runs(4, 3, 5) == [(4, 1), (0, 2)] and ring_runs(12, 5, 5) == [(2, 3), (0, 2)]
    # a ring that is a multiple of the batch never wraps inside a batch: one launch per batch
    assert all(len(ring_runs(k * 4, 4, 8)) == 1 for k in range(20))
    # every slot is handed out once per `slots` frames, in order
    cursor, seen = 0, []
    for n in (2, 3, 1, 4, 2, 3):
        for first, count in ring_runs(cursor, n, 5):
            seen += list(range(first, first + count))
        cursor += n
    assert seen == [k % 5 for k in range(15)]
    with pytest.raises(ValueError, match="does not fit"):
        ring_runs(0, 5, 4)
    with pytest.raises(ValueError):
        ring_runs(0, 0, 4)


def test_index_validation_happens_on_the_host():
    from fdgs.frames import check_index
    assert check_index([0, 3, 3, -1], 4) == [0, 3, 3, 3]
    assert check_index(torch.tensor([2, 1]), 3) == [2, 1]
    for bad in ([4], [-5], [0, 7, 1], [1.5]):
        with pytest.raises(ValueError, match="out of range"):
            check_index(bad, 4)
    with pytest.raises(ValueError, match="empty"):
        check_index([], 4)


def test_frame_array_validation():
    from fdgs.frames import FrameStore, _as_u8_frames
    a = np.zeros((5, 6, 3), np.uint8)
    assert tuple(_as_u8_frames([a, a]).shape) == (2, 5, 6, 3)
    assert tuple(_as_u8_frames(np.zeros((3, 5, 6, 4), np.uint8)).shape) == (3, 5, 6, 4)
    assert tuple(_as_u8_frames(torch.zeros((1, 2, 2, 3), dtype=torch.uint8)).shape) == (1, 2, 2, 3)
    with pytest.raises(ValueError, match="one shape"):
        _as_u8_frames([a, np.zeros((5, 7, 3), np.uint8)])
    with pytest.raises(ValueError, match="3 .RGB. or 4 .RGBA. channels"):
        _as_u8_frames(np.zeros((2, 5, 6, 2), np.uint8))
    with pytest.raises(ValueError, match="uint8"):
        _as_u8_frames(np.zeros((2, 5, 6, 3), np.float32))
    with pytest.raises(ValueError, match="uint8"):
        _as_u8_frames([a.astype(np.float32)])
    with pytest.raises(ValueError, match="no frames"):
        _as_u8_frames([])
    # checked before any device is touched
    with pytest.raises(ValueError, match="residency"):
        FrameStore(np.zeros((2, 5, 6, 3), np.uint8), residency="disk")
    with pytest.raises(ValueError, match="at least 2 slots"):
        FrameStore(np.zeros((2, 5, 6, 3), np.uint8), slots=1)
    with pytest.raises(ValueError, match="channels"):
        FrameStore(np.zeros((2, 5, 6, 2), np.uint8))


def test_decode_frames_refuses_cpu_tensors():
    from fdgs.frames import decode_frames
    u8 = torch.zeros((2, 4, 4, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="GPU tensor"):
        decode_frames(u8, torch.zeros(1, dtype=torch.int32), torch.zeros((1, 3, 4, 4)))
    with pytest.raises(ValueError, match="channels"):
        decode_frames(torch.zeros((2, 4, 4, 2), dtype=torch.uint8), torch.zeros(1, dtype=torch.int32), torch.zeros((1, 3, 4, 4)))


def test_library_exports_frames_decode_with_the_declared_signature():
    from fdgs import _capi
    assert "fdgs_frames_decode" in _capi.EXPORTED and hasattr(_capi.lib, "fdgs_frames_decode")
    with open(os.path.join(ROOT, "include", "fdgs.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    decl = re.search(r"int\s+fdgs_frames_decode\s*\((.*?)\)\s*;", text, re.S).group(1)
    types = [re.sub(r"\s*\w+$", "", " ".join(p.split())) for p in decl.split(",")]
    assert types == ["const uint8_t*", "int32_t", "int32_t", "int32_t", "int32_t", "const int32_t*", "int32_t", "float*", "int64_t",
                     "float*", "int64_t", "void*"], types
    want = {"const uint8_t*": C.c_void_p, "const int32_t*": C.c_void_p, "float*": C.c_void_p, "void*": C.c_void_p,
            "int32_t": C.c_int32, "int64_t": C.c_int64}
    assert list(_capi.lib.fdgs_frames_decode.argtypes) == [want[t] for t in types]
    assert _capi.lib.fdgs_frames_decode.restype is C.c_int


def test_frames_decode_argument_errors_without_a_launch():
    """FDGS_ERR_INVALID_ARG (1) for C outside {3, 4}, non-positive sizes, NULL pointers and short strides: all decided on the host side
    of the call, before any launch (this runs on a machine without a GPU)."""
    from fdgs import _capi
    f = _capi.lib.fdgs_frames_decode
    p = C.c_void_p(4096)   # never dereferenced: every call below is refused
    assert f(p, 2, 4, 4, 2, p, 1, p, 48, None, 0, None) == 1 and "C must be 3" in _capi.last_error()
    assert f(p, 2, 4, 4, 5, p, 1, p, 48, None, 0, None) == 1
    for N, H, W, B in ((0, 4, 4, 1), (2, 0, 4, 1), (2, 4, -1, 1), (2, 4, 4, 0), (2, 4, 4, 70000), (2, 65536, 65536, 1)):
        assert f(p, N, H, W, 3, p, B, p, 3 * max(H, 0) * max(W, 0), None, 0, None) == 1 and "bad sizes" in _capi.last_error()
    assert f(None, 2, 4, 4, 3, p, 1, p, 48, None, 0, None) == 1 and "missing pointer" in _capi.last_error()
    assert f(p, 2, 4, 4, 3, None, 1, p, 48, None, 0, None) == 1
    assert f(p, 2, 4, 4, 3, p, 1, None, 48, None, 0, None) == 1
    assert f(p, 2, 4, 4, 3, p, 2, p, 47, None, 0, None) == 1 and "out_stride" in _capi.last_error()
    assert f(p, 2, 4, 4, 4, p, 2, p, 48, p, 15, None) == 1 and "mask_stride" in _capi.last_error()
