"""GPU: fdgs.resize -- the resize kernels against the written definition (tests/resize_oracle.py, which equals Pillow byte for byte:
tests/test_resize_host.py), Pillow's recorded results (tests/golden/resize) and Pillow itself where it imports; the compositing
kernel; and the stores built from full-size frames.  Every comparison is bitwise: the arithmetic is integer, there is no tolerance."""
import functools
import os

import numpy as np
import pytest
import torch

import frames_oracle as fo
import resize_cases as rc
import resize_oracle as ro

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xA5
CASES = [(s, d, c) for s, d in rc.SHAPES for c in (3, 4)]

try:
    from PIL import Image
except ImportError:
    Image = None


@functools.lru_cache(maxsize=None)
def _case(src, dst, C):
    """(frames uint8 [6, Hs, Ws, C], the oracle's resize of them) -- computed once per module."""
    u8 = rc.contents(src[0], src[1], C)
    want = ro.resize(u8, (dst[1], dst[0]))
    want.setflags(write=False)
    u8.setflags(write=False)
    return u8, want


class _two_launches:
    """Every call inside takes the two-launch path (fdgs_debug_frames_resize_path)."""

    def __enter__(self):
        from fdgs import _capi
        _capi.lib.fdgs_debug_frames_resize_path(1)

    def __exit__(self, *exc):
        from fdgs import _capi
        _capi.lib.fdgs_debug_frames_resize_path(0)


def _resize_into_sentinels(u8_dev, size, index, extra=2):
    """resize_frames into the leading frames of a sentinel-filled ``out`` of B + extra frames (M > B)."""
    from fdgs.resize import resize_frames
    B = len(index)
    out = torch.full((B + extra, size[1], size[0], u8_dev.shape[3]), SENTINEL, dtype=torch.uint8, device=u8_dev.device)
    idx = torch.tensor(index, dtype=torch.int32, device=u8_dev.device)
    assert resize_frames(u8_dev, size, idx, out) is out
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    assert (res[B:] == SENTINEL).all(), "resize_frames wrote behind its B frames"
    return res[:B]


@pytest.mark.parametrize("src,dst,C", CASES, ids=[rc.case_id(*c) for c in CASES])
def test_resize_equals_the_oracle_and_pillow(src, dst, C, gpu_device):
    u8, want = _case(src, dst, C)
    golden = np.load(os.path.join(ROOT, "tests", "golden", "resize", rc.case_id(src, dst, C) + ".npz"))
    assert np.array_equal(golden["u8"], u8) and np.array_equal(golden["resized"], want)
    size = (dst[1], dst[0])
    dev = torch.from_numpy(u8.copy()).to(gpu_device)
    got = _resize_into_sentinels(dev, size, list(range(6)))
    assert np.array_equal(got, want), "fused / single-launch path: %d bytes differ" % int((got != want).sum())
    with _two_launches():
        got = _resize_into_sentinels(dev, size, list(range(6)))
    assert np.array_equal(got, want), "two-launch path: %d bytes differ" % int((got != want).sum())
    if src == dst and C == 4:
        assert np.array_equal(got, u8)      # a copy: no premultiply round trip


@pytest.mark.parametrize("C", [3, 4])
def test_batch_index_repeats_and_out_of_range_entries_on_a_side_stream(C, gpu_device):
    """B = 5 from N = 3 with a repeated index, an entry of -1 and one of N (their frames keep the sentinel), M > B, a non-default stream."""
    src, dst = (33, 47), (11, 16)
    u8, want = _case(src, dst, C)
    dev = torch.from_numpy(u8[:3].copy()).to(gpu_device)
    order = [2, -1, 0, 3, 2]
    stream = torch.cuda.Stream(gpu_device)
    stream.wait_stream(torch.cuda.current_stream(gpu_device))
    for two in (False, True):
        with torch.cuda.stream(stream):
            if two:
                with _two_launches():
                    got = _resize_into_sentinels(dev, (dst[1], dst[0]), order)
            else:
                got = _resize_into_sentinels(dev, (dst[1], dst[0]), order)
        for b, n in enumerate(order):
            if 0 <= n < 3:
                assert np.array_equal(got[b], want[n]), (two, b, n)
            else:
                assert (got[b] == SENTINEL).all(), (two, b, n)


@pytest.mark.parametrize("C", [3, 4])
def test_arrays_that_do_not_start_on_a_dword_take_the_byte_path(C, gpu_device):
    from fdgs.resize import resize_frames
    for src, dst in (((33, 47), (11, 16)), ((9, 9), (9, 9)), ((5, 6), (11, 13))):
        u8, want = _case(src, dst, C)
        flat = torch.zeros(u8.size + 1, dtype=torch.uint8, device=gpu_device)
        odd = flat[1:].view(u8.shape)
        odd.copy_(torch.from_numpy(u8.copy()))
        oflat = torch.full((want.size + 3,), SENTINEL, dtype=torch.uint8, device=gpu_device)
        out = oflat[3:].view(want.shape)
        assert odd.data_ptr() % 4 and out.data_ptr() % 4
        resize_frames(odd, (dst[1], dst[0]), out=out)
        assert np.array_equal(out.cpu().numpy(), want) and (oflat[:3] == SENTINEL).all()


@pytest.mark.parametrize("C", [3, 4])
def test_thousands_of_taps_need_the_intermediate_in_scratch(C, gpu_device):
    """20000 -> 2 columns take 40 001 taps: no tile's source window fits LDS, the call itself chooses the two-launch path."""
    from fdgs import _capi
    from fdgs.resize import resize_frames
    rng = np.random.default_rng(5)
    u8 = rng.integers(0, 256, (2, 4, 20000, C), dtype=np.uint8)
    assert _capi.lib.fdgs_frames_resize_scratch_bytes(2, 4, 20000, 5, 2, C) == 2 * 4 * 2 * C
    want = ro.resize(u8, (2, 5))
    got = resize_frames(torch.from_numpy(u8).to(gpu_device), (2, 5)).cpu().numpy()
    assert np.array_equal(got, want)


@pytest.mark.parametrize("C", [3, 4])
def test_a_full_size_frame(C, gpu_device):
    """2028 x 2704 -> 1014 x 1352, the benchmark's C5 -> C3 step: against Pillow where it imports, the oracle otherwise."""
    from fdgs.resize import resize_frames
    rng = np.random.default_rng(11 + C)
    u8 = rng.integers(0, 256, (1, 2028, 2704, C), dtype=np.uint8)
    if C == 4:
        u8[0, :1000, :, 3] = rc.ALPHAS[rng.integers(0, 6, (1000, 2704))]
    if Image is not None:
        want = np.array(Image.fromarray(u8[0], "RGB" if C == 3 else "RGBA").resize((1352, 1014)))[None]
    else:
        want = ro.resize(u8, (1352, 1014))
    dev = torch.from_numpy(u8).to(gpu_device)
    got = resize_frames(dev, (1352, 1014)).cpu().numpy()
    assert np.array_equal(got, want), "%d bytes differ" % int((got != want).sum())
    with _two_launches():
        got = resize_frames(dev, (1352, 1014)).cpu().numpy()
    assert np.array_equal(got, want), "two-launch path: %d bytes differ" % int((got != want).sum())


def test_composite_every_colour_alpha_pair(gpu_device):
    from fdgs.resize import composite
    b = np.arange(256, dtype=np.uint8)
    col, al = np.meshgrid(b, b, indexing="ij")
    rgba = np.ascontiguousarray(np.stack([col, col[::-1], np.roll(col, 31, 0), al], -1)[None])      # [1, 256, 256, 4]
    dev = torch.from_numpy(rgba).to(gpu_device)
    for white in (True, False):
        for keep in (False, True):
            got = composite(dev, white, keep_alpha=keep)
            assert tuple(got.shape) == (1, 256, 256, 4 if keep else 3)
            assert np.array_equal(got.cpu().numpy(), ro.composite(rgba, white, keep)), (white, keep)
    # an odd start: the byte path of both sides
    flat = torch.zeros(rgba.size + 1, dtype=torch.uint8, device=gpu_device)
    odd = flat[1:].view(rgba.shape)
    odd.copy_(dev)
    assert np.array_equal(composite(odd, True).cpu().numpy(), ro.composite(rgba, True))


def _store_frames(C):
    u8, _ = _case((33, 47), (11, 16), C)
    return np.concatenate([u8, u8[:1, ::-1]])      # N = 7: no multiple of chunk 3


def _check_store(store, want_u8, rgba):
    N = len(want_u8)
    img, mask = fo.decode(want_u8)
    assert len(store) == N and store.shape == want_u8.shape[1:]
    idx = [N - 1, 0, 3, 0]
    got = store.batch(idx)
    assert all(torch.equal(g.cpu(), torch.from_numpy(img[i])) for g, i in zip(got, idx))
    if rgba:
        got, mk = store.batch(idx, masks=True)
        assert all(torch.equal(g.cpu(), torch.from_numpy(img[i])) for g, i in zip(got, idx))
        assert all(torch.equal(m.cpu(), torch.from_numpy(mask[i])) for m, i in zip(mk, idx))


@pytest.mark.parametrize("source", ["host", "device"])
@pytest.mark.parametrize("residency", ["device", "host"])
def test_resized_store_equals_decode_of_the_oracle_resize(source, residency, gpu_device):
    from fdgs.resize import resized_store
    size = (16, 11)
    for C in (3, 4):
        u8 = _store_frames(C)
        frames = torch.from_numpy(u8.copy()).to(gpu_device) if source == "device" else u8
        want = ro.resize(u8, size)
        stores = [resized_store(frames, size, residency=residency, chunk=chunk, device=gpu_device) for chunk in (1, 3, 64)]
        for st in stores:
            assert st.residency == residency and st.frames.is_cuda == (residency == "device")
            assert np.array_equal(st.frames.cpu().numpy(), want)          # the result does not depend on chunk
        _check_store(stores[1], want, C == 4)
    # with a background: composited (RGBA in, RGB out), then resized
    u8 = _store_frames(4)
    frames = torch.from_numpy(u8.copy()).to(gpu_device) if source == "device" else list(u8)
    for bg in ("white", "black"):
        want = ro.resize(ro.composite(u8, bg == "white"), size)
        for chunk in (1, 3, 64):
            st = resized_store(frames, size, residency=residency, chunk=chunk, background=bg, device=gpu_device)
            assert np.array_equal(st.frames.cpu().numpy(), want), (bg, chunk)
        _check_store(st, want, False)


def test_pinned_host_frames_skip_the_pinned_staging(gpu_device):
    from fdgs.resize import resized_store
    u8 = _store_frames(3)
    st = resized_store(torch.from_numpy(u8.copy()).pin_memory(), (16, 11), chunk=2, device=gpu_device)
    assert np.array_equal(st.frames.cpu().numpy(), ro.resize(u8, (16, 11)))


def test_pyramid_equals_separate_stores(gpu_device):
    from fdgs.resize import pyramid, resized_store
    u8 = _store_frames(4)
    sizes = [(24, 17), (16, 11)]
    for kw in (dict(residency="device", chunk=3), dict(residency="host", chunk=2, background="white")):
        levels = pyramid(u8, sizes, device=gpu_device, **kw)
        assert len(levels) == 2
        for st, size in zip(levels, sizes):
            alone = resized_store(u8, size, device=gpu_device, **kw)
            assert st.shape == alone.shape == (size[1], size[0], 3 if "background" in kw else 4)
            assert torch.equal(st.frames.cpu(), alone.frames.cpu())


@pytest.mark.parametrize("name,C", [("33x47_to_11x16", 3), ("33x47_to_11x16", 4), ("203x270_to_102x135", 3)])
def test_loss_is_identical_with_pillow_resized_ground_truth(name, C, gpu_device):
    """One fused_l1_ssim of a render against a frame from ``resized_store`` and against the same frame from a FrameStore built from
    Pillow's recorded resize: the identical float."""
    from fdgs.frames import FrameStore
    from fdgs.loss import fused_l1_ssim
    from fdgs.resize import resized_store
    d = np.load(os.path.join(ROOT, "tests", "golden", "resize", "%s_c%d.npz" % (name, C)))
    size = tuple(int(s) for s in d["size"])
    ours = resized_store(d["u8"], size, chunk=4, device=gpu_device)
    theirs = FrameStore(d["resized"], device=gpu_device)
    render = torch.rand((3, size[1], size[0]), generator=torch.Generator().manual_seed(3)).to(gpu_device)
    for i in range(len(d["u8"])):
        a = float(fused_l1_ssim(render, ours[i]))
        b = float(fused_l1_ssim(render, theirs[i]))
        assert a == b and np.isfinite(a), (i, a, b)
