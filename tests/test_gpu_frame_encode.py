"""GPU: fdgs.frames' way back -- fdgs_frames_encode / fdgs_frames_encode_gray against the PyTorch-CPU expression
``img.mul(255).add(0.5).clamp(0, 255).to(uint8)`` (torchvision's save_image; NaN -> 0) and the reference's easy_cmap, and the
FrameWriter's ring on the device and into pinned host memory.  Every comparison is bitwise: the operations are fixed and IEEE."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
CANARY = 0xA5


def cpu_encode(x):
    """The CPU expression, NaN handled explicitly (``.to(uint8)`` of a NaN is undefined)."""
    t = x.detach().cpu().float().mul(255).add(0.5)
    t = torch.where(torch.isnan(t), torch.zeros_like(t), t)
    return t.clamp(0, 255).to(torch.uint8)


def cpu_frames(images, alphas=None):
    """[B, 3, H, W] (+ [B, 1, H, W]) -> uint8 [B, H, W, 3 or 4]"""
    q = cpu_encode(images if alphas is None else torch.cat((images.cpu(), alphas.cpu()), 1))
    return q.permute(0, 2, 3, 1).contiguous()


def cpu_gray(planes):
    """easy_cmap (utils/image_utils.py:21-28) per plane, then the quantisation: [B, 1, H, W] -> uint8 [B, H, W, 1]"""
    out = []
    for x in planes.detach().cpu().float():
        x_max, x_min = x.max(), x.min()
        out.append(cpu_encode(torch.clamp((x - x_min) / (x_max - x_min), 0, 1)))
    return torch.stack(out).permute(0, 2, 3, 1).contiguous()


def special_values():
    """Every k / 255.0f and (k + 0.5) / 255 with their two fp32 neighbours, out-of-range values, +-inf, NaN, denormals, -0."""
    k = torch.arange(256, dtype=torch.float32)
    exact = k / 255.0
    half = ((k.double() + 0.5) / 255.0).float()
    up = lambda t: torch.nextafter(t, torch.full_like(t, 2.0))       # noqa: E731
    down = lambda t: torch.nextafter(t, torch.full_like(t, -2.0))    # noqa: E731
    odd = torch.tensor([-0.0, -1e-3, -7.5, 1.0 + 1e-6, 1.002, 3.0, 1e30, -1e30, float("inf"), float("-inf"), float("nan"),
                        1e-45, -1e-45, 1e-39, 1.1754942e-38, 0.5 / 255.0, 255.5 / 255.0, 0.99999994])
    return torch.cat([exact, up(exact), down(exact), half, up(half), down(half), odd])


def make_inputs(B, planes, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B * planes * H * W, generator=g) * 2.0 - 0.5       # below 0 and above 1
    sp = special_values()
    n = min(sp.numel(), x.numel())
    pos = torch.randperm(x.numel(), generator=g)[:n]
    x[pos] = sp[:n]
    return x.view(B, planes, H, W), n == sp.numel()


def _encode_into_canaries(images, alphas, order, N, dev):
    """encode_frames from strided inputs into frames 0 .. N-1 of N + 2 canary-filled ones; returns (frames, untouched outside?)."""
    from fdgs.frames import encode_frames
    B, _, H, W = images.shape
    C = 3 if alphas is None else 4
    pad = 24
    ring = torch.full((B, 3 * H * W + pad), -7.25, device=dev)
    src = ring[:, :3 * H * W].unflatten(1, (3, H, W))
    src.copy_(images)
    asrc = None
    if alphas is not None:
        aring = torch.full((B, H * W + pad), -7.25, device=dev)
        asrc = aring[:, :H * W].unflatten(1, (1, H, W))
        asrc.copy_(alphas)
    assert B == 1 or src.stride(0) > 3 * H * W
    flat = torch.full(((N + 2) * H * W * C,), CANARY, dtype=torch.uint8, device=dev)
    frames = flat[H * W * C:(N + 1) * H * W * C].view(N, H, W, C)
    index = torch.tensor(order, dtype=torch.int32, device=dev)
    assert encode_frames(src, index, frames, asrc) is frames
    torch.cuda.synchronize()
    clean = bool((flat[:H * W * C] == CANARY).all() and (flat[(N + 1) * H * W * C:] == CANARY).all())
    return frames.cpu(), clean


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("shape", [(4, 13, 15), (4, 17, 20), (4, 16, 18), (4, 1014, 1352)], ids=lambda s: "%dx%dx%d" % s)
def test_encode_equals_the_cpu_expression(shape, C, gpu_device):
    """13 x 15: H*W*3 = 585 bytes per frame, no frame but the first starts on a dword -- the byte-wise path (C = 3), and a tail of 3
    pixels on the vector path (C = 4); 17 x 20 and 16 x 18: the vector path, the canary frame in front puts 17 x 20's frames at an
    odd multiple of 1020 bytes, still a dword; 1014 x 1352: the benchmark's size.  Slots shuffled, one of them out of range."""
    B, H, W = shape
    images, all_special = make_inputs(B, 3, H, W, seed=H)
    assert all_special
    alphas = make_inputs(B, 1, H, W, seed=H + 1)[0] if C == 4 else None
    N = B + 2
    order = [3, N + 5, 0, 4]       # image 1 goes nowhere; frames 1, 2, 5 are not selected
    want = cpu_frames(images, alphas)
    got, clean = _encode_into_canaries(images, alphas, order, N, gpu_device)
    assert clean, "encode_frames wrote outside the frame array"
    for b, n in enumerate(order):
        if 0 <= n < N:
            diff = int((got[n] != want[b]).sum())
            assert diff == 0, (b, n, diff)
    for n in sorted(set(range(N)) - set(order)):
        assert bool((got[n] == CANARY).all()), "frame %d was not selected and has been written" % n


def test_encode_is_the_inverse_of_decode(gpu_device):
    from fdgs.frames import decode_frames, encode_frames
    dev = gpu_device
    b = torch.arange(256, dtype=torch.uint8)
    zero = torch.zeros(1, dtype=torch.int32, device=dev)
    rgb = torch.stack([b, b.flip(0), b.roll(77)], -1).reshape(1, 16, 16, 3).to(dev)
    img = torch.empty((1, 3, 16, 16), device=dev)
    decode_frames(rgb, zero, img)
    back = torch.full_like(rgb, CANARY)
    encode_frames(img, zero, back)
    assert torch.equal(back.cpu(), rgb.cpu()), int((back != rgb).sum())
    # RGBA with alpha byte 255: the colours return unchanged, the fourth byte is the encoded alpha plane
    rgba = torch.cat((rgb, torch.full((1, 16, 16, 1), 255, dtype=torch.uint8, device=dev)), -1).contiguous()
    mk = torch.empty((1, 1, 16, 16), device=dev)
    decode_frames(rgba, zero, img, mk)
    assert bool((mk == 1.0).all())
    alpha = torch.rand(1, 1, 16, 16, generator=torch.Generator().manual_seed(3)).to(dev) * 1.2 - 0.1
    back = torch.full_like(rgba, CANARY)
    encode_frames(img, zero, back, alpha)
    assert torch.equal(back[..., :3].cpu(), rgb.cpu())
    assert torch.equal(back[..., 3].cpu(), cpu_encode(alpha)[:, 0])
    encode_frames(img, zero, back, mk)
    assert torch.equal(back.cpu(), rgba.cpu())


@pytest.mark.parametrize("shape", [(3, 13, 15), (2, 16, 18), (1, 17, 21), (2, 1014, 1352)], ids=lambda s: "%dx%dx%d" % s)
def test_grey_depth_equals_easy_cmap(shape, gpu_device):
    from fdgs.frames import encode_gray
    B, H, W = shape
    g = torch.Generator().manual_seed(W)
    planes = torch.rand(B, 1, H, W, generator=g) * 7.0 + 0.2
    planes[0, 0, H // 2, W // 3] = -3.0
    planes[-1].fill_(4.5)                          # a constant plane: 0 / 0 everywhere -> all 0
    if B > 2:
        planes[1, 0, H - 1, W - 1] = 90.0          # the maximum in the last pixel: the reduction must see the tail (13 * 15 = 4 * 48 + 3)
    if B == 1:
        planes[0].uniform_(0.0, 1.0, generator=g)
        planes[0, 0, H - 1, W - 1] = -55.0         # the minimum in the last pixel of 17 * 21 = 4 * 89 + 1
    want = cpu_gray(planes)
    assert bool((want[-1] == 0).all()) or B == 1
    N = B + 1
    flat = torch.full(((N + 2) * H * W,), CANARY, dtype=torch.uint8, device=gpu_device)
    frames = flat[H * W:(N + 1) * H * W].view(N, H, W, 1)
    order = list(range(B, 0, -1))                  # frames B .. 1, frame 0 stays
    index = torch.tensor(order, dtype=torch.int32, device=gpu_device)
    pad = torch.full((B, H * W + 8), -7.25, device=gpu_device)
    src = pad[:, :H * W].unflatten(1, (1, H, W))
    src.copy_(planes)
    encode_gray(src, index, frames)
    torch.cuda.synchronize()
    got = frames.cpu()
    for b, n in enumerate(order):
        diff = int((got[n] != want[b]).sum())
        assert diff == 0, (b, n, diff)
    assert bool((got[0] == CANARY).all()) and bool((flat[:H * W] == CANARY).all()) and bool((flat[(N + 1) * H * W:] == CANARY).all())
    # a NaN in the plane: min and max are NaN (torch.min / torch.max), every pixel 0
    src[0, 0, 1, 1] = float("nan")
    encode_gray(src[:1], index[:1], frames)
    assert bool((frames[order[0]] == 0).all())


@pytest.mark.parametrize("residency", ["device", "host"])
@pytest.mark.parametrize("C", [3, 4])
def test_frame_writer(residency, C, gpu_device):
    from fdgs.frames import FrameStore, FrameWriter
    N, H, W = 7, 13, 18
    images = make_inputs(N, 3, H, W, seed=5)[0]
    alphas = make_inputs(N, 1, H, W, seed=6)[0] if C == 4 else None
    want = cpu_frames(images, alphas)
    di, da = images.to(gpu_device), (alphas.to(gpu_device) if C == 4 else None)
    w = FrameWriter(N, H, W, channels=C, residency=residency, slots=2, device=gpu_device)
    assert len(w) == N and w.shape == (H, W, C)
    with pytest.raises(RuntimeError, match="before finish"):
        w.frames
    for i in [4, 0, 6, 2, 5, 1, 3]:                # singly, shuffled: 7 frames through 2 slots
        w.write(i, di[i], None if da is None else da[i])
    assert w.launches == 7
    out = w.finish()
    assert out is w.frames and tuple(out.shape) == (N, H, W, C) and out.dtype == torch.uint8
    assert out.is_pinned() if residency == "host" else out.is_cuda
    assert torch.equal(out.cpu(), want)
    # batches: 3 + 4 frames; host residency cuts a batch into runs of `slots`
    w2 = FrameWriter(N, H, W, channels=C, residency=residency, slots=2, device=gpu_device)
    w2.write_batch(3, di[3:], None if da is None else da[3:])
    w2.write_batch(0, di[:3], None if da is None else da[:3])
    assert w2.launches == (2 if residency == "device" else 4)
    with pytest.raises(RuntimeError, match="before finish"):
        w2.frames
    assert torch.equal(w2.finish().cpu(), want)
    # what comes out is what a FrameStore takes
    store = FrameStore(w2.frames, residency=residency, device=gpu_device)
    assert len(store) == N and store.shape == (H, W, C)


def test_frame_writer_grey_and_default_ring(gpu_device):
    from fdgs.frames import FrameWriter
    N, H, W = 5, 16, 18
    planes = torch.rand(N, 1, H, W, generator=torch.Generator().manual_seed(8)) * 3.0
    want = cpu_gray(planes)
    dp = planes.to(gpu_device)
    for residency in ("device", "host"):
        w = FrameWriter(N, H, W, channels=1, residency=residency, device=gpu_device)
        assert w.slots == (N if residency == "device" else 2)
        w.write_gray(3, dp[3:])
        for i in (2, 0, 1):
            w.write_gray(i, dp[i])
        assert torch.equal(w.finish().cpu(), want), residency


def test_invalid_arguments_raise_without_a_launch(gpu_device):
    from fdgs import _capi
    from fdgs.frames import FrameWriter, encode_frames, encode_gray
    dev = gpu_device
    H, W = 13, 18
    img = torch.rand(2, 3, H, W, device=dev)
    idx = torch.zeros(2, dtype=torch.int32, device=dev)
    frames = torch.full((3, H, W, 3), CANARY, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="channels"):
        encode_frames(img, idx, torch.zeros((3, H, W, 2), dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match="GPU tensor"):
        encode_frames(img.cpu(), idx, frames)
    with pytest.raises(ValueError, match="GPU tensor"):
        encode_frames(img, idx.cpu(), frames)
    with pytest.raises(ValueError, match="GPU tensor"):
        encode_frames(img, idx, frames.cpu())
    with pytest.raises(ValueError, match="int32"):
        encode_frames(img, idx.long(), frames)
    with pytest.raises(ValueError, match="images must be float32"):
        encode_frames(img[:1], idx, frames)
    with pytest.raises(ValueError, match="images must be float32"):
        encode_frames(img.double(), idx, frames)
    with pytest.raises(ValueError, match="alphas go with RGBA"):
        encode_frames(img, idx, frames, torch.ones(2, 1, H, W, device=dev))
    with pytest.raises(ValueError, match="alphas go with RGBA"):
        encode_frames(img, idx, torch.zeros((3, H, W, 4), dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match="one channel"):
        encode_gray(img[:, :1], idx, frames)
    # the C entry points themselves: FDGS_ERR_INVALID_ARG, nothing launched
    f = _capi.lib.fdgs_frames_encode
    HW = H * W
    assert f(img.data_ptr(), 3 * HW, None, 0, 2, H, W, 2, frames.data_ptr(), 3, idx.data_ptr(), None) == 1 and "C must be" in _capi.last_error()
    assert f(img.data_ptr(), 3 * HW, None, 0, 2, H, W, 3, frames.data_ptr(), 3, None, None) == 1 and "missing pointer" in _capi.last_error()
    assert f(img.data_ptr(), 3 * HW, None, 0, 2, H, W, 4, frames.data_ptr(), 3, idx.data_ptr(), None) == 1 and "missing pointer" in _capi.last_error()
    assert f(img.data_ptr(), 3 * HW - 1, None, 0, 2, H, W, 3, frames.data_ptr(), 3, idx.data_ptr(), None) == 1 and "image_stride" in _capi.last_error()
    assert f(img.data_ptr(), 3 * HW, None, 0, 65536, H, W, 3, frames.data_ptr(), 3, idx.data_ptr(), None) == 1 and "bad sizes" in _capi.last_error()
    assert f(img.data_ptr(), 3 * HW, None, 0, 2, 65536, 65536, 3, frames.data_ptr(), 3, idx.data_ptr(), None) == 1 and "bad sizes" in _capi.last_error()
    gq = _capi.lib.fdgs_frames_encode_gray
    assert gq(img.data_ptr(), HW, 2, H, W, frames.data_ptr(), 3, idx.data_ptr(), None, None) == 1 and "missing pointer" in _capi.last_error()
    assert gq(img.data_ptr(), HW - 1, 2, H, W, frames.data_ptr(), 3, idx.data_ptr(), idx.data_ptr(), None) == 1 and "plane_stride" in _capi.last_error()
    assert _capi.lib.fdgs_frames_encode_gray_scratch_bytes(0, H, W) == -1 and _capi.lib.fdgs_frames_encode_gray_scratch_bytes(2, H, W) == 16
    # the writer
    with pytest.raises(ValueError, match="residency"):
        FrameWriter(3, H, W, residency="disk")
    with pytest.raises(ValueError, match="channels"):
        FrameWriter(3, H, W, channels=2)
    with pytest.raises(ValueError, match="empty"):
        FrameWriter(0, H, W)
    for residency in ("device", "host"):
        w = FrameWriter(3, H, W, residency=residency, device=dev)
        with pytest.raises(ValueError, match="out of range"):
            w.write(3, img[0])
        with pytest.raises(ValueError, match="out of range"):
            w.write_batch(2, img)
        with pytest.raises(ValueError, match="images must be float32"):
            w.write(0, img[0, :, :-1])
        with pytest.raises(ValueError, match="images must be float32"):
            w.write(0, img[0].double())
        with pytest.raises(ValueError, match="alphas go with 4 channels"):
            w.write(0, img[0], img[0, :1])
        with pytest.raises(ValueError, match="grey writer"):
            w.write_gray(0, img[0, :1])
        assert w.launches == 0
    torch.cuda.synchronize()
    assert bool((frames == CANARY).all())
