"""GPU: fdgs.frames -- the decode kernel against the reference loader's own results (tests/golden/frames) and the CPU expression
``u8 / 255``, and the FrameStore's ring on the device and from pinned host memory.  Every comparison is bitwise: the operations are
fixed and IEEE, there is no tolerance anywhere."""
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "frames", "*.npz")))
CANARY = -7.25


def cpu_decode(u8):
    """The CPU expression: torch's true division of the bytes by 255, [N, H, W, C] -> images [N, 3, H, W], masks [N, 1, H, W] / None."""
    q = (u8.cpu() / 255.0).permute(0, 3, 1, 2).contiguous()
    assert q.dtype == torch.float32
    if q.shape[1] == 3:
        return q, None
    return (q[:, :3] * q[:, 3:4]).contiguous(), q[:, 3:4].contiguous()


def _decode_into_canaries(u8_dev, order, with_mask):
    """decode_frames into slots 1 .. B of B + 2 padded slots filled with a canary; returns (images, masks, untouched?)."""
    from fdgs.frames import decode_frames
    dev = u8_dev.device
    N, H, W, Cn = u8_dev.shape
    B, pad = len(order), 24
    ring = torch.full((B + 2, 3 * H * W + pad), CANARY, device=dev)
    mring = torch.full((B + 2, H * W + pad), CANARY, device=dev)
    out = ring[1:B + 1, :3 * H * W].unflatten(1, (3, H, W))
    mk = mring[1:B + 1, :H * W].unflatten(1, (1, H, W)) if with_mask else None
    index = torch.tensor(order, dtype=torch.int32, device=dev)
    assert decode_frames(u8_dev, index, out, mk) is out
    torch.cuda.synchronize()
    clean = bool((ring[0] == CANARY).all() and (ring[B + 1] == CANARY).all() and (ring[1:B + 1, 3 * H * W:] == CANARY).all())
    if with_mask:
        clean = clean and bool((mring[0] == CANARY).all() and (mring[B + 1] == CANARY).all() and (mring[1:B + 1, H * W:] == CANARY).all())
    else:
        clean = clean and bool((mring == CANARY).all())
    return out.cpu(), None if mk is None else mk.cpu(), clean


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_decode_equals_the_reference_loader(path, gpu_device):
    d = np.load(path)
    u8 = torch.from_numpy(d["u8"]).to(gpu_device)
    N, rgba = u8.shape[0], u8.shape[3] == 4
    want, want_mask = torch.from_numpy(d["image"]), (torch.from_numpy(d["mask"]) if rgba else None)
    orders = [list(range(N)), [N - 1, 0, N - 1, 1 % N, 0], [N - 1]]      # in order; permuted with repeats; B = 1
    for order in orders:
        for with_mask in ((True, False) if rgba else (False,)):
            img, mk, clean = _decode_into_canaries(u8, order, with_mask)
            assert clean, "decode_frames wrote outside the addressed slots (%s)" % (order,)
            assert torch.equal(img, want[order]), (order, with_mask)
            if with_mask:
                assert torch.equal(mk, want_mask[order]), order


def test_every_byte_and_every_colour_alpha_pair(gpu_device):
    """All 256 bytes in an RGB frame and all 65 536 (colour, alpha) pairs in an RGBA frame against ``torch.arange(...) / 255.0`` on the
    CPU: a kernel that multiplies by 1/255 misses 126 of the bytes, one that divides u * a by 65025 misses 37 247 of the pairs."""
    from fdgs.frames import decode_frames
    b = torch.arange(256, dtype=torch.uint8)
    rgb = torch.stack([b, b.flip(0), b.roll(77)], -1).reshape(1, 16, 16, 3)
    out = torch.empty((1, 3, 16, 16), device=gpu_device)
    decode_frames(rgb.to(gpu_device), torch.zeros(1, dtype=torch.int32, device=gpu_device), out)
    unit = torch.arange(256, dtype=torch.float32) / 255.0
    want = torch.stack([unit, unit.flip(0), unit.roll(77)]).reshape(1, 3, 16, 16)
    assert torch.equal(out.cpu(), want)
    col, al = torch.meshgrid(b, b, indexing="ij")
    rgba = torch.stack([col, col.flip(0), col.roll(31, 0), al], -1)[None].contiguous()      # [1, 256, 256, 4]
    out = torch.empty((1, 3, 256, 256), device=gpu_device)
    mk = torch.empty((1, 1, 256, 256), device=gpu_device)
    decode_frames(rgba.to(gpu_device), torch.zeros(1, dtype=torch.int32, device=gpu_device), out, mk)
    c, a = unit[:, None].expand(256, 256), unit[None, :].expand(256, 256)
    want = torch.stack([c * a, c.flip(0) * a, c.roll(31, 0) * a])[None]
    assert torch.equal(mk.cpu()[0, 0], a)
    assert torch.equal(out.cpu(), want), int((out.cpu() != want).sum())


def test_a_batch_of_full_size_frames(gpu_device):
    """Four 1014 x 1352 RGB frames (the benchmark's image size) out of six, random bytes."""
    from fdgs.frames import decode_frames
    g = torch.Generator().manual_seed(11)
    u8 = torch.randint(0, 256, (6, 1014, 1352, 3), generator=g, dtype=torch.uint8)
    order = [4, 1, 5, 2]
    out = torch.empty((4, 3, 1014, 1352), device=gpu_device)
    decode_frames(u8.to(gpu_device), torch.tensor(order, dtype=torch.int32, device=gpu_device), out)
    want, _ = cpu_decode(u8[order])
    assert torch.equal(out.cpu(), want)


def _store_frames(N=7, H=13, W=18, Cn=4, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (N, H, W, Cn), generator=g, dtype=torch.uint8)


@pytest.mark.parametrize("residency", ["device", "host"])
@pytest.mark.parametrize("Cn", [3, 4])
def test_frame_store(residency, Cn, gpu_device):
    from fdgs.frames import FrameStore
    u8 = _store_frames(Cn=Cn)
    want, want_mask = cpu_decode(u8)
    store = FrameStore(u8.numpy(), residency=residency, slots=4, device=gpu_device)
    assert len(store) == 7 and store.shape == (13, 18, Cn) and store.has_alpha == (Cn == 4)
    assert store.frames.is_pinned() if residency == "host" else store.frames.is_cuda
    # batch, one launch
    got = store.batch([2, 5])
    assert store.launches == 1 and [tuple(t.shape) for t in got] == [(3, 13, 18)] * 2 and all(t.is_contiguous() for t in got)
    assert torch.equal(got[0].cpu(), want[2]) and torch.equal(got[1].cpu(), want[5])
    # __getitem__, negative index, IndexError past the end (the sequence protocol)
    assert torch.equal(store[6].cpu(), want[6]) and torch.equal(store[-7].cpu(), want[0])
    with pytest.raises(IndexError):
        store[7]
    # the four slots have been handed out once: `got` is still what it was, one more frame overwrites its first tensor
    assert torch.equal(got[0].cpu(), want[2])
    first = store.batch([3])[0]
    assert first.data_ptr() == got[0].data_ptr() and torch.equal(got[0].cpu(), want[3]) and torch.equal(got[1].cpu(), want[5])
    # prefetch then batch; batch without prefetch; a prefetch that is never asked for
    store.prefetch([1, 4])
    a = store.batch([1, 4])              # slots 1, 2
    b = store.batch([0, 0])              # a repeat, no prefetch; slots 3 and 0: the ring wraps inside the batch (two launches)
    assert store.launches == 7
    store.prefetch([6, 2])
    c = store.batch([5])                 # not the prefetched batch: uploaded on the spot; slot 1 = a[0]
    for t, f in zip([a[1]] + b + c + [a[0]], [4, 0, 0, 5, 5]):
        assert torch.equal(t.cpu(), want[f]), f
    # more fetches than slots: the later tensors are right, the earlier ones hold later frames
    seq = [0, 1, 2, 3, 4, 5, 6, 0]
    held = [store[f] for f in seq]
    for k in range(len(seq) - 4, len(seq)):
        assert torch.equal(held[k].cpu(), want[seq[k]]), k
    assert held[0].data_ptr() == held[4].data_ptr() and torch.equal(held[0].cpu(), want[seq[4]])
    # two consecutive prefetch / batch rounds that reuse the staging slots (2 x 3 frames through a ring of 4)
    store.prefetch([4, 5, 6])
    x = [t.clone() for t in store.batch([4, 5, 6])]
    store.prefetch([2, 1, 0])
    y = [t.clone() for t in store.batch([2, 1, 0])]
    store.prefetch([3, 3, 6])
    z = store.batch([3, 3, 6])
    for t, f in zip(x + y + z, [4, 5, 6, 2, 1, 0, 3, 3, 6]):
        assert torch.equal(t.cpu(), want[f]), f
    if Cn == 4:
        store.prefetch([6, 0])
        ims, mks = store.batch([6, 0], masks=True)
        assert [tuple(m.shape) for m in mks] == [(1, 13, 18)] * 2
        for im, mk, f in zip(ims, mks, [6, 0]):
            assert torch.equal(im.cpu(), want[f]) and torch.equal(mk.cpu(), want_mask[f])
        assert torch.equal(store.masks([3])[0].cpu(), want_mask[3])
    else:
        with pytest.raises(ValueError, match="alpha"):
            store.batch([0], masks=True)


def test_frame_store_default_ring_and_launch_count(gpu_device):
    """Without ``slots`` the ring is twice the first batch (at least 2; ``reserve`` = what harness.train asks for): a batch never wraps
    it, so every batch is ONE launch; a list of arrays builds the same store."""
    from fdgs.frames import FrameStore
    u8 = _store_frames(N=9, Cn=3)
    want, _ = cpu_decode(u8)
    store = FrameStore([f.numpy() for f in u8], device=gpu_device)
    store.reserve(3)
    assert store.slots == 6
    for k in range(5):
        idx = [(3 * k + j) % 9 for j in range(3)]
        got = store.batch(idx)
        assert store.launches == k + 1
        for t, f in zip(got, idx):
            assert torch.equal(t.cpu(), want[f])
    one = FrameStore(u8, device=gpu_device)
    assert torch.equal(one[4].cpu(), want[4]) and one.slots == 2
    one.reserve(4)     # a ring that was sized by default grows
    assert one.slots == 8 and torch.equal(one.batch([8, 7, 6, 5])[3].cpu(), want[5])


def test_invalid_arguments_raise_without_a_launch(gpu_device):
    from fdgs import _capi
    from fdgs.frames import FrameStore, decode_frames
    dev = gpu_device
    u8 = _store_frames(N=3, Cn=3).to(dev)
    idx = torch.zeros(2, dtype=torch.int32, device=dev)
    out = torch.full((2, 3, 13, 18), CANARY, device=dev)
    with pytest.raises(ValueError, match="channels"):
        decode_frames(torch.zeros((3, 13, 18, 2), dtype=torch.uint8, device=dev), idx, out)
    with pytest.raises(ValueError, match="GPU tensor"):
        decode_frames(u8, idx.cpu(), out)
    with pytest.raises(ValueError, match="GPU tensor"):
        decode_frames(u8.cpu(), idx, out)
    with pytest.raises(ValueError, match="GPU tensor"):
        decode_frames(u8, idx, out.cpu())
    with pytest.raises(ValueError, match="int32"):
        decode_frames(u8, idx.long(), out)
    with pytest.raises(ValueError, match="out must be float32"):
        decode_frames(u8, idx, out[:1])
    with pytest.raises(ValueError, match="out must be float32"):
        decode_frames(u8, idx, out.double())
    with pytest.raises(ValueError, match="mask_out needs RGBA"):
        decode_frames(u8, idx, out, torch.empty((2, 1, 13, 18), device=dev))
    # the C entry point itself: FDGS_ERR_INVALID_ARG, nothing launched
    f = _capi.lib.fdgs_frames_decode
    assert f(u8.data_ptr(), 3, 13, 18, 2, idx.data_ptr(), 2, out.data_ptr(), 3 * 13 * 18, None, 0, None) == 1
    assert f(u8.data_ptr(), 3, 13, 18, 3, None, 2, out.data_ptr(), 3 * 13 * 18, None, 0, None) == 1
    assert f(u8.data_ptr(), 3, 13, 18, 3, idx.data_ptr(), 2, out.data_ptr(), 3 * 13 * 18 - 1, None, 0, None) == 1
    store = FrameStore(u8, slots=2)
    for bad in ([3], [0, -4]):
        with pytest.raises(ValueError, match="out of range"):
            store.batch(bad)
        with pytest.raises(ValueError, match="out of range"):
            store.prefetch(bad)
    with pytest.raises(ValueError, match="does not fit a ring of 2 slots"):
        store.batch([0, 1, 2])
    with pytest.raises(ValueError, match="does not fit a ring of 2 slots"):
        store.reserve(4)
    assert store.launches == 0
    torch.cuda.synchronize()
    assert bool((out == CANARY).all())
