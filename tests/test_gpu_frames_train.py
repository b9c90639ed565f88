"""GPU: harness.train and metrics.evaluate fed from a FrameStore (fdgs.frames) against the same calls fed with the float tensors
``u8 / 255``.  Same kernels on the same numbers in the same batch order, so the bar is the one tests/test_gpu_api.py applies to two runs
of ONE pipeline (float-atomics noise, which grows behind every Adam step): the first step's loss at rtol 1e-6 / atol 1e-7 (identical
inputs), the later losses at rtol 1e-4 / atol 1e-6, the parameters by that file's statistic against what two runs from float tensors
differ by."""
import numpy as np
import pytest
import torch

from util import synth

pytestmark = pytest.mark.gpu
V, B, STEPS = 12, 4, 10


class Recording:
    """A camera list that remembers in which order its items were asked for: the sequence of batches a run drew."""

    def __init__(self, items):
        self.items, self.asked = list(items), []

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        self.asked.append(int(i))
        return self.items[i]


def _setup(dev, rgba):
    """A C1-sized scene, V cameras, and the ground truth as 8-bit frames [V, H, W, 3 or 4]: the target's renders quantised as
    examples/train_synthetic.py --u8-frames does; the alpha channel (rgba) is the target's own opacity, 0 .. 255."""
    from fdgs import train_host
    from fdgs.fused import render_raw
    scene = synth.make_scene(synth.CONFIGS["C1"], seed=0)
    pipe, bg = train_host.PipelineFlags(), scene["bg"].to(dev)
    target = train_host.GaussianParams(scene, dev)
    cams = [train_host.SyntheticCamera(scene, dev, timestamp=(v + 0.5) / V * scene["time_duration"]) for v in range(V)]
    frames = []
    with torch.no_grad():
        for c in cams:
            r = render_raw(c, target, pipe, bg)
            planes = [r["render"]]
            if rgba:   # stretched to the whole range, so that the masks hold 0, 1 and everything between
                al = r["alpha"].reshape(1, *r["render"].shape[1:])
                planes.append((al - al.min()) / (al.max() - al.min()))
            frames.append((torch.cat(planes).clamp(0, 1) * 255 + 0.5).to(torch.uint8).permute(1, 2, 0))
    u8 = torch.stack(frames).contiguous()
    return scene, cams, u8, pipe, bg


def _student(scene, dev):
    from fdgs import train_host
    m = train_host.GaussianParams(scene, dev)
    g = torch.Generator(device="cpu").manual_seed(1)
    with torch.no_grad():
        m.params["_features"].add_(0.3 * torch.randn(m.params["_features"].shape, generator=g).to(dev))
        m.params["_opacity"].add_(0.5 * torch.randn(m.params["_opacity"].shape, generator=g).to(dev))
    return m, train_host.make_optimizer(m)


def _floats(u8):
    """q = u8.float() / 255 by torch on the device, as a division by a device tensor (torch turns a division by a Python number into a
    product with its reciprocal on the GPU, which is not the loader's arithmetic): images [V, 3, H, W], masks [V, 1, H, W] or None."""
    q = (u8.float() / torch.tensor(255.0, device=u8.device)).permute(0, 3, 1, 2).contiguous()
    if q.shape[1] == 3:
        return q, None
    return (q[:, :3] * q[:, 3:4]).contiguous(), q[:, 3:4].contiguous()


def _run(scene, cams, gts, pipe, bg, dev, **kw):
    from fdgs import harness
    m, opt = _student(scene, dev)
    rec = Recording(cams)
    hist = harness.train(m, opt, rec, gts, pipe, bg, iterations=STEPS, batch_size=B, log_every=1, log=lambda s: None, **kw)
    torch.cuda.synchronize()
    assert hist["iteration"] == list(range(1, STEPS + 1))
    return {"loss": np.array(hist["loss"]), "psnr": np.array(hist["psnr"]), "flat": m.flat.detach().clone(), "feat": m.offsets["_features"],
            "batches": [rec.asked[k:k + B] for k in range(0, len(rec.asked), B)]}


def _same_run(got, want, again):
    """``got`` against ``want`` by tests/test_gpu_api.py's bars; ``again``: a second run of what ``want`` ran (the noise)."""
    assert got["batches"] == want["batches"] and len(got["batches"]) == STEPS and all(len(b) == B for b in got["batches"])
    print("loss", got["loss"], "\nwant", want["loss"], "\nrel", np.abs(got["loss"] - want["loss"]) / np.abs(want["loss"]),
          "\nnoise rel", np.abs(again["loss"] - want["loss"]) / np.abs(want["loss"]))
    np.testing.assert_allclose(got["loss"][:1], want["loss"][:1], rtol=1e-6, atol=1e-7)       # first step: identical inputs
    np.testing.assert_allclose(got["loss"], want["loss"], rtol=1e-4, atol=1e-6)               # what two runs of one pipeline differ by
    b, e = want["feat"]
    perr, noise = (got["flat"][b:e] - want["flat"][b:e]).abs(), (again["flat"][b:e] - want["flat"][b:e]).abs()
    print("features: frac > 1e-2", (perr > 1e-2).float().mean().item(), "noise", (noise > 1e-2).float().mean().item())
    assert (perr > 1e-2).float().mean().item() <= max(1e-3, 4.0 * (noise > 1e-2).float().mean().item()), (perr > 1e-2).float().mean().item()
    perr, noise = (got["flat"][:b] - want["flat"][:b]).abs(), (again["flat"][:b] - want["flat"][:b]).abs()
    print("geometry: frac > 2e-3", (perr > 2e-3).float().mean().item(), "noise", (noise > 2e-3).float().mean().item(), "max",
          perr.max().item(), "noise max", noise.max().item())
    assert (perr > 2e-3).float().mean().item() <= max(2e-3, 4.0 * (noise > 2e-3).float().mean().item()), (perr > 2e-3).float().mean().item()
    assert perr.max().item() <= max(0.25, 2.0 * noise.max().item())


def test_train_from_a_frame_store_equals_training_from_float_tensors(gpu_device):
    from fdgs.frames import FrameStore
    dev = gpu_device
    scene, cams, u8, pipe, bg = _setup(dev, rgba=False)
    q, _ = _floats(u8)
    check = FrameStore(u8, device=dev)
    assert all(torch.equal(check[v], q[v]) for v in range(V))       # the same numbers, bit for bit
    gts = list(q.unbind(0))
    want = _run(scene, cams, gts, pipe, bg, dev)
    again = _run(scene, cams, gts, pipe, bg, dev)
    assert again["batches"] == want["batches"]
    for residency in ("device", "host"):
        store = FrameStore(u8, residency=residency, device=dev)
        got = _run(scene, cams, store, pipe, bg, dev)
        assert store.slots == 2 * B and store.launches == STEPS     # one launch per step (the logging line uses the step's tensor)
        _same_run(got, want, again)


def test_train_takes_the_opacity_masks_from_an_rgba_store(gpu_device):
    from fdgs.frames import FrameStore
    dev = gpu_device
    scene, cams, u8, pipe, bg = _setup(dev, rgba=True)
    alpha = u8[..., 3]
    assert int(alpha.min()) == 0 and int(alpha.max()) == 255 and len(torch.unique(alpha)) > 100
    q, masks = _floats(u8)
    gts, mlist = list(q.unbind(0)), list(masks.unbind(0))
    want = _run(scene, cams, gts, pipe, bg, dev, lambda_opa_mask=0.5, alpha_masks=mlist)
    again = _run(scene, cams, gts, pipe, bg, dev, lambda_opa_mask=0.5, alpha_masks=mlist)
    plain = _run(scene, cams, gts, pipe, bg, dev)
    assert np.abs(plain["flat"].cpu().numpy() - want["flat"].cpu().numpy()).max() > 1e-4     # the term does something here
    for residency in ("device", "host"):
        got = _run(scene, cams, FrameStore(u8, residency=residency, device=dev), pipe, bg, dev, lambda_opa_mask=0.5)
        _same_run(got, want, again)


def test_evaluate_from_a_frame_store_is_bit_identical(gpu_device):
    from fdgs import train_host
    from fdgs.frames import FrameStore
    from fdgs.metrics import evaluate
    dev = gpu_device
    scene, cams, u8, pipe, bg = _setup(dev, rgba=False)
    q, _ = _floats(u8)
    model, _opt = _student(scene, dev)
    want = evaluate(model, cams, list(q.unbind(0)), pipe, bg)
    assert want["rows"].shape == (V, 4) and bool(torch.isfinite(want["rows"]).all())
    for residency in ("device", "host"):
        got = evaluate(model, cams, FrameStore(u8, residency=residency, device=dev), pipe, bg)     # 12 views through a ring of 2 slots
        assert torch.equal(got["rows"], want["rows"]), residency
        assert all(got[k] == want[k] for k in ("l1", "psnr", "ssim", "msssim", "views"))


def test_harness_evaluation_sets_from_frame_stores(gpu_device):
    """test_iterations with ``gts`` and ``test_gts`` both stores: the five training views and the test views go through rings of
    fewer slots than views, and the numbers equal the run from float tensors."""
    from fdgs import harness
    from fdgs.frames import FrameStore
    dev = gpu_device
    scene, cams, u8, pipe, bg = _setup(dev, rgba=False)
    q, _ = _floats(u8)
    tcams, tu8, tq = cams[1::4], u8[1::4].contiguous(), q[1::4]
    evs = []
    for mode in ("float", "host"):
        m, opt = _student(scene, dev)
        gts = list(q.unbind(0)) if mode == "float" else FrameStore(u8, residency="host", device=dev)
        tgts = list(tq.unbind(0)) if mode == "float" else FrameStore(tu8, residency="host", slots=2, device=dev)
        hist = harness.train(m, opt, cams, gts, pipe, bg, iterations=2, batch_size=B, test_cameras=tcams, test_gts=tgts, test_iterations=[1])
        evs.append(hist["eval"])
    assert [(e["set"], e["views"]) for e in evs[1]] == [("train", 5), ("test", 3)]
    for a, b in zip(evs[0], evs[1]):
        # the evaluated model is behind one Adam step, i.e. behind float-atomics noise: the later-losses bar of two runs of one pipeline
        for k in ("l1", "psnr", "ssim", "msssim"):
            np.testing.assert_allclose(b[k], a[k], rtol=1e-4, atol=1e-6)
