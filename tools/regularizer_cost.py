"""Times the k-NN query (k = 20), the rigid / motion regulariser forward and backward and the opacity-mask kernel at C3
(300 k Gaussians, 1352 x 1014) on the GPU.  Prints one JSON line of medians in milliseconds.

    python tools/regularizer_cost.py [--reps 50]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _median_ms(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--config", default="C3")
    args = ap.parse_args()
    from fdgs import _capi, synth, train_host
    from fdgs.knn import knn
    from fdgs.loss import opa_mask_loss, rigid_motion_loss

    dev = torch.device("cuda:0")
    scene = synth.make_scene(synth.CONFIGS[args.config], seed=0)
    m = train_host.ReferenceStyleModel(scene, dev)
    P, k = int(m._xyz.shape[0]), 20
    xyz = m._xyz.detach()[None]
    out = {"config": args.config, "P": P, "k": k}
    out["knn_ms"] = _median_ms(lambda: knn(xyz, xyz, k), args.reps)

    # the regulariser's own kernels, on a fixed k-NN result
    idx, d2 = knn(xyz, xyz, k)
    ins = [t.detach().contiguous() for t in (m._scaling, m._scaling_t, m._rotation, m._rotation_r, m._t)]
    vel = torch.empty(P, 3, device=dev)
    losses = torch.empty(2, device=dev)
    g = torch.ones(2, device=dev)
    grads = [torch.zeros_like(t) for t in ins[:4]]
    scratch = torch.empty(_capi.lib.fdgs_rigid_motion_scratch_bytes(P, k), dtype=torch.uint8, device=dev)
    stream = _capi.current_stream_handle(dev)

    def fwd():
        _capi._check(_capi.lib.fdgs_rigid_motion_forward(P, k, *[t.data_ptr() for t in ins], idx.data_ptr(), d2.data_ptr(), vel.data_ptr(),
                                                         losses.data_ptr(), scratch.data_ptr(), stream), "forward")

    def bwd():
        _capi._check(_capi.lib.fdgs_rigid_motion_backward(P, k, *[t.data_ptr() for t in ins], idx.data_ptr(), d2.data_ptr(), vel.data_ptr(),
                                                          g.data_ptr(), 1.0, *[t.data_ptr() for t in grads], scratch.data_ptr(), stream),
                     "backward")
    out["regularizer_fwd_ms"] = _median_ms(fwd, args.reps)
    out["regularizer_bwd_ms"] = _median_ms(bwd, args.reps)

    def full():
        lr, lm = rigid_motion_loss(m, k)
        (lr + lm).backward()
    out["rigid_motion_loss_fwd_bwd_ms"] = _median_ms(full, args.reps)

    H, W = scene["H"], scene["W"]
    alpha = torch.rand(1, H, W, device=dev)
    mask = (torch.rand(1, H, W, device=dev) > 0.5).float()
    nparts = _capi.lib.fdgs_opa_mask_num_partials(H, W)
    parts = torch.empty(nparts, device=dev)
    gout = torch.empty_like(alpha)
    val = torch.empty(1, device=dev)
    out["opa_mask_value_and_grad_ms"] = _median_ms(lambda: _capi._check(_capi.lib.fdgs_opa_mask_loss(
        H, W, alpha.data_ptr(), 0, mask.data_ptr(), None, 1.0, gout.data_ptr(), 0, parts.data_ptr(), val.data_ptr(), stream), "opa"), args.reps)
    a = alpha.clone().requires_grad_(True)
    out["opa_mask_loss_autograd_ms"] = _median_ms(lambda: opa_mask_loss(a, mask).backward(), args.reps)
    out["knn_plus_regularizer_ms"] = out["knn_ms"] + out["regularizer_fwd_ms"] + out["regularizer_bwd_ms"]

    # the four-view StepPipeline step with lego's weights (configs/dnerf/lego.yaml: lambda_rigid 1.0) against the plain step
    from fdgs.pipeline import StepPipeline
    del m
    pipe, bg = train_host.PipelineFlags(), torch.tensor([0.1, 0.2, 0.3], device=dev)
    cams = [train_host.SyntheticCamera(scene, dev, timestamp=(b + 0.5) / 4 * scene["time_duration"]) for b in range(4)]
    gen = torch.Generator(device="cpu").manual_seed(7)
    gts = [torch.rand(3, H, W, generator=gen).to(dev) for _ in range(4)]
    for name, kw in (("step_plain_ms", {}), ("step_lego_rigid_ms", dict(lambda_rigid=1.0))):
        gp = train_host.GaussianParams(scene, dev)
        sp = StepPipeline(gp, train_host.make_optimizer(gp), world_size=1, lambda_dssim=0.2, **kw)
        out[name] = _median_ms(lambda: sp.step(cams, gts, pipe, bg), args.reps)
        del sp, gp
    print(json.dumps({kk: (round(v, 4) if isinstance(v, float) else v) for kk, v in out.items()}))


if __name__ == "__main__":
    main()
