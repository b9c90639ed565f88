"""Depth supervision on a synthetic scene: three training cameras, a depth prior per view that is the ground-truth depth put through
an unknown affine map plus noise (what a monocular depth network gives), trained once without and once with the depth term.

    python examples/train_with_depth.py --iterations 300
    python examples/train_with_depth.py --bench          # the new kernels at 1352 x 1014 next to their PyTorch formulation

Prints the held-out PSNR and the held-out depth error after alignment (the scale-and-shift-invariant L1 against the true depth) of
both runs.  The depth terms reach the model through render_raw() + autograd: fdgs.depth.depth_loss and depth_normals are
torch.autograd.Functions whose gradients enter the rasterizer backward as dL/d depth and dL/d alpha.
"""
import argparse, math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

TRAIN_POSES, TEST_POSE = ("rig0", "rig1", "rig3"), "rig2"


def _camera(scene, pose, dev):
    from fdgs import synth, train_host
    return train_host.SyntheticCamera(dict(scene, **synth.camera_for(pose, scene["W"], scene["H"])), dev)


def run(dev, iterations=300, lambda_depth=0.5, lambda_normal=0.0, mode="ssi", W=200, H=152, P=4000, s0=0.08, seed=0, log=print):
    """Trains a perturbed copy of a fdgs.synth scene from three cameras; returns a dict of the held-out PSNR, the held-out aligned depth
    error, and the training views' aligned depth error before and after."""
    from fdgs import depth, synth, train_host
    from fdgs.fused import render_raw
    from fdgs.loss import fused_l1_ssim
    cfg = synth.SceneConfig("depth", P, W, H, 1, 0, s0, 1.0, True, 4, True)
    scene = synth.make_scene(cfg, seed=seed)
    pipe, bg = train_host.PipelineFlags(), scene["bg"].to(dev)
    target = train_host.GaussianParams(scene, dev)
    cams, tcam = [_camera(scene, p, dev) for p in TRAIN_POSES], _camera(scene, TEST_POSE, dev)
    intr = [depth.intrinsics_of(c) for c in cams]
    g = torch.Generator().manual_seed(seed + 1)
    gts, priors, normal_priors = [], [], []
    with torch.no_grad():
        for v, c in enumerate(cams + [tcam]):
            pkg = render_raw(c, target, pipe, bg)
            ok = pkg["alpha"] >= 0.5
            z = torch.where(ok, pkg["depth"] / pkg["alpha"].clamp(min=0.5), torch.zeros_like(pkg["depth"]))
            gts.append((pkg["render"].clone(), z))
            if v < len(cams):
                s, b = 0.4 + 0.3 * v, 0.5 + 1.0 * v            # unknown to the trainer, different in every view
                noise = 0.03 * torch.randn(z.shape, generator=g).to(dev)
                priors.append(torch.where(ok, s * z + b + noise, torch.zeros_like(z)))      # 0: no prior there
                normal_priors.append(depth.depth_normals(pkg["depth"], pkg["alpha"], intr[v])[0])
    student = train_host.GaussianParams(scene, dev)
    with torch.no_grad():
        student.params["_xyz"].add_(0.05 * torch.randn(student.params["_xyz"].shape, generator=g).to(dev))
        student.params["_features"].add_(0.2 * torch.randn(student.params["_features"].shape, generator=g).to(dev))
        student.params["_opacity"].add_(0.5 * torch.randn(student.params["_opacity"].shape, generator=g).to(dev))
    del target
    opt = train_host.make_optimizer(student)

    def aligned_error(cam, z_true):
        with torch.no_grad():
            pkg = render_raw(cam, student, pipe, bg)
            return depth.depth_loss(pkg["depth"], pkg["alpha"], z_true, mode="ssi")

    def train_error():
        return float(sum(aligned_error(c, gts[v][1]) for v, c in enumerate(cams))) / len(cams)
    before = train_error()
    for it in range(iterations):
        v = it % len(cams)
        student.zero_grad()
        pkg = render_raw(cams[v], student, pipe, bg)
        loss = fused_l1_ssim(pkg["render"], gts[v][0], 0.2)
        if lambda_depth:
            loss = loss + lambda_depth * depth.depth_loss(pkg["depth"], pkg["alpha"], priors[v], mode=mode)
        if lambda_normal:
            n, valid = depth.depth_normals(pkg["depth"], pkg["alpha"], intr[v])
            loss = loss + lambda_normal * depth.normal_loss(n, valid, normal_priors[v])
        loss.backward()
        opt.step()
        if log and (it + 1) % max(1, iterations // 5) == 0:
            log("  iteration %4d  loss %.5f" % (it + 1, float(loss.detach())))
    with torch.no_grad():
        img = render_raw(tcam, student, pipe, bg)["render"]
        mse = float(((img.clamp(0, 1) - gts[-1][0].clamp(0, 1)) ** 2).mean())
    return {"heldout_psnr": -10.0 * math.log10(max(mse, 1e-12)), "heldout_depth_error": float(aligned_error(tcam, gts[-1][1])),
            "train_depth_error_before": before, "train_depth_error_after": train_error()}


# ---- the PyTorch formulation of the same terms (float32, on the GPU), for --bench ----
def torch_depth_loss(depth, alpha, prior, mode, alpha_min=0.5):
    ok = (alpha >= alpha_min) & torch.isfinite(prior) & (prior > 0)
    v = ok.float()
    z = torch.where(ok, depth / torch.where(ok, alpha, torch.ones_like(alpha)), torch.zeros_like(depth))
    p = torch.where(ok, prior, torch.zeros_like(prior))
    n = v.sum()
    zm, pm = z.sum() / n, p.sum() / n
    dz, dp = (z - zm) * v, (p - pm) * v
    vz, vp, cov = (dz * dz).sum() / n, (dp * dp).sum() / n, (dz * dp).sum() / n
    if mode == "pearson":
        return 1.0 - cov / torch.sqrt(vz * vp)
    s = (cov / vz).detach()
    b = (pm - s * zm).detach()
    return ((s * z + b - p) * v).abs().sum() / n


def torch_depth_normals(depth, alpha, intr, alpha_min=0.5):
    fl_x, fl_y, cx, cy = intr
    ok = (alpha >= alpha_min)[0]
    z = (depth / torch.where(alpha >= alpha_min, alpha, torch.ones_like(alpha)))[0]
    H, W = z.shape
    xs = (torch.arange(W, dtype=torch.float32, device=z.device) + 0.5 - cx) / fl_x
    ys = (torch.arange(H, dtype=torch.float32, device=z.device) + 0.5 - cy) / fl_y
    P = torch.stack([xs[None, :] * z, ys[:, None] * z, z])
    a, b = P[:, 1:-1, 2:] - P[:, 1:-1, :-2], P[:, 2:, 1:-1] - P[:, :-2, 1:-1]
    N = torch.linalg.cross(b, a, dim=0)
    len2 = (N * N).sum(0)
    v = ok[1:-1, 1:-1] & ok[1:-1, 2:] & ok[1:-1, :-2] & ok[2:, 1:-1] & ok[:-2, 1:-1] & (len2 > 1e-20)
    n = torch.where(v[None], N / torch.sqrt(torch.where(v, len2, torch.ones_like(len2)))[None], torch.zeros_like(N))
    return torch.nn.functional.pad(n, (1, 1, 1, 1)), torch.nn.functional.pad(v, (1, 1, 1, 1))[None]


def bench(dev, W=1352, H=1014, reps=50):
    """The kernels alone (the C calls back to back on one stream, events around ``reps`` calls), with the bytes of the float32 images a
    call reads and writes over that time; then value + gradient through autograd, the kernels next to their PyTorch formulation.
    Bytes per pixel: a loss reads depth, alpha, prior twice (moments, gradient) and writes two gradients: 32; the normals read depth and
    alpha and write 3 floats and a byte: 21; their backward reads depth, alpha, dL/dn and writes two gradients: 28."""
    import ctypes as C
    from fdgs import _capi, depth
    g = torch.Generator().manual_seed(0)
    z = 2.0 + torch.rand(1, H, W, generator=g).to(dev) * 4.0
    alpha = (0.4 + 0.6 * torch.rand(1, H, W, generator=g)).to(dev)
    d = (z * alpha).contiguous()
    prior = (0.6 * z + 1.0 + 0.05 * torch.randn(1, H, W, generator=g).to(dev)).contiguous()
    intr = (0.9 * W, 0.9 * W, 0.5 * W, 0.5 * H)
    w = torch.randn(3, H, W, generator=g).to(dev)
    px = H * W

    def timed(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize(dev)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize(dev)
        return a.elapsed_time(b) / reps * 1e3       # microseconds

    din = _capi.FdgsDepthIn(H, W, d.data_ptr(), alpha.data_ptr(), None, 0.5)
    gd, ga = torch.empty_like(d), torch.empty_like(d)
    grads = _capi.FdgsDepthGrads(gd.data_ptr(), ga.data_ptr(), None, 1.0, 0)
    parts = torch.empty(_capi.lib.fdgs_depth_loss_num_partials(H, W), dtype=torch.float64, device=dev)
    out = torch.empty(4, dtype=torch.float32, device=dev)
    normals, valid = torch.empty(3, H, W, device=dev), torch.empty(1, H, W, dtype=torch.uint8, device=dev)
    st = _capi.current_stream_handle(dev)
    lib = _capi.lib
    raw = (("fdgs_depth_loss pearson", lambda: lib.fdgs_depth_loss(C.byref(din), prior.data_ptr(), 0, C.byref(grads), parts.data_ptr(), out.data_ptr(), st), 32),
           ("fdgs_depth_loss ssi", lambda: lib.fdgs_depth_loss(C.byref(din), prior.data_ptr(), 1, C.byref(grads), parts.data_ptr(), out.data_ptr(), st), 32),
           ("fdgs_depth_normals", lambda: lib.fdgs_depth_normals(C.byref(din), *intr, None, normals.data_ptr(), valid.data_ptr(), st), 21),
           ("fdgs_depth_normals_backward", lambda: lib.fdgs_depth_normals_backward(C.byref(din), *intr, None, w.data_ptr(), C.byref(grads), st), 28))
    rows = []
    with torch.cuda.device(dev):
        for name, fn, bpp in raw:
            us = timed(fn)
            rows.append((name, us, bpp * px / (us * 1e-6) / 1e9))
            print("%-28s %dx%d: %7.1f us per call, %6.0f GB/s of the %.1f MB of images it moves" % (name, W, H, us, rows[-1][2], bpp * px / 1e6))

    def value_and_grad(loss_of):
        def fn():
            dd, aa = d.detach().requires_grad_(True), alpha.detach().requires_grad_(True)
            loss_of(dd, aa).backward()
        return fn
    for name, hip, ref in (
            ("pearson", lambda dd, aa: depth.depth_loss(dd, aa, prior, mode="pearson"), lambda dd, aa: torch_depth_loss(dd, aa, prior, "pearson")),
            ("ssi", lambda dd, aa: depth.depth_loss(dd, aa, prior, mode="ssi"), lambda dd, aa: torch_depth_loss(dd, aa, prior, "ssi")),
            ("normals", lambda dd, aa: (depth.depth_normals(dd, aa, intr)[0] * w).sum(), lambda dd, aa: (torch_depth_normals(dd, aa, intr)[0] * w).sum())):
        t_hip, t_ref = timed(value_and_grad(hip)), timed(value_and_grad(ref))
        rows.append((name + " autograd", t_hip, t_ref))
        print("%-28s %dx%d: value + gradient through autograd %7.1f us, PyTorch formulation %8.1f us (%.1f x)" % (name, W, H, t_hip, t_ref, t_ref / t_hip))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=300)
    ap.add_argument("--lambda-depth", type=float, default=0.5)
    ap.add_argument("--lambda-normal", type=float, default=0.0)
    ap.add_argument("--mode", choices=("pearson", "ssi"), default="ssi")
    ap.add_argument("--bench", action="store_true", help="time the new kernels at 1352 x 1014 next to their PyTorch formulation")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    if args.bench:
        bench(dev)
        return
    for label, lam_d, lam_n in (("without the depth term", 0.0, 0.0), ("with the depth term", args.lambda_depth, args.lambda_normal)):
        print(label)
        r = run(dev, args.iterations, lam_d, lam_n, args.mode)
        print("  held-out PSNR %.2f dB, held-out depth error after alignment %.4f (training views: %.4f -> %.4f)" % (
            r["heldout_psnr"], r["heldout_depth_error"], r["train_depth_error_before"], r["train_depth_error_after"]))


if __name__ == "__main__":
    main()
