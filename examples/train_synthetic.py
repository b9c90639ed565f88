"""Frame-parallel training on a synthetic 4D scene (no dataset needed): ground truth is rendered from a target model,
a perturbed copy is trained back.  One process per GPU:

    python examples/train_synthetic.py --iterations 300
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 examples/train_synthetic.py

Uses fdgs.harness.train (FrameShard + StepPipeline + one gradient all-reduce per step over RCCL).
"""
import argparse, math, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if int(os.environ.get("WORLD_SIZE", "1")) > 1:
    # the step's own streams fill the runtime's default of 4 hardware queues; RCCL adds its own
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C2")
    ap.add_argument("--iterations", type=int, default=300)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--batch-size", type=int, default=4)
    ap.add_argument("--lambda-rigid", type=float, default=0.0, help="the rigid term's weight (configs/dnerf/lego.yaml: 1.0; rot_4d scenes)")
    ap.add_argument("--env-map-res", type=int, default=0, help="train an environment map of this resolution behind the Gaussians "
                    "(configs/dynerf/coffee_martini.yaml: 500); the ground truth is rendered over a known smooth environment")
    ap.add_argument("--test-views", type=int, default=0, help="hold out this many cameras at timestamps half-way between two training "
                    "ones and evaluate them and five training views (L1, PSNR, SSIM, MS-SSIM) at 7000, 30000 and the last iteration")
    ap.add_argument("--exhaust-test", action="store_true", help="also evaluate every 500 iterations (train.py:392-393); without "
                    "--test-views only the five training views are evaluated")
    ap.add_argument("--u8-frames", choices=("device", "host"), default=None, help="quantise the rendered ground truth to 8-bit images, as a "
                    "dataset's are, and train from a FrameStore of them kept on the device or in pinned host memory (fdgs.frames)")
    args = ap.parse_args()
    world, rank, local = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29500")
        dist.init_process_group(backend="nccl", rank=rank, world_size=world, device_id=dev)
    from fdgs import harness, synth, train_host
    from fdgs.fused import render_raw
    scene = synth.make_scene(synth.CONFIGS[args.workload], seed=0)
    pipe, bg = train_host.PipelineFlags(), scene["bg"].to(dev)
    target = train_host.GaussianParams(scene, dev)
    cams = [train_host.SyntheticCamera(scene, dev, timestamp=(v + 0.5) / args.views * scene["time_duration"]) for v in range(args.views)]
    if args.env_map_res:
        pipe.env_map_res = R = args.env_map_res
        # the known environment: a few low harmonics in longitude and latitude
        u = (torch.arange(R, dtype=torch.float32, device=dev) + 0.5) / R
        truth = torch.stack([0.5 + 0.3 * torch.sin(2 * math.pi * (u[None, :] + ph)) * torch.cos(math.pi * (u[:, None] - 0.5))
                             for ph in (0.0, 0.33, 0.66)])
        target.env_map = truth
    # held-out views: training view j sits at (j + 0.5) / views of the time span; test view v half-way between training views j and j + 1,
    # at (j + 1) / views, with the j spread evenly over 0 .. views - 2
    if args.test_views > args.views - 1:
        ap.error("--test-views must be at most --views - 1 (one held-out timestamp between two training ones)")
    tcams = [train_host.SyntheticCamera(scene, dev, timestamp=((2 * v + 1) * (args.views - 1) // (2 * args.test_views) + 1) / args.views
                                        * scene["time_duration"]) for v in range(args.test_views)]
    with torch.no_grad():
        gts = [render_raw(c, target, pipe, bg)["render"].clone() for c in cams]
        tgts = [render_raw(c, target, pipe, bg)["render"].clone() for c in tcams]
    if args.u8_frames:
        from fdgs.frames import FrameStore
        quantise = lambda ims: torch.stack([(x.clamp(0, 1) * 255 + 0.5).to(torch.uint8).permute(1, 2, 0) for x in ims])   # [N, H, W, 3]
        gts = FrameStore(quantise(gts), residency=args.u8_frames, device=dev)
        tgts = FrameStore(quantise(tgts), residency=args.u8_frames, device=dev) if tgts else tgts
    test_iterations = ()   # training_report's five training views, plus the held-out ones if there are any
    if args.test_views or args.exhaust_test:
        test_iterations = [7000, 30000, args.iterations]
        if args.exhaust_test:
            test_iterations += list(range(0, args.iterations + 1, 500))
    student = train_host.GaussianParams(scene, dev)
    g = torch.Generator(device="cpu").manual_seed(1)   # same perturbation on every rank: replicas start identical
    with torch.no_grad():
        student.params["_features"].add_(0.3 * torch.randn(student.params["_features"].shape, generator=g).to(dev))
        student.params["_opacity"].add_(0.5 * torch.randn(student.params["_opacity"].shape, generator=g).to(dev))
    del target
    opt = train_host.make_optimizer(student)
    torch.cuda.synchronize(); t0 = time.time()
    harness.train(student, opt, cams, gts, pipe, bg, iterations=args.iterations, batch_size=args.batch_size,
                  world_size=world, rank=rank, log_every=max(1, args.iterations // 10), lambda_rigid=args.lambda_rigid,
                  env_lr=2e-2 if args.env_map_res else 2.5e-3, test_cameras=tcams or None, test_gts=tgts or None,
                  test_iterations=test_iterations)   # harness.train logs one line per evaluated set
    torch.cuda.synchronize()
    if rank == 0 and args.env_map_res:
        from fdgs.envmap import composite_backward
        seen = torch.zeros_like(truth)    # the texels the cameras see
        for c in cams[:8]:
            composite_backward(torch.ones(c.image_height, c.image_width, device=dev), torch.ones(3, c.image_height, c.image_width, device=dev),
                               truth, c, g_env=seen, accumulate_env=True)
        seen = seen > 0
        print("environment map: mean error on the %d seen texels %.4f (untrained: %.4f)" % (
            int(seen.sum()), float((student.env_map.detach() - truth)[seen].abs().mean()), float(truth[seen].abs().mean())))
    if rank == 0:
        dt = time.time() - t0
        print("%d iterations x %d views x %d ranks in %.2f s: %.0f images/s" % (args.iterations, args.batch_size, world, dt,
                                                                              args.iterations * args.batch_size * world / dt))


if __name__ == "__main__":
    main()
