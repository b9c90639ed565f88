#!/usr/bin/env python3
"""Generates tests/golden/trained_<fixture>.npz: the state a TRAINING RUN leaves behind, with the reference's outputs on it.

Every other parity scene comes from fdgs.synth.  These hold raw quaternions that are not unit, raw scales Adam has moved, split children
at scale / 1.6 on top of their siblings, clones, opacities pinned at 0.01 right after a reset, SH colours clamped at 0, SH degrees
part-way up the ramp with the allocated coefficients beyond them still zero, and the densification statistics of real steps.

    python tests/golden/make_golden_trained.py train  <dir> [--cases ...]     once, on the GPU: writes <dir>/snap_<fixture>.npz
    python tests/golden/make_golden_trained.py golden <dir> [--cases ...]     on the CPU, needs the reference build: writes the fixtures

Stage ``train``
    fdgs.harness.train on the teacher / student recipe of tests/test_gpu_train.py::test_training_with_densification, shrunk (RECIPE and
    CASE_RECIPE below): 400 initial Gaussians, 96x72, 12 cameras on the fdgs.synth.POSES rigs with timestamps spread over the duration,
    199 iterations from SH degrees (0, 0) with a short sh_increase_interval, densification every 25 iterations from 20 on, an opacity
    reset every 60, rows in the reference's order (spatial_order=False).  The student's coefficients beyond the DC term start at zero, as
    in a run from a point cloud.  The volume reaches beyond what the rigs see, so that some Gaussians are seen by no view of an interval.
    The densification threshold is set for a 96x72 image: its view-space gradients are an order of magnitude above a full-size image's,
    and at the default threshold the model doubles at every densification.

    Snapshots are taken through save_iterations / on_save.  Each holds the raw parameter tensors, the active and allocated degrees, the
    DensificationStats arrays, the counts of the densify reports so far (cloned, split, pruned), the cameras and the recipe.

        rot4d        (M = 48)          2 iterations after an opacity reset ("rot4d_reset") and at the end ("rot4d_end")
        dim4_norot   (force_sh_3d)     the end ("dim4_norot_end")
        dim3                           the end ("dim3_end")

    The end is an iteration with iteration % densification_interval == interval - 1: the statistics hold a whole interval.

    The learning rates of ``_rotation`` / ``_rotation_r`` are 10 x the default (optimizer.set_lr before training).  The gradient of a
    normalised quaternion is orthogonal to q, so |q| drifts only at second order: at the default 1e-3, 200 steps move it by about 4e-4.
    At 10 x it reaches what a 20 000-iteration run has and more (recorded: |q| from 0.6 to 2.4, median 1.1 - 1.2).

    A new ``train`` run is a NEW RECORDING, not a reproduction: the float atomics of the backward land in another order every run, Adam
    amplifies that, and the densification decisions follow.  The committed fixtures are the recording.

Stage ``golden``
    Activates each snapshot's raw state in torch (exp, sigmoid, normalize) into the scene-dict format and picks two of its training
    cameras: the first two, in recorded order, that put no Gaussian on the temporal-cull cliff and fewer than 1e-3 of the pixels on a
    threshold cliff (the port oracle's border_g / border).  The state is never edited.  The reference's own kernels
    (pyoracle.Oracle(kind="reference")) then run forward and backward with synth.make_upstream_grads(seed=1, scale=1e-2).  Written:

        raw_<param>               the raw parameter tensors
        stats_<name>              the DensificationStats arrays
        meta_<name>               degrees, counts, recipe, visible Gaussians and util.ill_conditioned_count per view
        in_<key>                  scales, scales_t, rotations, rotations_r, opacities (activated) and flow_2d: the same for both views, stored
                                  once; means3D / ts / shs ARE raw_xyz / raw_t / raw_features and are not stored twice
        meta_up_seed / _scale     the upstream gradients are synth.make_upstream_grads(W, H, seed, scale) for both views: not stored
        v<k>_in_<key>             the camera tensors and background of view k
        v<k>_sc_* / fw_* / bw_*   per view, as make_golden.py writes them

    tests/golden_util.py::load_trained puts the shared parts back into every view.
"""
import argparse
import json
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from fdgs import synth  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SC = synth.SceneConfig
NAMES = ("_xyz", "_opacity", "_scaling", "_rotation", "_t", "_scaling_t", "_rotation_r", "_features")
STATS = ("xyz_gradient_accum", "t_gradient_accum", "denom", "max_radii2D")

RECIPE = dict(P0=400, W=96, H=72, views=12, iterations=199, batch_size=4, densify_from_iter=20, densification_interval=25,
              opacity_reset_interval=60, densify_until_num_points=1500, cameras_extent=2.0, percent_dense=0.035, rotation_lr_scale=10.0,
              s0=0.08, volume_scale=1.3, densify_grad_threshold=5.5e-3, seed=0)
# case -> (scene config (name, P, W, H, D, D_t, s0, duration, rot_4d, gaussian_dim, force_sh_3d) with the ALLOCATED degrees,
#          scene seed, sh_increase_interval, {fixture name: snapshot iteration})
CASES = {
    "rot4d": (lambda r: SC("t", r["P0"], r["W"], r["H"], 3, 2, r["s0"], 4.0, True, 4, False), 31, 45, {"rot4d_reset": 122, "rot4d_end": 199}),
    "dim4_norot": (lambda r: SC("t", r["P0"], r["W"], r["H"], 3, 0, r["s0"], 1.0, False, 4, True), 32, 80, {"dim4_norot_end": 199}),
    "dim3": (lambda r: SC("t", r["P0"], r["W"], r["H"], 3, 0, r["s0"], 1.0, False, 3, False), 33, 80, {"dim3_end": 199}),
}
# per-case changes to RECIPE: M = 48 makes a rot4d row four times as large, so that model grows more slowly (a fixture stays below 1 MiB)
# a 3D model has no temporal cull: its volume reaches further beyond the rigs' frusta, so that it too has Gaussians no view saw
CASE_RECIPE = {"rot4d": dict(densify_grad_threshold=6.5e-3), "dim3": dict(volume_scale=1.8)}
POSE_NAMES = ("rig0", "rig1", "rig2", "rig3")
CAM_KEYS = ("world_view_transform", "full_proj_transform", "camera_center")


# ------------------------------------------------------------------------------------------------------------------------------
# stage 1: train (GPU)
# ------------------------------------------------------------------------------------------------------------------------------

def train_case(case, recipe, out_dir):
    from fdgs import harness, train_host
    from fdgs.fused import render_raw
    dev = torch.device("cuda:0")
    make_cfg, seed, sh_interval, snaps = CASES[case]
    cfg = make_cfg(recipe)
    scene = synth.make_scene(cfg, seed=seed)
    # a teacher whose colours span [0, 1]: the student's overshoot below 0 is what the clamp sees
    scene["shs"] = scene["shs"].clone()
    scene["shs"][:, 0, :] *= 1.8
    # a volume that reaches beyond what the rigs see: Gaussians no view of an interval saw (denom == 0)
    scene["means3D"] = (scene["means3D"] * recipe["volume_scale"]).contiguous()
    W, H, V, dur = cfg.W, cfg.H, recipe["views"], scene["time_duration"]
    pipe, bg = train_host.PipelineFlags(), torch.zeros(3, device=dev)
    target = train_host.GaussianParams(scene, dev)
    poses = [POSE_NAMES[v % len(POSE_NAMES)] for v in range(V)]
    stamps = [(v + 0.5) / V * dur for v in range(V)]
    cam_tensors = [synth.camera_for(p, W, H) for p in poses]
    cams = [train_host.SyntheticCamera(dict(scene, **ct), dev, timestamp=t) for ct, t in zip(cam_tensors, stamps)]
    with torch.no_grad():
        gts = [render_raw(c, target, pipe, bg)["render"].clone() for c in cams]
    student = train_host.GaussianParams(scene, dev)
    g = torch.Generator(device="cpu").manual_seed(recipe["seed"])
    with torch.no_grad():
        f = student.params["_features"]
        f[:, 1:, :] = 0.0                                                        # a run from a point cloud: only the DC term is set
        f[:, 0, :].add_(0.5 * torch.randn(f[:, 0, :].shape, generator=g).to(dev))
        student.params["_xyz"].add_(0.01 * torch.randn(student.params["_xyz"].shape, generator=g).to(dev))
    opt = train_host.make_optimizer(student)
    for n in ("_rotation", "_rotation_r"):
        opt.set_lr(n, 1e-3 * recipe["rotation_lr_scale"])
    lines, written = [], []
    pat = re.compile(r"densify: (\d+) -> (\d+) Gaussians \((\d+) cloned, (\d+) split\)")
    by_iter = {it: name for name, it in snaps.items()}

    def counts():
        c = dict(cloned=0, split=0, pruned=0, densifications=0)
        for l in lines:
            m = pat.search(l)
            if m:
                p_old, p_new, cl, sp = (int(x) for x in m.groups())
                c["cloned"] += cl; c["split"] += sp; c["densifications"] += 1
                c["pruned"] += p_old + cl + sp - p_new       # N = 2: a split parent goes, two children come
        return c

    def on_save(iteration, model, optimizer, stats):
        torch.cuda.synchronize()
        name = by_iter[iteration]
        d = {"raw" + n: model.params[n].detach().cpu().numpy().copy() for n in NAMES}
        for k in STATS:
            d["stats_" + k] = getattr(stats, k).cpu().numpy().copy()
        meta = dict(case=case, name=name, iteration=iteration, P0=cfg.P, P=model.P, active_sh_degree=model.active_sh_degree,
                    active_sh_degree_t=model.active_sh_degree_t, max_sh_degree=model.max_sh_degree, max_sh_degree_t=model.max_sh_degree_t,
                    rot_4d=cfg.rot_4d, gaussian_dim=cfg.gaussian_dim, force_sh_3d=cfg.force_sh_3d, time_duration=dur,
                    sh_increase_interval=sh_interval, scene_seed=seed, poses=poses, timestamps=stamps, recipe=recipe, **counts())
        d["meta_json"] = np.array(json.dumps(meta))
        for k in CAM_KEYS:
            d["cam_" + k] = np.stack([ct[k].numpy() for ct in cam_tensors])
        d["cam_tanfov"] = np.array([[ct["tanfovx"], ct["tanfovy"]] for ct in cam_tensors], np.float64)
        d["cam_fov"] = np.array([[ct["FoVx"], ct["FoVy"]] for ct in cam_tensors], np.float64)
        path = os.path.join(out_dir, "snap_%s.npz" % name)
        np.savez_compressed(path, **d)
        written.append(path)
        q = np.linalg.norm(d["raw_rotation"], axis=1)
        op = 1.0 / (1.0 + np.exp(-d["raw_opacity"]))
        print("%s it %d: P %d -> %d, degrees %d/%d of %d/%d, %s; | |q| - 1 | > 1e-3 on %.0f %%, max opacity %.4f, denom == 0 on %d, "
              "max_radii2D > 20 on %d, max scale %.3f" % (
                  name, iteration, cfg.P, model.P, model.active_sh_degree, model.active_sh_degree_t, model.max_sh_degree,
                  model.max_sh_degree_t, counts(), 100.0 * float((np.abs(q - 1) > 1e-3).mean()), float(op.max()),
                  int((d["stats_denom"] == 0).sum()), int((d["stats_max_radii2D"] > 20).sum()), float(np.exp(d["raw_scaling"]).max())), flush=True)

    r = recipe
    harness.train(student, opt, cams, gts, pipe, bg, iterations=r["iterations"], batch_size=r["batch_size"], seed=r["seed"], log_every=50,
                  log=lines.append, sh_degree_start=(0, 0), sh_increase_interval=sh_interval, densify_from_iter=r["densify_from_iter"],
                  densification_interval=r["densification_interval"], opacity_reset_interval=r["opacity_reset_interval"],
                  densify_grad_threshold=r["densify_grad_threshold"], cameras_extent=r["cameras_extent"], percent_dense=r["percent_dense"],
                  densify_until_num_points=r["densify_until_num_points"], spatial_order=False, save_iterations=sorted(snaps.values()),
                  on_save=on_save)
    torch.cuda.synchronize()
    for l in lines:
        print("   ", l)
    assert len(written) == len(snaps), written


def stage_train(args):
    os.makedirs(args.dir, exist_ok=True)
    for case in (args.cases or list(CASES)):
        train_case(case, dict(RECIPE, **CASE_RECIPE.get(case, {})), args.dir)


# ------------------------------------------------------------------------------------------------------------------------------
# stage 2: golden (CPU, the reference's own kernels)
# ------------------------------------------------------------------------------------------------------------------------------

FIXTURES = ("rot4d_reset", "rot4d_end", "dim4_norot_end", "dim3_end")
PER_GAUSSIAN = ("means3D", "ts", "scales", "scales_t", "rotations", "rotations_r", "opacities", "shs", "flow_2d")
PER_VIEW = ("bg", "world_view_transform", "full_proj_transform", "camera_center")
SCALAR_KEYS = ("W", "H", "sh_degree", "sh_degree_t", "timestamp", "time_duration", "rot_4d", "gaussian_dim",
               "force_sh_3d", "scale_modifier", "prefilter_var", "tanfovx", "tanfovy")
RAW_ALIAS = {"means3D": "_xyz", "ts": "_t", "shs": "_features"}   # inputs that ARE raw parameters: not stored twice
MAX_BYTES = 1 << 20   # a committed file stays below 1 MiB


def activate(snap):
    """The reference's getters (scene/gaussian_model.py:179-219) on the raw tensors, in torch."""
    t = {n: torch.from_numpy(snap["raw" + n].copy()) for n in NAMES}
    P = t["_xyz"].shape[0]
    return {"means3D": t["_xyz"], "ts": t["_t"], "scales": torch.exp(t["_scaling"]), "scales_t": torch.exp(t["_scaling_t"]),
            "rotations": torch.nn.functional.normalize(t["_rotation"]), "rotations_r": torch.nn.functional.normalize(t["_rotation_r"]),
            "opacities": torch.sigmoid(t["_opacity"]), "shs": t["_features"], "flow_2d": torch.zeros(P, 2)}


def view_scene(snap, meta, act, v):
    r = meta["recipe"]
    sc = dict(act)
    for k in CAM_KEYS:
        sc[k] = torch.from_numpy(snap["cam_" + k][v].copy())
    sc.update(bg=torch.zeros(3), W=r["W"], H=r["H"], M=int(act["shs"].shape[1]), sh_degree=meta["active_sh_degree"],
              sh_degree_t=meta["active_sh_degree_t"], timestamp=float(meta["timestamps"][v]), time_duration=float(meta["time_duration"]),
              rot_4d=bool(meta["rot_4d"]), gaussian_dim=int(meta["gaussian_dim"]), force_sh_3d=bool(meta["force_sh_3d"]),
              scale_modifier=1.0, prefilter_var=-1.0, tanfovx=float(snap["cam_tanfov"][v, 0]), tanfovy=float(snap["cam_tanfov"][v, 1]))
    return sc


def stage_golden(args):
    from oracle import pyoracle
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from util import ill_conditioned_count
    if pyoracle.build_ref() is None:
        raise SystemExit("needs the reference tree to build oracle/_ref/liboracle_ref.so")
    for name in (args.cases or FIXTURES):
        snap = np.load(os.path.join(args.dir, "snap_%s.npz" % name))
        meta = json.loads(str(snap["meta_json"]))
        act = activate(snap)
        data = {k: snap[k] for k in snap.files if k.startswith(("raw_", "stats_"))}
        for k in PER_GAUSSIAN:
            if k not in RAW_ALIAS:
                data["in_" + k] = act[k].numpy()
        up = synth.make_upstream_grads(meta["recipe"]["W"], meta["recipe"]["H"], seed=1, scale=1e-2)
        data["meta_up_seed"], data["meta_up_scale"] = np.asarray(1), np.asarray(1e-2)   # (regenerated by the loader: 180 KB of noise)
        picked, cond, nvis = [], [], []
        for v in range(len(meta["timestamps"])):
            if len(picked) == 2:
                break
            sc = view_scene(snap, meta, act, v)
            o = pyoracle.Oracle(sc, kind="port")
            ref = o.forward()
            n_bg, frac = int(ref["border_g"].sum()), float(ref["border"].mean())
            if n_bg or frac >= 1e-3:
                print("%s: camera %d left out (%d Gaussians on the temporal-cull cliff, cliff pixel fraction %.2e)" % (name, v, n_bg, frac))
                o.close()
                continue
            vis = ref["radii"] > 0
            cond.append(ill_conditioned_count(o, up, vis))
            nvis.append(int(vis.sum()))
            o.close()
            o = pyoracle.Oracle(sc, kind="reference")
            out = dict(o.forward())
            gr = o.backward(up["grad_color"], up["grad_depth"], up["grad_alpha"], up["grad_flow"])
            pre = "v%d_" % len(picked)
            for k in PER_VIEW:
                data[pre + "in_" + k] = sc[k].numpy()
            for k in SCALAR_KEYS:
                data[pre + "sc_" + k] = np.asarray(sc[k])
            for k, a in out.items():
                if k not in ("border", "border_g"):
                    data[pre + "fw_" + k] = a.copy()
            data[pre + "fw_R"] = np.asarray(o.R)
            for k, a in gr.items():
                data[pre + "bw_" + k] = a.copy()
            clamped = int((out["clamped"][vis].any(1)).sum())
            print("%s view %d = camera %d (%s, t = %.3f): R %d, %d visible, %d with a clamped channel, cliff pixels %.2e, "
                  "port oracle vs itself beyond 1e-4 on %d" % (name, len(picked), v, meta["poses"][v], meta["timestamps"][v], o.R, nvis[-1],
                                                           clamped, frac, cond[-1]))
            o.close()
            picked.append(v)
        assert len(picked) == 2, "%s: fewer than two cliff-free cameras" % name
        for k in ("iteration", "P0", "P", "active_sh_degree", "active_sh_degree_t", "max_sh_degree", "max_sh_degree_t", "rot_4d", "gaussian_dim",
                  "force_sh_3d", "time_duration", "cloned", "split", "pruned", "densifications", "sh_increase_interval", "scene_seed"):
            data["meta_" + k] = np.asarray(meta[k])
        data["meta_views"] = np.asarray(picked)
        data["meta_view_poses"] = np.asarray([meta["poses"][v] for v in picked])
        data["meta_visible"] = np.asarray(nvis)
        data["meta_ill_conditioned"] = np.asarray(cond)
        for k, x in meta["recipe"].items():
            data["meta_recipe_" + k] = np.asarray(x)
        path = os.path.join(HERE, "trained_%s.npz" % name)
        np.savez_compressed(path, **data)
        size = os.path.getsize(path)
        print("%-16s P %d  %7.1f KiB" % (name, meta["P"], size / 1024))
        assert size <= MAX_BYTES, "%s: %d bytes; lower the point cap" % (path, size)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("stage", choices=("train", "golden"))
    ap.add_argument("dir", help="where the snapshots are written (train) / read (golden)")
    ap.add_argument("--cases", nargs="*", default=None, help="train: rot4d dim4_norot dim3; golden: fixture names (default: all)")
    args = ap.parse_args()
    if args.stage == "train":
        stage_train(args)
    else:
        stage_golden(args)


if __name__ == "__main__":
    main()
