#!/usr/bin/env python3
"""Pinned bits of the SH kernels (preprocess_fwd.hip: the colour half of preprocess_fwd_kernel and colour_batch_kernel; sh_bwd.hip:
sh_bwd_kernel<true / false>, sh_bwd_batch_kernel, sh_flush_kernel<0>): for the edge shapes of tests/test_gpu_api.py
(_SH_EDGE_TABLE) at 1, 65 and 97 Gaussians seen by 5 views, what the forward's colours and the SH backward of crafted colour
gradients are, as raw 32-bit patterns.  tests/test_gpu_api.py::test_sh_kernels_pinned_bits makes the same calls through
``run_case`` below and compares with ``==``.  The tests that compare the two kernels of a pair with each other
(test_colour_batch_edge_shapes_bitwise, test_sh_backward_paths_bitwise) pass when both change the same way; these fixtures do not.

The fixtures are NOT an oracle's results: they are what the library computed, on an MI355X, at commit 92e3dce ("Place, retime
and merge 4D models"), the commit before the per-view SH evaluation moved into csrc/sh_eval.h.  They pin the arithmetic of these
kernels (every operation, its order, its double promotions, the quirks Q1-Q4) under one toolchain; a change that is meant to alter
a bit has to re-record them, and a compiler that schedules the same source into other IEEE operations would too.  To re-record, on
a machine with the GPU and a built library:

    python tests/golden/make_golden_sh.py      ->  tests/golden/sh/<row>_P<P>_{inputs,fwd,bwd_ref,bwd_analytic,dsh_ref,dsh_analytic}.npz

``FDGS_LIB`` selects another build of the library (fdgs/_capi.py), e.g. one of an earlier commit.

<..>_inputs.npz holds every input of the case -- the cameras' matrices, centres and timestamps, the raw parameter tensors, the
coefficients, the crafted colour gradients -- as tests/test_gpu_api.py's ``_sh_edge_setup`` and ``_crafted_colour_gradients`` built
them; they are stored, not derived at test time, so no host libm enters.  No file is larger than the largest one under
tests/golden/geometry/: dL_dsh is pinned at P <= 65 only.
"""
import ctypes as C
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                    # tests/ (util, test_gpu_api)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # the repository root (fdgs)

OUT_DIR = os.path.join(HERE, "sh")
SIZES = (1, 65, 97)      # one Gaussian, one past a wave, the batch kernel's second round of 32 rows
DSH_MAX_P = 65           # dL_dsh is pinned up to here (file size)
NV = 5                   # all five liveness patterns, both view parities of the batch kernel, a parity with more than one view
MODES = {"ref": False, "analytic": True}
TENSORS = ("xyz", "feats", "opacity", "ts", "scaling", "scaling_t", "rotation", "rotation_r")
SETTINGS_INT = ("image_height", "image_width", "sh_degree", "sh_degree_t", "gaussian_dim")
SETTINGS_FLOAT = ("tanfovx", "tanfovy", "scale_modifier", "time_duration")
SETTINGS_BOOL = ("rot_4d", "force_sh_3d", "prefiltered", "debug")
FORWARD_KEYS = tuple("%s_%s" % (path, k) for path in ("single", "batch") for k in ("rgb", "clamped_bits", "radii"))
BACKWARD_KEYS = ("stage_single", "stage_batch", "words_single", "words_batch")
DSH_KEYS = ("dsh_direct", "dsh_flush")


def table():
    """(id, (D, D_t, M, sh3d, misaligned)) of every row of the edge table"""
    import test_gpu_api as T
    return list(zip(T._SH_EDGE_IDS, T._SH_EDGE_TABLE))


def make_inputs(P, row, device):
    """The case's inputs as numpy arrays, from the edge-shape setup of tests/test_gpu_api.py."""
    import test_gpu_api as T
    D, D_t, M, sh3d, misaligned = row
    scene, rss, tens = T._sh_edge_setup(P, D, D_t, M, sh3d, misaligned, device, NV)
    d = {"crafted": T._crafted_colour_gradients(P, NV, 7 + P + M).numpy(), "prefilter_var": np.float64(tens[8]),
         "bg": rss[0].bg.cpu().numpy(), "timestamp": np.array([rs.timestamp for rs in rss], dtype=np.float64)}
    for k in ("viewmatrix", "projmatrix", "campos"):
        d[k] = np.stack([getattr(rs, k).cpu().numpy() for rs in rss])
    for k in SETTINGS_INT + SETTINGS_BOOL:
        d[k] = np.int64(getattr(rss[0], k))
    for k in SETTINGS_FLOAT:
        d[k] = np.float64(getattr(rss[0], k))
    for k, t in zip(TENSORS, tens):
        d[k] = t.detach().cpu().numpy()
    assert all(v.dtype in (np.float32, np.float64, np.int64) for v in d.values())
    return d


def settings_of(inp, misaligned, device):
    """The views' raster settings and the parameter tensors (the coefficients optionally one float off their alignment)."""
    from fdgs.gaussian_renderer.diff_gaussian_rasterization import GaussianRasterizationSettings
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)   # noqa: E731
    common = {k: int(inp[k]) for k in SETTINGS_INT}
    common.update({k: float(inp[k]) for k in SETTINGS_FLOAT})
    common.update({k: bool(inp[k]) for k in SETTINGS_BOOL})
    bg = t(inp["bg"])
    rss = [GaussianRasterizationSettings(bg=bg, viewmatrix=t(inp["viewmatrix"][b]), projmatrix=t(inp["projmatrix"][b]),
                                         campos=t(inp["campos"][b]), timestamp=float(inp["timestamp"][b]), **common) for b in range(NV)]
    tens = [t(inp[k]) for k in TENSORS]
    n = inp["feats"].size
    store = torch.zeros(n + 4, device=device)
    off = 1 if misaligned else 0
    sh = store[off:off + n].view(inp["feats"].shape)
    sh.copy_(tens[1])
    assert sh.is_contiguous() and (sh.data_ptr() % 16 != 0) == bool(misaligned)
    tens[1] = sh
    return rss, tuple(tens) + (float(inp["prefilter_var"]),)


def run_case(inp, row, device):
    """The forward's colours view by view and batched, then the SH backward's paths on the crafted colour gradients (num_rendered
    = 0: no blend backward, no atomics).  {"fwd": ..., "bwd_<mode>": ..., "dsh_<mode>": ...}: numpy arrays by name."""
    from fdgs import _capi
    from fdgs.fused import raw_backward, raw_forward, raw_preprocess_batch
    from fdgs.gaussian_renderer.diff_gaussian_rasterization import _C
    from util import collect_forward
    D, D_t, M, sh3d, misaligned = row
    rss, tens = settings_of(inp, misaligned, device)
    (xyz, feats, opacity, ts, scaling, scaling_t, rotation, rotation_r, pv) = tens
    P, W, H = int(xyz.shape[0]), rss[0].image_width, rss[0].image_height
    out = {}

    # ---- forward: preprocess_fwd_kernel<0> per view, then geometry per view + colour_batch_kernel ----
    fwd = [raw_forward(rs, *tens) for rs in rss]
    single = [collect_forward(f, P, W, H) for f in fwd]
    handles = raw_preprocess_batch(rss, *tens)
    batch = [collect_forward(raw_forward(rss[b], *tens, preprocessed=handles[b]), P, W, H) for b in range(NV)]
    out["fwd"] = {"%s_%s" % (name, k): np.stack([i[k] for i in info]) for name, info in (("single", single), ("batch", batch))
                  for k in ("rgb", "clamped_bits", "radii")}

    # ---- backward ----
    gacc = torch.zeros((NV, P, 16), device=device)
    stage = torch.zeros((2, NV, P, 8), device=device)
    dsh = torch.zeros((P, M, 3), device=device)
    ups = torch.zeros(3, H, W, device=device)
    pend = []
    for b in range(NV):
        (R, color, flow, depth, T, radii, geom, binb, img, _covs, om) = fwd[b]
        pend.append(raw_backward(rss[b], xyz, om, radii, feats, opacity, ts, scaling, scaling_t, rotation, rotation_r, pv, geom, R, binb, img,
                                 ups, None, None, None, None, False, grad_accum=gacc[b], sh_stage=stage[0, b], begin_only=True))
    torch.cuda.synchronize()
    for p in pend:
        p["bin"].num_rendered = 0        # fdgs_rasterize_backward: no blend backward
        assert p["bout"].grad_accum_clean == 1   # ... and no memset of the accumulator

    def sh_backward(p):
        p["bout"].stage_mask = 1
        with torch.cuda.device(device):
            rc = _capi.lib.fdgs_rasterize_backward(C.byref(p["scene"]), C.byref(p["bin"]), C.byref(p["bout"]), _capi.current_stream_handle(device))
        _capi._check(rc, "fdgs_rasterize_backward")

    snap = torch.zeros((NV, P, 16), device=device)
    snap[:, :, 0:3] = torch.from_numpy(inp["crafted"]).to(device)
    for mode, analytic in MODES.items():
        for p in pend:
            p["scene"].analytic_sh_grad = int(analytic)
        words = []
        # sh_bwd_kernel<true> view by view, then sh_bwd_batch_kernel
        for path in (0, 1):
            gacc.copy_(snap)
            stage[path].fill_(float("nan"))
            for b, p in enumerate(pend):
                p["bout"].sh_stage = stage[path, b].data_ptr()
                if path == 0:
                    sh_backward(p)
            if path == 1:
                _C.sh_backward_batch(pend)
            torch.cuda.synchronize()
            words.append(gacc[:, :, 12:16].cpu().numpy())
        st = stage.cpu().numpy()
        out["bwd_" + mode] = {"stage_single": st[0], "stage_batch": st[1], "words_single": words[0], "words_batch": words[1]}
        if P > DSH_MAX_P:
            continue
        # sh_bwd_kernel<false>: the first view overwrites, the others accumulate; and the flush of the per-view stages
        gacc.copy_(snap)
        dsh.fill_(float("nan"))
        for b, p in enumerate(pend):
            p["bout"].sh_stage = None
            p["bout"].dL_dsh = dsh.data_ptr()
            p["bout"].accumulate = int(b > 0)
            sh_backward(p)
        flushed = torch.full((P, M, 3), float("nan"), device=device)
        _capi.sh_flush(stage[0].contiguous(), flushed, D, D_t, rss[0].gaussian_dim, rss[0].force_sh_3d, analytic)
        torch.cuda.synchronize()
        out["dsh_" + mode] = {"dsh_direct": dsh.cpu().numpy(), "dsh_flush": flushed.cpu().numpy()}
    gacc.zero_()
    return out


def files_of(P):
    """the output files of a case: name -> keys"""
    f = {"fwd": FORWARD_KEYS}
    for mode in MODES:
        f["bwd_" + mode] = BACKWARD_KEYS
        if P <= DSH_MAX_P:
            f["dsh_" + mode] = DSH_KEYS
    return f


def fixture_path(row_id, P, name):
    return os.path.join(OUT_DIR, "%s_P%d_%s.npz" % (row_id, P, name))


def check_contents(inp, got):
    """What a case must contain: the live sets the kernels' paths need (stage records: dRGB != 0 where live)."""
    P = inp["xyz"].shape[0]
    live = (got["bwd_ref"]["stage_single"][:, :, :3] != 0).any(2)     # [NV, P]
    if P >= 63:
        assert (got["fwd"]["single_radii"] > 0).any() and (got["fwd"]["single_rgb"] != 0).any()
        assert (live.any(0) & ~live.all(0)).any()    # some Gaussian is live in one view and dead in another
    if P >= 97:   # the batch kernel's second round of 32 rows
        union = live.any(0)
        assert max(int(union[s:s + 64].sum()) for s in range(0, P, 64)) >= 33


def main():
    os.makedirs(OUT_DIR, exist_ok=True)
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: the fixtures are the library's own results")
    dev = torch.device("cuda:0")
    limit = max(os.path.getsize(os.path.join(HERE, "geometry", f)) for f in os.listdir(os.path.join(HERE, "geometry")))
    total = 0
    for row_id, row in table():
        for P in SIZES:
            inp = make_inputs(P, row, dev)
            got, again = run_case(inp, row, dev), run_case(inp, row, dev)
            check_contents(inp, got)
            files = dict(got, inputs=inp)
            assert set(got) == set(files_of(P))
            for name, d in files.items():
                if name != "inputs":
                    assert set(d) == set(files_of(P)[name])
                    for k in d:
                        assert d[k].tobytes() == again[name][k].tobytes(), ("not reproducible", row_id, P, name, k)
                path = fixture_path(row_id, P, name)
                np.savez_compressed(path, **d)
                size = os.path.getsize(path)
                assert size <= limit, (path, size, limit)
                total += size
    print("%d bytes under %s, the largest file allowed %d" % (total, OUT_DIR, limit))


if __name__ == "__main__":
    sys.exit(main())
