"""CPU: the C-ABI library loads and exports everything include/fdgs.h declares; host-side argument handling
(no GPU compute is launched here)."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    with open(os.path.join(ROOT, "include", "fdgs.h")) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(fdgs_[a-z_0-9]+)\s*\(", text)) - {"fdgs_alloc_fn"})


def test_library_exports_every_declared_symbol():
    from fdgs import _capi
    names = _declared_symbols()
    assert len(names) >= 12
    for n in names:
        assert hasattr(_capi.lib, n), "libfdgs.so does not export %s" % n
        assert n in _capi.EXPORTED or n in ("fdgs_alloc_fn",), "binding list misses %s" % n
    assert _capi.lib.fdgs_version() == _capi.FDGS_VERSION == 502
    with open(os.path.join(ROOT, "include", "fdgs.h")) as f:
        assert re.search(r"#define FDGS_VERSION (\d+)", f.read()).group(1) == str(_capi.FDGS_VERSION)


def test_scratch_sizes_are_monotone_and_aligned():
    from fdgs import _capi
    g1, g2 = _capi.lib.fdgs_geometry_bytes(1000), _capi.lib.fdgs_geometry_bytes(300000)
    assert 0 < g1 < g2 and g1 % 256 == 0 and g2 % 256 == 0
    assert g2 / 300000 < 100  # 89 B / Gaussian of scratch
    i = _capi.lib.fdgs_image_bytes(1352, 1014)
    assert i % 256 == 0 and i >= 1352 * 1014 * 8
    b = _capi.lib.fdgs_binning_bytes(3_000_000, 1352, 1014)
    assert b % 256 == 0 and 12 * 3_000_000 <= b < 13 * 3_000_000  # point_list 4 B + (depth bits, id) pairs 8 B per instance + cull planes
    # the cull planes (one bit per list entry and 8x8 block + one word per tile and plane): 4 x (R / 64 + T + 2) 64-bit words
    T = ((1352 + 15) // 16) * ((1014 + 15) // 16)
    assert b >= 12 * 3_000_000 + 32 * (3_000_000 // 64 + T + 2)
    small = _capi.lib.fdgs_binning_bytes(10, 1352, 1014)   # few instances on many tiles: the per-tile words dominate
    assert small >= 32 * (T + 2) and small < 64 * (T + 2) + 4096


def test_argument_errors_are_reported_without_touching_the_gpu():
    from fdgs import _capi
    scene = _capi.FdgsScene()
    scene.P, scene.W, scene.H = 10, 0, 16
    out = _capi.FdgsForwardOut()
    R = C.c_int32(0)
    cb = _capi.ALLOC_FN(lambda u, w, n: None)
    rc = _capi.lib.fdgs_rasterize_forward(C.byref(scene), C.byref(out), cb, None, None, C.byref(R))
    assert rc == 1 and "bad sizes" in _capi.last_error()
    scene.W = 16  # sizes fine, required pointers missing
    rc = _capi.lib.fdgs_rasterize_forward(C.byref(scene), C.byref(out), cb, None, None, C.byref(R))
    assert rc == 1 and "must not be NULL" in _capi.last_error()
    assert _capi.lib.fdgs_mark_visible(-1, None, None, None, None, None) == 1
    # the tile binning test hook turns sizes it cannot take away before it looks at a pointer
    for P, gx, T, what in ((1, 4, 0, "T = 0"), (1, 4, 1 << 24, "T = 16777216"), (1, 0, 8, "grid_x = 0"), (0, 4, 8, "P = 0")):
        assert _capi.lib.fdgs_debug_tile_bin(P, None, None, gx, T, 0, 16, 0, *([None] * 9)) == 1
        assert "fdgs_debug_tile_bin" in _capi.last_error() and what in _capi.last_error()
    assert _capi.lib.fdgs_debug_tile_bin(1, None, None, 4, 8, 0, 16, 0, *([None] * 9)) == 1 and "NULL" in _capi.last_error()
    assert _capi.lib.fdgs_debug_tile_bin_scratch_bytes(1200, 5000) % 256 == 0
    assert _capi.lib.fdgs_profile_read(99, None, None) == 1


def test_structs_carry_their_size_and_a_short_struct_is_rejected():
    """Every ABI struct starts with struct_size; a caller built against another header (here: a size that is off by one field) gets
    FDGS_ERR_INVALID_ARG instead of the library reading past the end of its struct."""
    from fdgs import _capi
    for cls in (_capi.FdgsScene, _capi.FdgsForwardOut, _capi.FdgsBackwardIn, _capi.FdgsBackwardOut, _capi.FdgsDebugView):
        assert cls().struct_size == C.sizeof(cls) and cls._fields_[0][0] == "struct_size"
    scene, out = _capi.FdgsScene(), _capi.FdgsForwardOut()
    scene.P, scene.W, scene.H = 10, 16, 16
    R = C.c_int32(0)
    cb = _capi.ALLOC_FN(lambda u, w, n: None)
    scene.struct_size -= 4
    assert _capi.lib.fdgs_rasterize_forward(C.byref(scene), C.byref(out), cb, None, None, C.byref(R)) == 1
    assert "struct_size" in _capi.last_error() and "fdgs_scene" in _capi.last_error()
    scene.struct_size += 4
    out.struct_size = 0
    assert _capi.lib.fdgs_rasterize_forward(C.byref(scene), C.byref(out), cb, None, None, C.byref(R)) == 1
    assert "fdgs_forward_out" in _capi.last_error()
    bi, bo = _capi.FdgsBackwardIn(), _capi.FdgsBackwardOut()
    bo.struct_size += 8
    assert _capi.lib.fdgs_rasterize_backward(C.byref(scene), C.byref(bi), C.byref(bo), None) == 1
    assert "fdgs_backward_out" in _capi.last_error()


def _settings(**kw):
    from fdgs.gaussian_renderer.diff_gaussian_rasterization import GaussianRasterizationSettings
    base = dict(image_height=32, image_width=32, tanfovx=0.5, tanfovy=0.5, bg=torch.zeros(3), scale_modifier=1.0,
                viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=0, sh_degree_t=0, campos=torch.zeros(3),
                timestamp=0.0, time_duration=1.0, rot_4d=True, gaussian_dim=4, force_sh_3d=False, prefiltered=False,
                debug=False)
    base.update(kw)
    return GaussianRasterizationSettings(**base)


def test_rasterizer_keeps_the_reference_exceptions_and_signature():
    """gaussian_renderer/diff_gaussian_rasterization.py:263-280: same keyword names / defaults, same Exceptions."""
    import inspect
    from fdgs.gaussian_renderer.diff_gaussian_rasterization import GaussianRasterizer, GaussianRasterizationSettings
    assert list(GaussianRasterizationSettings._fields) == [
        "image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix", "projmatrix",
        "sh_degree", "sh_degree_t", "campos", "timestamp", "time_duration", "rot_4d", "gaussian_dim", "force_sh_3d",
        "prefiltered", "debug"]
    sig = inspect.signature(GaussianRasterizer.forward)
    assert list(sig.parameters)[1:] == ["means3D", "means2D", "opacities", "shs", "colors_precomp", "flow_2d", "ts",
                                        "scales", "scales_t", "rotations", "rotations_r", "cov3D_precomp",
                                        "prefilter_var"]
    assert sig.parameters["prefilter_var"].default == -1.0
    r = GaussianRasterizer(_settings())
    P = 4
    m, o = torch.zeros(P, 3), torch.ones(P, 1)
    with pytest.raises(Exception, match="excatly one of either SHs or precomputed colors"):
        r(m, m, o)
    with pytest.raises(Exception, match="excatly one of either SHs or precomputed colors"):
        r(m, m, o, shs=torch.zeros(P, 1, 3), colors_precomp=torch.zeros(P, 3))
    with pytest.raises(Exception, match="scale/rotation pair or precomputed 3D covariance"):
        r(m, m, o, colors_precomp=torch.zeros(P, 3))
    with pytest.raises(Exception, match="scale/rotation pair or precomputed 3D covariance"):
        r(m, m, o, colors_precomp=torch.zeros(P, 3), scales=torch.ones(P, 3), rotations=torch.ones(P, 4),
          cov3D_precomp=torch.zeros(P, 6))
    with pytest.raises(Exception, match="rotations_r and scales_t and ts"):
        r(m, m, o, colors_precomp=torch.zeros(P, 3), scales=torch.ones(P, 3), rotations=torch.ones(P, 4))


def test_no_cpu_fallback():
    """The product path must fail loudly, not silently fall back, when handed CPU tensors."""
    from fdgs.gaussian_renderer.diff_gaussian_rasterization import GaussianRasterizer
    r = GaussianRasterizer(_settings(rot_4d=False, gaussian_dim=3))
    P = 4
    with pytest.raises(RuntimeError, match="no CPU path"):
        r(torch.zeros(P, 3), torch.zeros(P, 3), torch.ones(P, 1), colors_precomp=torch.zeros(P, 3),
          scales=torch.ones(P, 3), rotations=torch.ones(P, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        r.markVisible(torch.zeros(P, 3))


def test_product_never_imports_the_oracle():
    """The oracle is test infrastructure: nothing under the package may import, include or load it."""
    pkg = os.path.join(ROOT, "4d-gaussian-splatting_amd")
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            if not fn.endswith((".py", ".hip", ".h", ".sh")):
                continue
            with open(os.path.join(dirpath, fn)) as f:
                for ln in f:
                    low = ln.lower()
                    if "oracle" in low or "ref_hip" in low or "refhip" in low:
                        assert not any(tok in low for tok in ("import", "#include", "cdll", "dlopen", "liboracle", "ref_hip", "refhip")), \
                            "%s references the oracle: %s" % (fn, ln.strip())


def test_only_the_baseline_leg_of_the_bench_touches_the_oracle():
    """bench.py may use oracle/ in its baseline leg only (cpu_baseline and its GPU half, reference_kernels_on_this_gpu): every import of it
    sits inside those two functions."""
    import ast
    with open(os.path.join(ROOT, "bench.py")) as f:
        tree = ast.parse(f.read())
    allowed = {"cpu_baseline", "reference_kernels_on_this_gpu"}
    for node in ast.walk(tree):
        if isinstance(node, ast.FunctionDef):
            for sub in ast.walk(node):
                if isinstance(sub, ast.ImportFrom) and sub.module and sub.module.split(".")[0] == "oracle":
                    assert node.name in allowed, "bench.py::%s imports the oracle" % node.name
    top = [n for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom))]
    assert not any(getattr(n, "module", "") and n.module.split(".")[0] == "oracle" for n in top)


def test_fdgs_adam_rejects_what_it_does_not_implement():
    """fdgs.optim.Adam (the torch.optim.Optimizer of the drop-in path): no weight decay / amsgrad, no CPU parameters."""
    import pytest
    import torch
    from fdgs.optim import Adam
    p = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(ValueError, match="weight_decay"):
        Adam([{"params": [p], "name": "xyz"}], lr=0.0, weight_decay=0.1)
    opt = Adam([{"params": [p], "name": "xyz"}], lr=0.0)
    assert not opt.bucketable() and not opt.ensure_homed()
    p.grad = torch.ones(4)
    with pytest.raises(RuntimeError, match="GPU"):
        opt.step()


def test_blend_bwd_inline_asm_register_allocation():
    """csrc/blend_bwd.hip's joint DPP reductions take b[] as plain inputs that are read after a[] has been written; that no b[k]
    shares a VGPR with an a[j] is checked in the gfx950 assembly the compiler produces (tools/check_reduce_regs.py), so that a
    compiler bump cannot break it silently."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("check_reduce_regs", os.path.join(ROOT, "tools", "check_reduce_regs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    sizes = [r[0] for r in mod.check()]
    assert 9 in sizes and 12 in sizes


def test_register_budgets_of_the_built_kernels():
    """Occupancy is part of the design (DESIGN.md sections 4 and 8): the per-Gaussian kernels are built without the SLP vectorizer, whose
    packed operations on register pairs cost preprocess_fwd 62 VGPRs and preprocess_bwd 35; the SSIM forward filters four packed channels.
    The VGPR counts of the gfx950 code the compiler produces with build.sh's flags are checked here, so that a flag that goes missing or a
    compiler bump shows up as a failed test and not as a slower step."""
    import re
    import subprocess
    from concurrent.futures import ThreadPoolExecutor
    csrc = os.path.join(ROOT, "4d-gaussian-splatting_amd", "csrc")
    with open(os.path.join(csrc, "build.sh")) as f:
        sh = f.read()
    extra = dict(re.findall(r'\[(\w+)\]="([^"]*)"', re.search(r"declare -A EXTRA=\((.*?)\)\n", sh, re.S).group(1)))
    common = re.search(r'COMMON="([^"]*)"', sh).group(1).replace("$ARCH", "gfx950").split()
    budgets = {   # kernel name fragment -> (translation unit, most VGPRs, fewest waves per SIMD that means)
        "preprocess_fwd_kernelILi0E": ("preprocess_fwd", 184, 2), "preprocess_fwd_kernelILi2E": ("preprocess_fwd", 168, 3),
        "preprocess_bwd_kernelE": ("preprocess_bwd", 104, 4), "ssim_fwd_kernel": ("ssim", 96, 5), "ssim_bwd_kernel": ("ssim", 96, 5),
    }

    def vgprs(tu):
        cmd = ["/opt/rocm/bin/hipcc"] + common + extra.get(tu, "").split() + ["-S", "--cuda-device-only", "-o", "-", os.path.join(csrc, tu + ".hip")]
        asm = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
        return {m.group(1): (int(m.group(2)), int(m.group(3))) for m in
                re.finditer(r"\.name:\s+(\S+)\n.*?\.vgpr_count:\s+(\d+)\n.*?\.vgpr_spill_count:\s+(\d+)", asm, re.S)}
    tus = sorted({v[0] for v in budgets.values()})
    with ThreadPoolExecutor(len(tus)) as ex:
        got = dict(zip(tus, ex.map(vgprs, tus)))
    for frag, (tu, most, waves) in budgets.items():
        hits = {k: v for k, v in got[tu].items() if frag in k}
        assert hits, (frag, list(got[tu]))
        for name, (n, spills) in hits.items():
            assert n <= most and spills == 0, "%s: %d VGPRs, %d spills (budget %d = %d waves per SIMD)" % (name, n, spills, most, waves)
            assert 512 // ((n + 7) // 8 * 8) >= waves, (name, n)


# (entry point, arguments it rejects before its first HIP call, text its message must carry).  The first block: every entry point
# that used to return a bare code without a message -- its new message names it.  The second: one entry point of each other
# translation unit, with the text it always had.
_N = None
_REJECTED = [
    ("fdgs_l1_ssim_value_and_grad", (_N, _N, 0, 0, 0, _N, 0.2, _N, _N, _N, _N), "fdgs_l1_ssim_value_and_grad"),
    ("fdgs_l1_ssim_forward", (_N, _N, 0, 0, 0, _N, _N, _N, _N, _N, _N), "fdgs_l1_ssim_forward"),
    ("fdgs_l1_ssim_backward", (_N, _N, 0, 0, 0, _N, _N, _N, _N, 0.2, _N, _N), "fdgs_l1_ssim_backward"),
    ("fdgs_l1_ssim_loss", (_N, _N, 0, 3, 16, 16, 0.2, _N, _N), "fdgs_l1_ssim_loss"),
    ("fdgs_l1_ssim_loss_batch", (_N, 0, 1, 3, 16, 16, 0.2, _N, _N), "fdgs_l1_ssim_loss_batch"),
    ("fdgs_densify_stats_local", (-1, 1, _N, _N, _N, _N, _N, _N), "fdgs_densify_stats_local"),
    ("fdgs_densify_stats_local", (8, 1, _N, _N, _N, _N, _N, _N), "fdgs_densify_stats_local"),
    ("fdgs_densify_stats_apply", (-1, _N, _N, _N, _N, 1.0, _N, _N, _N, _N, _N), "fdgs_densify_stats_apply"),
    ("fdgs_densify_stats_apply", (8, _N, _N, _N, _N, 1.0, _N, _N, _N, _N, _N), "fdgs_densify_stats_apply"),
    ("fdgs_densify_classify", (-1, _N, _N, _N, _N, _N, 1.0, 1.0, 1.0, 1.0, 1.0, 2, 0, _N, _N), "fdgs_densify_classify"),
    ("fdgs_densify_classify", (8, _N, _N, _N, _N, _N, 1.0, 1.0, 1.0, 1.0, 1.0, 2, 0, _N, _N), "fdgs_densify_classify"),
    ("fdgs_densify_gather", (0, _N, 0, 0) + (_N,) * 9, "fdgs_densify_gather"),
    ("fdgs_densify_split", (-1, 2, 0, 4) + (_N,) * 14, "fdgs_densify_split"),
    ("fdgs_densify_split", (8, 2, 0, 4) + (_N,) * 14, "fdgs_densify_split"),
    ("fdgs_dist2_knn3", (-1, _N, _N, _N, _N), "fdgs_dist2_knn3"),
    ("fdgs_dist2_knn3", (8, _N, _N, _N, _N), "fdgs_dist2_knn3"),
    ("fdgs_adam_step", (_N, _N, _N, _N, 0, _N, 0, 0.9, 0.999, 1e-15, 1, _N), "fdgs_adam_step"),
    ("fdgs_adam_step_sh", (_N, _N, _N, _N, -1, 0, 0, 0, 4, 0, 0, 1, _N, 1e-3, 1e-3, 0.9, 0.999, 1e-15, 1, _N), "fdgs_adam_step_sh"),
    ("fdgs_profile_read", (99, _N, _N), "fdgs_profile_read"),
    ("fdgs_profile_sample_every", (0,), "fdgs_profile_sample_every"),
    ("fdgs_set_sparse_lists_budget", (-1, 1), "fdgs_set_sparse_lists_budget"),

    ("fdgs_mark_visible", (-1, _N, _N, _N, _N, _N), "P < 0"),
    ("fdgs_rigid_motion_forward", (0, 1) + (_N,) * 11, "fdgs_rigid_motion_forward: no Gaussians"),
    ("fdgs_opa_mask_loss", (0, 0, _N, 0, _N, _N, 1.0, _N, 0, _N, _N, _N), "fdgs_opa_mask_loss: bad image size"),
    ("fdgs_env_composite", (0, 0, _N, _N, 1.0, 1.0, 0.0, 0.0, _N, 1, 1, 1.0, _N, _N, _N, _N), "fdgs_env_composite: bad image / map size"),
    ("fdgs_eval_metrics", (_N, _N, 3, 16, 16, 0, _N, _N, _N), "fdgs_eval_metrics: missing pointer"),
    ("fdgs_frames_decode", (_N, 1, 1, 1, 5, _N, 1, _N, 0, _N, 0, _N), "fdgs_frames_decode: C must be 3"),
    ("fdgs_frames_encode", (_N, 0, _N, 0, 1, 1, 1, 5, _N, 1, _N, _N), "fdgs_frames_encode: C must be 3"),
    ("fdgs_frames_resize", (_N, 1, 1, 1, 5, _N, 1, _N, 1, 1, 1, _N, _N, 1, _N, _N, 1, _N, _N), "fdgs_frames_resize: C must be 3"),
    ("fdgs_knn_query", (-1, 0, 0, 1, _N, _N, _N, _N, _N, _N), "fdgs_knn_query: negative size"),
    ("fdgs_kmeans_assign", (0, 1, 1, _N, _N, _N, _N, _N, _N), "fdgs_kmeans_assign: N must be at least 1 (N=0 K=1 D=1)"),
    ("fdgs_gaussian_flow_forward", (_N, _N, _N), "fdgs_gaussian_flow_forward: in must not be NULL"),
    ("fdgs_depth_normals", (_N, 1.0, 1.0, 0.0, 0.0, _N, _N, _N, _N), "fdgs_depth_normals: in must not be NULL"),
    ("fdgs_tsdf_integrate", (_N, 0, _N, _N), "fdgs_tsdf_integrate: volume must not be NULL"),
    ("fdgs_surface_extract", (_N, 0.0, _N, _N, _N), "fdgs_surface_extract: volume must not be NULL"),
    ("fdgs_mesh_smooth", (_N, _N, _N, _N), "fdgs_mesh_smooth: mesh must not be NULL"),
    ("fdgs_mesh_simplify", (_N, _N, _N, _N, _N), "fdgs_mesh_simplify: mesh must not be NULL"),
]


@pytest.mark.parametrize("row", range(len(_REJECTED)), ids=lambda i: "%s-%d" % (_REJECTED[i][0], i))
def test_every_rejection_carries_its_own_message(row):
    """fdgs_last_error() describes the call that failed, not an earlier one: after the rasterizer's "bad sizes" failure on the same
    thread, every rejected call leaves its own text.  All of these are turned away before anything touches the GPU."""
    from fdgs import _capi
    name, args, text = _REJECTED[row]
    scene, out, R = _capi.FdgsScene(), _capi.FdgsForwardOut(), C.c_int32(0)
    scene.P, scene.W, scene.H = 10, 0, 16
    cb = _capi.ALLOC_FN(lambda u, w, n: None)
    assert _capi.lib.fdgs_rasterize_forward(C.byref(scene), C.byref(out), cb, None, None, C.byref(R)) == 1
    assert "bad sizes" in _capi.last_error()   # the poison
    assert getattr(_capi.lib, name)(*args) == 1
    err = _capi.last_error()
    print(name, "->", err)
    assert text in err and "bad sizes" not in err


def test_every_nonzero_return_goes_through_fail():
    """No source line under csrc/ returns an error code directly: fdgs::fail (capi.hip) writes the message and returns the code, and
    nothing else does.  The helpers it replaced are gone."""
    src = os.path.join(ROOT, "4d-gaussian-splatting_amd", "csrc")
    files = sorted(f for f in os.listdir(src) if f.endswith((".hip", ".h")))
    assert "capi.hip" in files and "fdgs_common.h" in files and len(files) >= 30
    for f in files:
        with open(os.path.join(src, f)) as fh:
            text = fh.read()
        if f == "capi.hip":   # the definition of fail is the one place a code may be returned from
            m = re.search(r"^int fdgs::fail\(int code, const char\* fmt, \.\.\.\)\n\{\n.*?^\}\n", text, flags=re.S | re.M)
            assert m and "return code;" in m.group(0)
            text = text.replace(m.group(0), "")
        assert "return FDGS_ERR_" not in text, f
        for gone in ("set_error", "mesh_fail", "tsdf_fail", "flow_fail", "depth_fail"):
            assert gone not in text, (f, gone)


def test_scratch_sizes_did_not_move():
    """Every exported *_bytes / *_scratch* function returns what the build before the layouts were rewritten returned
    (tests/golden/scratch_sizes.json, recorded from that build by tests/golden/make_golden_scratch_sizes.py)."""
    import json
    from fdgs import _capi
    with open(os.path.join(ROOT, "tests", "golden", "scratch_sizes.json")) as f:
        table = json.load(f)
    with open(os.path.join(ROOT, "include", "fdgs.h")) as f:
        declared = set(re.findall(r"\b(fdgs_\w*(?:_bytes|scratch)\w*)\s*\(", re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)))
    assert declared == set(table) and len(declared) == 19
    for name, rows in table.items():
        assert len(rows) >= 6
        for args, want in rows:
            assert int(getattr(_capi.lib, name)(*args)) == want, (name, args)


def _golden_module(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_signatures_did_not_move():
    """restype / argtypes of every exported function and the layout of every struct are what the binding had when each function spelled
    them out (tests/golden/capi_signatures.json, recorded from that commit by tests/golden/make_golden_capi_signatures.py).  The one
    difference: the three functions without arguments went from unset argtypes to an empty list.  EXPORTED is the table's keys."""
    import json
    from fdgs import _capi
    with open(os.path.join(ROOT, "tests", "golden", "capi_signatures.json")) as f:
        want = json.load(f)
    for name in ("fdgs_profile_reset", "fdgs_last_error", "fdgs_version"):
        assert want["functions"][name]["argtypes"] is None
        want["functions"][name]["argtypes"] = []
    got = _golden_module("make_golden_capi_signatures").describe(_capi)
    assert set(got["functions"]) == set(want["functions"]) and set(got["structs"]) == set(want["structs"])
    for name, sig in want["functions"].items():
        assert got["functions"][name] == sig, name
    for name, layout in want["structs"].items():
        assert got["structs"][name] == layout, name
    assert len(_capi.EXPORTED) == len(set(_capi.EXPORTED)) == 95 and set(_capi.EXPORTED) == set(_capi.SIGNATURES)
    for name, (restype, argtypes) in _capi.SIGNATURES.items():
        fn = getattr(_capi.lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


class _NoGuard:
    entered = 0

    def __init__(self, dev):
        type(self).entered += 1

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def test_call_path(monkeypatch):
    """_capi.call without a GPU: a recording stub in place of one entry point, a counting null context in place of torch.cuda.device."""
    from fdgs import _capi
    seen, rc = [], [0]

    def stub(*args):
        seen.append(args)
        return rc[0]
    stream = C.c_void_p(0x1234)
    monkeypatch.setattr(_capi.lib, "fdgs_mark_visible", stub)
    monkeypatch.setattr(_capi, "current_stream_handle", lambda dev: stream)
    monkeypatch.setattr(_capi, "last_error", lambda: "the library's own text")
    monkeypatch.setattr(torch.cuda, "device", _NoGuard)
    _NoGuard.entered = 0
    assert _capi.call("fdgs_mark_visible", "cuda:0", 7, None, "x") is None          # rc == 0 returns
    assert seen == [(7, None, "x", stream)] and _NoGuard.entered == 1              # the stream last, once; the guard entered once
    _capi.call("fdgs_mark_visible", "cuda:0", 8, guard=False)
    assert seen[1] == (8, stream) and _NoGuard.entered == 1                        # the no-guard form does not enter it
    own = C.c_void_p(0)                                                            # (the null stream: falsy, and still the one passed)
    _capi.call("fdgs_mark_visible", "cuda:0", 9, guard=False, stream=own)
    assert seen.pop() == (9, own)                                                  # a stream of the caller's takes the current one's place
    rc[0] = 1
    with pytest.raises(Exception) as e:
        _capi.call("fdgs_mark_visible", "cuda:0", 1)
    assert type(e.value) is Exception and str(e.value) == "the library's own text"
    with pytest.raises(ValueError) as e:                                            # fdgs.metrics / frames / resize
        _capi.call("fdgs_mark_visible", "cuda:0", 1, arg_error=ValueError)
    assert type(e.value) is ValueError and str(e.value) == "the library's own text"
    rc[0] = 2
    for kw in ({}, {"arg_error": ValueError}, {"guard": False}):
        with pytest.raises(RuntimeError) as e:
            _capi.call("fdgs_mark_visible", "cuda:0", 1, **kw)
        assert str(e.value) == "fdgs_mark_visible failed (code 2): the library's own text"
    assert all(a[-1] is stream and sum(x is stream for x in a) == 1 for a in seen) and _NoGuard.entered == 5


def _rejections():
    import json
    with open(os.path.join(ROOT, "tests", "golden", "cpu_rejections.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(_rejections()))
def test_cpu_rejections_did_not_move(name):
    """Every public function that refuses CPU tensors before it touches the GPU raises the type and the text it raised before the
    refusals were folded into _capi.need_gpu (tests/golden/cpu_rejections.json, recorded by tests/golden/make_golden_cpu_rejections.py
    from the calls in tests/cpu_rejection_cases.py).  Not covered, because a GPU is needed to get as far as their check: fdgs.optim.Adam
    (test_fdgs_adam_rejects_what_it_does_not_implement above has it), compress.decode_into's q / rows / index, update's codebook / index."""
    import cpu_rejection_cases
    table, calls = _rejections(), dict(cpu_rejection_cases.cases())
    assert set(table) == set(calls) and {n.split(".")[0] for n in table} >= {
        "depth", "features", "flow", "surface", "compress", "knn", "loss", "metrics", "envmap", "slice", "edit", "importance", "frames", "resize"}
    got = _golden_module("make_golden_cpu_rejections").record(calls[name])
    assert got == table[name]


def test_every_launch_goes_through_call():
    """The Python side's counterpart of test_every_nonzero_return_goes_through_fail: outside _capi.py no module checks a return code,
    spells the no-CPU-path sentence or sizes a byte buffer itself -- _capi.call, need_gpu and scratch do."""
    pkg = os.path.join(ROOT, "4d-gaussian-splatting_amd")
    files = [os.path.join(d, f) for d, _, fs in os.walk(pkg) for f in fs if f.endswith(".py") and f != "_capi.py"]
    assert len(files) >= 28
    for path in files:
        with open(path) as fh:
            for n, line in enumerate(fh, 1):
                where = "%s:%d" % (os.path.relpath(path, ROOT), n)
                assert not re.search(r"rc = _capi\.lib\.", line), where
                assert not re.search(r"_capi\._check\(", line), where
                assert "must live on the GPU (got" not in line, where
                assert not ("dtype=torch.uint8" in line and "_bytes(" in line), where
