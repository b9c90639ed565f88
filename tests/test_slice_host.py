"""CPU: the float64 statement of the time slice (tests/slice_oracle.py) against fixtures made with the reference's own functions
(tests/golden/make_golden_slice.py), the PLY round trip of fdgs.slice and its argument errors."""
import glob
import os

import numpy as np
import pytest
import torch

import slice_oracle as so

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "slice")
GEO = sorted(glob.glob(os.path.join(GOLDEN, "geo_*.npz")))
SH = sorted(glob.glob(os.path.join(GOLDEN, "sh_t*.npz")))


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def test_fixture_set_is_complete():
    names = {os.path.basename(p) for p in GEO}
    assert names == {"geo_%s_pf%s_mod%s.npz" % (r, p, m) for r in ("rot4d", "dim4") for p in ("on", "off") for m in ("1", "07")}
    assert [os.path.basename(p) for p in SH] == ["sh_t0.npz", "sh_t1.npz", "sh_t2.npz"]


@pytest.mark.parametrize("path", GEO, ids=[os.path.basename(p)[:-4] for p in GEO])
def test_oracle_geometry_matches_the_reference(path):
    """Means, cov6 and marginal of the oracle against the reference's get_current_covariance_and_mean_offset / get_covariance /
    get_marginal_t, float64 against float64: 1e-12 relative."""
    d = np.load(path)
    rot_4d, mod, t, pv = bool(d["rot_4d"]), float(d["mod"]), float(d["timestamp"]), float(d["prefilter_var"])
    assert d["xyz"].dtype == np.float64
    p = {"xyz": d["xyz"], "opacity": np.ones(d["xyz"].shape[0]), "scales": np.exp(d["scaling"]), "scales_t": np.exp(d["scaling_t"]).reshape(-1),
         "rot": d["rotation"], "rot_r": d["rotation_r"], "ts": d["t"].reshape(-1)}
    sl = so.slice_oracle(p, t, mod=mod, prefilter_var=pv, rot_4d=rot_4d)
    if rot_4d:
        assert _rel(sl["cov6"], d["cov"]) <= 1e-12
    else:
        # The reference has two 3D covariances: its kernel builds R S^2 R^T (forward.cu:242-276, GLM fills R column by column), its
        # Python get_covariance R^T S^2 R (L = S R, L^T L).  The slice follows the kernel, whose bits it must reproduce; the fixture
        # holds the Python one, which is the kernel's at the conjugate quaternion (R(q*) = R(q)^T).
        conj = d["rotation"] * np.array([1.0, -1.0, -1.0, -1.0])
        assert _rel(so.upper6(so.sigma3(p["scales"], conj, mod)), d["cov"]) <= 1e-12
        assert _rel(sl["cov6"], so.upper6(so.sigma3(p["scales"], d["rotation"], mod))) == 0.0
    assert _rel(sl["marginal"], d["marginal_t"].reshape(-1)) <= 1e-12
    assert _rel(sl["opacity"], d["marginal_t"].reshape(-1)) <= 1e-12
    want_xyz = d["xyz"] + d["mean_offset"] if rot_4d else d["xyz"]
    assert _rel(sl["xyz"], want_xyz) <= 1e-12
    assert np.array_equal(sl["live"], d["marginal_t"].reshape(-1) > 0.05)
    assert 0 < sl["live"].sum() < sl["live"].size, "the fixture should have Gaussians on both sides of the cull"
    assert np.array_equal(sl["index"], np.nonzero(sl["live"])[0]) and (np.diff(sl["index"]) > 0).all()


@pytest.mark.parametrize("path", SH, ids=[os.path.basename(p)[:-4] for p in SH])
def test_folded_row_evaluates_to_the_4d_colour(path):
    """eval_sh(3, folded row, dirs) == the reference's eval_shfs_4d(3, D_t, sh, dirs, dirs_t, T) to 1e-6."""
    from fdgs.sh_utils import eval_sh
    d = np.load(path)
    D_t, T = int(d["D_t"]), float(d["T"])
    ts = d["dirs_t"].reshape(-1)                       # dir_t = ts - t with t = 0
    t1, t2 = so.time_factors(ts, 0.0, T)
    folded = so.fold_sh(d["sh"], t1, t2, 3, D_t)
    got = eval_sh(3, torch.from_numpy(folded).transpose(1, 2), torch.from_numpy(d["dirs"])).numpy()
    assert np.abs(got - d["colour"]).max() <= 1e-6
    if D_t > 0:   # the time blocks matter: without them the colour is off by far more than the bar
        plain = eval_sh(3, torch.from_numpy(d["sh"].astype(np.float64)[:, :16]).transpose(1, 2), torch.from_numpy(d["dirs"])).numpy()
        assert np.abs(plain - d["colour"]).max() > 1e-2


def test_fold_respects_degree_and_force_sh_3d():
    """A self-check of tests/slice_oracle.py alone (it runs no code of the package): the statement the GPU test of the folded rows
    is held to must itself truncate at (D + 1)^2 and leave the time blocks out below degree 3 and with force_sh_3d."""
    g = np.random.default_rng(0)
    sh = g.standard_normal((5, 48, 3))
    t1, t2 = g.standard_normal(5), g.standard_normal(5)
    for D in (0, 1, 2):
        out = so.fold_sh(sh, t1, t2, D, 2)
        n0 = (D + 1) ** 2
        assert np.array_equal(out[:, :n0], sh[:, :n0]) and not out[:, n0:].any()
    assert np.array_equal(so.fold_sh(sh, t1, t2, 3, 2, force_sh_3d=True), sh[:, :16])
    assert np.allclose(so.fold_sh(sh, t1, t2, 3, 1), sh[:, :16] + t1[:, None, None] * sh[:, 16:32], rtol=0, atol=1e-15)


# ---- PLY ----

def _read_ply(path):
    """A reader of its own: header lines -> (property names, [n, len(names)] float32)."""
    with open(path, "rb") as fh:
        raw = fh.read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").strip().split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    n = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[2])
    names = []
    for ln in lines[3:]:
        kind, typ, name = ln.split()
        assert kind == "property" and typ == "float"
        names.append(name)
    assert len(body) == 4 * n * len(names)
    return names, np.frombuffer(body, "<f4").reshape(n, len(names))


def _cpu_slice(n=37, seed=3, decompose=True):
    from fdgs.slice import TimeSlice
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    q = torch.nn.functional.normalize(rn(n, 4), dim=1)
    opacity = torch.rand(n, generator=g)
    scales = torch.exp(rn(n, 3) - 3.0)
    if n > 2:
        opacity[0], opacity[1] = 1.0, 0.0      # a saturated sigmoid and an underflowed one: their logits must stay finite
        scales[2, 0] = 1e-15                   # the kernel's floor
    return TimeSlice(n, torch.arange(n, dtype=torch.int32) * 2, rn(n, 3), rn(n, 6), opacity, rn(n, 16, 3), 3,
                     scales if decompose else None, q if decompose else None, 2 * n, 0.25)


def test_ply_round_trip_is_bitwise(tmp_path):
    from fdgs.slice import PLY_PROPERTIES, load_ply, ply_fields, save_ply
    sl = _cpu_slice()
    path = str(tmp_path / "slice.ply")
    save_ply(path, sl)
    names, rows = _read_ply(path)
    assert names == (["x", "y", "z", "nx", "ny", "nz"] + ["f_dc_%d" % i for i in range(3)] + ["f_rest_%d" % i for i in range(45)]
                     + ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]) == list(PLY_PROPERTIES)
    assert rows.shape == (sl.n, 62) and np.isfinite(rows).all()
    want = ply_fields(sl)
    assert np.array_equal(rows.view(np.uint32), want.view(np.uint32))
    col = {k: i for i, k in enumerate(names)}
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)  # noqa: E731
    shs = sl.shs.numpy()
    assert np.array_equal(bits(rows[:, 0:3]), bits(sl.xyz.numpy())) and not rows[:, 3:6].any()
    for c in range(3):   # channel-major: f_rest_{c * 15 + (k - 1)} is coefficient k of channel c
        assert np.array_equal(bits(rows[:, col["f_dc_%d" % c]]), bits(shs[:, 0, c]))
        for k in (1, 7, 15):
            assert np.array_equal(bits(rows[:, col["f_rest_%d" % (c * 15 + k - 1)]]), bits(shs[:, k, c]))
    # logit and log of what the slice holds (float64, rounded once)
    o = sl.opacity.numpy().astype(np.float64)
    mid = slice(2, None)
    assert np.allclose(rows[mid, col["opacity"]], np.log(o[mid] / (1 - o[mid])), rtol=1e-6, atol=1e-6)
    assert np.allclose(rows[:, col["scale_0"]], np.log(sl.scales.numpy()[:, 0].astype(np.float64)), rtol=1e-6)
    m = load_ply(path, "cpu")
    assert m.gaussian_dim == 3 and not m.rot_4d and m.max_sh_degree == 3 and m._xyz.shape[0] == sl.n
    assert np.array_equal(bits(m._xyz.detach().numpy()), bits(sl.xyz.numpy()))
    assert np.array_equal(bits(m._features.detach().numpy()), bits(shs))
    assert np.array_equal(bits(m._rotation.detach().numpy()), bits(sl.rotations.numpy()))
    assert np.array_equal(bits(m._opacity.detach().numpy().reshape(-1)), bits(want[:, 54]))
    assert np.array_equal(bits(m._scaling.detach().numpy()), bits(want[:, 55:58]))
    # and what the 3D model's activations give back is the slice, to the rounding of one log / exp pair
    assert np.allclose(m.get_scaling.detach().numpy(), sl.scales.numpy(), rtol=1e-5, atol=0)
    assert np.allclose(m.get_opacity.detach().numpy().reshape(-1)[mid], sl.opacity.numpy()[mid], rtol=1e-5, atol=1e-7)


def test_ply_of_an_empty_slice(tmp_path):
    from fdgs.slice import save_ply
    sl = _cpu_slice(n=0)
    path = str(tmp_path / "empty.ply")
    save_ply(path, sl)
    names, rows = _read_ply(path)
    assert len(names) == 62 and rows.shape == (0, 62)


def test_argument_errors():
    from fdgs.slice import save_ply, time_slice

    class Model3D:
        gaussian_dim = 3

    with pytest.raises(ValueError, match="3D"):
        time_slice(Model3D(), 0.5)
    with pytest.raises(ValueError, match="decompose=True"):
        save_ply("/nonexistent/never_written.ply", _cpu_slice(decompose=False))


def test_c_entry_checks_its_arguments_without_touching_the_gpu():
    import ctypes as C
    from fdgs import _capi
    a_in, a_out = _capi.FdgsSliceIn(), _capi.FdgsSliceOut()
    assert a_in.struct_size == C.sizeof(_capi.FdgsSliceIn) and a_out.struct_size == C.sizeof(_capi.FdgsSliceOut)
    assert _capi.lib.fdgs_time_slice(None, None, None, None) == 1
    a_in.struct_size -= 4
    assert _capi.lib.fdgs_time_slice(C.byref(a_in), C.byref(a_out), None, None) == 1
    assert "struct_size" in _capi.last_error() and "fdgs_slice_in" in _capi.last_error()
    a_in.struct_size += 4
    a_in.P = 10
    assert _capi.lib.fdgs_time_slice(C.byref(a_in), C.byref(a_out), None, None) == 1 and "n_live" in _capi.last_error()
    a_in.P = -1
    assert _capi.lib.fdgs_time_slice(C.byref(a_in), C.byref(a_out), None, None) == 1 and "bad sizes" in _capi.last_error()
    # sizes and pointers fine, time blocks active and a zero duration: the time factors would divide by it
    a_in.P, a_in.D, a_in.D_t, a_in.M, a_in.time_duration = 10, 3, 1, 48, 0.0
    for f in ("means3D", "shs", "opacities", "ts", "scales", "scales_t", "rotations"):
        setattr(a_in, f, 256)   # never dereferenced: the call is turned away first
    a_out.n_live = 256
    assert _capi.lib.fdgs_time_slice(C.byref(a_in), C.byref(a_out), 256, None) == 1 and "time_duration" in _capi.last_error()
    a_in.M, a_in.time_duration = 16, 1.0
    assert _capi.lib.fdgs_time_slice(C.byref(a_in), C.byref(a_out), 256, None) == 1 and "too small" in _capi.last_error()
    b0, b1 = _capi.lib.fdgs_time_slice_scratch_bytes(1), _capi.lib.fdgs_time_slice_scratch_bytes(300000)
    assert 0 < b0 <= b1 and b1 % 256 == 0 and b1 < 300000   # 36 bytes per 256 Gaussians
