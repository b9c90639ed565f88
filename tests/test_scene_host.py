"""CPU: fdgs.scene against what the reference's readers and camera code made of the same folders (tests/golden/scene, recorded by
tests/golden/make_golden_scene.py), the point-cloud PLY reader / writer, and the ValueErrors of fdgs.scene / fdgs.seed.

Bars: R, T, the fields of view and the timestamps are float64 results of the same numpy calls: exact.  ``world_view_transform`` is
computed in float64 and cast: exact.  ``full_proj_transform`` (a float32 4x4 product) and ``camera_center`` (a float32 inverse) are the
reference's own float32 arithmetic, repeated here with the same torch calls: held to float32 round-off of the entries they are made
of, 4 x 2^-23 x the largest magnitude of the matrix."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "scene")
CASES = ("fov", "frame_intrinsics", "global_intrinsics")


def _recorder():
    spec = importlib.util.spec_from_file_location("make_golden_scene", os.path.join(ROOT, "tests", "golden", "make_golden_scene.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    rec, out = _recorder(), {}
    for case in CASES:
        with open(os.path.join(GOLD, case + ".json")) as f:
            spec = json.load(f)
        folder = str(tmp_path_factory.mktemp(case))
        rec.write_folder(folder, spec)
        out[case] = (folder, spec, dict(np.load(os.path.join(GOLD, case + ".npz"))))
    return rec, out


def _f32_close(got, want):
    tol = 4 * 2.0 ** -23 * float(np.abs(want).max())
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= tol


@pytest.mark.parametrize("case", CASES)
def test_cameras_against_the_recorded_reference(folders, case):
    from fdgs import scene
    rec, table = folders
    folder, spec, want = table[case]
    for read, kw in rec.READS.items():
        for split in ("train", "test"):
            infos = scene.read_transforms(folder, "transforms_%s.json" % split, **kw)
            tag = "%s/%s" % (read, split)
            assert len(infos) == len(want[tag + "/time"]) > 0
            assert np.array_equal(np.stack([c.R for c in infos]), want[tag + "/R"])
            assert np.array_equal(np.stack([c.T for c in infos]), want[tag + "/T"])
            assert np.array_equal(np.array([[c.FovX, c.FovY] for c in infos]), want[tag + "/fov"])
            assert np.array_equal(np.array([[c.fl_x, c.fl_y, c.cx, c.cy] for c in infos]), want[tag + "/intr"])
            assert np.array_equal(np.array([c.timestamp for c in infos]), want[tag + "/time"])
            for res in (1, 2):
                cams = [scene.Camera(c, (round(c.width / res), round(c.height / res)), scale=res) for c in infos]
                wv = np.stack([c.world_view_transform.numpy() for c in cams])
                assert np.array_equal(wv, want["%s/res%d/world_view_transform" % (tag, res)])
                _f32_close(np.stack([c.full_proj_transform.numpy() for c in cams]), want["%s/res%d/full_proj_transform" % (tag, res)])
                _f32_close(np.stack([c.camera_center.numpy() for c in cams]), want["%s/res%d/camera_center" % (tag, res)])
                for c in cams:
                    assert (c.image_width, c.image_height) == (round(spec["width"] / res), round(spec["height"] / res))
                    assert 0.0 < c.FoVx < np.pi and 0.0 < c.FoVy < np.pi and c.timestamp == infos[cams.index(c)].timestamp
                    if case != "fov":      # centre shift: the third row of the (transposed) projection is filled
                        assert c.projection_matrix[2, 0] != 0.0 or c.cx == c.image_width / 2
    if case == "fov":
        assert all(c.cx == c.image_width / 2 and c.projection_matrix[2, 0] == 0.0 for c in cams)


@pytest.mark.parametrize("case", CASES)
def test_filtering_eval_and_extent(folders, case):
    from fdgs import scene
    rec, table = folders
    folder, spec, want = table[case]
    for read, kw in rec.READS.items():
        for ev in (True, False):
            sc = scene.Scene(folder, eval=ev, **kw)
            tag = "%s/%s" % (read, "eval" if ev else "merged")
            assert [c.uid for c in sc.train_infos] == want[tag + "/train_uids"].tolist()
            assert [c.uid for c in sc.test_infos] == want[tag + "/test_uids"].tolist()
            assert (len(sc.test_infos) == 0) == (not ev)
            assert sc.cameras_extent == float(want[tag + "/radius"])
            assert np.array_equal(sc.nerf_normalization["translate"], want[tag + "/translate"])
            assert sc.cloud is None and len(sc.cameras("train")) == len(sc.train_infos)
    full, window = scene.Scene(folder, eval=True), scene.Scene(folder, eval=True, time_duration=[0.2, 0.8])
    assert len(window.train_infos) < len(full.train_infos) == 6
    assert all(0.2 <= c.timestamp <= 0.8 for c in window.train_infos)
    half = scene.Scene(folder, eval=True, time_duration=[0.0, 0.3], frame_ratio=2)
    assert [c.timestamp for c in half.train_infos] == [c.timestamp / 2 for c in full.train_infos if c.timestamp / 2 <= 0.3]


def _cloud(n, timed, seed=0):
    from fdgs.seed import PointCloud
    g = torch.Generator().manual_seed(seed)
    return PointCloud(torch.randn((n, 3), generator=g), torch.randint(0, 256, (n, 3), generator=g).float() / 255.0,
                      torch.rand(n, generator=g) if timed else None)


@pytest.mark.parametrize("timed", [True, False], ids=["time", "no_time"])
@pytest.mark.parametrize("normals", [True, False], ids=["normals", "no_normals"])
@pytest.mark.parametrize("binary", [True, False], ids=["binary", "ascii"])
def test_ply_round_trip(tmp_path, binary, normals, timed):
    from fdgs import seed
    cloud = _cloud(37, timed)
    path = str(tmp_path / "points3d.ply")
    seed.save_ply(path, cloud, binary=binary, normals=normals)
    with open(path, "rb") as f:
        head = f.read(400).split(b"end_header")[0].decode()
    assert ("binary_little_endian" in head) == binary and ("property float nx" in head) == normals and ("property float time" in head) == timed
    back = seed.load_ply(path)
    assert torch.equal(back.xyz, cloud.xyz)                                    # float32 survives both formats
    assert torch.equal((back.rgb * 255).round(), (cloud.rgb * 255).round())      # 8-bit colours
    assert (back.t is None) == (not timed) and (not timed or torch.equal(back.t, cloud.t))
    v = seed.read_ply_vertices(path)
    assert v["red"].dtype == np.uint8 and v["x"].dtype == np.float32 and (("nx" in v) == normals)
    empty = str(tmp_path / "empty.ply")
    seed.save_ply(empty, _cloud(0, timed), binary=binary)
    assert len(seed.load_ply(empty)) == 0


def test_scene_reads_points3d_ply(folders, tmp_path):
    from fdgs import scene, seed
    rec, table = folders
    _, spec, _ = table["fov"]
    folder = str(tmp_path)
    rec.write_folder(folder, spec)
    seed.save_ply(os.path.join(folder, "points3d.ply"), _cloud(50, True))
    sc = scene.Scene(folder, eval=True, time_duration=[0.0, 1.0])
    assert len(sc.cloud) == 50 and sc.cloud.t is not None and sc.cloud.device.type == "cpu"


def test_value_errors(folders, tmp_path):
    from PIL import Image
    from fdgs import scene, seed
    rec, table = folders
    _, spec, _ = table["fov"]
    folder = str(tmp_path)
    rec.write_folder(folder, spec)
    with pytest.raises(ValueError, match="num_pts"):
        scene.Scene(folder, num_pts=0)
    with pytest.raises(ValueError, match="transforms_train.json"):
        scene.Scene(os.path.join(folder, "train"))
    Image.new("RGB", (spec["width"] + 2, spec["height"]), (0, 0, 0)).save(os.path.join(folder, "train", "r_1.png"))
    with pytest.raises(ValueError, match="mixed image sizes"):
        scene.Scene(folder)
    with pytest.raises(ValueError, match="mixed image sizes"):
        scene.load_rgba(scene.read_transforms(folder, "transforms_train.json"))
    # thinning: key-range overflow, sizes and non-finite coordinates are turned away before anything needs a GPU
    cloud = _cloud(100, True)
    with pytest.raises(ValueError, match="65536"):
        seed.thin(cloud, 1e-6)
    with pytest.raises(ValueError, match="65536"):
        seed.thin(cloud, 0.5, 1e-9)
    with pytest.raises(ValueError, match="cell must be positive"):
        seed.thin(cloud, 0.0)
    with pytest.raises(ValueError, match="num_pts"):
        seed.thin_to(cloud, 0)
    bad = _cloud(10, False)
    bad.xyz[3, 1] = float("nan")
    with pytest.raises(ValueError, match="not finite"):
        seed.thin(bad, 0.5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        seed.thin(cloud, 0.5)                                                    # a fine grid, a CPU cloud
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        seed.PointCloud(torch.zeros(4, 2), torch.zeros(4, 2))
