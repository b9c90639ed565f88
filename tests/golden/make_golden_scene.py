"""Records tests/golden/scene/*.json|npz: what the REFERENCE's readers and camera code make of three small dataset folders.

Run once, where the reference tree is available:  python tests/golden/make_golden_scene.py /path/to/reference
The reference's ``readCamerasFromTransforms`` / ``getNerfppNorm`` (scene/dataset_readers.py) and ``getWorld2View2`` /
``getProjectionMatrix`` / ``getProjectionMatrixCenterShift`` (utils/graphics_utils.py) are imported at recording time only; the
matrices are put together as scene/cameras.py:65-71 does.  Committed: the folders' settings (``<case>.json``: the two transforms files
and the image size -- the test writes the folder again from them, with blank images) and the recorded arrays (``<case>.npz``).
"""
import importlib.util
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "scene")
READS = {   # name -> keywords of one read of the folder
    "all": dict(time_duration=None, frame_ratio=1),
    "window": dict(time_duration=[0.2, 0.8], frame_ratio=1),
    "ratio2": dict(time_duration=[0.0, 0.3], frame_ratio=2),
}


def _pose(rng):
    """A camera-to-world matrix in OpenGL axes: a random rotation, a centre a few units out."""
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] *= -1
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = q, rng.normal(size=3) * 3.0
    return m.tolist()


def datasets():
    rng = np.random.default_rng(7)
    W, H = 40, 30
    out = {}
    for case in ("fov", "frame_intrinsics", "global_intrinsics"):
        files = {}
        for split, n in (("train", 6), ("test", 3)):
            frames = []
            for k in range(n):
                fr = {"file_path": "%s/r_%d" % (split, k), "time": round((k + 0.5) / n, 4), "transform_matrix": _pose(rng)}
                if case == "frame_intrinsics":
                    fr.update(fl_x=35.0 + k, fl_y=36.5 + k, cx=W / 2 + 1.5 - k, cy=H / 2 - 2.25 + 0.5 * k)
                frames.append(fr)
            top = {"frames": frames}
            if case == "fov":
                top["camera_angle_x"] = 0.6911112070083618
            if case == "global_intrinsics":
                top.update(fl_x=41.25, fl_y=40.5, cx=23.0, cy=13.5)
            files["transforms_%s.json" % split] = top
        out[case] = {"width": W, "height": H, "files": files}
    return out


def write_folder(folder, spec):
    from PIL import Image
    for name, top in spec["files"].items():
        with open(os.path.join(folder, name), "w") as f:
            json.dump(top, f)
        for fr in top["frames"]:
            p = os.path.join(folder, fr["file_path"] + ".png")
            os.makedirs(os.path.dirname(p), exist_ok=True)
            Image.new("RGB", (spec["width"], spec["height"]), (10, 20, 30)).save(p)


def _reference(root):
    for name in ("pointops2", "pointops2.functions", "pointops2.functions.pointops", "simple_knn", "simple_knn._C", "plyfile", "imagesize", "scene"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["pointops2.functions.pointops"].furthestsampling = None
    sys.modules["pointops2.functions.pointops"].knnquery = None
    sys.modules["simple_knn._C"].distCUDA2 = None
    sys.modules["plyfile"].PlyData = sys.modules["plyfile"].PlyElement = None
    def _size(path):        # the readers' dataloader mode asks imagesize for (width, height) instead of decoding the image
        from PIL import Image
        with Image.open(path) as im:
            return im.size
    sys.modules["imagesize"].get = _size
    sys.modules["scene"].__path__ = [os.path.join(root, "scene")]     # its submodules, without scene/__init__.py
    sys.path.insert(0, root)
    spec = importlib.util.spec_from_file_location("ref_dataset_readers", os.path.join(root, "scene", "dataset_readers.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    import utils.graphics_utils as gu
    return mod, gu


def record(root):
    readers, gu = _reference(root)
    os.makedirs(OUT, exist_ok=True)
    for case, spec in datasets().items():
        arrays = {}
        with tempfile.TemporaryDirectory() as folder:
            write_folder(folder, spec)
            for read, kw in READS.items():
                train = readers.readCamerasFromTransforms(folder, "transforms_train.json", False, ".png", dataloader=True, **kw)
                test = readers.readCamerasFromTransforms(folder, "transforms_test.json", False, ".png", dataloader=True, **kw)
                for ev in (True, False):
                    cams = train if ev else train + test                       # readNerfSyntheticInfo: if not eval: extend
                    norm = readers.getNerfppNorm(cams)
                    tag = "%s/%s" % (read, "eval" if ev else "merged")
                    arrays[tag + "/radius"] = np.float64(norm["radius"])
                    arrays[tag + "/translate"] = np.asarray(norm["translate"])
                    arrays[tag + "/train_uids"] = np.array([c.uid for c in cams], np.int64)
                    arrays[tag + "/test_uids"] = np.array([c.uid for c in (test if ev else [])], np.int64)
                for split, cams in (("train", train), ("test", test)):
                    tag = "%s/%s" % (read, split)
                    arrays[tag + "/R"] = np.stack([c.R for c in cams])
                    arrays[tag + "/T"] = np.stack([c.T for c in cams])
                    arrays[tag + "/fov"] = np.array([[c.FovX, c.FovY] for c in cams], np.float64)
                    arrays[tag + "/intr"] = np.array([[c.fl_x, c.fl_y, c.cx, c.cy] for c in cams], np.float64)
                    arrays[tag + "/time"] = np.array([c.timestamp for c in cams], np.float64)
                    for res in (1, 2):                                         # loadCam's scale, scene/cameras.py:65-71
                        w, h = round(spec["width"] / res), round(spec["height"] / res)
                        wv, fp, cc = [], [], []
                        for c in cams:
                            view = torch.tensor(gu.getWorld2View2(c.R, c.T)).transpose(0, 1)
                            if c.cx / res > 0:
                                proj = gu.getProjectionMatrixCenterShift(0.01, 100.0, c.cx / res, c.cy / res, c.fl_x / res, c.fl_y / res, w, h)
                            else:
                                proj = gu.getProjectionMatrix(znear=0.01, zfar=100.0, fovX=c.FovX, fovY=c.FovY)
                            proj = proj.transpose(0, 1)
                            wv.append(view.numpy())
                            fp.append(view.unsqueeze(0).bmm(proj.unsqueeze(0)).squeeze(0).numpy())
                            cc.append(view.inverse()[3, :3].numpy())
                        arrays["%s/res%d/world_view_transform" % (tag, res)] = np.stack(wv)
                        arrays["%s/res%d/full_proj_transform" % (tag, res)] = np.stack(fp)
                        arrays["%s/res%d/camera_center" % (tag, res)] = np.stack(cc)
        with open(os.path.join(OUT, case + ".json"), "w") as f:
            json.dump(spec, f, indent=1)
        np.savez_compressed(os.path.join(OUT, case + ".npz"), **arrays)
        print(case, len(arrays), "arrays")


if __name__ == "__main__":
    record(sys.argv[1])
