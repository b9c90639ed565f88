"""A dataset folder as cameras, 8-bit frames and an initial model: what the reference's ``Scene(...)`` does before iteration 0.

Host code for Blender / D-NeRF / converted-DyNeRF folders (``transforms_train.json`` + ``transforms_test.json``, images, an optional
``points3d.ply``), after ``readNerfSyntheticInfo`` / ``readCamerasFromTransforms`` (scene/dataset_readers.py:212-391),
``loadCam`` (utils/camera_utils.py:19-69), ``Camera`` (scene/cameras.py:19-73) and utils/graphics_utils.py:

* ``read_transforms``  -- one ``CameraInfo`` per kept frame: the OpenGL -> COLMAP axis flip, the inverse, ``R`` stored transposed, ``T``;
  ``camera_angle_x`` or per-frame / global ``fl_x fl_y cx cy``; ``time`` / ``frame_ratio`` / the ``time_duration`` filter.
* ``nerfpp_norm``      -- ``getNerfppNorm``: the cameras' centre and 1.1 x the largest distance from it (``cameras_extent``).
* ``Camera``           -- the matrices as the reference builds them, and the attributes ``render_raw`` reads.
* ``Scene``            -- the folder read, the images as a ``FrameStore`` at the training resolution (composited over the background
  and resized on the GPU, ``fdgs.resize``), the point cloud (``points3d.ply``, or the reference's random cloud), ``create_model``.

COLMAP ``sparse/0`` folders are not read here."""
import json
import math
import os
from pathlib import Path
from typing import List, NamedTuple, Optional, Sequence

import numpy as np
import torch

ZNEAR, ZFAR = 0.01, 100.0   # scene/cameras.py:59-60


class CameraInfo(NamedTuple):
    uid: int
    R: np.ndarray            # [3, 3] float64, the world-to-camera rotation TRANSPOSED (the reference's convention)
    T: np.ndarray            # [3] float64
    FovY: float              # -1 with stored intrinsics
    FovX: float
    image_path: str
    image_name: str
    width: int
    height: int
    timestamp: float = 0.0
    fl_x: float = -1.0
    fl_y: float = -1.0
    cx: float = -1.0
    cy: float = -1.0


def fov2focal(fov, pixels):
    return pixels / (2 * math.tan(fov / 2))


def focal2fov(focal, pixels):
    return 2 * math.atan(pixels / (2 * focal))


def world_to_view(R, t, translate=np.array([0.0, 0.0, 0.0]), scale=1.0):
    """``getWorld2View2``: float64 throughout, cast to float32 at the end."""
    Rt = np.zeros((4, 4))
    Rt[:3, :3] = R.transpose()
    Rt[:3, 3] = t
    Rt[3, 3] = 1.0
    C2W = np.linalg.inv(Rt)
    C2W[:3, 3] = (C2W[:3, 3] + translate) * scale
    return np.float32(np.linalg.inv(C2W))


def _frustum(top, bottom, left, right, znear, zfar):
    P = torch.zeros(4, 4)
    P[0, 0] = 2.0 * znear / (right - left)
    P[1, 1] = 2.0 * znear / (top - bottom)
    P[0, 2] = (right + left) / (right - left)
    P[1, 2] = (top + bottom) / (top - bottom)
    P[3, 2] = 1.0
    P[2, 2] = zfar / (zfar - znear)
    P[2, 3] = -(zfar * znear) / (zfar - znear)
    return P


def projection_matrix(znear, zfar, fovX, fovY):
    """``getProjectionMatrix``: Python floats stored into a float32 tensor."""
    top, right = math.tan(fovY / 2) * znear, math.tan(fovX / 2) * znear
    return _frustum(top, -top, -right, right, znear, zfar)


def projection_matrix_center_shift(znear, zfar, cx, cy, fl_x, fl_y, w, h):
    """``getProjectionMatrixCenterShift``: the principal point where the file puts it."""
    return _frustum(cy / fl_y * znear, -(h - cy) / fl_y * znear, -(w - cx) / fl_x * znear, cx / fl_x * znear, znear, zfar)


def _image_size(path):
    from PIL import Image
    with Image.open(path) as im:
        return int(im.size[0]), int(im.size[1])


def read_transforms(path: str, transformsfile: str, extension: str = ".png", time_duration: Optional[Sequence[float]] = None,
                    frame_ratio: float = 1) -> List[CameraInfo]:
    """``readCamerasFromTransforms`` without the pixels: the frames of ``transformsfile`` whose time, divided by ``frame_ratio`` when
    that is above 1, lies within ``time_duration`` (frames without a ``time`` are always kept, at timestamp 0)."""
    with open(os.path.join(path, transformsfile)) as f:
        contents = json.load(f)
    fovx = contents.get("camera_angle_x")
    keys = ("fl_x", "fl_y", "cx", "cy")
    infos = []
    for idx, frame in enumerate(contents["frames"]):
        timestamp = frame.get("time", 0.0)
        if frame_ratio > 1:
            timestamp /= frame_ratio
        if time_duration is not None and "time" in frame and (timestamp < time_duration[0] or timestamp > time_duration[1]):
            continue
        cam_name = os.path.join(path, frame["file_path"] + extension)
        c2w = np.array(frame["transform_matrix"], dtype=np.float64)
        c2w[:3, 1:3] *= -1                       # OpenGL / Blender axes (Y up, Z back) -> COLMAP (Y down, Z forward)
        w2c = np.linalg.inv(c2w)
        R, T = np.transpose(w2c[:3, :3]), w2c[:3, 3]
        width, height = _image_size(cam_name)
        common = dict(uid=idx, R=R, T=T, image_path=cam_name, image_name=Path(cam_name).stem, width=width, height=height, timestamp=timestamp)
        src = frame if all(k in frame for k in keys) else contents if all(k in contents for k in keys) else None
        if src is not None:
            infos.append(CameraInfo(FovY=-1.0, FovX=-1.0, fl_x=src["fl_x"], fl_y=src["fl_y"], cx=src["cx"], cy=src["cy"], **common))
        else:
            if fovx is None:
                raise ValueError("fdgs.scene: %s has neither camera_angle_x nor fl_x / fl_y / cx / cy" % transformsfile)
            infos.append(CameraInfo(FovY=focal2fov(fov2focal(fovx, width), height), FovX=fovx, **common))
    return infos


def nerfpp_norm(cam_infos: Sequence[CameraInfo]) -> dict:
    """``getNerfppNorm``: {"translate": minus the mean camera centre, "radius": 1.1 x the largest distance of a centre from it}."""
    centers = []
    for cam in cam_infos:
        centers.append(np.linalg.inv(world_to_view(cam.R, cam.T))[:3, 3:4])    # the float32 matrix, inverted in float32
    centers = np.hstack(centers)
    center = np.mean(centers, axis=1, keepdims=True)
    diagonal = np.max(np.linalg.norm(centers - center, axis=0, keepdims=True))
    return {"translate": -center.flatten(), "radius": diagonal * 1.1}


class Camera:
    """``scene.cameras.Camera`` without the image: the reference's matrices (row-vector convention: ``world_view_transform`` and
    ``full_proj_transform`` are the transposes of the column-vector matrices) and the attribute set ``render_raw`` reads, as
    ``train_host.SyntheticCamera`` has it.  With stored intrinsics (``cx`` > 0) the projection is the centre-shift one; ``FoVx`` /
    ``FoVy``, which the reference leaves at -1 then, are the field of view of ``fl_x`` / ``fl_y``."""

    def __init__(self, info: CameraInfo, resolution, scale: float = 1.0, device="cpu", uid: Optional[int] = None):
        self.uid, self.colmap_id = info.uid if uid is None else uid, info.uid
        self.R, self.T = info.R, info.T
        self.image_name, self.image_path, self.timestamp = info.image_name, info.image_path, info.timestamp
        self.image_width, self.image_height = int(resolution[0]), int(resolution[1])
        self.cx, self.cy, self.fl_x, self.fl_y = info.cx / scale, info.cy / scale, info.fl_x / scale, info.fl_y / scale   # loadCam
        self.znear, self.zfar = ZNEAR, ZFAR
        self.world_view_transform = torch.tensor(world_to_view(info.R, info.T)).transpose(0, 1)
        if self.cx > 0:
            proj = projection_matrix_center_shift(self.znear, self.zfar, self.cx, self.cy, self.fl_x, self.fl_y, self.image_width, self.image_height)
            self.FoVx, self.FoVy = focal2fov(self.fl_x, self.image_width), focal2fov(self.fl_y, self.image_height)
        else:
            proj = projection_matrix(self.znear, self.zfar, info.FovX, info.FovY)
            self.FoVx, self.FoVy = info.FovX, info.FovY
            self.fl_x, self.fl_y = fov2focal(self.FoVx, self.image_width), fov2focal(self.FoVy, self.image_height)   # for get_rays
            self.cx, self.cy = 0.5 * self.image_width, 0.5 * self.image_height
        self.projection_matrix = proj.transpose(0, 1)
        self.full_proj_transform = self.world_view_transform.unsqueeze(0).bmm(self.projection_matrix.unsqueeze(0)).squeeze(0)
        self.camera_center = self.world_view_transform.inverse()[3, :3]
        self.to(device)

    def to(self, device) -> "Camera":
        for k in ("world_view_transform", "projection_matrix", "full_proj_transform", "camera_center"):
            setattr(self, k, getattr(self, k).to(device).contiguous())
        return self

    def get_rays(self):
        from .train_host import SyntheticCamera
        return SyntheticCamera.get_rays(self)


def load_rgba(infos: Sequence[CameraInfo]) -> np.ndarray:
    """The images of ``infos`` as uint8 [N, H, W, 4] (PIL, converted to RGBA as the reference's reader does).  ``ValueError``: images
    of different sizes -- one store holds one size."""
    from PIL import Image
    frames = []
    for info in infos:
        with Image.open(info.image_path) as im:
            a = np.array(im.convert("RGBA"))
        if frames and a.shape != frames[0].shape:
            raise ValueError("fdgs.scene: mixed image sizes: %s is %dx%d, %s is %dx%d" % (
                info.image_path, a.shape[1], a.shape[0], infos[0].image_path, frames[0].shape[1], frames[0].shape[0]))
        frames.append(a)
    return np.stack(frames) if frames else np.zeros((0, 1, 1, 4), np.uint8)


class Scene:
    """A dataset folder read as the reference's ``Scene`` reads a Blender-style one.

    ``train_infos`` / ``test_infos``: the kept frames (``eval=False`` appends the test frames to the training ones, as the reference
    does); ``cameras_extent``; ``white_background``; ``cloud``: ``points3d.ply`` as a host ``PointCloud``, None without the file
    (``create_model`` then draws the reference's random cloud).  Nothing here touches the GPU until ``frames`` or ``create_model``."""

    def __init__(self, path: str, *, white_background: bool = False, eval: bool = False, extension: str = ".png",
                 time_duration: Optional[Sequence[float]] = None, frame_ratio: float = 1, resolution=1, num_pts: int = 100_000,
                 num_extra_pts: int = 0, seed: int = 0):
        if not os.path.exists(os.path.join(path, "transforms_train.json")):
            raise ValueError("fdgs.scene: %s has no transforms_train.json (COLMAP folders are not read here)" % path)
        if int(num_pts) < 1:
            raise ValueError("fdgs.scene: num_pts must be at least 1, got %r" % (num_pts,))
        self.path, self.white_background, self.time_duration = path, bool(white_background), time_duration
        self.resolution, self.num_pts, self.num_extra_pts, self.seed = resolution, int(num_pts), int(num_extra_pts), int(seed)
        kw = dict(extension=extension, time_duration=time_duration, frame_ratio=frame_ratio)
        self.train_infos = read_transforms(path, "transforms_train.json", **kw)
        test_file = "transforms_val.json" if path.endswith("lego") else "transforms_test.json"
        self.test_infos = read_transforms(path, test_file, **kw) if os.path.exists(os.path.join(path, test_file)) else []
        if not eval:
            self.train_infos, self.test_infos = self.train_infos + self.test_infos, []
        if not self.train_infos:
            raise ValueError("fdgs.scene: no training frame of %s lies within time_duration %r" % (path, time_duration))
        sizes = {(c.width, c.height) for c in self.train_infos + self.test_infos}
        if len(sizes) != 1:
            raise ValueError("fdgs.scene: mixed image sizes %s: one FrameStore holds one size" % sorted(sizes))
        self.nerf_normalization = nerfpp_norm(self.train_infos)
        self.cameras_extent = float(self.nerf_normalization["radius"])
        self.ply_path = os.path.join(path, "points3d.ply")
        from .seed import load_ply
        self.cloud = load_ply(self.ply_path) if os.path.exists(self.ply_path) else None

    def _resolution(self, info):
        from .resize import target_resolution
        size, scale, _ = target_resolution(info.width, info.height, self.resolution)
        return size, scale

    def cameras(self, split: str = "train", device="cpu") -> List[Camera]:
        """``cameraList_from_camInfos``: the cameras of "train" or "test" at the training resolution, uid = position in the list."""
        infos = self.train_infos if split == "train" else self.test_infos
        return [Camera(c, *self._resolution(c), device=device, uid=k) for k, c in enumerate(infos)]

    def frames(self, split: str = "train", residency: str = "device", device=None, chunk: int = 8):
        """The images of a split as a ``FrameStore`` [N, H, W, 3]: read with PIL as 8-bit RGBA, composited over the background
        (``fdgs.resize.composite``: the readers' float64 formula) and resized to ``target_resolution`` on the GPU
        (``fdgs.resize.resized_store``), indexed like ``cameras(split)``."""
        from .resize import resized_store
        infos = self.train_infos if split == "train" else self.test_infos
        if not infos:
            raise ValueError("fdgs.scene: the %s split is empty" % split)
        size, _ = self._resolution(infos[0])
        return resized_store(load_rgba(infos), size, residency=residency, chunk=chunk, background="white" if self.white_background else "black",
                             device=device)

    def point_cloud(self, device="cuda"):
        """The cloud a model starts from, on ``device``: ``points3d.ply`` thinned to at most ``num_pts`` points (``fdgs.seed.thin_to``
        in place of the reference's draw with replacement), cut to the open ``time_duration`` interval if it has times, as the
        reference cuts its thinned cloud; without the file, the reference's random cloud in the 2.6-box.  Then ``num_extra_pts``
        grey points on the sphere of radius 60, at the middle of the time span."""
        from . import seed
        if self.cloud is None:
            cloud = seed.random_cloud(self.num_pts, self.seed, device=device)
        else:
            cloud = self.cloud.to(device)
            if len(cloud) > self.num_pts:
                cloud = seed.thin_to(cloud, self.num_pts).cloud
                if cloud.t is not None and self.time_duration is not None:
                    cloud = cloud.select((cloud.t < self.time_duration[1]) & (cloud.t > self.time_duration[0]))
        if self.num_extra_pts > 0:
            mid = None if cloud.t is None else 0.5 * (self.time_duration[0] + self.time_duration[1])
            cloud = seed.PointCloud.cat([cloud, seed.sphere_shell(self.num_extra_pts, 60.0, self.seed, device, time=mid)])
        return cloud

    def create_model(self, *, sh_degree: int = 3, sh_degree_t: int = 0, gaussian_dim: int = 3, rot_4d: bool = False,
                     force_sh_3d: bool = False, device="cuda", M: Optional[int] = None):
        """``thin_to`` -> ``distCUDA2`` -> ``create_from_pcd``: the ``GaussianParams`` a run starts from, with ``spatial_lr_scale`` =
        ``cameras_extent`` (what the reference's ``create_from_pcd`` is handed) as an attribute."""
        from . import seed
        from .knn import distCUDA2
        cloud = self.point_cloud(device)
        td = self.time_duration if self.time_duration is not None else (0.0, 1.0)
        model = seed.create_from_pcd(cloud, sh_degree=sh_degree, sh_degree_t=sh_degree_t, gaussian_dim=gaussian_dim, rot_4d=rot_4d,
                                     force_sh_3d=force_sh_3d, time_duration=td, seed=self.seed, dist2=distCUDA2(cloud.xyz), M=M)
        model.spatial_lr_scale = self.cameras_extent
        return model
