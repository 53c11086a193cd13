"""Scene loading and ray tables (reference ``src/data.py``).

Same public names as the reference (``Intrinsics``, ``NerfData``, ``PoseDataset``, ``RaysDataset``,
``parse_nerf_synthetic``); the difference is where the rays live: the reference keeps them on the CPU and
feeds them through ``DataLoader(num_workers=8)`` one ray per ``__getitem__`` (run.py:116-122), which cannot
feed >= 1e8 samples/s; here ``generate_rays`` runs on the device and ``RaysDataset`` is three flat HBM tables
that the harness indexes with device-side random indices.

Photographed scenes (``parse_nerfstudio``, which the reference stubs) have a camera per image and lens distortion; their
datasets (``CameraRaysDataset``, ``CameraPoseDataset``) hold a camera table and the 8-bit colours instead of ray tables, and the
rays are made on the device when they are drawn (``rays.CameraRays``).
"""
from __future__ import annotations

import json
from dataclasses import dataclass
from pathlib import Path
from typing import List, Optional, Tuple, Union

import numpy as np
import torch

from .rays import CameraRays, Intrinsics, generate_rays as _generate_rays


@dataclass
class NerfData:
    """Images + camera poses (data.py:21-76)."""
    cameras: torch.Tensor                      # [n_images, 4, 4]
    intrinsics: Union[Intrinsics, List[Intrinsics]]      # one for the split, or one per image (data.py:21-31 allows both)
    imgs: Optional[List[torch.Tensor]] = None  # [n_images][h, w, 3] float in [0,1], or uint8 (photographed scenes: parse_nerfstudio)
    bg_color: Optional[torch.Tensor] = None
    # photographed scenes; None = one pinhole camera without distortion, as the synthetic loader makes it
    lens: Optional[torch.Tensor] = None        # [n_images, 6] k1 k2 k3 k4 p1 p2
    models: Optional[List[int]] = None         # [n_images] 0 pinhole, 1 OpenCV, 2 OpenCV fisheye (_lib.LENS_*)
    names: Optional[List[str]] = None          # [n_images] the frames' file_path

    @property
    def n_img(self) -> int:
        return len(self.cameras)

    def img_intrinsics(self, idx: int) -> Intrinsics:
        return self.intrinsics[idx] if isinstance(self.intrinsics, (list, tuple)) else self.intrinsics

    def generate_rays(self, device: torch.device | str = "cpu") -> Tuple[torch.Tensor, torch.Tensor]:
        """rays_o, rays_d of shape [n_images, h, w, 3] (data.py:48-73), built on `device`."""
        if isinstance(self.intrinsics, (list, tuple)) or (self.models is not None and any(self.models)):
            raise ValueError("NerfData.generate_rays makes the ray tables of ONE pinhole camera; per-image cameras and lens models "
                             "go through CameraRaysDataset / CameraPoseDataset")
        return _generate_rays(self.cameras.to(device), self.intrinsics)

    def camera_rays(self, device: torch.device | str = "cuda") -> CameraRays:
        """the split as a camera table + 8-bit colours (rays.CameraRays).  Float images are taken back to the bytes they were decoded
        from (round(255 v): exact for v = byte / 255)."""
        n = self.n_img
        K = [self.img_intrinsics(i) for i in range(n)]
        lens = torch.zeros((n, 10), dtype=torch.float32)
        lens[:, :4] = torch.tensor([[k.fx, k.fy, k.cx, k.cy] for k in K], dtype=torch.float64).float()
        if self.lens is not None:
            lens[:, 4:] = self.lens.float()
        rgb = None
        if self.imgs is not None:
            rgb = [im if im.dtype == torch.uint8 else torch.round(im * 255.).clamp(0, 255).to(torch.uint8) for im in self.imgs]
        return CameraRays(self.cameras[:, :3, :], lens, self.models if self.models is not None else [0] * n, [[k.w, k.h] for k in K], rgb, device)

    def scene_scale(self) -> float:
        return torch.max(torch.var(self.cameras[:, :3, 3], 0)).item()      # data.py:75-76


class PoseDataset:
    """Per-image rays for inference (data.py:78-100)."""

    def __init__(self, data: NerfData, device: torch.device | str = "cpu"):
        self.rays_o, self.rays_d = data.generate_rays(device)
        self.cameras = data.cameras                # [n, 4, 4] on the host: a pose-only camera table can be made of the split (tsdf.camera_table)
        self.rgbs = None if data.imgs is None else [_as_float(im).to(device) for im in data.imgs]
        self.scene_scale = data.scene_scale()
        self.bg_color = data.bg_color
        self.intrinsics = data.intrinsics

    def img_intrinsics(self, idx: int) -> Intrinsics:
        return self.intrinsics

    def __len__(self) -> int:
        return self.rays_o.size(0)

    def __getitem__(self, idx: int):
        out = {"rays_o": self.rays_o[idx], "rays_d": self.rays_d[idx]}
        if self.rgbs is not None:
            out["rgbs"] = self.rgbs[idx]
        return out


class RaysDataset:
    """All training rays as flat device tables [M,3] (data.py:102-120 without the per-ray __getitem__ path)."""

    def __init__(self, data: NerfData, device: torch.device | str = "cpu"):
        assert data.imgs is not None, "rays datasets requires rgbs"
        o, d = data.generate_rays(device)
        self.rays_o = o.reshape(-1, 3).contiguous()
        self.rays_d = d.reshape(-1, 3).contiguous()
        self.rgbs = torch.cat([_as_float(im).reshape(-1, 3) for im in data.imgs]).to(device).contiguous()
        self.scene_scale = data.scene_scale()
        self.bg_color = data.bg_color

    def __len__(self) -> int:
        return self.rays_o.size(0)

    def __getitem__(self, idx):
        return {"rays_o": self.rays_o[idx], "rays_d": self.rays_d[idx], "rgbs": self.rgbs[idx]}


def _as_float(im: torch.Tensor) -> torch.Tensor:
    """uint8 images as the loaders' float32 byte / 255 (the same bits as _composite_over's)"""
    if im.dtype != torch.uint8:
        return im
    return torch.from_numpy(im.numpy().astype(np.float32) / np.float32(255.))


class _ImageColours:
    """``CameraPoseDataset.rgbs``: image i's colours as float [h, w, 3], made from the bytes when asked for"""

    def __init__(self, source: CameraRays):
        self.source = source

    def __len__(self) -> int:
        return self.source.n_img

    def __getitem__(self, idx: int) -> torch.Tensor:
        return self.source.image_rgb(idx)


class CameraPoseDataset:
    """PoseDataset on a camera table (rays.CameraRays): per-image cameras, lens models and sizes; image i's rays are made when
    ``dataset[i]`` is read -- nothing per pixel is stored except the 8-bit colours."""

    def __init__(self, data: NerfData, device: torch.device | str = "cuda"):
        self.source = data.camera_rays(device)
        self.device = self.source.device
        self.rgbs = None if data.imgs is None else _ImageColours(self.source)
        self.scene_scale = data.scene_scale()
        self.bg_color = data.bg_color
        self.intrinsics = [data.img_intrinsics(i) for i in range(data.n_img)]

    def img_intrinsics(self, idx: int) -> Intrinsics:
        return self.intrinsics[idx]

    def __len__(self) -> int:
        return self.source.n_img

    def __getitem__(self, idx: int):
        o, d, rgb = self.source.image(idx)
        out = {"rays_o": o, "rays_d": d}
        if rgb is not None:
            out["rgbs"] = rgb
        return out


class CameraRaysDataset:
    """RaysDataset on a camera table: all training rays of the split as flat pixel indices; ``run.train`` hands ``source`` to the
    trainer, which draws its batches with ``tn_camera_rays``."""

    def __init__(self, data: NerfData, device: torch.device | str = "cuda"):
        assert data.imgs is not None, "rays datasets requires rgbs"
        self.source = data.camera_rays(device)
        self.device = self.source.device
        self.scene_scale = data.scene_scale()
        self.bg_color = data.bg_color

    def __len__(self) -> int:
        return self.source.n_rays

    def __getitem__(self, idx):
        idx = torch.as_tensor(idx, device=self.device).reshape(-1).to(torch.int32)
        o, d, rgb = (torch.empty((idx.numel(), 3), dtype=torch.float32, device=self.device) for _ in range(3))
        self.source.gather(idx, o, d, rgb)
        return {"rays_o": o, "rays_d": d, "rgbs": rgb}


def _composite_over(img, bg_color):
    """PIL image -> float32 [h,w,3] in [0,1]; RGBA is composited over `bg_color` first."""
    from PIL import Image
    if img.mode == "RGBA":
        img = Image.alpha_composite(Image.new("RGBA", img.size, bg_color), img).convert("RGB")
    return torch.from_numpy(np.asarray(img, dtype=np.float32) / np.float32(255.))


def parse_nerf_synthetic(scene_path: Path, split: str = "train", bg_color: Tuple[int, int, int] = (255, 255, 255)) -> NerfData:
    """Blender-synthetic scenes (https://www.matthewtancik.com/nerf), data.py:123-158: frames listed in
    ``transforms_<split>.json``, RGBA composited over `bg_color`, one pinhole camera for the whole split with
    focal = w / (2 tan(camera_angle_x / 2)) and the principal point at the image centre."""
    from PIL import Image
    root = Path(scene_path)
    meta = json.loads((root / f"transforms_{split}.json").read_text())
    frames = meta["frames"]
    if not frames:
        raise ValueError(f"{root}: no frames in split {split!r}")
    images = []
    size = None
    for frame in frames:
        with Image.open((root / frame["file_path"]).with_suffix(".png")) as img:
            size = size or img.size
            images.append(_composite_over(img, bg_color))
    width, height = size
    focal = width / (2. * np.tan(0.5 * meta["camera_angle_x"]))
    poses = torch.tensor([frame["transform_matrix"] for frame in frames], dtype=torch.float)
    return NerfData(cameras=poses, intrinsics=Intrinsics(focal, focal, width / 2., height / 2., width, height), imgs=images,
                    bg_color=torch.tensor(bg_color, dtype=torch.float) / 255.)


_LENS_KEYS = ("k1", "k2", "k3", "k4", "p1", "p2")
# nerfstudio's names; SIMPLE_RADIAL (k1 only) is the OpenCV model with the other coefficients 0
_CAMERA_MODELS = {"PINHOLE": 0, "OPENCV": 1, "SIMPLE_RADIAL": 1, "OPENCV_FISHEYE": 2}


def _composite_bytes(img, bg_color):
    """PIL image -> PIL RGB image; RGBA is composited over `bg_color` as _composite_over does"""
    from PIL import Image
    if img.mode == "RGBA":
        return Image.alpha_composite(Image.new("RGBA", img.size, bg_color), img).convert("RGB")
    return img if img.mode == "RGB" else img.convert("RGB")


def orient_poses(c2w: np.ndarray) -> np.ndarray:
    """[n, 4, 4] float64 camera-to-world -> the same cameras after ONE similarity: translated by the mean camera position, rotated so
    that the mean camera up axis (+y column) becomes world +z, scaled by 1 / (largest absolute coordinate of any camera position)."""
    c2w = np.array(c2w, dtype=np.float64)
    t = c2w[:, :3, 3] - c2w[:, :3, 3].mean(0)
    up = c2w[:, :3, 1].mean(0)
    norm = np.linalg.norm(up)
    rot = np.eye(3)
    if norm > 1e-12:
        a = up / norm
        c = a[2]                                            # a . z
        if c < -1.0 + 1e-12:
            rot = np.diag([1.0, -1.0, -1.0])                # straight down: half a turn about x
        else:
            v = np.array([a[1], -a[0], 0.0])                # a x z
            vx = np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])
            rot = np.eye(3) + vx + vx @ vx / (1.0 + c)      # Rodrigues: the rotation about a x z that takes a to z
    t = t @ rot.T
    largest = np.abs(t).max()
    out = c2w.copy()
    out[:, :3, :3] = rot @ c2w[:, :3, :3]
    out[:, :3, 3] = t / largest if largest > 0 else t
    return out


def _find_image(root: Path, file_path: str) -> Path:
    path = root / file_path
    if path.exists():
        return path
    for suffix in (".png", ".jpg", ".jpeg", ".PNG", ".JPG", ".JPEG"):
        if path.with_name(path.name + suffix).exists():
            return path.with_name(path.name + suffix)
    raise FileNotFoundError(path)


def parse_nerfstudio(scene_path: Path, split: str = "train", bg_color: Tuple[int, int, int] = (255, 255, 255), downscale: int = 1,
                     holdout_every: int = 8, orient: bool = True) -> NerfData:
    """A nerfstudio-format capture (the reference only stubs this loader, data.py:162-167): ``transforms.json`` in `scene_path` (or
    `scene_path` itself, if it is the file) with ``fl_x fl_y cx cy w h k1 k2 k3 k4 p1 p2 camera_model`` at top level, each of which a
    frame may override.  Missing coefficients are 0, a missing principal point is the image centre, a missing ``fl_y`` is ``fl_x``;
    a missing ``camera_model`` is OPENCV if any coefficient is non-zero and PINHOLE otherwise; PINHOLE, OPENCV and OPENCV_FISHEYE
    (and SIMPLE_RADIAL, the OpenCV model with k1 alone) are known, any other name raises NotImplementedError.  The lens models are those of ``tn_camera_rays``.

    * images: ``file_path`` relative to the json, PNG or JPEG, kept as uint8; RGBA is composited over `bg_color` as the synthetic
      loader does.  ``downscale = N > 1``: the file of the same name under ``images_N/`` if that folder exists, otherwise the image
      is box-filtered by ``PIL.Image.reduce(N)``; ``fl_x fl_y cx cy`` are divided by N, ``w h`` are those of the loaded image.
    * splits: ``train_filenames`` / ``val_filenames`` / ``test_filenames`` if the json has any of them; otherwise the frames are
      sorted by ``file_path`` and every `holdout_every`-th (index % N == 0) is ``val`` and ``test``, the rest ``train`` (the LLFF /
      Mip-NeRF 360 rule).
    * poses: ``orient`` applies ``orient_poses`` -- computed once over ALL frames of the json in float64, not per split, so that the
      splits share one world; ``orient=False`` leaves ``transform_matrix`` alone.
    * ignored: ``applied_transform``, ``mask_path``, ``depth_file_path`` and every other key."""
    from PIL import Image
    root = Path(scene_path)
    meta_path = root if root.is_file() else root / "transforms.json"
    root = meta_path.parent
    meta = json.loads(meta_path.read_text())
    frames = list(meta.get("frames", []))
    if not frames:
        raise ValueError(f"{meta_path}: no frames")
    downscale = int(downscale)
    if downscale < 1:
        raise ValueError(f"downscale = {downscale} must be >= 1")
    if split not in ("train", "val", "test"):
        raise ValueError(f"unknown split {split!r}")

    def value(frame, key, default=None):
        return frame.get(key, meta.get(key, default))

    # camera models first: an unknown one fails before any image is decoded
    models = []
    for frame in frames:
        name = value(frame, "camera_model")
        if name is None:
            name = "OPENCV" if any(float(value(frame, k, 0.0)) != 0.0 for k in _LENS_KEYS) else "PINHOLE"
        if name not in _CAMERA_MODELS:
            raise NotImplementedError(f"{meta_path}: camera_model {name!r} is not supported (known: {', '.join(sorted(_CAMERA_MODELS))})")
        models.append(_CAMERA_MODELS[name])
    poses = np.array([frame["transform_matrix"] for frame in frames], dtype=np.float64)
    if poses.shape[1:] != (4, 4):
        raise ValueError(f"{meta_path}: transform_matrix must be 4 x 4")
    if orient:
        poses = orient_poses(poses)

    listed = [k for k in ("train_filenames", "val_filenames", "test_filenames") if k in meta]
    if listed:
        wanted = set(meta.get(f"{split}_filenames", []))
        chosen = [i for i, frame in enumerate(frames) if frame["file_path"] in wanted]
    else:
        if holdout_every < 1:
            raise ValueError(f"holdout_every = {holdout_every} must be >= 1")
        order = sorted(range(len(frames)), key=lambda i: frames[i]["file_path"])
        held = [i for pos, i in enumerate(order) if pos % holdout_every == 0]
        chosen = held if split != "train" else [i for pos, i in enumerate(order) if pos % holdout_every != 0]
    if not chosen:
        raise ValueError(f"{meta_path}: no frames in split {split!r}")

    images, intrinsics, lens = [], [], []
    small = root / f"images_{downscale}"
    for i in chosen:
        frame = frames[i]
        path = _find_image(root, frame["file_path"])
        reduce_by = 1
        if downscale > 1:
            if small.is_dir():
                path = _find_image(small, path.name)
            else:
                reduce_by = downscale
        with Image.open(path) as img:
            if downscale == 1 and (int(value(frame, "w", img.size[0])), int(value(frame, "h", img.size[1]))) != img.size:
                raise ValueError(f"{path}: the image is {img.size[0]} x {img.size[1]}, the json says {value(frame, 'w')} x {value(frame, 'h')}")
            rgb = _composite_bytes(img, bg_color)
            if reduce_by > 1:
                rgb = rgb.reduce(reduce_by)
            images.append(torch.from_numpy(np.array(rgb, dtype=np.uint8)))
        height, width = images[-1].shape[:2]
        full_w, full_h = value(frame, "w"), value(frame, "h")
        fx = value(frame, "fl_x")
        if fx is None:
            raise ValueError(f"{meta_path}: no fl_x for frame {frame['file_path']!r}")
        fy = value(frame, "fl_y", fx)
        cx = value(frame, "cx", None if full_w is None else 0.5 * float(full_w))
        cy = value(frame, "cy", None if full_h is None else 0.5 * float(full_h))
        cx = 0.5 * width if cx is None else float(cx) / downscale
        cy = 0.5 * height if cy is None else float(cy) / downscale
        intrinsics.append(Intrinsics(float(fx) / downscale, float(fy) / downscale, cx, cy, width, height))
        lens.append([float(value(frame, k, 0.0)) for k in _LENS_KEYS])
    return NerfData(cameras=torch.from_numpy(poses[chosen]).float(), intrinsics=intrinsics, imgs=images,
                    bg_color=torch.tensor(bg_color, dtype=torch.float) / 255., lens=torch.tensor(lens, dtype=torch.float32),
                    models=[models[i] for i in chosen], names=[frames[i]["file_path"] for i in chosen])
