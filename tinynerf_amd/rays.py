"""Ray tables on the device (reference ``src/data.py:48-73`` ray generation).

The reference builds rays on the CPU and feeds them through a ``DataLoader`` one ray at a time; at
>= 1e9 samples/s that loader is the bottleneck, so rays live in HBM as flat [M,3] tables and batches
are drawn by device-side random indices.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch


@dataclass
class Intrinsics:
    fx: float
    fy: float
    cx: float
    cy: float
    w: int
    h: int


def generate_rays(cameras: torch.Tensor, K: Intrinsics) -> Tuple[torch.Tensor, torch.Tensor]:
    """cameras [n,4,4] (camera-to-world) -> rays_o, rays_d of shape [n, h, w, 3].

    Pixel centres at +0.5, fy negated, z = -1, directions normalised -- data.py:52-70."""
    dev = cameras.device
    center = torch.tensor([K.cx, K.cy], dtype=torch.float, device=dev)
    focal = torch.tensor([K.fx, -K.fy], dtype=torch.float, device=dev)
    xs, ys = torch.meshgrid(torch.arange(K.w, dtype=torch.float, device=dev),
                            torch.arange(K.h, dtype=torch.float, device=dev), indexing="xy")
    grid = (torch.stack([xs, ys], -1) - center + 0.5) / focal
    grid = torch.nn.functional.pad(grid, (0, 1), "constant", -1.)
    R, t = cameras[:, :3, :3], cameras[:, :3, 3]
    d = torch.einsum("hwc,nkc->nhwk", grid, R)
    d = d / torch.norm(d, dim=-1, keepdim=True)
    o = t[:, None, None, :].expand_as(d)
    return o.contiguous(), d.contiguous()


class CameraRays:
    """The rays of one split of a photographed scene WITHOUT ray tables: a camera table on the device -- pose, lens and
    size per image, 96 B each -- plus the 8-bit colours, 3 B per pixel; origins and directions are made by ``tn_camera_rays``
    whenever a batch or an image is drawn.  A flat pixel index runs over the images in order, row-major inside an image.

    ``c2w`` [n, 3 or 4, 4] camera-to-world (x right, y up, looking down -z), ``lens`` [n, 10] = fx fy cx cy k1 k2 k3 k4 p1 p2,
    ``model`` [n] (``_lib.LENS_*``), ``size`` [n, 2] = w h, ``rgb`` a list of uint8 [h, w, 3] images or None (pose-only sets)."""

    MAX_PIXELS = 2 ** 31          # the trainer's shuffled ray stream is int32 (torch.randperm(dtype=int32), tn_camera_rays' idx)

    def __init__(self, c2w, lens, model, size, rgb=None, device: torch.device | str = "cuda"):
        size = torch.as_tensor(size, dtype=torch.int64).reshape(-1, 2)
        n_img = size.size(0)
        if n_img < 1:
            raise ValueError("CameraRays: no images")
        if bool((size < 1).any()):
            raise ValueError("CameraRays: every image needs w >= 1 and h >= 1")
        offsets = torch.zeros(n_img + 1, dtype=torch.int64)
        offsets[1:] = torch.cumsum(size[:, 0] * size[:, 1], 0)
        n_pixels = int(offsets[-1])
        if n_pixels >= CameraRays.MAX_PIXELS:            # (before anything is allocated or uploaded)
            raise ValueError(f"CameraRays: this split has {n_pixels} pixels, the ray stream is int32 and holds fewer than 2^31: "
                             "load the scene at a lower resolution (train.py --downscale)")
        c2w = torch.as_tensor(c2w, dtype=torch.float32)
        lens = torch.as_tensor(lens, dtype=torch.float32)
        model = torch.as_tensor(model, dtype=torch.int32).reshape(-1)
        if c2w.dim() != 3 or c2w.size(0) != n_img or c2w.size(1) not in (3, 4) or c2w.size(2) != 4:
            raise ValueError("CameraRays: c2w must be [n_img, 3 or 4, 4]")
        if tuple(lens.shape) != (n_img, 10) or model.numel() != n_img:
            raise ValueError("CameraRays: lens must be [n_img, 10] and model [n_img]")
        if bool(((model < 0) | (model > 2)).any()):
            raise ValueError("CameraRays: model must be 0 (pinhole), 1 (OpenCV) or 2 (OpenCV fisheye)")
        if rgb is not None:
            if len(rgb) != n_img:
                raise ValueError("CameraRays: one image per camera")
            for im, (w, h) in zip(rgb, size.tolist()):
                if im.dtype != torch.uint8 or tuple(im.shape) != (h, w, 3):
                    raise ValueError("CameraRays: images must be uint8 [h, w, 3] of the size the table states")
        from . import _lib as L
        self.device = torch.device(device)
        self.n_img, self.n_rays = n_img, n_pixels
        self.sizes = [(int(w), int(h)) for w, h in size.tolist()]            # host copies: no read-back when an image is drawn
        self.offsets = [int(v) for v in offsets.tolist()]
        self.c2w = c2w[:, :3, :].contiguous().to(self.device)
        self.lens = lens.contiguous().to(self.device)
        self.model = model.contiguous().to(self.device)
        self.size = size.to(torch.int32).contiguous().to(self.device)
        self.pixel_offset = offsets.to(self.device)
        self.rgb = None if rgb is None else torch.cat([im.reshape(-1, 3) for im in rgb]).contiguous().to(self.device)
        self.table = L.CameraTable(self.c2w.data_ptr(), self.lens.data_ptr(), self.model.data_ptr(), self.size.data_ptr(),
                                   self.pixel_offset.data_ptr(), None if self.rgb is None else self.rgb.data_ptr(), n_pixels, n_img, 0)

    def nbytes(self) -> int:
        """device memory the source holds"""
        return sum(t.numel() * t.element_size() for t in (self.c2w, self.lens, self.model, self.size, self.pixel_offset, self.rgb) if t is not None)

    def gather(self, idx: Optional[torch.Tensor], out_o: torch.Tensor, out_d: torch.Tensor, out_rgb: Optional[torch.Tensor] = None,
               first: int = 0, stride: int = 1, n: Optional[int] = None) -> None:
        """rays of the flat pixels ``first + stride * idx[i]`` (``idx`` int32 on the device; None: ``i`` itself, ``n`` of them) into
        the caller's [n, 3] float32 buffers, in one launch"""
        import ctypes as C
        from . import _lib as L
        if idx is not None:
            if idx.dtype != torch.int32:
                raise RuntimeError("CameraRays.gather: idx must be int32")
            n = idx.numel() if n is None else n
        elif n is None:
            raise ValueError("CameraRays.gather: n is needed when idx is None")
        dev = L.require_cuda(self.c2w, idx, out_o, out_d, out_rgb)
        for t in (out_o, out_d, out_rgb):
            if t is not None and (t.dtype != torch.float32 or t.numel() < 3 * n):
                raise RuntimeError("CameraRays.gather: outputs must be float32 [n, 3]")
        L.call("tn_camera_rays", dev, C.byref(self.table), L.ptr(idx), C.c_int64(first), C.c_int64(stride), C.c_int64(n), L.ptr(out_o),
               L.ptr(out_d), L.ptr(out_rgb))

    def image(self, i: int, colours: bool = True):
        """(rays_o, rays_d, rgb or None) of image ``i``, each [h, w, 3] float32, made on demand"""
        if not 0 <= i < self.n_img:
            raise IndexError(i)
        (w, h), n = self.sizes[i], self.sizes[i][0] * self.sizes[i][1]
        o = torch.empty((h, w, 3), dtype=torch.float32, device=self.device)
        d = torch.empty_like(o)
        rgb = torch.empty_like(o) if colours and self.rgb is not None else None
        self.gather(None, o, d, rgb, first=self.offsets[i], stride=1, n=n)
        return o, d, rgb

    def image_rays(self, i: int) -> Tuple[torch.Tensor, torch.Tensor]:
        o, d, _ = self.image(i, colours=False)
        return o, d

    def image_rgb(self, i: int) -> torch.Tensor:
        if self.rgb is None:
            raise ValueError("CameraRays: this split has no colours")
        return self.image(i)[2]


def look_at_origin_poses(n_views: int, radius: float = 4.0311, seed: int = 0, device: str = "cpu") -> torch.Tensor:
    """Blender-synthetic style cameras: on a sphere of `radius`, upper hemisphere, looking at the origin
    (camera looks down its -z axis, +y up) -- the pose distribution of SURVEY 8(d)."""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(n_views, generator=g)
    v = torch.rand(n_views, generator=g)
    theta = 2 * math.pi * u
    phi = torch.acos(v * 0.95)                        # elevation: keep off the exact pole
    pos = radius * torch.stack([torch.sin(phi) * torch.cos(theta), torch.sin(phi) * torch.sin(theta), torch.cos(phi)], -1)
    fwd = -pos / pos.norm(dim=-1, keepdim=True)       # viewing direction
    up = torch.tensor([0., 0., 1.]).expand_as(fwd)
    right = torch.cross(fwd, up, dim=-1)
    right = right / right.norm(dim=-1, keepdim=True)
    cam_up = torch.cross(right, fwd, dim=-1)
    c2w = torch.eye(4).repeat(n_views, 1, 1)
    c2w[:, :3, 0] = right
    c2w[:, :3, 1] = cam_up
    c2w[:, :3, 2] = -fwd
    c2w[:, :3, 3] = pos
    return c2w.to(device)


def blender_intrinsics(res: int = 800, camera_angle_x: float = 0.6911112070083618) -> Intrinsics:
    """data.py:140-142: focal = w / (2 tan(angle/2)); 800x800 -> 1111.111."""
    focal = res / (2.0 * math.tan(0.5 * camera_angle_x))
    return Intrinsics(focal, focal, res / 2.0, res / 2.0, res, res)


def synthetic_scene(n_views: int = 100, res: int = 800, seed: int = 0, device: str = "cuda",
                    with_colors: bool = True) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor], Intrinsics, torch.Tensor]:
    """Flat ray tables [M,3] for `n_views` synthetic 800x800 cameras plus smooth pseudo-colours.

    Colours are an analytic function of the ray (a shaded ball in front of the white background) so that
    training has a signal without any dataset on disk."""
    K = blender_intrinsics(res)
    cams = look_at_origin_poses(n_views, seed=seed, device=device)
    o, d = generate_rays(cams, K)
    o, d = o.reshape(-1, 3), d.reshape(-1, 3)
    rgbs = None
    if with_colors:
        # ray / sphere(radius .75) intersection -> lambert-ish colour by hit position, else white
        b = (o * d).sum(-1)
        c = (o * o).sum(-1) - 0.75 ** 2
        disc = b * b - c
        hit = disc > 0
        t = -b - torch.sqrt(disc.clamp_min(0))
        p = o + d * t[:, None]
        col = 0.5 + 0.5 * torch.sin(4.0 * p)
        rgbs = torch.where(hit[:, None], col, torch.ones_like(col)).contiguous()
    return o, d, rgbs, K, cams
