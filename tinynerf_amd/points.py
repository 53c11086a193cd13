"""Coloured point cloud of a trained scene: the rendered depth of every ray back-projected along the ray, what is not
a surface or lies outside a box dropped, the rest written with its colour as a PLY.

* ``compact_points`` -- one call of ``tn_points_compact`` over flat rays and the maps of ``Trainer.render_rays(maps=True)``;
* ``export_pointcloud`` -- the views of a pose dataset, rendered (or taken from ``infer(maps=True)``), compacted, concatenated and
  thinned to ``n_points``;
* ``export_oriented_pointcloud`` -- the same cloud with the rays' surface normals, the input of surface reconstruction;
* ``write_ply`` / ``read_ply`` -- binary little-endian PLY, 15 B per vertex, 27 B with normals.

The points are in the frame the rays are in: for a capture that is the frame after ``data.orient_poses``, not the capture's own.
torch is plumbing only; there is no CPU path.  No reference counterpart: the reference renders images and exports no geometry.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L

DEPTH_KEYS = {"expected": "depth", "median": "median_depth"}
PLY_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])      # packed: 15 B
_PLY_HEADER = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
               "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
# the dialect with normals: float nx, ny, nz after x, y, z, 27 B per vertex
PLY_VERTEX_N = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                         ("red", "u1"), ("green", "u1"), ("blue", "u1")])
_PLY_HEADER_N = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                 "property float nx\nproperty float ny\nproperty float nz\n"
                 "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")


def _flat(t: torch.Tensor, cols: Optional[int]) -> torch.Tensor:
    t = t.reshape(-1, cols) if cols else t.reshape(-1)
    return t if t.dtype == torch.float32 and t.is_contiguous() else t.float().contiguous()


def compact_points(rays_o: torch.Tensor, rays_d: torch.Tensor, maps: dict, bg: Optional[torch.Tensor], box=None,
                   min_opacity: float = 0.5, depth: str = "expected", capacity: Optional[int] = None):
    """``(points [M,3] float32, colors [M,3] uint8, src [M] int32)`` on the device: ray i of the flat rays becomes the point
    ``o_i + depth_i d_i`` when ``opacity_i >= min_opacity``, its depth is positive and finite and the point lies inside ``box``
    (6 values, lo xyz then hi xyz, faces inclusive; ``None``: no crop); its colour is the composited colour with ``bg`` taken out
    again, ``(rgb - (1 - opacity) bg) / opacity``, as bytes (``bg`` ``None``: nothing to take out).  ``maps`` is the dict of
    ``Trainer.render_rays(maps=True)`` (any shape with one entry per ray), ``depth`` picks its ``depth`` or ``median_depth``.  The
    points keep ray order and ``src`` holds their ray indices.  ``capacity=None`` allocates a row per ray, reads the count back
    once and returns views of the first M rows; with a number, at most that many rows come back (the first ones)."""
    if depth not in DEPTH_KEYS:
        raise ValueError(f"compact_points: depth must be one of {sorted(DEPTH_KEYS)}, not {depth!r}")
    if not float(min_opacity) > 0.0:
        raise ValueError("compact_points: min_opacity must be > 0 (the colour is divided by the opacity)")
    o, d = _flat(rays_o, 3), _flat(rays_d, 3)
    rgb, opacity, dist = _flat(maps["rgb"], 3), _flat(maps["opacity"], None), _flat(maps[DEPTH_KEYS[depth]], None)
    n = o.size(0)
    if not (d.size(0) == rgb.size(0) == opacity.numel() == dist.numel() == n):
        raise RuntimeError("compact_points: rays and maps must hold one entry per ray")
    dev = L.require_cuda(o, d, rgb, opacity, dist)
    if bg is not None:
        bg = torch.as_tensor(bg, dtype=torch.float32).to(dev).reshape(3).contiguous()
    if box is not None:
        box = torch.as_tensor(box, dtype=torch.float32).to(dev).reshape(6).contiguous()
    cap = n if capacity is None else int(capacity)
    if cap < 0:
        raise ValueError("compact_points: capacity must be >= 0")
    nbytes = C.c_int64(0)
    L.call_plain("tn_points_workspace_bytes", C.c_int64(n), C.byref(nbytes))
    workspace = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    points = torch.empty((cap, 3), dtype=torch.float32, device=dev)
    colors = torch.empty((cap, 3), dtype=torch.uint8, device=dev)
    src = torch.empty(cap, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    L.call("tn_points_compact", dev, L.ptr(o), L.ptr(d), L.ptr(rgb), L.ptr(opacity), L.ptr(dist), L.ptr(bg), L.ptr(box),
           C.c_float(min_opacity), C.c_int64(n), C.c_int64(cap), L.ptr(points), L.ptr(colors), L.ptr(src), L.ptr(count), L.ptr(workspace))
    m = min(int(count.item()), cap)
    return points[:m], colors[:m], src[:m]


def default_crop(cfg):
    """the box inside which the marcher samples uniformly: the AABB scenes' +-1.5 box, +-scene_scale for an unbounded scene (beyond
    it the samples are contracted and depth is coarse)"""
    half = 1.5 if cfg.scene_type == "aabb" else float(cfg.scene_scale)
    return [-half] * 3 + [half] * 3


def _export(trainer, dataset, indices, path, n_points, min_opacity, depth, crop, seed, rendered, oriented: bool):
    """``export_pointcloud`` (oriented False) / ``export_oriented_pointcloud``: one routine, the normals gathered with ``src`` when asked for"""
    who = "export_oriented_pointcloud" if oriented else "export_pointcloud"
    if getattr(trainer, "world", 1) > 1:
        raise ValueError(f"{who} runs on one rank: world_size > 1 is not supported")
    indices = list(range(len(dataset))) if indices is None else list(indices)
    if rendered is not None and len(rendered) != len(indices):
        raise ValueError(f"{who}: `rendered` must hold one dict per index")
    if oriented and rendered is not None and any("normal" not in r for r in rendered):
        raise ValueError(f"{who}: `rendered` must come from infer(maps=True, normals=True): a dict lacks 'normal'")
    box = None if crop is False else default_crop(trainer.cfg) if crop is None else crop
    if box is not None:
        box = torch.as_tensor(box, dtype=torch.float32).reshape(6).to(trainer.device)
    bg = trainer.renderer._bg(trainer.device)
    points, colors, normals = [], [], []
    for k, i in enumerate(indices):
        item = dataset[i]
        o, d = item["rays_o"].reshape(-1, 3).to(trainer.device), item["rays_d"].reshape(-1, 3).to(trainer.device)
        if rendered is not None:
            maps = rendered[k]
        else:
            maps = trainer.render_rays(o, d, maps=True, normals=True) if oriented else trainer.render_rays(o, d, maps=True)
        p, c, src = compact_points(o, d, maps, bg, box, min_opacity, depth)
        points.append(p)
        colors.append(c)
        if oriented:
            normals.append(_flat(maps["normal"], 3)[src.long()])
    if points:
        points, colors = torch.cat(points, 0), torch.cat(colors, 0)
        normals = torch.cat(normals, 0) if oriented else None
    else:
        points = torch.empty((0, 3), dtype=torch.float32, device=trainer.device)
        colors = torch.empty((0, 3), dtype=torch.uint8, device=trainer.device)
        normals = torch.empty((0, 3), dtype=torch.float32, device=trainer.device) if oriented else None
    if points.size(0) > n_points:
        gen = torch.Generator(device="cpu")
        gen.manual_seed(int(seed))
        keep = torch.randperm(points.size(0), generator=gen)[:n_points].sort().values.to(trainer.device)
        points, colors = points[keep], colors[keep]
        normals = normals[keep] if oriented else None
    if path is not None:
        if oriented:
            write_ply(path, points, colors, normals)
        else:
            write_ply(path, points, colors)
    return (points, colors, normals) if oriented else (points, colors)


@torch.no_grad()
def export_pointcloud(trainer, dataset, indices: Optional[Sequence[int]] = None, path=None, n_points: int = 1_000_000,
                      min_opacity: float = 0.5, depth: str = "expected", crop=None, seed: int = 0, rendered=None):
    """Point cloud of the views ``indices`` (default: all) of a ``PoseDataset`` / ``CameraPoseDataset``: every view's rays are
    rendered with ``trainer.render_rays(maps=True)`` -- or taken from ``rendered``, the dicts ``infer(maps=True)`` made for the same
    indices --, compacted (``compact_points``) and concatenated in view order.  More than ``n_points`` in total: a random subset of
    exactly ``n_points`` is kept, the first ``n_points`` of ``torch.randperm`` under a generator seeded with ``seed``, sorted, so
    view order and ray order survive.  ``crop``: 6 values (lo xyz, hi xyz); ``None``: ``default_crop`` of the trainer's
    configuration; ``False``: no box.  Returns ``(points [M,3] float32, colors [M,3] uint8)`` on the device and writes ``path`` (a
    PLY) when one is given."""
    return _export(trainer, dataset, indices, path, n_points, min_opacity, depth, crop, seed, rendered, False)


@torch.no_grad()
def export_oriented_pointcloud(trainer, dataset, indices: Optional[Sequence[int]] = None, path=None, n_points: int = 1_000_000,
                               min_opacity: float = 0.5, depth: str = "expected", crop=None, seed: int = 0, rendered=None):
    """``export_pointcloud`` with the surface orientation: ``(points [M,3] float32, colors [M,3] uint8, normals [M,3] float32)``, the
    normals being the kept rays' ``normal`` rows of ``trainer.render_rays(maps=True, normals=True)`` -- or of ``rendered``, the dicts
    ``infer(maps=True, normals=True)`` made; dicts without ``normal`` are a ``ValueError`` -- unit length or zero, pointing from dense
    to empty.  Same parameters, same points and colours; ``path`` is written in ``write_ply``'s dialect with normals.  K-Planes and
    hash-grid fields only (``core.sample_normals``)."""
    return _export(trainer, dataset, indices, path, n_points, min_opacity, depth, crop, seed, rendered, True)


def _host(x, dtype) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x, dtype=dtype)


def write_ply(path, points, colors, normals=None) -> None:
    """Binary little-endian PLY 1.0 with ``element vertex M`` and the properties float x, y, z, uchar red, green, blue: 15 B per
    vertex, written from one structured array.  ``points`` [M,3] float32 and ``colors`` [M,3] uint8, tensors or arrays.  With
    ``normals`` [M,3] float32 the second dialect is written: float nx, ny, nz after x, y, z, 27 B per vertex."""
    xyz, rgb = _host(points, np.float32).reshape(-1, 3), _host(colors, np.uint8).reshape(-1, 3)
    if xyz.shape[0] != rgb.shape[0]:
        raise ValueError("write_ply: points and colors differ in length")
    nrm = None if normals is None else _host(normals, np.float32).reshape(-1, 3)
    if nrm is not None and nrm.shape[0] != xyz.shape[0]:
        raise ValueError("write_ply: points and normals differ in length")
    vertex = np.empty(xyz.shape[0], dtype=PLY_VERTEX if nrm is None else PLY_VERTEX_N)
    for k, name in enumerate(("x", "y", "z")):
        vertex[name] = xyz[:, k]
    if nrm is not None:
        for k, name in enumerate(("nx", "ny", "nz")):
            vertex[name] = nrm[:, k]
    for k, name in enumerate(("red", "green", "blue")):
        vertex[name] = rgb[:, k]
    with open(path, "wb") as f:
        f.write(((_PLY_HEADER if nrm is None else _PLY_HEADER_N) % vertex.shape[0]).encode("ascii"))
        f.write(vertex.tobytes())


def read_ply(path, normals: bool = False):
    """``(points [M,3] float32, colors [M,3] uint8)`` as numpy arrays from a file in ``write_ply``'s dialect; with ``normals``
    ``(points, colors, normals [M,3] float32)`` from a file in its dialect with normals.  Any other header -- the other dialect
    included -- raises ``ValueError``."""
    header, dtype = (_PLY_HEADER_N, PLY_VERTEX_N) if normals else (_PLY_HEADER, PLY_VERTEX)
    with open(path, "rb") as f:
        raw = f.read()
    end = raw.find(b"end_header\n")
    if end < 0:
        raise ValueError(f"{path}: not a PLY file (no end_header)")
    head, body = raw[:end + 11].decode("ascii", errors="replace"), raw[end + 11:]
    lines = head.split("\n")
    try:
        m = int(lines[2].split()[2]) if lines[2].startswith("element vertex ") else -1
    except (IndexError, ValueError):
        m = -1
    if m < 0 or head != header % m:
        raise ValueError(f"{path}: not the PLY dialect asked for (binary little-endian, float xyz"
                         f"{' + float normals' if normals else ''} + uchar rgb)")
    if len(body) != dtype.itemsize * m:
        raise ValueError(f"{path}: {len(body)} bytes of vertices, the header promises {dtype.itemsize * m}")
    vertex = np.frombuffer(body, dtype=dtype, count=m)
    out = (np.stack([vertex["x"], vertex["y"], vertex["z"]], 1), np.stack([vertex["red"], vertex["green"], vertex["blue"]], 1))
    return out + (np.stack([vertex["nx"], vertex["ny"], vertex["nz"]], 1),) if normals else out
