"""Triangle mesh of what the model RENDERS: the depth maps of known cameras fused into a truncated signed distance field
on ``mesh.extract``'s grid, its zero level extracted, the cells no view has observed masked out, small pieces dropped.  Against the
level set of the raw density (``mesh.export_mesh``) the level is 0 whatever the grid, the depth along a ray is already a weighted sum
over the whole ray, so fog averages out, and views that disagree vote.

* ``integrate`` -- ``tn_tsdf_integrate``: the views of a camera table and their depth maps added into ``(S, W)``;
* ``integrate_color`` -- ``tn_tsdf_integrate_color``: the same views' rendered colours added into the colour volume ``C``;
* ``sample_colors`` -- ``tn_tsdf_sample_colors``: the colour volume at points, e.g. the mesh's vertices;
* ``field`` -- the mesh field ``-S / W`` (``-1`` where ``W == 0``), level 0, inside ``>= 0``;
* ``mask_faces`` -- ``tn_tsdf_mask_faces``: faces of cells with an unobserved corner become ``(-1, -1, -1)``;
* ``camera_table`` -- the pose-only ``rays.CameraRays`` of a ``PoseDataset`` / ``CameraPoseDataset``;
* ``export_tsdf_mesh`` -- render, integrate, extract, mask, filter, colour (the decoder's, or ``"fused"`` from the renders), write;
* ``export_smooth_tsdf_mesh`` -- the same with ``mesh.smooth_mesh`` as the last step before the file.

torch is plumbing only; there is no CPU path.  No reference counterpart: the reference renders images and exports no geometry.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from .mesh import _grid, cut_box
from .rays import CameraRays

# Views per launch.  Every split gives the same bytes (the definition), so this is a matter of time alone: all views in one launch make
# every workgroup sweep every map, chunks cost 8 B of read-modify-write per node and launch.  Measured (scripts/tsdf_time.py):
# 100 views of 200 x 200 into 257^3 nodes take 6.3 ms in one launch, 3.3 ms at 16 views per launch, 6.4 ms at one view per launch.
# The colour pass (16 B per node and launch) has the same optimum: 6.6 ms, 3.5 ms and 10.1 ms.
VIEWS_PER_LAUNCH = 16


def integrate(cams: CameraRays, depth: torch.Tensor, opacity: Optional[torch.Tensor], box, dims: Sequence[int], trunc: float,
              min_opacity: float = 0.5, state: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
              views: Optional[Tuple[int, int]] = None):
    """``(S, W)``, float32 ``[nz+1, ny+1, nx+1]`` each, on the device: the views of the camera table ``cams`` added into the TSDF on
    the grid of ``box`` (lo xyz, hi xyz) cut into ``dims = (nx, ny, nz)`` cells (include/tinynerf_hip.h has the definition).  ``depth``
    holds one distance along the unit ray per pixel of the table, in its flat pixel order; ``opacity`` likewise, or ``None`` (then
    ``min_opacity`` is not used).  ``state``: the ``(S, W)`` of an earlier call, added to IN PLACE (``None``: zeros).  ``views``:
    ``(first, count)`` (``None``: all).  The views go to the kernel ``VIEWS_PER_LAUNCH`` at a time; every split gives the same bytes."""
    lo, h, dims = cut_box(box, dims, "tsdf")
    if not (math.isfinite(float(trunc)) and float(trunc) > 0.0):
        raise ValueError("tsdf.integrate: trunc must be finite and > 0")
    first, count = (0, cams.n_img) if views is None else (int(views[0]), int(views[1]))
    if first < 0 or count < 0 or first + count > cams.n_img:
        raise ValueError("tsdf.integrate: views must lie inside the camera table")
    if depth.numel() != cams.n_rays or (opacity is not None and opacity.numel() != cams.n_rays):
        raise ValueError("tsdf.integrate: depth and opacity must hold one entry per pixel of the camera table")
    if depth.dtype != torch.float32 or (opacity is not None and opacity.dtype != torch.float32):
        raise ValueError("tsdf.integrate: depth and opacity must be float32")
    shape = (dims[2] + 1, dims[1] + 1, dims[0] + 1)
    dev = L.require_cuda(cams.c2w, depth, opacity)
    if state is None:
        S, W = torch.zeros(shape, dtype=torch.float32, device=dev), torch.zeros(shape, dtype=torch.float32, device=dev)
    else:
        S, W = state
        if tuple(S.shape) != shape or tuple(W.shape) != shape or S.dtype != torch.float32 or W.dtype != torch.float32:
            raise ValueError("tsdf.integrate: state must be two float32 tensors [nz+1, ny+1, nx+1]")
        L.require_cuda(S, W, depth)
    lo_c, h_c, dims_c = _grid(lo, h, dims)
    for v in range(first, first + count, VIEWS_PER_LAUNCH):
        L.call("tn_tsdf_integrate", dev, C.byref(cams.table), L.ptr(depth), L.ptr(opacity), C.c_float(min_opacity), dims_c, lo_c, h_c,
               C.c_float(trunc), C.c_int32(v), C.c_int32(min(VIEWS_PER_LAUNCH, first + count - v)), L.ptr(S), L.ptr(W))
    return S, W


def integrate_color(cams: CameraRays, depth: torch.Tensor, opacity: Optional[torch.Tensor], rgb: torch.Tensor, bg: Optional[torch.Tensor], box,
                    dims: Sequence[int], trunc: float, min_opacity: float = 0.5, state: Optional[torch.Tensor] = None,
                    views: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """``C``, float32 ``[nz+1, ny+1, nx+1, 4]`` on the device: ``(sum w r, sum w g, sum w b, sum w)`` per node of ``integrate``'s grid
    -- the views' rendered colours ``rgb [n_pixels, 3]`` (composited over ``bg [3]``; ``None``: black), the background taken out
    again, added at the weight ``w = 1 - |sdf| / trunc`` wherever a view puts the node within ``trunc`` of its surface
    (include/tinynerf_hip.h has the definition).  ``depth``, ``opacity`` (with one, ``min_opacity`` must be ``> 0``), ``box``,
    ``dims``, ``trunc`` and ``views`` are ``integrate``'s; ``state``: the ``C`` of an earlier call, added to IN PLACE (``None``:
    zeros).  The views go to the kernel ``VIEWS_PER_LAUNCH`` at a time; every split gives the same bytes."""
    lo, h, dims = cut_box(box, dims, "tsdf")
    if not (math.isfinite(float(trunc)) and float(trunc) > 0.0):
        raise ValueError("tsdf.integrate_color: trunc must be finite and > 0")
    if opacity is not None and not float(min_opacity) > 0.0:
        raise ValueError("tsdf.integrate_color: with an opacity map min_opacity must be > 0 (the colour is divided by the opacity)")
    first, count = (0, cams.n_img) if views is None else (int(views[0]), int(views[1]))
    if first < 0 or count < 0 or first + count > cams.n_img:
        raise ValueError("tsdf.integrate_color: views must lie inside the camera table")
    if depth.numel() != cams.n_rays or (opacity is not None and opacity.numel() != cams.n_rays) or rgb.numel() != 3 * cams.n_rays:
        raise ValueError("tsdf.integrate_color: depth and opacity must hold one entry per pixel of the camera table, rgb three")
    if depth.dtype != torch.float32 or (opacity is not None and opacity.dtype != torch.float32) or rgb.dtype != torch.float32:
        raise ValueError("tsdf.integrate_color: depth, opacity and rgb must be float32")
    if bg is not None and (bg.numel() != 3 or bg.dtype != torch.float32):
        raise ValueError("tsdf.integrate_color: bg must be three float32 values")
    shape = (dims[2] + 1, dims[1] + 1, dims[0] + 1, 4)
    dev = L.require_cuda(cams.c2w, depth, opacity, rgb, bg)
    if state is None:
        vol = torch.zeros(shape, dtype=torch.float32, device=dev)
    else:
        vol = state
        if tuple(vol.shape) != shape or vol.dtype != torch.float32:
            raise ValueError("tsdf.integrate_color: state must be a float32 tensor [nz+1, ny+1, nx+1, 4]")
        L.require_cuda(vol, depth)
    lo_c, h_c, dims_c = _grid(lo, h, dims)
    for v in range(first, first + count, VIEWS_PER_LAUNCH):
        L.call("tn_tsdf_integrate_color", dev, C.byref(cams.table), L.ptr(depth), L.ptr(opacity), C.c_float(min_opacity), L.ptr(rgb), L.ptr(bg),
               dims_c, lo_c, h_c, C.c_float(trunc), C.c_int32(v), C.c_int32(min(VIEWS_PER_LAUNCH, first + count - v)), L.ptr(vol))
    return vol


def sample_colors(C: torch.Tensor, box, dims: Sequence[int], points: torch.Tensor):
    """``(rgb [n,3] float32, den [n] float32)``: the colour volume ``C`` of ``integrate_color`` on the grid of ``box`` and ``dims`` at
    ``points [n,3]`` (``tn_tsdf_sample_colors``) -- the trilinear interpolants of ``sum w rgb`` and of ``sum w`` in the point's cell
    (a point outside the box is clamped onto it), divided; nodes without colour carry no weight and drop out of the average.
    ``den == 0`` (then ``rgb == 0``): no coloured node around the point, or a coordinate that is not finite."""
    lo, h, dims = cut_box(box, dims, "tsdf")
    if points.dim() != 2 or points.size(1) != 3 or points.dtype != torch.float32:
        raise ValueError("tsdf.sample_colors: points must be [n,3] float32")
    if C.dtype != torch.float32 or tuple(C.shape) != (dims[2] + 1, dims[1] + 1, dims[0] + 1, 4):
        raise ValueError("tsdf.sample_colors: C must be a float32 tensor [nz+1, ny+1, nx+1, 4]")
    from ctypes import c_int64                                     # (the module's alias C is the volume here)
    dev = L.require_cuda(C, points)
    n = points.size(0)
    out = torch.zeros((n, 4), dtype=torch.float32, device=dev)     # (zeros: an axis of 0 cells launches nothing)
    lo_c, h_c, dims_c = _grid(lo, h, dims)
    if n:
        L.call("tn_tsdf_sample_colors", dev, L.ptr(C), dims_c, lo_c, h_c, L.ptr(points), c_int64(n), L.ptr(out))
    return out[:, :3].contiguous(), out[:, 3].contiguous()


def field(S: torch.Tensor, W: torch.Tensor) -> torch.Tensor:
    """the mesh field of a TSDF: ``-S / W`` where ``W > 0``, ``-1`` (empty) elsewhere; the surface is its level 0, inside ``>= 0``"""
    seen = W > 0
    return torch.where(seen, -S / torch.where(seen, W, torch.ones_like(W)), torch.full_like(S, -1.0))


def mask_faces(W: torch.Tensor, dims: Sequence[int], cell_ids: torch.Tensor, n_vertices: int, faces: torch.Tensor) -> torch.Tensor:
    """a copy of ``faces [F,3] int32`` in which every face that names a vertex of a cell with an unobserved corner (``W == 0``), or an
    index outside ``[0, n_vertices)``, is ``(-1, -1, -1)`` (``tn_tsdf_mask_faces``); ``cell_ids`` is ``mesh.extract_with_cells``'s
    map.  ``mesh.filter_components(min_faces >= 1)`` then drops those faces and the vertices they orphan."""
    dims = tuple(int(d) for d in dims)
    V = int(n_vertices)
    if faces.dim() != 2 or faces.size(1) != 3 or faces.dtype != torch.int32 or V < 0:
        raise ValueError("mask_faces: faces must be [F,3] int32 and n_vertices >= 0")
    if len(dims) != 3 or min(dims) < 0 or W.dtype != torch.float32 or W.numel() != (dims[0] + 1) * (dims[1] + 1) * (dims[2] + 1):
        raise ValueError("mask_faces: W must be float32 with one entry per node of dims")
    if cell_ids.dtype != torch.int32 or cell_ids.numel() != dims[0] * dims[1] * dims[2]:
        raise ValueError("mask_faces: cell_ids must be int32 with one entry per cell of dims")
    dev = L.require_cuda(W, cell_ids, faces)
    out = faces.clone()
    observed = torch.empty(max(V, 1), dtype=torch.uint8, device=dev)
    L.call("tn_tsdf_mask_faces", dev, L.ptr(W), (C.c_int32 * 3)(*dims), L.ptr(cell_ids) if cell_ids.numel() else None,
           C.c_int64(V), L.ptr(out) if out.size(0) else None, C.c_int64(out.size(0)), L.ptr(observed))
    return out


def camera_table(dataset, indices: Optional[Sequence[int]] = None, device=None) -> CameraRays:
    """the pose-only camera table (no colours) of the views ``indices`` (``None``: all) of a ``data.PoseDataset`` -- one pinhole camera,
    its poses kept as ``cameras`` -- or a ``data.CameraPoseDataset`` -- the rows of its ``source``"""
    src = getattr(dataset, "source", None)
    idx = list(range(len(dataset))) if indices is None else [int(i) for i in indices]
    if src is not None:
        sel = torch.as_tensor(idx, dtype=torch.long)
        return CameraRays(src.c2w.cpu()[sel], src.lens.cpu()[sel], src.model.cpu()[sel], src.size.cpu()[sel], None, device or src.device)
    if not hasattr(dataset, "cameras"):
        raise ValueError("tsdf: the dataset must be a data.PoseDataset or a data.CameraPoseDataset")
    K = [dataset.img_intrinsics(i) for i in idx]
    lens = torch.zeros((len(idx), 10), dtype=torch.float32)
    if idx:
        lens[:, :4] = torch.tensor([[k.fx, k.fy, k.cx, k.cy] for k in K], dtype=torch.float64).float()
    return CameraRays(dataset.cameras[idx][:, :3, :], lens, [0] * len(idx), [[k.w, k.h] for k in K], None, device or dataset.rays_o.device)


@torch.no_grad()
def export_tsdf_mesh(trainer, dataset, path=None, resolution: int = 256, trunc: Optional[float] = None, crop=None,
                     indices: Optional[Sequence[int]] = None, min_faces: int = 0, keep_fraction: float = 0.0, depth: str = "expected",
                     colors: bool = True):
    """The mesh of what the trainer renders from the views ``indices`` (``None``: all) of ``dataset`` (a ``PoseDataset`` or a
    ``CameraPoseDataset``): every view rendered through ``render_rays(maps=True)``, its ``depth`` (``"expected"`` or ``"median"``) and
    opacity integrated into a TSDF on ``mesh.grid_dims(crop, resolution)`` (``crop`` ``None``: ``points.default_crop``) with the
    truncation ``trunc`` (``None``: ``4 max(h)``), the zero level extracted (``mesh.extract``), the faces of unobserved cells masked,
    and ``mesh.filter_components(max(1, min_faces), keep_fraction)`` -- which drops the masked faces and orphaned vertices, and the
    pieces below the threshold.  Returns ``(vertices, normals, colors, faces)`` on the device as ``mesh.export_mesh`` does -- colours
    from ``mesh.vertex_colors``, zeros when switched off -- and writes ``path`` (``mesh.write_mesh_ply``) when one is given.
    ``colors="fused"``: the colours come from the renders instead of the decoder -- the render loop also keeps every
    view's ``rgb`` (12 B per pixel beside the 8 B of depth and opacity it keeps anyway), ``integrate_color`` fuses them into a colour
    volume with the renderer's background taken out, and the surviving vertices take ``mesh.color_bytes(sample_colors(...))``; a
    vertex no coloured node surrounds (``den == 0``) takes the decoder's colour.  Any other string is a ``ValueError``."""
    return _export_tsdf_mesh("export_tsdf_mesh", trainer, dataset, path, resolution, trunc, crop, indices, min_faces, keep_fraction, depth, colors, 0, 0.5, -0.53)


@torch.no_grad()
def export_smooth_tsdf_mesh(trainer, dataset, path=None, resolution: int = 256, trunc: Optional[float] = None, crop=None,
                            indices: Optional[Sequence[int]] = None, min_faces: int = 0, keep_fraction: float = 0.0, depth: str = "expected",
                            colors: bool = True, smooth: int = 0, smooth_lambda: float = 0.5, smooth_mu: float = -0.53):
    """``export_tsdf_mesh`` with ``mesh.smooth_mesh(vertices, normals, faces, smooth, smooth_lambda, smooth_mu)`` as the last step
    before the file -- after the mask, the filter and the colours, which are asked or sampled at the EXTRACTED positions
    with the extracted normals (the decoder's, the fused volume's and the fallback for bare vertices alike).  With ``smooth == 0``
    it returns and writes what ``export_tsdf_mesh`` does and launches nothing of the smoothing.  (``export_tsdf_mesh`` keeps its
    signature, so this is a function beside it.)"""
    from . import mesh as M
    smooth = M.check_smooth("export_smooth_tsdf_mesh", smooth, smooth_lambda, smooth_mu)
    return _export_tsdf_mesh("export_smooth_tsdf_mesh", trainer, dataset, path, resolution, trunc, crop, indices, min_faces, keep_fraction, depth, colors,
                             smooth, smooth_lambda, smooth_mu)


def _export_tsdf_mesh(who, trainer, dataset, path, resolution, trunc, crop, indices, min_faces, keep_fraction, depth, colors, smooth, smooth_lambda, smooth_mu):
    from . import mesh as M
    from .points import DEPTH_KEYS
    M._one_rank(who, trainer)
    M.component_threshold(min_faces, keep_fraction, 0)             # the arguments, before any device work
    if depth not in DEPTH_KEYS:
        raise ValueError(f"{who}: depth must be one of {sorted(DEPTH_KEYS)}, not {depth!r}")
    if isinstance(colors, str) and colors != "fused":
        raise ValueError(f"{who}: colors must be True, False or 'fused', not {colors!r}")
    fused = isinstance(colors, str)
    box, lo, h, dims, trunc = M._export_grid(who, trainer, crop, resolution, trunc, lambda h: 4.0 * float(np.max(h)), "trunc")
    idx = list(range(len(dataset))) if indices is None else [int(i) for i in indices]
    dev = trainer.device
    S = torch.zeros((dims[2] + 1, dims[1] + 1, dims[0] + 1), dtype=torch.float32, device=dev)
    W = torch.zeros_like(S)
    volume = torch.zeros(S.shape + (4,), dtype=torch.float32, device=dev) if fused else None
    if idx:
        cams = camera_table(dataset, idx, dev)
        dist = torch.empty(cams.n_rays, dtype=torch.float32, device=dev)
        opacity = torch.empty(cams.n_rays, dtype=torch.float32, device=dev)
        rgb = torch.empty((cams.n_rays, 3), dtype=torch.float32, device=dev) if fused else None
        for k, i in enumerate(idx):
            item = dataset[i]
            o, d = item["rays_o"].reshape(-1, 3).to(dev), item["rays_d"].reshape(-1, 3).to(dev)
            if o.size(0) != cams.offsets[k + 1] - cams.offsets[k]:
                raise RuntimeError(f"{who}: a view's rays do not match the size its camera states")
            maps = trainer.render_rays(o, d, maps=True)
            dist[cams.offsets[k]:cams.offsets[k + 1]] = maps[DEPTH_KEYS[depth]].reshape(-1)
            opacity[cams.offsets[k]:cams.offsets[k + 1]] = maps["opacity"].reshape(-1)
            if fused:
                rgb[cams.offsets[k]:cams.offsets[k + 1]] = maps["rgb"].reshape(-1, 3)
        integrate(cams, dist, opacity, box, dims, trunc, state=(S, W))          # (box and dims give lo and h again: cut_box both times)
        if fused:
            integrate_color(cams, dist, opacity, rgb, trainer.renderer._bg(dev), box, dims, trunc, state=volume)
    vertices, normals, faces, cells = M.extract_with_cells(field(S, W), lo, h, 0.0)
    faces = mask_faces(W, dims, cells, vertices.size(0), faces)
    vertices, normals, _, faces = M.filter_components(vertices, normals, None, faces, min_faces=max(1, int(min_faces)), keep_fraction=keep_fraction)
    if not fused:
        return M._finish_export(trainer, path, vertices, normals, faces, colors, smooth, smooth_lambda, smooth_mu)
    sampled, den = sample_colors(volume, box, dims, vertices)
    out = M.color_bytes(sampled)
    bare = (den == 0).nonzero().reshape(-1)                        # no coloured node around the vertex: ask the decoder, for these alone
    if bare.numel():
        out[bare] = M.vertex_colors(trainer, vertices[bare].contiguous(), normals[bare].contiguous())
    return M._write_export(path, vertices, normals, out, faces, smooth, smooth_lambda, smooth_mu)
