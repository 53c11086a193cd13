"""Triangle mesh of a trained scene's density: the density sampled at the nodes of a regular grid over a box, its level
set extracted by naive Surface Nets on the device -- one vertex per cell the surface passes through, one quad per grid edge it
crosses; an indexed mesh, closed and consistently oriented wherever the surface does not reach the box --, written as a PLY.

* ``extract`` -- ``tn_mesh_extract`` over a tensor of node values: vertices, normals, faces; ``extract_with_cells`` -- and the cell -> vertex id map;
* ``density_grid`` / ``extract_mesh`` -- the node values of a trainer / of any density callable, and their mesh;
* ``export_mesh`` -- a trainer's mesh with vertex colours from its colour decoder, written to ``path``;
* ``adjacency`` / ``smooth`` / ``vertex_normals`` / ``smooth_mesh`` -- Taubin smoothing of a mesh and the normals of its faces;
* ``write_mesh_ply`` / ``read_mesh_ply`` -- binary little-endian PLY, 27 B per vertex, 13 B per face.

The mesh is in the frame the rays are in: for a capture that is the frame after ``data.orient_poses``, not the capture's own.
torch is plumbing only; there is no CPU path.  No reference counterpart: the reference renders images and exports no geometry.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Callable, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L

MESH_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                        ("red", "u1"), ("green", "u1"), ("blue", "u1")])                       # packed: 27 B
MESH_FACE = np.dtype([("n", "u1"), ("a", "<i4"), ("b", "<i4"), ("c", "<i4")])                  # packed: 13 B
_MESH_HEADER = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
                "element face %d\nproperty list uchar int vertex_indices\nend_header\n")


def _triple(x, ctype):
    return (ctype * 3)(*[x[0], x[1], x[2]])


def _grid(lo, h, dims):
    """host arrays of the C ABI: lo / h as float32 (the values the kernels use), dims (nx, ny, nz)"""
    lo32, h32 = np.asarray(lo, np.float32).reshape(3), np.asarray(h, np.float32).reshape(3)
    return _triple(lo32.tolist(), C.c_float), _triple(h32.tolist(), C.c_float), _triple([int(d) for d in dims], C.c_int32)


def grid_nodes(lo, h, dims: Sequence[int], first: int, n: int, device) -> torch.Tensor:
    """``[n,3]`` world positions of nodes ``first .. first + n`` (x fastest) of the grid, ``fmaf(idx, h, lo)`` per axis (``tn_grid_nodes``)"""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("tinynerf_amd: grid_nodes needs a CUDA (HIP) device -- there is no CPU path")
    out = torch.empty((int(n), 3), dtype=torch.float32, device=device)
    lo_c, h_c, dims_c = _grid(lo, h, dims)
    L.call("tn_grid_nodes", device, lo_c, h_c, dims_c, C.c_int64(first), C.c_int64(n), L.ptr(out))
    return out


def extract(values: torch.Tensor, lo, h, level: float, normals: bool = True, capacity: Optional[Tuple[int, int]] = None):
    """``(vertices [V,3] float32, normals [V,3] float32 or None, faces [F,3] int32)`` on the device: the Surface Nets mesh of the level
    set ``values == level`` (inside: ``values >= level``) of ``values [nz+1, ny+1, nx+1]``, the field at the nodes ``lo + idx h`` of a
    grid of ``nx x ny x nz`` cells (include/tinynerf_hip.h has the definition).  The normals point from inside to outside.
    ``capacity=None``: a count-only call, one read-back, then the call that writes; ``(vertex rows, face rows)``: one call into buffers
    of that size -- at most that many rows come back (the first ones), the faces still naming the full mesh's vertices."""
    return _extract(values, lo, h, level, normals, capacity, False)


def extract_with_cells(values: torch.Tensor, lo, h, level: float, normals: bool = True, capacity: Optional[Tuple[int, int]] = None):
    """``extract`` with a fourth entry, ``cell_ids [nz, ny, nx] int32``: every cell's vertex id, -1 for a cell without a vertex -- a
    copy of the map the extractor leaves in its workspace (``tsdf.mask_faces`` reads it)"""
    return _extract(values, lo, h, level, normals, capacity, True)


def _extract(values, lo, h, level, normals, capacity, return_cells):
    if values.dim() != 3 or min(values.shape) < 1:
        raise ValueError("extract: values must be [nz+1, ny+1, nx+1]")
    v = values if values.dtype == torch.float32 and values.is_contiguous() else values.float().contiguous()
    dev = L.require_cuda(v)
    dims = (v.size(2) - 1, v.size(1) - 1, v.size(0) - 1)
    lo_c, h_c, dims_c = _grid(lo, h, dims)
    nbytes = C.c_int64(0)
    L.call_plain("tn_mesh_workspace_bytes", dims_c[0], dims_c[1], dims_c[2], C.byref(nbytes))
    workspace = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)

    def run(vcap: int, fcap: int):
        vert = torch.empty((vcap, 3), dtype=torch.float32, device=dev)
        nrm = torch.empty((vcap, 3), dtype=torch.float32, device=dev) if normals else None
        faces = torch.empty((fcap, 3), dtype=torch.int32, device=dev)
        L.call("tn_mesh_extract", dev, L.ptr(v), dims_c, lo_c, h_c, C.c_float(level), C.c_int64(vcap), C.c_int64(fcap),
               L.ptr(vert) if vcap else None, L.ptr(nrm) if vcap else None, L.ptr(faces) if fcap else None, L.ptr(counts), L.ptr(workspace))
        return vert, nrm, faces

    def cells(written: bool):
        """the id map: behind the ballots and counts of ceil(cells / 256) workgroups, 144 B each; only a call with a capacity > 0 writes it"""
        n = dims[0] * dims[1] * dims[2]
        if not written or n == 0:
            return torch.full((dims[2], dims[1], dims[0]), -1, dtype=torch.int32, device=dev)
        first = 144 * (-(-n // 256))
        return workspace[first:first + 4 * n].view(torch.int32).view(dims[2], dims[1], dims[0]).clone()

    if capacity is None:
        run(0, 0)
        n_v, n_f = counts.tolist()
        out = run(n_v, n_f)
        return out + (cells(n_v > 0 or n_f > 0),) if return_cells else out
    vcap, fcap = int(capacity[0]), int(capacity[1])
    if vcap < 0 or fcap < 0:
        raise ValueError("extract: capacity must be >= 0")
    vert, nrm, faces = run(vcap, fcap)
    n_v, n_f = counts.tolist()
    n_v, n_f = min(n_v, vcap), min(n_f, fcap)
    out = vert[:n_v], None if nrm is None else nrm[:n_v], faces[:n_f]
    return out + (cells(vcap > 0 or fcap > 0),) if return_cells else out


def cut_box(box, dims: Sequence[int], who: Optional[str] = None):
    """``(lo, h, dims)``: ``box`` (lo xyz, hi xyz) cut into ``dims = (nx, ny, nz)`` cells -- ``lo`` and ``h = extent / dims`` rounded to
    float32, as the kernels use them.  With ``who``, box and dims are checked first (``ValueError`` in that name) and an axis of 0
    cells keeps its whole extent as ``h``."""
    box = np.asarray(box, np.float64).reshape(6)
    dims = tuple(int(d) for d in dims)
    cells = np.float64(dims)
    if who is not None:
        if len(dims) != 3 or min(dims) < 0:
            raise ValueError(f"{who}: dims must be three cell counts >= 0")
        if not np.isfinite(box).all() or not (box[3:] > box[:3]).all():
            raise ValueError(f"{who}: the box must be finite with a positive extent on every axis")
        cells = np.maximum(cells, 1.0)
    return box[:3].astype(np.float32), ((box[3:] - box[:3]) / cells).astype(np.float32), dims


def grid_dims(box, resolution: int):
    """``(lo, h, dims)``: ``resolution`` cells on the longest axis of ``box`` (lo xyz, hi xyz), ``ceil(resolution extent / longest)``
    on the others -- near-cubic cells; ``lo`` and ``h`` from ``cut_box``"""
    box = np.asarray(box, np.float64).reshape(6)
    extent = box[3:] - box[:3]
    if int(resolution) < 1 or not (extent > 0).all() or not np.isfinite(box).all():
        raise ValueError("mesh: resolution must be >= 1 and the box finite with a positive extent on every axis")
    return cut_box(box, [max(1, int(math.ceil(int(resolution) * e / extent.max() - 1e-9))) for e in extent])


@torch.no_grad()
def _log_density(sigma_fn: Callable, contraction, lo, h, dims, device, chunk: int) -> torch.Tensor:
    nx, ny, nz = dims
    n = (nx + 1) * (ny + 1) * (nz + 1)
    out = torch.empty(n, dtype=torch.float32, device=device)
    for first in range(0, n, chunk):
        m = min(chunk, n - first)
        x = grid_nodes(lo, h, dims, first, m, device)
        if contraction is not None:
            x = contraction(x)[0]                          # exactly as the sampler contracts a sample
        sigma = sigma_fn(x).detach().reshape(-1).float()
        out[first:first + m] = torch.log(sigma.clamp_min(1e-30))
    return out.view(nz + 1, ny + 1, nx + 1)


def density_grid(trainer, box, dims: Sequence[int], chunk: int = 1 << 21):
    """``(values [nz+1, ny+1, nx+1], lo, h)``: ``log(max(sigma, 1e-30))`` of the trainer's density at the nodes of ``box`` (lo xyz, hi xyz)
    cut into ``dims = (nx, ny, nz)`` cells -- the nodes from ``tn_grid_nodes``, contracted with the trainer's contraction,
    ``trainer.sigma_fn`` under ``no_grad``, ``chunk`` nodes per call"""
    lo, h, dims = cut_box(box, dims)
    trainer.renderer.eval()
    return _log_density(trainer.sigma_fn, trainer.ray_provider.contraction, lo, h, dims, trainer.device, chunk), lo, h


def default_level(h) -> float:
    """the density at which a segment one cell long has opacity 0.5 -- ``compact_points``' ``min_opacity``: ``ln 2 / max(h)``"""
    return math.log(2.0) / float(np.max(np.asarray(h, np.float64)))


def extract_mesh(sigma_fn: Callable, box, resolution: int, level: Optional[float] = None, contraction=None, device=None,
                 chunk: int = 1 << 21):
    """``extract`` of ``log sigma_fn`` on the grid ``grid_dims(box, resolution)``, for any callable from points ``[n,3]`` on the device
    (contracted by ``contraction`` first, when given) to densities ``[n]``.  ``level``: the density of the surface (default
    ``default_level``).  Returns ``(vertices, normals, faces)``."""
    lo, h, dims = grid_dims(box, resolution)
    device = torch.device("cuda") if device is None else device
    values = _log_density(sigma_fn, contraction, lo, h, dims, device, chunk)
    sigma = default_level(h) if level is None else float(level)
    if not sigma > 0.0 or not math.isfinite(sigma):
        raise ValueError("mesh: level is a density: it must be finite and > 0")
    return extract(values, lo, h, math.log(sigma))


def color_bytes(c: torch.Tensor) -> torch.Tensor:
    """colours -> bytes as ``tn_points_compact`` does: clamp to [0,1] with NaN -> 0, ``(uint8) fmaf(c, 255, 0.5)`` (the float64 product
    and sum are exact: their rounding to float32 is the fma's)"""
    c = c.float()
    c = torch.where(c > 0, c.clamp_max(1.0), torch.zeros_like(c))
    return (c.double() * 255.0 + 0.5).float().to(torch.uint8)


@torch.no_grad()
def vertex_colors(trainer, vertices: torch.Tensor, normals: torch.Tensor, chunk: int = 1 << 20) -> torch.Tensor:
    """``[V,3] uint8``: the colour decoder's output at the vertices -- the feature module at the contracted vertex, the view direction
    ``-n`` (looking at the surface head-on), ``(0,0,-1)`` where ``n = 0``"""
    r = trainer.renderer
    r.eval()
    out = torch.empty((vertices.size(0), 3), dtype=torch.uint8, device=vertices.device)
    for k in range(0, vertices.size(0), chunk):
        x, n = vertices[k:k + chunk], normals[k:k + chunk]
        d = torch.where((n == 0).all(1, keepdim=True), torch.tensor([0.0, 0.0, -1.0], device=n.device), -n).contiguous()
        feats = r.feature_module(trainer.ray_provider.contraction(x.contiguous())[0])
        out[k:k + chunk] = color_bytes(r.rgb_decoder(feats, d))
    return out


def _one_rank(who, trainer):
    if getattr(trainer, "world", 1) > 1:
        raise ValueError(f"{who} runs on one rank: world_size > 1 is not supported")


def _export_grid(who, trainer, crop, resolution, level, default, what):
    """``(box, lo, h, dims, level)`` of an export: the grid ``grid_dims(crop, resolution)`` (``crop`` ``None``:
    ``points.default_crop``) and ``level`` (``None``: ``default(h)``), which must be finite and > 0 -- ``what`` says of what"""
    from .points import default_crop
    box = default_crop(trainer.cfg) if crop is None else crop
    lo, h, dims = grid_dims(box, resolution)
    level = default(h) if level is None else float(level)
    if not (math.isfinite(level) and level > 0.0):
        raise ValueError(f"{who}: {what} must be finite and > 0")
    return box, lo, h, dims, level


def _density_surface(trainer, lo, h, dims, sigma):
    trainer.renderer.eval()
    values = _log_density(trainer.sigma_fn, trainer.ray_provider.contraction, lo, h, dims, trainer.device, 1 << 21)
    return extract(values, lo, h, math.log(sigma))


def _write_export(path, vertices, normals, rgb, faces, smooth, smooth_lambda, smooth_mu):
    """the last step of every mesh export: ``smooth_mesh`` when ``smooth`` > 0 (the colours were taken at the extracted positions),
    ``path`` written (``write_mesh_ply``) when one is given -> ``(vertices, normals, colors, faces)``"""
    if smooth:
        vertices, normals = smooth_mesh(vertices, normals, faces, smooth, lam=smooth_lambda, mu=smooth_mu)
    if path is not None:
        write_mesh_ply(path, vertices, normals, rgb, faces)
    return vertices, normals, rgb, faces


def _finish_export(trainer, path, vertices, normals, faces, colors, smooth=0, smooth_lambda=0.5, smooth_mu=-0.53):
    """the end of every mesh export: colours from ``vertex_colors`` (zeros when switched off or without vertices), then
    ``_write_export`` -> ``(vertices, normals, colors, faces)``"""
    rgb = vertex_colors(trainer, vertices, normals) if colors and vertices.size(0) else torch.zeros((vertices.size(0), 3), dtype=torch.uint8, device=vertices.device)
    return _write_export(path, vertices, normals, rgb, faces, smooth, smooth_lambda, smooth_mu)


@torch.no_grad()
def export_mesh(trainer, path=None, resolution: int = 256, level: Optional[float] = None, crop=None, colors: bool = True):
    """The mesh of the trainer's density inside ``crop`` (6 values, lo xyz then hi xyz; ``None``: ``points.default_crop`` of its
    configuration) on ``grid_dims(crop, resolution)``, at the density ``level`` (default ``default_level``).  Returns ``(vertices [V,3]
    float32, normals [V,3] float32, colors [V,3] uint8, faces [F,3] int32)`` on the device -- ``colors`` (``vertex_colors``) zeros
    when switched off -- and writes ``path`` (``write_mesh_ply``) when one is given."""
    _one_rank("export_mesh", trainer)
    _, lo, h, dims, sigma = _export_grid("export_mesh", trainer, crop, resolution, level, default_level, "level is a density: it")
    vertices, normals, faces = _density_surface(trainer, lo, h, dims, sigma)
    return _finish_export(trainer, path, vertices, normals, faces, colors)


def components(faces: torch.Tensor, n_vertices: int):
    """``(labels [V] int32, face_counts [V] int32, stats)`` of the mesh ``faces [F,3] int32`` over ``n_vertices`` vertices
    (``tn_mesh_components``): ``labels[v]`` the smallest vertex id of ``v``'s connected component, ``face_counts[r]`` the
    valid faces of the component whose label is ``r`` (0 elsewhere), ``stats = (components, components with a face, largest face
    count)`` as ints, from one read-back.  A face with an index outside ``[0, n_vertices)`` takes no part."""
    V = int(n_vertices)
    if faces.dim() != 2 or faces.size(1) != 3 or faces.dtype != torch.int32 or V < 0:
        raise ValueError("components: faces must be [F,3] int32 and n_vertices >= 0")
    dev = L.require_cuda(faces)
    F = faces.size(0)
    nbytes = C.c_int64(0)
    L.call_plain("tn_mesh_components_workspace_bytes", C.c_int64(V), C.c_int64(F), C.byref(nbytes))
    workspace = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    labels, face_counts = torch.empty(V, dtype=torch.int32, device=dev), torch.empty(V, dtype=torch.int32, device=dev)
    stats = torch.empty(3, dtype=torch.int64, device=dev)
    L.call("tn_mesh_components", dev, L.ptr(faces) if F else None, C.c_int64(V), C.c_int64(F), L.ptr(labels) if V else None,
           L.ptr(face_counts) if V else None, L.ptr(stats), L.ptr(workspace) if V else None)
    return labels, face_counts, tuple(stats.tolist())


def component_threshold(min_faces: int, keep_fraction: float, largest: int) -> int:
    """The filter's face-count threshold ``T = max(min_faces, ceil(keep_fraction * largest))``, in exact arithmetic (the float
    ``keep_fraction`` taken as the rational it is): ``keep_fraction = 1.0`` gives ``largest`` -- only the largest component stays,
    ties all kept.  ``ValueError`` for ``min_faces < 0``, for ``keep_fraction`` outside ``[0, 1]`` or NaN."""
    from fractions import Fraction
    if isinstance(min_faces, bool) or int(min_faces) != min_faces or int(min_faces) < 0:
        raise ValueError("filter_components: min_faces must be an integer >= 0")
    k = float(keep_fraction)
    if not 0.0 <= k <= 1.0:                                        # (NaN fails both comparisons)
        raise ValueError("filter_components: keep_fraction must lie in [0, 1]")
    return max(int(min_faces), math.ceil(Fraction(k) * int(largest)))


def filter_components(vertices: torch.Tensor, normals: Optional[torch.Tensor], colors: Optional[torch.Tensor], faces: torch.Tensor,
                      min_faces: int = 0, keep_fraction: float = 0.0, return_src: bool = False):
    """``(vertices, normals, colors, faces)`` on the device -- and ``src [V'] int32``, the old id of every kept vertex, with
    ``return_src`` --: the connected components of the mesh with at least ``component_threshold(min_faces, keep_fraction, largest)``
    faces (``tn_mesh_components`` + ``tn_mesh_filter``).  Kept vertices and faces keep their order, the rows are copied bit
    for bit, the faces renumbered; faces with an index outside ``[0, V)`` are dropped.  ``normals`` / ``colors`` (``[V,3] uint8``) may
    be ``None`` and come back as ``None``.  One read-back for the statistics, a count-only call, one read-back, the writing call."""
    component_threshold(min_faces, keep_fraction, 0)               # the arguments, before any device work
    if vertices.dim() != 2 or vertices.size(1) != 3 or vertices.dtype != torch.float32 or faces.dtype != torch.int32:
        raise ValueError("filter_components: vertices must be [V,3] float32 and faces [F,3] int32")
    V, F = vertices.size(0), faces.size(0)
    for name, t, dtype in (("normals", normals, torch.float32), ("colors", colors, torch.uint8)):
        if t is not None and (t.shape != vertices.shape or t.dtype != dtype):
            raise ValueError(f"filter_components: {name} must be [V,3] {dtype}")
    dev = L.require_cuda(vertices, normals, colors, faces)
    labels, face_counts, stats = components(faces, V)
    threshold = component_threshold(min_faces, keep_fraction, stats[2])
    nbytes = C.c_int64(0)
    L.call_plain("tn_mesh_filter_workspace_bytes", C.c_int64(V), C.c_int64(F), C.byref(nbytes))
    workspace = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)

    def run(vcap: int, fcap: int):
        out_v = torch.empty((vcap, 3), dtype=torch.float32, device=dev)
        out_n = None if normals is None else torch.empty((vcap, 3), dtype=torch.float32, device=dev)
        out_c = None if colors is None else torch.empty((vcap, 3), dtype=torch.uint8, device=dev)
        src = torch.empty(vcap, dtype=torch.int32, device=dev)
        out_f = torch.empty((fcap, 3), dtype=torch.int32, device=dev)
        some = lambda t, n: L.ptr(t) if n and t is not None else None      # noqa: E731  (an empty tensor's pointer is not passed)
        L.call("tn_mesh_filter", dev, some(faces, F), some(labels, V), some(face_counts, V), C.c_int64(threshold), some(vertices, V),
               some(normals, V), some(colors, V), C.c_int64(V), C.c_int64(F), C.c_int64(vcap), C.c_int64(fcap), some(out_v, vcap),
               some(out_n, vcap), some(out_c, vcap), some(src, vcap), some(out_f, fcap), L.ptr(counts), some(workspace, V))
        return out_v, out_n, out_c, out_f, src

    run(0, 0)
    n_v, n_f = counts.tolist()
    out = run(n_v, n_f)
    return out if return_src else out[:4]


@torch.no_grad()
def export_clean_mesh(trainer, path=None, resolution: int = 256, level: Optional[float] = None, crop=None, colors: bool = True,
                      min_faces: int = 0, keep_fraction: float = 0.0):
    """``export_mesh`` with ``filter_components(min_faces, keep_fraction)`` between the extraction and the colours: floaters and
    fragments below the threshold leave the mesh, and the colour decoder is only asked about vertices that stay.  With both options
    at 0 it returns and writes exactly what ``export_mesh`` does."""
    _one_rank("export_clean_mesh", trainer)
    component_threshold(min_faces, keep_fraction, 0)
    if not min_faces and not keep_fraction:
        return export_mesh(trainer, path, resolution=resolution, level=level, crop=crop, colors=colors)
    vertices, normals, faces = _clean_surface("export_clean_mesh", trainer, resolution, level, crop, min_faces, keep_fraction)
    return _finish_export(trainer, path, vertices, normals, faces, colors)


def _clean_surface(who, trainer, resolution, level, crop, min_faces, keep_fraction):
    """``(vertices, normals, faces)``: the density's surface on the export grid, through ``filter_components`` when an option is not 0"""
    _, lo, h, dims, sigma = _export_grid(who, trainer, crop, resolution, level, default_level, "level is a density: it")
    vertices, normals, faces = _density_surface(trainer, lo, h, dims, sigma)
    if min_faces or keep_fraction:
        vertices, normals, _, faces = filter_components(vertices, normals, None, faces, min_faces=min_faces, keep_fraction=keep_fraction)
    return vertices, normals, faces


@torch.no_grad()
def export_smooth_mesh(trainer, path=None, resolution: int = 256, level: Optional[float] = None, crop=None, colors: bool = True,
                       min_faces: int = 0, keep_fraction: float = 0.0, smooth: int = 0, smooth_lambda: float = 0.5, smooth_mu: float = -0.53):
    """``export_clean_mesh`` with ``smooth_mesh(vertices, normals, faces, smooth, smooth_lambda, smooth_mu)`` as the last step before
    the file: the order is extraction, component filter (when ``min_faces`` or ``keep_fraction`` is not 0), colours,
    smoothing.  The colours are the decoder's at the EXTRACTED positions with the extracted normals; the tuple and the file carry the
    smoothed positions and the normals of the smoothed faces.  With ``smooth == 0`` it IS a call of ``export_clean_mesh`` -- the same
    bytes, nothing of the smoothing launched.  (``export_mesh`` and ``export_clean_mesh`` keep their signatures, so this is a
    function beside them.)"""
    _one_rank("export_smooth_mesh", trainer)
    component_threshold(min_faces, keep_fraction, 0)
    if not check_smooth("export_smooth_mesh", smooth, smooth_lambda, smooth_mu):
        return export_clean_mesh(trainer, path, resolution=resolution, level=level, crop=crop, colors=colors, min_faces=min_faces, keep_fraction=keep_fraction)
    vertices, normals, faces = _clean_surface("export_smooth_mesh", trainer, resolution, level, crop, min_faces, keep_fraction)
    return _finish_export(trainer, path, vertices, normals, faces, colors, smooth, smooth_lambda, smooth_mu)


def check_smooth(who, iterations, lam=0.5, mu=-0.53) -> int:
    """``iterations`` as an int; ``ValueError`` in the name ``who`` for ``iterations < 0`` or not an integer, for a ``lam`` / ``mu`` that is not finite"""
    if isinstance(iterations, bool) or int(iterations) != iterations or int(iterations) < 0:
        raise ValueError(f"{who}: the smoothing iterations must be an integer >= 0")
    if not (math.isfinite(float(lam)) and math.isfinite(float(mu))):
        raise ValueError(f"{who}: the smoothing factors lambda and mu must be finite")
    return int(iterations)


def _check_mesh(who, vertices, faces, **rows):
    """shapes and dtypes of a mesh: ``vertices [V,3] float32``, ``faces [F,3] int32``, every given ``rows`` tensor ``[V,3] float32``"""
    if vertices.dim() != 2 or vertices.size(1) != 3 or vertices.dtype != torch.float32:
        raise ValueError(f"{who}: vertices must be [V,3] float32")
    if faces.dim() != 2 or faces.size(1) != 3 or faces.dtype != torch.int32:
        raise ValueError(f"{who}: faces must be [F,3] int32")
    for name, t in rows.items():
        if t is not None and (t.shape != vertices.shape or t.dtype != torch.float32):
            raise ValueError(f"{who}: {name} must be [V,3] float32")


def adjacency(faces: torch.Tensor, n_vertices: int):
    """``(offsets [V+1] int32, pairs [3F,2] int32, pinned [V] uint8, stats)`` of the mesh ``faces [F,3] int32`` over ``n_vertices``
    vertices (``tn_mesh_adjacency``): vertex ``v``'s row ``pairs[offsets[v]:offsets[v+1]]`` holds the other two corners
    ``(a, b)`` of every face that names ``v``, in the face's cyclic order, the faces ascending; ``pinned[v]`` is 1 for a vertex
    without faces, on an open boundary or on a non-manifold edge; ``stats = (participating faces, free vertices, largest degree)`` as
    ints, from one read-back.  A face with an index outside ``[0, n_vertices)`` or a repeated index takes no part; rows of ``pairs``
    from ``offsets[V]`` on are not written.  The same bytes on every call."""
    V = int(n_vertices)
    if faces.dim() != 2 or faces.size(1) != 3 or faces.dtype != torch.int32 or V < 0:
        raise ValueError("adjacency: faces must be [F,3] int32 and n_vertices >= 0")
    dev = L.require_cuda(faces)
    F = faces.size(0)
    nbytes = C.c_int64(0)
    L.call_plain("tn_mesh_adjacency_workspace_bytes", C.c_int64(V), C.c_int64(F), C.byref(nbytes))
    workspace = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    offsets = torch.zeros(V + 1, dtype=torch.int32, device=dev)    # (zeros: V == 0 launches nothing)
    pairs = torch.empty((max(3 * F, 1), 2), dtype=torch.int32, device=dev)[:3 * F]      # (a pointer even without faces)
    pinned = torch.empty(V, dtype=torch.uint8, device=dev)
    stats = torch.empty(3, dtype=torch.int64, device=dev)
    L.call("tn_mesh_adjacency", dev, L.ptr(faces) if F else None, C.c_int64(V), C.c_int64(F), L.ptr(offsets), L.ptr(pairs), L.ptr(pinned) if V else None,
           L.ptr(stats), L.ptr(workspace) if V else None)
    return offsets, pairs, pinned, tuple(stats.tolist())


def _adjacency_of(who, faces, V, adjacency_):
    offsets, pairs, pinned = adjacency(faces, V)[:3] if adjacency_ is None else tuple(adjacency_)[:3]
    if offsets.dtype != torch.int32 or offsets.numel() != V + 1 or pairs.dtype != torch.int32 or pinned.dtype != torch.uint8 or pinned.numel() != V:
        raise ValueError(f"{who}: adjacency must be mesh.adjacency's (offsets [V+1] int32, pairs [.,2] int32, pinned [V] uint8, ...)")
    return offsets, pairs, pinned


def smooth(vertices: torch.Tensor, faces: torch.Tensor, iterations: int, lam: float = 0.5, mu: float = -0.53, pin_boundary: bool = True,
           adjacency=None) -> torch.Tensor:
    """``vertices [V,3] float32`` after ``iterations`` Taubin iterations over the mesh ``faces`` (``tn_mesh_smooth``): each
    a pass ``p += lam (c - p)`` and a pass ``p += mu (c - p)``, ``c`` the mean of the vertex's row of ``adjacency`` -- the uniform
    umbrella operator; with ``mu < -lam < 0`` a low-pass filter that does not shrink the shape.  ``pin_boundary``: vertices on an open
    boundary or a non-manifold edge stay where they are (``pinned``); without it every vertex with a face moves.  ``adjacency``: what
    ``adjacency(faces, V)`` returned, to build it once for several calls.  ``iterations == 0`` returns ``vertices`` itself."""
    n = check_smooth("smooth", iterations, lam, mu)
    _check_mesh("smooth", vertices, faces)
    if n == 0:
        return vertices
    dev = L.require_cuda(vertices, faces)
    V = vertices.size(0)
    offsets, pairs, pinned = _adjacency_of("smooth", faces, V, adjacency)
    scratch, out = torch.empty_like(vertices), torch.empty_like(vertices)
    if V:
        L.call("tn_mesh_smooth", dev, L.ptr(vertices), L.ptr(offsets), L.ptr(pairs), L.ptr(pinned) if pin_boundary else None, C.c_int64(V),
               C.c_int32(n), C.c_float(lam), C.c_float(mu), L.ptr(scratch), L.ptr(out))
    return out


def vertex_normals(vertices: torch.Tensor, faces: torch.Tensor, fallback: Optional[torch.Tensor] = None, adjacency=None) -> torch.Tensor:
    """``[V,3] float32``: the unit normals of the mesh's vertices from its faces (``tn_mesh_vertex_normals``) -- the
    area-weighted sum of the normals of the faces around the vertex, normalised; faces counter-clockwise seen from outside give
    normals that point outside, as ``extract``'s do.  A vertex without faces or with a sum of length 0 or not finite takes its row of
    ``fallback``, or 0 without one."""
    _check_mesh("vertex_normals", vertices, faces, fallback=fallback)
    dev = L.require_cuda(vertices, faces, fallback)
    V = vertices.size(0)
    offsets, pairs, _ = _adjacency_of("vertex_normals", faces, V, adjacency)
    out = torch.empty_like(vertices)
    if V:
        L.call("tn_mesh_vertex_normals", dev, L.ptr(vertices), L.ptr(offsets), L.ptr(pairs), C.c_int64(V), L.ptr(fallback), L.ptr(out))
    return out


def smooth_mesh(vertices: torch.Tensor, normals: Optional[torch.Tensor], faces: torch.Tensor, iterations: int, lam: float = 0.5, mu: float = -0.53,
                pin_boundary: bool = True):
    """``(vertices, normals)``: ``smooth`` and then ``vertex_normals`` of the smoothed faces with the old ``normals`` as the fallback,
    over one ``adjacency``.  ``iterations == 0`` still recomputes the normals from the faces."""
    check_smooth("smooth_mesh", iterations, lam, mu)
    _check_mesh("smooth_mesh", vertices, faces, normals=normals)
    adj = adjacency(faces, vertices.size(0))
    moved = smooth(vertices, faces, iterations, lam=lam, mu=mu, pin_boundary=pin_boundary, adjacency=adj)
    return moved, vertex_normals(moved, faces, fallback=normals, adjacency=adj)


def _host(x, dtype) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x, dtype=dtype)


def write_mesh_ply(path, vertices, normals, colors, faces) -> None:
    """Binary little-endian PLY 1.0: ``element vertex V`` with float x y z, float nx ny nz, uchar red green blue (27 B each), then
    ``element face F`` with ``property list uchar int vertex_indices`` (a 3 and three int32: 13 B each).  Tensors or arrays."""
    xyz, nrm = _host(vertices, np.float32).reshape(-1, 3), _host(normals, np.float32).reshape(-1, 3)
    rgb, tri = _host(colors, np.uint8).reshape(-1, 3), _host(faces, np.int32).reshape(-1, 3)
    if not (xyz.shape[0] == nrm.shape[0] == rgb.shape[0]):
        raise ValueError("write_mesh_ply: vertices, normals and colors differ in length")
    vertex = np.empty(xyz.shape[0], dtype=MESH_VERTEX)
    for k, name in enumerate(("x", "y", "z")):
        vertex[name] = xyz[:, k]
    for k, name in enumerate(("nx", "ny", "nz")):
        vertex[name] = nrm[:, k]
    for k, name in enumerate(("red", "green", "blue")):
        vertex[name] = rgb[:, k]
    face = np.empty(tri.shape[0], dtype=MESH_FACE)
    face["n"] = 3
    for k, name in enumerate(("a", "b", "c")):
        face[name] = tri[:, k]
    with open(path, "wb") as f:
        f.write((_MESH_HEADER % (vertex.shape[0], face.shape[0])).encode("ascii"))
        f.write(vertex.tobytes())
        f.write(face.tobytes())


def read_mesh_ply(path):
    """``(vertices [V,3] float32, normals [V,3] float32, colors [V,3] uint8, faces [F,3] int32)`` as numpy arrays from a file in
    ``write_mesh_ply``'s dialect; any other header, a body of another length or a face that is not a triangle raises ``ValueError``"""
    with open(path, "rb") as f:
        raw = f.read()
    end = raw.find(b"end_header\n")
    if end < 0:
        raise ValueError(f"{path}: not a PLY file (no end_header)")
    head, body = raw[:end + 11].decode("ascii", errors="replace"), raw[end + 11:]
    lines = head.split("\n")
    try:
        n_v = int(lines[2].split()[2]) if lines[2].startswith("element vertex ") else -1
        n_f = int(lines[12].split()[2]) if lines[12].startswith("element face ") else -1
    except (IndexError, ValueError):
        n_v = n_f = -1
    if n_v < 0 or n_f < 0 or head != _MESH_HEADER % (n_v, n_f):
        raise ValueError(f"{path}: not the mesh PLY dialect (binary little-endian, float xyz + float normals + uchar rgb, triangle list)")
    if len(body) != MESH_VERTEX.itemsize * n_v + MESH_FACE.itemsize * n_f:
        raise ValueError(f"{path}: {len(body)} bytes of elements, the header promises {MESH_VERTEX.itemsize * n_v + MESH_FACE.itemsize * n_f}")
    vertex = np.frombuffer(body, dtype=MESH_VERTEX, count=n_v)
    face = np.frombuffer(body, dtype=MESH_FACE, count=n_f, offset=MESH_VERTEX.itemsize * n_v)
    if n_f and not (face["n"] == 3).all():
        raise ValueError(f"{path}: a face that is not a triangle")
    return (np.stack([vertex["x"], vertex["y"], vertex["z"]], 1), np.stack([vertex["nx"], vertex["ny"], vertex["nz"]], 1),
            np.stack([vertex["red"], vertex["green"], vertex["blue"]], 1), np.stack([face["a"], face["b"], face["c"]], 1))
