"""Renderer core with the API of the reference's ``src/core.py``, backed by HIP kernels.

Same class names, constructor signatures and call conventions as the reference so that a
``train.py``-style harness can switch imports; every tensor operation goes through
``libtinynerf_hip.so`` (C ABI ``include/tinynerf_hip.h``) on the current HIP stream.  There is no
CPU path: CPU tensors raise ``RuntimeError`` exactly like the reference's ``CHECK_CUDA``.

Reference map: ContractionMip360/AABB core.py:11-31, RayMarcherUnbounded/AABB core.py:36-88,
OccupancyGrid core.py:93-156, RayProvider core.py:158-188, NerfWeights core.py:192-207,
NerfRenderer core.py:209-267.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from functools import cached_property
from typing import Any, Callable, List, Optional, Tuple

import torch

from . import _lib as L


def _f32c(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float32).contiguous()


_HOST_COPIES: dict = {}


def _host_floats(t: torch.Tensor) -> list:
    """Host copy of a small device tensor, cached per (storage, version): descriptors are rebuilt every step and a
    device -> host read here would drain the whole queue each time (measured: 2.6 ms per training step)."""
    key = (t.data_ptr(), t._version, str(t.device), tuple(t.shape), tuple(t.stride()))
    hit = _HOST_COPIES.get(key)
    if hit is None:
        if len(_HOST_COPIES) > 64:
            _HOST_COPIES.clear()
        vals = [float(v) for v in t.detach().to("cpu", torch.float32).reshape(-1).tolist()]
        _HOST_COPIES[key] = hit = (t, vals)        # the entry keeps the tensor alive: its address cannot be reused meanwhile
    return hit[1]


def _fill_aabb(desc: L.SamplerDesc, aabb: torch.Tensor) -> None:
    vals = _host_floats(aabb)
    for i in range(6):
        desc.aabb[i] = vals[i]


# --------------------------------------------------------------------------------------------
# contractions (reference core.py:11-31)
# --------------------------------------------------------------------------------------------
@dataclass
class ContractionMip360:
    order: float | int = float("inf")

    def _code(self) -> int:
        if math.isinf(float(self.order)):
            return L.CONTRACT_MIP360_INF
        if float(self.order) == 2.0:
            return L.CONTRACT_MIP360_L2
        raise NotImplementedError("ContractionMip360 supports order inf and 2")

    def _describe(self, desc: L.SamplerDesc) -> None:
        desc.contraction = self._code()

    @torch.no_grad()
    def __call__(self, coords: torch.Tensor) -> Tuple[torch.Tensor, None]:
        """Mip-NeRF 360 contraction, halved into [-1,1] (core.py:15-20)."""
        desc = L.SamplerDesc(n_samples=1)
        self._describe(desc)
        x = _f32c(coords)
        dev = L.require_cuda(x)
        out = torch.empty_like(x)
        L.call("tn_contract", dev, C.byref(desc), L.ptr(x), C.c_int64(x.numel() // 3), L.ptr(out), C.c_void_p(None))
        return out, None


@dataclass
class ContractionAABB:
    aabb: torch.Tensor  # [2,3]

    def _describe(self, desc: L.SamplerDesc) -> None:
        desc.contraction = L.CONTRACT_AABB
        _fill_aabb(desc, self.aabb)

    @torch.no_grad()
    def __call__(self, coords: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """Map the box to [-1,1]^3 and flag points inside it (core.py:26-31)."""
        desc = L.SamplerDesc(n_samples=1)
        self._describe(desc)
        x = _f32c(coords)
        dev = L.require_cuda(x)
        out = torch.empty_like(x)
        mask = torch.empty(x.shape[:-1], dtype=torch.uint8, device=dev)
        L.call("tn_contract", dev, C.byref(desc), L.ptr(x), C.c_int64(x.numel() // 3), L.ptr(out), L.ptr(mask))
        return out, mask.bool()


Contraction = ContractionMip360 | ContractionAABB


# --------------------------------------------------------------------------------------------
# ray marchers (reference core.py:36-88)
# --------------------------------------------------------------------------------------------
@dataclass
class RayMarcherUnbounded:
    n_samples: int = 200
    near: float = 0.
    far: float = 1e5
    uniform_range: float = 1.
    _tables: dict = field(default_factory=dict, repr=False, compare=False)

    @cached_property
    def step_size(self) -> float:
        return self.uniform_range / self.n_samples

    def _table(self, device: torch.device) -> Tuple[torch.Tensor, torch.Tensor]:
        """t[S], delta[S] of core.py:52-55.  The table is built once per device with
        torch.linspace (a torch primitive whose rounding the reference inherits as well)."""
        key = str(device)
        if key not in self._tables:
            S = self.n_samples
            u = torch.linspace(0., 1. - (1. / (S + 2)), S + 1, device=device)
            fu = torch.where(u < 0.5, 2 * u, 1 / (2 - 2 * u))
            t = fu * self.uniform_range + self.near
            self._tables[key] = (t[:-1].contiguous(), (t[1:] - t[:-1]).contiguous())
        return self._tables[key]

    def _describe(self, desc: L.SamplerDesc, device: torch.device) -> None:
        t, dl = self._table(device)
        desc.marcher = L.MARCH_UNBOUNDED
        desc.n_samples = self.n_samples
        desc.t_table = t.data_ptr()
        desc.delta_table = dl.data_ptr()

    @torch.no_grad()
    def __call__(self, rays_o: torch.Tensor, rays_d: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        dev = L.require_cuda(_f32c(rays_o))
        t, dl = self._table(dev)
        n = rays_o.size(0)
        return torch.broadcast_to(t, (n, self.n_samples)), torch.broadcast_to(dl, (n, self.n_samples))


@dataclass
class RayMarcherAABB:
    aabb: torch.Tensor
    n_samples: int = 200
    near: float = 0.
    far: float = 1e5

    @cached_property
    def step_size(self) -> torch.Tensor:
        # 0-dim fp32 tensor like the reference (core.py:68-70)
        return torch.norm(self.aabb[1] - self.aabb[0]) / self.n_samples

    def _describe(self, desc: L.SamplerDesc, device: torch.device) -> None:
        desc.marcher = L.MARCH_AABB
        desc.n_samples = self.n_samples
        desc.near = self.near
        desc.far = self.far
        desc.step_size = _host_floats(self.step_size)[0]
        _fill_aabb(desc, self.aabb)

    @torch.no_grad()
    def __call__(self, rays_o: torch.Tensor, rays_d: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        o, d = _f32c(rays_o), _f32c(rays_d)
        dev = L.require_cuda(o, d)
        desc = L.SamplerDesc()
        self._describe(desc, dev)
        n = o.size(0)
        t = torch.empty((n, self.n_samples), device=dev)
        dl = torch.empty_like(t)
        L.call("tn_march_rays", dev, C.byref(desc), L.ptr(o), L.ptr(d), C.c_int64(n), L.ptr(t), L.ptr(dl))
        return t, dl


RayMarcher = RayMarcherUnbounded | RayMarcherAABB


# --------------------------------------------------------------------------------------------
# occupancy grid (reference core.py:93-156)
# --------------------------------------------------------------------------------------------
class OccupancyGrid(torch.nn.Module):
    def __init__(
        self,
        size: List[int] | int,  # [depth, height, width]
        step_size: float,
        threshold: float = 0.01,
        decay: float = 0.95,
    ):
        super().__init__()
        size = list(size) if isinstance(size, (list, tuple)) else [size, size, size]
        self.decay = decay
        self.step_size = step_size
        self.base_threshold = threshold
        self.grid: torch.Tensor
        self.register_buffer("grid", torch.ones(size, dtype=torch.float))
        self.size = torch.tensor(size, dtype=torch.float)
        self.mean = 1.
        self._dims = tuple(int(s) for s in size)
        self._n_updates = 0
        self.use_coarse = True     # sampler early reject through block maxima (identical masks; False: every candidate reads its taps)

    @property
    def threshold(self) -> float:
        return min(self.base_threshold, self.mean)

    @property
    def device(self) -> torch.device:
        return self.grid.device

    def coarse_maxima(self) -> torch.Tensor:
        """Block maxima for the sampler's conservative early reject (tn_occupancy_coarsen), rebuilt whenever the grid has
        changed: through ``update`` (tracked here) or through in-place torch ops on ``grid`` (its version counter)."""
        key = (self.grid.data_ptr(), self.grid._version, self._n_updates)
        if getattr(self, "_coarse_key", None) != key:
            D, H, W = self._dims
            dev = L.require_cuda(self.grid)
            self._coarse = torch.empty(((D + 3) // 4, (H + 3) // 4, (W + 3) // 4), device=dev)
            L.call("tn_occupancy_coarsen", dev, L.ptr(self.grid), C.c_int(D), C.c_int(H), C.c_int(W), L.ptr(self._coarse))
            self._coarse_key = key
        return self._coarse

    def _stats_device(self) -> torch.Tensor:
        """[sum of cells, cells above the threshold] as a device tensor (no host sync)"""
        dev = L.require_cuda(self.grid)
        stats = torch.empty(2, dtype=torch.float64, device=dev)
        L.call("tn_occupancy_stats", dev, L.ptr(self.grid), C.c_int64(self.grid.numel()),
               C.c_float(self.threshold), L.ptr(stats))
        return stats

    def _stats(self) -> Tuple[float, float]:
        s, c = self._stats_device().tolist()
        return s, c

    @torch.no_grad()
    def occupancy(self) -> float:
        """Fraction of cells above the threshold (core.py:121-123)."""
        return self._stats()[1] / self.grid.numel()

    @torch.no_grad()
    def update(self, sigma_fn: Callable[[torch.Tensor], torch.Tensor], jitters: Optional[torch.Tensor] = None,
               slices_per_call: Optional[int] = None, seed: Optional[int] = None):
        """Decay/refresh sweep of core.py:133-145.

        Voxel centres are jittered on the device by a counter-based RNG seeded from torch's
        generator, or from ``seed`` when given (``jitters`` [D,H,W,3] overrides it for parity runs).  The threshold is constant
        during a sweep, so slices are independent: ``slices_per_call`` of them are evaluated by one
        ``sigma_fn`` call (default: as many as give <= 2^21 points) instead of one call per slice.
        """
        D, H, W = self._dims
        dev = L.require_cuda(self.grid)
        thr = float(self.threshold)
        step = float(self.step_size)
        seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else int(seed)
        per = slices_per_call or max(1, min(D, (1 << 21) // (H * W)))
        coords = torch.empty((per * H * W, 3), device=dev)
        for i0 in range(0, D, per):
            n_sl = min(per, D - i0)
            for j in range(n_sl):
                jit = None if jitters is None else _f32c(jitters[i0 + j]).to(dev)
                L.call("tn_occupancy_slice_coords", dev, C.c_int(D), C.c_int(H), C.c_int(W), C.c_int(i0 + j),
                       L.ptr(jit), C.c_uint64(seed), C.c_void_p(coords.data_ptr() + j * H * W * 12))
            pts = coords[: n_sl * H * W]
            sig = _f32c(sigma_fn(pts).detach().reshape(-1))
            cells = self.grid[i0:i0 + n_sl]
            L.call("tn_occupancy_apply", dev, L.ptr(cells), L.ptr(sig), C.c_int64(n_sl * H * W),
                   C.c_float(step), C.c_float(thr), C.c_float(self.decay))
        self._n_updates += 1                       # the kernels write through raw pointers: no version bump
        self.mean = self._stats()[0] / self.grid.numel()

    @torch.no_grad()
    def forward(self, coords: torch.Tensor) -> torch.Tensor:
        """coords [...,3] in [-1,1] -> bool, trilinear lookup > threshold (core.py:147-156)."""
        x = _f32c(coords)
        dev = L.require_cuda(x, self.grid)
        D, H, W = self._dims
        out = torch.empty(x.shape[:-1], dtype=torch.uint8, device=dev)
        L.call("tn_occupancy_query", dev, L.ptr(self.grid), C.c_int(D), C.c_int(H), C.c_int(W), L.ptr(x),
               C.c_int64(x.numel() // 3), C.c_float(self.threshold), L.ptr(out), C.c_void_p(None))
        return out.bool()


# --------------------------------------------------------------------------------------------
# sample packing (reference core.py:158-188)
# --------------------------------------------------------------------------------------------
@dataclass
class RayProvider:
    occupancy_grid: OccupancyGrid
    contraction: Contraction
    ray_marcher: RayMarcher

    def _desc(self, device: torch.device, training: bool, jitter: Optional[torch.Tensor]) -> L.SamplerDesc:
        desc = L.SamplerDesc()
        self.ray_marcher._describe(desc, device)
        self.contraction._describe(desc)
        g = self.occupancy_grid
        desc.grid_d, desc.grid_h, desc.grid_w = g._dims
        desc.grid = g.grid.data_ptr()
        desc.threshold = float(g.threshold)
        desc.coarse = g.coarse_maxima().data_ptr() if g.use_coarse else None
        if jitter is not None:
            desc.jitter = jitter.data_ptr()
        elif training:
            desc.use_rng = 1
            desc.seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        return desc

    @torch.no_grad()
    def __call__(self, rays_o: torch.Tensor, rays_d: torch.Tensor, training: bool,
                 jitter: Optional[torch.Tensor] = None, return_ray_ids: bool = False, return_t: bool = False):
        """packed_samples [N,7] = (contracted xyz, ray dir, step), packing_info [R,2] int32 =
        (start,count) -- core.py:165-188.  ``jitter`` ([R,S] U[0,1)) replaces the device RNG that
        stands in for ``torch.rand_like`` when ``training`` (parity runs).

        Returns ``(packed, info)``, then ``ray_ids [N] int32`` if ``return_ray_ids``, then ``t [N]`` if ``return_t``:
        the ray parameter each sample was taken at, jitter included (a distance: rays are unit length), for
        ``NerfRenderer.render_maps``."""
        o, d = _f32c(rays_o), _f32c(rays_d)
        dev = L.require_cuda(o, d, self.occupancy_grid.grid)
        R = o.size(0)
        S = self.ray_marcher.n_samples
        if jitter is not None:
            jitter = _f32c(jitter)
            L.require_cuda(jitter)
        desc = self._desc(dev, training, jitter)
        n_chunks = (S + 63) // 64
        maskbits = torch.empty((R, n_chunks), dtype=torch.int64, device=dev)
        counts = torch.empty(R, dtype=torch.int32, device=dev)
        info = torch.empty((R, 2), dtype=torch.int32, device=dev)
        total = torch.zeros(1, dtype=torch.int32, device=dev)
        L.call("tn_sample_mask", dev, C.byref(desc), L.ptr(o), L.ptr(d), C.c_int64(R), L.ptr(maskbits), L.ptr(counts))
        L.call("tn_sample_scan", dev, L.ptr(counts), C.c_int64(R), C.c_void_p(None), L.ptr(info), L.ptr(total))
        n = int(total.item())                      # the one host sync: the output shape
        packed = torch.empty((n, 7), device=dev)
        ray_ids = torch.empty(n, dtype=torch.int32, device=dev) if return_ray_ids else None
        t = torch.empty(n, device=dev) if return_t else None
        L.call("tn_sample_pack_t", dev, C.byref(desc), L.ptr(o), L.ptr(d), C.c_int64(R), L.ptr(maskbits), L.ptr(info),
               C.c_void_p(None), L.ptr(packed), L.ptr(ray_ids), C.c_void_p(None), L.ptr(t), C.c_int64(n))
        out = (packed, info) + ((ray_ids,) if return_ray_ids else ()) + ((t,) if return_t else ())
        return out


# --------------------------------------------------------------------------------------------
# rendering (reference core.py:192-267)
# --------------------------------------------------------------------------------------------
def _check_info(info: torch.Tensor) -> None:
    if info.dtype != torch.int32 or info.dim() != 2 or info.size(1) != 2:
        raise RuntimeError("packing_info must be an int32 tensor of shape [n_rays, 2]")


class NerfWeights(torch.autograd.Function):
    """w_k = T_k (1 - exp(-sigma_k delta_k)) with early termination (core.py:192-207, cuda.cu:3-58)."""

    @staticmethod
    def forward(ctx: Any, sigmas: torch.Tensor, steps: torch.Tensor, info: torch.Tensor, threshold: float) -> torch.Tensor:  # type: ignore
        sigmas = sigmas.contiguous()
        steps = steps.contiguous()
        info = info.contiguous()
        if sigmas.dim() != 1 or steps.dim() != 1:
            raise RuntimeError("sigmas and steps must be 1-D")
        _check_info(info)
        dev = L.require_cuda(sigmas, steps, info)
        weights = torch.zeros_like(sigmas)       # cuda.cu:84: samples no (start, count) covers keep weight 0
        L.call("tn_weights_fwd", dev, L.ptr(sigmas), L.ptr(steps), L.ptr(info), C.c_float(threshold), L.ptr(weights),
               C.c_int64(sigmas.numel()), C.c_int64(info.size(0)))
        ctx.save_for_backward(sigmas, steps, info, weights)
        return weights

    @staticmethod
    def backward(ctx: Any, grad_weights: torch.Tensor):  # type: ignore
        grad_weights = grad_weights.contiguous()
        sigmas, steps, info, weights = ctx.saved_tensors
        dev = L.require_cuda(grad_weights)
        grad_sigmas = torch.zeros_like(sigmas)
        L.call("tn_weights_bwd", dev, L.ptr(sigmas), L.ptr(steps), L.ptr(info), L.ptr(weights), L.ptr(grad_weights),
               L.ptr(grad_sigmas), C.c_int64(sigmas.numel()), C.c_int64(info.size(0)))
        return grad_sigmas, None, None, None


class _Composite(torch.autograd.Function):
    """rendered[r] = sum_k w_k rgb_k (+ bg (1 - sum_k w_k)) -- core.py:256-265 as one kernel."""

    @staticmethod
    def forward(ctx: Any, rgbs: torch.Tensor, weights: torch.Tensor, info: torch.Tensor, bg: Optional[torch.Tensor]):  # type: ignore
        rgbs, weights, info = rgbs.contiguous(), weights.contiguous(), info.contiguous()
        dev = L.require_cuda(rgbs, weights, info)
        R = info.size(0)
        out = torch.empty((R, 3), device=dev)
        L.call("tn_composite_fwd", dev, L.ptr(rgbs), L.ptr(weights), L.ptr(info), L.ptr(bg), L.ptr(out), C.c_void_p(None),
               C.c_int64(weights.numel()), C.c_int64(R))
        ctx.save_for_backward(rgbs, weights, info, bg)
        return out

    @staticmethod
    def backward(ctx: Any, grad_out: torch.Tensor):  # type: ignore
        rgbs, weights, info, bg = ctx.saved_tensors
        grad_out = grad_out.contiguous()
        dev = grad_out.device
        g_rgb = torch.zeros_like(rgbs) if ctx.needs_input_grad[0] else None
        g_w = torch.zeros_like(weights) if ctx.needs_input_grad[1] else None
        L.call("tn_composite_bwd", dev, L.ptr(rgbs), L.ptr(weights), L.ptr(info), L.ptr(bg), L.ptr(grad_out),
               L.ptr(g_rgb), L.ptr(g_w), C.c_int64(weights.numel()), C.c_int64(info.size(0)))
        return g_rgb, g_w, None, None


def distortion_warp(ray_marcher: RayMarcher) -> Tuple[int, float, float]:
    """``(warp, near, range)`` of ``RayDistortion`` / ``NerfRenderer.distortion_warp`` for a marcher: the AABB marcher's samples are
    uniform in t, normalised by the box diagonal (= n_samples * step_size, so a ray spans at most 1); the unbounded marcher's are
    uniform in u = g((t - near) / uniform_range), the inverse of its table (core.py:52), and the loss is taken in u."""
    if isinstance(ray_marcher, RayMarcherUnbounded):
        return L.DIST_UNBOUNDED, float(ray_marcher.near), float(ray_marcher.uniform_range)
    if isinstance(ray_marcher, RayMarcherAABB):
        return L.DIST_LINEAR, 0.0, float(_host_floats(ray_marcher.step_size)[0]) * ray_marcher.n_samples
    raise TypeError(f"no distortion warp for {type(ray_marcher).__name__}")


def _check_warp(warp: int, range_: float) -> None:
    if warp not in (L.DIST_LINEAR, L.DIST_UNBOUNDED) or not range_ > 0:
        raise ValueError("distortion warp must be (DIST_LINEAR | DIST_UNBOUNDED, near, range > 0)")


class RayDistortion(torch.autograd.Function):
    """Per-ray distortion loss of Mip-NeRF 360, ``L_r = sum_ij w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 d_i`` (``tn_distortion_fwd``):
    ``weights, t, steps [N]``, ``info [R,2]`` -> ``[R]``.  ``t`` is the ray parameter of every packed sample
    (``RayProvider(..., return_t=True)``), ``(warp, near, range)`` come from ``distortion_warp(marcher)``.  Differentiable in
    ``weights`` only: ``t`` and ``steps`` are sampler outputs."""

    @staticmethod
    def forward(ctx: Any, weights: torch.Tensor, t: torch.Tensor, steps: torch.Tensor, info: torch.Tensor, warp: int, near: float,
                range_: float) -> torch.Tensor:  # type: ignore
        weights, t, steps, info = _f32c(weights), _f32c(t), _f32c(steps), info.contiguous()
        _check_info(info)
        _check_warp(warp, range_)
        if not (weights.dim() == t.dim() == steps.dim() == 1 and weights.size(0) == t.size(0) == steps.size(0)):
            raise RuntimeError("weights, t and steps must be 1-D and hold one value per packed sample")
        dev = L.require_cuda(weights, t, steps, info)
        R = info.size(0)
        loss = torch.zeros(R, device=dev)
        if weights.numel() > 0:
            L.call("tn_distortion_fwd", dev, L.ptr(weights), L.ptr(t), L.ptr(steps), L.ptr(info), C.c_int64(R), C.c_int32(warp),
                   C.c_float(near), C.c_float(range_), L.ptr(loss), C.c_void_p(None))
        ctx.save_for_backward(weights, t, steps, info)
        ctx.warp = (warp, near, range_)
        return loss

    @staticmethod
    def backward(ctx: Any, grad_loss: torch.Tensor):  # type: ignore
        weights, t, steps, info = ctx.saved_tensors
        warp, near, range_ = ctx.warp
        grad_loss = _f32c(grad_loss)
        g_w = torch.zeros_like(weights)          # samples no ray owns keep gradient 0
        if weights.numel() > 0:
            L.call("tn_distortion_bwd", weights.device, L.ptr(weights), L.ptr(t), L.ptr(steps), L.ptr(info), C.c_int64(info.size(0)),
                   C.c_int32(warp), C.c_float(near), C.c_float(range_), L.ptr(grad_loss), C.c_float(1.0), C.c_void_p(None), L.ptr(g_w))
        return g_w, None, None, None, None, None, None


def normal_frame(contraction: Optional[Contraction]) -> L.NormalFrame:
    """``tn_normal_frame`` of a contraction (``None``: the none frame, J = I) for ``sample_normals`` / ``NerfRenderer.normal_frame``"""
    frame = L.NormalFrame(contraction=L.CONTRACT_NONE)
    if contraction is None:
        return frame
    if isinstance(contraction, ContractionMip360):
        frame.contraction = contraction._code()
    elif isinstance(contraction, ContractionAABB):
        frame.contraction = L.CONTRACT_AABB
        vals = _host_floats(contraction.aabb)
        for i in range(6):
            frame.aabb[i] = vals[i]
    else:
        raise TypeError(f"no normal frame for {type(contraction).__name__}")
    return frame


@torch.no_grad()
def sample_normals(renderer: "NerfRenderer", packed: torch.Tensor, gate: Optional[torch.Tensor] = None, return_grad: bool = False):
    """Unit world-frame surface normals ``[n,3]`` of packed samples (columns 0..2 of ``packed`` [n, >= 3]: the contracted position): the
    negated, normalised gradient of the density with respect to the position, analytically through the field and the sigma head
    (``tn_kplanes_normals`` / ``tn_hashgrid_normals``), taken to the world frame by ``renderer.normal_frame``.  ``gate`` [n]
    (the renderer passes the weights): rows whose gate is 0 get zeros.  ``return_grad``: ``(normals, grad)`` with ``grad`` [n,3] the
    gradient of the head's pre-activation in the contracted frame.  Inference only; K-Planes and hash-grid fields in front of a
    ``VanillaOpacityDecoder`` -- anything else raises ``NotImplementedError``."""
    from . import models as M
    fm, sd = renderer.feature_module, renderer.sigma_decoder
    if not isinstance(fm, (M.KPlanesFeatureField, M.HashGridFeatureField)):
        raise NotImplementedError(f"sample_normals: no analytic density gradient through {type(fm).__name__} (K-Planes and hash-grid fields only: "
                                  "the 10-layer Vanilla and Cobafa stacks are not differentiated with respect to position)")
    if not isinstance(sd, M.VanillaOpacityDecoder):
        raise NotImplementedError(f"sample_normals: the sigma decoder must be a VanillaOpacityDecoder, not {type(sd).__name__}")
    params = sd.net.params()
    F = int(fm.feature_dim)
    if len(params) != 4 or tuple(params[0].shape) != (64, F) or tuple(params[2].shape) != (1, 64):
        raise NotImplementedError(f"sample_normals: the sigma head must be {F} -> 64 -> 1")
    if packed.dim() != 2 or packed.size(1) < 3:
        raise RuntimeError("sample_normals: packed must be [n, >= 3] (contracted xyz first)")
    x = packed if packed.dtype == torch.float32 else packed.float()
    if x.stride(1) != 1 or (x.size(0) > 1 and x.stride(0) < 3):
        x = x.contiguous()
    n = x.size(0)
    tensors = [x] + [p.detach() for p in params]
    if gate is not None:
        gate = _f32c(gate.detach()).reshape(-1)
        if gate.numel() != n:
            raise RuntimeError("sample_normals: gate must hold one value per sample")
        tensors.append(gate)
    dev = x.device
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError("tinynerf_amd: tensor must be a CUDA (HIP) tensor -- there is no CPU path")
    normals = torch.empty((n, 3), device=dev)
    grad = torch.empty((n, 3), device=dev) if return_grad else None
    if n > 0:
        head = M._mlp_desc([p.detach() for p in params], F, L.ENC_NONE, 0, L.ACT_EXP_M1, None)
        frame = renderer.normal_frame if renderer.normal_frame is not None else L.NormalFrame(contraction=L.CONTRACT_NONE)
        stride = x.stride(0) if n > 1 else x.size(1)
        if isinstance(fm, M.KPlanesFeatureField):
            desc, keep = M._kplanes_desc([p.detach() for p in fm.plane_tensors()])
            name = "tn_kplanes_normals"
        else:
            table = fm.table.detach()
            if not table.is_contiguous() or table.dtype != torch.float32:
                raise RuntimeError("tinynerf_amd: the hash grid's table must be a contiguous fp32 tensor")
            desc, keep = M._hashgrid_desc(fm.plan, table.size(1), table), [table]
            name = "tn_hashgrid_normals"
        L.call(name, dev, C.byref(desc), L.ptr(x), C.c_int64(stride), C.c_int64(n), C.byref(head), C.byref(frame), L.ptr(gate),
               L.ptr(normals), L.ptr(grad))
        del keep
    return (normals, grad) if return_grad else normals


@torch.no_grad()
def ray_normals(weights: torch.Tensor, normals: torch.Tensor, packing_info: torch.Tensor) -> torch.Tensor:
    """``[R,3]``: the weighted sum of every ray's sample normals, normalised (0 where it vanishes or the ray is empty) -- ``tn_ray_normals``"""
    _check_info(packing_info)
    R = packing_info.size(0)
    out = torch.zeros((R, 3), device=packing_info.device)
    if R > 0 and weights.numel() > 0:
        w, nrm, info = _f32c(weights.detach()), _f32c(normals), packing_info.contiguous()
        dev = L.require_cuda(w, nrm, info)
        L.call("tn_ray_normals", dev, L.ptr(w), L.ptr(nrm), L.ptr(info), C.c_int64(R), L.ptr(out))
    return out


class NerfRenderer(torch.nn.Module):
    def __init__(
        self,
        feature_module: torch.nn.Module,
        sigma_decoder: torch.nn.Module,
        rgb_decoder: torch.nn.Module,
        bg_color: torch.Tensor | None = None,
    ):
        super().__init__()
        self.feature_module = feature_module
        self.sigma_decoder = sigma_decoder
        self.rgb_decoder = rgb_decoder
        self.bg_color = bg_color
        # K-Planes + Vanilla decoders are rendered by one fused autograd node (tinynerf_amd/fused.py);
        # set to False for the module-by-module path that mirrors the reference's data flow
        self.fused = True
        self.accumulate_into_grad = False      # harness option: add parameter grads straight into param.grad
        self.reuse_buffers = False             # harness option: capacity-based scratch arena (fused.Arena)
        # render_with_distortion: (warp, near, range) of the marcher that made the samples (distortion_warp(marcher)); the trainer sets it
        self.distortion_warp: Optional[Tuple[int, float, float]] = None
        # render_maps(normals=True) / sample_normals: the frame of the contraction that made the samples (normal_frame(contraction));
        # None = no contraction.  The trainer sets it.
        self.normal_frame: Optional[L.NormalFrame] = None
        assert hasattr(self.feature_module, "feature_dim"), "feature module requires a feature_dim attribute"

    def _bg(self, device: torch.device) -> Optional[torch.Tensor]:
        if self.bg_color is None:
            return None
        if self.bg_color.device != device or self.bg_color.dtype != torch.float32:
            self.bg_color = self.bg_color.to(device, torch.float32)
        return self.bg_color.contiguous()

    def forward(
        self,
        packed_samples: torch.Tensor,  # [n_samples, 7]
        packing_info: torch.Tensor,  # [n_rays, 2]
        early_termination_threshold: float = 1e-4,
    ) -> torch.Tensor:
        """Module-by-module renderer of core.py:225-267: features -> sigma -> weights -> colour of
        the samples with w > 0 -> per-ray composite.  Each stage is a HIP launch; the fully fused
        K-Planes path lives in ``tinynerf_amd.fused``."""
        return self._render(packed_samples, packing_info, early_termination_threshold, None)

    def _render(self, packed_samples: torch.Tensor, packing_info: torch.Tensor, early_termination_threshold: float, dist: Optional[dict]):
        """``forward``; with ``dist`` (render_with_distortion: t and the warp) -> (rgb, per-ray distortion of the weights it composited with)"""
        device = packed_samples.device
        n_samples = packed_samples.size(0)
        n_rays = packing_info.size(0)
        _check_info(packing_info)
        bg = self._bg(device)
        if self.fused and n_samples > 0 and n_rays > 0:
            from . import fused
            if fused.supports(self):
                return fused.render(self, packed_samples, packing_info, early_termination_threshold, self.accumulate_into_grad, dist)
        empty = n_samples == 0
        if not empty:
            feats = self.feature_module(packed_samples[:, :3])
            sigmas = self.sigma_decoder(feats).ravel()
            weights: torch.Tensor = NerfWeights.apply(sigmas, packed_samples[:, 6], packing_info, early_termination_threshold)  # type: ignore
            active = torch.nonzero(weights > 0.).squeeze(1)       # host sync, like `mask.any()` in the reference
            empty = active.numel() == 0
            self.__dict__.setdefault("_stats", {}).update(gate=weights.detach().amax().reshape(1), pre_gated=False)
        if empty:
            # core.py:251-254: every sample masked -> background only, gradients are zero
            print("Empty iteration, every sample is masked")
            self.__dict__.setdefault("_stats", {}).update(gate=torch.zeros(1, device=device), pre_gated=False)
            rgbs = torch.zeros((n_samples, 3), device=device, requires_grad=True)
            weights = torch.zeros(n_samples, device=device, requires_grad=True)
        else:
            if active.numel() == n_samples:                 # nothing masked: the gather / scatter pair is the identity
                rgbs = self.rgb_decoder(feats, packed_samples[:, 3:6].contiguous())
            else:
                rgb_active = self.rgb_decoder(feats[active], packed_samples[:, 3:6][active])
                rgbs = torch.zeros((n_samples, 3), device=device).index_copy(0, active, rgb_active)
        handout = self.__dict__.get("_stats", {}).get("maps_handout")
        if handout is not None:             # render_maps: the weights this forward composites with
            handout["weights"] = weights
        if n_rays == 0:
            rendered = torch.zeros((0, 3), device=device)
        else:
            rendered = _Composite.apply(rgbs, weights, packing_info.contiguous(), bg)
        if dist is None:
            return rendered
        if n_rays == 0 or n_samples == 0:
            return rendered, torch.zeros(n_rays, device=device)
        return rendered, RayDistortion.apply(weights, dist["t"], packed_samples[:, 6], packing_info, *dist["warp"])

    def render_with_distortion(
        self,
        packed_samples: torch.Tensor,  # [n_samples, 7]
        packing_info: torch.Tensor,  # [n_rays, 2]
        t: torch.Tensor,  # [n_samples], RayProvider(..., return_t=True)
        early_termination_threshold: float = 1e-4,
    ) -> Tuple[torch.Tensor, torch.Tensor]:
        """``forward``'s colour (the same bits) and the per-ray distortion loss ``[R]`` of the weights it composited with
        (``RayDistortion``), both differentiable.  Same dispatch as ``forward``: on the module-by-module path the loss hangs on the
        weights ``NerfWeights`` returned; the fused nodes hand it out as a second output whose gradient joins the composite's in
        front of the weights backward (``tn_distortion_bwd`` -> ``tn_render_rays_bwd_dw``).  The warp is ``self.distortion_warp``
        (``distortion_warp(marcher)``; ``(DIST_LINEAR, 0, 1)`` when unset: t as it is)."""
        if t.dim() != 1 or t.size(0) != packed_samples.size(0):
            raise RuntimeError("t must hold one value per packed sample (RayProvider(..., return_t=True))")
        warp, near, range_ = self.distortion_warp if self.distortion_warp is not None else (L.DIST_LINEAR, 0.0, 1.0)
        _check_warp(warp, range_)
        return self._render(packed_samples, packing_info, early_termination_threshold,
                            {"t": _f32c(t), "warp": (int(warp), float(near), float(range_))})

    @torch.no_grad()
    def _maps(self, weights: torch.Tensor, packing_info: torch.Tensor, t: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        R = packing_info.size(0)
        dev = packing_info.device
        opacity, depth, median = (torch.zeros(R, device=dev) for _ in range(3))
        if R > 0 and weights.numel() > 0:
            w, info, t = _f32c(weights), packing_info.contiguous(), _f32c(t)
            L.require_cuda(w, info, t)
            L.call("tn_ray_maps", dev, L.ptr(w), L.ptr(t), L.ptr(info), C.c_int64(R), L.ptr(opacity), L.ptr(depth), L.ptr(median))
        return opacity, depth, median

    def render_maps(
        self,
        packed_samples: torch.Tensor,  # [n_samples, 7]
        packing_info: torch.Tensor,  # [n_rays, 2]
        t: torch.Tensor,  # [n_samples], RayProvider(..., return_t=True)
        early_termination_threshold: float = 1e-4,
        normals: bool = False,
    ) -> dict:
        """Inference: ``forward``'s colour plus per-ray maps of the weights it composited with, as a dict of
        ``rgb [R,3]`` (bit-identical to ``forward``), ``opacity [R]`` (sum of the weights), ``depth [R]`` (expected
        depth given a hit: sum w t / opacity) and ``median_depth [R]`` (t where the weights' prefix reaches half the
        opacity); rays with opacity 0 get depth 0.  Same dispatch as ``forward`` (fused nodes or the module path);
        the weights are handed out by that forward, not recomputed (``tn_ray_maps``).  The maps carry no gradient:
        call it under ``torch.no_grad()`` when parameters require grad.  ``normals``: the dict also holds ``normal [R,3]``, the
        normalised weighted sum of the samples' surface normals (``sample_normals`` gated by the handed-out weights, then
        ``tn_ray_normals``; 0 for rays with opacity 0) -- a pass after the forward; every other entry keeps its bits."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise RuntimeError("NerfRenderer.render_maps is inference only: call it under torch.no_grad()")
        if t.dim() != 1 or t.size(0) != packed_samples.size(0):
            raise RuntimeError("t must hold one value per packed sample (RayProvider(..., return_t=True))")
        stats = self.__dict__.setdefault("_stats", {})
        handout: dict = {}
        stats["maps_handout"] = handout
        try:
            rgb = self.forward(packed_samples, packing_info, early_termination_threshold)
        finally:
            stats.pop("maps_handout", None)
        weights = handout.get("weights")
        if weights is None:
            weights = torch.zeros(0, device=packed_samples.device)
        opacity, depth, median = self._maps(weights.detach(), packing_info, t)
        out = {"rgb": rgb, "opacity": opacity, "depth": depth, "median_depth": median}
        if normals:
            if weights.numel() > 0:
                out["normal"] = ray_normals(weights, sample_normals(self, packed_samples, gate=weights), packing_info)
            else:
                sample_normals(self, packed_samples[:0])          # (still says so when the field has no normals)
                out["normal"] = torch.zeros((packing_info.size(0), 3), device=packed_samples.device)
        return out
