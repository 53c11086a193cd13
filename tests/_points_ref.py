"""The definition of tn_points_compact (include/tinynerf_hip.h) restated in numpy, without the kernel -- the yardstick of
tests/test_hip_points.py.

The predicate and the points use float64 products of the float32 inputs: depth * d is exact in float64 (24 x 24 significand bits),
so the float64 point is the exact value rounded once.  The colours are computed in float64 from the same float32 `1 - opacity` the
kernel forms."""
import numpy as np


def points64(rays_o, rays_d, depth):
    """[n,3] float64: o + depth d, the product exact, the sum rounded once"""
    with np.errstate(all="ignore"):
        return rays_o.astype(np.float64) + depth.astype(np.float64)[:, None] * rays_d.astype(np.float64)


def keep_mask(rays_o, rays_d, opacity, depth, box, min_opacity):
    """[n] bool.  A float64 point that is finite but beyond float32's range counts as overflowed: the kernel's fp32 point is inf."""
    p = points64(rays_o, rays_d, depth)
    f32max = float(np.finfo(np.float32).max)
    with np.errstate(all="ignore"):
        keep = opacity.astype(np.float64) >= float(np.float32(min_opacity))               # False for NaN
        keep &= (depth > 0) & np.isfinite(depth)
        keep &= (np.isfinite(p) & (np.abs(p) <= f32max)).all(1)
        if box is not None:
            b = np.asarray(box, np.float32).astype(np.float64)
            keep &= ((p >= b[:3]) & (p <= b[3:])).all(1)
    return keep


def colors64(rgb, opacity, bg):
    """(bytes [n,3] uint8, value [n,3] float64 = c * 255 + 0.5 before the truncation)"""
    t = (np.float32(1.0) - opacity.astype(np.float32)).astype(np.float64)                  # the float32 difference, as the kernel's
    bgv = np.zeros(3) if bg is None else np.asarray(bg, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        u = (rgb.astype(np.float64) - t[:, None] * bgv[None, :]) / opacity.astype(np.float64)[:, None]
        c = np.where(np.isnan(u), 0.0, np.clip(u, 0.0, 1.0))
        v = c * 255.0 + 0.5
    return np.floor(v).astype(np.uint8), v


def compact(rays_o, rays_d, rgb, opacity, depth, bg, box, min_opacity):
    """(src [M] int32, points [M,3] float64, colors [M,3] uint8, colour values [M,3] float64) of the kept rays, in ray order"""
    keep = keep_mask(rays_o, rays_d, opacity, depth, box, min_opacity)
    src = np.nonzero(keep)[0].astype(np.int32)
    col, val = colors64(rgb[src], opacity[src], bg)
    return src, points64(rays_o[src], rays_d[src], depth[src]), col, val


def ulp32(x):
    """spacing of float32 at |x| (x float64), at least the smallest normal's"""
    return np.spacing(np.maximum(np.abs(x), np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)
