"""The yardstick of the TSDF colour fusion: tn_tsdf_integrate_color and tn_tsdf_sample_colors as include/tinynerf_hip.h
defines them, restated in numpy without the kernels -- float64 arithmetic on the float32 inputs, steps 1-5 of the per-view update
from tests/_tsdf_ref.py (`project`, `nodes`; the margins to the decision edges are `_tsdf_ref.integrate`'s).  Besides the results
both functions return what the tests' bounds are made of; the bounds themselves are derived in tests/test_hip_tsdf_color.py."""
import numpy as np

import _tsdf_ref as ref
from _tsdf_ref import nodes, project

E = 2.0 ** -24                                                     # the relative error of one float32 rounding
SECOND = 1.0 + 2.0 ** -20                                          # products of two such errors, which the first-order bounds leave out


def uncomposite(rgb, op, bg):
    """the expected colour given a hit, the background taken out again: (rgb - (1 - op) bg) / op clamped to [0, 1] with NaN -> 0, and
    the unclamped value; rgb [n,3], op [n], bg [3], float64"""
    with np.errstate(all="ignore"):
        raw = (rgb - (1.0 - op)[:, None] * bg[None, :]) / op[:, None]
        return np.where(raw > 0, np.minimum(raw, 1.0), 0.0), raw


def integrate_color(dims, lo, h, c2w, models, lenses, sizes, depth, opacity, min_opacity, rgb, bg, trunc, views=None, state=None,
                    margins=False):
    """dims (nx, ny, nz); the table, depth, opacity (or None), min_opacity and trunc as `_tsdf_ref.integrate` takes them; rgb
    [n_pixels,3] float32; bg [3] or None (zeros); views = (first, count); state = C [nodes,4] of an earlier call.  Returns a dict:
    C float64 [nodes,4] = sum w r, sum w g, sum w b, sum w; and per node what the bound is made of, summed over the views that pass
    step 5 with |sdf| <= trunc + 2^-22 |p| (the contributing views, and those the float32 sdf may still put inside the band):
      n_views   their number
      dw        sum of 2^-22 |p| / trunc + 2^-23: the error of a view's weight
      dterm     [nodes,3] sum of dw_view u_c + (w + dw_view) 2^-24 ((1 - op) |bg_c| / op + 2 |u_raw|): the error of w u_c
      sum_w, sum_wu [nodes,3]: the sums of the terms' magnitudes.
    With `margins`, the margin_* entries of `_tsdf_ref.integrate` on the same inputs are added."""
    x = nodes(dims, lo, h)
    n = x.shape[0]
    sizes = np.asarray(sizes, np.int64).reshape(-1, 2)
    offsets = np.concatenate([[0], np.cumsum(sizes[:, 0] * sizes[:, 1])])
    depth32 = np.ascontiguousarray(depth, np.float32)
    opacity32 = None if opacity is None else np.ascontiguousarray(opacity, np.float32)
    rgb64 = np.ascontiguousarray(rgb, np.float32).reshape(-1, 3).astype(np.float64)
    bg64 = np.zeros(3) if bg is None else np.float32(bg).astype(np.float64).reshape(3)
    trunc64, min_op = np.float64(np.float32(trunc)), np.float32(min_opacity)
    C = np.zeros((n, 4)) if state is None else np.array(state, np.float64).reshape(n, 4)
    n_views, dw, sum_w = np.zeros(n), np.zeros(n), np.zeros(n)
    dterm, sum_wu = np.zeros((n, 3)), np.zeros((n, 3))
    first, count = (0, len(models)) if views is None else views
    for view in range(first, first + count):
        w_img, h_img = sizes[view]
        pr = project(x, c2w[view], int(models[view]), lenses[view])
        dist = pr["dist"]
        with np.errstate(all="ignore"):
            u, v = pr["u"], pr["v"]
            alive = (pr["z"] > 0) & (pr["guard"] > 0) & (u >= 0) & (u < w_img) & (v >= 0) & (v < h_img)
        g = np.zeros(n, np.int64)
        g[alive] = offsets[view] + np.floor(v[alive]).astype(np.int64) * w_img + np.floor(u[alive]).astype(np.int64)
        D = depth32[g]
        alive &= np.isfinite(D) & (D > 0)
        op = np.ones(n)
        if opacity32 is not None:
            with np.errstate(invalid="ignore"):
                alive &= opacity32[g] >= min_op
            op = np.where(alive, opacity32[g].astype(np.float64), 1.0)
        with np.errstate(invalid="ignore"):
            sdf = np.where(alive, D.astype(np.float64) - dist, np.inf)
        band = alive & (sdf >= -trunc64) & (sdf <= trunc64)
        near = alive & (np.abs(sdf) <= trunc64 + 2.0 ** -22 * dist)
        w = np.where(band, 1.0 - np.abs(sdf) / trunc64, 0.0)
        col, raw = uncomposite(rgb64[g], op, bg64)
        C[:, :3] += w[:, None] * col
        C[:, 3] += w
        a = np.where(near, 2.0 ** -22 * dist / trunc64 + 2.0 ** -23, 0.0)
        with np.errstate(invalid="ignore"):
            # beyond |u_raw| = 2 both sides clamp alike, and a NaN is 0 on both sides: no error from the un-compositing there
            du = np.where(np.abs(raw) <= 2.0, SECOND * E * (np.abs(1.0 - op)[:, None] * np.abs(bg64)[None, :] / op[:, None] + 2.0 * np.abs(raw)), 0.0)
        n_views += near
        dw += a
        dterm += a[:, None] * col + np.where(near, w + a, 0.0)[:, None] * du
        sum_w += w
        sum_wu += w[:, None] * col
    out = dict(C=C, n_views=n_views, dw=dw, dterm=dterm, sum_w=sum_w, sum_wu=sum_wu)
    if margins:
        m = ref.integrate(dims, lo, h, c2w, models, lenses, sizes, depth, opacity, min_opacity, trunc, views=views)
        out.update({k: m[k] for k in m if k.startswith("margin_")})
    return out


CORNERS = [(d & 1, (d >> 1) & 1, d >> 2) for d in range(8)]       # grid_device.h's order: d = dx + 2 dy + 4 dz


def sample_colors(C, dims, lo, h, points, volume64=False):
    """C [nodes,4] (float32 values; with `volume64` float64 values, as `integrate_color` returns them), points [n,3] float32.
    Returns a dict: rgb float64 [n,3] and den [n] -- (0, 0, 0, 0) where den is not > 0 or a coordinate is not finite --; num [n,3];
    and per point what the bound is made of:
      du        [n,3] 2^-23 (n_c + 1): the error of u_c
      near_face [n] some g_c lies within du_c of an integer: only there may the float32 floor name the neighbouring cell
      spread    [n,4] the largest difference of each accumulator between two corners of the cell; for a near_face point, between any
                two nodes of the 4 x 4 x 4 block of the cell and its neighbours (the interpolant is continuous across the face)
      size      [n,4] the largest magnitude of each accumulator among the same nodes
      idx       [n,3] the cell"""
    nx, ny, nz = (int(d) for d in dims)
    nd = np.int64([nx, ny, nz])
    C = (np.asarray(C, np.float64) if volume64 else np.asarray(C, np.float32).astype(np.float64)).reshape(nz + 1, ny + 1, nx + 1, 4)
    p32 = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    n = p32.shape[0]
    lo64, h64 = np.float32(lo).astype(np.float64), np.float32(h).astype(np.float64)
    finite = np.isfinite(p32).all(1)
    p = np.where(finite[:, None], p32.astype(np.float64), lo64[None, :])
    g = (p - lo64) / h64
    idx = np.clip(np.floor(g), 0, nd - 1).astype(np.int64)
    u = np.clip(g - idx, 0.0, 1.0)
    num, den = np.zeros((n, 3)), np.zeros(n)
    for dx, dy, dz in CORNERS:
        t = (u[:, 0] if dx else 1.0 - u[:, 0]) * (u[:, 1] if dy else 1.0 - u[:, 1]) * (u[:, 2] if dz else 1.0 - u[:, 2])
        c = C[idx[:, 2] + dz, idx[:, 1] + dy, idx[:, 0] + dx]
        num += t[:, None] * c[:, :3]
        den += t * c[:, 3]
    ok = finite & (den > 0)
    rgb = np.where(ok[:, None], num / np.where(ok, den, 1.0)[:, None], 0.0)
    du = np.broadcast_to(2.0 ** -23 * (nd + 1.0), (n, 3))
    near_face = (np.abs(g - np.rint(g)) <= du).any(1)

    def extremes(offsets):
        lo_v, hi_v = np.full((n, 4), np.inf), np.full((n, 4), -np.inf)
        for dz in offsets:
            for dy in offsets:
                for dx in offsets:
                    c = C[np.clip(idx[:, 2] + dz, 0, nz), np.clip(idx[:, 1] + dy, 0, ny), np.clip(idx[:, 0] + dx, 0, nx)]
                    lo_v, hi_v = np.minimum(lo_v, c), np.maximum(hi_v, c)
        return lo_v, hi_v

    # away from the faces float32 and float64 name the same cell: its own 8 corners; within du of a face, the neighbours as well
    (lo_c, hi_c), (lo_b, hi_b) = extremes(range(0, 2)), extremes(range(-1, 3))
    lo_v, hi_v = np.where(near_face[:, None], lo_b, lo_c), np.where(near_face[:, None], hi_b, hi_c)
    return dict(rgb=rgb, den=np.where(ok, den, 0.0), num=np.where(ok[:, None], num, 0.0), finite=finite, du=du, spread=hi_v - lo_v,
                size=np.maximum(np.abs(lo_v), np.abs(hi_v)), near_face=near_face, idx=idx)
