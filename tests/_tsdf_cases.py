"""The shared inputs of the TSDF tests: camera tables with mixed image sizes, off-centre principal points and the fixture
lenses of DESIGN 6d, analytic sphere depths with specks of bad values, and the yardstick's result for each case -- computed once
(functools.lru_cache) and read only."""
import functools

import numpy as np

import _camera_ref as cam
import _tsdf_ref as ref

RADIUS, FAR = 0.6, 5.0                       # the sphere; the depth of a ray that misses it (beyond the box: free space all along)
TRUNC = 0.25
SIZES = [(128, 96), (96, 72), (64, 48), (128, 80)]
MIXED = ["pinhole", "opencv_a", "fisheye", "opencv_c", "opencv_b"]
TIE = {"margin_pixel": 2.0 ** -12, "margin_z": 2.0 ** -16, "margin_guard": 2.0 ** -14, "margin_trunc": 2.0 ** -21}

# name: (dims, views, lens -- a fixture's name or "mixed" --, opacity)
CASES = {
    "1x1x1-1-pinhole": ((1, 1, 1), 1, "pinhole", False),
    "2x2x2-3-opencv_a": ((2, 2, 2), 3, "opencv_a", True),
    "5x3x4-3-fisheye": ((5, 3, 4), 3, "fisheye", False),
    "16x12x18-3-opencv_c": ((16, 12, 18), 3, "opencv_c", True),
    "16x12x18-8-mixed": ((16, 12, 18), 8, "mixed", True),
    "16x12x18-8-fisheye": ((16, 12, 18), 8, "fisheye", False),
    "33x31x35-8-pinhole": ((33, 31, 35), 8, "pinhole", False),
    "33x31x35-8-mixed": ((33, 31, 35), 8, "mixed", True),
}


def grid(dims):
    lo = np.float32([-1.0, -1.0, -1.0])
    return lo, (2.0 / np.float64(dims)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def table(n_views, lens, seed=1):
    """c2w [n,3,4], models [n], lenses [n,10], sizes [n,2]: float32 / int values held as float64 / int64.  With 3 views or more,
    view 1 looks AWAY from the box and view 2 stands inside it, so that there are nodes behind it"""
    c2w = ref.ring_cameras(n_views, seed=seed)
    if n_views >= 3:
        eye = c2w[1][:, 3]
        c2w[1] = np.float32(ref.look_at(eye, 2.0 * eye)).astype(np.float64)
        c2w[2] = np.float32(ref.look_at([0.31, -0.22, 0.13], [1.0, 0.4, -0.1])).astype(np.float64)
    models, lenses, sizes = [], [], []
    for i in range(n_views):
        w, h = SIZES[i % len(SIZES)]
        model, L = cam.scaled(cam.FIXTURES[MIXED[i % len(MIXED)] if lens == "mixed" else lens], w, h)
        L = L.copy()
        L[2], L[3] = 0.5 * w + 0.37, 0.5 * h - 0.21                # off centre: with an integer cx the nodes on the axis sit on a pixel edge
        models.append(model), lenses.append(np.float32(L).astype(np.float64)), sizes.append((w, h))
    return c2w, np.int64(models), np.stack(lenses), np.int64(sizes)


@functools.lru_cache(maxsize=None)
def maps(n_views, lens, seed=1):
    """depth, opacity float32 [n_pixels]: the sphere seen through every pixel's centre ray, FAR where it is missed; 1 pixel in 16 holds
    a speck (0, a negative depth, NaN, +inf, -inf); the opacity is 1 with a tenth of the pixels below 0.5 and a few NaN"""
    c2w, models, lenses, sizes = table(n_views, lens, seed)
    n = int((sizes[:, 0] * sizes[:, 1]).sum())
    o, d, _ = cam.table_rays(c2w, models, lenses, sizes, np.arange(n))
    depth = ref.sphere_depth(o, d, RADIUS)
    depth = np.where(np.isfinite(depth), depth, FAR).astype(np.float32)
    rng = np.random.default_rng(seed + 100)
    speck = rng.random(n) < 1.0 / 16.0
    depth[speck] = rng.choice(np.float32([0.0, -1.5, np.nan, np.inf, -np.inf]), int(speck.sum()))
    opacity = np.where(rng.random(n) < 0.1, 0.3, 1.0).astype(np.float32)
    opacity[rng.random(n) < 0.01] = np.nan
    return depth, opacity


@functools.lru_cache(maxsize=None)
def case(name):
    """dict: dims, lo, h, the table, depth, opacity (None without), min_opacity, trunc, and `want`, the yardstick's result"""
    dims, n_views, lens, with_opacity = CASES[name]
    lo, h = grid(dims)
    c2w, models, lenses, sizes = table(n_views, lens)
    depth, opacity = maps(n_views, lens)
    c = dict(dims=dims, lo=lo, h=h, c2w=c2w, models=models, lenses=lenses, sizes=sizes, depth=depth, opacity=opacity if with_opacity else None,
             min_opacity=0.5, trunc=TRUNC, n_views=n_views)
    c["want"] = ref.integrate(dims, lo, h, c2w, models, lenses, sizes, depth, c["opacity"], 0.5, TRUNC)
    for v in [depth, opacity, lo, h, c2w, lenses] + [a for a in c["want"].values()]:
        v.setflags(write=False)
    return c


def ambiguous(want):
    """nodes at which some view came closer to a decision edge than the tie margin"""
    return np.logical_or.reduce([want[k] < TIE[k] for k in TIE])


def s_bound(want):
    """the issue's bound on |S - S_ref| at an unambiguous node: sum over the contributing views of (2^-22 |p| / trunc + 2^-22), plus
    (n - 1) 2^-24 sum |s| for the n - 1 additions"""
    return want["bound_views"] + np.maximum(want["W"] - 1.0, 0.0) * 2.0 ** -24 * want["sum_abs"]
