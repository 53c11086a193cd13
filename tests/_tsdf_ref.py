"""The yardstick of the TSDF fusion: tn_tsdf_integrate and tn_tsdf_mask_faces as include/tinynerf_hip.h defines them,
restated in numpy without the kernels -- float64 arithmetic on the float32 inputs (node positions by the kernel's own fmaf, which
float64 reproduces exactly; table, depth, opacity, trunc and min_opacity as the float32 values the kernel is handed), the depth and
opacity gates exact float32 comparisons.  Besides S and W it returns, per node, how close any view came to a DECISION edge -- a
float32 kernel may fall on the other side of an edge the node sits on, and no tolerance on S covers a vote that is cast or not --
and what the bound on S needs.  Also the mesh field, the face mask, and the analytic scenes of the tests."""
import numpy as np

PINHOLE, OPENCV, FISHEYE = 0, 1, 2


def nodes(dims, lo, h):
    """float64 [n, 3]: the float32 positions fmaf((float)idx, h, lo) of the grid's nodes, i fastest.  idx * h is exact in float64
    (24 + 24 bits) and so is the sum unless it needs more than 53 bits, which these grids are far from; its rounding to float32 is
    the fma's."""
    nx, ny, nz = (int(d) for d in dims)
    lo64, h64 = np.float32(lo).astype(np.float64), np.float32(h).astype(np.float64)
    k, j, i = np.meshgrid(np.arange(nz + 1), np.arange(ny + 1), np.arange(nx + 1), indexing="ij")
    idx = np.stack([i.reshape(-1), j.reshape(-1), k.reshape(-1)], 1).astype(np.float64)
    return (idx * h64 + lo64).astype(np.float32).astype(np.float64)


def _poly(s, c1, c2, c3, c4):
    return 1.0 + s * (c1 + s * (c2 + s * (c3 + s * c4)))


def project(x, c2w, model, lens):
    """one view's steps 1-4 for nodes x [n,3]: dict of z, u, v, guard (the polynomial's value, +inf for a pinhole), guard_size (the sum
    of its terms' magnitudes) and dist = |p|; entries are NaN / arbitrary where z <= 0"""
    c2w, L = np.float32(c2w).astype(np.float64).reshape(-1)[:12].reshape(3, 4), np.float32(lens).astype(np.float64)
    p = x - c2w[:, 3]
    q = p @ c2w[:, :3]                                             # R^T p
    z = -q[:, 2]
    with np.errstate(all="ignore"):
        xu, yu = q[:, 0] / z, -q[:, 1] / z
        k1, k2, k3, k4, p1, p2 = L[4:]
        r2 = xu * xu + yu * yu
        guard, size = np.full(x.shape[0], np.inf), np.ones(x.shape[0])
        xd, yd = xu, yu
        if model == OPENCV:
            rad = _poly(r2, k1, k2, k3, k4)
            xd = xu * rad + 2.0 * p1 * xu * yu + p2 * (r2 + 2.0 * xu * xu)
            yd = yu * rad + 2.0 * p2 * xu * yu + p1 * (r2 + 2.0 * yu * yu)
            s = r2
        elif model == FISHEYE:
            r = np.sqrt(r2)
            th = np.arctan(r)
            s = th * th
            scale = np.where(r > 0, th * _poly(s, k1, k2, k3, k4) / np.where(r > 0, r, 1.0), 1.0)
            xd, yd = xu * scale, yu * scale
        if model != PINHOLE:
            guard = _poly(s, 3.0 * k1, 5.0 * k2, 7.0 * k3, 9.0 * k4)
            size = _poly(s, abs(3.0 * k1), abs(5.0 * k2), abs(7.0 * k3), abs(9.0 * k4))
        u, v = L[0] * xd + L[2], L[1] * yd + L[3]
    return {"z": z, "u": u, "v": v, "guard": guard, "guard_size": size, "dist": np.sqrt((p * p).sum(1))}


def _edge_distance(u, n):
    """distance of u to the nearest pixel edge 0, 1, .., n: the places where floor(u), or the inside test, changes"""
    return np.abs(u - np.clip(np.rint(u), 0, n))


def integrate(dims, lo, h, c2w, models, lenses, sizes, depth, opacity, min_opacity, trunc, views=None, state=None):
    """dims (nx, ny, nz); c2w [n,3,4], models [n], lenses [n,10], sizes [n,2] = w h; depth / opacity [n_pixels] float32 (opacity may be
    None); views = (first, count).  Returns a dict: S, W float64 [nodes]; margin_pixel (px), margin_z and margin_trunc (as a fraction
    of |p|), margin_guard (as a fraction of the polynomial's terms' magnitudes): the smallest distance of any view to that decision
    edge, +inf where no view came to the decision; bound_views = sum over the contributing views of (2^-22 |p| / trunc + 2^-22) and
    sum_abs = sum |s|, for the bound on S."""
    x = nodes(dims, lo, h)
    n = x.shape[0]
    sizes = np.asarray(sizes, np.int64).reshape(-1, 2)
    offsets = np.concatenate([[0], np.cumsum(sizes[:, 0] * sizes[:, 1])])
    depth32 = np.ascontiguousarray(depth, np.float32)
    opacity32 = None if opacity is None else np.ascontiguousarray(opacity, np.float32)
    trunc64, min_op = np.float64(np.float32(trunc)), np.float32(min_opacity)
    S, W = (np.zeros(n), np.zeros(n)) if state is None else (state[0].copy(), state[1].copy())
    out = {k: np.full(n, np.inf) for k in ("margin_pixel", "margin_z", "margin_guard", "margin_trunc")}
    bound_views, sum_abs = np.zeros(n), np.zeros(n)
    first, count = (0, len(models)) if views is None else views
    for view in range(first, first + count):
        w, hh = sizes[view]
        pr = project(x, c2w[view], int(models[view]), lenses[view])
        dist = pr["dist"]
        with np.errstate(all="ignore"):
            out["margin_z"] = np.minimum(out["margin_z"], np.abs(pr["z"]) / dist)
            alive = pr["z"] > 0
            out["margin_guard"] = np.where(alive, np.minimum(out["margin_guard"], np.abs(pr["guard"]) / pr["guard_size"]), out["margin_guard"])
            alive &= pr["guard"] > 0
            u, v = pr["u"], pr["v"]
            edge = np.minimum(_edge_distance(u, w), _edge_distance(v, hh))
            out["margin_pixel"] = np.where(alive, np.minimum(out["margin_pixel"], edge), out["margin_pixel"])
            alive &= (u >= 0) & (u < w) & (v >= 0) & (v < hh)
        g = np.zeros(n, np.int64)
        g[alive] = offsets[view] + np.floor(v[alive]).astype(np.int64) * w + np.floor(u[alive]).astype(np.int64)
        D = depth32[g]
        alive &= np.isfinite(D) & (D > 0)
        if opacity32 is not None:
            with np.errstate(invalid="ignore"):
                alive &= opacity32[g] >= min_op
        sdf = D.astype(np.float64) - dist
        out["margin_trunc"] = np.where(alive, np.minimum(out["margin_trunc"], np.abs(sdf + trunc64) / dist), out["margin_trunc"])
        alive &= ~(sdf < -trunc64)
        s = np.where(alive, np.minimum(sdf / trunc64, 1.0), 0.0)
        S += s
        W += alive
        bound_views += np.where(alive, 2.0 ** -22 * dist / trunc64 + 2.0 ** -22, 0.0)
        sum_abs += np.abs(s)
    out.update(S=S, W=W, bound_views=bound_views, sum_abs=sum_abs)
    return out


def field(S, W):
    """the mesh field: -S / W where W > 0, -1 elsewhere"""
    S, W = np.asarray(S, np.float64), np.asarray(W, np.float64)
    return np.where(W > 0, -S / np.where(W > 0, W, 1.0), -1.0)


def mask_faces(W, dims, cell_ids, n_vertices, faces):
    """faces with (-1, -1, -1) where an index lies outside [0, V) or names a vertex whose cell has a corner at W == 0"""
    nx, ny, nz = (int(d) for d in dims)
    seen = np.asarray(W).reshape(nz + 1, ny + 1, nx + 1) > 0
    cell_ok = np.ones((nz, ny, nx), bool)
    for d in range(8):
        dx, dy, dz = d & 1, (d >> 1) & 1, d >> 2
        cell_ok &= seen[dz:dz + nz, dy:dy + ny, dx:dx + nx]
    ids = np.asarray(cell_ids, np.int64).reshape(-1)
    observed = np.zeros(max(int(n_vertices), 1), bool)
    named = (ids >= 0) & (ids < n_vertices)
    observed[ids[named]] = cell_ok.reshape(-1)[named]
    faces = np.array(faces, np.int32).reshape(-1, 3)
    valid = ((faces >= 0) & (faces < n_vertices)).all(1)
    keep = valid & observed[np.where(valid[:, None], faces, 0)].all(1)
    faces[~keep] = -1
    return faces


# ------------------------------------------------------------------------------------------------------------ analytic scenes
def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    """c2w [3,4] of a camera at `eye` looking at `target`: x right, y up, looking down -z"""
    eye, target, up = np.float64(eye), np.float64(target), np.float64(up)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    return np.stack([right, np.cross(right, fwd), -fwd, eye], 1)


def ring_cameras(n, radius=2.6, seed=0):
    """n cameras around the origin, looking at it, at mixed heights (float32 values as float64)"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        a = 2.0 * np.pi * (i + 0.3 * rng.random()) / n
        e = 0.9 * (rng.random() - 0.5)
        out.append(look_at(radius * np.array([np.cos(a) * np.cos(e), np.sin(a) * np.cos(e), np.sin(e)])))
    return np.float32(np.stack(out)).astype(np.float64)


def sphere_depth(o, d, radius, centre=(0.0, 0.0, 0.0)):
    """distance along the unit rays (o, d) to the sphere, +inf where they miss it (float64)"""
    oc = np.asarray(o, np.float64) - np.float64(centre)
    d = np.asarray(d, np.float64)
    b = (oc * d).sum(-1)
    disc = b * b - ((oc * oc).sum(-1) - radius * radius)
    with np.errstate(invalid="ignore"):
        t = -b - np.sqrt(disc)
    return np.where((disc > 0) & (t > 0), t, np.inf)
