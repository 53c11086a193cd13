"""The yardstick of the mesh extraction: naive Surface Nets as include/tinynerf_hip.h defines it, restated in numpy without
the kernel -- float64 arithmetic on the float32 inputs, insideness an exact float32 comparison --, the per-element error bounds of
the float32 kernel against it, the analytic fields of the tests and the mesh properties they check."""
import functools

import numpy as np

EPS = 2.0 ** -24


def _corner(a, d, n):
    nz, ny, nx = n
    dx, dy, dz = d & 1, (d >> 1) & 1, d >> 2
    return a[dz:dz + nz, dy:dy + ny, dx:dx + nx].reshape(-1)


def surface_nets(values, lo, h, level):
    """values [nz+1, ny+1, nx+1] float32, lo / h 3 float32 each, level a float32 -> dict of
    cells [V] (the active cells in cell order), vertices / normals [V,3] float64, faces [F,3] int32, quads [F/2,4],
    vertex_bound / normal_bound [V,3] / [V]: what the float32 kernel may differ by (issue / DESIGN 6h)"""
    v32 = np.ascontiguousarray(values, np.float32)
    n = tuple(s - 1 for s in v32.shape)
    nz, ny, nx = n
    lo64, h64, level32 = np.float32(lo).astype(np.float64), np.float32(h).astype(np.float64), np.float32(level)
    inside = v32 >= level32
    ins_all = np.stack([_corner(inside, d, n) for d in range(8)], 1)                      # [cells, 8]
    count_in = ins_all.sum(1)
    cells = np.flatnonzero((count_in > 0) & (count_in < 8))
    ins = ins_all[cells]
    val = np.stack([_corner(v32, d, n)[cells] for d in range(8)], 1).astype(np.float64)
    idx = np.stack([cells % nx, (cells // nx) % ny, cells // (nx * ny)], 1) if cells.size else np.zeros((0, 3), np.int64)
    lvl = np.float64(level32)
    total, crossed_n = np.zeros((cells.size, 3)), np.zeros(cells.size)
    with np.errstate(all="ignore"):
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            for e in range(4):
                ob, oc = e & 1, e >> 1
                d0 = (ob << b) | (oc << c)
                d1 = d0 | (1 << a)
                crossed = ins[:, d0] != ins[:, d1]
                v0, v1 = val[:, d0], val[:, d1]
                t = np.clip((lvl - v0) / (v1 - v0), 0.0, 1.0)
                t = np.where(np.isfinite(v0) & np.isfinite(v1), t, 0.5)
                total[:, a] += np.where(crossed, t, 0.0)
                total[:, b] += np.where(crossed, ob, 0.0)
                total[:, c] += np.where(crossed, oc, 0.0)
                crossed_n += crossed
        u = total / crossed_n[:, None]
        vertices = (idx + u) * h64 + lo64
        dims = np.float64([nx, ny, nz])
        vertex_bound = h64 * (2.0 ** -17 + EPS * (dims + 1)) + EPS * np.abs(vertices)
        # normal: minus the gradient at u of the cell's trilinear interpolant, normalised
        grad, a_sum, d_max = np.zeros((cells.size, 3)), np.zeros((cells.size, 3)), np.zeros((cells.size, 3))

        def g_of(a, ub, uc):
            b, c = (a + 1) % 3, (a + 2) % 3
            s, sb, sc = 1 << a, 1 << b, 1 << c
            return ((val[:, s] - val[:, 0]) * (1 - ub) * (1 - uc) + (val[:, s | sb] - val[:, sb]) * ub * (1 - uc)
                    + (val[:, s | sc] - val[:, sc]) * (1 - ub) * uc + (val[:, s | sb | sc] - val[:, sb | sc]) * ub * uc) / h64[a]

        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            ub, uc = u[:, b], u[:, c]
            grad[:, a] = g_of(a, ub, uc)
            for d in range(8):                              # the 8 terms of g_a: corner value x weight / h_a
                wb, wc = (ub if (d >> b) & 1 else 1 - ub), (uc if (d >> c) & 1 else 1 - uc)
                a_sum[:, a] += np.abs(val[:, d]) * wb * wc / h64[a]
            d_max[:, a] = np.maximum(np.abs(g_of(a, 1.0, uc) - g_of(a, 0.0, uc)), np.abs(g_of(a, ub, 1.0) - g_of(a, ub, 0.0)))
        length = np.sqrt((grad * grad).sum(1))
        ok = np.isfinite(length) & (length > 0)
        normals = np.where(ok[:, None], -grad / np.where(ok, length, 1.0)[:, None], 0.0)
        g_bound = 16 * EPS * a_sum + 2.0 ** -17 * d_max
        normal_bound = np.where(ok, 2 * np.sqrt((g_bound * g_bound).sum(1)) / np.where(ok, length, 1.0) + 8 * EPS, np.inf)
    # faces: cells in order, axes in order
    vid = np.full(nx * ny * nz, -1, np.int64)
    vid[cells] = np.arange(cells.size)
    all_cells = np.arange(nx * ny * nz)
    aidx = [all_cells % nx, (all_cells // nx) % ny, all_cells // (nx * ny)]
    emits = np.zeros((all_cells.size, 3), bool)
    for a in range(3):
        emits[:, a] = (ins_all[:, 0] != ins_all[:, 1 << a]) & (aidx[(a + 1) % 3] >= 1) & (aidx[(a + 2) % 3] >= 1)
    qc, qa = np.nonzero(emits)                              # C order: (cell, axis)
    stride = np.int64([1, nx, nx * ny])
    sb, sc = stride[(qa + 1) % 3], stride[(qa + 2) % 3]
    quads = np.stack([vid[qc - sb - sc], vid[qc - sc], vid[qc], vid[qc - sb]], 1) if qc.size else np.zeros((0, 4), np.int64)
    quads = np.where(ins_all[qc, 0][:, None], quads, quads[:, ::-1])
    faces = np.stack([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]], 1).reshape(-1, 3).astype(np.int32)
    return {"cells": cells, "vertices": vertices, "normals": normals, "faces": faces, "quads": quads, "vertex_bound": vertex_bound,
            "normal_bound": normal_bound}


# ------------------------------------------------------------------------------------------------------------ grids and fields
def grid(dims, lo=(-1.0, -0.75, -1.25), hi=(1.0, 0.75, 1.25)):
    """(lo, h) float32 of a box cut into dims = (nx, ny, nz) cells; h is the float32 nearest to the extent / n"""
    lo32 = np.float32(lo)
    return lo32, ((np.float64(hi) - lo32.astype(np.float64)) / np.float64(dims)).astype(np.float32)


def node_positions(dims, lo, h):
    """[nz+1, ny+1, nx+1, 3] float32: fmaf(idx, h, lo) emulated in float64 -- the product of an index below 2^24 and a 24-bit h is
    exact, and for the tests' small indices and boxes of order 1 so is its sum with lo, so the cast is the fma's one rounding"""
    nx, ny, nz = dims
    lo64, h64 = np.float32(lo).astype(np.float64), np.float32(h).astype(np.float64)
    k, j, i = np.meshgrid(np.arange(nz + 1), np.arange(ny + 1), np.arange(nx + 1), indexing="ij")
    return np.stack([i * h64[0] + lo64[0], j * h64[1] + lo64[1], k * h64[2] + lo64[2]], -1).astype(np.float32)


def _unit(x, lo, hi):
    """positions -> the box's own coordinates in [-1, 1]^3: the fields are defined there, so every grid resolves them alike"""
    lo, hi = np.float64(lo), np.float64(hi)
    return (x.astype(np.float64) - (lo + hi) / 2) / ((hi - lo) / 2)


def field(name, x, lo=(-1.0, -0.75, -1.25), hi=(1.0, 0.75, 1.25), seed=0):
    """float32 values of the named field at positions x [...,3]; level 0 everywhere except `level` (0.25) -- positive inside"""
    s = _unit(x, lo, hi)
    if name == "sphere":
        f = 0.7 - np.linalg.norm(s - [0.04, -0.03, 0.02], axis=-1)
    elif name == "torus":                                   # axis y: the tube is thin along the axis with the fewest cells of (17, 9, 33)
        f = 0.3 - np.sqrt((np.sqrt(s[..., 0] ** 2 + s[..., 2] ** 2) - 0.5) ** 2 + (0.8 * s[..., 1] + 0.02) ** 2)
    elif name == "two_spheres":
        f = np.maximum(0.33 - np.linalg.norm(s - [-0.45, 0.1, -0.4], axis=-1), 0.36 - np.linalg.norm(s - [0.42, -0.05, 0.45], axis=-1))
    elif name == "plane":                                   # tilted: touches every face of the box
        f = s @ np.float64([0.3, 0.5, -0.4]) + 0.013
    elif name == "all_inside":
        f = np.ones(s.shape[:-1])
    elif name == "all_outside":
        f = -np.ones(s.shape[:-1])
    elif name == "level":                                   # values exactly on the level (0.25) at many nodes: the >= edge
        f = np.round(2 * (0.9 - np.linalg.norm(s, axis=-1))) / 4 + 0.25
    elif name in ("noise", "specks"):
        rng = np.random.default_rng([seed, s.size])
        f = rng.standard_normal(s.shape[:-1])
        if name == "specks":
            kind = rng.integers(0, 40, f.shape)
            f = np.where(kind == 0, np.nan, np.where(kind == 1, np.inf, np.where(kind == 2, -np.inf, f)))
    else:
        raise KeyError(name)
    return f.astype(np.float32)


FIELDS = ("sphere", "torus", "two_spheres", "plane", "all_inside", "all_outside", "level", "noise", "specks")
CLOSED = {"sphere": 2, "torus": 0, "two_spheres": 4}         # field -> V - E + F
LEVEL = {"level": 0.25}


@functools.lru_cache(maxsize=None)
def case(name, dims):
    """(values [nz+1,ny+1,nx+1] float32, lo, h, level, the yardstick's dict) of a field on a grid: computed once, shared, read only"""
    lo, h = grid(dims)
    values = field(name, node_positions(dims, lo, h))
    level = np.float32(LEVEL.get(name, 0.0))
    want = surface_nets(values, lo, h, level)
    for a in (values, lo, h, *want.values()):
        a.setflags(write=False)
    return values, lo, h, level, want


# ------------------------------------------------------------------------------------------------------------ mesh properties
def edge_report(faces):
    """(every undirected edge lies in exactly two triangles, every directed edge has its reverse exactly once, number of edges)"""
    f = np.asarray(faces, np.int64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)
    big = int(f.max()) + 1 if f.size else 1
    key = d[:, 0] * big + d[:, 1]
    rev = d[:, 1] * big + d[:, 0]
    uniq, cnt = np.unique(key, return_counts=True)
    directed_ok = bool((cnt == 1).all() and np.array_equal(uniq, np.unique(rev)))
    und, ucnt = np.unique(np.minimum(key, rev), return_counts=True)
    return bool((ucnt == 2).all()), directed_ok, int(und.size)


def signed_volume(vertices, faces):
    p = np.asarray(vertices, np.float64)[np.asarray(faces, np.int64)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


def degenerate_faces(faces):
    f = np.asarray(faces)
    return int(((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).sum())
