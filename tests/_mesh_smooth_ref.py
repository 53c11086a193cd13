"""The yardstick of the mesh smoothing: the vertex adjacency, the smoothing pass, Taubin smoothing and the vertex normals of
the faces as include/tinynerf_hip.h defines them, restated in numpy without the kernels -- the adjacency in integers, passes and normals
in float64 on whatever positions they are given --, the per-element error bounds of the fp32 kernels against them, and the meshes and
mesh properties the tests share."""
import functools

import numpy as np

import _mesh_ref as mref

EPS = 2.0 ** -24
LAMBDA, MU = 0.5, -0.53


# ------------------------------------------------------------------------------------------------------------ adjacency
def participating(faces, V):
    """[F] bool: the three indices lie in [0, V) and are pairwise different"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    inside = ((f >= 0) & (f < V)).all(1)
    return inside & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])


def adjacency(faces, V):
    """(offsets [V+1] int32, pairs [3F',2] int32 -- the rows up to offsets[V] --, pinned [V] uint8, stats), in integers: the corners of
    the participating faces in face order, sorted by their vertex with a STABLE sort (a face names a vertex at most once, so a row is
    in ascending face id); pinned from the counts of every (vertex, id) among the rows' entries.  `adjacency_loop` is the same thing
    as a plain loop, for small meshes."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    f = f[participating(f, V)]
    vertex = f.reshape(-1)                                          # corner 3 f + k names f[k]; its pair is (f[k+1], f[k+2])
    pair = np.stack([f[:, [1, 2, 0]].reshape(-1), f[:, [2, 0, 1]].reshape(-1)], 1)
    order = np.argsort(vertex, kind="stable")
    owner, pairs = vertex[order], pair[order].astype(np.int32).reshape(-1, 2)
    degree = np.bincount(owner, minlength=V).astype(np.int64)[:V] if V else np.zeros(0, np.int64)
    offsets = np.concatenate([[0], np.cumsum(degree)]).astype(np.int32)
    key, counts = np.unique(np.repeat(owner, 2) * max(V, 1) + pairs.reshape(-1), return_counts=True)
    bad = np.zeros(V, bool)
    bad[key[counts != 2] // max(V, 1)] = True
    pinned = ((degree == 0) | bad).astype(np.uint8)
    stats = (f.shape[0], int((pinned == 0).sum()), int(degree.max()) if V else 0)
    return offsets, pairs, pinned, stats


def adjacency_loop(faces, V):
    """`adjacency` as a plain loop over the faces in ascending id, every face appending (its other two corners in cyclic order) to
    the rows of its three corners"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    rows = [[] for _ in range(V)]
    for face in f[participating(f, V)]:
        for k in range(3):
            rows[face[k]].append((face[(k + 1) % 3], face[(k + 2) % 3]))
    degree = np.array([len(r) for r in rows], np.int64).reshape(V)
    offsets = np.concatenate([[0], np.cumsum(degree)]).astype(np.int32)
    pairs = np.array([p for r in rows for p in r], np.int32).reshape(-1, 2)
    pinned = np.ones(V, np.uint8)
    for v, r in enumerate(rows):
        if r:
            _, counts = np.unique(np.array(r).reshape(-1), return_counts=True)
            pinned[v] = 0 if (counts == 2).all() else 1
    stats = (int(degree.sum()) // 3, int((pinned == 0).sum()), int(degree.max()) if V else 0)
    return offsets, pairs, pinned, stats


def _row_index(offsets):
    """(vertex of every pair row, d [V])"""
    d = np.diff(offsets.astype(np.int64))
    return np.repeat(np.arange(d.size), d), d


def moves(offsets, pinned):
    d = np.diff(offsets.astype(np.int64))
    return (d > 0) if pinned is None else ((d > 0) & (np.asarray(pinned) == 0))


# ------------------------------------------------------------------------------------------------------------ pass, Taubin
def smooth_pass(p, offsets, pairs, pinned, f):
    """(out [V,3] float64, bound [V,3]): one pass with the factor f in float64 on p (any float dtype; not moved rows returned as they
    are, as float64), and what the fp32 kernel may differ by on the rows that move, per component:
    2^-24 (|f| (A + |c| + 3 |c - p|) + 2 |p|), A the sum of the absolute values of the row's 2 d terms"""
    p = np.asarray(p, np.float64)
    V = p.shape[0]
    owner, d = _row_index(offsets)
    terms = p[pairs[:owner.size].astype(np.int64)]                 # [rows, 2, 3]
    s, A = np.zeros((V, 3)), np.zeros((V, 3))
    with np.errstate(all="ignore"):
        np.add.at(s, owner, terms.sum(1))
        np.add.at(A, owner, np.abs(terms).sum(1))
        c = s / np.maximum(2 * d, 1)[:, None]
        move = moves(offsets, pinned)[:, None]
        out = np.where(move, p + f * (c - p), p)
        bound = np.where(move, EPS * (abs(f) * (A + np.abs(c) + 3 * np.abs(c - p)) + 2 * np.abs(p)), 0.0)
    return out, bound


def carry_bound(E, b, offsets, pairs, pinned, f):
    """the bound after a pass, E the bound before it and b the pass's own: E' = |1 - f| E[v] + |f| mean(E[row]) + b on the rows that
    move, E on the others"""
    owner, d = _row_index(offsets)
    mean = np.zeros_like(E)
    np.add.at(mean, owner, E[pairs[:owner.size].astype(np.int64)].sum(1))
    mean /= np.maximum(2 * d, 1)[:, None]
    return np.where(moves(offsets, pinned)[:, None], abs(1 - f) * E + abs(f) * mean + b, E)


def taubin(p, offsets, pairs, pinned, iterations, lam=LAMBDA, mu=MU):
    """(out float64, bound): `iterations` times a pass with lam and a pass with mu in float64, the per-pass bound carried through"""
    x, E = np.asarray(p, np.float64), np.zeros((len(p), 3))
    for _ in range(iterations):
        for f in (lam, mu):
            x, b = smooth_pass(x, offsets, pairs, pinned, f)
            E = carry_bound(E, b, offsets, pairs, pinned, f)
    return x, E


# ------------------------------------------------------------------------------------------------------------ normals
def vertex_normals(p, offsets, pairs, fallback=None):
    """(normals [V,3] float64, g [V,3], bound [V]): g = the sum over the row of (p[a] - p[v]) x (p[b] - p[v]), n = g / |g|, the
    fallback row (or 0) where d == 0 or |g| is 0 or not finite; bound = 2 |bound_g| / |g| + 8 2^-24 with bound_g,i = (4 d + 8) 2^-24
    S_i, S_i the sum of the absolute values of the products in component i (inf where the fallback is taken)"""
    p = np.asarray(p, np.float64)
    V = p.shape[0]
    owner, d = _row_index(offsets)
    pr = pairs[:owner.size].astype(np.int64)
    e, f = p[pr[:, 0]] - p[owner], p[pr[:, 1]] - p[owner]
    g, S = np.zeros((V, 3)), np.zeros((V, 3))
    with np.errstate(all="ignore"):
        for i in range(3):
            j, k = (i + 1) % 3, (i + 2) % 3
            np.add.at(g[:, i], owner, e[:, j] * f[:, k] - e[:, k] * f[:, j])
            np.add.at(S[:, i], owner, np.abs(e[:, j] * f[:, k]) + np.abs(e[:, k] * f[:, j]))
        length = np.sqrt((g * g).sum(1))
        ok = (d > 0) & np.isfinite(length) & (length > 0)
        other = np.zeros((V, 3)) if fallback is None else np.asarray(fallback, np.float64)
        n = np.where(ok[:, None], g / np.where(ok, length, 1.0)[:, None], other)
        bg = (4 * d + 8)[:, None] * EPS * S
        bound = np.where(ok, 2 * np.sqrt((bg * bg).sum(1)) / np.where(ok, length, 1.0) + 8 * EPS, np.inf)
    return n, g, bound


# ------------------------------------------------------------------------------------------------------------ meshes
def radial_std(p, centre):
    return float(np.linalg.norm(np.asarray(p, np.float64) - centre, axis=1).std())


BINARY_CENTRE = np.float64([0.013, 0.013, 0.013])


@functools.lru_cache(maxsize=None)
def binary_sphere():
    """(vertices [590,3] float64, normals, faces [1176,3] int32) of the yardstick's Surface Nets mesh of the field that is 1 at the nodes
    with |x - 0.013| < 0.7 and 0 elsewhere, level 0.5, 16^3 cells over [-1,1]^3: the staircase smoothing is for.  Read only."""
    dims = (16, 16, 16)
    lo, h = mref.grid(dims, (-1, -1, -1), (1, 1, 1))
    x = mref.node_positions(dims, lo, h).astype(np.float64)
    values = (np.linalg.norm(x - BINARY_CENTRE, axis=-1) < 0.7).astype(np.float32)
    want = mref.surface_nets(values, lo, h, np.float32(0.5))
    out = want["vertices"], want["normals"], want["faces"]
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def tilted_plane():
    """(vertices, normals, faces) of the yardstick's tilted plane cut by a box of 9 x 7 x 8 cells: an open mesh, its rim pinned"""
    want = mref.case("plane", (9, 7, 8))[4]
    return want["vertices"], want["normals"], want["faces"]


def fan(n):
    """a closed disk fan of n faces around vertex 0, rim 1 .. n: the hub free (degree n), the rim on the boundary"""
    i = np.arange(n)
    return np.stack([np.zeros(n, np.int64), 1 + i, 1 + (i + 1) % n], 1).astype(np.int32), n + 1


def strip(V):
    """a triangle strip over V vertices, triangle i = (i, i+1, i+2) with every other one reversed: consistently oriented"""
    i = np.arange(V - 2)
    return np.where((i % 2 == 0)[:, None], np.stack([i, i + 1, i + 2], 1), np.stack([i + 1, i, i + 2], 1)).astype(np.int32), V
