"""Fixtures of the sampler / occupancy edge tests (test_sampler_cases.py on the CPU, test_hip_sampler_edges.py on the GPU): numpy only,
nothing from tinynerf_amd.  Everything is seeded and built once per process; callers must not write into what they get.

Rays (R = 300, float32, finite, unit directions), shuffled by a fixed permutation so that the prefixes R = 1, 3, 4, 5 around the
sampler's four waves per workgroup hold mixed kinds; ``KIND`` names the kind of every ray:
  plain    origins on the sphere of radius 3, looking at the centre with noise (some of them miss the boxes)
  inside   40 origins inside both boxes
  zero_pos 20 rays with one direction component exactly +0.0      zero_neg   10 with one exactly -0.0
  away     20 rays that point away from the boxes and miss them
  face     20 origins exactly on the face plane x = hi[0] (= 1 in both boxes)

Boxes: ``mixed`` has extents 2, 2.25, 1.25 (one power of two: the sampler divides, pow2 == 0); ``pow2`` has extents 2, 4, 1 (non-cubic,
the sampler multiplies by the exact reciprocal, pow2 == 1).

Grid (12, 20, 16), threshold 0.01.  The Mip-360 contractions map ALL of space into the grid, so with cells spread evenly every ray
keeps something; the occupied cells therefore sit where only some rays go: a central block (the boxes' neighbourhood in contracted
space) and the whole x = W - 1 face (which the rays that leave towards +x end on, and which the face-plane origins of the box pairs
read with their x1 tap out of bounds).  Occupied cells are uniform in [0.005, 0.03] -- both sides of the threshold --, a share of the cells
inside the block is exactly 0, everything else is exactly 0: 22 % of the cells are occupied, 17 % lie above the threshold.  (An evenly
spread grid with 60 % of its cells occupied leaves no ray of the four Mip-360 pairs empty; test_sampler_cases.py asserts the conditions
the GPU tests rely on -- kept share, empty and non-empty rays, kept samples on zero-component and inside rays -- for every pair.)
"""
import functools

import numpy as np

f32 = np.float32

PAIRS = [(m, c) for m in ("aabb", "unbounded") for c in ("aabb", "mip360_inf", "mip360_l2")]
BOXES = {
    "mixed": np.array([[-1.0, -1.25, -0.75], [1.0, 1.0, 0.5]], f32),
    "pow2": np.array([[-1.0, -2.0, -0.5], [1.0, 2.0, 0.5]], f32),
}
GRID_SHAPE = (12, 20, 16)
THRESHOLD = 0.01
NEAR = 0.05
UNIFORM_RANGE = 2.0
S_VALUES = (1, 63, 64, 65, 200)
R = 300
R_PREFIXES = (1, 3, 4, 5)
S_LONG = 8256                                   # 129 chunks of 64: the zero-fill's second loop needs more than 64 skipped chunks
R_LONG = 64
N_KIND = {"inside": 40, "zero_pos": 20, "zero_neg": 10, "away": 20, "face": 20}
ORDER = {"mip360_inf": float("inf"), "mip360_l2": 2}


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def rays():
    """(rays_o [R,3], rays_d [R,3], KIND [R] of str); read-only"""
    rng = np.random.default_rng(20240607)
    o = _unit(rng.standard_normal((R, 3))) * 3.0
    d = _unit(-o / 3.0 + 0.4 * rng.standard_normal((R, 3)))
    kind = np.array(["plain"] * R, dtype=object)
    at = 0
    spans = {}
    for name, n in N_KIND.items():
        spans[name] = slice(at, at + n)
        kind[at:at + n] = name
        at += n
    s = spans["inside"]                                   # inside both boxes: |x| < 1, -1.25 < y < 1, |z| < 0.5
    o[s] = (rng.random((40, 3)) * 2 - 1) * [0.8, 0.8, 0.4]
    d[s] = _unit(rng.standard_normal((40, 3)))
    for name, zero in (("zero_pos", 0.0), ("zero_neg", -0.0)):
        s = spans[name]
        n = s.stop - s.start
        d[s] = _unit(-o[s] / 3.0 + 0.1 * rng.standard_normal((n, 3)))
        d[np.arange(s.start, s.stop), rng.integers(0, 3, n)] = 0.0
        d[s] = _unit(d[s])
    s = spans["away"]
    d[s] = _unit(o[s] / 3.0 + 0.2 * rng.standard_normal((20, 3)))
    s = spans["face"]
    o[s] = np.stack([np.ones(20), rng.random(20) * 1.6 - 0.8, rng.random(20) * 0.8 - 0.4], -1)
    d[s] = _unit(rng.standard_normal((20, 3)) * [1.0, 1.0, 0.5])
    o, d = o.astype(f32), d.astype(f32)
    for name, zero in (("zero_pos", 0.0), ("zero_neg", -0.0)):   # (the signed zero, after the float32 cast)
        s = spans[name]
        z = d[s] == 0
        assert (z.sum(1) == 1).all()
        d[s] = np.where(z, f32(zero), d[s])
    perm = np.random.default_rng(7).permutation(R)
    # the first five rays: one of each of these kinds -- of "plain" and "zero_neg" the ray that passes closest to the centre, of "face" the
    # one that heads inwards most steeply, so that the short prefixes hold rays that keep samples
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    score = np.linalg.norm(o64 - (o64 * d64).sum(1, keepdims=True) * d64, axis=1)
    score[kind == "face"] = d64[kind == "face", 0]
    for i, name in enumerate(("inside", "plain", "zero_neg", "face", "away")):
        rest = perm[i:]
        j = i + int(np.argmin(np.where(kind[rest] == name, score[rest], np.inf)))
        perm[[i, j]] = perm[[j, i]]
    o, d, kind = np.ascontiguousarray(o[perm]), np.ascontiguousarray(d[perm]), kind[perm]
    o.setflags(write=False); d.setflags(write=False); kind.setflags(write=False)
    return o, d, kind


@functools.lru_cache(maxsize=None)
def grid():
    """[12,20,16] float32; read-only"""
    rng = np.random.default_rng(99)
    D, H, W = GRID_SHAPE
    g = (0.005 + 0.025 * rng.random(GRID_SHAPE)).astype(f32)
    zz, yy, xx = np.meshgrid(np.linspace(-1, 1, D), np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing="ij")
    block = (np.abs(xx) < 0.62) & (np.abs(yy) < 0.62) & (np.abs(zz) < 0.62)
    keep = block & (rng.random(GRID_SHAPE) < 0.85)
    keep[:, :, W - 1] = True
    g = np.where(keep, g, f32(0)).astype(f32)
    g.setflags(write=False)
    return g


def jitter_table(S, n_rays=R):
    """the explicit jitter table of (S, R): U[0,1) in float32, a few exact 0 among them"""
    rng = np.random.default_rng(1000 + S)
    j = rng.random((n_rays, S), dtype=f32)
    j[rng.random((n_rays, S)) < 0.01] = 0.0
    return j


def pack_mask(mask):
    """[R,S] bool -> [R, ceil(S/64)] uint64, bit k % 64 of word k // 64 is candidate k (bits at k >= S are 0)"""
    n_rays, S = mask.shape
    n_chunks = (S + 63) // 64
    padded = np.zeros((n_rays, n_chunks * 64), bool)
    padded[:, :S] = mask
    return np.packbits(padded.reshape(n_rays, n_chunks, 64), axis=-1, bitorder="little").view("<u8").reshape(n_rays, n_chunks)


def oracle_sampler(marcher, contraction, box, S, jitter=None, n_rays=R, grid_=None):
    """``orc.ray_provider`` on the fixture rays, plus the [R,S] mask it packs by (its own steps, core.py:165-178, through the same
    oracle functions; ``test_sampler_cases`` holds the two against each other).  Returns packed [N,7], info [R,2], mask [R,S], t [N]."""
    from oracle import tinynerf_oracle as orc
    o, d, _ = rays()
    o, d = o[:n_rays], d[:n_rays]
    aabb = BOXES[box]
    g = grid() if grid_ is None else grid_
    kw = dict(marcher=marcher, contraction="aabb" if contraction == "aabb" else "mip360", grid=g, threshold=THRESHOLD, n_samples=S,
              near=NEAR, aabb=aabb, uniform_range=UNIFORM_RANGE, order=ORDER.get(contraction, float("inf")), jitter=jitter)
    packed, info = orc.ray_provider(o, d, **kw)
    if marcher == "aabb":
        t, dl = orc.march_aabb(o, d, aabb, S, NEAR)
    else:
        t, dl = orc.march_unbounded(o, d, S, NEAR, 1e5, UNIFORM_RANGE)
    if jitter is not None:
        t = (t + np.asarray(jitter, f32) * dl).astype(f32)
    pts = (o[:, None, :] + (d[:, None, :] * t[..., None]).astype(f32)).astype(f32)
    if contraction == "aabb":
        c, inside = orc.contract_aabb(pts, aabb)
    else:
        c, inside = orc.contract_mip360(pts, ORDER[contraction])
    mask = orc.occupancy_query(g, c, THRESHOLD)
    if inside is not None:
        mask = mask & inside
    return packed, info, mask, np.ascontiguousarray(np.broadcast_to(t, mask.shape)[mask])


# ---------------------------------------------------------------------------------------------- points for tn_contract
def box_points(box, n=257):
    """[n,3]: on every face of ``box``, at the float32 neighbours of every face (in and out), then random points around the box"""
    aabb = BOXES[box]
    rng = np.random.default_rng(5)
    pts = []
    mid = (aabb[0] + aabb[1]) / 2
    for axis in range(3):
        for side in (0, 1):
            face = aabb[side, axis]
            for v in (face, np.nextafter(face, f32(-np.inf)), np.nextafter(face, f32(np.inf))):
                p = (mid + (rng.random(3).astype(f32) - f32(0.5)) * (aabb[1] - aabb[0]) * f32(0.9)).astype(f32)
                p[axis] = v
                pts.append(p)
    pts.append(aabb[0].copy()); pts.append(aabb[1].copy())                       # two corners: on three faces at once
    rest = (mid + (rng.random((n - len(pts), 3)).astype(f32) - f32(0.5)) * (aabb[1] - aabb[0]) * f32(1.4)).astype(f32)
    return np.concatenate([np.stack(pts), rest]).astype(f32)


def mip_points(n=257):
    """[n,3]: norm exactly 1 in each order and its float32 neighbour above, the origin, 1e30, 3e38, then random points of norm 0.01 .. 100"""
    rng = np.random.default_rng(6)
    up = lambda p: np.nextafter(np.asarray(p, f32), np.asarray(p, f32) * f32(2))          # noqa: E731  (away from zero)
    sp = [(1.0, 0.5, -0.2), (0.6, 0.8, 0.0), (-0.2, -1.0, 0.5), (0.0, 0.0, 1.0)]
    pts = [np.asarray(p, f32) for p in sp] + [up(p) for p in sp]
    pts += [np.zeros(3, f32), np.array([1e30, -2e29, 3e28], f32), np.array([3e38, 1e38, -3e38], f32), np.array([0.0, -3e38, 1.0], f32)]
    rest = _unit(rng.standard_normal((n - len(pts), 3))) * 10.0 ** rng.uniform(-2, 2, (n - len(pts), 1))
    return np.concatenate([np.stack(pts), rest.astype(f32)]).astype(f32)


# ---------------------------------------------------------------------------------------------- points for the trilinear lookup
TRILINEAR_SHAPES = ((12, 20, 16), (1, 5, 9), (5, 1, 3), (4, 7, 1), (2, 2, 2), (1, 1, 1))


def trilinear_grid(shape):
    rng = np.random.default_rng(sum(shape) * 31 + shape[0])
    g = rng.random(shape, dtype=f32)
    g[rng.random(shape) < 0.2] = 0.0
    if g.size == 1:
        g[...] = 0.7
    return g


def trilinear_points(shape, n=4000):
    """[n,3] in (x,y,z) = (w,h,d) order: +-1, exact nodes, the float32 neighbours of +-1, points up to 1.3, 1e30, +-inf and NaN"""
    D, H, W = shape
    rng = np.random.default_rng(D * 400 + H * 20 + W)
    p = (rng.random((n, 3)) * 2.6 - 1.3).astype(f32)
    one = f32(1)
    edge = np.array([one, -one, np.nextafter(one, f32(0)), np.nextafter(one, f32(2)), np.nextafter(-one, f32(0)), np.nextafter(-one, f32(-2))], f32)
    k = n // 4
    p[:k] = edge[rng.integers(0, 6, (k, 3))]                                   # every combination of the six edge values
    sel = rng.random((k, 3)) < 0.5                                             # ... half of the components, the rest inside
    p[:k] = np.where(sel, p[:k], (rng.random((k, 3)) * 2 - 1).astype(f32))
    for axis, size in ((0, W), (1, H), (2, D)):                                # exact nodes: -1 + 2 i / (size - 1)
        if size > 1:
            i = rng.integers(0, size, k)
            p[k:2 * k, axis] = (-1.0 + 2.0 * i / (size - 1)).astype(f32)
        else:
            p[k:2 * k, axis] = rng.choice(np.array([-1.0, 0.0, 1.0, 0.5], f32), k)
    bad = np.array([1e30, -1e30, np.inf, -np.inf, np.nan], f32)
    m = 60
    p[2 * k:2 * k + m, :] = (rng.random((m, 3)) * 2 - 1).astype(f32)
    p[np.arange(2 * k, 2 * k + m), rng.integers(0, 3, m)] = bad[np.arange(m) % 5]
    p[2 * k + m] = np.nan
    p[2 * k + m + 1] = np.inf
    return p


# ---------------------------------------------------------------------------------------------- occupancy refresh
def apply_case(n, step, thr, seed=3):
    """cells (0,1] with exact 1.0 and +0.0, sigmas log-uniform in [1e-4, 1e3] plus the special values; draws whose float64 alpha lies
    within 1e-6 of the threshold are redrawn.  Returns cells, sigmas, alpha64, number of redraws."""
    rng = np.random.default_rng(seed + n)
    cells = (1.0 - rng.random(n)).astype(f32)                                 # (0, 1]
    cells[rng.random(n) < 0.05] = 1.0
    cells[rng.random(n) < 0.05] = 0.0
    sig = (10.0 ** rng.uniform(-4, 3, n)).astype(f32)
    special = np.array([0.0, -0.0, -1.0, 1e30, np.inf, np.nan], f32)
    if n >= 12:
        sig[rng.choice(n, 12, replace=False)] = np.tile(special, 2)
    elif n == 1:
        sig[0] = np.nan
    alpha = lambda s: 1.0 - np.exp(-s.astype(np.float64) * np.float64(f32(step)))            # noqa: E731
    redrawn = 0
    while True:
        close = np.abs(alpha(sig) - np.float64(f32(thr))) <= 1e-6
        if not close.any():
            break
        redrawn += int(close.sum())
        sig[close] = (10.0 ** rng.uniform(-4, 3, int(close.sum()))).astype(f32)
    return cells, sig, alpha(sig), redrawn


COARSEN_SHAPES = ((1, 1, 1), (3, 5, 9), (4, 4, 4), (5, 8, 13), (37, 41, 30))


def coarsen_grid(shape):
    rng = np.random.default_rng(shape[0] * 7 + shape[2])
    g = rng.random(shape, dtype=f32)
    g[rng.random(shape) < 0.03] = -0.3
    if g.size == 1:
        g[...] = -0.3
    return g


def coarsen_ref(g):
    """block b of an axis covers cells 4b .. min(4b + 4, N - 1); the maximum is clamped at 0"""
    D, H, W = g.shape
    out = np.empty(((D + 3) // 4, (H + 3) // 4, (W + 3) // 4), f32)
    for bz in range(out.shape[0]):
        for by in range(out.shape[1]):
            for bx in range(out.shape[2]):
                blk = g[4 * bz:min(4 * bz + 4, D - 1) + 1, 4 * by:min(4 * by + 4, H - 1) + 1, 4 * bx:min(4 * bx + 4, W - 1) + 1]
                out[bz, by, bx] = max(blk.max(), f32(0))
    return out
