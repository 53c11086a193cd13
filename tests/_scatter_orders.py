"""Sample orders that drive every branch of the run-merged plane / grid scatters, and the fp64 references they are checked against.

The K-Planes backward (csrc/kplanes_scatter.h, phase B) walks a tile's 32 samples in order and keeps the partial sums of a RUN of
samples that share a cell in registers.  At each sample the run goes on (same cell) or ends in one of nine ways: x+-1 / y+-1 (two
texels carried into the next run), one of the four diagonals (one texel carried) or a plain flush.  Cell ids live on a padded
(H + 4) x (W + 4) lattice, so a move from clamped column W + 1 to column -2 of the next row is a FALSE x-neighbour (dcell == 1).
The Cobafa backward (csrc/cobafa.hip) merges runs keyed on (voxel base, tap mask) inside 64-sample waves.  I.i.d. random points
almost never form runs, so the families here are built to hit each of those cases, and `kplanes_classes` / `cobafa_runs` count
what a stream actually hits (numpy float32 restatements of the kernels' cell arithmetic).

Coordinates are multiples of 2^-13 (`snap`): then (u + 1) / 2 * (W - 1) is exact in fp32 and in fp64 for every plane or grid up to
513 texels a side and |u| <= 3, so the kernel and the fp64 reference agree on every source index, cell and floor, and the
reference's tolerance only has to cover the weights', products' and sums' roundings.

Exact fixtures: plane side lengths with W - 1 and H - 1 powers of two, coordinates on the half-texel grid of the coarsest side,
plane values in {-1, 0, 1}, small-integer upstream gradients.  Every product and partial sum is then a multiple of 2^-G small
enough for fp32, whatever order the atomics add in; `assert_exact` checks that precondition against the fp64 reference itself.
"""
from __future__ import annotations

import itertools
import zlib
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

QUANT = 2.0 ** -13
TILE_KP, WAVE_CB = 32, 64
PAIRS = ((0, 1), (0, 2), (1, 2))          # (u, v) coordinate of plane p: kplanes_device.h pair_uv, models.py:146
DIRS26 = [d for d in itertools.product((-1, 0, 1), repeat=3) if d != (0, 0, 0)]
KP_CLASSES = ("same", "x+", "x-", "y+", "y-", "++", "-+", "+-", "--", "flush", "false_wrap", "tail", "tile_end")


def snap(x: np.ndarray) -> np.ndarray:
    return (np.round(np.asarray(x, np.float64) / QUANT) * QUANT).astype(np.float32)


def cell_width(res: int) -> float:
    """width of one texel cell in coordinate units, align_corners=True"""
    return 2.0 / max(res - 1, 1)


# ------------------------------------------------------------------------------------------------ order families
def fam_iid(n: int, res: int, rng) -> np.ndarray:
    return rng.uniform(-1.0, 1.0, (n, 3))


def fam_rays26(n: int, res: int, rng) -> np.ndarray:
    """straight rays, 2.5 - 6 samples per cell of the finest axis, cycling through all 26 directions.  Half the rays start on a
    texel corner (every coordinate crosses a cell line at the same step: pure diagonal / axis moves), half anywhere."""
    h = cell_width(res)
    out, k, i = [], 0, 0
    while k < n:
        d = np.array(DIRS26[i % 26], np.float64)
        ln = int(rng.integers(8, 120))
        step = h / rng.uniform(2.5, 6.0)
        if i % 2 == 0:
            o = -1.0 + h * (rng.integers(0, max(res - 1, 1), 3) + rng.uniform(0.01, 0.99))
        else:
            o = -1.0 + h * rng.integers(0, max(res - 1, 1), 3) + h * rng.uniform(0.05, 0.95)
        o = o - d * step * ln / 2
        out.append(o + np.arange(ln)[:, None] * step * d)
        k += ln
        i += 1
    return np.concatenate(out)[:n]


def fam_runs(n: int, res: int, rng, lengths=(32, 45, 64, 70, 97)) -> np.ndarray:
    """piecewise-constant cells: whole tiles in one cell, and runs that straddle 32- and 64-sample boundaries"""
    h = cell_width(res)
    out, k = [], 0
    while k < n:
        ln = int(rng.choice(lengths))
        c = rng.integers(0, max(res - 1, 1), 3)
        out.append(-1.0 + h * (c + rng.uniform(0.05, 0.95, (ln, 3))))
        k += ln
    return np.concatenate(out)[:n]


def _morton(ijk: np.ndarray) -> np.ndarray:
    code = np.zeros(len(ijk), np.int64)
    for b in range(11):
        for a in range(3):
            code |= ((ijk[:, a] >> b) & 1).astype(np.int64) << (3 * b + a)
    return code


def fam_morton(n: int, res: int, rng) -> np.ndarray:
    """i.i.d. points sorted by the Morton code of their cell: the order a spatially sorted training step would hand over"""
    x = fam_iid(n, res, rng)
    ijk = np.clip(np.floor((x + 1.0) / cell_width(res)), 0, 2047).astype(np.int64)
    return x[np.argsort(_morton(ijk), kind="stable")]


def fam_rowmajor(n: int, res: int, rng) -> np.ndarray:
    x = fam_iid(n, res, rng)
    ijk = np.clip(np.floor((x + 1.0) / cell_width(res)), 0, 2047).astype(np.int64)
    return x[np.lexsort((ijk[:, 0], ijk[:, 1], ijk[:, 2]))]


def fam_back_and_forth(n: int, res: int, rng) -> np.ndarray:
    """every sample jumps between two neighbouring cells, for each of the 26 moves (all plane pairs see x+-, y+- and diagonals)"""
    h = cell_width(res)
    out, k, i = [], 0, 0
    while k < n:
        d = np.array(DIRS26[i % 26], np.float64)
        ln = int(rng.integers(10, 80))
        c = rng.integers(1, max(res - 2, 2), 3)
        a = -1.0 + h * (c + rng.uniform(0.1, 0.9, 3))
        pts = np.where((np.arange(ln) % 2 == 0)[:, None], a, a + h * d)
        out.append(pts + h * rng.uniform(-0.05, 0.05, (ln, 3)))
        k += ln
        i += 1
    return np.concatenate(out)[:n]


_EDGES = np.array([-3.0, -1.0 - 2.0 ** -10, -1.0, -1.0 + 2.0 ** -10, 1.0 - 2.0 ** -10, 1.0, 1.0 + 2.0 ** -10, 3.0])


def fam_leave_reenter(n: int, res: int, rng) -> np.ndarray:
    """rays that leave the plane and come back in, plus points exactly at +-1, +-1 +- 2^-10 and far outside (+-3)"""
    h = cell_width(res)
    out, k = [], 0
    while k < n:
        ln = int(rng.integers(20, 90))
        o = rng.uniform(-1.0, 1.0, 3)
        d = rng.choice([-1.0, 0.0, 1.0], 3)
        d[rng.integers(0, 3)] = rng.choice([-1.0, 1.0])
        t = np.abs(np.arange(ln) - ln / 2) * h / 2.0 * 4.0          # out and back along the same line
        seg = o + t[:, None] * d
        e = rng.integers(0, len(_EDGES), (ln, 3))
        hit = rng.random((ln, 3)) < 0.3
        seg = np.where(hit, _EDGES[e], seg)
        out.append(seg)
        k += ln
    return np.concatenate(out)[:n]


def row_wrap_pairs(H: int, W: int) -> np.ndarray:
    """for each plane pair p: (row r, column W + 1 (clamped)) -> (row r + 1, column -2 (clamped)): dcell == +1 between two cells that
    are not neighbours, and back.  Coordinates for the padded rows -2 .. H + 1 on the v axis."""
    hu, hv = cell_width(W), cell_width(H)
    pts = []
    for p, (a, b) in enumerate(PAIRS):
        for r in range(-2, H + 1):
            right, left = np.zeros(3), np.zeros(3)
            right[a], left[a] = 7.0, -7.0                     # columns clamp to W + 1 / -2 (W = 2 included)
            right[b] = -1.0 + hv * (r + 0.5)
            left[b] = -1.0 + hv * (r + 1.5)
            third = 3 - a - b
            right[third] = left[third] = 0.25
            pts += [right, left, right, left, left]
        # and a pair of real cells at the row ends (column W - 1 -> column 0 of the next row is NOT a neighbour either)
        for r in range(0, H - 1):
            e, s = np.zeros(3), np.zeros(3)
            e[a] = -1.0 + hu * (W - 1.5)
            s[a] = -1.0 + hu * 0.5
            e[b], s[b] = -1.0 + hv * (r + 0.5), -1.0 + hv * (r + 1.5)
            pts += [e, s]
    return np.array(pts)


def fam_row_wrap(n: int, res: int, rng, shapes: Sequence[Tuple[int, int]] = ()) -> np.ndarray:
    base = np.concatenate([row_wrap_pairs(H, W) for H, W in (shapes or [(res, res)])])
    reps = -(-n // len(base))
    x = np.concatenate([base] * reps)[:n]
    return x + rng.uniform(-1e-4, 1e-4, x.shape) * (np.abs(x) < 2.0)


def fam_texel_lines(n: int, res: int, rng) -> np.ndarray:
    """coordinates exactly on texel lines and corners (fx == 0 or fy == 0), moving one texel at a time"""
    h = cell_width(res)
    idx = rng.integers(0, res, (n, 3)).astype(np.float64)
    walk = np.cumsum(rng.integers(-1, 2, (n, 3)), 0) % res
    idx = np.where(np.arange(n)[:, None] % 64 < 32, walk, idx)
    x = -1.0 + h * idx
    half = rng.random((n, 3)) < 0.3                              # some coordinates half-way: corners, edges and plain lines
    return np.where(half, x + h / 2, x)


def fam_mixed(n: int, res: int, rng) -> np.ndarray:
    """all families in short interleaved chunks (the ragged tail included)"""
    fams = [f for k, f in FAMILIES.items() if k != "mixed"]
    out, k = [], 0
    while k < n:
        f = fams[int(rng.integers(0, len(fams)))]
        m = int(rng.integers(1, 200))
        out.append(f(m, res, rng))
        k += m
    return np.concatenate(out)[:n]


FAMILIES = {
    "iid": fam_iid, "rays26": fam_rays26, "runs": fam_runs, "morton": fam_morton, "rowmajor": fam_rowmajor,
    "back_and_forth": fam_back_and_forth, "leave_reenter": fam_leave_reenter, "row_wrap": fam_row_wrap,
    "texel_lines": fam_texel_lines, "mixed": fam_mixed,
}
SIZES = (1, 31, 32, 33, 1000 + 17, 262144 + 4096 + 5)        # the last: the stand-alone kernel's persistent tile loop, second round


def seed_of(*parts) -> int:
    """a seed that does not depend on the interpreter's string hashing"""
    return zlib.crc32(repr(parts).encode()) % 100000


def stream(family: str, n: int, shapes: Sequence[Tuple[int, int]], seed: int) -> np.ndarray:
    """n coordinates of one family; step sizes follow the finest side of `shapes` ((H, W) per scale), the row-wrap family covers
    every shape"""
    rng = np.random.default_rng(seed)
    res = max(max(s) for s in shapes)
    f = FAMILIES[family]
    x = f(n, res, rng, shapes) if family == "row_wrap" else f(n, res, rng)
    return snap(x)


# ------------------------------------------------------------------------------------------------ kernels' cell arithmetic
def plane_cells(u: np.ndarray, v: np.ndarray, H: int, W: int) -> np.ndarray:
    """float32 restatement of plane_taps' cell id (kplanes_device.h)"""
    f32 = np.float32
    u, v = np.asarray(u, f32), np.asarray(v, f32)
    ix = ((u + f32(1)) * f32(0.5)) * f32(W - 1)
    iy = ((v + f32(1)) * f32(0.5)) * f32(H - 1)
    cx = np.clip(np.floor(ix), -2, W + 1).astype(np.int64)
    cy = np.clip(np.floor(iy), -2, H + 1).astype(np.int64)
    return (cy + 2) * (W + 4) + cx + 2


def kplanes_classes(x: np.ndarray, H: int, W: int, p: int) -> Dict[str, int]:
    """how often phase B of kp_scatter_scale takes each branch for plane pair p of an [H, W] scale (tiles of 32 samples)"""
    n = len(x)
    a, b = PAIRS[p]
    cell = plane_cells(x[:, a], x[:, b], H, W)
    rowlen = W + 4
    j = np.arange(n) % TILE_KP
    nxt = np.arange(n) + 1
    inner = (j < TILE_KP - 1) & (nxt < n)
    d = np.zeros(n, np.int64)
    d[inner] = cell[nxt[inner]] - cell[inner]
    cnt = {k: 0 for k in KP_CLASSES}
    cnt["tile_end"] = int(np.count_nonzero(j == TILE_KP - 1))
    cnt["tail"] = int(np.count_nonzero((j < TILE_KP - 1) & (nxt >= n)))
    di = d[inner]
    moves = {"same": 0, "x+": 1, "x-": -1, "y+": rowlen, "y-": -rowlen, "++": rowlen + 1, "-+": rowlen - 1, "+-": -rowlen + 1,
             "--": -rowlen - 1}
    for k, m in moves.items():
        cnt[k] = int(np.count_nonzero(di == m))
    cnt["flush"] = int(np.count_nonzero(~np.isin(di, list(moves.values()))))
    col = cell[inner] % rowlen
    cnt["false_wrap"] = int(np.count_nonzero((di == 1) & (col == rowlen - 1)))
    return cnt


def _sawtooth(x: np.ndarray, f: float) -> np.ndarray:
    if f <= 0:
        return x
    v = np.float32(f) * x
    return np.float32(2) * (v - np.floor(v)) - np.float32(1)


def grid_keys(p: np.ndarray, D: int, H: int, W: int) -> np.ndarray:
    """float32 restatement of cobafa.hip cell3's run key (voxel base, tap mask) as one int64"""
    f32 = np.float32
    p = np.asarray(p, f32)
    i = [((p[:, c] + f32(1)) * f32(0.5)) * f32(s - 1) for c, s in enumerate((W, H, D))]
    x0, y0, z0 = (np.floor(v).astype(np.int64) for v in i)
    m = np.zeros(len(p), np.int64)
    for k in range(8):
        cx, cy, cz = x0 + (k & 1), y0 + ((k >> 1) & 1), z0 + (k >> 2)
        ok = (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H) & (cz >= 0) & (cz < D)
        m |= ok.astype(np.int64) << k
    base = np.where(m != 0, (z0 * H + y0) * W + x0, 0)
    return base * 256 + m


def cobafa_runs(x: np.ndarray, grids: Sequence[Tuple[Tuple[int, int, int], float]]) -> Dict[str, int]:
    """per lookup (grid resolution (D, H, W), sawtooth frequency; 0 = the coefficient grid): runs that cross a 64-sample wave
    boundary, merged samples, and waves whose end-of-wave flush carries a run of two or more samples"""
    out = {"cross_wave": 0, "merged": 0, "end_mid_run": 0, "lookups": len(grids)}
    n = len(x)
    for (D, H, W), f in grids:
        key = grid_keys(_sawtooth(np.asarray(x, np.float32), f), D, H, W)
        same = key[1:] == key[:-1]
        pos = np.arange(1, n)
        out["merged"] += int(np.count_nonzero(same & (pos % WAVE_CB != 0)))
        out["cross_wave"] += int(np.count_nonzero(same & (pos % WAVE_CB == 0)))
        last = np.arange(WAVE_CB - 1, n, WAVE_CB)
        out["end_mid_run"] += int(np.count_nonzero(key[last] == key[last - 1]))
    return out


# ------------------------------------------------------------------------------------------------ exact fixtures
def is_pow2(v: int) -> bool:
    return v >= 1 and (v & (v - 1)) == 0


def exact_coords(x: np.ndarray, sides: Sequence[int]) -> np.ndarray:
    """snap to the half-texel grid of the COARSEST side (all sides - 1 powers of two): fx in {0, 1/2} there, fx == 0 on the finer
    sides -- every weight is then 0, 1/4, 1/2 or 1"""
    assert all(is_pow2(s - 1) for s in sides), sides
    q = 1.0 / min(s - 1 for s in sides)             # (u + 1) / 2 on multiples of q / 2
    return (np.round((np.asarray(x, np.float64) + 1.0) / q) * q - 1.0).astype(np.float32)


def exact_values(shape, rng, lo: int = -1, hi: int = 1) -> np.ndarray:
    return rng.integers(lo, hi + 1, shape).astype(np.float32)


def dyadic_bits(a) -> int:
    """the least k with a * 2^k integral everywhere (fp64 input)"""
    a = np.asarray(a, np.float64).ravel()
    for k in range(0, 60):
        s = a * 2.0 ** k
        if np.array_equal(s, np.round(s)):
            return k
    raise AssertionError("not a dyadic fixture")


def assert_exact(ref: np.ndarray, abs_ref: np.ndarray, bits: int, name: str = "") -> None:
    """every term and every partial sum, in any order, is a multiple of 2^-bits bounded by sum |terms|: exact in fp32 when that
    sum times 2^bits stays below 2^24; the fp64 reference must then be its own fp32 rounding"""
    ref, abs_ref = np.asarray(ref, np.float64), np.asarray(abs_ref, np.float64)
    assert float(abs_ref.max(initial=0.0)) * 2.0 ** bits < 2.0 ** 24, (name, bits, float(abs_ref.max(initial=0.0)))
    assert np.array_equal(ref, ref.astype(np.float32).astype(np.float64)), name
    s = ref * 2.0 ** bits
    assert np.array_equal(s, np.round(s)), name


# ------------------------------------------------------------------------------------------------ fp64 references (torch, CPU)
def _gs2(plane: torch.Tensor, u: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """[1, C, H, W] plane, n points -> [n, C]; align_corners=True, zeros padding (models.py:105-113)"""
    g = torch.stack([u, v], -1).view(1, -1, 1, 2)
    return torch.nn.functional.grid_sample(plane, g, mode="bilinear", padding_mode="zeros", align_corners=True)[0, :, :, 0].t()


def kplanes_ref(x: np.ndarray, planes: Sequence, g: np.ndarray):
    """fp64 features, plane gradients and the same two on |planes|, |g| (the per-texel sums of |terms|).  planes: list of [H, W, C]
    arrays per (scale, pair), None = absent (factor 1); g: [n, S*C]; x: [n, 3], or one [n, 3] per scale.  Returns feat, abs_feat, grads, abs_grads (None entries kept)."""
    S = len(planes) // 3
    xs = [torch.as_tensor(np.asarray(xx, np.float64)) for xx in (x if isinstance(x, (list, tuple)) else [x] * S)]
    res = []
    for absolute in (False, True):
        pl = [None if p is None else torch.as_tensor(np.asarray(p, np.float64)).permute(2, 0, 1)[None].clone().requires_grad_(True)
              for p in planes]
        if absolute:
            pl = [None if p is None else p.detach().abs().requires_grad_(True) for p in pl]
        feats = []
        for s in range(S):
            prod = None
            for p, (a, b) in enumerate(PAIRS):
                if pl[3 * s + p] is None:
                    continue
                v = _gs2(pl[3 * s + p], xs[s][:, a], xs[s][:, b])
                prod = v if prod is None else prod * v
            feats.append(prod)
        feat = torch.cat(feats, -1)
        gt = torch.as_tensor(np.asarray(g, np.float64))
        if absolute:
            gt = gt.abs()
        live = [p for p in pl if p is not None]
        gr = torch.autograd.grad(feat, live, gt)
        it = iter(gr)
        grads = [None if p is None else next(it)[0].permute(1, 2, 0).numpy() for p in pl]
        res.append((feat.detach().numpy(), grads))
    (feat, grads), (afeat, agrads) = res
    return feat, afeat, grads, agrads


def tap_counts(x: np.ndarray, H: int, W: int, p: int) -> np.ndarray:
    """[H, W] number of samples whose bilinear footprint on plane pair p includes the texel (bincount of tap indices)"""
    a, b = PAIRS[p]
    x64 = np.asarray(x, np.float64)
    ix = (x64[:, a] + 1.0) / 2.0 * (W - 1)
    iy = (x64[:, b] + 1.0) / 2.0 * (H - 1)
    x0, y0 = np.floor(ix).astype(np.int64), np.floor(iy).astype(np.int64)
    cnt = np.zeros(H * W, np.int64)
    for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        tx, ty = x0 + dx, y0 + dy
        ok = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
        cnt += np.bincount((ty * W + tx)[ok], minlength=H * W)
    return cnt.reshape(H, W)


def cobafa_ref(x: np.ndarray, coef: np.ndarray, basis: Sequence[np.ndarray], freqs: Sequence[float], g: np.ndarray):
    """fp64 Cobafa features / gradients (models.py:209-266) and the same on |grids|, |g|.  coef [D, H, W, L], basis[l] [D, H, W, C_l]."""
    xt = torch.as_tensor(np.asarray(x, np.float64))
    res = []
    for absolute in (False, True):
        mk = lambda a: torch.as_tensor(np.abs(a) if absolute else a, dtype=torch.float64).permute(3, 0, 1, 2)[None].clone().requires_grad_(True)
        cg, bg = mk(coef), [mk(b) for b in basis]
        look = lambda grid, pts: torch.nn.functional.grid_sample(grid, pts.view(1, -1, 1, 1, 3), mode="bilinear", padding_mode="zeros",
                                                                 align_corners=True)[0, :, :, 0, 0].t()
        cv = look(cg, xt)
        feats = []
        for l, (b, f) in enumerate(zip(bg, freqs)):
            y = 2.0 * torch.remainder(f * xt, 1.0) - 1.0 if f > 0 else xt
            feats.append(look(b, y) * cv[:, l:l + 1])
        feat = torch.cat(feats, -1)
        gt = torch.as_tensor(np.abs(g) if absolute else g, dtype=torch.float64)
        grads = torch.autograd.grad(feat, [cg, *bg], gt)
        res.append((feat.detach().numpy(), [t[0].permute(1, 2, 3, 0).numpy() for t in grads]))
    (feat, grads), (afeat, agrads) = res
    return feat, afeat, grads, agrads


def grid_tap_counts(p: np.ndarray, D: int, H: int, W: int) -> np.ndarray:
    """[D, H, W] number of lookups whose trilinear footprint includes the voxel"""
    p = np.asarray(p, np.float64)
    i = [(p[:, c] + 1.0) / 2.0 * (s - 1) for c, s in enumerate((W, H, D))]
    x0, y0, z0 = (np.floor(v).astype(np.int64) for v in i)
    cnt = np.zeros(D * H * W, np.int64)
    for k in range(8):
        cx, cy, cz = x0 + (k & 1), y0 + ((k >> 1) & 1), z0 + (k >> 2)
        ok = (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H) & (cz >= 0) & (cz < D)
        cnt += np.bincount(((cz * H + cy) * W + cx)[ok], minlength=D * H * W)
    return cnt.reshape(D, H, W)


def sawtooth64(x: np.ndarray, f: float) -> np.ndarray:
    x = np.asarray(x, np.float64)
    return 2.0 * np.mod(f * x, 1.0) - 1.0 if f > 0 else x


def source_index_coords(x: np.ndarray, side: int) -> np.ndarray:
    """fp64 coordinates whose align_corners=True source index on a side of `side` texels is the one fp32 computes from x (one rounding
    per operation, as ATen and plane_taps do): a reference for coordinates that are not exact in fp32"""
    f32 = np.float32
    ix = ((np.asarray(x, f32) + f32(1)) * f32(0.5)) * f32(side - 1)
    return ix.astype(np.float64) * 2.0 / (side - 1) - 1.0


def assert_within(got, ref, abs_ref, m, rounds: int, name: str = "", atol: float = 1e-30) -> None:
    """|got - ref| <= (m + rounds) * 2^-24 * A per element, A = the reference on |inputs| (sum of |terms|), m = terms summed there:
    a bound from the inputs alone.  `rounds` counts the roundings of one term before it is summed (see the callers).  Where A == 0
    nothing may arrive at all."""
    got, ref, abs_ref = (np.asarray(a, np.float64) for a in (got, ref, abs_ref))
    m = np.broadcast_to(np.asarray(m, np.float64), ref.shape)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.isfinite(got).all(), name
    bound = (m + rounds) * 2.0 ** -24 * abs_ref * (1.0 + 2.0 ** -10) + atol
    err = np.abs(got - ref)
    bad = err > bound
    if bad.any():
        i = np.unravel_index(int(np.argmax(np.where(bad, err / bound, 0))), ref.shape)
        raise AssertionError(f"{name}: {int(bad.sum())} of {ref.size} elements outside (m + {rounds}) 2^-24 A; worst at {i}: got "
                             f"{got[i]!r} ref {ref[i]!r} A {abs_ref[i]!r} m {m[i]}")
    stray = (abs_ref == 0) & (np.abs(got) > atol)
    assert not stray.any(), f"{name}: {int(stray.sum())} elements receive a value where no term lands"


# ------------------------------------------------------------------------------------------------ the cases the GPU tests run
# K-Planes stand-alone: name -> (channels, [(H, W) per scale], single-plane lookup).  General fixtures take any side lengths, exact
# ones need W - 1, H - 1 powers of two (the reference resolutions 128 / 256 / 512 become 129 / 257 / 513 there).
KP_GENERAL = {
    "c32_s3_square": (32, [(17, 17), (33, 33), (65, 65)], False),
    "c8_s1_2x2": (8, [(2, 2)], False),
    "c16_s2_nonsquare": (16, [(33, 9), (9, 33)], False),
    "c8_s4_mixed": (8, [(9, 17), (17, 2), (2, 9), (40, 23)], False),
    "c32_s3_reference": (32, [(128, 128), (256, 256), (512, 512)], False),
    "c16_single_plane": (16, [(33, 17)], True),
}
KP_EXACT = {
    "c32_s3_square": (32, [(17, 17), (17, 17), (17, 17)], False),
    "c8_s1_2x2": (8, [(2, 2)], False),
    "c16_s2_nonsquare": (16, [(33, 9), (9, 33)], False),
    "c8_s4_mixed": (8, [(9, 17), (17, 5), (5, 9), (9, 9)], False),
    "c32_s3_reference": (32, [(129, 129), (257, 257), (513, 513)], False),
    "c16_single_plane": (16, [(33, 17)], True),
}
N_GENERAL, N_EXACT = (1 << 14) + 13, 6000 + 7
# Cobafa: name -> (coef (D, H, W), [(basis (D, H, W), freq, channels) per level]).  Power-of-two frequencies: f * x is exact, so the
# sawtooth's wrap lands on the same sample in fp32 and fp64.
CB_GENERAL = {
    "l6": ((33, 17, 9), [((9, 9, 9), 1.0, 1), ((5, 17, 9), 2.0, 2), ((17, 5, 5), 4.0, 3), ((3, 3, 3), 1.0, 4),
                         ((33, 9, 9), 2.0, 8), ((2, 2, 2), 8.0, 5)]),
    "l1": ((5, 5, 5), [((17, 17, 17), 1.0, 8)]),
    "l3": ((9, 9, 9), [((65, 9, 5), 0.5, 8), ((9, 9, 9), 2.0, 1), ((3, 17, 33), 1.0, 4)]),
    "l8": ((17, 17, 17), [((9, 9, 9), 1.0, 1), ((5, 5, 5), 2.0, 2), ((17, 9, 5), 4.0, 3), ((3, 5, 9), 8.0, 4),
                          ((9, 9, 9), 1.0, 5), ((2, 3, 5), 2.0, 6), ((33, 17, 9), 1.0, 7), ((5, 9, 17), 2.0, 8)]),
}
CB_EXACT = {
    "l6": ((17, 9, 9), [((9, 9, 9), 1.0, 1), ((5, 9, 5), 2.0, 2), ((3, 3, 3), 4.0, 3), ((9, 5, 9), 1.0, 4),
                        ((17, 9, 9), 1.0, 8), ((2, 2, 2), 8.0, 5)]),
    "l1": ((5, 5, 5), [((9, 9, 9), 1.0, 8)]),
    "l3": ((9, 9, 9), [((9, 5, 3), 1.0, 8), ((5, 5, 5), 2.0, 1), ((3, 9, 17), 1.0, 4)]),
    "l8": ((9, 9, 9), [((9, 9, 9), 1.0, 1), ((5, 5, 5), 2.0, 2), ((9, 9, 5), 1.0, 3), ((3, 5, 9), 1.0, 4),
                       ((9, 9, 9), 1.0, 5), ((2, 3, 5), 2.0, 6), ((17, 9, 9), 1.0, 7), ((5, 9, 17), 1.0, 8)]),
}
N_COBAFA = (1 << 13) + 29


def kp_fixture(cases: dict, name: str, family: str, n: int, seed: int):
    """(x [n, 3], planes: [H, W, C] float32 arrays per (scale, pair), None = absent, g [n, S*C], exact) for one case / family"""
    C, shapes, single = cases[name]
    exact = cases is KP_EXACT
    rng = np.random.default_rng(seed)
    x = stream(family, n, shapes, seed)
    planes: List = []
    for H, W in shapes:
        for p in range(3):
            if single and p > 0:
                planes.append(None)
            elif exact:
                planes.append(exact_values((H, W, C), rng))
            else:
                planes.append(rng.uniform(-1.0, 1.0, (H, W, C)).astype(np.float32))
    if exact:
        x = exact_coords(x, [s for hw in shapes for s in hw])
        g = exact_values((n, len(shapes) * C), rng, -2, 2)
    else:
        g = (rng.standard_normal((n, len(shapes) * C)) * np.exp(rng.uniform(-3, 3, (n, 1)))).astype(np.float32)
    if single:
        x[:, 2] = 0.0                           # KPlanesFeaturePlane's lookups: (x, y, 0)
    return x, planes, g, exact


def kp_exact_bits(x: np.ndarray, shapes, planes, g: np.ndarray) -> Tuple[int, int]:
    """(feature bits, gradient-term bits): every interpolation weight of pair p is a multiple of 2^-(bits(ix) + bits(iy))"""
    x64 = np.asarray(x, np.float64)
    fb = tb = 0
    for s, (H, W) in enumerate(shapes):
        w = 0
        for p, (a, b) in enumerate(PAIRS):
            if planes[3 * s + p] is None:
                continue
            w += dyadic_bits((x64[:, a] + 1.0) / 2.0 * (W - 1)) + dyadic_bits((x64[:, b] + 1.0) / 2.0 * (H - 1))
        fb, tb = max(fb, w), max(tb, w + dyadic_bits(g))
    return fb, tb


def cb_fixture(cases: dict, name: str, family: str, n: int, seed: int):
    """(x, coef [D, H, W, L], basis [D, H, W, C_l] per level, freqs, g [n, sum C_l], exact)"""
    cres, levels = cases[name]
    exact = cases is CB_EXACT
    rng = np.random.default_rng(seed)
    sides = [s for s in cres] + [s for r, _, _ in levels for s in r]
    x = stream(family, n, [(max(sides), max(sides))], seed)
    mk = (lambda shape: exact_values(shape, rng)) if exact else (lambda shape: rng.uniform(-1.0, 1.0, shape).astype(np.float32))
    coef = mk((*cres, len(levels)))
    basis = [mk((*r, c)) for r, _, c in levels]
    F = sum(c for _, _, c in levels)
    if exact:
        x = exact_coords(x, list(cres))
        g = exact_values((n, F), rng, -2, 2)
    else:
        g = (rng.standard_normal((n, F)) * np.exp(rng.uniform(-3, 3, (n, 1)))).astype(np.float32)
    return x, coef, basis, [f for _, f, _ in levels], g, exact


def cb_exact_bits(x: np.ndarray, cres, levels, g: np.ndarray) -> Tuple[int, int]:
    def wbits(pts, res):
        return sum(dyadic_bits((pts[:, c] + 1.0) / 2.0 * (s - 1)) for c, s in enumerate(reversed(res)))
    x64 = np.asarray(x, np.float64)
    bc = wbits(x64, cres)
    bl = max(wbits(sawtooth64(x64, f), r) for r, f, _ in levels)
    return bc + bl, bc + bl + dyadic_bits(g)
