"""Sizes, fixtures and forward-only fp64 references for the per-sample tests of the fused K-Planes launches
(tests/test_hip_kplanes_fused.py; tests/test_kplanes_fused_cases.py checks this module on the CPU).

Launches (csrc/mlp.hip plan_fwd, csrc/mlp_bwd2.hip launch_chain; grids from csrc/mlp_stage.h):

    name               entry point                              waves  grid
    train_f16x2        tn_kplanes_mlp_fwd_pair, stashed, f16x2    8    grid_blocks(n, 8, 256)       (TN_F2_KP_WAVES)
    train_fp32         tn_kplanes_mlp_fwd_pair, stashed, fp32    12    grid_blocks(n, 12, 256)
    chain              tn_kplanes_mlp_bwd_pair, chain + scatter   8    grid_blocks(n, 8, 256)       (WPK)
    infer_pair_f16x2   tn_kplanes_mlp_fwd_pair, no workspaces     8    grid_per_cu(n, 8, lds)
    infer_pair_fp32    tn_kplanes_mlp_fwd_pair, no workspaces    12    grid_per_cu(n, 12, lds)
    infer_sigma        tn_kplanes_mlp_fwd, either arithmetic     12    grid_per_cu(n, 12, lds)

`grid_blocks(n, waves, cap)` = min(ceil(ceil(n / 32) / waves), cap) blocks of `waves` 32-sample tiles; a block walks tiles
blockIdx * waves + wave, + gridDim * waves, ...: with the cap reached, ROUND r of that loop covers samples [r, r + 1) * cap * waves * 32.
`grid_per_cu(n, waves, lds)` = grid_blocks(n, waves, 256 * per_cu), per_cu = max(1, min(160 KiB / lds, 2048 / (waves * 64))).

Derivations.
* Workgroup edges: 32 * waves - 1, 32 * waves, 32 * waves + 1 samples -- one block whose last wave has one sample missing, a full
  block, a second block of one sample (255 / 256 / 257 for 8 waves, 383 / 384 / 385 for 12).
* Second round, training forward and chain (cap 256): 256 * waves * 32 + 37 = 65 573 (8 waves) or 98 341 (12 waves): round 1 holds
  two tiles, the second of them ragged (5 samples).
* Second round, inference launches: `lds` is the staged weights of the launch's heads.  `lds_bytes` restates lay_out_lds
  (mlp_stage.h: fp32 rows of K_pad + 4 floats and a bias per layer) and plan_f2 (mlp_f2_heads.h: two fp16 planes of rows of
  K_pad16 + 8 halfs per hidden layer, the fp32 last layer, scales) for the two fixed heads, colour 147 -> 64 x 4 -> 3 and sigma
  96 -> 64 -> 1: pair 94 016 + 26 144 = 120 160 B (fp32) or 100 336 + 27 312 = 127 648 B (f16x2), sigma alone 26 144 / 27 312 B.
  So per_cu = min(160 KiB / lds, 2048 / (waves * 64)) is 1 for both pair forms and 2 for the sigma launch (`per_cu`).  That
  restatement is not checked against the library (no query returns the bytes and none is added for a test), so the second-round n
  does not lean on it: it is built from the LARGEST per_cu the thread limit allows, 2048 / (waves * 64) = 4 (8 waves) or 2 (12
  waves): n = 256 * 4 * 8 * 32 + 37 = 262 181 and 256 * 2 * 12 * 32 + 37 = 196 645 exceed one round for EVERY per_cu in 1 .. 4
  (1 .. 2), so all three launches reach a later round and end in a ragged tile for certain.  With the derived per_cu (1, 1, 2)
  sample 262 144 / 196 608 / 196 608 opens a round -- the fifth, the third, the second -- whose only tiles are the last two.
* A round of an 8-wave launch ends at a multiple of 65 536 * per_cu, of a 12-wave launch at a multiple of 98 304 * per_cu;
  `ROUND_EDGES` lists the first round's end for every per_cu either can have -- 65 536, 131 072, 196 608, 262 144 and 98 304
  (, 196 608) -- and every fixture long enough gets planted samples in the tile before and in the tile behind each.

Planted edge samples.  The "mixed" order family alone puts no out-of-range sample into tile 0 or into the last tile at these sizes,
so `plant` overwrites one coordinate (0, 1, 2 in turn) of chosen samples with the values of _scatter_orders._EDGES (-3, -1 - 2^-10,
-1, -1 + 2^-10, 1 - 2^-10, 1, 1 + 2^-10, 3; snapped with exact_coords in the exact fixture): the first and the last sample of tile
0, every sample of the last tile, and every sample of the tile before and of the tile behind each round edge.  The k-th planted
sample (in index order) takes coordinate k % 3 and the values in turn (`planted_values`): 24 consecutive ones take every
(coordinate, value) pair once, sample 0 and sample n - 1 straddle an edge.
`tap_classes` names what a sample's footprints do -- "inside", "straddle" (some plane reads both real texels and taps outside, weight
0) and "outside" (a plane with all four taps outside: that scale's factor and with it the product is 0).  A sample whose planted
coordinate is +-3 is "outside" for every scale: its whole feature row is exactly 0, and so is A there (nothing may arrive).

Probe positions of the backward (`probes`): 0, 31, 32, n - 1, the last sample of the first round, the first of the second, and one
sample in the middle of the last tile, clipped to n, duplicates removed.

Out of scope here: plane_gather reads texel 0 with weight 0 for a tap outside the plane, so a non-finite texel 0 reaches such a sample
as NaN where ATen's grid_sample reads nothing.  Fixtures keep their planes finite; that path is neither tested nor changed.
"""
from __future__ import annotations

import functools
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

import _scatter_orders as so

TILE, CUS, LDS_LIMIT_BYTES, CU_THREADS = 32, 256, 160 * 1024, 2048

# launch -> (waves per block, blocks per CU the grid is capped at: 1 = grid_blocks(n, waves, 256), None = grid_per_cu)
LAUNCHES: Dict[str, Tuple[int, int | None]] = {
    "train_f16x2": (8, 1), "train_fp32": (12, 1), "chain": (8, 1),
    "infer_pair_f16x2": (8, None), "infer_pair_fp32": (12, None), "infer_sigma": (12, None),
}


def grid_blocks(n: int, waves: int, cap: int) -> int:
    return min(((n + TILE - 1) // TILE + waves - 1) // waves, cap)


def per_cu_max(waves: int) -> int:
    return CU_THREADS // (waves * 64)


def grid_per_cu(n: int, waves: int, lds: int) -> int:
    return grid_blocks(n, waves, CUS * max(1, min(LDS_LIMIT_BYTES // lds, per_cu_max(waves))))


HEAD_DIMS = {"colour": (147, 64, 64, 64, 64, 3), "sigma": (96, 64, 1)}       # [PE_8(d), d, feat] -> rgb; feat -> sigma


def lds_bytes(dims: Sequence[int], f2: bool) -> int:
    """staged weights of one width-64 head with <= 4 outputs: lay_out_lds (fp32) / plan_f2 (f16x2), in bytes"""
    L, H, out = len(dims) - 1, dims[1], dims[-1]
    k0 = (dims[0] + 7) & ~7
    off = 0
    if f2:
        for l in range(L - 1):
            kp = ((k0 if l == 0 else H) + 15) & ~15
            off += H * (kp + 8) + H
        off += out * (H + 4) + 4 + 2 * L + 32
        return ((off + 3) & ~3) * 4
    for l in range(L):
        rows = out if l == L - 1 else H
        off += rows * ((k0 if l == 0 else H) + 4) + ((rows + 3) & ~3)
    return off * 4


def per_cu(launch: str) -> int:
    """blocks per CU of the launch's grid cap: 1 for grid_blocks(n, waves, 256), grid_per_cu's answer for the inference launches"""
    waves, pc = LAUNCHES[launch]
    if pc is not None:
        return pc
    f2 = launch.endswith("f16x2")
    if launch == "infer_sigma":         # 12 waves in either arithmetic; the larger of the two footprints decides nothing here
        lds = max(lds_bytes(HEAD_DIMS["sigma"], False), lds_bytes(HEAD_DIMS["sigma"], True))
    else:
        lds = lds_bytes(HEAD_DIMS["colour"], f2) + lds_bytes(HEAD_DIMS["sigma"], f2)
    return max(1, min(LDS_LIMIT_BYTES // lds, per_cu_max(waves)))


def round_samples(launch: str) -> int:
    """samples of one round of the launch's persistent tile loop with the grid at its cap (inference: at the largest cap the thread
    limit allows, a multiple of the round at the derived per_cu)"""
    waves, pc = LAUNCHES[launch]
    return CUS * (pc if pc is not None else per_cu_max(waves)) * waves * TILE


def second_round_n(launch: str) -> int:
    return round_samples(launch) + TILE + 5


def sizes(launch: str) -> List[int]:
    w = LAUNCHES[launch][0]
    return [1, 31, 32, 33, TILE * w - 1, TILE * w, TILE * w + 1, second_round_n(launch)]


# size keys the GPU tests are parametrised with: the same eight cases for every launch, resolved with its wave count
SIZE_KEYS = ("1", "31", "32", "33", "wg-1", "wg", "wg+1", "round2")
SMALL_KEYS = SIZE_KEYS[:-1]


def size_of(launch: str, key: str) -> int:
    return sizes(launch)[SIZE_KEYS.index(key)]


# the end of the first round for every wave count and every per_cu it can have
ROUND_EDGES = tuple(sorted({CUS * pc * w * TILE for w, _ in LAUNCHES.values() for pc in range(1, per_cu_max(w) + 1)}))


def planted_positions(n: int) -> np.ndarray:
    last = (n - 1) // TILE * TILE
    pos = {0, min(TILE - 1, n - 1), *range(last, n)}
    for e in ROUND_EDGES:
        if e < n:
            pos.update(range(e - TILE, min(e + TILE, n)))
    return np.array(sorted(pos), np.int64)


# the order the planted values are taken in: a straddling value first (index into _scatter_orders._EDGES: 1 + 2^-10, -3, -1 - 2^-10, 1, 3, -1,
# -1 + 2^-10, 1 - 2^-10; the first, second, fourth and fifth stay outside the plane after the exact fixture's snap as well)
EDGE_ORDER = (6, 0, 1, 5, 7, 2, 3, 4)


def planted_values(n: int):
    """(positions, coordinate, value) of the planted samples: the k-th of K takes coordinate k % 3 and value min(k, K - 1 - k) % 8 of
    EDGE_ORDER -- counted from both ends, so that sample 0 and sample n - 1 straddle a plane's edge and their planted neighbours (the
    last sample of tile 0 when there is more than one tile) lie outside"""
    pos = planted_positions(n)
    k = np.arange(len(pos))
    v = so._EDGES[np.array(EDGE_ORDER)[np.minimum(k, len(pos) - 1 - k) % len(EDGE_ORDER)]]
    return pos, k % 3, v


def plant(x: np.ndarray, exact_sides: Sequence[int] = ()) -> np.ndarray:
    """x with the edge values written into the planted positions (a copy); `exact_sides`: snap them as the exact fixture's coordinates"""
    x = np.array(x, np.float32)
    pos, c, v = planted_values(len(x))
    x[pos, c] = so.exact_coords(v, exact_sides) if len(exact_sides) else so.snap(v)
    return x


def tap_classes(x: np.ndarray, shapes: Sequence[Tuple[int, int]]) -> np.ndarray:
    """per sample: 0 "inside" (every tap of every plane on a texel), 1 "straddle" (some plane has taps outside, none has all four
    outside), 2 "outside" (some plane has all four taps outside: the feature row has an exactly zero scale)"""
    x64 = np.asarray(x, np.float64)
    some = np.zeros(len(x64), bool)
    whole = np.zeros(len(x64), bool)
    for H, W in shapes:
        for a, b in so.PAIRS:
            x0 = np.floor((x64[:, a] + 1.0) / 2.0 * (W - 1)).astype(np.int64)
            y0 = np.floor((x64[:, b] + 1.0) / 2.0 * (H - 1)).astype(np.int64)
            okx = [(x0 >= 0) & (x0 < W), (x0 + 1 >= 0) & (x0 + 1 < W)]
            oky = [(y0 >= 0) & (y0 < H), (y0 + 1 >= 0) & (y0 + 1 < H)]
            taps = np.stack([ox & oy for ox in okx for oy in oky])
            some |= ~taps.all(0)
            whole |= ~taps.any(0)
    return np.where(whole, 2, np.where(some, 1, 0))


def probes(n: int, launch: str = "chain") -> np.ndarray:
    r = round_samples(launch)
    last = (n - 1) // TILE * TILE
    want = [0, 31, 32, n - 1, r - 1, r, last + (n - last) // 2]
    return np.array(sorted({p for p in want if 0 <= p < n}), np.int64)


# ------------------------------------------------------------------------------------------------ fixtures
GENERAL = {"small": (32, [(17, 17), (33, 33), (65, 65)], False), "nonsquare": (32, [(9, 33), (33, 9), (17, 65)], False)}
EXACT_NAME = "c32_s3_square"
FIXTURES = ("small", "nonsquare", "exact")


def shapes_of(name: str) -> List[Tuple[int, int]]:
    return so.KP_EXACT[EXACT_NAME][1] if name == "exact" else GENERAL[name][1]


@functools.lru_cache(maxsize=None)
def fixture(name: str, n: int):
    """(x [n, 3] float32 with the planted samples, planes [H, W, 32] float32 per (scale, pair), exact) -- computed once, read-only"""
    if name == "exact":
        x, planes, _, exact = so.kp_fixture(so.KP_EXACT, EXACT_NAME, "mixed", n, so.seed_of("fused", name, n))
        x = plant(x, [s for hw in shapes_of(name) for s in hw])
    else:
        x, planes, _, exact = so.kp_fixture(GENERAL, name, "mixed", n, so.seed_of("fused", name, n))
        x = plant(x)
    x.setflags(write=False)
    for p in planes:
        p.setflags(write=False)
    return x, tuple(planes), exact


def features_fp64(x: np.ndarray, planes: Sequence[np.ndarray]):
    """forward-only fp64 features [n, 96] (grid_sample as _scatter_orders._gs2: align_corners=True, zeros padding) and the same on
    |planes|: A, the sum of |terms| per element"""
    xs = torch.as_tensor(np.asarray(x, np.float64))
    out = []
    with torch.no_grad():
        for absolute in (False, True):
            feats = []
            for s in range(len(planes) // 3):
                prod = None
                for p, (a, b) in enumerate(so.PAIRS):
                    pl = torch.as_tensor(np.asarray(planes[3 * s + p], np.float64)).permute(2, 0, 1)[None]
                    v = so._gs2(pl.abs() if absolute else pl, xs[:, a], xs[:, b])
                    prod = v if prod is None else prod * v
                feats.append(prod)
            out.append(torch.cat(feats, -1).numpy())
    return out[0], out[1]


@functools.lru_cache(maxsize=8)
def reference(name: str, n: int):
    """(fp64 features, A) of fixture(name, n), read-only; the few largest cases are recomputed rather than all kept"""
    x, planes, _ = fixture(name, n)
    ref, aref = features_fp64(x, planes)
    ref.setflags(write=False)
    aref.setflags(write=False)
    return ref, aref


def ray_counts(n: int, seed: int) -> np.ndarray:
    """rays of 1 .. 256 samples covering n samples (the cut of test_hip_scatter._rays)"""
    rng = np.random.default_rng(seed)
    cnt: List[int] = []
    total = 0
    while total < n:
        cnt.append(int(rng.integers(1, 257)))
        total += cnt[-1]
    cnt[-1] -= total - n
    return np.array(cnt, np.int32)
