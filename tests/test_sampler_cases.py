"""CPU: the fixtures of tests/_sampler_cases.py are what test_hip_sampler_edges.py needs them to be, shown on the oracle alone, and the
oracle equals ATen (torch's CPU kernels, the reference's own arithmetic) at exactly the trilinear and inf-norm inputs the GPU tests use."""
import numpy as np
import pytest
import torch

import _sampler_cases as sc
from oracle import tinynerf_oracle as orc

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.int32)


def same_bits_or_nan(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(bits(a)[~np.isnan(a)], bits(b)[~np.isnan(b)])


# ---------------------------------------------------------------------------------------------- rays, boxes, grid
def test_rays_are_what_the_docstring_says():
    o, d, kind = sc.rays()
    assert o.shape == d.shape == (sc.R, 3) and o.dtype == d.dtype == f32
    assert np.isfinite(o).all() and np.isfinite(d).all()
    np.testing.assert_allclose(np.linalg.norm(d.astype(np.float64), axis=1), 1.0, atol=1e-6)
    for name, n in sc.N_KIND.items():
        assert (kind == name).sum() == n
    lo, hi = np.maximum(sc.BOXES["mixed"][0], sc.BOXES["pow2"][0]), np.minimum(sc.BOXES["mixed"][1], sc.BOXES["pow2"][1])
    ins = o[kind == "inside"]
    assert ((ins > lo) & (ins < hi)).all()
    zp, zn = d[kind == "zero_pos"], d[kind == "zero_neg"]
    assert ((bits(zp) == 0).sum(1) == 1).all()                                            # exactly +0.0: all bits clear
    assert ((bits(zn) == np.int32(-2 ** 31)).sum(1) == 1).all() and not (bits(zn) == 0).any()   # exactly -0.0: the sign bit alone
    face = o[kind == "face"]
    for box in sc.BOXES.values():
        assert (face[:, 0] == box[1, 0]).all()
    away = kind == "away"
    assert ((o[away] * d[away]).sum(1) > 0).all()
    sphere = np.isin(kind, ["plain", "zero_pos", "zero_neg", "away"])
    np.testing.assert_allclose(np.linalg.norm(o[sphere].astype(np.float64), axis=1), 3.0, atol=1e-6)
    assert kind[:5].tolist() == ["inside", "plain", "zero_neg", "face", "away"]            # the short prefixes are mixed


@pytest.mark.parametrize("marcher,contraction", [("aabb", "aabb"), ("unbounded", "mip360_inf")])
def test_short_prefixes_keep_something(marcher, contraction):
    """R = 1, 3, 4, 5 at S = 65 (a second chunk of one candidate): the first ray keeps samples and so does a later one; under the Mip-360
    contraction some ray keeps candidate 64 (with the box pair it lies a box diagonal behind the entry: never inside)"""
    for box in sc.BOXES:
        _, info, mask, _ = sc.oracle_sampler(marcher, contraction, box, 65, None, n_rays=5)
        assert info[0, 1] > 0 and (info[:, 1] > 0).sum() >= 2
        _, _, full, _ = sc.oracle_sampler(marcher, contraction, box, 65, None)
        assert np.array_equal(full[:5], mask) and (full[:, 64].any() or contraction == "aabb")


def test_boxes_take_both_contraction_paths():
    """``pow2`` of sampler.hip's make_args: every extent a power of two"""
    def pow2(box):
        m, _ = np.frexp((box[1] - box[0]).astype(f32))
        return m == 0.5
    assert pow2(sc.BOXES["mixed"]).tolist() == [True, False, False]
    assert pow2(sc.BOXES["pow2"]).all() and len(set((sc.BOXES["pow2"][1] - sc.BOXES["pow2"][0]).tolist())) == 3


def test_oracle_step_size_equals_torch_cpu():
    """core.py:68-70 by torch's CPU kernels: the value test_hip_sampler_edges.py installs in the box marcher"""
    for box in sc.BOXES.values():
        b = torch.from_numpy(box.copy())
        for S in sc.S_VALUES + (17, sc.S_LONG):
            assert bits((torch.norm(b[1] - b[0]) / S).numpy()) == bits(orc.aabb_step_size(box, S))


def test_grid_straddles_the_threshold():
    g = sc.grid()
    assert g.shape == sc.GRID_SHAPE and g.dtype == f32
    nz = g[g != 0]
    assert nz.min() >= f32(0.005) and nz.max() <= f32(0.03)
    assert (nz > f32(sc.THRESHOLD)).mean() > 0.5 and (nz < f32(sc.THRESHOLD)).mean() > 0.1
    assert 0.15 < (g != 0).mean() < 0.7
    assert (g[:, :, -1] != 0).all()                                                       # the face the face-plane origins read


@pytest.mark.parametrize("S", [s for s in sc.S_VALUES if s >= 63])
@pytest.mark.parametrize("box", list(sc.BOXES))
@pytest.mark.parametrize("marcher,contraction", sc.PAIRS)
def test_every_pair_keeps_a_useful_share(marcher, contraction, box, S):
    """kept share in [0.02, 0.9]; >= 10 % of the rays keep nothing and >= 10 % keep something; a kept sample on a ray with a zero direction
    component and one from an inside origin -- without and with the jitter table"""
    _, _, kind = sc.rays()
    for jit in (None, sc.jitter_table(S)):
        packed, info, mask, t = sc.oracle_sampler(marcher, contraction, box, S, jit)
        cnt = mask.sum(1)
        # the mask restated next to ray_provider is ray_provider's
        assert np.array_equal(cnt, info[:, 1]) and packed.shape[0] == cnt.sum() == t.shape[0]
        assert 0.02 <= mask.mean() <= 0.9, mask.mean()
        assert (cnt == 0).mean() >= 0.1 and (cnt > 0).mean() >= 0.1, (cnt == 0).mean()
        assert cnt[np.isin(kind, ["zero_pos", "zero_neg"])].sum() >= 1
        assert cnt[kind == "zero_neg"].sum() >= 1
        assert cnt[kind == "inside"].sum() >= 1
    words = sc.pack_mask(mask)
    k = np.arange(S)
    assert np.array_equal(((words[:, k // 64] >> (k % 64).astype(np.uint64)) & np.uint64(1)).astype(bool), mask)
    if S % 64:
        assert not (words[:, -1] >> np.uint64(S % 64)).any()


def test_face_plane_origins_read_the_out_of_bounds_tap():
    """(aabb, aabb): an origin on x = hi[0] with near = 0.05 is moved off the face by the first step, so the exact face is NOT among its
    candidates; what the fixture does reach is the outermost cell layer, x0 = W - 2 .. W - 1, on kept samples"""
    _, _, kind = sc.rays()
    for box in sc.BOXES:
        packed, info, mask, _ = sc.oracle_sampler("aabb", "aabb", box, 200, None)
        ids = np.repeat(np.arange(sc.R), info[:, 1])
        x = packed[kind[ids] == "face", 0]
        assert x.size and x.max() > 1 - 2 / (sc.GRID_SHAPE[2] - 1)


def test_long_case_leaves_more_than_64_chunks_unevaluated():
    """S = 8256: at least one of the first 64 rays leaves the box before candidate 64 * (129 - 65), in a float64 slab test, so the
    sampler's second zero-fill loop (chunks n_active + 64 and later) has words to write"""
    o, d, _ = sc.rays()
    o, d = o[:sc.R_LONG].astype(np.float64), d[:sc.R_LONG].astype(np.float64)
    n_chunks = (sc.S_LONG + 63) // 64
    assert n_chunks == 129
    for box in sc.BOXES.values():
        b = box.astype(np.float64)
        den = np.where(d == 0, 1e-9, d)
        t0, t1 = (b[0] - o) / den, (b[1] - o) / den
        t_in = np.maximum(np.minimum(t0, t1).max(1), sc.NEAR)
        t_out = np.maximum(t0, t1).min(1)
        step = np.linalg.norm(b[1] - b[0]) / sc.S_LONG
        k_exit = (t_out - t_in) / step
        early = (t_out > t_in) & (k_exit + 64 < 64 * (n_chunks - 65))          # (a chunk of slack for the kernel's own rounding)
        assert early.sum() >= 1, k_exit
        assert ((t_out > t_in) & (k_exit > 64)).sum() >= 1                     # ... and rays that keep candidates before they leave


# ---------------------------------------------------------------------------------------------- the oracle against ATen
@pytest.mark.parametrize("shape", sc.TRILINEAR_SHAPES)
def test_oracle_trilinear_equals_grid_sample(shape):
    g, p = sc.trilinear_grid(shape), sc.trilinear_points(shape)
    assert np.isnan(p).any() and np.isinf(p).any() and (np.abs(p) == 1).any() and (np.abs(p[np.isfinite(p)]) > 1.2).any()
    ref = torch.nn.functional.grid_sample(torch.from_numpy(g)[None, None], torch.from_numpy(p)[None, None, None], mode="bilinear",
                                          padding_mode="zeros", align_corners=True).reshape(-1).numpy()
    with np.errstate(all="ignore"):                       # (infinite and NaN points are part of the set)
        got = orc.trilinear_zeros_align(g, p)
    assert same_bits_or_nan(got, ref)
    assert (got != 0).sum() > 100 or g.size == 1


def test_oracle_mip360_inf_equals_torch():
    p = sc.mip_points()
    x = torch.from_numpy(p)
    n = torch.norm(x, p=float("inf"), dim=-1, keepdim=True)
    ref = (torch.where(n <= 1, x, (2 - 1 / n) * x / n) / 2).numpy()
    with np.errstate(all="ignore"):
        got, _ = orc.contract_mip360(p, float("inf"))
    assert same_bits_or_nan(got, ref)
    assert (np.abs(p).max(1) == 1).sum() >= 3 and (np.abs(p).max(1) == 0).any()


def test_contract_points_hold_the_edges():
    for box, aabb in sc.BOXES.items():
        p = sc.box_points(box)
        assert p.shape == (257, 3)
        for axis in range(3):
            for side in (0, 1):
                face = aabb[side, axis]
                for v in (face, np.nextafter(face, f32(-np.inf)), np.nextafter(face, f32(np.inf))):
                    assert (p[:, axis] == v).any()
        _, mask = orc.contract_aabb(p, aabb)
        assert 0.2 < mask.mean() < 0.8
    p = sc.mip_points()
    with np.errstate(over="ignore"):
        sq = p.astype(f32) * p.astype(f32)
        n2 = np.sqrt((sq[:, 0] + sq[:, 1]) + sq[:, 2])
    assert (n2 == 1).any() and (n2 == np.nextafter(f32(1), f32(2))).any() and np.isinf(n2).any()


# ---------------------------------------------------------------------------------------------- occupancy refresh fixtures
@pytest.mark.parametrize("n", [1, 255, 257, 5000])
def test_apply_case_is_decided_in_float64(n):
    cells, sig, alpha, redrawn = sc.apply_case(n, 1 / 1024., 0.01)
    assert redrawn < 0.01 * n or n == 1 and redrawn == 0
    assert not (np.abs(alpha[~np.isnan(alpha)] - np.float64(f32(0.01))) <= 1e-6).any()
    assert (cells > 0).sum() + (cells == 0).sum() == n and cells.max() <= 1
    if n >= 255:
        assert (cells == 0).any() and (cells == 1).any() and np.isnan(sig).sum() == 2 and np.isinf(sig).sum() == 2 and (sig == -1).sum() == 2
        assert (np.signbit(sig) & (sig == 0)).sum() == 2
        assert 0.2 < (alpha > 0.01).mean() < 0.8


@pytest.mark.parametrize("shape", sc.COARSEN_SHAPES)
def test_coarsen_reference_is_the_brute_force_maximum(shape):
    """every tap a point of block b can read -- floor index 4b .. 4b + 3, taps at it and one above -- lies in the block's cell range"""
    g = sc.coarsen_grid(shape)
    ref = sc.coarsen_ref(g)
    assert (g < 0).any() and ref.min() >= 0
    D, H, W = shape
    for z0 in range(-1, D):
        for y0 in range(-1, H):
            for x0 in range(-1, W):
                taps = [g[z, y, x] for z in (z0, z0 + 1) for y in (y0, y0 + 1) for x in (x0, x0 + 1)
                        if 0 <= z < D and 0 <= y < H and 0 <= x < W]
                assert max(taps + [0]) <= ref[max(z0, 0) >> 2, max(y0, 0) >> 2, max(x0, 0) >> 2]
