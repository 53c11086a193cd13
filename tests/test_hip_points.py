"""GPU tests of the point-cloud export: tn_points_compact through the C ABI against the numpy restatement of its definition
(tests/_points_ref.py) -- selection and order exactly, points to an fp32 ulp, colours to a level and exactly on dyadic inputs --,
the capacity contract, points.export_pointcloud on an analytic sphere, and train(pointcloud=N) end to end on a scene on disk."""
import ctypes as C
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _points_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"

BOX = np.float32([-1.0, -0.75, -0.5, 1.0, 0.75, 0.5])
MIN_OPACITY = 0.375
BG = np.float32([1.0, 0.5, 0.25])
PATTERNS = ("all", "none", "first", "last", "alternating", "random50", "random1")
SIZES = (1, 63, 64, 65, 255, 256, 257, 4099, 65536 + 257, 2 ** 20 + 13)      # wave, workgroup, scan-trip (1024 x 256 rays) and customary sizes


# ------------------------------------------------------------------------------------------------------------ inputs (numpy only)
def _pattern_mask(n, pattern, rng):
    want = np.zeros(n, bool)
    if pattern == "all":
        want[:] = True
    elif pattern == "first":
        want[0] = True
    elif pattern == "last":
        want[-1] = True
    elif pattern == "alternating":
        want[::2] = True
    elif pattern == "random50":
        want = rng.random(n) < 0.5
    elif pattern == "random1":
        want = rng.random(n) < 0.01
    return want


def _draw(want, rng):
    """rays whose point / opacity say `want`: kept rays end inside BOX with opacity above MIN_OPACITY; dropped rays miss the box
    (reason 0), lie below the opacity (1) or both (2)"""
    n = want.size
    lo, hi = BOX[:3].astype(np.float64), BOX[3:].astype(np.float64)
    reason = np.where(want, -1, rng.integers(0, 3, n))
    p = lo + (hi - lo) * (0.01 + 0.98 * rng.random((n, 3)))                       # inside, 1 % of the side from every face
    out = (reason == 0) | (reason == 2)
    axis, side = rng.integers(0, 3, n), rng.integers(0, 2, n)
    beyond = np.where(side == 1, hi[axis], lo[axis]) + np.where(side == 1, 1.0, -1.0) * (0.01 + rng.random(n))
    p[out, axis[out]] = beyond[out]
    depth = (0.5 + 2.5 * rng.random(n)).astype(np.float32)
    d = rng.standard_normal((n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    o = (p - depth[:, None].astype(np.float64) * d).astype(np.float32)
    low = (reason == 1) | (reason == 2)
    opacity = np.where(low, MIN_OPACITY * (0.05 + 0.9 * rng.random(n)), MIN_OPACITY + 0.01 + (1 - MIN_OPACITY - 0.01) * rng.random(n)).astype(np.float32)
    return o, d, depth, opacity


def make_case(n, pattern, seed=0):
    """float32 inputs of n rays that keep `pattern`; redrawn until no point lies within 1e-4 of a face of BOX and no opacity within
    1e-6 of MIN_OPACITY (tests/test_points_host.py checks this on the CPU), so the fp32 and the fp64 predicate agree"""
    rng = np.random.default_rng([n, PATTERNS.index(pattern), seed])
    want = _pattern_mask(n, pattern, rng)
    o, d, depth, opacity = _draw(want, rng)
    for _ in range(100):
        p = ref.points64(o, d, depth)
        near = np.minimum(np.abs(p - BOX[:3].astype(np.float64)), np.abs(p - BOX[3:].astype(np.float64))).min(1) <= 1e-4
        near |= np.abs(opacity.astype(np.float64) - MIN_OPACITY) <= 1e-6
        if not near.any():
            break
        o2, d2, depth2, opacity2 = _draw(want[near], rng)
        o[near], d[near], depth[near], opacity[near] = o2, d2, depth2, opacity2
    else:
        raise AssertionError("could not draw inputs clear of the thresholds")
    colour = rng.random((n, 3))
    rgb = (opacity[:, None] * colour + (1.0 - opacity[:, None]) * BG[None, :]).astype(np.float32)     # what the renderer composites
    return {"rays_o": o, "rays_d": d, "depth": depth, "opacity": opacity, "rgb": rgb, "want": want}


# ------------------------------------------------------------------------------------------------------------ the call
SENTINEL_F, SENTINEL_B, SENTINEL_I = -7.25, 0xA5, -12345


def run(case, box=BOX, bg=BG, min_opacity=MIN_OPACITY, capacity=None, null_outputs=False, guard=(0, 64), spare=0):
    """tn_points_compact through the C ABI on sentinel-filled outputs -> (count, points, colors, src) as numpy, ALL `capacity` rows.
    The workspace is tn_points_workspace_bytes + `spare` bytes with `guard` bytes of a fixed pattern before and behind it."""
    from tinynerf_amd import _lib as L
    dev = torch.device(DEV)
    t = {k: torch.from_numpy(np.ascontiguousarray(case[k])).to(dev) for k in ("rays_o", "rays_d", "rgb", "opacity", "depth")}
    n = t["opacity"].numel()
    cap = n if capacity is None else capacity
    bg_t = None if bg is None else torch.from_numpy(np.float32(bg)).to(dev)
    box_t = None if box is None else torch.from_numpy(np.float32(box)).to(dev)
    nbytes = C.c_int64(0)
    L.call_plain("tn_points_workspace_bytes", C.c_int64(n), C.byref(nbytes))
    first, last = guard[0], guard[0] + nbytes.value + spare
    work = torch.full((last + guard[1],), 0x5A, dtype=torch.uint8, device=dev)
    points = torch.full((cap, 3), SENTINEL_F, dtype=torch.float32, device=dev)
    colors = torch.full((cap, 3), SENTINEL_B, dtype=torch.uint8, device=dev)
    src = torch.full((cap,), SENTINEL_I, dtype=torch.int32, device=dev)
    count = torch.full((1,), -1, dtype=torch.int64, device=dev)
    outs = (None, None, None) if null_outputs else (L.ptr(points), L.ptr(colors), L.ptr(src))
    L.call("tn_points_compact", dev, L.ptr(t["rays_o"]), L.ptr(t["rays_d"]), L.ptr(t["rgb"]), L.ptr(t["opacity"]), L.ptr(t["depth"]),
           L.ptr(bg_t), L.ptr(box_t), C.c_float(min_opacity), C.c_int64(n), C.c_int64(cap), *outs, L.ptr(count), L.ptr(work[first:]))
    torch.cuda.synchronize()
    assert bool((work[:first] == 0x5A).all()) and bool((work[last:] == 0x5A).all()), "the workspace was overrun"
    return int(count.item()), points.cpu().numpy(), colors.cpu().numpy(), src.cpu().numpy()


def check_against_yardstick(case, got, box=BOX, bg=BG, min_opacity=MIN_OPACITY, tag=""):
    count, points, colors, src = got
    want_src, want_p, want_c, val = ref.compact(case["rays_o"], case["rays_d"], case["rgb"], case["opacity"], case["depth"], bg, box, min_opacity)
    m = want_src.size
    assert count == m, (tag, count, m)
    assert np.array_equal(src[:m], want_src), tag                                  # selection and order: exact
    err = np.abs(points[:m].astype(np.float64) - want_p) / ref.ulp32(want_p) if m else np.zeros(1)
    level = np.abs(colors[:m].astype(np.int64) - want_c.astype(np.int64)) if m else np.zeros(1, np.int64)
    assert err.max() <= 1.0, (tag, err.max())                                      # fp32 fma: the exact value rounded once
    assert level.max() <= 1, (tag, level.max())
    # a level may differ only where the float64 value sits at a boundary: fp32 error x 255 is ~1e-4 of a level
    if m and level.any():
        assert np.abs(val - np.round(val))[level > 0].max() < 1e-3, tag
    assert (points[m:] == np.float32(SENTINEL_F)).all() and (colors[m:] == SENTINEL_B).all() and (src[m:] == SENTINEL_I).all(), tag
    return m, float(err.max()), int(level.sum())


# ------------------------------------------------------------------------------------------------------------ selection, order, values
@pytest.mark.parametrize("n", SIZES)
def test_selection_order_and_values(n):
    for pattern in PATTERNS:
        case = make_case(n, pattern)
        m, err, levels = check_against_yardstick(case, run(case), tag=(n, pattern))
        assert m == int(case["want"].sum())
        print(f"n {n} {pattern}: kept {m}, worst point error {err:.2f} ulp, colour bytes off by one level: {levels}")


@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_the_workspace_is_what_the_size_function_says(n):
    """a wave that starts past n and a last workgroup with one live lane store their ballots and counts inside the layout: a
    workspace of exactly tn_points_workspace_bytes in the middle of a larger buffer leaves the bytes around it alone (`run`
    asserts that) and gives the outputs of a generous one"""
    for pattern in ("all", "last", "random50"):
        case = make_case(n, pattern)
        tight, generous = run(case, guard=(256, 256)), run(case, guard=(256, 256), spare=4096)
        assert tight[0] == generous[0] == int(case["want"].sum()), (n, pattern)
        assert all(np.array_equal(a, b) for a, b in zip(tight[1:], generous[1:])), (n, pattern)


def _dyadic_batch(n=300):
    """n copies of a ray whose every intermediate is exact: o = 0, d = +x, depth 0.5, opacity 0.5, inside the box [-0.5, 0.5]^3 with
    its point ON the +x face and its opacity ON the bound"""
    o = np.zeros((n, 3), np.float32)
    d = np.tile(np.float32([1, 0, 0]), (n, 1))
    return {"rays_o": o, "rays_d": d, "depth": np.full(n, 0.5, np.float32), "opacity": np.full(n, 0.5, np.float32),
            "rgb": np.tile(np.float32([0.5, 0.25, 0.75]), (n, 1))}


HALF_BOX = np.float32([-0.5] * 3 + [0.5] * 3)
UP, DOWN = np.nextafter(np.float32(0.5), np.float32(1)), np.nextafter(np.float32(0.5), np.float32(0))


def test_faces_and_the_opacity_bound_are_inclusive():
    case = _dyadic_batch(12)
    for k in range(6):                                             # ray k ends on face k: -x -y -z +x +y +z; rays 6..11 one ulp beyond it
        for j in (k, k + 6):
            case["rays_d"][j] = 0
            case["rays_d"][j, k % 3] = -1.0 if k < 3 else 1.0
        case["depth"][k + 6] = UP
    count, points, colors, src = run(case, box=HALF_BOX, bg=None, min_opacity=0.5)
    assert count == 6 and src[:6].tolist() == [0, 1, 2, 3, 4, 5]
    want = np.zeros((6, 3), np.float32)
    for k in range(6):
        want[k, k % 3] = -0.5 if k < 3 else 0.5
    assert np.array_equal(points[:6], want)                        # exact
    assert np.array_equal(colors[:6], np.tile(np.uint8([255, 128, 255]), (6, 1)))      # 0.5 / 0.5, 0.25 / 0.5 -> 128, 1.5 clamped
    check_against_yardstick(case, (count, points, colors, src), box=HALF_BOX, bg=None, min_opacity=0.5)


def test_rejections_inside_a_kept_batch():
    base = _dyadic_batch()
    n = base["opacity"].size
    kept_all = run(base, box=HALF_BOX, bg=None, min_opacity=0.5)
    assert kept_all[0] == n
    rejects = {"nan opacity": ("opacity", np.nan), "opacity one ulp low": ("opacity", DOWN), "nan depth": ("depth", np.nan),
               "+inf depth": ("depth", np.inf), "-inf depth": ("depth", -np.inf), "zero depth": ("depth", 0.0),
               "-0 depth": ("depth", -0.0), "negative depth": ("depth", -0.5), "depth one ulp beyond the face": ("depth", UP)}
    at = [0, 1, 63, 64, 65, 127, 128, 255, 256, 299]               # wave and workgroup edges
    for k, (name, (key, value)) in enumerate(rejects.items()):
        case = {kk: v.copy() for kk, v in base.items()}
        i = at[k % len(at)]
        case[key][i] = value
        count, points, colors, src = run(case, box=HALF_BOX, bg=None, min_opacity=0.5)
        assert count == n - 1 and src[:n - 1].tolist() == [j for j in range(n) if j != i], name
    # a point that overflows to inf, without a box (a box would reject it as well); finite inputs
    case = {kk: v.copy() for kk, v in base.items()}
    case["rays_d"][130] = [3e30, 0, 0]
    case["depth"][130] = 3e30
    count, _, _, src = run(case, box=None, bg=None, min_opacity=0.5)
    assert count == n - 1 and 130 not in src[:n - 1].tolist()
    # a NaN origin: the point is not finite
    case["rays_o"][7, 1] = np.nan
    count, _, _, src = run(case, box=None, bg=None, min_opacity=0.5)
    assert count == n - 2 and 7 not in src[:n - 2].tolist()


def test_colours_are_exact_on_a_dyadic_grid():
    """u = k / 256 and bg = j / 256 with opacity in {0.5, 0.75, 1}: rgb = opacity u + (1 - opacity) bg is a multiple of 1 / 1024, the
    fma gives opacity u exactly, the division u exactly, u 255 + 0.5 has 16 significant bits -- the byte is floor((255 k + 128) / 256)"""
    ks = np.arange(-64, 321)                                       # u from -0.25 to 1.25: both clamps
    ops = (0.5, 0.75, 1.0)
    n = len(ops) * ks.size
    case = _dyadic_batch(n)
    u = np.tile(ks / 256.0, len(ops))
    op = np.repeat(ops, ks.size)
    want = np.floor((255 * np.clip(np.tile(ks, len(ops)), 0, 256) + 128) / 256).astype(np.uint8)
    case["opacity"] = op.astype(np.float32)
    for bg in ([0.0, 1.0, 0.5], [37 / 256, 0.25, 1.0]):
        rgb = op[:, None] * u[:, None] + (1 - op[:, None]) * np.float64(bg)[None, :]
        case["rgb"] = rgb.astype(np.float32)
        assert np.array_equal(case["rgb"].astype(np.float64), rgb)                 # exactly representable
        count, _, colors, src = run(case, box=None, bg=np.float32(bg), min_opacity=0.5)
        assert count == n and np.array_equal(src, np.arange(n))
        assert np.array_equal(colors, np.repeat(want[:, None], 3, 1))
        assert np.array_equal(colors, ref.colors64(case["rgb"], case["opacity"], bg)[0])


def test_nan_colour_is_zero_and_no_background_is_a_zero_background():
    case = make_case(4099, "random50", seed=3)
    case["rgb"][::5, 1] = np.nan
    count, points, colors, src = run(case, bg=None)
    m, _, _ = check_against_yardstick(case, (count, points, colors, src), bg=None)
    nan_rows = np.isin(src[:m], np.arange(0, 4099, 5))
    assert nan_rows.any() and (colors[:m][nan_rows, 1] == 0).all() and colors[:m][~nan_rows, 1].any()
    zeros = run(case, bg=np.zeros(3, np.float32))
    assert zeros[0] == count and all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(zeros[1:], (points, colors, src)))
    # opacity = +inf passes the bound; its colour is NaN -> 0 with a background, rgb / inf = 0 without
    case["opacity"][case["want"].argmax()] = np.inf
    check_against_yardstick(case, run(case, bg=BG), bg=BG)


# ------------------------------------------------------------------------------------------------------------ capacity
def test_capacity_bounds_what_is_written():
    case = make_case(4099, "random50", seed=1)
    full = run(case)
    kept = full[0]
    assert 1500 < kept < 2600
    assert run(case, capacity=0, null_outputs=True)[0] == kept                    # count only
    for cap in (kept - 1, kept, kept + 7):
        count, points, colors, src = run(case, capacity=cap)
        m = min(kept, cap)
        assert count == kept, cap                                                  # the full number, whatever the capacity
        assert np.array_equal(points[:m].view(np.uint32), full[1][:m].view(np.uint32)) and np.array_equal(colors[:m], full[2][:m])
        assert np.array_equal(src[:m], full[3][:m])
        assert (points[m:].view(np.uint32) == np.float32(SENTINEL_F).view(np.uint32)).all() and (colors[m:] == SENTINEL_B).all()
        assert (src[m:] == SENTINEL_I).all()
    again = run(case)
    assert again[0] == kept and all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(again[1:], full[1:]))


def test_no_rays():
    empty = {k: np.zeros((0, 3), np.float32) for k in ("rays_o", "rays_d", "rgb")}
    empty.update(opacity=np.zeros(0, np.float32), depth=np.zeros(0, np.float32))
    assert run(empty)[0] == 0
    from tinynerf_amd import points as P
    z = torch.zeros((0, 3), device=DEV)
    p, c, s = P.compact_points(z, z, {"rgb": z, "opacity": z[:, 0], "depth": z[:, 0], "median_depth": z[:, 0]}, None)
    assert p.shape == (0, 3) and c.shape == (0, 3) and c.dtype == torch.uint8 and s.shape == (0,) and s.dtype == torch.int32


# ------------------------------------------------------------------------------------------------------------ host layer, analytic sphere
RADIUS, RES, VIEWS = 0.5, 40, 5


def _sphere_views():
    """cameras on a ring of radius 2 looking at a sphere of radius 0.5 around the origin: per view rays [RES, RES, 3] and numpy-made
    maps -- the hit distance solved in float64 for the float32 rays as they are (|d| is 1 only to rounding: the quadratic carries
    d.d), opacity 1 on a hit and 0 off it, colour a function of the hit point on a 1/32 grid (exact bytes), white behind"""
    views, maps, hits = [], [], []
    for v in range(VIEWS):
        a = 2 * np.pi * v / VIEWS
        eye = np.array([2 * np.cos(a), 2 * np.sin(a), 0.4])
        fwd = -eye / np.linalg.norm(eye)
        right = np.cross(fwd, [0, 0, 1.0]); right /= np.linalg.norm(right)
        up = np.cross(right, fwd)
        s = (np.arange(RES) + 0.5) / RES - 0.5
        x, y = np.meshgrid(s * 0.8, -s * 0.8)
        d = fwd[None, None] + x[..., None] * right + y[..., None] * up
        d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
        o = np.broadcast_to(eye.astype(np.float32), d.shape).copy()
        o64, d64 = o.astype(np.float64), d.astype(np.float64)
        qa, qb, qc = (d64 * d64).sum(-1), (o64 * d64).sum(-1), (o64 * o64).sum(-1) - RADIUS ** 2
        disc = qb * qb - qa * qc
        hit = disc > 1e-6                                          # (grazing rays within rounding of the limb count as misses)
        t = np.where(hit, (-qb - np.sqrt(np.maximum(disc, 0))) / qa, 0.0)
        p = o64 + t[..., None] * d64
        colour = np.round((p + 0.5) * 32) / 32
        rgb = np.where(hit[..., None], colour, 1.0).astype(np.float32)
        views.append({"rays_o": torch.from_numpy(o).to(DEV), "rays_d": torch.from_numpy(d).to(DEV)})
        maps.append({"rgb": torch.from_numpy(rgb).to(DEV), "opacity": torch.from_numpy(hit.astype(np.float32)).to(DEV),
                     "depth": torch.from_numpy(t.astype(np.float32)).to(DEV), "median_depth": torch.from_numpy(t.astype(np.float32)).to(DEV)})
        hits.append((hit.reshape(-1), rgb.reshape(-1, 3)))
    return views, maps, hits


def test_export_on_an_analytic_sphere(tmp_path):
    from tinynerf_amd import points as P
    from tinynerf_amd.run import TrainConfig
    white = torch.ones(3, device=DEV)
    trainer = SimpleNamespace(world=1, device=torch.device(DEV), cfg=TrainConfig(method="kplanes", scene_type="aabb"),
                              renderer=SimpleNamespace(_bg=lambda device: white))
    views, maps, hits = _sphere_views()
    total = sum(int(h.sum()) for h, _ in hits)
    assert total > 1500 and all(0 < h.sum() < h.size for h, _ in hits)
    path = tmp_path / "sphere.ply"
    points, colors = P.export_pointcloud(trainer, views, path=path, rendered=maps)
    assert points.shape == (total, 3) and colors.shape == (total, 3) and points.is_cuda            # every hitting ray, nothing else
    p = points.cpu().numpy().astype(np.float64)
    assert np.abs(np.linalg.norm(p, axis=1) - RADIUS).max() <= 1e-6
    want = np.concatenate([np.floor(rgb[h].astype(np.float64) * 255 + 0.5).astype(np.uint8) for h, rgb in hits])
    assert np.array_equal(colors.cpu().numpy(), want)                                              # view order, ray order, exact bytes
    got_p, got_c = P.read_ply(path)
    assert np.array_equal(got_p.view(np.uint32), points.cpu().numpy().view(np.uint32)) and np.array_equal(got_c, want)
    # the median depth is the same map here; the default crop (+-1.5) keeps everything, a tighter one cuts
    again = P.export_pointcloud(trainer, views, rendered=maps, depth="median")
    assert torch.equal(again[0], points) and torch.equal(again[1], colors)
    half = P.export_pointcloud(trainer, views, rendered=maps, crop=[-1, -1, 0, 1, 1, 1])[0]
    assert 0 < half.size(0) < total and bool((half[:, 2] >= 0).all())
    assert int((points[:, 2] >= 0).sum()) == half.size(0)
    assert P.export_pointcloud(trainer, views, rendered=maps, crop=False)[0].size(0) == total
    assert P.export_pointcloud(trainer, views, indices=[3, 1], rendered=[maps[3], maps[1]])[0].size(0) == int(hits[3][0].sum() + hits[1][0].sum())
    # fewer points than there are: exactly n_points, the same for the same seed, in the original order
    k = 1000
    a, ca = P.export_pointcloud(trainer, views, rendered=maps, n_points=k, seed=4)
    b, cb = P.export_pointcloud(trainer, views, rendered=maps, n_points=k, seed=4)
    c, _ = P.export_pointcloud(trainer, views, rendered=maps, n_points=k, seed=5)
    assert a.shape == (k, 3) and ca.shape == (k, 3) and torch.equal(a, b) and torch.equal(ca, cb) and not torch.equal(a, c)
    row = {r.tobytes(): i for i, r in enumerate(points.cpu().numpy())}
    assert len(row) == total                                       # (the points are distinct: a row names its place)
    for sub, col in ((a, ca), (c, None)):
        at = np.array([row[r.tobytes()] for r in sub.cpu().numpy()])
        assert (np.diff(at) > 0).all()                             # still view order and ray order
        if col is not None:
            assert np.array_equal(col.cpu().numpy(), want[at])
    gen = torch.Generator().manual_seed(4)
    assert np.array_equal(np.sort(torch.randperm(total, generator=gen)[:k].numpy()), np.array([row[r.tobytes()] for r in a.cpu().numpy()]))


# ------------------------------------------------------------------------------------------------------------ end to end
def _scene_on_disk(root):
    """the 48 x 48 synthetic ball in Blender format: three training views, the first of them as the test split"""
    from PIL import Image
    from tinynerf_amd import rays
    o, d, rgb, K, cams = rays.synthetic_scene(n_views=3, res=48, seed=5, device="cpu")
    imgs = (rgb.reshape(3, 48, 48, 3) * 255).to(torch.uint8).numpy()
    (root / "train").mkdir()
    frames = []
    for i in range(3):
        Image.fromarray(imgs[i]).save(root / "train" / f"r_{i}.png")
        frames.append({"file_path": f"./train/r_{i}", "transform_matrix": cams[i].tolist()})
    for split in ("train", "test"):
        json.dump({"camera_angle_x": 0.6911112070083618, "frames": frames[:3 if split == "train" else 2]},
                  open(root / f"transforms_{split}.json", "w"))


def test_train_writes_a_point_cloud(tmp_path, monkeypatch):
    """train(pointcloud=5000) on a scene on disk, with and without render_maps, and train(pointcloud=0).

    What is compared exactly is what is deterministic: a run's file against a standalone export_pointcloud of the trainer that
    run returns -- with render_maps the file was made from the dicts of the final test render, so equal bytes say that the shared
    and the standalone path agree --, and the entry points, sizes and scalar arguments of every launch of the three training steps
    with and without the flag, with tr.last.  Files and losses of two separate runs are not compared bit for bit: the training step
    adds plane and weight gradients with fp32 atomics in arrival order, two identical trainers differ after one step
    (tests/test_hip_distortion.py: test_distortion_weight_zero_is_the_plain_step), with or without this feature.  Across runs the
    first loss, taken before any update, agrees to the reordering of its fp64 sum (1e-12); the next two agree to 1e-3 -- a step
    that drew other rays or updated differently moves the loss by per cent, the atomics' order by parts in 1e7."""
    from tinynerf_amd import _lib as L, data, points as P
    from tinynerf_amd.run import TrainConfig, train
    _scene_on_disk(tmp_path)
    dev = torch.device(DEV)
    train_rays = data.RaysDataset(data.parse_nerf_synthetic(tmp_path, "train"), dev)
    test_set = data.PoseDataset(data.parse_nerf_synthetic(tmp_path, "test"), dev)
    calls = []
    orig = L.call

    def record(name, *args):
        calls.append((name,) + tuple(x.value for x in args if isinstance(x, (C.c_int, C.c_int32, C.c_int64, C.c_float))))
        return orig(name, *args)
    monkeypatch.setattr(L, "call", record)
    from tinynerf_amd import run as run_module
    infer = run_module.infer

    def marked_infer(*args, **kw):
        calls.append(("infer",))                                   # where the training loop's launches end
        return infer(*args, **kw)
    monkeypatch.setattr(run_module, "infer", marked_infer)

    def go(name, steps, **kw):
        out = tmp_path / name
        out.mkdir()
        cfg = TrainConfig(method="kplanes", batch_size=512, n_samples=64, occupancy_res=32, kplanes_resolutions=(16, 32, 64), seed=3)
        del calls[:]
        tr, tm, _, _ = train(cfg, train_rays, None, test_set, out, max_steps=steps, log_every=50, **kw)
        return out, tr, [m["loss"] for m in tm], list(calls)

    files = {}
    for name, kw in (("maps", {"render_maps": True}), ("plain", {})):
        out, tr, _, seq = go(name, 40, pointcloud=5000, **kw)
        raw = open(out / "pointcloud.ply", "rb").read()
        p, c = P.read_ply(out / "pointcloud.ply")
        files[name] = p
        assert 0 < p.shape[0] <= 5000 and c.shape == p.shape
        assert (np.abs(p) <= 1.5).all()                            # the marcher's box
        assert sum(call[0] == "tn_points_compact" for call in seq) == len(test_set) == 2
        n_render = sum(call[0] == "tn_ray_maps" for call in seq)
        P.export_pointcloud(tr, test_set, path=out / "standalone.ply", n_points=5000, seed=3)
        assert open(out / "standalone.ply", "rb").read() == raw, name
        if name == "maps":
            assert (out / "test_full_maps_0000.npz").exists()
            maps_render = n_render
        else:
            assert n_render == maps_render                         # either way every view is rendered once
    print(f"points with render_maps {files['maps'].shape[0]}, without {files['plain'].shape[0]}; the two files are "
          f"{'equal' if np.array_equal(files['maps'], files['plain']) else 'different'}")
    # the flag leaves the training step alone
    out0, tr0, loss0, seq0 = go("off", 2, pointcloud=0)
    out1, tr1, loss1, seq1 = go("on", 2, pointcloud=5000)
    assert not (out0 / "pointcloud.ply").exists() and (out1 / "pointcloud.ply").exists()
    assert not any(call[0].startswith("tn_points") for call in seq0)
    steps0, steps1 = seq0[:seq0.index(("infer",))], seq1[:seq1.index(("infer",))]
    assert len(steps0) >= 3 and steps0 == steps1                  # three steps: entry points, sizes and scalar arguments
    assert sum(call[0] == "tn_points_compact" for call in seq1) == 2 and not any(call[0].startswith("tn_points") for call in steps1)
    assert tr0.last == tr1.last and len(loss0) == len(loss1) == 3
    print("losses without the flag", loss0, "with it", loss1)
    np.testing.assert_allclose(loss1[0], loss0[0], rtol=1e-12)
    np.testing.assert_allclose(loss1[1:], loss0[1:], rtol=1e-3)
