"""GPU tests of the TSDF colour fusion: tn_tsdf_integrate_color and tn_tsdf_sample_colors through the C ABI against the
float64 yardstick of tests/_tsdf_color_ref.py on the shared cases of tests/_tsdf_cases.py, the call forms, the host layer, a sphere
coloured by its normals fused from eight views, and train(tsdf_mesh=R, tsdf_colors="fused") end to end.

What is compared, with e = 2^-24 the relative error of one float32 rounding.

Integration.  Steps 1-5 are tn_tsdf_integrate's, so the nodes that a view brings within a tie margin of one of their decision edges
(_tsdf_cases.ambiguous) are left out, at most 2 % of a case's nodes.  The truncation edges are no decision edges here -- w is 0 on
both -- and the bound below counts a view whose float64 sdf lies up to 2^-22 |p| outside the band as if it contributed (the float32
sdf may still be inside); keeping the margin at -trunc only leaves out a few more nodes.  At every other node the kernel and the
yardstick look at the same pixels, and per view:
  sdf = D - |p| has the error 2^-22 |p| (tests/test_hip_tsdf.py derives it: 2 e from p, three roundings under the root halved by it,
  the root's, the subtraction's).  |sdf| / trunc is a correctly rounded quotient <= 1: e more.  1 - quotient lies in [0, 1]: one
  rounding, <= e.  So |dw| <= a := 2^-22 |p| / trunc + 2^-23, which is the first term of 6j's bound with half its constant.
  u_c = fmaf(-(1 - op), bg_c, rgb_c) / op: 1 - op has the relative error e, the fmaf rounds its exact result once, the division once
  more: |du_c| <= e ((1 - op) |bg_c| / op + 2 |u_raw|) -- nothing where |u_raw| > 2 or u_raw is NaN, where both sides clamp alike --
  and the clamp to [0, 1] enlarges nothing.  With u_c <= 1 the exact product has |d(w u_c)| <= a u_c + (w + a) |du_c|.
  C_c = fmaf(w, u_c, C_c) rounds once per contributing view, each time a partial sum of non-negative terms: n e (sum w u_c + the
  terms' errors) in all; C_3 += w rounds n - 1 times, the first sum being 0 + w.
  |C_c - ref| <= sum (a u_c + (w + a) |du_c|) + n e (sum w u_c + that),  |C_3 - ref| <= sum a + (n - 1) e (sum w + sum a),
  both times (1 + 2^-20) for the products of two errors: 6j's shape, the per-view constant enlarged by (w + a) |du_c| for the extra
  division, fmaf and product.  _tsdf_color_ref.integrate_color returns the sums.

Sampling.  The same float32 volume goes to both sides.  g_c = (p_c - lo_c) / h_c is a subtraction and a division: relative error
2 e = 2^-23, so |du_c| <= 2^-23 (n_c + 1) wherever the point is not clamped (g_c - (float)i_c itself is exact).  A trilinear
interpolant moves by at most |du_c| times the cell's largest difference between two corners, per axis ("spread").  Where no g_c
lies within du_c of an integer the float32 floor names the float64 cell, and the cell's own 8 corners are all there is; only within
du_c of a face may it name the neighbouring cell, where the interpolant continues, and for those points alone the difference is taken
over the 4 x 4 x 4 nodes of the cell and its neighbours.  Each weight t_k = (a_0 a_1) a_2 carries three roundings (1 - u_c, two
products), the chain of 8 fmaf eight more, each of a partial sum below the largest magnitude among the same nodes ("size"):
  |dnum_c| <= sum_a 2^-23 (n_a + 1) spread_c + 11 e size_c,  |dden| likewise,  both times (1 + 2^-20);
  |d(num_c / den)| <= (|dnum_c| + (num_c / den) |dden|) / (den - |dden|) (1 + e) + e num_c / den, one division.
The quotient is compared where den > 2 |dden|; below that only den is (a point within float32 resolution of the last coloured node:
its colour is a quotient of two roundings).  A row whose yardstick den is 0 must be exactly (0, 0, 0, 0) -- unless the point lies
within du of a cell face, where the float32 floor may name the coloured neighbour: then den <= |dden| is asked.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _tsdf_cases as tc
import _tsdf_color_ref as cref
import _tsdf_ref as ref
from test_hip_tsdf import _dev, _scene_on_disk, bits, device_table, run_integrate

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 16                                                         # floats: 64 guard bytes behind C
SENTINEL = -7.25
BG = np.float32([0.2, 0.7, 0.1])
E = cref.E
FORMS = [(name, op) for name in tc.CASES for op in (False, True)]


# ------------------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def colours(n_views, lens):
    """rgb float32 [n_pixels,3]: seeded, uniform in [0, 1], one entry in 24 a speck of NaN, -0.3 or 1.7"""
    n = tc.maps(n_views, lens)[0].size
    rng = np.random.default_rng(7 + n_views)
    rgb = rng.random((n, 3)).astype(np.float32)
    speck = rng.random((n, 3)) < 1.0 / 24.0
    rgb[speck] = rng.choice(np.float32([np.nan, -0.3, 1.7]), int(speck.sum()))
    rgb.setflags(write=False)
    return rgb


@functools.lru_cache(maxsize=None)
def form(name, with_opacity):
    """a case of _tsdf_cases with or without an opacity map, the colours, and the yardstick's result with the margins.  The map is the
    case's own with its ones replaced by seeded values in [0.5, 1]: the same pixels pass the gate, and the division by the opacity and
    the background have something to do"""
    c = dict(tc.case(name))
    lens = tc.CASES[name][2]
    c["opacity"] = None
    if with_opacity:
        op = tc.maps(c["n_views"], lens)[1].copy()
        fill = np.random.default_rng(3).uniform(0.5, 1.0, op.size).astype(np.float32)
        fill[::5] = 0.5                                            # the gate's own value passes
        c["opacity"] = np.where(op == 1.0, fill, op)
        c["opacity"].setflags(write=False)
    c["rgb"] = colours(c["n_views"], lens)
    c["want"] = cref.integrate_color(c["dims"], c["lo"], c["h"], c["c2w"], c["models"], c["lenses"], c["sizes"], c["depth"], c["opacity"],
                                     c["min_opacity"], c["rgb"], BG, c["trunc"], margins=True)
    for a in c["want"].values():
        a.setflags(write=False)
    return c


def run_color(c, cams, ranges=None, state=None, rgb=None, bg=BG):
    """tn_tsdf_integrate_color through the C ABI, one call per (first, count) of `ranges` (default: all views in one), on a C with 64
    guard bytes behind it -> C float32 numpy [nodes,4]"""
    from tinynerf_amd import _lib as L
    from tinynerf_amd.mesh import _grid
    dev = torch.device(DEV)
    n = 4 * (c["dims"][0] + 1) * (c["dims"][1] + 1) * (c["dims"][2] + 1)
    buf = torch.full((n + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    buf[:n] = 0.0 if state is None else torch.from_numpy(np.ascontiguousarray(state, np.float32).reshape(-1)).to(dev)
    depth, opacity, colour, back = _dev(c["depth"]), _dev(c["opacity"]), _dev(c["rgb"] if rgb is None else rgb), _dev(bg)
    lo_c, h_c, dims_c = _grid(c["lo"], c["h"], c["dims"])
    for first, count in ([(0, c["n_views"])] if ranges is None else ranges):
        L.call("tn_tsdf_integrate_color", dev, C.byref(cams.table), L.ptr(depth), L.ptr(opacity), C.c_float(c["min_opacity"]), L.ptr(colour),
               L.ptr(back), dims_c, lo_c, h_c, C.c_float(c["trunc"]), C.c_int32(first), C.c_int32(count), L.ptr(buf))
    torch.cuda.synchronize()
    assert bool((buf[n:] == SENTINEL).all()), "C was overrun"
    return buf[:n].cpu().numpy().reshape(-1, 4)


def color_bounds(want):
    """(bound on the three colour accumulators [nodes,3], bound on the weight accumulator [nodes]): the docstring's"""
    n = want["n_views"]
    col = want["dterm"] + n[:, None] * E * (want["sum_wu"] + want["dterm"])
    den = want["dw"] + np.maximum(n - 1.0, 0.0) * E * (want["sum_w"] + want["dw"])
    return cref.SECOND * col, cref.SECOND * den


# ------------------------------------------------------------------------------------------------------------ against the yardstick
@pytest.mark.parametrize("name,with_opacity", FORMS)
def test_integrate_color_against_the_yardstick(name, with_opacity):
    c = form(name, with_opacity)
    want = c["want"]
    got = run_color(c, device_table(c["n_views"], tc.CASES[name][2])).astype(np.float64)
    amb = tc.ambiguous(want)
    clear = ~amb
    b_col, b_den = color_bounds(want)
    e_col, e_den = np.abs(got[:, :3] - want["C"][:, :3]), np.abs(got[:, 3] - want["C"][:, 3])
    r_col = float((e_col[clear] / b_col[clear].clip(1e-300)).max()) if clear.any() else 0.0
    r_den = float((e_den[clear] / b_den[clear].clip(1e-300)).max()) if clear.any() else 0.0
    print(f"{name} opacity={with_opacity}: {got.shape[0]} nodes, {100.0 * amb.mean():.3f} % ambiguous, {int((want['C'][:, 3] > 0).sum())} coloured, "
          f"sum w {want['C'][:, 3].sum():.1f}, max |C - C_ref| / bound = {r_col:.4f} (colour) {r_den:.4f} (weight)")
    assert amb.mean() <= 0.02
    assert np.isfinite(got).all() and (got >= 0).all()
    assert np.all(e_den[clear] <= b_den[clear]) and np.all(e_col[clear] <= b_col[clear])
    untouched = clear & (want["n_views"] == 0)
    assert not got[untouched].any()                                # no view in or near the band: the node keeps its zeros
    if got.shape[0] > 1000:                                        # the case exercises what it is meant to
        w = want["C"][:, 3]
        assert (w == 0).any() and untouched.any() and ((w > 0) & (w < 0.1)).any() and (c["n_views"] < 8 or (w > 1.5).any())


def test_the_colours_hold_specks_and_the_un_compositing_bites():
    c = form("16x12x18-8-mixed", True)
    rgb = c["rgb"]
    assert np.isnan(rgb).any() and (rgb < 0).any() and (rgb > 1).any() and rgb[np.isfinite(rgb)].min() == np.float32(-0.3)
    op = c["opacity"]
    assert form("16x12x18-8-mixed", False)["opacity"] is None and np.isnan(op).any() and (op < 0.5).any() and (op == 0.5).any()
    assert ((op > 0.5) & (op < 1.0)).mean() > 0.5
    assert np.array_equal(op >= 0.5, tc.case("16x12x18-8-mixed")["opacity"] >= 0.5)            # the gate passes the pixels it passed
    args = (c["dims"], c["lo"], c["h"], c["c2w"], c["models"], c["lenses"], c["sizes"], c["depth"], op, 0.5, rgb)
    plain = cref.integrate_color(*args, None, c["trunc"])["C"]
    assert np.array_equal(plain[:, 3], c["want"]["C"][:, 3]) and np.abs(plain[:, :3] - c["want"]["C"][:, :3]).max() > 0.1
    cams = device_table(8, "mixed")
    without = run_color(c, cams, bg=None)                          # NULL is black
    assert np.array_equal(bits(without), bits(run_color(c, cams, bg=np.zeros(3, np.float32))))
    assert np.abs(without.astype(np.float64) - plain).max() < 1e-4 and not np.array_equal(without, run_color(c, cams))


# ------------------------------------------------------------------------------------------------------------ call forms
def test_split_ranges_an_empty_range_repeated_calls_and_equal_channels():
    c, cams = form("16x12x18-8-mixed", True), device_table(8, "mixed")
    whole = run_color(c, cams)
    for ranges in ([(0, 3), (3, 5)], [(v, 1) for v in range(8)], None):
        assert np.array_equal(bits(whole), bits(run_color(c, cams, ranges)))
    rng = np.random.default_rng(0)
    state = rng.standard_normal(whole.shape).astype(np.float32)
    same = run_color(c, cams, [(0, 0), (8, 0), (3, 0)], state=state)
    assert np.array_equal(bits(same), bits(state))                 # an empty range leaves C as it is, whatever it holds
    part = run_color(c, cams, [(0, 3)])
    assert np.array_equal(bits(run_color(c, cams, [(3, 5)], state=part)), bits(whole))
    # all-ones colours over a black background without an opacity map: u_c = 1, and fmaf(w, 1, C_c) is C_3 + w bit for bit
    c1 = form("33x31x35-8-mixed", False)
    ones = run_color(c1, cams, rgb=np.ones_like(c1["rgb"]), bg=np.zeros(3, np.float32))
    assert (ones[:, 3] > 0).sum() > 1000
    for k in range(3):
        assert np.array_equal(bits(ones[:, k]), bits(ones[:, 3]))
    assert np.array_equal(bits(ones[:, 3]), bits(run_color(c1, cams)[:, 3]))      # the weights do not depend on the colours


def test_host_layer_integrate_color(monkeypatch):
    from tinynerf_amd import tsdf
    c, cams = form("16x12x18-8-mixed", True), device_table(8, "mixed")
    whole = run_color(c, cams)
    box = [-1.0] * 3 + [1.0] * 3
    depth, opacity, rgb, bg = _dev(c["depth"]), _dev(c["opacity"]), _dev(c["rgb"]), _dev(BG)
    vol = tsdf.integrate_color(cams, depth, opacity, rgb, bg, box, c["dims"], c["trunc"])
    assert vol.shape == (19, 13, 17, 4) and np.array_equal(bits(vol.cpu().numpy().reshape(-1, 4)), bits(whole))
    monkeypatch.setattr(tsdf, "VIEWS_PER_LAUNCH", 3)               # chunks of 3, 3 and 2 views: the same bytes
    assert torch.equal(tsdf.integrate_color(cams, depth, opacity, rgb, bg, box, c["dims"], c["trunc"]), vol)
    half = tsdf.integrate_color(cams, depth, opacity, rgb, bg, box, c["dims"], c["trunc"], views=(0, 5))
    full = tsdf.integrate_color(cams, depth, opacity, rgb, bg, box, c["dims"], c["trunc"], state=half, views=(5, 3))
    assert full is half and torch.equal(full, vol)
    none = tsdf.integrate_color(cams, depth, None, rgb, None, box, c["dims"], c["trunc"])
    assert np.array_equal(bits(none.cpu().numpy().reshape(-1, 4)), bits(run_color(form("16x12x18-8-mixed", False), cams, bg=None)))
    with pytest.raises(ValueError):
        tsdf.integrate_color(cams, depth, opacity, rgb, bg, box, c["dims"], c["trunc"], min_opacity=0.0)
    with pytest.raises(ValueError):
        tsdf.integrate_color(cams, depth, opacity, rgb[:-1], bg, box, c["dims"], c["trunc"])
    with pytest.raises(ValueError):
        tsdf.integrate_color(cams, depth, opacity, rgb, bg, box, c["dims"], c["trunc"], state=vol[..., :3])


# ------------------------------------------------------------------------------------------------------------ sampling
def run_sample(vol, dims, lo, h, points):
    """tn_tsdf_sample_colors through the C ABI on an output with 64 guard bytes behind it -> [n,4] float32 numpy"""
    from tinynerf_amd import _lib as L
    from tinynerf_amd.mesh import _grid
    dev = torch.device(DEV)
    n = points.shape[0]
    out = torch.full((4 * n + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    v, p = _dev(np.asarray(vol).reshape(-1)), _dev(np.asarray(points).reshape(-1))
    lo_c, h_c, dims_c = _grid(lo, h, dims)
    L.call("tn_tsdf_sample_colors", dev, L.ptr(v), dims_c, lo_c, h_c, L.ptr(p), C.c_int64(n), L.ptr(out))
    torch.cuda.synchronize()
    assert bool((out[4 * n:] == SENTINEL).all()), "out was overrun"
    return out[:4 * n].cpu().numpy().reshape(n, 4)


def sample_bounds(want, dims):
    """(|dnum| [n,3], |dden| [n], bound on num / den [n,3] -- inf where den <= 2 |dden|): the docstring's"""
    moved = want["du"].sum(1)[:, None] * want["spread"] + 11.0 * E * want["size"]
    d_all = cref.SECOND * moved
    d_num, d_den = d_all[:, :3], d_all[:, 3]
    den = want["den"]
    safe = den > 2.0 * d_den
    room = np.where(safe, den - d_den, 1.0)
    quotient = (d_num + want["rgb"] * d_den[:, None]) / room[:, None] * (1.0 + E) + E * want["rgb"]
    return d_num, d_den, np.where(safe[:, None], quotient, np.inf)


def check_samples(got, want, dims, what):
    """the docstring's comparison of tn_tsdf_sample_colors' rows with the yardstick's; returns the largest error over bound"""
    got = got.astype(np.float64)
    _, d_den, b_rgb = sample_bounds(want, dims)
    assert np.isfinite(got).all()
    zero = want["den"] == 0
    exact = zero & (~want["near_face"] | ~want["finite"] | (want["size"][:, 3] == 0))
    assert not got[exact].any(), what
    e_den = np.abs(got[:, 3] - want["den"])
    assert np.all(e_den <= d_den), what
    compared = np.isfinite(b_rgb[:, 0])
    e_rgb = np.abs(got[:, :3] - want["rgb"])
    assert np.all(e_rgb[compared] <= b_rgb[compared]), what
    assert (got[:, :3] >= 0).all() and (got[want["den"] > 0, 3] >= 0).all()
    ratio = max(float((e_den / d_den.clip(1e-300)).max()), float((e_rgb[compared] / b_rgb[compared].clip(1e-300)).max()) if compared.any() else 0.0)
    return ratio, int(compared.sum()), int(zero.sum()), int((zero & ~exact).sum())


def sample_points(c, vol, n_random, seed):
    """points for a case's grid: the extractor's vertices of the case's own TSDF, uniform random ones, points exactly on nodes, on cell
    faces and on box faces, points outside the box, a NaN row -- shuffled, float32 [n,3]"""
    from tinynerf_amd import mesh as M, tsdf
    dev = torch.device(DEV)
    nx, ny, nz = c["dims"]
    S, W = (torch.from_numpy(a).to(dev).view(nz + 1, ny + 1, nx + 1) for a in run_integrate(c, device_table(c["n_views"], "mixed")))
    vertices = M.extract(tsdf.field(S, W), c["lo"], c["h"], 0.0)[0].cpu().numpy()
    assert vertices.shape[0] > 100
    rng = np.random.default_rng(seed)
    lo, h = c["lo"].astype(np.float64), c["h"].astype(np.float64)
    x = ref.nodes(c["dims"], c["lo"], c["h"])
    on_nodes = x[rng.integers(0, x.shape[0], 300)]
    cell = rng.integers(0, [nx, ny, nz], (300, 3))
    on_faces = lo + (cell + rng.random((300, 3))) * h
    axis = rng.integers(0, 3, 300)
    on_faces[np.arange(300), axis] = x.reshape(nz + 1, ny + 1, nx + 1, 3)[cell[:, 2], cell[:, 1], cell[:, 0]][np.arange(300), axis]
    on_box = rng.uniform(-1.0, 1.0, (200, 3))
    on_box[np.arange(200), rng.integers(0, 3, 200)] = rng.choice([-1.0, 1.0], 200)
    outside = rng.uniform(-1.0, 1.0, (200, 3))
    outside[np.arange(200), rng.integers(0, 3, 200)] = rng.choice([-1.0, 1.0], 200) * rng.uniform(1.0, 40.0, 200)
    outside[:4] = [[1e30, 0.0, 0.0], [0.0, -1e30, 0.0], [3.0e38, 3.0e38, -3.0e38], [-5.0, 7.0, 9.0]]
    bad = np.float64([[np.nan, 0.1, 0.2], [0.1, np.inf, 0.2], [0.1, 0.2, -np.inf], [np.nan] * 3])
    points = np.concatenate([vertices, rng.uniform(-1.0, 1.0, (n_random, 3)), on_nodes, on_faces, on_box, outside, bad]).astype(np.float32)
    return points[rng.permutation(points.shape[0])]


@pytest.mark.parametrize("name", ["16x12x18-8-mixed", "33x31x35-8-mixed"])
def test_sample_colors_against_the_yardstick(name):
    c = form(name, True)
    nx, ny, nz = c["dims"]
    vol = run_color(c, device_table(8, "mixed")).reshape(nz + 1, ny + 1, nx + 1, 4).copy()
    vol[nz // 4:nz // 2 + 2, ny // 3:ny // 3 + 5, nx // 2 - 3:nx // 2 + 4] = 0.0      # a block without colour, across the surface
    points = sample_points(c, vol, 2500, 11)
    want = cref.sample_colors(vol.reshape(-1, 4), c["dims"], c["lo"], c["h"], points)
    got = run_sample(vol, c["dims"], c["lo"], c["h"], points)
    ratio, compared, zero, loose = check_samples(got, want, c["dims"], name)
    n = points.shape[0]
    mixed = ((want["den"] > 0) & (want["size"][:, 3] > 0) & (want["spread"][:, 3] == want["size"][:, 3])).sum()
    print(f"{name}: {n} points, {compared} quotients compared, {zero} rows with den = 0 ({loose} of them within du of a face beside colour), "
          f"{int(mixed)} cells with an uncoloured node nearby, max error / bound = {ratio:.4f}")
    assert n > 3000 and compared > n // 5 and zero > 100 and mixed > 50
    for m in (1, 255, 256, 257):                                   # a lone lane, a workgroup less one, a full one, one lane into the next
        part = run_sample(vol, c["dims"], c["lo"], c["h"], points[:m])
        assert np.array_equal(bits(part), bits(got[:m])), m
    # the host layer: the same rows, split into colours and weights
    from tinynerf_amd import tsdf
    rgb, den = tsdf.sample_colors(_dev(vol), [-1.0] * 3 + [1.0] * 3, c["dims"], _dev(points))
    assert rgb.shape == (n, 3) and den.shape == (n,)
    assert np.array_equal(bits(rgb.cpu().numpy()), bits(got[:, :3])) and np.array_equal(bits(den.cpu().numpy()), bits(got[:, 3]))
    empty = tsdf.sample_colors(_dev(vol), [-1.0] * 3 + [1.0] * 3, c["dims"], _dev(points)[:0])
    assert empty[0].shape == (0, 3) and empty[1].shape == (0,)


# ------------------------------------------------------------------------------------------------------------ sphere, end to end
SPHERE_BG = np.float32([0.2, 0.7, 0.1])


def corner_max(field, idx, dims):
    """per point the largest value of the per-node `field` over the 8 corners of its cell `idx`"""
    nx, ny, nz = dims
    f = field.reshape(nz + 1, ny + 1, nx + 1)
    out = np.zeros(idx.shape[0])
    for dx, dy, dz in cref.CORNERS:
        out = np.maximum(out, f[idx[:, 2] + dz, idx[:, 1] + dy, idx[:, 0] + dx])
    return out


def test_a_sphere_coloured_by_its_normals():
    """6j's sphere -- rays from tn_camera_rays itself, analytic depths, eight views from the corners of a cube, radius 0.6 in the +-1
    box, 32 cells a side -- with analytic colours 0.5 + 0.4 n, composited at opacity 0.8 over SPHERE_BG; where the sphere is missed the
    pixel is the background at opacity 0.  The tolerance against the analytic colour is pixel and cell discretisation, which nobody
    can derive: twice the float64 pipeline's own largest deviation (DESIGN 6k has the figure)."""
    from tinynerf_amd import mesh as M, tsdf
    from tinynerf_amd.rays import CameraRays
    dev = torch.device(DEV)
    eyes = [2.6 / np.sqrt(3.0) * np.array([a, b, c]) for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)]
    c2w = np.float32(np.stack([ref.look_at(e) for e in eyes]))
    lens = np.float32([[176.0, 176.0, 64.37, 63.79, 0, 0, 0, 0, 0, 0]] * 8)
    sizes = np.int64([[128, 128]] * 8)
    cams = CameraRays(torch.from_numpy(c2w), torch.from_numpy(lens), [0] * 8, sizes.tolist(), None, dev)
    depth, opacity, rgb = [], [], []
    for i in range(8):
        o, d = (t.cpu().numpy().astype(np.float64).reshape(-1, 3) for t in cams.image_rays(i))
        t = ref.sphere_depth(o, d, tc.RADIUS)
        hit = np.isfinite(t)
        normal = (o + np.where(hit, t, 0.0)[:, None] * d) / tc.RADIUS
        colour = np.where(hit[:, None], 0.8 * (0.5 + 0.4 * normal) + 0.2 * SPHERE_BG.astype(np.float64), SPHERE_BG.astype(np.float64))
        depth.append(t), opacity.append(np.where(hit, 0.8, 0.0)), rgb.append(colour)
    depth, opacity, rgb = (np.concatenate(a).astype(np.float32) for a in (depth, opacity, rgb))
    dims, box = (32, 32, 32), [-1.0] * 3 + [1.0] * 3
    lo, h, _ = M.grid_dims(box, 32)
    trunc = 4.0 * float(h.max())
    d_dev, o_dev, c_dev, bg_dev = _dev(depth), _dev(opacity), _dev(rgb), _dev(SPHERE_BG)
    S, W = tsdf.integrate(cams, d_dev, o_dev, box, dims, trunc)
    vol = tsdf.integrate_color(cams, d_dev, o_dev, c_dev, bg_dev, box, dims, trunc)
    vertices, normals, faces, cells = M.extract_with_cells(tsdf.field(S, W), lo, h, 0.0)
    faces = tsdf.mask_faces(W, dims, cells, vertices.size(0), faces)
    vertices, normals, _, faces = M.filter_components(vertices, normals, None, faces, min_faces=1)
    got_rgb, got_den = (t.cpu().numpy().astype(np.float64) for t in tsdf.sample_colors(vol, box, dims, vertices))
    V = vertices.size(0)
    assert V > 1000 and (got_den > 0).all()                        # every surviving vertex has colour
    # the float64 pipeline on the same inputs, at the same vertices
    p = vertices.cpu().numpy()
    table = (c2w.astype(np.float64), np.int64([0] * 8), lens.astype(np.float64), sizes)
    want_vol = cref.integrate_color(dims, lo, h, *table, depth, opacity, 0.5, rgb, SPHERE_BG, trunc, margins=True)
    exact = cref.sample_colors(want_vol["C"], dims, lo, h, p, volume64=True)
    # (a) the kernel's rows against the yardstick's rows of the kernel's own volume: the sampling bound
    own = cref.sample_colors(vol.cpu().numpy().reshape(-1, 4), dims, lo, h, p)
    ratio = check_samples(np.concatenate([got_rgb, got_den[:, None]], 1), own, dims, "sphere")[0]
    # (b) the yardstick's rows of the two volumes, both float64 in the same cell: the weights t_k sum to 1, so numerators and
    #     denominator move by at most the largest integration bound among the cell's 8 corners, and the quotient follows.  A vertex
    #     with an ambiguous corner is left out of this comparison (not of (a) or (c), which cover every vertex).  How many that may be
    #     cannot be derived from the 2 % allowed among the grid's nodes: 35 937 nodes stand against some 1 800 vertices, ambiguity
    #     follows the pixel edges and so is not independent from node to node, and 2 % of the nodes, each a corner of 8 cells, could
    #     touch every vertex.  What can be held to the issue's 2 % is the set of nodes this comparison rests on -- the corners of the
    #     vertices' cells --, and the share of the vertices then follows from counting: a vertex is left out for at least one
    #     ambiguous corner, an ambiguous corner node belongs to at most 8 of the cells, so at most 8 x (ambiguous corner nodes) vertices are left out
    b_col, b_den = color_bounds(want_vol)
    ambiguous = tc.ambiguous(want_vol)
    amb = corner_max(ambiguous.astype(np.float64), exact["idx"], dims) > 0
    d_num = np.stack([corner_max(b_col[:, k], exact["idx"], dims) for k in range(3)], 1)
    d_den = corner_max(b_den, exact["idx"], dims)
    moved = (d_num + exact["rgb"] * d_den[:, None]) / (exact["den"] - d_den)[:, None]
    _, _, b_own = sample_bounds(own, dims)
    err = np.abs(got_rgb - exact["rgb"])
    clear = ~amb
    corners = np.zeros(ambiguous.shape, bool)
    nodes_x, nodes_xy = dims[0] + 1, (dims[0] + 1) * (dims[1] + 1)
    for dx, dy, dz in cref.CORNERS:
        corners[(exact["idx"][:, 0] + dx) + nodes_x * (exact["idx"][:, 1] + dy) + nodes_xy * (exact["idx"][:, 2] + dz)] = True
    ambiguous_corners = int((ambiguous & corners).sum())
    assert ambiguous.mean() <= 0.02 and ambiguous_corners <= 0.02 * corners.sum() and amb.sum() <= 8 * ambiguous_corners
    assert np.isfinite(b_own).all() and (exact["den"] > 2.0 * d_den).all()
    assert np.all(err[clear] <= (b_own + moved)[clear])
    # (c) against the analytic colour
    analytic = 0.5 + 0.4 * p / np.linalg.norm(p, axis=1, keepdims=True)
    deviation = float(np.abs(exact["rgb"] - analytic).max())
    tolerance = 2.0 * deviation
    worst = float(np.abs(got_rgb - analytic).max())
    no_bg = tsdf.integrate_color(cams, d_dev, o_dev, c_dev, None, box, dims, trunc)
    leaked = tsdf.sample_colors(no_bg, box, dims, vertices)[0].cpu().numpy().astype(np.float64)
    miss = np.abs(leaked - analytic)
    print(f"sphere: {V} vertices, {100.0 * ambiguous.mean():.3f} % of the nodes ambiguous, {100.0 * ambiguous_corners / corners.sum():.3f} % of the {int(corners.sum())} corner nodes, {100.0 * amb.mean():.2f} % of the vertices beside one, sampling error / bound {ratio:.4f}, "
          f"max |rgb - float64 pipeline| = {float(err[clear].max()):.3e} (bound {float((b_own + moved)[clear].max()):.3e}); float64 pipeline "
          f"against 0.5 + 0.4 n: {deviation:.4f}, kernels: {worst:.4f}, tolerance {tolerance:.4f}; without taking bg out: "
          f"largest miss {float(miss.max()):.4f}, smallest per-vertex miss {float(miss.max(1).min()):.4f}")
    assert worst <= tolerance
    assert float(miss.max()) > tolerance                           # the background leaks unless it is taken out
    assert bool(torch.equal(no_bg[..., 3], vol[..., 3]))           # (the weights are the same volume)


# ------------------------------------------------------------------------------------------------------------ training, end to end
STEPS = 200                                                        # 6j's tiny K-Planes scene: 148 vertices after 200 steps, none after 20


def test_train_writes_a_tsdf_mesh_with_fused_colours(tmp_path, monkeypatch):
    from tinynerf_amd import data, mesh as M, tsdf
    from tinynerf_amd.run import TrainConfig, train
    _scene_on_disk(tmp_path)
    dev = torch.device(DEV)
    train_rays = data.RaysDataset(data.parse_nerf_synthetic(tmp_path, "train"), dev)
    test_set = data.PoseDataset(data.parse_nerf_synthetic(tmp_path, "test"), dev)
    asked = []
    decoder = M.vertex_colors
    monkeypatch.setattr(M, "vertex_colors", lambda trainer, vertices, normals, *a, **k: (asked.append(vertices.size(0)), decoder(trainer, vertices, normals, *a, **k))[1])

    def go(name, **more):
        out = tmp_path / name
        out.mkdir()
        cfg = TrainConfig(method="kplanes", batch_size=512, n_samples=64, occupancy_res=32, seed=3, kplanes_resolutions=(16, 32, 64))
        return out, train(cfg, train_rays, None, test_set, out, max_steps=STEPS, log_every=1000, **more)[0]

    out, tr = go("fused", tsdf_mesh=24, tsdf_colors="fused")
    vert, nrm, rgb, faces = M.read_mesh_ply(out / "tsdf_mesh.ply")
    calls_in_train = list(asked)
    assert ((faces >= 0) & (faces < vert.shape[0])).all() and np.unique(faces).size == vert.shape[0]
    # the same call by hand gives the same file
    got = tsdf.export_tsdf_mesh(tr, test_set, out / "again.ply", resolution=24, colors="fused")
    assert open(out / "again.ply", "rb").read() == open(out / "tsdf_mesh.ply", "rb").read() and got[0].size(0) == vert.shape[0]
    assert got[2].dtype == torch.uint8 and got[2].shape == (vert.shape[0], 3)
    # geometry does not depend on where the colours come from; the decoder is asked about the vertices without fused colour alone
    del asked[:]
    plain = tsdf.export_tsdf_mesh(tr, test_set, out / "decoder.ply", resolution=24)
    assert asked == ([vert.shape[0]] if vert.shape[0] else [])
    for k in (0, 1, 3):
        assert torch.equal(plain[k], got[k])
    differing = int((plain[2] != got[2]).any(1).sum())
    print(f"tsdf_mesh.ply after {STEPS} steps: {vert.shape[0]} vertices, {faces.shape[0]} faces; the decoder was asked about {calls_in_train} vertices "
          f"in the fused export; {differing} vertices differ in colour from the decoder's export")
    assert all(0 < n < vert.shape[0] for n in calls_in_train) and len(calls_in_train) <= 1
    if STEPS >= 200:
        assert vert.shape[0] > 50 and differing > 0
    # a vertex without fused colour (den == 0) takes the decoder's colour, and the decoder is asked about those alone
    sampler = tsdf.sample_colors

    def thinned(*a):
        colour, den = sampler(*a)
        den[::3] = 0.0
        return colour, den
    monkeypatch.setattr(tsdf, "sample_colors", thinned)
    del asked[:]
    mixed = tsdf.export_tsdf_mesh(tr, test_set, None, resolution=24, colors="fused")
    monkeypatch.setattr(tsdf, "sample_colors", sampler)
    V = vert.shape[0]
    assert asked == ([len(range(0, V, 3))] if V else [])
    assert torch.equal(mixed[2][::3], plain[2][::3]) and torch.equal(mixed[2][1::3], got[2][1::3]) and torch.equal(mixed[2][2::3], got[2][2::3])
    # the default keyword writes the decoder's file, the parent's
    out2, tr2 = go("default", tsdf_mesh=24)
    tsdf.export_tsdf_mesh(tr2, test_set, out2 / "again.ply", resolution=24, colors=True)
    assert open(out2 / "again.ply", "rb").read() == open(out2 / "tsdf_mesh.ply", "rb").read()
    with pytest.raises(ValueError):
        tsdf.export_tsdf_mesh(tr2, test_set, None, resolution=24, colors="nonsense")
