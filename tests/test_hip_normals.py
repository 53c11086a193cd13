"""GPU tests of the surface normals (tn_kplanes_normals / tn_hashgrid_normals / tn_ray_normals, core.sample_normals,
NerfRenderer.render_maps(normals=True), train(normals=True)) against the float64 yardstick tests/_normals_ref.py.

Bounds.  grad: |got - ref| <= (F + 64 + 16) 2^-24 A per element, A the sum of the absolute values of the terms of the nested sum over
hidden units, features and taps -- the worst case of an fp32 evaluation in any order.  Rows with a ReLU tie in the yardstick
(|h_j| <= 1e-5 (sum |W1 f| + |b1|)) or a non-finite x are skipped.  normals: unit to 4 2^-24 or exactly 0; exactly 0 for gated rows and
rows with a non-finite x; |n_got - n_ref| <= 2 bound(v) / |v_ref| + 8 2^-24 with bound(v) the gradient bound pushed through |J|^T; rows
where that passes 1e-2 are left to the gradient comparison.  At most 1 % of a case's finite rows are skipped either way
(tests/test_normals_ref.py holds the seeds to that on the CPU).  Ray normals: the sum to (count + 8) 2^-24 sum |w n|, then the
normalisation.  The largest observed ratios are printed; DESIGN 6g records them."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import _hashgrid_ref as hg
import _normals_cases as cases
import _normals_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------------- ABI helpers
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def head_desc(m, keep):
    from tinynerf_amd import _lib as L
    d = L.MlpDesc()
    d.n_layers, d.in_dim, d.encoding = 2, m["F"], L.ENC_NONE
    d.dims[0], d.dims[1], d.dims[2] = m["F"], 64, 1
    w1, b1, w2, b2 = _t(m["W1"]), _t(m["b1"]), _t(m["w2"]), _t(np.array([m["b2"]], np.float32))
    keep += [w1, b1, w2, b2]
    d.weights[0], d.biases[0], d.weights[1], d.biases[1] = w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr()
    return d


def field_desc(m, keep):
    from tinynerf_amd import _lib as L
    if m["field"] == "kplanes":
        d = L.KPlanesDesc()
        d.n_scales, d.channels = len(m["planes"]), m["planes"][0][0].shape[2]
        for s, scale in enumerate(m["planes"]):
            d.height[s], d.width[s] = scale[0].shape[:2]
            for p in range(3):
                t = _t(scale[p])
                keep.append(t)
                d.planes[s][p] = t.data_ptr()
        return "tn_kplanes_normals", d
    res, hashed, entries, offsets = m["plan"]
    d = L.HashGridDesc()
    d.n_levels, d.features = len(res), m["table"].shape[1]
    for l in range(len(res)):
        d.res[l], d.hashed[l], d.entries[l], d.offset[l] = res[l], int(hashed[l]), entries[l], offsets[l]
    t = _t(m["table"])
    keep.append(t)
    d.table = t.data_ptr()
    return "tn_hashgrid_normals", d


def frame_desc(kind):
    from tinynerf_amd import _lib as L
    f = L.NormalFrame(contraction=kind)
    for i in range(6):
        f.aabb[i] = cases.BOX[i]
    return f


def run_kernel(m, x, kind, stride=3, gate=None, want=("normals", "grad")):
    """-> (normals, grad) numpy (None where not asked for); the other columns of a strided x hold NaN"""
    from tinynerf_amd import _lib as L
    keep = []
    name, fd = field_desc(m, keep)
    hd = head_desc(m, keep)
    n = len(x)
    xb = torch.full((n, stride), float("nan"), device=DEV)
    xb[:, :3] = _t(np.array(x))
    nrm = torch.full((n, 3), float("nan"), device=DEV) if "normals" in want else None
    grd = torch.full((n, 3), float("nan"), device=DEV) if "grad" in want else None
    g = None if gate is None else _t(gate.astype(np.float32))
    fr = frame_desc(kind)
    L.call(name, torch.device(DEV), C.byref(fd), L.ptr(xb), C.c_int64(stride), C.c_int64(n), C.byref(hd), C.byref(fr), L.ptr(g),
           L.ptr(nrm), L.ptr(grd))
    torch.cuda.synchronize()
    return (None if nrm is None else nrm.cpu().numpy(), None if grd is None else grd.cpu().numpy())


def check_grad(c, got, rows, tag):
    use = rows & c["finite"] & ~c["tie"]
    err, bound = np.abs(got.astype(np.float64) - c["grad"])[use], c["bound"][use]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    worst = ratio.max(initial=0.0)
    print(f"{tag}: grad error / bound, largest of {int(use.sum())} rows: {worst:.3f}")
    assert worst <= 1.0, (tag, worst)
    return worst


def check_normals(c, got, kind, rows, tag):
    r = c["normals"][kind]
    got = got.astype(np.float64)
    length = np.sqrt((got * got).sum(1))
    is_zero = (got == 0).all(1)
    assert (is_zero | (np.abs(length - 1) <= 4 * U)).all(), tag                    # unit or exactly 0, every row
    assert is_zero[~c["finite"]].all(), tag                                       # a non-finite x: exactly 0
    use = rows & c["finite"] & ~c["tie"]
    assert is_zero[use & r["zero"]].all(), tag                                    # nothing to differentiate: exactly 0
    cmp = use & ~r["zero"] & ~r["loose"]
    err = np.sqrt(((got - r["n"]) ** 2).sum(1))[cmp]
    worst = (err / r["tol"][cmp]).max(initial=0.0)
    print(f"{tag}: normal error / bound, largest of {int(cmp.sum())} rows: {worst:.3f}")
    assert worst <= 1.0, (tag, worst)


# ---------------------------------------------------------------------------------------------------------------- the two kernels
@pytest.mark.parametrize("n", cases.NS)
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_gradient_and_normals_against_the_yardstick(name, n):
    """every case at every n: grad (stride 3, none frame) and the normals of all four frames (stride 7: the packed layout)"""
    m, c = cases.model(name), cases.reference(name, n)
    every = np.ones(n, bool)
    nrm, grd = run_kernel(m, c["x"], ref.NONE, stride=3)
    check_grad(c, grd, every, f"{name} n={n}")
    check_normals(c, nrm, ref.NONE, every, f"{name} n={n} none")
    for kind in (ref.AABB, ref.MIP_INF, ref.MIP_L2):
        nrm2, grd2 = run_kernel(m, c["x"], kind, stride=7)
        assert np.array_equal(grd2.view(np.uint32), grd.view(np.uint32))          # the frame and the stride do not touch grad
        check_normals(c, nrm2, kind, every, f"{name} n={n} frame {kind}")
    only_n, none = run_kernel(m, c["x"], ref.NONE, want=("normals",))
    none2, only_g = run_kernel(m, c["x"], ref.NONE, want=("grad",))
    assert none is None and none2 is None
    assert np.array_equal(only_n.view(np.uint32), nrm.view(np.uint32)) and np.array_equal(only_g.view(np.uint32), grd.view(np.uint32))


@pytest.mark.parametrize("name", ["kplanes_3x32_r4_9_16", "kplanes_1x4", "hashgrid_small_f4"])
def test_gates(name):
    """single rows, a whole tile and every row gated: zeros there, the ungated rows keep their bits"""
    n = 197
    m, c = cases.model(name), cases.reference(name, n)
    nrm0, grd0 = run_kernel(m, c["x"], ref.AABB, stride=7)
    rng = np.random.default_rng(3)
    single = np.ones(n)
    single[[0, 5, 31, 32, 100, 196]] = 0
    tile = rng.uniform(0.1, 1, n)
    tile[64:96] = 0                                                                # tile 2 of 7
    tile[130] = 0
    for tag, gate in (("single", single), ("tile", tile), ("all", np.zeros(n))):
        nrm, grd = run_kernel(m, c["x"], ref.AABB, stride=7, gate=gate)
        off = gate == 0
        assert (nrm[off] == 0).all() and (grd[off] == 0).all(), (name, tag)
        assert np.array_equal(nrm[~off].view(np.uint32), nrm0[~off].view(np.uint32)), (name, tag)
        assert np.array_equal(grd[~off].view(np.uint32), grd0[~off].view(np.uint32)), (name, tag)


def test_a_dead_tile_reads_no_texel():
    """a 32-row tile whose gates are all 0 is not evaluated: its rows come out 0 although its planes hold NaN everywhere"""
    m = dict(cases.model("kplanes_2x8_6x11"))
    m["planes"] = [[np.full_like(p, np.nan) for p in scale] for scale in m["planes"]]
    x = cases.points("kplanes_2x8_6x11", 64)
    nrm, grd = run_kernel(m, x, ref.NONE, gate=np.zeros(64))
    assert (nrm == 0).all() and (grd == 0).all()
    live = np.zeros(64)
    live[40] = 1
    nrm, grd = run_kernel(m, x, ref.NONE, gate=live)
    assert (grd[:32] == 0).all() and np.isnan(grd[40]).all() and (nrm == 0).all()  # tile 1 was evaluated (NaN), tile 0 was not


def test_analytic_cases():
    """a linear dense hash-grid level -> the constant normal -a/|a| inside; planes that vary along x0 only -> -e0, also under the
    non-cubic AABB frame (no yardstick involved)"""
    a = np.array([0.3, -1.1, 0.7])
    plan, table = ref.linear_hashgrid(6, 2, a, 0)
    W1, b1, w2, b2 = ref.make_head(2, 1, positive=True)
    m = dict(field="hashgrid", plan=plan, table=table, F=2, W1=W1, b1=b1, w2=w2, b2=b2)
    x = np.random.default_rng(2).uniform(-0.999, 0.999, (500, 3)).astype(np.float32)
    nrm, _ = run_kernel(m, x, ref.NONE)
    assert np.abs(nrm + a / np.linalg.norm(a)).max() < 2e-5
    sizes = [(5, 7), (9, 4)]
    W1, b1, w2, b2 = ref.make_head(8, 4, positive=True)
    m = dict(field="kplanes", planes=ref.x0_planes(2, 4, sizes, 3), F=8, W1=W1, b1=b1, w2=w2, b2=b2)
    for kind in (ref.NONE, ref.AABB):
        nrm, grd = run_kernel(m, x, kind)
        assert (grd[:, 0] > 0).all() and np.abs(grd[:, 1:]).max() <= 1e-5 * np.abs(grd[:, 0]).max()
        assert np.abs(nrm - np.array([-1.0, 0, 0])).max() < 2e-5, kind


def test_plane_cell_agrees_with_plane_taps_at_nodes_and_faces():
    """the derivative is taken in the cell the forward interpolates in: at exact nodes, the last node and just off the faces the
    kernel's gradient stays within the bound of the yardstick, which forms ix, iy as plane_taps does -- a derivative taken in the
    neighbouring cell is off by a whole term"""
    m = cases.model("kplanes_2x8_6x11")
    H, W = 6, 11
    xs = []
    for q in range(W):
        u = np.float32(2.0 * q / (W - 1) - 1.0)
        for v in (u, np.nextafter(u, np.float32(2)), np.nextafter(u, np.float32(-2))):
            xs.append([v, np.float32(2.0 * (q % H) / (H - 1) - 1.0), np.float32(0.3)])
    x = np.array(xs, np.float32)
    grad, A, tie = cases.gradient(m, x)
    _, got = run_kernel(m, x, ref.NONE, want=("grad",))
    use = ~tie
    assert use.sum() >= len(x) - 1
    assert (np.abs(got - grad)[use] <= ref.grad_bound(A, m["F"])[use]).all()


# -------------------------------------------------------------------------------------------------------------------- ray normals
@pytest.mark.parametrize("n_rays", [0, 1, 63, 64, 65, 200])
def test_ray_normals(n_rays):
    from tinynerf_amd import _lib as L
    rng = np.random.default_rng(n_rays)
    counts = rng.integers(0, 150, n_rays).astype(np.int32)
    if n_rays > 2:
        counts[1] = 0                                                              # a ray without samples
        counts[2] = 129                                                            # more than two chunks of 64
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int32) if n_rays else np.zeros(0, np.int32)
    info = np.stack([starts, counts], 1).astype(np.int32).reshape(n_rays, 2)
    N = int(counts.sum())
    w = rng.uniform(0, 0.2, N).astype(np.float32)
    nrm = rng.standard_normal((N, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    if n_rays > 4:
        w[starts[3]:starts[3] + counts[3]] = 0                                     # all-zero weights
    out = torch.full((n_rays, 3), float("nan"), device=DEV)
    wt, nt, it = _t(w), _t(nrm), _t(info)
    L.call("tn_ray_normals", torch.device(DEV), L.ptr(wt), L.ptr(nt), L.ptr(it), C.c_int64(n_rays), L.ptr(out))
    got = out.cpu().numpy().astype(np.float64)
    if n_rays == 0:
        return
    S, A, cnt = ref.ray_normals(w, nrm, info)
    norm = np.sqrt((S * S).sum(1))
    dead = A.sum(1) == 0
    assert (got[dead] == 0).all()
    length = np.sqrt((got * got).sum(1))
    assert (np.abs(length[~dead] - 1) <= 4 * U).all()
    # the sum is held to (count + 8) 2^-24 sum |w n| per component, the unit vector to twice that over |N| plus the normalisation
    bound = (cnt + 8)[:, None] * U * A
    tol = 2 * np.sqrt((bound * bound).sum(1))[~dead] / norm[~dead] + 8 * U
    err = np.sqrt(((got - S / np.where(dead, 1, norm)[:, None]) ** 2).sum(1))[~dead]
    print(f"n_rays={n_rays}: ray normal error / bound {np.max(err / tol, initial=0.0):.3f}")
    assert (err <= tol).all()
    all_zero = torch.full((n_rays, 3), float("nan"), device=DEV)
    zw = torch.zeros_like(wt)
    L.call("tn_ray_normals", torch.device(DEV), L.ptr(zw), L.ptr(nt), L.ptr(it), C.c_int64(n_rays), L.ptr(all_zero))
    assert (all_zero == 0).all()


# ----------------------------------------------------------------------------------------------------------------------- renderer
def _renderer(method):
    """a renderer whose sigma head is drawn like the kernel cases' (tests/_normals_ref.make_head: half of the hidden units on, little
    cancellation over them -- torch's default initialisation leaves 11 % of the samples' normal bounds above 1e-2), scaled so that the
    density saturates a ray within a few dozen samples; fields of either sign"""
    from tinynerf_amd import core, models
    torch.manual_seed(7)
    if method == "kplanes":
        field = models.KPlanesFeatureField(32, (8, 12, 16))
        with torch.no_grad():
            for p in field.plane_tensors():
                p.uniform_(-1, 1)
    else:
        field = models.HashGridFeatureField(4, 2, 10, 4, 32)
        with torch.no_grad():
            field.table.uniform_(-1, 1)
    F = field.feature_dim
    r = core.NerfRenderer(field, models.VanillaOpacityDecoder(F), models.VanillaColorDecoder(8, F, 64, 3), torch.ones(3)).to(DEV)
    W1, b1, w2, _ = ref.make_head(F, 21)
    scale = 0.125 if method == "kplanes" else 0.5
    with torch.no_grad():
        for p, v in zip(r.sigma_decoder.net.params(), (W1 * scale, b1 * scale, w2 * scale, np.array([2.0], np.float32))):
            p.copy_(torch.from_numpy(np.ascontiguousarray(v)))
    return r


@pytest.mark.parametrize("method", ["kplanes", "hashgrid"])
def test_render_maps_with_normals(method):
    from tinynerf_amd import core
    r = _renderer(method)
    dev = torch.device(DEV)
    aabb = torch.tensor([[-1.5] * 3, [1.5] * 3], device=dev)
    grid = core.OccupancyGrid(16, 1 / 64.).to(dev)                                  # all ones: full occupancy
    R, S = 96, 48
    torch.manual_seed(1)
    o = torch.nn.functional.normalize(torch.randn(R, 3, device=dev), dim=-1) * 3.5
    d = torch.nn.functional.normalize(-o + 0.3 * torch.randn(R, 3, device=dev), dim=-1)
    d[:4] = torch.nn.functional.normalize(o[:4], dim=-1)                            # four rays that miss the box: opacity 0
    contraction = core.ContractionAABB(aabb)
    provider = core.RayProvider(grid, contraction, core.RayMarcherAABB(aabb, S, 0.1))
    packed, info, t = provider(o, d, training=False, return_t=True)
    r.normal_frame = core.normal_frame(contraction)
    with torch.no_grad():
        plain = r.render_maps(packed, info, t)
        full = r.render_maps(packed, info, t, normals=True)
    assert sorted(plain) == ["depth", "median_depth", "opacity", "rgb"] and sorted(full) == sorted(list(plain) + ["normal"])
    for k in plain:
        assert torch.equal(plain[k].view(torch.int32), full[k].view(torch.int32)), k
    assert full["normal"].shape == (R, 3)
    assert (full["normal"][full["opacity"] == 0] == 0).all() and (full["opacity"][:4] == 0).all()
    # the pass by hand, on the weights the forward composited with
    stats = r.__dict__.setdefault("_stats", {})
    handout = {}
    stats["maps_handout"] = handout
    with torch.no_grad():
        r(packed, info)
    stats.pop("maps_handout")
    w = handout["weights"].detach()
    with torch.no_grad():
        sn, sg = core.sample_normals(r, packed, gate=w, return_grad=True)
        by_hand = core.ray_normals(w, sn, info)
    assert torch.equal(by_hand.view(torch.int32), full["normal"].view(torch.int32))
    assert (sn[w == 0] == 0).all() and (sg[w == 0] == 0).all()
    # ... and against the yardstick
    head = [p.detach().cpu().numpy() for p in r.sigma_decoder.net.params()]
    x = packed[:, :3].cpu().numpy()
    if method == "kplanes":
        planes = [[p.detach().permute(0, 2, 3, 1)[0].cpu().numpy() for p in r.feature_module.plane_tensors()[3 * s:3 * s + 3]] for s in range(3)]
        grad, A, tie = ref.kplanes_gradient(planes, x, head[0], head[1], head[2])
    else:
        grad, A, tie = ref.hashgrid_gradient(r.feature_module.table.detach().cpu().numpy(), x, r.feature_module.plan, head[0], head[1], head[2])
    F = r.feature_module.feature_dim
    bound = ref.grad_bound(A, F)
    live = (w.cpu().numpy() != 0) & ~tie
    assert tie.sum() <= 0.01 * len(x)
    assert (np.abs(sg.cpu().numpy() - grad)[live] <= bound[live]).all()
    nref, v, bv, ok = ref.normals(ref.AABB, x, grad, bound, [-1.5] * 3 + [1.5] * 3)
    vn, bvn = np.sqrt((v * v).sum(1)), np.sqrt((bv * bv).sum(1))
    zero = (vn == 0) & (bvn == 0)                           # every hidden unit off: nothing to differentiate, the normal is exactly 0
    assert (sn.cpu().numpy()[live & zero] == 0).all()
    tol = 2 * bvn / np.maximum(vn, 1e-300) + 8 * U
    cmp = live & ok & ~zero & (tol <= 1e-2)
    skipped = live & ~zero & ~cmp
    assert skipped.sum() <= 0.01 * live.sum(), (int(skipped.sum()), int(live.sum()))                      # the cap of the kernel cases
    print(f"{method}: {int(live.sum())} live samples, {int((live & zero).sum())} without a gradient, {int(skipped.sum())} left to the gradient comparison")
    # rays: the fp64 sum of the yardstick's normals under the handed-out weights
    wn = np.where(live[:, None], nref, sn.cpu().numpy().astype(np.float64))
    Sr, Ar, cnt = ref.ray_normals(w.cpu().numpy(), wn, info.cpu().numpy())
    per_sample = np.where(cmp, tol, np.where(skipped, 2.0, 0.0))       # a sample left out above may point anywhere; a dead one enters as it is
    extra = np.array([(np.abs(w.cpu().numpy()[s:s + c]) * per_sample[s:s + c]).sum() for s, c in info.cpu().numpy()])
    norm = np.sqrt((Sr * Sr).sum(1))
    hit = norm > 0
    rtol = 2 * (np.sqrt((((cnt + 8)[:, None] * U * Ar) ** 2).sum(1)) + extra)[hit] / norm[hit] + 8 * U
    err = np.sqrt(((full["normal"].cpu().numpy() - Sr / np.where(hit, norm, 1)[:, None]) ** 2).sum(1))[hit]
    assert (err <= rtol).all()


def test_sample_normals_refuses_other_fields():
    from tinynerf_amd import core, models
    r = core.NerfRenderer(models.VanillaFeatureMLP(4, 64, 2), models.VanillaOpacityDecoder(64), models.VanillaColorDecoder(4, 64, 64, 1)).to(DEV)
    with pytest.raises(NotImplementedError, match="VanillaFeatureMLP"):
        core.sample_normals(r, torch.zeros(4, 7, device=DEV))


# --------------------------------------------------------------------------------------------------------------------- end to end
def _scene_on_disk(root):
    """a 16 x 16 synthetic ball in Blender format: two views, both also the test split"""
    from PIL import Image
    from tinynerf_amd import rays
    o, d, rgb, K, cams = rays.synthetic_scene(n_views=2, res=16, seed=5, device="cpu")
    imgs = (rgb.reshape(2, 16, 16, 3) * 255).to(torch.uint8).numpy()
    (root / "train").mkdir()
    frames = []
    for i in range(2):
        Image.fromarray(imgs[i]).save(root / "train" / f"r_{i}.png")
        frames.append({"file_path": f"./train/r_{i}", "transform_matrix": cams[i].tolist()})
    for split in ("train", "test"):
        json.dump({"camera_angle_x": 0.6911112070083618, "frames": frames}, open(root / f"transforms_{split}.json", "w"))


@pytest.mark.parametrize("method", ["kplanes", "hashgrid"])
def test_train_writes_normal_maps_and_an_oriented_point_cloud(tmp_path, method):
    from PIL import Image
    from tinynerf_amd import data, points as P
    from tinynerf_amd.run import TrainConfig, train
    _scene_on_disk(tmp_path)
    dev = torch.device(DEV)
    train_rays = data.RaysDataset(data.parse_nerf_synthetic(tmp_path, "train"), dev)
    test_set = data.PoseDataset(data.parse_nerf_synthetic(tmp_path, "test"), dev)
    out = tmp_path / "out"
    out.mkdir()
    cfg = TrainConfig(method=method, batch_size=256, n_samples=48, occupancy_res=16, kplanes_resolutions=(8, 16, 32), hashgrid_log2_table_size=12, seed=3)
    tr, _, _, _ = train(cfg, train_rays, None, test_set, out, max_steps=20, log_every=50, render_maps=True, normals=True, pointcloud=500)
    for i in range(2):
        png = np.asarray(Image.open(out / f"test_full_normal_{i:04d}.png"))
        assert png.shape == (16, 16, 3) and png.dtype == np.uint8
        maps = np.load(out / f"test_full_maps_{i:04d}.npz")
        nrm = maps["normal"]
        assert nrm.shape == (16, 16, 3) and nrm.dtype == np.float32
        assert np.array_equal(png, np.round(255.0 * (nrm.astype(np.float64) + 1) / 2).astype(np.uint8))
        length = np.sqrt((nrm.astype(np.float64) ** 2).sum(-1))
        assert (((nrm == 0).all(-1)) | (np.abs(length - 1) <= 4 * U)).all()
        assert ((nrm == 0).all(-1) | (maps["opacity"] > 0)).all()
    p, c, nn = P.read_ply(out / "pointcloud.ply", normals=True)
    with pytest.raises(ValueError):
        P.read_ply(out / "pointcloud.ply")
    assert 0 <= p.shape[0] <= 500 and nn.shape == p.shape and c.shape == p.shape
    length = np.sqrt((nn.astype(np.float64) ** 2).sum(-1))
    assert (((nn == 0).all(-1)) | (np.abs(length - 1) <= 4 * U)).all()
    sp, sc, sn = P.export_oriented_pointcloud(tr, test_set, path=out / "standalone.ply", n_points=500, seed=3)
    assert open(out / "standalone.ply", "rb").read() == open(out / "pointcloud.ply", "rb").read()
    assert np.array_equal(sn.cpu().numpy().view(np.uint32), nn.view(np.uint32)) and np.array_equal(sp.cpu().numpy().view(np.uint32), p.view(np.uint32))
    p2, c2 = P.export_pointcloud(tr, test_set, n_points=500, seed=3)
    assert torch.equal(p2, sp) and torch.equal(c2, sc)                              # the same points and colours without the normals
