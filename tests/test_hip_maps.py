"""GPU tests of the depth / opacity maps (tn_sample_pack_t, tn_ray_maps, NerfRenderer.render_maps, Trainer.render_rays(maps=True),
infer(maps=True), train(render_maps=True)).

Definitions (include/tinynerf_hip.h): for ray r with samples k and weights w_k at distances t_k,
opacity = sum w_k; depth = sum w_k t_k / opacity (0 when opacity == 0); median_depth = t_j of the first j whose inclusive
prefix of w reaches opacity / 2 (0 when opacity == 0)."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5


def cu(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


def maps_fp64(w, t, info):
    """the definitions in fp64; also the inclusive prefixes and the half marks (for the median's tie band)"""
    w, t = np.asarray(w, np.float64), np.asarray(t, np.float64)
    R = info.shape[0]
    op, dp, idx, pref = np.zeros(R), np.zeros(R), np.full(R, -1), []
    for r, (s, c) in enumerate(info):
        ww, tt = w[s:s + c], t[s:s + c]
        p = np.cumsum(ww)
        pref.append(p)
        op[r] = ww.sum()
        if op[r] > 0:
            dp[r] = (ww * tt).sum() / op[r]
            idx[r] = int(np.argmax(p >= 0.5 * op[r]))
    return op, dp, idx, pref


def accepted_median_indices(p, half, eps):
    """the fp64 index, and its neighbours where the fp64 prefix lies within eps of the half-opacity mark"""
    j = int(np.argmax(p >= half))
    ok = {j}
    if abs(p[j] - half) <= eps and j + 1 < len(p):
        ok.add(j + 1)
    if j > 0 and abs(p[j - 1] - half) <= eps:
        ok.add(j - 1)
    return ok


# ------------------------------------------------------------------------------------------------ 1. t of the packed samples
def _pack_both(prov, o, d, jitter):
    """mask + scan as RayProvider does, then tn_sample_pack and tn_sample_pack_t with every output"""
    from tinynerf_amd import _lib as L
    dev = o.device
    R, S = o.size(0), prov.ray_marcher.n_samples
    desc = prov._desc(dev, False, jitter)
    n_chunks = (S + 63) // 64
    maskbits = torch.empty((R, n_chunks), dtype=torch.int64, device=dev)
    counts = torch.empty(R, dtype=torch.int32, device=dev)
    info = torch.empty((R, 2), dtype=torch.int32, device=dev)
    total = torch.zeros(1, dtype=torch.int32, device=dev)
    L.call("tn_sample_mask", dev, C.byref(desc), L.ptr(o), L.ptr(d), C.c_int64(R), L.ptr(maskbits), L.ptr(counts))
    L.call("tn_sample_scan", dev, L.ptr(counts), C.c_int64(R), C.c_void_p(None), L.ptr(info), L.ptr(total))
    n = int(total.item())
    outs = []
    for with_t in (False, True):
        packed = torch.full((n, 7), float("nan"), device=dev)
        ray_ids = torch.full((n,), -1, dtype=torch.int32, device=dev)
        steps = torch.full((n,), float("nan"), device=dev)
        t = torch.full((n,), float("nan"), device=dev)
        if with_t:
            L.call("tn_sample_pack_t", dev, C.byref(desc), L.ptr(o), L.ptr(d), C.c_int64(R), L.ptr(maskbits), L.ptr(info),
                   C.c_void_p(None), L.ptr(packed), L.ptr(ray_ids), L.ptr(steps), L.ptr(t), C.c_int64(n))
        else:
            L.call("tn_sample_pack", dev, C.byref(desc), L.ptr(o), L.ptr(d), C.c_int64(R), L.ptr(maskbits), L.ptr(info),
                   C.c_void_p(None), L.ptr(packed), L.ptr(ray_ids), L.ptr(steps), C.c_int64(n))
        outs.append((packed, ray_ids, steps, t))
    return info, maskbits, outs


def _bits(x):
    return x.detach().cpu().numpy().view(np.int32)


@pytest.mark.parametrize("jittered", [False, True])
@pytest.mark.parametrize("S", [8, 200, 1000])
@pytest.mark.parametrize("contraction", ["aabb", "mip360_inf", "mip360_l2"])
@pytest.mark.parametrize("marcher", ["aabb", "unbounded"])
def test_sample_pack_t_is_the_marched_t(marcher, contraction, S, jittered):
    from tinynerf_amd import core
    g = torch.Generator().manual_seed(S + 7 * len(contraction) + (3 if jittered else 0))
    R = 300
    aabb = torch.tensor([[-1.5] * 3, [1.5] * 3], device=DEV)
    grid = core.OccupancyGrid(24, 1 / 256.).to(DEV)
    grid.grid.copy_((torch.rand(24, 24, 24, generator=g) > 0.4).float())
    o = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1) * 3.5
    d = torch.nn.functional.normalize(-o + 0.6 * torch.randn(R, 3, generator=g), dim=-1)
    o, d = o.to(DEV).contiguous(), d.to(DEV).contiguous()
    m = core.RayMarcherAABB(aabb, S, 0.1) if marcher == "aabb" else core.RayMarcherUnbounded(S, 0.05, 1e5, 2.0)
    c = {"aabb": core.ContractionAABB(aabb), "mip360_inf": core.ContractionMip360(float("inf")),
         "mip360_l2": core.ContractionMip360(2)}[contraction]
    prov = core.RayProvider(grid, c, m)
    jitter = torch.rand(R, S, generator=g).to(DEV) if jittered else None
    info, maskbits, ((p0, r0, s0, _), (p1, r1, s1, t1)) = _pack_both(prov, o, d, jitter)
    n = p0.size(0)
    assert n > 0
    assert np.array_equal(_bits(p0), _bits(p1)) and torch.equal(r0, r1) and np.array_equal(_bits(s0), _bits(s1))
    # t of every kept candidate: tn_march_rays' t (+ jitter * delta, one fp32 rounding each, as core.py:173)
    tm, dl = m(o, d)
    tm, dl = tm.cpu().numpy().astype(np.float32), dl.cpu().numpy().astype(np.float32)
    if jittered:
        tm = tm + (jitter.cpu().numpy() * dl).astype(np.float32)
    bits = maskbits.cpu().numpy().view(np.uint64)
    k = np.arange(S)
    keep = ((bits[:, k // 64] >> (k % 64).astype(np.uint64)) & np.uint64(1)).astype(bool)
    assert keep.sum() == n
    assert np.array_equal(t1.cpu().numpy().view(np.int32), tm[keep].view(np.int32))
    # ... and through RayProvider: the tuple is (packed, info, ray_ids, t), the rest unchanged
    a = prov(o, d, training=False, jitter=jitter, return_ray_ids=True)
    b = prov(o, d, training=False, jitter=jitter, return_ray_ids=True, return_t=True)
    assert len(b) == 4 and all(torch.equal(x, y) for x, y in zip(a, b[:3]))
    assert np.array_equal(_bits(b[3]), _bits(t1))
    assert len(prov(o, d, training=False, jitter=jitter, return_t=True)) == 3


# ------------------------------------------------------------------------------------------------ 2. tn_ray_maps against fp64
def _random_rays(counts, seed):
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, np.int32)
    info = np.stack([np.cumsum(counts) - counts, counts], -1).astype(np.int32)
    n = int(counts.sum())
    w = (rng.random(n) * (rng.random(n) > 0.25)).astype(np.float32)
    w[info[-1, 0]:info[-1, 0] + info[-1, 1]] = 0.0          # last ray: samples, every weight 0
    t = np.zeros(n, np.float32)
    for s, c in info:
        t[s:s + c] = 0.1 + np.cumsum(rng.random(c) * 0.05)
    return w, t, info


def _ray_maps(w, t, info, which=(True, True, True)):
    from tinynerf_amd import _lib as L
    R = info.size(0)
    outs = [torch.full((R,), float("nan"), device=DEV) if on else None for on in which]
    L.call("tn_ray_maps", torch.device(DEV), L.ptr(w), L.ptr(t), L.ptr(info), C.c_int64(R), *[L.ptr(x) for x in outs])
    return outs


def test_ray_maps_vs_fp64():
    from tinynerf_amd import _lib as L
    counts = [0, 1, 63, 64, 65, 1000, 4096, 0, 7, 130, 3, 5]
    w, t, info = _random_rays(counts, 1)
    wg, tg, ig = cu(w), cu(t), cu(info, torch.int32)
    op, dp, md = _ray_maps(wg, tg, ig)
    # opacity: the bits of tn_composite_fwd's opacity output
    R = ig.size(0)
    rgbs = torch.rand(w.size, 3, device=DEV)
    rendered, op_c = torch.empty(R, 3, device=DEV), torch.empty(R, device=DEV)
    L.call("tn_composite_fwd", torch.device(DEV), L.ptr(rgbs), L.ptr(wg), L.ptr(ig), C.c_void_p(None), L.ptr(rendered), L.ptr(op_c),
           C.c_int64(w.size), C.c_int64(R))
    assert np.array_equal(_bits(op), _bits(op_c))
    o64, d64, idx, pref = maps_fp64(w, t, info)
    op, dp, md = op.cpu().numpy(), dp.cpu().numpy(), md.cpu().numpy()
    np.testing.assert_allclose(op, o64, rtol=TOL, atol=0)
    np.testing.assert_allclose(dp, d64, rtol=TOL, atol=0)
    for r, (s, c) in enumerate(info):
        if o64[r] == 0:
            assert op[r] == 0 and dp[r] == 0 and md[r] == 0, r
            continue
        ok = accepted_median_indices(pref[r], 0.5 * o64[r], 1e-6 * o64[r])
        assert md[r] in {float(t[s + j]) for j in ok}, (r, md[r], [t[s + j] for j in ok])
    # every NULL combination gives the same values in the outputs it was asked for
    full = (op, dp, md)
    for mask in range(8):
        which = tuple(bool(mask >> i & 1) for i in range(3))
        got = _ray_maps(wg, tg, ig, which)
        for on, x, ref in zip(which, got, full):
            if on:
                assert np.array_equal(x.cpu().numpy().view(np.int32), ref.view(np.int32)), which


def test_ray_maps_median_on_terminated_rays():
    """rays whose mass sits in one chunk out of many (the second pass stops there), and a ray whose half mark falls exactly
    on a sample"""
    counts = [4096, 300, 4]
    info = np.stack([np.cumsum(counts) - counts, counts], -1).astype(np.int32)
    n = sum(counts)
    w, t = np.zeros(n, np.float32), np.arange(n, dtype=np.float32) * 0.01
    w[info[0, 0] + 2000] = 0.9                                 # one live sample deep in the ray
    w[info[1, 0] + 70:info[1, 0] + 75] = 0.1                   # five in the second chunk
    w[info[2, 0]:info[2, 0] + 4] = [0.25, 0.25, 0.25, 0.25]    # the prefix reaches exactly 0.5 at sample 1
    op, dp, md = (x.cpu().numpy() for x in _ray_maps(cu(w), cu(t), cu(info, torch.int32)))
    assert md[0] == t[info[0, 0] + 2000] and md[1] == t[info[1, 0] + 72] and md[2] == t[info[2, 0] + 1]
    assert op[0] == np.float32(0.9) and abs(dp[0] - t[info[0, 0] + 2000]) <= 1e-6 * t[info[0, 0] + 2000]


# ------------------------------------------------------------------------------------------------ 3. geometry
SLAB = (20, 23)             # occupied grid cells along z of a 33^3 grid over [-1, 1]^3 (cell spacing 1/16)


def _slab_scene(S=256, fused=True):
    """sigma constant and large (the sigma head's last layer: zero weights, bias 10 -> sigma = e^9 ~ 8100), the occupancy grid
    set only in a slab of cells; with threshold 0.5 the sampler keeps the points whose interpolated value exceeds 0.5, i.e.
    z in (z(a - 1/2), z(b + 1/2)) = (0.21875, 0.46875)"""
    from tinynerf_amd import core, models as m
    torch.manual_seed(0)
    aabb = torch.tensor([[-1.0] * 3, [1.0] * 3], device=DEV)
    grid = core.OccupancyGrid(33, 1 / 256., threshold=0.5).to(DEV)
    grid.grid.zero_()
    grid.grid[SLAB[0]:SLAB[1] + 1] = 1.0                       # [D, H, W]: D indexes z
    prov = core.RayProvider(grid, core.ContractionAABB(aabb), core.RayMarcherAABB(aabb, S, 0.0))
    r = core.NerfRenderer(m.KPlanesFeatureField(32, (16, 32, 64)), m.VanillaOpacityDecoder(96), m.VanillaColorDecoder(8, 96, 64, 3),
                          torch.ones(3)).to(DEV)
    with torch.no_grad():
        r.sigma_decoder.net.net[2].weight.zero_()
        r.sigma_decoder.net.net[2].bias.fill_(10.0)
    r.fused = fused
    return prov, r, float(prov.ray_marcher.step_size)


@pytest.mark.parametrize("fused", [True, False])
def test_maps_of_a_slab(fused):
    prov, r, step = _slab_scene(fused=fused)
    z_in = -1.0 + (SLAB[0] - 0.5) / 16.0
    dirs = [(0.0, 0.0, 1.0), (0.3, 0.2, 1.0), (-0.25, 0.4, 1.0), (0.1, -0.1, 1.0)]
    o = torch.tensor([[0.0, 0.0, -3.0], [-0.5, -0.3, -3.0], [0.6, -0.7, -3.0], [0.05, 0.02, -2.5]])
    d = torch.nn.functional.normalize(torch.tensor(dirs), dim=-1)
    t_entry = ((z_in - o[:, 2]) / d[:, 2]).numpy()
    # rays that miss the slab: parallel to it inside the box, outside the box, away from it
    o_miss = torch.tensor([[-3.0, 0.0, -0.5], [0.0, 3.0, 0.9], [0.0, 0.0, -3.0]])
    d_miss = torch.tensor([[1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, -1.0]])
    oo, dd = torch.cat([o, o_miss]).to(DEV), torch.cat([d, d_miss]).to(DEV)
    packed, info, t = prov(oo, dd, training=False, return_t=True)
    with torch.no_grad():
        res = r.render_maps(packed, info, t)
    op, dp, md = (res[k].cpu().numpy() for k in ("opacity", "depth", "median_depth"))
    n_hit = len(dirs)
    assert np.all(info[:n_hit, 1].cpu().numpy() > 0)
    np.testing.assert_allclose(op[:n_hit], 1.0, atol=1e-6)
    assert np.all(np.abs(dp[:n_hit] - t_entry) <= step), (dp[:n_hit], t_entry, step)
    assert np.all(np.abs(md[:n_hit] - t_entry) <= step), (md[:n_hit], t_entry, step)
    assert np.all(md[:n_hit] >= t_entry - 1e-6)                # the first sample inside the slab, not before it
    assert np.all(op[n_hit:] == 0) and np.all(dp[n_hit:] == 0) and np.all(md[n_hit:] == 0)
    # an empty grid: no sample at all ("Empty iteration" of the module path) -> 0, 0, 0 and the background
    prov.occupancy_grid.grid.zero_()
    packed, info, t = prov(oo, dd, training=False, return_t=True)
    assert packed.size(0) == 0
    with torch.no_grad():
        res = r.render_maps(packed, info, t)
    assert all(bool((res[k] == 0).all()) for k in ("opacity", "depth", "median_depth"))
    assert torch.equal(res["rgb"], torch.ones_like(res["rgb"]))


# ------------------------------------------------------------------------------------------------ 4. renderer parity
def _t_of(packed, info):
    """any positive per-sample distances do for the maps: the running sum of the steps along each ray"""
    steps = packed[:, 6].cpu().numpy().astype(np.float64)
    t = np.zeros_like(steps)
    for s, c in info.cpu().numpy():
        t[s:s + c] = 0.5 + np.cumsum(steps[s:s + c])
    return cu(t.astype(np.float32))


def _check_parity(r, packed, info, t, module_weights):
    with torch.no_grad():
        ref = r(packed, info)
        res = r.render_maps(packed, info, t)
    assert torch.equal(res["rgb"], ref)
    o64, d64, _, _ = maps_fp64(module_weights.cpu().numpy(), t.cpu().numpy(), info.cpu().numpy())
    np.testing.assert_allclose(res["opacity"].cpu().numpy(), o64, rtol=0, atol=TOL)
    live = o64 > 1e-3
    scale = float(t.abs().max())
    np.testing.assert_allclose(res["depth"].cpu().numpy()[live], d64[live], rtol=0, atol=TOL * scale)
    op = res["opacity"].cpu().numpy()
    assert np.all(res["depth"].cpu().numpy()[op == 0] == 0) and np.all(res["median_depth"].cpu().numpy()[op == 0] == 0)
    return res


def _module_weights(r, packed, info):
    from tinynerf_amd import core
    with torch.no_grad():
        sig = r.sigma_decoder(r.feature_module(packed[:, :3])).ravel()
        return core.NerfWeights.apply(sig, packed[:, 6].contiguous(), info, 1e-4)


@pytest.mark.parametrize("form", ["module", "gated", "pair"])
def test_render_maps_kplanes_g9(form, monkeypatch):
    from tinynerf_amd import core, fused, models as m
    g = load_golden("G9_renderer_kplanes")
    sd = {k[3:]: torch.as_tensor(v) for k, v in g.items() if k.startswith("sd.")}
    field = m.KPlanesFeatureField(32)
    field.planes = torch.nn.ModuleList([torch.nn.ModuleList([
        m.KPlanesFeaturePlane(32, tuple(sd[f"feature_module.planes.{s}.0.plane"].shape[2:])) for _ in range(3)]) for s in range(3)])
    r = core.NerfRenderer(field, m.VanillaOpacityDecoder(96), m.VanillaColorDecoder(8, 96, 64, 3), cu(g["bg"]))
    r.load_state_dict(sd)
    r = r.to(DEV)
    r.fused = form != "module"
    packed, info = cu(g["packed"]), cu(g["info"], torch.int32)
    t = _t_of(packed, info)
    monkeypatch.setattr(fused, "INFER_PAIR", True)
    monkeypatch.setattr(fused, "_infer_prefers_pair", lambda stats: form == "pair")
    calls = []
    orig = fused.L.call
    monkeypatch.setattr(fused.L, "call", lambda name, *a: (calls.append(name), orig(name, *a))[1])
    _check_parity(r, packed, info, t, _module_weights(r, packed, info))
    if form == "pair":
        assert "tn_kplanes_mlp_fwd_pair" in calls and "tn_kplanes_mlp_fwd" not in calls, calls
    elif form == "gated":
        assert "tn_kplanes_mlp_fwd" in calls and "tn_kplanes_mlp_fwd_pair" not in calls, calls
    else:
        assert not any(c.startswith("tn_kplanes_mlp") for c in calls), calls


@pytest.mark.parametrize("fused", [True, False])
def test_render_maps_vanilla_g14(fused):
    from tinynerf_amd import core, models as m
    g = load_golden("G14_renderer_vanilla")
    r = core.NerfRenderer(m.VanillaFeatureMLP(10, 256, 8), m.VanillaOpacityDecoder(256), m.VanillaColorDecoder(8, 256, 64, 3), cu(g["bg"]))
    r.load_state_dict({k[3:]: torch.as_tensor(v) for k, v in g.items() if k.startswith("sd.")})
    r = r.to(DEV)
    r.fused = fused
    packed, info = cu(g["packed"]), cu(g["info"], torch.int32)
    _check_parity(r, packed, info, _t_of(packed, info), _module_weights(r, packed, info))


@pytest.mark.parametrize("fused", [True, False])
def test_render_maps_cobafa_g15(fused):
    """unbounded marcher + Mip-360 contraction + Cobafa: t straight from the sampler"""
    from tinynerf_amd import core, models as m
    g = load_golden("G15_config5_cobafa_unbounded")
    S = int(g["n_samples"])
    grid = core.OccupancyGrid(24, float(g["uniform_range"]) / S).to(DEV)
    grid.grid.copy_(cu(g["grid"]))
    grid.mean = float(grid.grid.mean().item())
    marcher = core.RayMarcherUnbounded(S, float(g["near"]), 1e5, float(g["uniform_range"]))
    prov = core.RayProvider(grid, core.ContractionMip360(float("inf")), marcher)
    packed, info, t = prov(cu(g["rays_o"]), cu(g["rays_d"]), training=False, return_t=True)
    freqs = [float(f) for f in g["freqs"]]
    cf = m.CobafaFeatureField(basis_res=[8, 10, 12], coef_res=8, freqs=freqs, channels=[8, 8, 4], mlp_hidden_dim=128)
    r = core.NerfRenderer(cf, m.VanillaOpacityDecoder(128), m.VanillaColorDecoder(8, 128, 64, 3), None)
    r.load_state_dict({k[3:]: torch.as_tensor(v) for k, v in g.items() if k.startswith("sd.")})
    r.to(DEV).eval()
    r.fused = fused
    assert float(t.min()) >= float(g["near"])
    res = _check_parity(r, packed, info, t, _module_weights(r, packed, info))
    assert float(res["opacity"].max()) > 0.1


# ------------------------------------------------------------------------------------------------ 5. trainer, infer, train
def _trainer():
    from tinynerf_amd import rays
    from tinynerf_amd.run import TrainConfig, Trainer
    o, d, rgb, K, cams = rays.synthetic_scene(n_views=2, res=64, seed=3, device="cpu")
    dev = torch.device(DEV)
    cfg = TrainConfig(method="kplanes", scene_type="aabb", batch_size=128, n_samples=64, seed=5, occupancy_res=32)
    tr = Trainer(cfg, o.contiguous().to(dev), d.contiguous().to(dev), rgb.contiguous().to(dev), torch.ones(3, device=dev), dev)
    for _ in range(3):
        tr.step()
    return tr, o, d


def test_render_rays_maps_chunking_and_rgb():
    tr, o, d = _trainer()
    oo, dd = o[:6000].to(DEV), d[:6000].to(DEV)
    a = tr.render_rays(oo, dd, batch_size=1000, maps=True)
    b = tr.render_rays(oo, dd, maps=True)
    rgb = tr.render_rays(oo, dd)
    assert set(a) == {"rgb", "opacity", "depth", "median_depth"}
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(a["rgb"], rgb)
    assert a["opacity"].shape == (6000,) and float(a["opacity"].max()) > 0.1          # (3 steps in: a faint field)
    assert float(a["opacity"].max()) <= 1.0 + 1e-6 and float(a["depth"].min()) >= 0.0


def test_infer_writes_maps(tmp_path):
    from PIL import Image
    from tinynerf_amd.run import infer
    tr, o, d = _trainer()
    H, W = 40, 50
    ds = [{"rays_o": o[i * H * W:(i + 1) * H * W].reshape(H, W, 3), "rays_d": d[i * H * W:(i + 1) * H * W].reshape(H, W, 3)} for i in range(2)]
    out = infer(tr, ds, [0, 1], tmp_path, "img", maps=True)
    assert len(out) == 2 and out[1]["rgb"].shape == (H, W, 3) and out[1]["depth"].shape == (H, W)
    assert torch.equal(out[0]["rgb"], infer(tr, ds, [0])[0])
    for i in (0, 1):
        for kind in ("depth", "opacity"):
            im = Image.open(tmp_path / f"img_{kind}_{i:04d}.png")
            assert im.size == (W, H) and im.mode.startswith("I;16"), (kind, im.mode)
        z = np.load(tmp_path / f"img_maps_{i:04d}.npz")
        for k in ("depth", "median_depth", "opacity"):
            assert z[k].shape == (H, W) and z[k].dtype == np.float32, k
        np.testing.assert_array_equal(z["depth"], out[i]["depth"].cpu().numpy())
        assert float(z["depth_scale"]) == pytest.approx(float(z["depth"].max()))
        png = np.asarray(Image.open(tmp_path / f"img_depth_{i:04d}.png"), dtype=np.float64) / 65535.0 * float(z["depth_scale"])
        np.testing.assert_allclose(png, z["depth"], atol=float(z["depth_scale"]) / 65535.0)


def test_train_render_maps_on_a_scene_on_disk(tmp_path):
    from PIL import Image
    from tinynerf_amd import data, rays
    from tinynerf_amd.run import TrainConfig, train
    o, d, rgb, K, cams = rays.synthetic_scene(n_views=3, res=48, seed=5, device="cpu")
    imgs = (rgb.reshape(3, 48, 48, 3) * 255).to(torch.uint8).numpy()
    (tmp_path / "train").mkdir()
    frames = []
    for i in range(3):
        Image.fromarray(imgs[i]).save(tmp_path / "train" / f"r_{i}.png")
        frames.append({"file_path": f"./train/r_{i}", "transform_matrix": cams[i].tolist()})
    for split in ("train", "test"):
        json.dump({"camera_angle_x": 0.6911112070083618, "frames": frames[:3 if split == "train" else 1]},
                  open(tmp_path / f"transforms_{split}.json", "w"))
    dev = torch.device(DEV)
    train_rays = data.RaysDataset(data.parse_nerf_synthetic(tmp_path, "train"), dev)
    test_set = data.PoseDataset(data.parse_nerf_synthetic(tmp_path, "test"), dev)
    out = tmp_path / "out"; out.mkdir()
    cfg = TrainConfig(method="kplanes", batch_size=512, n_samples=64, occupancy_res=32, kplanes_resolutions=(16, 32, 64), seed=3)
    train(cfg, train_rays, None, test_set, out, max_steps=20, log_every=50, render_maps=True)
    assert (out / "test_full_0000.png").exists() and (out / "metrics_test.json").exists()
    for f in ("test_full_depth_0000.png", "test_full_opacity_0000.png", "test_full_maps_0000.npz"):
        assert (out / f).exists(), f
    assert np.load(out / "test_full_maps_0000.npz")["opacity"].shape == (48, 48)
