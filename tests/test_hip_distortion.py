"""GPU tests of the distortion loss: tn_distortion_fwd / tn_distortion_bwd against the fp64 pairwise definition
(tests/_distortion_ref.py), tn_render_rays_bwd_dw against the launches it fuses, NerfRenderer.render_with_distortion on both fused
nodes and on the module-by-module path against the CPU port, and TrainConfig.distortion_weight in the trainer."""
import ctypes as C

import numpy as np
import pytest
import torch

import _distortion_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _info(counts):
    cnt = torch.as_tensor(counts, dtype=torch.int32)
    return torch.stack([torch.cumsum(cnt, 0, dtype=torch.int32) - cnt, cnt], -1)


def _call(name, *args):
    from tinynerf_amd import _lib as L
    L.call(name, torch.device(DEV), *args)


def _ptr(t):
    from tinynerf_amd import _lib as L
    return L.ptr(t)


# ------------------------------------------------------------------------------------ 1. the two kernels against fp64
# a ray per boundary of the 64-sample chunks, of the register form (<= 512 samples) and of the streaming form behind it
COUNTS = [0, 1, 2, 63, 64, 65, 128, 129, 511, 512, 513, 1024, 2500, 0, 200, 200, 200, 37, 300]
STEP = 5.2 / 1024


def _rays(t0, seed):
    """weights from tn_weights_fwd on random sigmas: thin rays (every sample alive), dense rays (terminated early within the first
    samples) and empty space (sigma = 0: every weight 0); t = t0 + (k + jitter) * step"""
    g = torch.Generator().manual_seed(seed)
    info = _info(COUNTS)
    n = int(info[:, 1].sum())
    density = torch.tensor([0.5, 40.0, 2000.0, 0.0])[torch.arange(len(COUNTS)) % 4]          # per ray
    ray_of = torch.repeat_interleave(torch.arange(len(COUNTS)), info[:, 1].long())
    sigmas = (torch.rand(n, generator=g) * density[ray_of]).to(DEV)
    steps = (STEP * (0.75 + 0.5 * torch.rand(n, generator=g))).to(DEV)
    k = torch.arange(n) - info[ray_of, 0]
    t = (t0 + 0.01 * ray_of + (k + torch.rand(n, generator=g)) * STEP).float().to(DEV)
    weights = torch.zeros(n, device=DEV)
    info = info.to(DEV)
    _call("tn_weights_fwd", _ptr(sigmas), _ptr(steps), _ptr(info), C.c_float(1e-4), _ptr(weights), C.c_int64(n), C.c_int64(len(COUNTS)))
    return weights, t, steps, info


@pytest.mark.parametrize("t0", [2.0, 50.0])
@pytest.mark.parametrize("warp,near,rng", [(ref.LINEAR, 0.0, 5.2), (ref.UNBOUNDED, 0.1, 1.0), (ref.UNBOUNDED, 0.1, 4.0)])
def test_distortion_kernels_against_fp64(warp, near, rng, t0):
    """per ray |L - L64| <= 1e-5 L64 (floor 1e-12), per sample |g - g64| <= 1e-5 of the ray's largest |g64|; the yardstick is the fp64
    pairwise definition on the kernels' fp32 inputs.  t near 50 is the case fp32 prefixes of unshifted positions fail (4e-5 .. 3e-4)."""
    w, t, steps, info = _rays(t0, seed=int(t0) + warp)
    R, n = info.size(0), w.numel()
    wc = w.cpu().numpy()
    dead = [r for r, (a, c) in enumerate(info.cpu().numpy()) if c > 8 and not wc[a:a + c].any()]
    cut = [r for r, (a, c) in enumerate(info.cpu().numpy()) if c > 8 and wc[a] > 0 and wc[a + c - 1] == 0]
    assert dead and cut, "the fixture must hold all-zero rays and rays that terminated early"
    loss = torch.full((R,), -1.0, device=DEV)
    total = torch.zeros(1, dtype=torch.float64, device=DEV)
    args = (_ptr(w), _ptr(t), _ptr(steps), _ptr(info), C.c_int64(R), C.c_int32(warp), C.c_float(near), C.c_float(rng))
    _call("tn_distortion_fwd", *args, _ptr(loss), _ptr(total))
    grad = torch.full((n,), 7.0, device=DEV)
    _call("tn_distortion_bwd", *args, C.c_void_p(None), C.c_float(1.0), C.c_void_p(None), _ptr(grad))
    near32, rng32 = float(np.float32(near)), float(np.float32(rng))
    l64, g64 = ref.distortion(wc, t.cpu().numpy(), steps.cpu().numpy(), info.cpu().numpy(), warp, near32, rng32)
    got_l, got_g = loss.cpu().numpy().astype(np.float64), grad.cpu().numpy().astype(np.float64)
    worst_l = worst_g = 0.0
    for r, (a, c) in enumerate(info.cpu().numpy()):
        err = abs(got_l[r] - l64[r])
        worst_l = max(worst_l, err / max(l64[r], 1e-300) if l64[r] > 0 else 0.0)
        assert err <= max(1e-5 * l64[r], 1e-12), (r, c, got_l[r], l64[r])
        if c:
            gmax = np.abs(g64[a:a + c]).max()
            gerr = np.abs(got_g[a:a + c] - g64[a:a + c]).max()
            worst_g = max(worst_g, gerr / gmax if gmax > 0 else 0.0)
            assert gerr <= 1e-5 * gmax, (r, c, gerr, gmax)
    print(f"warp {warp} range {rng} t0 {t0}: worst loss error {worst_l:.2e} of the ray's loss, worst gradient error {worst_g:.2e} of the ray's largest")
    assert l64[dead].max() == 0.0 and min(l64[r] for r in cut) > 0.0
    # sum: the fp64 sum of the fp32 per-ray values, in some order
    want = float(got_l.sum())
    assert abs(float(total.item()) - want) <= 1e-12 * want
    # it accumulates, and NULL is allowed
    _call("tn_distortion_fwd", *args, _ptr(loss), _ptr(total))
    assert abs(float(total.item()) - 2 * want) <= 1e-12 * 2 * want
    # grad_loss, scale and scale_dev multiply through
    gl = (torch.rand(R, device=DEV) + 0.5)
    sd = torch.tensor([3.0], device=DEV)
    scaled = torch.empty(n, device=DEV)
    _call("tn_distortion_bwd", *args, _ptr(gl), C.c_float(0.5), _ptr(sd), _ptr(scaled))
    ray_of = torch.repeat_interleave(torch.arange(R, device=DEV), info[:, 1].long())
    want_g = (grad.double() * 1.5 * gl.double()[ray_of]).cpu().numpy()
    np.testing.assert_allclose(scaled.cpu().numpy(), want_g, rtol=1e-6, atol=0)


# ------------------------------------------------------------------------------------ 2. tn_render_rays_bwd_dw
@pytest.mark.parametrize("with_bg", [True, False])
def test_render_rays_bwd_dw_is_the_launches_it_fuses(with_bg):
    torch.manual_seed(3)
    counts = [0, 5, 64, 65, 700, 1, 1100, 130, 0, 33]
    info = _info(counts).to(DEV)
    R, n = len(counts), int(sum(counts))
    sig = torch.rand(n, device=DEV) * torch.tensor([1.0, 30.0, 400.0], device=DEV)[torch.arange(n, device=DEV) % 3]
    steps = torch.full((n,), 0.01, device=DEV) * (0.5 + torch.rand(n, device=DEV))
    rgbs = torch.rand(n, 3, device=DEV)
    bg = torch.rand(3, device=DEV) if with_bg else None
    go = torch.randn(R, 3, device=DEV)
    w, out = torch.zeros(n, device=DEV), torch.empty(R, 3, device=DEV)
    _call("tn_render_rays_fwd", _ptr(sig), _ptr(steps), _ptr(rgbs), _ptr(info), _ptr(bg), C.c_float(1e-4), _ptr(w), _ptr(out),
          C.c_void_p(None), C.c_int64(n), C.c_int64(R))
    assert int((w == 0).sum()) > 0 and int((w > 0).sum()) > 0
    sizes = (C.c_int64(n), C.c_int64(R))

    def plain():
        gr, gs = torch.empty(n, 3, device=DEV), torch.empty(n, device=DEV)
        _call("tn_render_rays_bwd", _ptr(sig), _ptr(steps), _ptr(rgbs), _ptr(info), _ptr(bg), _ptr(w), _ptr(go), _ptr(gr), _ptr(gs), *sizes)
        return gr, gs

    def dw(extra):
        gr, gs = torch.empty(n, 3, device=DEV), torch.empty(n, device=DEV)
        _call("tn_render_rays_bwd_dw", _ptr(sig), _ptr(steps), _ptr(rgbs), _ptr(info), _ptr(bg), _ptr(w), _ptr(go), _ptr(extra), _ptr(gr),
              _ptr(gs), *sizes)
        return gr, gs
    gr0, gs0 = plain()
    gr1, gs1 = dw(torch.zeros(n, device=DEV))
    assert torch.equal(gr0, gr1) and torch.equal(gs0, gs1)
    extra = torch.randn(n, device=DEV) * 0.3
    gr2, gs2 = dw(extra)
    gr3, gw = torch.empty(n, 3, device=DEV), torch.empty(n, device=DEV)
    _call("tn_composite_bwd", _ptr(rgbs), _ptr(w), _ptr(info), _ptr(bg), _ptr(go), _ptr(gr3), _ptr(gw), *sizes)
    gw = gw + extra
    gs3 = torch.empty(n, device=DEV)
    _call("tn_weights_bwd", _ptr(sig), _ptr(steps), _ptr(info), _ptr(w), _ptr(gw), _ptr(gs3), *sizes)
    assert torch.equal(gr2, gr3) and torch.equal(gs2, gs3)
    assert not torch.equal(gs2, gs0)


# ------------------------------------------------------------------------------------ 3. the renderer
def _renderer(kind):
    from tinynerf_amd import core, models as m
    torch.manual_seed(11)
    if kind == "kplanes":
        field = m.KPlanesFeatureField(32, (16, 40, 96))
    else:
        field = m.VanillaFeatureMLP(10, 256, 8)
    dim = field.feature_dim
    r = core.NerfRenderer(field, m.VanillaOpacityDecoder(dim), m.VanillaColorDecoder(8, dim, 64, 3), torch.tensor([1.0, 0.5, 0.25])).to(DEV)
    with torch.no_grad():
        r.sigma_decoder.net.net[2].bias += 3.0          # a medium dense enough that some rays terminate
    return r


def _render_batch(n_rays=48, per_ray=60):
    g = torch.Generator().manual_seed(5)
    cnt = torch.randint(0, per_ray, (n_rays,), dtype=torch.int32, generator=g)
    cnt[3] = 0
    info = _info(cnt)
    n = int(cnt.sum())
    ray_of = torch.repeat_interleave(torch.arange(n_rays), cnt.long())
    packed = torch.rand(n, 7, generator=g)
    packed[:, :3] = packed[:, :3] * 1.9 - 0.95
    packed[:, 3:6] = torch.nn.functional.normalize(torch.randn(n_rays, 3, generator=g), dim=-1)[ray_of]
    packed[:, 6] = 0.05
    k = torch.arange(n) - info[ray_of, 0]
    t = 2.0 + (k + torch.rand(n, generator=g)) * 0.05
    target = torch.rand(n_rays, 3, generator=g)
    return packed, info, t.float(), target


WARP = (ref.UNBOUNDED, 0.1, 2.0)
LAMBDA = 0.05


def _port_loss(sd, packed, info, bg, target, t, lam, vanilla_freqs):
    """oracle/torch_port.render (core.py:225-267 on the CPU) with the weights kept, plus lam * the mean over rays of the pairwise
    definition written in torch, fp64"""
    from oracle import torch_port as tp
    n, R = packed.size(0), info.size(0)
    feat = tp.features(sd, packed[:, :3], vanilla_freqs)
    sig = tp._TruncExp.apply(tp.mlp(sd, "sigma_decoder.net.net.", feat) - 1.).ravel()
    w = tp._Weights.apply(sig, packed[:, 6].contiguous(), info, 1e-4)
    mask = w > 0
    d = packed[:, 3:6][mask]
    inp = torch.cat([tp.posenc(d, sd["rgb_decoder.pe.freqs"]), d, feat[mask]], -1)
    rgbs = torch.zeros((n, 3)).index_put((torch.nonzero(mask).squeeze(1),), torch.sigmoid(tp.mlp(sd, "rgb_decoder.net.net.", inp))) * w[:, None]
    idx = torch.repeat_interleave(torch.arange(R), info[:, 1].long())
    out = torch.zeros((R, 3)).index_add(0, idx, rgbs) + bg * (1 - torch.zeros(R).index_add(0, idx, w)[:, None])
    loss = torch.nn.functional.mse_loss(out, target).double()
    if lam:
        m, dd = ref.warp_md(t.numpy(), packed[:, 6].numpy(), WARP[0], float(np.float32(WARP[1])), float(np.float32(WARP[2])))
        m, dd, w64 = torch.from_numpy(m), torch.from_numpy(dd), w.double()
        per_ray = []
        for a, c in info.tolist():
            wr, mr = w64[a:a + c], m[a:a + c]
            per_ray.append((wr[:, None] * wr[None, :] * (mr[:, None] - mr[None, :]).abs()).sum() + (wr * wr * dd[a:a + c]).sum() / 3.0)
        loss = loss + lam * torch.stack(per_ray).mean()
    return loss


def _hip_grads(r, fused_path, packed, info, t, target, lam):
    r.fused = fused_path
    r.zero_grad(set_to_none=True)
    rgb, dist = r.render_with_distortion(packed, info, t)
    (torch.nn.functional.mse_loss(rgb, target) + lam * dist.mean()).backward()
    return rgb.detach(), dist.detach(), {k: p.grad.detach().cpu().numpy().copy() for k, p in r.named_parameters()}


@pytest.mark.parametrize("kind", ["kplanes", "vanilla"])
def test_render_with_distortion(kind):
    """rgb is forward's, bit for bit; the distortion is tn_distortion_fwd on the weights the forward composited with; the gradients of
    mse + lambda mean(distortion) match the CPU port and the fused node matches the module path, at the 2e-5 of a tensor's largest
    element that tests/test_hip_renderer.py (test_fused_accumulates_into_existing_grads) uses for such gradients.  Where the SAME
    gradients with lambda = 0 are already further than half of that from the port (fp32 weights backward, fp16-split heads), the
    distortion run is allowed twice that distance: both numbers are printed per tensor."""
    from oracle import torch_port as tp
    r = _renderer(kind)
    r.distortion_warp = WARP
    packed, info, t, target = (x.to(DEV) for x in _render_batch())
    vf = 10 if kind == "vanilla" else 0
    res = {}

    def check_forward():
        """in the current grad mode (the training and the inference forward are different launches)"""
        plain = r(packed, info).detach()
        handout = {}
        r.__dict__.setdefault("_stats", {})["maps_handout"] = handout
        try:
            rgb, dist = r.render_with_distortion(packed, info, t)
        finally:
            r._stats.pop("maps_handout", None)
        assert torch.equal(plain, rgb.detach())
        w = handout["weights"].detach().contiguous()
        want = torch.empty(info.size(0), device=DEV)
        _call("tn_distortion_fwd", _ptr(w), _ptr(t), _ptr(packed[:, 6].contiguous()), _ptr(info), C.c_int64(info.size(0)), C.c_int32(WARP[0]),
              C.c_float(WARP[1]), C.c_float(WARP[2]), _ptr(want), C.c_void_p(None))
        assert torch.equal(dist.detach(), want)
        assert float(dist.detach().max()) > 0 and float(dist.detach()[3]) == 0.0
        assert dist.requires_grad == torch.is_grad_enabled()
        return plain, want
    for fused_path in (True, False):
        r.fused = fused_path
        with torch.no_grad():
            check_forward()
        plain, want = check_forward()
        for lam in (0.0, LAMBDA):
            rgb, dist, grads = _hip_grads(r, fused_path, packed, info, t, target, lam)
            assert torch.equal(rgb, plain) and torch.equal(dist, want)
            res[fused_path, lam] = grads
    sd = {k: v.detach().cpu().contiguous() for k, v in r.state_dict().items()}
    cpu = [x.cpu() for x in (packed, info, t, target)]
    port = {lam: tp.grads_of(sd, lambda p: _port_loss(p, cpu[0], cpu[1], r.bg_color.cpu(), cpu[3], cpu[2], lam, vf))[0] for lam in (0.0, LAMBDA)}
    TOL = 2e-5

    def rel(a, b):
        return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max() / max(float(np.abs(b).max()), 1e-30))
    moved = 0.0
    for name in res[True, LAMBDA]:
        for fused_path in (True, False):
            e0 = rel(res[fused_path, 0.0][name], port[0.0][name])
            e1 = rel(res[fused_path, LAMBDA][name], port[LAMBDA][name])
            print(f"{kind} {'fused' if fused_path else 'module'} {name}: lambda = 0 {e0:.2e}, lambda = {LAMBDA} {e1:.2e} of the largest element")
            assert e1 <= max(TOL, 2.0 * e0), (name, fused_path, e0, e1)
        f0, f1 = rel(res[True, 0.0][name], res[False, 0.0][name]), rel(res[True, LAMBDA][name], res[False, LAMBDA][name])
        print(f"{kind} fused against module {name}: lambda = 0 {f0:.2e}, lambda = {LAMBDA} {f1:.2e}")
        assert f1 <= max(TOL, 2.0 * f0), (name, f0, f1)
        moved = max(moved, rel(port[LAMBDA][name], port[0.0][name]))
    assert moved > 1e-3, "the distortion term must move the gradients far more than the tolerances"


@pytest.mark.parametrize("fused_path", [True, False])
def test_an_all_masked_batch_has_no_distortion_and_no_gradient(fused_path, capsys):
    """ "Empty iteration" (core.py:251-254): a threshold above 1 ends every ray before its first sample"""
    r = _renderer("kplanes")
    r.fused = fused_path
    r.distortion_warp = WARP
    packed, info, t, target = (x.to(DEV) for x in _render_batch())
    rgb, dist = r.render_with_distortion(packed, info, t, early_termination_threshold=2.0)
    assert not dist.any()
    assert torch.equal(rgb, r.bg_color.expand_as(rgb))
    (torch.nn.functional.mse_loss(rgb, target) + dist.mean()).backward()
    for name, p in r.named_parameters():
        assert p.grad is None or not p.grad.any(), name


# ------------------------------------------------------------------------------------ 4. the trainer
def _scene():
    from tinynerf_amd import rays
    o, d, rgb, K, cams = rays.synthetic_scene(n_views=2, res=64, seed=3, device="cpu")
    return o.contiguous().to(DEV), d.contiguous().to(DEV), rgb.contiguous().to(DEV)


def _trainer(**kw):
    from tinynerf_amd.run import TrainConfig, Trainer
    o, d, rgb = _scene()
    cfg = TrainConfig(method="kplanes", scene_type="aabb", batch_size=256, n_samples=32, seed=2, occupancy_res=32, deterministic=True,
                      kplanes_resolutions=(16, 32, 64), **kw)
    return Trainer(cfg, o, d, rgb, torch.ones(3, device=DEV), torch.device(DEV))


def test_distortion_weight_zero_is_the_plain_step(monkeypatch):
    """no t buffer (the pack's t_values argument is NULL), the launches of a trainer that never heard of the option with the same sizes and scalars, and the same parameters
    after a step -- as far as a TrainConfig() trainer reproduces ITSELF: the plane scatter and the weight-gradient tiles add with fp32
    atomics in whatever order the waves arrive, so two identical trainers already differ after one step (measured on an MI355X:
    3.7e-9 = 2^-28 = 4 ulp of the learning rate on most tensors, 0 or 9e-10 on the two one-element biases, from run to run).  What
    the formats allow: Adam's first update is lr * m / (sqrt(v) + eps) with m / sqrt(v) = +-1 up to the ~8 roundings of the moment
    arithmetic, i.e. 8 ulp(lr) between two runs, and p - update rounds to an ulp of p.  Elements beyond that are gradients at the
    noise level whose SIGN differs (+- lr): at most 1e-5 of a tensor's elements, none seen."""
    from tinynerf_amd import _lib as L
    from tinynerf_amd.run import TrainConfig
    assert TrainConfig().distortion_weight == 0.0
    calls, pack_t = [], []
    orig = L.call

    def record(name, *args):
        if name == "tn_sample_pack_t":
            pack_t.append(args[11].value)                    # t_values: behind dev, desc, o, d, R, maskbits, info, base, packed, ray_ids, steps
        calls.append((name,) + tuple(x.value for x in args if isinstance(x, (C.c_int, C.c_int32, C.c_int64, C.c_float))))
        return orig(name, *args)
    monkeypatch.setattr(L, "call", record)
    seqs, trainers, ts = [], [], []
    for kw in ({}, {}, {"distortion_weight": 0.0}, {"distortion_weight": 0.01}):
        tr = _trainer(**kw)
        del calls[:], pack_t[:]
        tr.step()
        seqs.append(list(calls))
        ts.append(list(pack_t))
        trainers.append(tr)
    a, a2, b, c = trainers
    assert seqs[0] == seqs[1] == seqs[2]                     # entry points, sizes and scalar arguments
    seqs = [[call[0] for call in seq] for seq in seqs[1:]]
    assert not any(n in seqs[1] for n in ("tn_distortion_fwd", "tn_distortion_bwd", "tn_render_rays_bwd_dw"))
    assert all(n in seqs[2] for n in ("tn_distortion_fwd", "tn_distortion_bwd", "tn_render_rays_bwd_dw"))
    assert len(seqs[2]) == len(seqs[1]) + 2 and "tn_render_rays_bwd" not in seqs[2]
    # every pack goes through the one entry point; only the trainer with the loss hands it a t buffer
    assert all("tn_sample_pack_t" in seq and "tn_sample_pack" not in seq for seq in seqs)
    assert set(ts[0]) == set(ts[1]) == set(ts[2]) == {None} and set(ts[3]) == {c._arena["t_values"].data_ptr()}
    assert "t_values" not in b._arena and b._batch_t is None and "t_values" in c._arena
    lr_ulp = float(np.spacing(np.float32(1e-2)))
    for (name, p), p2, q in zip(a.renderer.named_parameters(), a2.renderer.parameters(), b.renderer.parameters()):
        own, got = float((p - p2).abs().max()), float((p - q).abs().max())
        print(f"{name}: two TrainConfig() trainers differ by {own:.2e}, distortion_weight = 0 from the first by {got:.2e} (largest |p| {float(p.abs().max()):.2e})")
        bound = 8.0 * lr_ulp + torch.from_numpy(np.spacing(p.detach().abs().cpu().numpy())).to(DEV)
        beyond = int(((p - q).abs() > bound).sum())
        assert beyond <= 1e-5 * p.numel(), (name, beyond, own, got)
    np.testing.assert_allclose(b.loss_value(), a.loss_value(), rtol=1e-6)       # (fp64 atomics in the MSE sum, read as fp32)


def test_trainer_loss_includes_the_weighted_mean_distortion():
    lam = 0.02
    tr = _trainer(distortion_weight=lam)
    for step in range(3):
        packed, info, target, k = tr.build_batch()
        t = tr._batch_t
        assert t is not None and t.shape == (packed.size(0),) and "t_values" in tr._arena
        packed, info, target, t = packed.clone(), info.clone(), target.clone(), t.clone()
        tr.renderer.train()
        with torch.no_grad():
            rgb, dist = tr.renderer.render_with_distortion(packed, info, t)
            reg = tr.tv_reg_alpha * tr.renderer.feature_module.loss_tv()
            want = float(torch.mean((rgb - target) ** 2) + reg) + lam * float(dist.double().mean())
        assert float(dist.mean()) > 0
        tr.renderer._batch_aux = None          # (the explicit batch is a copy: nothing the sampler wrote out covers it)
        tr.step_on_batch(packed, info, target, k, t=t)
        got = tr.loss_value()
        print(f"step {step}: loss {got:.6f} = mse + tv + {lam} * mean distortion {float(dist.mean()):.3e}")
        np.testing.assert_allclose(got, want, rtol=1e-5)        # (the tolerance of tests/test_hip_training.py's first-step losses)
    with pytest.raises(ValueError, match="needs t"):
        tr.step_on_batch(packed, info, target, k)


def test_training_with_the_loss_lowers_the_held_out_distortion():
    from tinynerf_amd import core
    o, d, rgb = _scene()
    held = torch.arange(0, o.size(0), 7, device=DEV)
    means = {}
    for lam in (0.0, 0.05):
        tr = _trainer(distortion_weight=lam)
        for _ in range(40):
            tr.step()
        tr.renderer.eval()
        with torch.no_grad():
            samples, info, t = tr.ray_provider(o[held], d[held], training=False, return_t=True)
            assert tr.renderer.distortion_warp == core.distortion_warp(tr.ray_provider.ray_marcher)
            _, dist = tr.renderer.render_with_distortion(samples, info, t)
        means[lam] = float(dist.double().mean())
    print(f"mean distortion of {held.numel()} held-out rays after 40 steps: {means[0.0]:.4e} without the loss, {means[0.05]:.4e} with it")
    assert means[0.05] < means[0.0], means


def test_more_than_one_rank_is_refused_for_now():
    from tinynerf_amd.run import TrainConfig, Trainer
    o, d, rgb = _scene()
    cfg = TrainConfig(method="kplanes", batch_size=256, n_samples=32, occupancy_res=32, kplanes_resolutions=(16, 32, 64), distortion_weight=0.01)
    with pytest.raises(ValueError, match="single-GPU"):
        Trainer(cfg, o, d, rgb, torch.ones(3, device=DEV), torch.device(DEV), rank=0, world_size=2)
