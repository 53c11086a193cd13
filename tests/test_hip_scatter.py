"""GPU: the run-merged K-Planes and Cobafa scatters against fp64, per texel, in sample orders that drive every merging branch.

Orders, fixtures and references: _scatter_orders.py (test_scatter_orders.py shows on the CPU which branches each stream hits).
Reference: torch grid_sample (align_corners=True, zeros padding) in fp64 on the CPU, with autograd; the same evaluation on |inputs|
gives A, the sum of |terms| per element, and a bincount of tap indices gives m, the number of terms summed there.

* exact fixtures (dyadic coordinates, values in {-1, 0, 1}, integer upstream gradients; no product or partial sum can round):
  features and gradients equal the fp64 reference bit for bit -- a lost, doubled or misrouted term fails however small it is;
* general fixtures: |got - ref| <= (m + r) 2^-24 A per element, and nothing arrives where A == 0.  r counts the fp32 roundings one
  term carries before it is summed (coordinates are exact, _scatter_orders.snap):
    K-Planes, gradient of plane p: the tap weight gx * gy (1), each other plane's interpolated value (weight 1 + product 1 + three
    fma 3 = 5, twice) and the two products g * val * val (2): 13; the run sums (fma, then one atomic per run) add at most m + 1
    roundings on any term's way: r = 14.  Features: three interpolated values (15) and two products: r = 17.
    Cobafa, basis gradient: weight (2) * coefficient value (8 taps: weight 2, product 1, a three-level tree 3) and two products:
    10 + m + 1.  Coefficient gradient: the 64-lane reduction of g * basis * w (2 + 1 + 1 + 6 = 10), times the coefficient weight
    (2 + 1) and the sums: 13 + m + 1.  r = 14 for both; features: 6 + 6 + 1 = 13.

A. stand-alone tn_kplanes_fwd / tn_kplanes_bwd (CS = 4) through models._KPlanesFeatures, every case x order family x fixture kind,
   the single-plane form (KPlanesFeaturePlane) included, and the sizes around tile and persistent-loop boundaries;
B. the plane scatter inside tn_kplanes_mlp_bwd_pair (CS = 8) through NerfRenderer, both head forms: the launch's own d loss / d feat
   (written on request to grad_feat) scattered in fp64 and by tn_kplanes_bwd; both HIP results within the bound of the fp64 one;
C. tn_cobafa_fwd / tn_cobafa_bwd through CobafaFeatureField.features: 6 levels (the NL = 6 kernel) and 1, 3, 8 (the generic one).
"""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import _scatter_orders as so

pytestmark = pytest.mark.gpu
DEV = "cuda"
FAMS = list(so.FAMILIES)
KP_BWD, KP_FWD, CB_BWD, CB_FWD = 14, 17, 14, 13


def _plane_param(hwc: np.ndarray) -> torch.nn.Parameter:
    """[H, W, C] -> the [1, C, H, W] channels_last parameter the models hold"""
    t = torch.as_tensor(hwc).permute(2, 0, 1)[None].to(DEV).contiguous(memory_format=torch.channels_last)
    return torch.nn.Parameter(t)


def _hwc(t: torch.Tensor) -> np.ndarray:
    return t.detach()[0].permute(1, 2, 0).cpu().numpy()


def _check_kplanes(x, planes, g, exact, shapes, feat, grads, name):
    ref, aref, rg, arg = so.kplanes_ref(x, planes, g)
    if exact:
        fb, tb = so.kp_exact_bits(x, shapes, planes, g)
        so.assert_exact(ref, aref, fb, name)
        assert np.array_equal(feat, ref.astype(np.float32)), f"{name}: features not bit-exact"
    else:
        so.assert_within(feat, ref, aref, 0, KP_FWD, f"{name} features")
    for i, got in enumerate(grads):
        if got is None:
            assert planes[i] is None
            continue
        s = i // 3
        H, W = shapes[s]
        if exact:
            so.assert_exact(rg[i], arg[i], tb, name)
            bad = got != rg[i].astype(np.float32)
            assert not bad.any(), f"{name} plane {i}: {int(bad.sum())} texel channels differ from the exact sum"
        else:
            m = so.tap_counts(x, H, W, i % 3)[:, :, None]
            so.assert_within(got, rg[i], arg[i], m, KP_BWD, f"{name} plane {i}")


def _run_standalone(x, planes, g, single):
    from tinynerf_amd import models
    xt = torch.as_tensor(x).to(DEV)
    gt = torch.as_tensor(g).to(DEV)
    if single:
        mod = models.KPlanesFeaturePlane(planes[0].shape[2], planes[0].shape[:2]).to(DEV)
        with torch.no_grad():
            mod.plane.copy_(_plane_param(planes[0]))
        out = mod(xt[:, :2])
        out.backward(gt)
        return out.detach().cpu().numpy(), [_hwc(mod.plane.grad), None, None]
    params = [None if p is None else _plane_param(p) for p in planes]
    out = models._KPlanesFeatures.apply(xt, *params)
    live = [p for p in params if p is not None]
    gr = iter(torch.autograd.grad(out, live, gt))
    return out.detach().cpu().numpy(), [None if p is None else _hwc(next(gr)) for p in params]


# ------------------------------------------------------------------------------------------------ A. stand-alone K-Planes
@pytest.mark.parametrize("kind", ["exact", "general"])
@pytest.mark.parametrize("family", FAMS)
@pytest.mark.parametrize("name", list(so.KP_GENERAL))
def test_kplanes_standalone_vs_fp64(name, family, kind):
    cases = so.KP_EXACT if kind == "exact" else so.KP_GENERAL
    n = so.N_EXACT if kind == "exact" else so.N_GENERAL
    x, planes, g, exact = so.kp_fixture(cases, name, family, n, so.seed_of(name, family, kind))
    feat, grads = _run_standalone(x, planes, g, cases[name][2])
    _check_kplanes(x, planes, g, exact, cases[name][1], feat, grads, f"{name}/{family}/{kind}")


@pytest.mark.parametrize("n", so.SIZES)
def test_kplanes_standalone_sizes(n):
    """1, 31, 32, 33 samples, a ragged tail, and more than 2048 blocks x 4 waves x 32 samples (a second round of the persistent
    tile loop), exact and general"""
    for kind, cases in (("exact", so.KP_EXACT), ("general", so.KP_GENERAL)):
        for name in ("c16_s2_nonsquare", "c32_s3_square"):
            x, planes, g, exact = so.kp_fixture(cases, name, "mixed", n, so.seed_of(name, n, kind))
            feat, grads = _run_standalone(x, planes, g, False)
            _check_kplanes(x, planes, g, exact, cases[name][1], feat, grads, f"{name}/n={n}/{kind}")


# ------------------------------------------------------------------------------------------------ B. fused scatter
def _fused_renderer(shapes, seed):
    from tinynerf_amd import core, models as m
    torch.manual_seed(seed)
    field = m.KPlanesFeatureField(32, [shapes[0][0]] * 3)
    field.planes = torch.nn.ModuleList([torch.nn.ModuleList([m.KPlanesFeaturePlane(32, hw) for _ in range(3)]) for hw in shapes])
    r = core.NerfRenderer(field, m.VanillaOpacityDecoder(96), m.VanillaColorDecoder(8, 96, 64, 3), torch.ones(3)).to(DEV)
    with torch.no_grad():
        r.sigma_decoder.net.net[2].bias += 3.0
        for p in field.plane_tensors():
            p.uniform_(-1.0, 1.0)
    return r


def _rays(x, seed):
    """packed [n, 7] in the given sample order, cut into rays of 1 .. 256 samples"""
    n = len(x)
    rng = np.random.default_rng(seed)
    cnt = []
    while sum(cnt) < n:
        cnt.append(int(rng.integers(1, 257)))
    cnt[-1] -= sum(cnt) - n
    cnt = np.array(cnt, np.int32)
    info = np.stack([np.cumsum(cnt) - cnt, cnt], -1).astype(np.int32)
    d = rng.standard_normal((len(cnt), 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    packed = np.zeros((n, 7), np.float32)
    packed[:, :3] = x
    packed[:, 3:6] = np.repeat(d, cnt, 0)
    packed[:, 6] = 0.004
    return torch.as_tensor(packed).to(DEV), torch.as_tensor(info).to(DEV)


def _fused_case(shapes, family, n, seed, monkeypatch):
    from tinynerf_amd import _lib as L, fused, models
    monkeypatch.setattr(fused, "FUSE_SCATTER", True)
    r = _fused_renderer(shapes, seed)
    x = so.stream(family, n, shapes, seed)
    packed, info = _rays(x, seed)
    seen = {}
    real_call = L.call

    def call(name, dev, *args):          # hand the chain launch a grad_feat buffer: it writes the d loss / d feat it scatters
        if name == "tn_kplanes_mlp_bwd_pair" and args[4]._obj.flags & L.MLP_CHAIN_ONLY:
            assert args[15].value is None
            seen["g"] = torch.zeros(n, 96, device=DEV)
            args = list(args)
            args[15] = L.ptr(seen["g"])
        return real_call(name, dev, *args)
    monkeypatch.setattr(L, "call", call)
    out = r(packed, info)
    torch.manual_seed(seed + 1)
    out.backward(torch.randn_like(out))
    monkeypatch.setattr(L, "call", real_call)
    assert "g" in seen, "the fused chain + scatter launch did not run"
    gfeat = seen["g"]
    planes_t = r.feature_module.plane_tensors()
    fused_g = [_hwc(p.grad) for p in planes_t]
    # the same grad_feat through the stand-alone scatter
    params = [torch.nn.Parameter(p.detach().clone()) for p in planes_t]
    xt = packed[:, :3].contiguous()
    feat = models._KPlanesFeatures.apply(xt, *params)
    solo_g = [_hwc(t) for t in torch.autograd.grad(feat, params, gfeat)]
    g = gfeat.cpu().numpy()
    assert np.isfinite(g).all() and np.count_nonzero(g) > 0
    planes = [_hwc(p) for p in planes_t]
    _, _, rg, arg = so.kplanes_ref(x, planes, g)
    for i in range(len(planes)):
        H, W = shapes[i // 3]
        m = so.tap_counts(x, H, W, i % 3)[:, :, None]
        so.assert_within(fused_g[i], rg[i], arg[i], m, KP_BWD, f"fused {family} plane {i}")
        so.assert_within(solo_g[i], rg[i], arg[i], m, KP_BWD, f"tn_kplanes_bwd {family} plane {i}")


FUSED_SHAPES = {"small": [(17, 17), (33, 33), (65, 65)], "nonsquare": [(9, 33), (33, 9), (17, 65)]}


@pytest.mark.parametrize("family", ["rays26", "morton", "back_and_forth", "runs", "mixed"])
@pytest.mark.parametrize("shape", list(FUSED_SHAPES))
def test_fused_pair_scatter_vs_fp64(shape, family, heads, monkeypatch):
    _fused_case(FUSED_SHAPES[shape], family, (1 << 15) + 21, so.seed_of(shape, family), monkeypatch)


def test_fused_pair_scatter_reference_resolution(heads, monkeypatch):
    """128 / 256 / 512 planes, about 2^20 samples in real ray order"""
    t0 = time.time()
    _fused_case([(128, 128), (256, 256), (512, 512)], "rays26", (1 << 20) + 13, 5, monkeypatch)
    print(f"reference-resolution fused case: {time.time() - t0:.1f} s")


# ------------------------------------------------------------------------------------------------ C. Cobafa
@pytest.mark.parametrize("kind", ["exact", "general"])
@pytest.mark.parametrize("family", FAMS)
@pytest.mark.parametrize("name", list(so.CB_GENERAL))
def test_cobafa_vs_fp64(name, family, kind):
    from tinynerf_amd import models as m
    cases = so.CB_EXACT if kind == "exact" else so.CB_GENERAL
    cres, levels = cases[name]
    x, coef, basis, freqs, g, exact = so.cb_fixture(cases, name, family, so.N_COBAFA, so.seed_of(name, family, kind))
    field = m.CobafaFeatureField([r for r, _, _ in levels], cres, freqs, [c for _, _, c in levels], 32).to(DEV)
    grid = lambda a: torch.as_tensor(a).permute(3, 0, 1, 2)[None].to(DEV).contiguous(memory_format=torch.channels_last_3d)
    with torch.no_grad():
        field.coef_grid.grid.copy_(grid(coef))
        for b, a in zip(field.basis_grids, basis):
            b.grid.copy_(grid(a))
    feat = field.features(torch.as_tensor(x).to(DEV))
    feat.backward(torch.as_tensor(g).to(DEV))
    dhwc = lambda t: t.detach()[0].permute(1, 2, 3, 0).cpu().numpy()
    got = [dhwc(field.coef_grid.grid.grad)] + [dhwc(b.grid.grad) for b in field.basis_grids]
    feat = feat.detach().cpu().numpy()
    ref, aref, rg, arg = so.cobafa_ref(x, coef, basis, freqs, g)
    tag = f"{name}/{family}/{kind}"
    if exact:
        fb, tb = so.cb_exact_bits(x, cres, levels, g)
        so.assert_exact(ref, aref, fb, tag)
        assert np.array_equal(feat, ref.astype(np.float32)), f"{tag}: features not bit-exact"
        for i in range(len(got)):
            so.assert_exact(rg[i], arg[i], tb, tag)
            bad = got[i] != rg[i].astype(np.float32)
            assert not bad.any(), f"{tag} grid {i}: {int(bad.sum())} voxel channels differ from the exact sum"
        return
    so.assert_within(feat, ref, aref, 0, CB_FWD, f"{tag} features")
    pts = [np.asarray(x, np.float64)] + [so.sawtooth64(x, f) for f in freqs]
    for i, (r, p) in enumerate(zip([cres] + [r for r, _, _ in levels], pts)):
        m = so.grid_tap_counts(p, *r)[..., None]
        so.assert_within(got[i], rg[i], arg[i], m, CB_BWD, f"{tag} grid {i}")
