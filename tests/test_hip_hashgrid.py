"""GPU tests of the multiresolution hash grid (tn_hashgrid_fwd / tn_hashgrid_bwd, models.HashGridFeatureField, the fused render node
in front of it) against the float64 yardstick tests/_hashgrid_ref.py.

Bounds.  Forward: the yardstick starts from the same fp32 (i, f) as the kernel, so what is left is 8 products of three fp32 weights
and their sum on entries of magnitude <= 1 -- a few 2^-24 -- held to the project's 1e-5.  Backward, per table entry e that receives
m_e terms: |got - ref| <= 2^-24 (m_e + 8) sum|terms|_e, the worst case of an fp32 sum of m_e terms in any order plus the terms' own
roundings (three products each); a dropped, doubled or misplaced contribution is off by a whole term.  Where the scatter adds to a
non-zero initial value, that value is one more term of the same sum (m_e + 1 terms, |initial| joins sum|terms|); entries that receive
nothing keep their initial bits."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _hashgrid_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5
U = 2.0 ** -24
CONFIGS = {"small2": (ref.SMALL, 2), "small4": (ref.SMALL, 4), "fine2": (ref.FINE, 2)}
SIZES = [1, 31, 33, 64, 4099]


def desc_for(plan, features, table):
    from tinynerf_amd import _lib as L
    res, hashed, entries, offsets = plan
    d = L.HashGridDesc()
    d.n_levels, d.features = len(res), features
    for l in range(len(res)):
        d.res[l], d.hashed[l], d.entries[l], d.offset[l] = res[l], int(hashed[l]), entries[l], offsets[l]
    d.table = table.data_ptr()
    return d


@functools.lru_cache(maxsize=None)
def case(name, n):
    """inputs and yardstick results of one (configuration, n), computed once and shared (read-only) by every test"""
    cfg, features = CONFIGS[name]
    plan = ref.levels(**cfg)
    rng = np.random.default_rng(1000 * n + len(name))
    x = ref.sample_points(n, plan, seed=n)
    table = rng.uniform(-1, 1, (ref.total_entries(plan), features)).astype(np.float32)
    g = rng.uniform(-1, 1, (n, len(plan[0]) * features)).astype(np.float32)
    feat = ref.forward(table, x, plan)
    grad, m, abs_sum = ref.backward(g, x, plan, features)
    out = dict(plan=plan, features=features, x=x, table=table, g=g, feat=feat, grad=grad, m=m, abs_sum=abs_sum)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def device_x(x, stride):
    """the points as columns 0..2 of rows of `stride` floats (7: the packed samples' layout; the other columns hold NaN)"""
    buf = torch.full((len(x), stride), float("nan"), device=DEV)
    buf[:, :3] = torch.from_numpy(np.array(x)).to(DEV)
    return buf


def abi_fwd(c, stride):
    from tinynerf_amd import _lib as L
    table = torch.from_numpy(np.array(c["table"])).to(DEV)
    xb = device_x(c["x"], stride)
    n = len(c["x"])
    feat = torch.full((n, c["feat"].shape[1]), float("nan"), device=DEV)
    L.call("tn_hashgrid_fwd", torch.device(DEV), C.byref(desc_for(c["plan"], c["features"], table)), L.ptr(xb), C.c_int64(stride), C.c_int64(n),
           L.ptr(feat))
    return feat


def abi_bwd(c, stride, init):
    from tinynerf_amd import _lib as L
    table = torch.from_numpy(np.array(c["table"])).to(DEV)
    xb = device_x(c["x"], stride)
    n = len(c["x"])
    grad = torch.from_numpy(init.copy()).to(DEV)
    g = torch.from_numpy(np.array(c["g"])).to(DEV)
    L.call("tn_hashgrid_bwd", torch.device(DEV), C.byref(desc_for(c["plan"], c["features"], table)), L.ptr(xb), C.c_int64(stride), C.c_int64(n),
           L.ptr(g), L.ptr(grad))
    return grad.cpu().numpy()


def check_scatter(c, got, init, what):
    got, init64 = got.astype(np.float64), init.astype(np.float64)
    m, touched = c["m"], c["m"] > 0
    assert np.array_equal(got[~touched], init64[~touched]), f"{what}: an entry that receives nothing changed"
    extra = (init != 0).astype(np.float64)                       # a non-zero initial value is one more term of the sum
    bound = U * (m[:, None] + extra + 8) * (c["abs_sum"] + np.abs(init64))
    err = np.abs(got - (init64 + c["grad"]))
    worst = float((err[touched] / np.maximum(bound[touched], 1e-300)).max())
    print(f"{what}: worst |got - ref| / bound = {worst:.3f}, largest m_e = {int(m.max())}")
    assert np.all(err[touched] <= bound[touched]), f"{what}: {int((err > bound).sum())} entries outside the fp32 summation bound"


def test_small_configuration_has_dense_and_hashed_levels():
    res, hashed, entries, _ = ref.levels(**ref.SMALL)
    assert hashed == [False, False, True, True] and [(r + 1) ** 3 for r in res[:2]] == [27, 216]


@pytest.mark.parametrize("stride", [3, 7])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_forward_matches_the_yardstick(name, n, stride):
    c = case(name, n)
    got = abi_fwd(c, stride).cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    err = float(np.abs(got - c["feat"]).max())
    print(f"forward {name} n={n} stride={stride}: max |got - ref| = {err:.3e}")
    assert err <= TOL


@pytest.mark.parametrize("stride", [3, 7])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_backward_matches_the_yardstick_per_entry(name, n, stride):
    c = case(name, n)
    E = c["table"].shape
    zeros = np.zeros(E, np.float32)
    check_scatter(c, abi_bwd(c, stride, zeros), zeros, f"backward {name} n={n} stride={stride} from zeros")
    init = np.random.default_rng(5).uniform(-2, 2, E).astype(np.float32)
    check_scatter(c, abi_bwd(c, stride, init), init, f"backward {name} n={n} stride={stride} onto an initial value")


def field_for(c):
    from tinynerf_amd.models import HashGridFeatureField
    cfg = [v for v, f in CONFIGS.values() if ref.levels(**v) == c["plan"]][0]
    fm = HashGridFeatureField(cfg["n_levels"], c["features"], cfg["log2_T"], cfg["n_min"], cfg["n_max"]).to(DEV)
    assert fm.table.shape == c["table"].shape
    with torch.no_grad():
        fm.table.copy_(torch.from_numpy(np.array(c["table"])))
    return fm


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_module_is_the_two_abi_calls(name):
    c = case(name, 4099)
    fm = field_for(c)
    assert fm.feature_dim == c["feat"].shape[1]
    for stride in (3, 7):
        xb = device_x(c["x"], stride)
        feat = fm(xb[:, :3])                                              # stride 7: the packed samples' view, read in place
        assert torch.equal(feat, abi_fwd(c, stride))
        fm.table.grad = None
        feat.backward(torch.from_numpy(np.array(c["g"])).to(DEV))
        zeros = np.zeros(c["table"].shape, np.float32)
        check_scatter(c, fm.table.grad.cpu().numpy(), zeros, f"module backward {name} stride={stride}")
    # leading dimensions
    x3 = torch.from_numpy(np.array(c["x"][:4096])).to(DEV).reshape(8, 512, 3)
    assert torch.equal(fm(x3).reshape(4096, -1), fm(x3.reshape(-1, 3)))


def test_accumulate_switch_adds_into_table_grad_in_place():
    c = case("small2", 4099)
    fm = field_for(c)
    init = np.random.default_rng(9).uniform(-2, 2, c["table"].shape).astype(np.float32)
    fm.table.grad = torch.from_numpy(init.copy()).to(DEV)
    ptr = fm.table.grad.data_ptr()
    fm.__dict__["accumulate_into_grad"] = True
    fm(torch.from_numpy(np.array(c["x"])).to(DEV)).backward(torch.from_numpy(np.array(c["g"])).to(DEV))
    assert fm.table.grad.data_ptr() == ptr
    check_scatter(c, fm.table.grad.cpu().numpy(), init, "accumulate switch")


def test_no_samples():
    c = case("small2", 64)
    fm = field_for(c)
    x = torch.zeros((0, 3), device=DEV)
    feat = fm(x)
    assert feat.shape == (0, fm.feature_dim)
    feat.sum().backward()
    assert fm.table.grad is not None and float(fm.table.grad.abs().max()) == 0.0


def _renderer_and_batch():
    import _g22
    from tinynerf_amd.run import TrainConfig, build_renderer
    o, d, _, bg = _g22.ray_table()
    cfg = TrainConfig(method="hashgrid", n_samples=64, occupancy_res=32, hashgrid_log2_table_size=14)
    torch.manual_seed(3)
    renderer, _, provider = build_renderer(cfg, torch.from_numpy(bg).to(DEV), torch.device(DEV))
    with torch.no_grad():
        renderer.feature_module.table.uniform_(-1, 1)                     # (the initialisation's 1e-4 would make every feature ~ 0)
    idx = np.arange(0, 80000, 263)[:300]
    packed, info = provider(torch.from_numpy(o[idx]).to(DEV), torch.from_numpy(d[idx]).to(DEV), training=False)
    return renderer, packed, info, bg


def test_renderer_takes_the_fused_node_and_equals_the_module_path():
    from tinynerf_amd import fused
    renderer, packed, info, _ = _renderer_and_batch()
    assert fused.supports(renderer) and packed.size(0) > 3000
    with torch.no_grad():
        a = renderer(packed, info)
        renderer.fused = False
        b = renderer(packed, info)
    assert a.shape == (300, 3) and torch.isfinite(a).all()
    err = float((a - b).abs().max())
    print(f"fused against module path on {packed.size(0)} samples: max difference {err:.3e}")
    assert err <= TOL and float(a.std()) > 1e-3


# ---------------------------------------------------------------------------------------------------------------------------------
# Backward of the render paths in front of a hash-grid field (fused._RenderHeads without a row-view link: 32-wide features, the colour
# head as TN_ENC_DIR_CAT with per-sample directions, the unpaired heads backward with TN_MLP_ACCUM_GRAD_X on the sigma head, a real
# d loss / d feat handed back to autograd, tn_hashgrid_bwd behind it) and of the module-by-module path, each against the CPU port
# evaluated in float64 on the same packed batch (oracle/torch_port.render with a float64 state dict: hash grid, both heads and the
# composite in float64; the weights scan stays the reference kernels' fp32 C restatement, whose conditioning the comparison allows
# for as everywhere else).  Rule: tests/_ties.assert_grads_match_up_to_relu_ties at 1e-4 of each tensor's largest element, the table
# as sixteen tensors, one per level.  Each path is bound against the port, not the two paths against each other.
# ---------------------------------------------------------------------------------------------------------------------------------
def _cut_into_rays(n, seed):
    """packing info that cuts n ray-ordered samples anew so that rays END at lanes 0, 31, 32 and 63 of a wave (counts 1, 31, 1, 31
    from sample 0), rays of a single sample exist, and the rest are 1 .. 256 samples long"""
    rng = np.random.default_rng(seed)
    cnt = [1, 31, 1, 31]
    while sum(cnt) < n:
        cnt.append(int(rng.integers(1, 257)))
    cnt[-1] -= sum(cnt) - n
    cnt = np.array(cnt, np.int32)
    info = np.stack([np.cumsum(cnt) - cnt, cnt], -1).astype(np.int32)
    ends = (info[:, 0] + info[:, 1] - 1) % 64
    assert {0, 31, 32, 63} <= set(ends.tolist()) and (cnt == 1).any() and cnt.min() >= 1 and n % 256 != 0
    return info


@functools.lru_cache(maxsize=None)
def render_case(cut):
    """renderer, packed batch, upstream gradient and the float64 port's inputs, made once and shared by the backward tests (which
    set the renderer's switches themselves and leave parameters and batch unchanged)"""
    renderer, packed, info, bg = _renderer_and_batch()
    plan = ref.levels(**ref.FINE)
    assert plan == tuple(renderer.feature_module.plan)
    if cut:
        n = packed.size(0) - (1 if (packed.size(0) - 1) % 256 else 2)          # drop a sample or two: not a multiple of 256
        packed = packed[:n].contiguous()
        info = torch.from_numpy(_cut_into_rays(n, 11)).to(DEV)
    R = info.size(0)
    # U(-1, 1) * 2^10, the trainer's gradient scale: per-level gradients of order 1, well above the rounding of the accumulate case's
    # one fp32 addition onto a pre-fill of magnitude 2
    G = (torch.rand((R, 3), generator=torch.Generator().manual_seed(17), dtype=torch.float64) * 2 - 1) * 1024.0
    sd64 = {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for k, v in renderer.state_dict().items()}
    port = dict(sd=sd64, packed=packed.cpu().double(), info=info.cpu(), bg=torch.from_numpy(bg).double(), G=G, plan=plan, memo={})
    return renderer, packed, info, G.float().to(DEV), port


def _split_levels(grads, plan):
    out = {k: v for k, v in grads.items() if k != "feature_module.table"}
    for l, (e, o) in enumerate(zip(plan[2], plan[3])):
        out[f"feature_module.table.level{l:02d}"] = grads["feature_module.table"][o:o + e]
    return out


def _port_grads(port):
    """d sum(out * G) / d parameter through the float64 port; evaluations the ties helper repeats unchanged (no tie unit forced) are
    computed once per batch"""
    from oracle import torch_port as tp
    ctrl = tp.ReluControl.current            # (the helper installs a fresh one for its base evaluation, forcing ones for flips)
    forced = ctrl is not None and bool(ctrl.force)
    key = (tp._Weights.exact_backward, tp._Weights.noise_probe, ctrl is not None)
    if not forced and key in port["memo"]:
        grads, found, state = port["memo"][key]
        if ctrl is not None:
            ctrl.found.extend(found)
            ctrl.state.update(state)
        return grads
    grads = tp.grads_of(port["sd"], lambda p: (tp.render(p, port["packed"], port["info"], port["bg"], hashgrid=port["plan"]) * port["G"]).sum())[0]
    grads = _split_levels(grads, port["plan"])
    if not forced:
        port["memo"][key] = (grads, list(ctrl.found) if ctrl is not None else [], dict(ctrl.state) if ctrl is not None else {})
    return grads


def _backward_against_the_port(cut, fused_node, accumulate):
    from _ties import assert_grads_match_up_to_relu_ties
    renderer, packed, info, G, port = render_case(cut)
    fm = renderer.feature_module
    params = dict(renderer.named_parameters())
    renderer.train()
    renderer.fused, renderer.accumulate_into_grad = fused_node, accumulate
    fm.__dict__["accumulate_into_grad"] = accumulate
    pre, ptrs = {}, {}
    try:
        for i, (k, p) in enumerate(params.items()):
            p.grad = None
            if accumulate:
                pre[k] = torch.rand(p.shape, generator=torch.Generator().manual_seed(100 + i)) * 4 - 2
                p.grad = pre[k].to(DEV)
                ptrs[k] = p.grad.data_ptr()
        out = renderer(packed, info)
        assert out.shape == G.shape and torch.isfinite(out).all()
        (out * G).sum().backward()
        got = {}
        for k, p in params.items():
            g = p.grad.detach().cpu().double()
            if accumulate:
                assert p.grad.data_ptr() == ptrs[k], f"{k}: the gradient tensor was replaced"
                g = g - pre[k].double()                   # pre-fill + fresh result: what is left must be the fresh result
            got[k] = g.numpy()
    finally:
        renderer.fused, renderer.accumulate_into_grad = True, False
        fm.__dict__["accumulate_into_grad"] = False
        for p in params.values():
            p.grad = None
    got, want = _split_levels(got, port["plan"]), {}
    flips = assert_grads_match_up_to_relu_ties(got, lambda: _port_grads(port), 1e-4, weights_conditioning=True, cond_cap=2e-3, matched=want)
    rel = want.pop("rel")
    ratios = [float(np.abs(got[k] - want[k]).max() / (rel[k] * np.abs(want[k]).max())) for k in sorted(want) if ".level" in k]
    print(f"{'fused node' if fused_node else 'module path'}, {'accumulate' if accumulate else 'fresh'}, {packed.size(0)} samples in "
          f"{info.size(0)} rays: table gradient error / allowance per level, worst {max(ratios):.3f} at level {int(np.argmax(ratios))}; "
          f"{flips} tie units flipped; smallest per-level max |gradient| {min(float(np.abs(want[k]).max()) for k in want if '.level' in k):.3e}")


@pytest.mark.parametrize("accumulate", [False, True], ids=["fresh", "accumulate"])
@pytest.mark.parametrize("fused_node", [True, False], ids=["fused", "modules"])
def test_renderer_backward_matches_the_fp64_port(fused_node, accumulate):
    """Accumulate: the renderer's and the field's switches set as run.Trainer sets them and every .grad pre-filled with U(-2, 2): the
    result is the pre-fill plus the fresh gradient (the rounding of that one fp32 addition, 2^-24 * 4, is far below 1e-4 of every
    level's largest element here: the smallest is printed) and every gradient tensor keeps its storage."""
    _backward_against_the_port(False, fused_node, accumulate)


@pytest.mark.parametrize("fused_node", [True, False], ids=["fused", "modules"])
def test_renderer_backward_on_rays_cut_inside_waves(fused_node):
    """The same samples cut into other rays: ray ends at lanes 0, 31, 32 and 63 of a wave, rays of one sample, a total that is no
    multiple of 256 -- what the trainer's ray-ordered batches feed the scan, the composite and the merged scatter on every step."""
    _backward_against_the_port(True, fused_node, fused_node)
