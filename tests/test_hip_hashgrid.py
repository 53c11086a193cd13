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


def test_renderer_takes_the_fused_node_and_equals_the_module_path():
    import _g22
    from tinynerf_amd import fused
    from tinynerf_amd.run import TrainConfig, build_renderer
    o, d, _, bg = _g22.ray_table()
    cfg = TrainConfig(method="hashgrid", n_samples=64, occupancy_res=32, hashgrid_log2_table_size=14)
    torch.manual_seed(3)
    renderer, _, provider = build_renderer(cfg, torch.from_numpy(bg).to(DEV), torch.device(DEV))
    with torch.no_grad():
        renderer.feature_module.table.uniform_(-1, 1)                     # (the initialisation's 1e-4 would make every feature ~ 0)
    idx = np.arange(0, 80000, 263)[:300]
    packed, info = provider(torch.from_numpy(o[idx]).to(DEV), torch.from_numpy(d[idx]).to(DEV), training=False)
    assert fused.supports(renderer) and packed.size(0) > 3000
    with torch.no_grad():
        a = renderer(packed, info)
        renderer.fused = False
        b = renderer(packed, info)
    assert a.shape == (300, 3) and torch.isfinite(a).all()
    err = float((a - b).abs().max())
    print(f"fused against module path on {packed.size(0)} samples: max difference {err:.3e}")
    assert err <= TOL and float(a.std()) > 1e-3
