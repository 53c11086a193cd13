"""GPU: the three fused K-Planes launches at the C ABI, per sample, at tile, workgroup and round edges.

    tn_kplanes_mlp_fwd_pair   gather + both heads: training form (lean and stash workspaces) and inference form (no workspaces)
    tn_kplanes_mlp_fwd        gather + sigma head
    tn_kplanes_mlp_bwd_pair   data-gradient chain + plane scatter, then the heads' weight gradients

Sizes, planted out-of-range samples, probe positions and every derivation behind them: tests/_kplanes_fused_cases.py (checked on the CPU
by tests/test_kplanes_fused_cases.py).  Heads: VanillaOpacityDecoder(96) and VanillaColorDecoder(8, 96, 64, 3) behind a per-ray table
(tn_dir_encode), the sigma bias raised by 3; rays of 1 .. 256 samples.  Forms: the `heads` fixture (f16x2, fp32); under f16x2 both the
lean (TN_MLP_LEAN) and the stash workspace.  Coordinates sit in rows of 3, 4 or 7 floats whose other columns hold NaN; every output
carries 64 guard rows behind n; workspaces start from one NaN bit pattern and are compared as int32.  The second-round sizes run
with stride 7 only.

Forward
  F1  feat against fp64 (grid_sample, forward only): general fixtures within (0 + 17) 2^-24 A per element and nothing where A == 0 --
      the bound the stand-alone tn_kplanes_fwd is held to (test_hip_scatter.py, KP_FWD); exact fixture: equal to the fp64 value
      (compared as numbers: an empty sum's zero has no sign to get wrong).
  F2  y, partner_y and feat equal, bit for bit and for every sample, those of tn_kplanes_fwd + tn_mlp_fwd_stash_pair.
  F3  both workspaces equal the two-launch sequence's in the columns of samples < n (ReLU bit rows, last pre-activation, H rows in the
      stash form); under TN_MLP_LEAN the H rows keep the prefill in both.
  F4  guard rows untouched.
  F5  inference pair (both workspaces NULL), with a feat buffer and with feat == NULL: y / partner_y equal tn_kplanes_fwd + tn_mlp_fwd of
      each head bit for bit; a given feat keeps its prefill whole; the coordinate buffer (NaN columns included) keeps its bits.
  F6  tn_kplanes_mlp_fwd: feat as F1, y bit for bit against tn_kplanes_fwd + tn_mlp_fwd, guard rows.
  F7  the inference form's refusals with real buffers (the table in test_mlp_workspace_abi.py has the same rows on dummy pointers):
      every output keeps its prefill.
Backward (workspaces and feat from the fused training forward of the same case; upstream gradients zero except on the probe samples,
there randn * exp(U(-6, 0)); grad_feat requested, prefilled with NaN)
  B1  grad_feat exactly 0 on every other sample, guard rows untouched.
  B2  probe rows of grad_feat against grad_x of tn_mlp_bwd_pair on the same workspaces: 2e-5 of the row's largest element (the heads'
      tolerance of test_hip_models.py / test_hip_mlp_fp64.py part B; both launches read the same stashed masks).
  B3  every head parameter gradient against tn_mlp_bwd_pair's: 2e-5 of the tensor's largest element.
  B4  plane gradients against the fp64 scatter of the launch's own grad_feat: (m + 14) 2^-24 A with m the probes' tap counts
      (test_hip_scatter.py, KP_BWD); a texel no probe touches keeps the fill's bits.
  The full call and the TN_MLP_CHAIN_ONLY + TN_MLP_WGRAD_ONLY split give the same numbers (==): grad_feat and the plane gradients
  always -- no texel sum has two non-zero terms in one atomic race -- and the head gradients wherever that premise holds for them too.
  A head-gradient sum has one term per weight-gradient flush, i.e. per group of tiles, and the flushes are fp32 atomics from different
  blocks: with probes in three or more tiles their order is free, and the FULL CALL DOES NOT REPEAT ITSELF (measured: 0 .. 500 elements
  of a tensor differ between two identical calls, by up to 1.1e-7 of its largest element, in every form at n >= 255; never at n <= 33,
  never in grad_feat or a plane).  So the head gradients of the two modes are compared with == in the all-probes run when the probes
  lie in at most two tiles (a two-term sum commutes), and in every case once more PER PROBE -- upstream gradient on that one sample only,
  every sum a single term -- which holds the split to the full call at each edge position; B3 holds the all-probes sums.
  Gradient buffers start from FILL = 2^-100, a known non-zero value: an entry nobody adds to must keep exactly those bits, while an
  entry that is added to loses the fill below the last bit of any sum larger than 2^-76 and otherwise moves it by less than the bound's
  absolute floor (1e-30) -- so B4's bound stays the one of the scatter alone, with `got - FILL` as the sum.

Observed on an MI355X, worst over all cases of a form (pytest -s prints them; reported, not tolerances):
    form          F1 err / bound   B2 row ratio   B3 tensor ratio   B4 err / bound
    f16x2/lean        0.335             0            1.5e-7            0.312
    f16x2/stash       0.335             0            1.5e-7            0.312
    fp32/stash        0.350             0            1.5e-7            0.312
    sigma launch      0.379 (F6, either arithmetic)
  B2 is 0 in every case: the probe rows of grad_feat are grad_x of tn_mlp_bwd_pair bit for bit.  B3 moves between runs with the
  order of the flush atomics (1.3e-7 .. 1.5e-7 seen).

Out of scope: a non-finite texel 0 reaching out-of-range samples through plane_gather's weight-0 read (_kplanes_fused_cases.py).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _kplanes_fused_cases as kc
import _scatter_orders as so

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD, SENT, FILL = 64, -777.25, 2.0 ** -100
KP_FWD, KP_BWD, HEAD_TOL = 17, 14, 2e-5
STRIDES = (3, 4, 7)
E_SIZE, E_CONFIG, E_ALIGN = -2, -3, -4
CASES = [(name, key, s) for name in kc.FIXTURES for key in kc.SMALL_KEYS for s in STRIDES] + [(name, "round2", 7) for name in kc.FIXTURES]
IDS = ["%s-%s-s%d" % c for c in CASES]
WORST = {}


def _note(form, what, ratio):
    k = (form, what)
    WORST[k] = max(WORST.get(k, 0.0), float(ratio))
    print(f"{form} {what}: this case {float(ratio):.4g}, worst so far {WORST[k]:.4g}")


def _forms(heads):
    """(label, TN_MLP_LEAN) per workspace form of this arithmetic"""
    return [("f16x2/lean", True), ("f16x2/stash", False)] if heads == "f16x2" else [("fp32/stash", False)]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return bool(torch.equal(_bits(a), _bits(b)))


def _nan_bits():
    return int(_bits(torch.full((1,), float("nan")))[0])


def _prefilled(shape, value):
    return torch.full(shape, value, device=DEV)


def _untouched(buf, n, value):
    """rows n .. of `buf` still hold the prefill's bits"""
    return _same_bits(buf[n:], torch.full_like(buf[n:], value))


@functools.lru_cache(maxsize=None)
def _heads():
    from tinynerf_amd import models as m
    torch.manual_seed(20)
    sig, cd = m.VanillaOpacityDecoder(96), m.VanillaColorDecoder(8, 96, 64, 3)
    with torch.no_grad():
        sig.net.net[2].bias += 3.0
    sig, cd = sig.to(DEV), cd.to(DEV)
    return ([p.detach().contiguous() for p in sig.net.params()], [p.detach().contiguous() for p in cd.net.params()],
            cd.pe.freqs.detach().contiguous())


class _Inputs:
    def __init__(self, name, n, stride):
        from tinynerf_amd import _lib as L, models
        self.name, self.n, self.stride, self.dev = name, n, stride, torch.device(DEV)
        self.x, self.planes, self.exact = kc.fixture(name, n)
        self.shapes = kc.shapes_of(name)
        self.coords = torch.full((n, stride), float("nan"), device=DEV)
        self.coords[:, :3] = torch.from_numpy(np.array(self.x)).to(DEV)
        self.plane_t = [torch.from_numpy(np.array(p)).permute(2, 0, 1)[None].to(DEV).contiguous(memory_format=torch.channels_last)
                        for p in self.planes]
        self.kdesc, self.keep = models._kplanes_desc(self.plane_t)
        seed = so.seed_of("rays", name, n)
        cnt = kc.ray_counts(n, seed)
        R = len(cnt)
        self.ray_ids = torch.repeat_interleave(torch.arange(R, dtype=torch.int32), torch.from_numpy(cnt).long()).to(DEV).contiguous()
        g = torch.Generator().manual_seed(seed)
        self.dirs = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1).to(DEV).contiguous()
        self.sp, self.rp, self.freqs = _heads()
        self.table = torch.empty(R, 56, device=DEV)
        L.call("tn_dir_encode", self.dev, L.ptr(self.dirs), C.c_int64(R), L.ptr(self.freqs), C.c_int(8), L.ptr(self.table), C.c_int(56))
        self.kp = (C.byref(self.kdesc), L.ptr(self.coords), C.c_int64(stride))

    def descs(self, rflags=0, sflags=0):
        from tinynerf_amd import fused
        return fused._head_descs(self.sp, self.rp, 96, 8, self.freqs, self.ray_ids, self.table, rflags, sflags)

    def workspaces(self, rdesc, sdesc):
        from tinynerf_amd import fused
        ws_r, rb = fused._workspace(rdesc, self.n, self.dev)
        ws_s, sb = fused._workspace(sdesc, self.n, self.dev)
        assert rb > 0 and sb > 0
        ws_r.fill_(float("nan"))
        ws_s.fill_(float("nan"))
        return ws_r, rb, ws_s, sb

    def outputs(self):
        n = self.n
        return _prefilled((n + GUARD, 96), SENT), _prefilled((n + GUARD, 3), SENT), _prefilled((n + GUARD, 1), SENT)

    def gather(self, feat):
        from tinynerf_amd import _lib as L
        L.call("tn_kplanes_fwd", self.dev, *self.kp, C.c_int64(self.n), L.ptr(feat))


def _train_fwd(inp, lean, fused_gather):
    """the training forward as one launch, or as tn_kplanes_fwd + tn_mlp_fwd_stash_pair; -> feat, y, partner_y, ws_r, rb, ws_s, sb"""
    from tinynerf_amd import _lib as L
    flags = L.MLP_LEAN if lean else 0
    rdesc, sdesc = inp.descs(flags, flags)
    ws_r, rb, ws_s, sb = inp.workspaces(rdesc, sdesc)
    feat, y, py = inp.outputs()
    n = C.c_int64(inp.n)
    if fused_gather:
        L.call("tn_kplanes_mlp_fwd_pair", inp.dev, *inp.kp, C.byref(rdesc), C.byref(sdesc), L.ptr(inp.table), n, L.ptr(feat), L.ptr(y), L.ptr(py),
               L.ptr(ws_r), C.c_int64(rb), L.ptr(ws_s), C.c_int64(sb))
    else:
        inp.gather(feat)
        L.call("tn_mlp_fwd_stash_pair", inp.dev, C.byref(rdesc), C.byref(sdesc), L.ptr(feat), L.ptr(inp.table), n, L.ptr(y), L.ptr(py),
               L.ptr(ws_r), C.c_int64(rb), L.ptr(ws_s), C.c_int64(sb))
    return feat, y, py, ws_r, rb, ws_s, sb


def _check_feat(inp, feat, form, what):
    """F1"""
    got = feat[:inp.n].cpu().numpy()
    ref, aref = kc.reference(inp.name, inp.n)
    if inp.exact:
        bad = got != ref.astype(np.float32)
        assert not bad.any(), f"{what}: {int(bad.sum())} features of {int(bad.any(1).sum())} samples differ from the exact value"
        return
    bound = KP_FWD * 2.0 ** -24 * aref * (1.0 + 2.0 ** -10) + 1e-30
    _note(form, "F1 |feat - fp64| / bound", (np.abs(got.astype(np.float64) - ref) / bound).max())
    so.assert_within(got, ref, aref, 0, KP_FWD, what)


def _tile_view(ws, n):
    return _bits(ws).view((n + 31) // 32, -1, 32)


def _check_workspaces(n, got, want, h_rows, lean, what):
    """F3: int32 equality in the columns of samples < n of every tile.  `h_rows`: a tile starts with its H rows, NH * H of them
    (mlp_stage.h StashTile::h, NH = n_layers - 1 hidden layers of width H = 64: 4 * 64 for the colour head, 64 for the sigma head)"""
    a, b = _tile_view(got, n), _tile_view(want, n)
    assert a.shape == b.shape
    live = (torch.arange(a.size(0) * 32, device=a.device) < n).view(-1, 1, 32)
    diff = (a != b) & live
    assert not bool(diff.any()), f"{what}: {int(diff.sum())} workspace words differ, first (tile, row, sample) {diff.nonzero()[0].tolist()}"
    nan = _nan_bits()
    for v in (a, b):
        if lean:
            assert bool((v[:, :h_rows] == nan).all()), f"{what}: a lean forward wrote H rows"
        else:
            assert not bool(((v[:, :h_rows] == nan) & live).any()), f"{what}: H rows of live samples left unwritten"


# ------------------------------------------------------------------------------------------------ forward, training form
@pytest.mark.parametrize("name,key,stride", CASES, ids=IDS)
def test_training_forward_per_sample(heads, name, key, stride):
    """F1 - F4"""
    for form, lean in _forms(heads):
        n = kc.size_of("train_" + heads, key)
        inp = _Inputs(name, n, stride)
        what = f"{form} {name} n={n} stride={stride}"
        feat, y, py, ws_r, _, ws_s, _ = _train_fwd(inp, lean, True)
        feat2, y2, py2, ws_r2, _, ws_s2, _ = _train_fwd(inp, lean, False)
        for a, b, label in ((y, y2, "y"), (py, py2, "partner_y"), (feat, feat2, "feat")):
            diff = (_bits(a[:n]) != _bits(b[:n])).any(1)
            assert not bool(diff.any()), f"{what}: {label} differs from the two-launch sequence at samples {diff.nonzero()[:8, 0].tolist()}"
            assert _untouched(a, n, SENT), f"{what}: {label} guard rows written"
        assert bool(torch.isfinite(y[:n]).all()) and bool(torch.isfinite(py[:n]).all())
        _check_workspaces(n, ws_r, ws_r2, 4 * 64, lean, what + " colour workspace")
        _check_workspaces(n, ws_s, ws_s2, 64, lean, what + " sigma workspace")
        _check_feat(inp, feat, form, what)


# ------------------------------------------------------------------------------------------------ forward, inference forms
def _infer_reference(inp):
    """tn_kplanes_fwd, then tn_mlp_fwd of each head, ungated"""
    from tinynerf_amd import _lib as L
    rdesc, sdesc = inp.descs()
    feat, y, py = inp.outputs()
    inp.gather(feat)
    n = C.c_int64(inp.n)
    L.call("tn_mlp_fwd", inp.dev, C.byref(rdesc), L.ptr(feat), L.ptr(inp.table), n, L.ptr(y), C.c_void_p(None))
    L.call("tn_mlp_fwd", inp.dev, C.byref(sdesc), L.ptr(feat), C.c_void_p(None), n, L.ptr(py), C.c_void_p(None))
    return feat, y, py


def _infer_pair(inp, feat, y, py, check=True):
    from tinynerf_amd import _lib as L
    rdesc, sdesc = inp.descs()
    args = (*inp.kp, C.byref(rdesc), C.byref(sdesc), L.ptr(inp.table), C.c_int64(inp.n), L.ptr(feat), L.ptr(y), L.ptr(py),
            C.c_void_p(None), C.c_int64(0), C.c_void_p(None), C.c_int64(0))
    if check:
        return L.call("tn_kplanes_mlp_fwd_pair", inp.dev, *args)
    with torch.cuda.device(inp.dev):
        return L.lib().tn_kplanes_mlp_fwd_pair(*args, L.stream(inp.dev))


@pytest.mark.parametrize("name,key,stride", CASES, ids=IDS)
def test_inference_pair_per_sample(heads, name, key, stride):
    """F5"""
    n = kc.size_of("infer_pair_" + heads, key)
    inp = _Inputs(name, n, stride)
    what = f"{heads} {name} n={n} stride={stride}"
    _, y2, py2 = _infer_reference(inp)
    before = inp.coords.clone()
    for with_feat in (False, True):
        feat, y, py = inp.outputs()
        if not with_feat and n * stride < 4:          # no 16 bytes of coordinates for the dummy operand line: refused, nothing written
            assert _infer_pair(inp, None, y, py, check=False) == E_SIZE
            assert _untouched(y, 0, SENT) and _untouched(py, 0, SENT) and _same_bits(inp.coords, before)
            continue
        _infer_pair(inp, feat if with_feat else None, y, py)
        tag = what + (" feat given" if with_feat else " feat NULL")
        for a, b, label in ((y, y2, "y"), (py, py2, "partner_y")):
            diff = (_bits(a[:n]) != _bits(b[:n])).any(1)
            assert not bool(diff.any()), f"{tag}: {label} differs from tn_kplanes_fwd + tn_mlp_fwd at samples {diff.nonzero()[:8, 0].tolist()}"
            assert _untouched(a, n, SENT), f"{tag}: {label} guard rows written"
        assert _untouched(feat, 0, SENT), f"{tag}: the inference form wrote feature rows"
        assert _same_bits(inp.coords, before), f"{tag}: the coordinate buffer changed"


@pytest.mark.parametrize("name,key,stride", CASES, ids=IDS)
def test_gather_sigma_per_sample(heads, name, key, stride):
    """F6"""
    from tinynerf_amd import _lib as L
    n = kc.size_of("infer_sigma", key)
    inp = _Inputs(name, n, stride)
    what = f"{heads} {name} n={n} stride={stride}"
    feat2, _, py2 = _infer_reference(inp)
    _, sdesc = inp.descs()
    feat, _, py = inp.outputs()
    L.call("tn_kplanes_mlp_fwd", inp.dev, *inp.kp, C.byref(sdesc), C.c_int64(n), L.ptr(feat), L.ptr(py))
    for a, b, label in ((py, py2, "y"), (feat, feat2, "feat")):
        diff = (_bits(a[:n]) != _bits(b[:n])).any(1)
        assert not bool(diff.any()), f"{what}: {label} differs from tn_kplanes_fwd + tn_mlp_fwd at samples {diff.nonzero()[:8, 0].tolist()}"
        assert _untouched(a, n, SENT), f"{what}: {label} guard rows written"
    _check_feat(inp, feat, heads + "/sigma", what)


def test_inference_pair_refusals_leave_the_outputs_alone(heads):
    """F7"""
    from tinynerf_amd import _lib as L
    inp = _Inputs("small", 40, 4)
    gate = torch.ones(40, device=DEV)
    shifted = torch.full((40 * 4 + 4,), float("nan"), device=DEV)
    shifted[1:161] = inp.coords.view(-1)

    def run(coords=None, stride=4, n=40, with_feat=True, gate_r=None, gate_s=None):
        rdesc, sdesc = inp.descs()
        rdesc.row_gate = None if gate_r is None else gate_r.data_ptr()
        sdesc.row_gate = None if gate_s is None else gate_s.data_ptr()
        feat, y, py = inp.outputs()
        cp = C.c_void_p(inp.coords.data_ptr() if coords is None else coords)
        with torch.cuda.device(inp.dev):
            rc = L.lib().tn_kplanes_mlp_fwd_pair(C.byref(inp.kdesc), cp, C.c_int64(stride), C.byref(rdesc), C.byref(sdesc), L.ptr(inp.table),
                                                 C.c_int64(n), L.ptr(feat if with_feat else None), L.ptr(y), L.ptr(py), C.c_void_p(None),
                                                 C.c_int64(0), C.c_void_p(None), C.c_int64(0), L.stream(inp.dev))
        torch.cuda.synchronize()
        assert _untouched(feat, 0, SENT) and _untouched(y, 0, SENT) and _untouched(py, 0, SENT), "a refused call wrote an output"
        return rc
    assert run(coords=shifted.data_ptr() + 4) == E_ALIGN
    assert run(coords=shifted.data_ptr() + 4, with_feat=False) == E_ALIGN
    assert run(stride=3, n=1, with_feat=False) == E_SIZE
    assert run(gate_r=gate) == E_CONFIG
    assert run(gate_s=gate) == E_CONFIG
    assert run(gate_s=gate, with_feat=False) == E_CONFIG


# ------------------------------------------------------------------------------------------------ backward
def _backward(inp, fw, lean, gy, gs, mode):
    """mode "heads": tn_mlp_bwd_pair (grad_x); "full": tn_kplanes_mlp_bwd_pair in one call; "split": CHAIN_ONLY, then WGRAD_ONLY.
    Every mode starts from clones of the forward's workspaces and from FILL in every gradient buffer."""
    from tinynerf_amd import _lib as L, fused
    feat, _, _, ws_r, rb, ws_s, sb = fw
    ws_r, ws_s = ws_r.clone(), ws_s.clone()
    n = inp.n
    base = L.MLP_STASHED | (L.MLP_LEAN if lean else 0)
    rdesc, sdesc = inp.descs(base, base)
    base = rdesc.flags
    g_sig, g_rgb = [torch.full_like(p, FILL) for p in inp.sp], [torch.full_like(p, FILL) for p in inp.rp]
    gw = fused._grad_ptrs(g_sig, g_rgb)
    gfeat = _prefilled((n + GUARD, 96), float("nan"))
    tail = (L.ptr(gfeat), L.ptr(ws_r), C.c_int64(rb), L.ptr(ws_s), C.c_int64(sb))
    if mode == "heads":
        L.call("tn_mlp_bwd_pair", inp.dev, C.byref(rdesc), C.byref(sdesc), L.ptr(feat), L.ptr(inp.table), L.ptr(gy), L.ptr(gs), C.c_int64(n),
               *gw, *tail)
        return gfeat, g_rgb + g_sig, None
    g_planes = [torch.full((H, W, 32), FILL, device=DEV) for H, W in inp.shapes for _ in range(3)]
    gp = ((C.c_void_p * 3) * L.TN_KPLANES_MAX_SCALES)(*[tuple(g.data_ptr() for g in g_planes[3 * s:3 * s + 3]) for s in range(3)])
    for phase in (0,) if mode == "full" else (L.MLP_CHAIN_ONLY, L.MLP_WGRAD_ONLY):
        rdesc.flags = base | phase
        L.call("tn_kplanes_mlp_bwd_pair", inp.dev, *inp.kp, gp, C.byref(rdesc), C.byref(sdesc), L.ptr(feat), L.ptr(inp.table), L.ptr(gy),
               L.ptr(gs), C.c_int64(n), *gw, *tail)
    return gfeat, g_rgb + g_sig, g_planes


@pytest.mark.parametrize("name,key,stride", CASES, ids=IDS)
def test_backward_probes_per_sample(heads, name, key, stride):
    """B1 - B4 and the split call"""
    n = kc.size_of("chain", key)
    inp = _Inputs(name, n, stride)
    pr = kc.probes(n)
    rng = np.random.default_rng(so.seed_of("probes", name, n))
    gy_h, gs_h = np.zeros((n, 3), np.float32), np.zeros((n, 1), np.float32)
    scale = np.exp(rng.uniform(-6.0, 0.0, (len(pr), 1)))
    gy_h[pr] = rng.standard_normal((len(pr), 3)) * scale
    gs_h[pr] = rng.standard_normal((len(pr), 1)) * scale
    gy, gs = torch.from_numpy(gy_h).to(DEV), torch.from_numpy(gs_h).to(DEV)
    probe = torch.zeros(n, dtype=torch.bool, device=DEV)
    probe[torch.from_numpy(pr).to(DEV)] = True
    for form, lean in _forms(heads):
        what = f"{form} {name} n={n} stride={stride}"
        fw = _train_fwd(inp, lean, True)
        gx_ref, heads_ref, _ = _backward(inp, fw, lean, gy, gs, "heads")
        gfeat, heads_full, planes_full = _backward(inp, fw, lean, gy, gs, "full")
        gfeat_s, heads_split, planes_split = _backward(inp, fw, lean, gy, gs, "split")
        # B1
        stray = (gfeat[:n] != 0).any(1) & ~probe
        assert not bool(stray.any()), f"{what}: grad_feat not 0 at samples {stray.nonzero()[:8, 0].tolist()} (no upstream gradient there)"
        assert _untouched(gfeat, n, float("nan")), f"{what}: grad_feat guard rows written"
        # B2
        got, ref = gfeat[:n][probe].double(), gx_ref[:n][probe].double()
        assert bool(torch.isfinite(got).all()) and float(ref.abs().max()) > 0
        ratio = ((got - ref).abs().amax(1) / ref.abs().amax(1).clamp_min(1e-300)).max()
        _note(form, "B2 |grad_feat - grad_x| / row max", ratio)
        assert float(ratio) <= HEAD_TOL, f"{what}: probe rows of grad_feat differ from tn_mlp_bwd_pair's grad_x by {float(ratio):.3g} of a row"
        # B3
        worst = 0.0
        for i, (a, b) in enumerate(zip(heads_full, heads_ref)):
            a, b = a.double() - FILL, b.double() - FILL
            assert bool(torch.isfinite(a).all())
            r = float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))
            worst = max(worst, r)
            assert r <= HEAD_TOL, f"{what}: head gradient {i} {tuple(a.shape)} differs from tn_mlp_bwd_pair's by {r:.3g} of its largest element"
        _note(form, "B3 |head grad - tn_mlp_bwd_pair's| / tensor max", worst)
        # B4
        g = gfeat[:n][probe].cpu().numpy()
        xp = np.array(inp.x)[pr]
        _, _, rg, arg = so.kplanes_ref(xp, list(inp.planes), g)
        worst = 0.0
        for i, gpl in enumerate(planes_full):
            H, W = inp.shapes[i // 3]
            m = so.tap_counts(xp, H, W, i % 3)[:, :, None]
            got = gpl.cpu().numpy()
            quiet = np.broadcast_to(m == 0, got.shape)
            assert np.array_equal(got[quiet].view(np.int32), np.full(int(quiet.sum()), FILL, np.float32).view(np.int32)), \
                f"{what} plane {i}: a texel no probe touches changed"
            acc = got.astype(np.float64) - FILL
            bound = (m + KP_BWD) * 2.0 ** -24 * arg[i] * (1.0 + 2.0 ** -10) + 1e-30
            worst = max(worst, float((np.abs(acc - rg[i]) / bound).max()))
            so.assert_within(acc, rg[i], arg[i], m, KP_BWD, f"{what} plane {i}")
        _note(form, "B4 |plane grad - fp64| / bound", worst)
        # the split call: the same numbers
        assert bool((gfeat_s[:n] == gfeat[:n]).all()), f"{what}: CHAIN_ONLY grad_feat differs from the full call's"
        for i, (a, b) in enumerate(zip(planes_split, planes_full)):
            assert bool((a == b).all()), f"{what}: plane gradient {i} of the split call differs from the full call's"
        if len({int(p) // 32 for p in pr}) <= 2:
            _heads_equal(heads_split, heads_full, what)
        # ... and per probe, where every head-gradient sum has one term
        for p in pr:
            gy1, gs1 = torch.zeros_like(gy), torch.zeros_like(gs)
            gy1[p], gs1[p] = gy[p], gs[p]
            f_gfeat, f_heads, f_planes = _backward(inp, fw, lean, gy1, gs1, "full")
            s_gfeat, s_heads, s_planes = _backward(inp, fw, lean, gy1, gs1, "split")
            tag = f"{what} probe {int(p)} alone"
            assert bool((s_gfeat[:n] == f_gfeat[:n]).all()) and bool((f_gfeat[p] == gfeat[p]).all()), f"{tag}: grad_feat"
            for i, (a, b) in enumerate(zip(s_planes, f_planes)):
                assert bool((a == b).all()), f"{tag}: plane gradient {i} of the split call differs from the full call's"
            _heads_equal(s_heads, f_heads, tag)


def _heads_equal(got, want, what):
    for i, (a, b) in enumerate(zip(got, want)):
        bad = a != b
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements of head gradient {i} of the split call differ from the full call's"
