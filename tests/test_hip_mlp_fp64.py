"""GPU: the MLP kernels (csrc/mlp.hip, mlp_bwd2.hip, mlp_bwd_layers.hip, mlp_f2_layers.hip, mlp_fused_f2.hip, mlp_b3_layers.hip,
mlp_wgrad_rc.hip, mlp_wgrad_rows.hip, heads_dx.hip) against fp64, per element, layer by layer and at tile edges.

A. Shallow stacks (one or two ReLU layers, tests/_mlp_ref.PART_A) through the module API against the fp64 reference's per-element
   rounding-error bound (tests/_mlp_ref.py): y, grad_x, every dW and db, element by element, nothing normalised by a tensor maximum.
   Samples that hold a tie unit (|pre| <= 2 E) are rejected when the fixture is drawn, so n and every sample's position are exact.
B. Production-depth stacks (the bound rejects every sample there) with SPARSE upstream gradients: grad_y is zero except on at most eight
   probe samples at the tile / round edges.  grad_x must be exactly zero on every other sample (NaN-prefilled buffer), and with at most
   eight terms per sum a lost or doubled edge sample is an error of 10 % or more of a parameter gradient, not 1 / n.  Compared with the
   fp32 network through oracle/torch_port.mlp up to the state of tie units (tests/_ties.py) at the tolerances these stacks already have
   in test_hip_models.py (3e-5 wide stacks, 2e-5 heads).  A dense run with the probes scaled by 2^12 repeats it on the dense path's data.

Sizes.  1, 31, 32, 33, 65 and the smallest n at which a persistent loop runs a second round: 8193 at every width, plus 16385 at widths 128
and 256.  Which launches that reaches, read off their grid computations (32-sample tiles, at most 256 x per_cu workgroups):
* 8193 (tile 256 = sample 8192 opens the second round): the weight-gradient launches with one tile per workgroup and round on 256
  workgroups -- fp32 mode at width 128 / 256: ``grid_blocks(n, 1, 256)`` = min(n_tiles, 256) in launch_wgrad_lds (mlp_bwd_layers.hip);
  width 64: ``grid_blocks(n, 1, 256)`` for mlp_wgrad4_kernel (mlp_bwd2.hip, grid_blocks in mlp_stage.h) -- and the width-256 layer forward /
  data-gradient kernels, ``stream_blocks(n, STREAMS)`` = min(ceil(n_tiles / STREAMS), 256) workgroups (mlp_layers.h) with STREAMS = 1
  (launch_*_wreg in mlp_bwd_layers.hip, launch_*_f2 in mlp_f2_layers.hip, launch_*_b3 in mlp_b3_layers.hip).
* 16385 (sample 16384): the f16x2 and bf16x3 weight-gradient launches, ``grid_blocks(n, 1, 256 * per_cu)`` = min(n_tiles, 256 * per_cu)
  with per_cu = 2 at both widths (launch_wgrad_f2 / launch_wgrad_b3: 48 / 72 KB of LDS, two workgroups per CU), and the width-128 layer
  forward / data-gradient kernels (STREAMS = 2).
* NOT reached by any n of part A: the cross-layer launches of mlp_fused_f2.hip (the default f16x2 form) run ``min(ceil(n_tiles / NW),
  256)`` workgroups with NW = 4 or 8 waves, so their second round opens at sample 32768 or 65536.  Part B reaches both: its 40037 gives
  the NW = 4 launches a second round (its probes 40004 and 40036 lie in it), and cobafa_128x6 also runs at 65573 = 256 x 8 x 32 + 37, where
  the NW = 8 launches -- the width-128 chain, fused_chain_kernel<128>, and the width-128 inference forward, fused_fwd_kernel<128, false> --
  open a second round of two tiles, the last one ragged (probes 65535 / 65536 on the round edge, 65540 and 65572 in the second round;
  the inference forward has a case of its own below, through tn_mlp_fwd_ws).  Still one round at every n here: the width-64 forward /
  chain launches (8 to 16 tiles per workgroup and round, 256 or 512 workgroups: a second round at sample 65536 or later).
Part B adds the ragged 40037 and, for cobafa_128x6, the ragged 65573.

The pair backward (tn_mlp_bwd_pair) only takes the 5-layer colour head: four ReLU layers, 98.9 % of the draws hold a tie unit
(tests/test_mlp_ref.py).  It is therefore held to the bound forward-only (part A, both head outputs, lean and stashed) and its backward
runs in part B; grad_x there is the sum of the two heads' and is compared with the sum of the references.

Observed on an MI355X (reported, not a tolerance; pytest -s prints every figure): the largest error of part A as a share of its bound,
over all shapes, sizes, stash on / off and both forms -- width 64: f16x2 y 0.002, grad_x 0.010, dW 0.032, db 0.053; fp32 0.003, 0.013,
0.046, 0.106.  Width 128: f16x2 0.010, 0.004, 0.078, 0.036; bf16x3 0.011, 0.004, 0.097, 0.041; fp32 0.011, 0.004, 0.061, 0.043.  Width
256: f16x2 0.004, < 0.001, 0.039, 0.029; bf16x3 0.004, < 0.001, 0.044, 0.029; fp32 0.005, < 0.001, 0.032, 0.023.  Pair forward: 0.003.
The layer-wise and the cross-layer forms, and stash on and off, give the same figures to three digits.  mlp36_128x2_37 (an output below the
width that is no multiple of 4: the element-wise y stores of the last layer's narrow epilogue, emit_last_narrow in mlp_layers.h, and a second
output block with five rows) stays below them: y 0.001, grad_x 0.003, dW 0.046, db 0.041 over the three modes.
Two shapes reach the edges of the width-64 kernels that the reference's decoders do not.  mlp40_64x1_3 (two layers: the two-pass backward,
stash on and off; in_dim 40, three outputs) runs mlp_wgrad_kernel<64, 1, 1, 8, 4> with a partial second k tile in its flush (k < K), the
chain's grad_x store with a partial second 32-column block, the <= 4-output layer with out = 3 and first_dgrad on the main head: f16x2 y
0.005, grad_x 0.041, dW 0.081, db 0.062; fp32 0.006, 0.052, 0.243, 0.124 (the largest dW and db shares are those of n = 1, one term per
sum).  mlp38_64x2_6 (in_dim % 4 != 0, six outputs) takes the generic first layer with the element-wise tail of fetch_input and the MFMA
output layer with element-wise y stores wherever tn_mlp_fwd runs it (mlp_fwd_kernel<64, true, 16, false, false, false>, under f16x2 as
well: the f16x2 heads need in_dim % 16 == 0); with three layers its stashed forward and its backward are the layer-by-layer form: f16x2
y 0.001, grad_x 0.008, dW 0.023, db 0.057; fp32 0.001, 0.011, 0.029, 0.098.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _mlp_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 5
SECOND_ROUND = 256 * 32 + 1                 # see the docstring
SIZES = (1, 31, 32, 33, 65, SECOND_ROUND)


def _sizes(spec, extra=()):
    return SIZES + ((2 * 256 * 32 + 1,) if spec.hidden >= 128 else ()) + tuple(extra)


def cu(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


_FX, _REF = {}, {}


def _fixture(key, spec, n, reject=True):
    if (key, n) not in _FX:
        _FX[(key, n)] = R.fixture(spec, n, SEED, reject_ties=reject)
    return _FX[(key, n)]


def _reference(key, fx, mode):
    k = (key, fx.x.shape[0], mode)
    if k not in _REF:
        ref = R.reference(fx.spec, fx.layers, fx.x, fx.aux, fx.freqs, fx.grad_y, R.C_MODE[mode])
        _REF[k] = {q: ref[q] for q in ("y", "E_y", "grad_x", "E_grad_x", "dW", "E_dW", "db", "E_db")}      # (not the per-layer activations)
    return _REF[k]


def _hold(got, ref, what, keys=("y", "grad_x", "dW", "db")):
    """every element inside its bound; the largest error as a share of the bound is printed (pytest -s), not asserted on"""
    res = R.compare(got, ref, keys)
    print(f"fp64 {what}: " + " ".join(f"{k}={v[0]:.3f}" for k, v in res.items()))
    bad = {k: (round(v[0], 2), tuple(int(i) for i in v[1])) for k, v in res.items() if not v[0] <= 1.0}
    assert not bad, f"{what}: outside the fp64 bound (x bound, at index): {bad}"
    return res


# ------------------------------------------------------------------------------------------------------------------------------
# A. shallow stacks through the module API
# ------------------------------------------------------------------------------------------------------------------------------
def _module(spec, layers):
    """the models.* module of `spec` holding `layers`, its MLP and a call (x, aux) -> y"""
    from tinynerf_amd import _lib as L, models as m
    if spec.enc == "posenc":
        mod = m.VanillaFeatureMLP(spec.F, spec.hidden, spec.n_hidden)
        assert spec.out == spec.hidden
        assert np.array_equal(mod.encoding.freqs.numpy(), R.default_freqs(spec.F))
        mlp, call = mod.net, (lambda x, aux: mod(x))
    elif spec.enc == "dircat":
        mod = m.VanillaColorDecoder(spec.F, spec.in_dim, spec.hidden, spec.n_hidden)
        assert spec.out == 3 and spec.act == "sigmoid" and np.array_equal(mod.pe.freqs.numpy(), R.default_freqs(spec.F))
        mlp, call = mod.net, (lambda x, aux: mod(x, aux))
    elif spec.act == "exp_m1" and spec.n_hidden == 0 and spec.hidden == 64:
        mod = m.VanillaOpacityDecoder(spec.in_dim)
        mlp, call = mod.net, (lambda x, aux: mod(x))
    else:
        mod = m.MLP(spec.in_dim, spec.hidden, spec.n_hidden, spec.out)
        act = {"none": L.ACT_NONE, "exp_m1": L.ACT_EXP_M1, "sigmoid": L.ACT_SIGMOID}[spec.act]
        mlp, call = mod, (lambda x, aux: mod.fused(x, None, L.ENC_NONE, 0, act))
    ps = mlp.params()
    assert len(ps) == 2 * len(layers)
    with torch.no_grad():
        for (W, b), pw, pb in zip(layers, ps[0::2], ps[1::2]):
            assert tuple(pw.shape) == W.shape
            pw.copy_(torch.from_numpy(W)); pb.copy_(torch.from_numpy(b))
    mod.to(DEV)
    return mod, mlp, call


def _train_step(mlp, call, fx):
    x = cu(fx.x).requires_grad_(fx.spec.enc != "posenc")
    aux = cu(fx.aux)
    for p in mlp.params():
        p.grad = None
    y = call(x, aux)
    y.backward(cu(fx.grad_y))
    ps = mlp.params()
    return dict(y=y.detach().cpu().numpy(), grad_x=None if x.grad is None else x.grad.cpu().numpy(),
                dW=[p.grad.cpu().numpy() for p in ps[0::2]], db=[p.grad.cpu().numpy() for p in ps[1::2]])


def _shallow(name, n, mode, monkeypatch):
    from tinynerf_amd import models as m
    spec = R.PART_A[name][0]
    fx = _fixture(name, spec, n)
    assert fx.rejected <= R.REJECTION_CAP
    ref = _reference(name, fx, mode)
    mod, mlp, call = _module(spec, fx.layers)
    # the cross-layer persistent launches (default) and one launch per layer (TN_MLP_LAYERWISE): the flag only exists for f16x2 stacks
    forms = (False, True) if (mode == "f16x2" and spec.hidden >= 128) else (False,)
    for layerwise in forms:
        monkeypatch.setattr(m._FusedMLP, "layerwise_training", layerwise)
        monkeypatch.setattr(m._FusedMLP, "layerwise_inference", layerwise)
        for stash in (True, False):
            monkeypatch.setattr(m._FusedMLP, "stash_forward", stash)
            got = _train_step(mlp, call, fx)
            _hold(got, ref, f"A {name} n={n} {mode} {'layerwise' if layerwise else 'default'} stash={int(stash)}")
        with torch.no_grad():                                       # the inference forward (tn_mlp_fwd / tn_mlp_fwd_ws)
            y = call(cu(fx.x), cu(fx.aux)).cpu().numpy()
        _hold(dict(y=y), ref, f"A {name} n={n} {mode} {'layerwise' if layerwise else 'default'} inference", keys=("y",))


_HEADS_A = [(k, n) for k, (s, f) in sorted(R.PART_A.items()) if f == "heads" for n in _sizes(s)]
_WIDE_A = [(k, n) for k, (s, f) in sorted(R.PART_A.items()) if f == "matmul" for n in _sizes(s)]


@pytest.mark.parametrize("name,n", _HEADS_A)
def test_shallow_width64_within_fp64_bound(name, n, heads, monkeypatch):
    _shallow(name, n, heads, monkeypatch)


@pytest.mark.parametrize("name,n", _WIDE_A)
def test_shallow_wide_within_fp64_bound(name, n, matmul, monkeypatch):
    _shallow(name, n, matmul, monkeypatch)


# ------------------------------------------------------------------------------------------------------------------------------
# B. production-depth stacks, sparse upstream gradients
# ------------------------------------------------------------------------------------------------------------------------------
STACKS_B = {     # name: (spec, tolerance of the stack in test_hip_models.py: per tensor, of its largest element)
    "vanilla_256x10": (R.Spec("posenc", 3, 10, 256, 8, 256, "none"), 3e-5),      # 60 -> 256 x 9 -> 256 (run.py:131)
    "cobafa_128x6":   (R.Spec("none", 36, 0, 128, 5, 128, "none"), 3e-5),        # 36 -> 128 x 6 -> 128 (run.py:141-147)
    "sigma_head":     (R.Spec("none", 96, 0, 64, 0, 1, "exp_m1"), 2e-5),
    "colour_head":    (R.Spec("dircat", 96, 8, 64, 3, 3, "sigmoid"), 2e-5),
}
RAGGED = 40037
ROUND_NW8 = 256 * 8 * 32                    # samples per round of the cross-layer launches with 8 waves per workgroup (see the docstring)
RAGGED_NW8 = ROUND_NW8 + 37


def _probes(n, width, edge=SECOND_ROUND - 1):
    """at most eight probe samples: 0; 31 and 32 (the first tile edge); the last sample before and the first sample of the second
    round (8191 / 8192: the one-tile-per-workgroup launches on 256 workgroups; widths 128 and 256 also 16384: the f16x2 / bf16x3 weight-gradient
    launches on 512 workgroups and the width-128 layer kernels' two tile streams); n - 33; n - 1.  `edge`: the first sample of the second
    round where it is another launch's (65536: the cross-layer launches with 8 waves; 8191 / 8192 are left to the sizes that have them)"""
    p = {0, 31, 32, edge - 1, edge, n - 33, n - 1}
    if width >= 128:
        p.add(2 * (SECOND_ROUND - 1))
    p = sorted(q for q in p if 0 <= q < n)
    assert 1 <= len(p) <= 8
    return p


def _abi_backward(spec, params, freqs, x, aux, gy, stash, extra_flags=0):
    """tn_mlp_fwd_stash (stash) + tn_mlp_bwd through the C ABI, as models._FusedMLP drives them, with grad_x prefilled with NaN:
    -> (gradients [w0, b0, w1, ...], grad_x or None)"""
    from tinynerf_amd import _lib as L
    from tinynerf_amd.models import _mlp_desc
    dev = x.device
    n = x.size(0)
    enc = {"none": L.ENC_NONE, "posenc": L.ENC_POSENC, "dircat": L.ENC_DIR_CAT}[spec.enc]
    act = {"none": L.ACT_NONE, "exp_m1": L.ACT_EXP_M1, "sigmoid": L.ACT_SIGMOID}[spec.act]
    d = _mlp_desc(params, x.size(1), enc, spec.F, act, freqs, extra_flags)
    fn = L.lib().tn_mlp_bwd_workspace_bytes
    fn.restype = C.c_int64
    nb = int(fn(C.byref(d), C.c_int64(n)))
    assert nb > 0, f"{spec}: no backward workspace, so stash on / off would be the same launches"
    ws = torch.full((nb // 4,), float("nan"), device=dev)
    if stash:
        y = torch.empty(n, spec.out, device=dev)
        L.call("tn_mlp_fwd_stash", dev, C.byref(d), L.ptr(x), L.ptr(aux), C.c_int64(n), L.ptr(y), L.ptr(ws), C.c_int64(nb))
        d.flags |= L.MLP_STASHED
    gs = [torch.zeros_like(p) for p in params]
    k = len(params) // 2
    gw = (C.c_void_p * k)(*[g.data_ptr() for g in gs[0::2]])
    gb = (C.c_void_p * k)(*[g.data_ptr() for g in gs[1::2]])
    gx = None if spec.enc == "posenc" else torch.full((n, x.size(1)), float("nan"), device=dev)
    L.call("tn_mlp_bwd", dev, C.byref(d), L.ptr(x), L.ptr(aux), L.ptr(gy), C.c_int64(n), gw, gb, L.ptr(gx), L.ptr(ws), C.c_int64(nb))
    return gs, gx


_TP = {}


def _cached(key, fn):
    """compute_ref for tests/_ties.py whose unforced evaluation (and the tie units it recorded) runs once per key"""
    from oracle import torch_port as tp

    def run():
        ctrl = tp.ReluControl.current
        plain = ctrl is not None and not ctrl.force
        if plain and key in _TP:
            res, found, state = _TP[key]
            ctrl.found.extend(found); ctrl.state.update(state)
            return res
        res = fn()
        if plain:
            _TP[key] = (res, list(ctrl.found), dict(ctrl.state))
        return res
    return run


def _port_grads(spec, layers, freqs, x, aux, gy):
    """the fp32 network through oracle/torch_port.mlp with torch ops on the device (rocBLAS), autograd: {dW*, db*, x}"""
    from oracle import torch_port as tp

    def run():
        sd = {}
        for i, (W, b) in enumerate(layers):
            sd[f"net.{i}.weight"] = cu(W).requires_grad_(True)
            sd[f"net.{i}.bias"] = cu(b).requires_grad_(True)
        xl = x.detach().clone().requires_grad_(spec.enc != "posenc")
        if spec.enc == "none":
            inp = xl
        elif spec.enc == "posenc":
            inp = tp.posenc(xl, freqs)
        else:
            inp = torch.cat([tp.posenc(aux, freqs), aux, xl], -1)
        v = tp.mlp(sd, "net.", inp)
        yy = {"none": lambda t: t, "sigmoid": torch.sigmoid, "exp_m1": lambda t: tp._TruncExp.apply(t - 1.)}[spec.act](v)
        yy.backward(gy)
        out = {}
        for i in range(len(layers)):
            out[f"dW{i}"] = sd[f"net.{i}.weight"].grad.cpu().numpy()
            out[f"db{i}"] = sd[f"net.{i}.bias"].grad.cpu().numpy()
        if xl.grad is not None:
            out["x"] = xl.grad.cpu().numpy()
        return out
    return run


def _got(gs, gx_rows):
    out = {}
    for i in range(len(gs) // 2):
        out[f"dW{i}"], out[f"db{i}"] = gs[2 * i].cpu().numpy(), gs[2 * i + 1].cpu().numpy()
    if gx_rows is not None:
        out["x"] = gx_rows.cpu().numpy()
    return out


def _deep(name, n, mode):
    from _ties import assert_grads_match_up_to_relu_ties
    from tinynerf_amd import _lib as L
    spec, rel = STACKS_B[name]
    fx = _fixture("B:" + name, spec, n, reject=False)
    probes = _probes(n, spec.hidden, ROUND_NW8 if n > ROUND_NW8 else SECOND_ROUND - 1)
    pt = torch.tensor(probes, device=DEV)
    others = torch.ones(n, dtype=torch.bool, device=DEV)
    others[pt] = False
    params = [cu(t) for wb in fx.layers for t in wb]
    x, aux, freqs = cu(fx.x), cu(fx.aux), cu(fx.freqs)
    gy_dense = cu(fx.grad_y)
    gy_sparse = torch.zeros_like(gy_dense)
    gy_sparse[pt] = gy_dense[pt]
    gy_scaled = gy_dense.clone()
    gy_scaled[pt] *= 4096.0
    # sparse: the parameter gradients are sums over the probe samples alone, so the reference evaluates only those rows
    ref_sparse = _cached((name, n, "sparse"), _port_grads(spec, fx.layers, freqs, x[pt], None if aux is None else aux[pt], gy_sparse[pt]))
    ref_scaled = _cached((name, n, "scaled"), _port_grads(spec, fx.layers, freqs, x, aux, gy_scaled))
    forms = (0, L.MLP_LAYERWISE) if (mode == "f16x2" and spec.hidden >= 128) else (0,)
    for flags in forms:
        for stash in (True, False):
            what = f"B {name} n={n} {mode} flags={flags} stash={int(stash)}"
            gs, gx = _abi_backward(spec, params, freqs, x, aux, gy_sparse, stash, flags)
            if gx is not None:
                stray = gx[others]
                assert bool((stray == 0).all()), f"{what}: grad_x is not exactly zero on {int((~(stray == 0)).any(1).sum())} samples without an upstream gradient"
            for g in gs:
                assert bool(torch.isfinite(g).all()), what
            flips = assert_grads_match_up_to_relu_ties(_got(gs, None if gx is None else gx[pt]), ref_sparse, rel)
            gs, gx = _abi_backward(spec, params, freqs, x, aux, gy_scaled, stash, flags)
            flips2 = assert_grads_match_up_to_relu_ties(_got(gs, gx), ref_scaled, rel)
            print(f"{what}: {len(probes)} probes, tie units flipped: sparse {flips}, dense {flips2}")


_WIDE_B = [(k, n) for k in ("vanilla_256x10", "cobafa_128x6") for n in _sizes(STACKS_B[k][0], (RAGGED,))] + [("cobafa_128x6", RAGGED_NW8)]
_HEADS_B = [(k, n) for k in ("sigma_head", "colour_head") for n in _sizes(STACKS_B[k][0], (RAGGED,))]


@pytest.mark.parametrize("name,n", _WIDE_B)
def test_deep_wide_stack_sparse_upstream(name, n, matmul):
    _deep(name, n, matmul)


@pytest.mark.parametrize("name,n", _HEADS_B)
def test_deep_head_sparse_upstream(name, n, heads):
    _deep(name, n, heads)


def test_cobafa_inference_second_round_of_the_eight_wave_launch(monkeypatch):
    """The inference forward of cobafa_128x6 in f16x2 mode at 65573 samples: fused_fwd_kernel<128, false> (8 waves per workgroup, 256
    workgroups) opens its second round at sample 65536, with two tiles, the last one ragged.  Through tn_mlp_fwd_ws -- the entry that runs
    the cross-layer launch, as models._FusedMLP calls it -- and through tn_mlp_fwd (the register-resident kernel of mlp.hip), each into a
    NaN-prefilled y: every element finite, and y within the stack's 3e-5 of its largest element of oracle/torch_port.mlp on the device."""
    from oracle import torch_port as tp
    from tinynerf_amd import _lib as L, models as m
    monkeypatch.setattr(m, "MATMUL", "f16x2")
    name, n = "cobafa_128x6", RAGGED_NW8
    spec, rel = STACKS_B[name]
    fx = _fixture("B:" + name, spec, n, reject=False)
    params = [cu(t) for wb in fx.layers for t in wb]
    x = cu(fx.x)
    with torch.no_grad():
        ref = tp.mlp({f"net.{i}.{k}": t for i in range(len(fx.layers)) for k, t in (("weight", params[2 * i]), ("bias", params[2 * i + 1]))},
                     "net.", x)
    top = float(ref.abs().max())
    d = m._mlp_desc(params, x.size(1), L.ENC_NONE, 0, L.ACT_NONE, None)
    assert d.flags & L.MLP_F16X2
    fn = L.lib().tn_mlp_fwd_workspace_bytes
    fn.restype = C.c_int64
    nb = int(fn(C.byref(d), C.c_int64(n)))
    assert nb > 0, "no workspace form: tn_mlp_fwd_ws would not run the cross-layer launch"
    ws = torch.full((nb // 4,), float("nan"), device=DEV)
    for entry in ("tn_mlp_fwd_ws", "tn_mlp_fwd"):
        y = torch.full((n, spec.out), float("nan"), device=DEV)
        if entry == "tn_mlp_fwd_ws":
            L.call(entry, x.device, C.byref(d), L.ptr(x), C.c_void_p(None), C.c_int64(n), L.ptr(y), L.ptr(ws), C.c_int64(nb))
        else:
            L.call(entry, x.device, C.byref(d), L.ptr(x), C.c_void_p(None), C.c_int64(n), L.ptr(y), C.c_void_p(None))
        assert bool(torch.isfinite(y).all()), f"{entry}: {int((~torch.isfinite(y)).any(1).sum())} samples of y are not finite"
        err = float((y - ref).abs().max())
        print(f"{entry} {name} n={n} f16x2: max |y - port| = {err:.3e} = {err / top:.3e} of the largest element {top:.4f}")
        assert err <= rel * top, f"{entry}: {err / top:.3e} of the largest element, allowed {rel:.0e}"


# ------------------------------------------------------------------------------------------------------------------------------
# the pair of heads on one feature tensor: tn_mlp_fwd_stash_pair / tn_mlp_bwd_pair, lean and stashed
# ------------------------------------------------------------------------------------------------------------------------------
def _pair(sp_c, sp_s, lay_c, lay_s, freqs, x, table, ray_ids, g_rgb, g_sig, lean):
    from tinynerf_amd import _lib as L
    from tinynerf_amd.models import _mlp_desc
    dev, n, F = x.device, x.size(0), x.size(1)
    rp = [cu(t) for wb in lay_c for t in wb]
    sp = [cu(t) for wb in lay_s for t in wb]
    fn = L.lib().tn_mlp_bwd_workspace_bytes
    fn.restype = C.c_int64
    flags = L.MLP_LEAN if lean else 0
    rd = _mlp_desc(rp, F, L.ENC_AUX_CAT, sp_c.F, L.ACT_SIGMOID, freqs, flags, ray_ids, table.size(1))
    sd = _mlp_desc(sp, F, L.ENC_NONE, 0, L.ACT_EXP_M1, None, flags, None, 0)
    if lean:
        assert L.lib().tn_mlp_lean_supported(C.byref(rd), C.byref(sd)) == 1
    nbr, nbs = int(fn(C.byref(rd), C.c_int64(n))), int(fn(C.byref(sd), C.c_int64(n)))
    wr, wsg = torch.full((nbr // 4,), float("nan"), device=dev), torch.full((nbs // 4,), float("nan"), device=dev)
    rgb, sigma = torch.empty(n, 3, device=dev), torch.empty(n, 1, device=dev)
    L.call("tn_mlp_fwd_stash_pair", dev, C.byref(rd), C.byref(sd), L.ptr(x), L.ptr(table), C.c_int64(n), L.ptr(rgb), L.ptr(sigma),
           L.ptr(wr), C.c_int64(nbr), L.ptr(wsg), C.c_int64(nbs))
    rd.flags |= L.MLP_STASHED
    sd.flags |= L.MLP_STASHED

    def backward(g_rgb, g_sig):
        grs, gss = [torch.zeros_like(p) for p in rp], [torch.zeros_like(p) for p in sp]
        arr = lambda gs, o: (C.c_void_p * (len(gs) // 2))(*[g.data_ptr() for g in gs[o::2]])
        gx = torch.full((n, F), float("nan"), device=dev)
        w1, w2 = wr.clone(), wsg.clone()            # the chain writes its G rows into the workspaces: every backward gets the forward's own
        L.call("tn_mlp_bwd_pair", dev, C.byref(rd), C.byref(sd), L.ptr(x), L.ptr(table), L.ptr(g_rgb), L.ptr(g_sig), C.c_int64(n),
               arr(grs, 0), arr(grs, 1), arr(gss, 0), arr(gss, 1), L.ptr(gx), L.ptr(w1), C.c_int64(nbr), L.ptr(w2), C.c_int64(nbs))
        torch.cuda.synchronize()                    # (w1 / w2 stay alive until the launches are done)
        return grs, gss, gx
    return rgb, sigma, backward


@pytest.mark.parametrize("n", SIZES + (RAGGED,))
def test_pair_heads_forward_bound_and_sparse_backward(n, heads):
    """The K-Planes heads (colour 147 -> 64 x 4 -> 3 through the per-ray table, sigma 96 -> 64 -> 1) on one x.  Forward: both outputs
    inside the fp64 bound (it needs no tie-free samples), stashed and -- under f16x2 -- lean.  Backward (tn_mlp_bwd_pair): sparse upstream
    gradients on the probe samples, grad_x = the SUM of the two heads' exactly zero elsewhere, everything against the sum of the references
    up to tie units at the heads' 2e-5; then dense with the probes scaled by 2^12."""
    from _ties import assert_grads_match_up_to_relu_ties
    from oracle import torch_port as tp
    from tinynerf_amd import _lib as L
    sp_c, sp_s = STACKS_B["colour_head"][0], STACKS_B["sigma_head"][0]
    fc = _fixture("B:colour_head", sp_c, n, reject=False)
    lay_s = R.make_layers(sp_s, SEED + 1)
    dev = torch.device(DEV)
    x, dirs, freqs = cu(fc.x), cu(fc.aux), cu(fc.freqs)
    ray_ids = torch.arange(n, dtype=torch.int32, device=dev)              # every sample its own ray: the table holds each sample's PE(d), d
    table = torch.full((n, 56), float("nan"), device=dev)
    L.call("tn_dir_encode", dev, L.ptr(dirs), C.c_int64(n), L.ptr(freqs), C.c_int(sp_c.F), L.ptr(table), C.c_int(56))
    g_rgb = cu(fc.grad_y)
    g_sig = cu(np.random.default_rng(SEED + 2).standard_normal((n, 1)).astype(np.float32))
    probes = _probes(n, 64)
    pt = torch.tensor(probes, device=dev)
    others = torch.ones(n, dtype=torch.bool, device=dev)
    others[pt] = False

    def upstream(kind):
        if kind == "sparse":
            a, b = torch.zeros_like(g_rgb), torch.zeros_like(g_sig)
            a[pt], b[pt] = g_rgb[pt], g_sig[pt]
        else:
            a, b = g_rgb.clone(), g_sig.clone()
            a[pt] *= 4096.0; b[pt] *= 4096.0
        return a, b

    def port(rows, a, b):
        def run():
            sd = {}
            for pre, lay in (("c.", fc.layers), ("s.", lay_s)):
                for i, (W, bb) in enumerate(lay):
                    sd[f"{pre}{i}.weight"] = cu(W).requires_grad_(True)
                    sd[f"{pre}{i}.bias"] = cu(bb).requires_grad_(True)
            xl = x[rows].clone().requires_grad_(True)
            dd = dirs[rows]
            co = torch.sigmoid(tp.mlp(sd, "c.", torch.cat([tp.posenc(dd, freqs), dd, xl], -1)))
            so = tp._TruncExp.apply(tp.mlp(sd, "s.", xl) - 1.)
            ((co * a[rows]).sum() + (so * b[rows]).sum()).backward()
            return {"x": xl.grad.cpu().numpy(), **{k: v.grad.cpu().numpy() for k, v in sd.items()}}
        return run

    def got(grs, gss, gx_rows):
        out = {"x": gx_rows.cpu().numpy()}
        for pre, gs in (("c.", grs), ("s.", gss)):
            for i in range(len(gs) // 2):
                out[f"{pre}{i}.weight"], out[f"{pre}{i}.bias"] = gs[2 * i].cpu().numpy(), gs[2 * i + 1].cpu().numpy()
        return out
    c_mode = R.C_MODE[heads]
    ref_c = R.forward(sp_c, fc.layers, fc.x, fc.aux, fc.freqs, c_mode)
    ref_s = R.forward(sp_s, lay_s, fc.x, None, None, c_mode)
    everything = slice(None)
    for lean in ((False, True) if heads == "f16x2" else (False,)):
        what = f"pair n={n} {heads} lean={int(lean)}"
        rgb, sigma, backward = _pair(sp_c, sp_s, fc.layers, lay_s, freqs, x, table, ray_ids, g_rgb, g_sig, lean)
        _hold(dict(y=rgb.cpu().numpy()), ref_c, what + " colour", keys=("y",))
        _hold(dict(y=sigma.cpu().numpy()), ref_s, what + " sigma", keys=("y",))
        a, b = upstream("sparse")
        grs, gss, gx = backward(a, b)
        stray = gx[others]
        assert bool((stray == 0).all()), f"{what}: grad_x is not exactly zero on {int((~(stray == 0)).any(1).sum())} samples without an upstream gradient"
        f1 = assert_grads_match_up_to_relu_ties(got(grs, gss, gx[pt]), _cached(("pair", n, "sparse"), port(pt, a, b)), 2e-5)
        a, b = upstream("scaled")
        grs, gss, gx = backward(a, b)
        f2 = assert_grads_match_up_to_relu_ties(got(grs, gss, gx), _cached(("pair", n, "scaled"), port(everything, a, b)), 2e-5)
        print(f"{what}: {len(probes)} probes, tie units flipped: sparse {f1}, dense {f2}")


# ------------------------------------------------------------------------------------------------------------------------------
# renderer level: the probes through the row handoff and the merged last layer
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["vanilla", "cobafa"])
def test_renderer_upstream_on_three_rays(method, heads):
    """tests/test_hip_rows._renderer with fused = True and the arena set up as run.Trainer does (row views between the wide stack and the
    heads and, under f16x2, the stack's output as rows only with its last layer merged into the heads' first layers: asserted on the link);
    after a warm-up step the upstream gradient is nonzero on three rays only: the first, the last and the one that holds sample 32.  Against the CPU port of the reference up to tie units, tolerances of test_hip_rows.py."""
    from _ties import assert_grads_match_up_to_relu_ties
    from oracle import torch_port as tp
    from test_hip_rows import _batch, _renderer
    from tinynerf_amd import models as m
    from tinynerf_amd.arena import Arena
    packed, info, _ = _batch(61, 40, 5)
    n_rays = info.size(0)
    start = info[:, 0].cpu().numpy().astype(np.int64)
    count = info[:, 1].cpu().numpy().astype(np.int64)
    holds32 = int(np.nonzero((start <= 32) & (32 < start + count))[0][0])
    rays = sorted({0, holds32, n_rays - 1})
    assert len(rays) == 3 and all(count[q] > 0 for q in rays)
    up = torch.zeros(n_rays, 3, device=DEV)
    up[rays] = torch.randn(3, 3, generator=torch.Generator().manual_seed(7)).to(DEV)
    r = _renderer(method, 21)
    r.fused = True
    for p in r.parameters():                                         # run.Trainer: gradient buffers, accumulation into them, the arena
        p.grad = torch.zeros_like(p)
    r.accumulate_into_grad = r.reuse_buffers = True
    arena = Arena()
    for i, mod in enumerate(mm for mm in r.feature_module.modules() if isinstance(mm, m.MLP)):
        mod.__dict__["scratch"] = (arena, f"mlp_ws{i}", {}, True, {})
    if method == "cobafa":
        r.feature_module.__dict__["accumulate_into_grad"] = True
    stacks = [mm for mm in r.feature_module.modules() if isinstance(mm, m.MLP)]
    assert len(stacks) == 1
    # a renderer's FIRST step only finds out which stack's rows the render node reads (fused.render sets _rows_producer at its end); the
    # rows-only handoff and the merged last layer (TN_MLP_ROWS_ONLY | TN_MLP_SKIP_LAST, tn_linear_merge_*) run from the second step on.
    # So: a warm-up step with a dense upstream gradient, the gradient buffers zeroed again, then the probed step.
    warm = r(packed, info)
    warm.backward(torch.randn(n_rays, 3, generator=torch.Generator().manual_seed(8)).to(DEV))
    assert r.__dict__.get("_rows_producer") is stacks[0]
    for p in r.parameters():
        p.grad.zero_()
    out = r(packed, info)
    link = stacks[0].__dict__["scratch"][2]
    assert link.get("n") == packed.size(0) and link["width"] == (256 if method == "vanilla" else 128)
    if heads == "f16x2":
        assert link.get("rows_only") is True and link.get("skipped_last") is True, dict(link)
    else:
        assert not link.get("rows_only") and not link.get("skipped_last")
    out.backward(up)
    assert link["delivered"] is False                                # d loss / d rows was consumed by the stack's backward
    grads = {k: p.grad.detach().cpu().numpy() for k, p in r.named_parameters()}
    sd = {k: v.detach().cpu().contiguous() for k, v in _renderer(method, 21).state_dict().items()}
    pk, inf_, upc = packed.cpu(), info.cpu(), up.cpu()
    kw = {"vanilla_freqs": 10} if method == "vanilla" else {"cobafa_freqs": (2.0, 3.5, 8.0)}

    def ref():
        return tp.grads_of(sd, lambda p: (tp.render(p, pk, inf_, torch.ones(3), **kw) * upc).sum())[0]
    rel = {k: (1e-4 if k.startswith("feature_module.net") else 2e-5) for k in grads}
    assert_grads_match_up_to_relu_ties(grads, ref, rel, weights_conditioning=True, cond_cap=2e-3)
