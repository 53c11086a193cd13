"""The explicit K-Planes decoders' product stage, the stand-alone encoders and the ray tables against their fp64 definition
(tests/_decoders_ref.py; tests/test_decoders_ref.py shows on the CPU that it is right and sharp), per element, through the C ABI.

A  tn_basis_dot_fwd / _bwd: error / bound <= 1 per element on the general fixtures (pre-activations in about [-8, 8], all four
   activations), bit equality on the exact ones, over _decoders_ref.cases() -- idle lanes, ragged lane-stride trips, K = 1..4, the
   persistent loop's second and third trip; the clamp rows; grad_basis = NULL; accumulate_f; sentinels behind every output, inputs from
   the middle of a NaN-filled allocation; models._BasisDot / truncated_exp return the ABI's bits.
B  tn_posenc_fwd, tn_dir_encode within E_SINCOS (exact columns for equality), tn_ray_aux for equality.
C  NerfRenderer over the explicit decoders (its module-by-module path) against oracle/torch_port.render(explicit=True).

Every case prints its worst error / bound.  The bounds rest on tests/_mlp_ref.py's ASSUMPTION of 2 ulp for the device sinf / cosf / expf.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _decoders_ref as dr
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 3                      # sentinel rows behind every output, NaN rows around every input
SENT = -7777.25


def _L():
    from tinynerf_amd import _lib
    return _lib


def _inside(a: np.ndarray):
    """a [n, ...] -> (view of rows PAD .. PAD + n of a NaN-filled device allocation, the allocation)"""
    n = a.shape[0]
    whole = torch.full((n + 2 * PAD,) + a.shape[1:], float("nan"), device=DEV)
    whole[PAD:PAD + n] = torch.from_numpy(np.ascontiguousarray(a))
    return whole[PAD:PAD + n], whole


def _outbuf(n: int, shape, fill):
    """[n + PAD, *shape]: rows < n hold `fill` (a number or an [n, *shape] array), the PAD rows behind them the sentinel"""
    t = torch.full((n + PAD,) + tuple(shape), SENT, device=DEV)
    t[:n] = torch.from_numpy(fill) if isinstance(fill, np.ndarray) else fill
    return t


def _take(t: torch.Tensor, n: int, name: str) -> np.ndarray:
    a = t.cpu().numpy()
    assert np.all(a[n:] == SENT), f"{name}: written behind its last row"
    return a[:n].copy()


def run_abi(fx: dr.Fixture):
    """forward; backward with grad_basis into a NaN-prefilled grad_f; backward without grad_basis; accumulating backward from fx.prefill
    -> {out, grad_basis, grad_f, grad_f_null, grad_f_acc} (numpy)"""
    L = _L()
    n, K, Cc = fx.basis.shape
    act = dr.ACTS[fx.act]
    (f, _kf), (b, _kb), (g, _kg) = _inside(fx.f), _inside(fx.basis), _inside(fx.grad_out)
    dims = (C.c_int64(n), C.c_int32(Cc), C.c_int32(K), C.c_int32(act))
    out = _outbuf(n, (K,), float("nan"))
    L.call("tn_basis_dot_fwd", f.device, L.ptr(f), L.ptr(b), *dims, L.ptr(out))
    nan = float("nan")
    gf, gb = _outbuf(n, (Cc,), nan), _outbuf(n, (K, Cc), nan)                    # accumulate_f = 0 must ignore what grad_f holds
    L.call("tn_basis_dot_bwd", f.device, L.ptr(f), L.ptr(b), L.ptr(g), *dims, L.ptr(gf), L.ptr(gb), C.c_int32(0))
    gf0 = _outbuf(n, (Cc,), nan)
    L.call("tn_basis_dot_bwd", f.device, L.ptr(f), L.ptr(b), L.ptr(g), *dims, L.ptr(gf0), C.c_void_p(None), C.c_int32(0))
    gfa = _outbuf(n, (Cc,), fx.prefill)
    where = gfa.data_ptr()
    L.call("tn_basis_dot_bwd", f.device, L.ptr(f), L.ptr(b), L.ptr(g), *dims, L.ptr(gfa), C.c_void_p(None), C.c_int32(1))
    torch.cuda.synchronize()
    assert gfa.data_ptr() == where
    for name, (view, whole) in (("f", (f, _kf)), ("basis", (b, _kb)), ("grad_out", (g, _kg))):      # inputs are inputs
        w = whole.cpu().numpy()
        assert np.isnan(w[:PAD]).all() and np.isnan(w[PAD + n:]).all(), name
    return dict(out=_take(out, n, "out"), grad_basis=_take(gb, n, "grad_basis"), grad_f=_take(gf, n, "grad_f"),
                grad_f_null=_take(gf0, n, "grad_f (grad_basis = NULL)"), grad_f_acc=_take(gfa, n, "grad_f (accumulate_f)"))


# ------------------------------------------------------------------------------------------------ A. basis_dot
@pytest.mark.parametrize("n,Cc,K,act", dr.cases())
def test_basis_dot_general_vs_fp64(n, Cc, K, act):
    fx = dr.general_fixture(n, Cc, K, act, dr.case_seed(n, Cc, K))
    got = run_abi(fx)
    ref = dr.reference(fx.f, fx.basis, act, fx.grad_out, fx.prefill)
    worst = dr.ratios(got, ref)
    print(f"basis_dot general n {n} C {Cc} K {K} {act}: worst error / bound " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    assert np.array_equal(got["grad_f_null"].view(np.uint32), got["grad_f"].view(np.uint32)), "grad_basis = NULL changed grad_f"
    assert set(worst) == {"out", "grad_basis", "grad_f", "grad_f_acc"} and max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("n,Cc,K", sorted({c[:3] for c in dr.cases()}))
def test_basis_dot_exact_bit_for_bit(n, Cc, K):
    fx = dr.exact_fixture(n, Cc, K, dr.case_seed(n, Cc, K))
    got = run_abi(fx)
    ref = dr.reference(fx.f, fx.basis, "none", fx.grad_out, fx.prefill)
    dr.assert_exact(ref["out"], ref["A_out"], "out")
    dr.assert_exact(ref["grad_f"], ref["A_grad_f"], "grad_f")
    dr.assert_exact(ref["grad_f_acc"], ref["A_grad_f_acc"], "grad_f_acc")
    dr.assert_exact(ref["grad_basis"], np.abs(ref["grad_basis"]), "grad_basis")
    ref["grad_f_null"] = ref["grad_f"]
    wrong = {k: int((got[k].astype(np.float64) != ref[k]).sum()) for k in got}
    print(f"basis_dot exact n {n} C {Cc} K {K}: elements that differ {wrong}")
    assert not any(wrong.values()), wrong


@pytest.mark.parametrize("act,at", [("exp_m1", "acc-1"), ("exp", "acc-1"), ("exp", "acc")])
def test_basis_dot_clamp_rows(act, at):
    """rows of 96 channels whose clamped quantity sits exactly at -40, -15.5, -15, 15, 15.5 and 20 (exp_m1: acc - 1; "the same rows"
    through exp; exp at its own edges): forward within the bound of exp(t), backward within the bound of g exp(clamp(t))"""
    fx = dr.clamp_fixture(act, at)
    got = run_abi(fx)
    ref = dr.reference(fx.f, fx.basis, act, fx.grad_out, fx.prefill)
    worst = dr.ratios(got, ref)
    print(f"basis_dot clamp rows {act} ({at} at the targets): worst error / bound " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    assert np.array_equal(got["grad_f_null"].view(np.uint32), got["grad_f"].view(np.uint32))
    assert len(worst) == 4 and max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("Cc,K,act", dr.REAL)
@pytest.mark.parametrize("basis_grad", [True, False])
def test_basis_dot_module_gives_the_abi_bits(Cc, K, act, basis_grad):
    from tinynerf_amd import models as m
    n = 8193
    fx = dr.general_fixture(n, Cc, K, act, dr.case_seed(n, Cc, K))
    want = run_abi(fx)
    f = torch.from_numpy(fx.f).to(DEV).requires_grad_(True)
    b = torch.from_numpy(fx.basis).to(DEV).requires_grad_(basis_grad)
    out = m._BasisDot.apply(f, b, K, dr.ACTS[act])
    out.backward(torch.from_numpy(fx.grad_out).to(DEV))
    assert out.shape == (n, K) and torch.equal(out.detach().cpu(), torch.from_numpy(want["out"]))
    assert torch.equal(f.grad.cpu(), torch.from_numpy(want["grad_f"]))
    if basis_grad:
        assert b.grad.shape == (n, K, Cc) and torch.equal(b.grad.cpu(), torch.from_numpy(want["grad_basis"]))
    else:
        assert b.grad is None


def test_truncated_exp_gives_the_abi_bits():
    from tinynerf_amd import models as m
    n = 8193
    x = np.random.default_rng(3).uniform(-20.0, 20.0, n).astype(np.float32)
    x[:6] = dr.CLAMP_TARGETS
    g = np.random.default_rng(4).standard_normal(n).astype(np.float32)
    fx = dr.Fixture(np.ones((n, 1), np.float32), x.reshape(n, 1, 1), g.reshape(n, 1), np.zeros((n, 1), np.float32), "exp")
    want = run_abi(fx)
    xt = torch.from_numpy(x).to(DEV).requires_grad_(True)
    y = m.truncated_exp(xt)
    y.backward(torch.from_numpy(g).to(DEV))
    assert torch.equal(y.detach().cpu(), torch.from_numpy(want["out"][:, 0]))
    assert torch.equal(xt.grad.cpu(), torch.from_numpy(want["grad_basis"][:, 0, 0]))
    ref = dr.reference(fx.f, fx.basis, "exp", fx.grad_out, fx.prefill)
    worst = dr.ratios(want, ref)
    print("truncated_exp (C = K = 1, x in [-20, 20]): worst error / bound " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


# ------------------------------------------------------------------------------------------------ B. encoders and ray tables
@pytest.mark.parametrize("Cc", [1, 3, 5])
@pytest.mark.parametrize("F", [1, 4, 10])
def test_posenc_vs_fp64(Cc, F):
    L = _L()
    worst = 0.0
    for n in (1, 255, 257, 4099):
        x, n_special = dr.posenc_x(n, Cc, 7 * n + Cc)
        xd, _keep = _inside(x)
        for freqs in (dr.default_freqs(F), None):
            fr = None if freqs is None else torch.from_numpy(freqs).to(DEV)
            out = _outbuf(n, (2 * F * Cc,), float("nan"))
            L.call("tn_posenc_fwd", xd.device, L.ptr(xd), C.c_int64(n), C.c_int(Cc), L.ptr(fr), C.c_int(F), L.ptr(out))
            got = _take(out, n, "posenc")
            ref, E = dr.posenc(x, freqs, F)
            ratio = np.where(np.isfinite(got), np.abs(got.astype(np.float64) - ref) / E, np.inf)
            worst = max(worst, float(ratio.max()))
            assert ratio.max() <= 1.0, (n, freqs is None, float(ratio.max()), np.unravel_index(int(ratio.argmax()), ratio.shape))
            if n_special:                                                        # x = 0: sin columns c 2F + f are 0, cos columns c 2F + F + f are 1
                zero = got[n - n_special].reshape(Cc, 2, F)
                assert np.all(zero[:, 0] == 0.0) and np.all(zero[:, 1] == 1.0)
    print(f"posenc C {Cc} F {F}: worst error / E_SINCOS {worst:.4f}")


def test_posenc_module_gives_the_abi_bits():
    from tinynerf_amd import models as m
    L = _L()
    F = 4
    x = (torch.rand(2, 3, 5, 3, generator=torch.Generator().manual_seed(0)) * 2 - 1).to(DEV)
    pe = m.PositionalEncoding(F).to(DEV)
    got = pe(x)
    flat = x.reshape(-1, 3).contiguous()
    out = torch.empty((30, 6 * F), device=DEV)
    L.call("tn_posenc_fwd", flat.device, L.ptr(flat), C.c_int64(30), C.c_int(3), L.ptr(pe.freqs), C.c_int(F), L.ptr(out))
    assert got.shape == (2, 3, 5, 6 * F) and torch.equal(got.reshape(30, -1), out)
    assert np.array_equal(pe.freqs.cpu().numpy(), dr.default_freqs(F))


@pytest.mark.parametrize("F", [1, 4, 8])
def test_dir_encode_vs_fp64(F):
    L = _L()
    worst = 0.0
    for si, stride in enumerate((6 * F + 3, 6 * F + 4, 56, 64)):
        for n in (1, 63, 65, 1000):
            d = np.random.default_rng(100 * F + n).standard_normal((n, 3))
            d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
            freqs = dr.default_freqs(F) if si % 2 == 0 else None
            fr = None if freqs is None else torch.from_numpy(freqs).to(DEV)
            dd, _keep = _inside(d)
            table = _outbuf(n, (stride,), float("nan"))
            L.call("tn_dir_encode", dd.device, L.ptr(dd), C.c_int64(n), L.ptr(fr), C.c_int(F), L.ptr(table), C.c_int(stride))
            got = _take(table, n, "dir_encode")
            ref, E = dr.dir_encode(d, freqs, F, stride)
            pe = slice(0, 6 * F)
            ratio = np.where(np.isfinite(got[:, pe]), np.abs(got[:, pe].astype(np.float64) - ref[:, pe]) / E[:, pe], np.inf)
            worst = max(worst, float(ratio.max()))
            assert ratio.max() <= 1.0, (stride, n, float(ratio.max()))
            assert np.array_equal(got[:, 6 * F:6 * F + 3].view(np.uint32), d.view(np.uint32)), (stride, n)       # the direction, bit for bit
            assert np.all(got[:, 6 * F + 3:].view(np.uint32) == 0), (stride, n)                                    # the pad: +0.0
    print(f"dir_encode F {F}: worst error / E_SINCOS {worst:.4f}")


def _ray_counts(R):
    base = [0, 1, 63, 0, 0, 64, 65, 300, 0]
    if R == 1:
        return np.array([300], np.int32)
    cnt = np.array([base[i % len(base)] for i in range(R)], np.int32)
    cnt[0] = cnt[-1] = 0                                                          # an empty ray first and last
    return cnt


@pytest.mark.parametrize("R", [1, 3, 4, 5, 1001])
def test_ray_aux_vs_definition(R):
    L = _L()
    cnt = _ray_counts(R)
    if R == 1001:
        assert set(cnt.tolist()) == {0, 1, 63, 64, 65, 300} and np.any((cnt[1:] == 0) & (cnt[:-1] == 0))
    info = np.stack([np.cumsum(cnt) - cnt, cnt], -1).astype(np.int32)
    N = int(cnt.sum())
    packed = np.random.default_rng(R).random((N, 7)).astype(np.float32)          # every sample its own direction: only the ray's FIRST is right
    pk, _keep = _inside(packed)
    ids = torch.full((N + 2 * PAD,), -5, dtype=torch.int32, device=DEV)
    steps = torch.full((N + 2 * PAD,), SENT, device=DEV)
    dirs = _outbuf(R, (3,), float("nan"))
    inf_d = torch.from_numpy(info).to(DEV)
    L.call("tn_ray_aux", pk.device, L.ptr(pk), L.ptr(inf_d), C.c_int64(R), L.ptr(ids[PAD:]), L.ptr(steps[PAD:]), L.ptr(dirs))
    want_ids, want_steps, want_dirs = dr.ray_aux(packed, info)
    ids, steps = ids.cpu().numpy(), steps.cpu().numpy()
    assert np.all(ids[:PAD] == -5) and np.all(ids[PAD + N:] == -5) and np.all(steps[:PAD] == SENT) and np.all(steps[PAD + N:] == SENT)
    assert np.array_equal(ids[PAD:PAD + N], want_ids) and np.array_equal(steps[PAD:PAD + N].view(np.uint32), want_steps.view(np.uint32))
    got_dirs = _take(dirs, R, "dirs")
    assert np.array_equal(got_dirs.view(np.uint32), want_dirs.view(np.uint32))
    assert np.all(got_dirs[cnt == 0].view(np.uint32) == 0)
    for r in np.nonzero(cnt > 0)[0]:
        assert np.array_equal(got_dirs[r], packed[info[r, 0], 3:6])


# ------------------------------------------------------------------------------------------------ C. the explicit decoders in a renderer
EXPLICIT_SEED = 0
SIGMA_BIAS_SHIFT = 0.33      # added to every element of the opacity decoder's bias: v = <f, W f + b> moves by 0.33 sum_c f_c ~ 0.33 * 12.1 = 4.0,
                             # which takes the seeded decoder's median density from 0.39 to 21 -- G9's own is 20.6 (CPU port, fp32)


def _explicit_renderer(g):
    from test_hip_renderer import build_renderer
    from tinynerf_amd import models as m
    r = build_renderer(g)
    torch.manual_seed(EXPLICIT_SEED)
    od, cd = m.KPlanesExplicitOpacityDecoder(96), m.KPlanesExplicitColorDecoder(96, 8, 128)
    with torch.no_grad():
        od.net.bias += SIGMA_BIAS_SHIFT
    r.sigma_decoder, r.rgb_decoder = od.to(DEV), cd.to(DEV)
    return r


def test_renderer_over_the_explicit_decoders_vs_the_port(matmul, monkeypatch):
    """NerfRenderer(KPlanesFeatureField, KPlanesExplicitOpacityDecoder(96), KPlanesExplicitColorDecoder(96, 8, 128)) -- the configuration of
    the reference's tests/test_models.py -- on G9's planes, batch, background and target, forward and backward, against
    oracle/torch_port.render(explicit=True).  Tolerances are test_renderer_forward_backward_vs_reference's on the same batch: TOL for the
    colours, 5e-5 of each gradient tensor's largest element or 4 x the port's own weights conditioning, under the same 4e-3 cap.
    Port-derived conditioning of this fixture (tp.weights_conditioning: _Weights.exact_backward + its three noise draws, CPU, nothing
    from the HIP result): sigma_decoder.net.bias 3.7e-4, net.weight 2.4e-4, the planes 5e-5 .. 1.1e-4, the basis MLP 0 (its gradient
    does not pass the weights backward) -- so the allowance 4 x that is 1.5e-3 at most, inside the existing 4e-3 cap (the Vanilla heads
    on the same batch: 3.6e-3).  The test prints each tensor's tolerance next to the distance actually found."""
    from _ties import assert_grads_match_up_to_relu_ties
    from oracle import torch_port as tp
    from test_hip_renderer import TOL, cu
    L = _L()
    g = load_golden("G9_renderer_kplanes")
    r = _explicit_renderer(g)
    calls = []
    orig = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), orig(name, *a))[1])
    packed, info = cu(g["packed"]), cu(g["info"], torch.int32)
    out = r(packed, info)
    loss = torch.nn.functional.mse_loss(out, cu(g["target"]))
    loss.backward()
    monkeypatch.setattr(L, "call", orig)
    assert "tn_basis_dot_fwd" in calls and "tn_basis_dot_bwd" in calls and "tn_linear_fwd" in calls, calls
    assert not [c for c in calls if c.startswith("tn_kplanes_mlp_")], calls          # the module path, not the fused node
    sd = {k: v.detach().cpu() for k, v in r.state_dict().items()}
    pk, inf_, bgc, tgt = torch.as_tensor(g["packed"]), torch.as_tensor(g["info"]), torch.as_tensor(g["bg"]), torch.as_tensor(g["target"])
    with torch.no_grad():
        want = tp.render(sd, pk, inf_, bgc, explicit=True)
        sig = tp.explicit_sigma(sd, tp.kplanes_features(sd, pk[:, :3]), "sigma_decoder.")
    print(f"explicit renderer ({matmul}): median density {float(sig.median()):.2f} (G9: {float(np.median(g['sigma'])):.2f})")
    assert 0.5 < float(sig.median()) / float(np.median(g["sigma"])) < 2.0
    assert out.shape == want.shape
    print(f"explicit renderer ({matmul}): worst colour error {float((out.detach().cpu() - want).abs().max()):.2e} (TOL {TOL:.0e})")
    np.testing.assert_allclose(out.detach().cpu().numpy(), want.numpy(), rtol=0, atol=TOL)
    np.testing.assert_allclose(loss.item(), float(torch.nn.functional.mse_loss(want, tgt)), rtol=1e-5)
    got = {name: p.grad.cpu().numpy() for name, p in r.named_parameters()}
    assert {"sigma_decoder.net.weight", "sigma_decoder.net.bias", "rgb_decoder.net.net.0.weight", "rgb_decoder.net.net.5.bias"} <= set(got)
    assert sum(k.startswith("feature_module.planes.") for k in got) == 9
    matched = {}
    flips = assert_grads_match_up_to_relu_ties(
        got, lambda: tp.grads_of(sd, lambda p: torch.nn.functional.mse_loss(tp.render(p, pk, inf_, bgc, explicit=True), tgt))[0], 5e-5,
        weights_conditioning=True, cond_cap=4e-3, matched=matched)
    rel = matched.pop("rel")
    used = {k: float(np.abs(got[k] - matched[k]).max() / max(float(np.abs(matched[k]).max()), 1e-30)) for k in got}
    print(f"explicit renderer ({matmul}): {flips} tie units flipped; tolerance (max of 5e-5 and 4 x the port's conditioning) / distance used, "
          "relative to each tensor's largest element:")
    for k in sorted(got):
        print(f"  {k}: {rel[k]:.1e} / {used[k]:.1e}")
