"""GPU: the wave-per-ray volume-rendering kernels of csrc/weights.hip against the fp64 yardstick of tests/_render_ref.py, on every
fixture of that module (chunk edges 63 / 64 / 65, the register and the streaming backward at 1024 / 1025, partial last blocks, gaps,
permuted rays, walls across the threshold on every edge, unbounded steps), with the per-element bounds derived there and nothing
excluded.  tests/test_render_ref.py shows on the CPU that an fp32 restatement of the kernels' order stays inside these bounds and
that each of eleven mutants of it does not.

  tn_weights_fwd / _gate      every fixture x thr in {1e-4, 1e-3, 0}: the zero set is the reference's, the rest inside the forward bound;
                              the gate rises iff some w_ref > 0 and is never lowered
  tn_weights_bwd              every fixture, w = the reference weights rounded to fp32
  tn_composite_fwd / _bwd     exact kind bit for bit (opacity included), general kind inside the bound, NaN colours at masked samples,
                              grad_rgbs / grad_weights NULL in turn
  tn_render_rays_fwd/_bwd/_dw against the yardstick directly; the forward also bit for bit against tn_composite_fwd on the weights it wrote
                              and tn_weights_fwd (the other equal-to-two-launches tests stay in test_hip_core / _distortion)
  tn_mse_grad / _gated        n in {1, 3, 255, 256, 257, 768, 131072, 131073}: grad bit for bit, sumsq inside its bound on top of a
                              non-zero start, scale_dev NULL and set, the gate at 1, 0, -1 and NaN

Largest err / bound per kernel, measured on an MI355X with EXPF_ULPS = 1 on the fixtures as they stand (each test prints its own
figure, the module prints the maxima at its end; LABNOTES 9.8 is the record of the run, in which the parent commit's library gave
the same figures in every row):
  tn_weights_fwd / _gate   0.755        tn_render_rays_fwd      0.496
  tn_weights_bwd           0.211        tn_render_rays_bwd      0.134
  tn_composite_fwd         0.293        tn_render_rays_bwd_dw   0.124
  tn_composite_bwd         0.573        tn_mse_grad(_gated)     0.091 (sumsq; grad bit for bit)
The exact composite kind, grad_rgbs and the MSE gradient matched bit for bit, and so did tn_render_rays_fwd with its two halves
(tn_composite_fwd on the weights it wrote, tn_weights_fwd on its inputs) on every fixture.  On the `singles` fixture expf's largest
error lay between 0.55 and 0.86 ulp (beyond the rounding of w, and with it); EXPF_ULPS stayed at 1 because every fixture passed
with it, not because of that figure.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _render_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32
WORST = {}


def _note(kernel, ratio):
    WORST[kernel] = max(WORST.get(kernel, 0.0), float(ratio))
    return ratio


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for kernel, ratio in sorted(WORST.items()):
        print(f"\nlargest err / bound, {kernel}: {ratio:.3f}", end="")
    print()


def _call(name, *args):
    from tinynerf_amd import _lib as L
    L.call(name, torch.device(DEV), *args)


def _ptr(t):
    from tinynerf_amd import _lib as L
    return L.ptr(t)


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _buf(*shape):
    """an output buffer prefilled with the sentinel, never of size 0 (an empty tensor has no address)"""
    shape = (max(shape[0], 1),) + tuple(shape[1:])
    return torch.full(shape, float(ref.SENTINEL), device=DEV)


def _np(t, n):
    return t.cpu().numpy()[:n]


def _sizes(fx):
    return C.c_int64(fx["n"]), C.c_int64(fx["R"])


class _Inputs:
    def __init__(self, fx):
        self.sig, self.step, self.info = _dev(fx["sig"]), _dev(fx["step"]), _dev(fx["info"], torch.int32)


# ------------------------------------------------------------------------------------------------ tn_weights_fwd / _gate
@pytest.mark.parametrize("thr", ref.THRESHOLDS)
@pytest.mark.parametrize("name", ref.FIXTURES)
def test_weights_fwd_against_fp64(name, thr):
    fx, r = ref.fixture(name), ref.forward_ref(name, thr)
    assert ref.danger_rays(r, fx["info"], thr) == []
    x = _Inputs(fx)
    n = fx["n"]
    w = _buf(n)
    _call("tn_weights_fwd", _ptr(x.sig), _ptr(x.step), _ptr(x.info), C.c_float(thr), _ptr(w), *_sizes(fx))
    got = _np(w, n)
    if n == 0:
        assert float(w[0]) == ref.SENTINEL
    ulps = ref.expf_ulps_single(fx["sig"], fx["step"], fx["info"], got)
    ratio = _note("tn_weights_fwd", ref.check_weights(got, r, fx["info"], f"{name} thr {thr} tn_weights_fwd"))
    print(f"{name} thr {thr}: tn_weights_fwd err / bound {ratio:.3f}"
          + ("" if ulps is None else f", largest expf error on its single-sample rays between {ulps[0]:.2f} and {ulps[1]:.2f} ulp"))
    if ulps is not None:
        _note("expf, single-sample rays: ulps left beyond the rounding of w", ulps[0])
        _note("expf, single-sample rays: ulps, the rounding of w included", ulps[1])
    want_gate = float((r["w"] > 0).any())
    for preset in (0.0, 1.0):
        w2, gate = _buf(n), torch.full((1,), preset, device=DEV)
        _call("tn_weights_fwd_gate", _ptr(x.sig), _ptr(x.step), _ptr(x.info), C.c_float(thr), _ptr(w2), _ptr(gate), *_sizes(fx))
        assert float(gate) == max(preset, want_gate), (name, thr, preset)
        ref.same_bits(_np(w2, n), got, f"{name} thr {thr} tn_weights_fwd_gate")


# ------------------------------------------------------------------------------------------------ tn_weights_bwd
@pytest.mark.parametrize("name", ref.FIXTURES)
def test_weights_bwd_against_fp64(name):
    fx = ref.fixture(name)
    x = _Inputs(fx)
    n = fx["n"]
    w = ref.forward_ref(name, 1e-4)["w"].astype(f32)
    gs = _buf(n)
    d_w, d_g = _dev(w), _dev(fx["g"])
    _call("tn_weights_bwd", _ptr(x.sig), _ptr(x.step), _ptr(x.info), _ptr(d_w), _ptr(d_g), _ptr(gs), *_sizes(fx))
    want, bound, _ = ref.weights_grad(fx["sig"], fx["step"], fx["info"], w, fx["g"])
    ratio = _note("tn_weights_bwd", ref.check_owned(_np(gs, n), want, bound, fx["info"], f"{name} tn_weights_bwd"))
    print(f"{name}: tn_weights_bwd err / bound {ratio:.3f}")


# ------------------------------------------------------------------------------------------------ tn_composite_fwd / _bwd
@pytest.mark.parametrize("with_bg", [True, False])
@pytest.mark.parametrize("kind", ["exact", "general"])
@pytest.mark.parametrize("name", ref.FIXTURES)
def test_composite_against_fp64(name, kind, with_bg):
    fx = ref.fixture(name)
    info, n, R = fx["info"], fx["n"], fx["R"]
    bg = ref.BG if with_bg else None
    if kind == "exact":
        w, go = fx["exact_w"], fx["exact_go"]
        rgb = ref.masked_rgb(fx["exact_rgb"], w)
    else:
        w, go = ref.forward_ref(name, 1e-4)["w"].astype(f32), fx["go"]
        rgb = ref.masked_rgb(fx["rgb"], w)
    own = ref.owned(info, n)
    assert n == 0 or np.isnan(rgb[own]).any() or not (w[own] == 0).any()
    d_rgb, d_w, d_info, d_bg, d_go = _dev(rgb), _dev(w), _dev(info, torch.int32), _dev(bg), _dev(go)
    out, opac = _buf(R, 3), _buf(R)
    _call("tn_composite_fwd", _ptr(d_rgb), _ptr(d_w), _ptr(d_info), _ptr(d_bg), _ptr(out), _ptr(opac), *_sizes(fx))
    out2 = _buf(R, 3)
    _call("tn_composite_fwd", _ptr(d_rgb), _ptr(d_w), _ptr(d_info), _ptr(d_bg), _ptr(out2), C.c_void_p(None), *_sizes(fx))
    assert torch.equal(out, out2)                           # the opacity output is optional
    grgb, gw = _buf(n, 3), _buf(n)
    _call("tn_composite_bwd", _ptr(d_rgb), _ptr(d_w), _ptr(d_info), _ptr(d_bg), _ptr(d_go), _ptr(grgb), _ptr(gw), *_sizes(fx))
    grgb2, gw2 = _buf(n, 3), _buf(n)
    _call("tn_composite_bwd", _ptr(d_rgb), _ptr(d_w), _ptr(d_info), _ptr(d_bg), _ptr(d_go), _ptr(grgb2), C.c_void_p(None), *_sizes(fx))
    _call("tn_composite_bwd", _ptr(d_rgb), _ptr(d_w), _ptr(d_info), _ptr(d_bg), _ptr(d_go), C.c_void_p(None), _ptr(gw2), *_sizes(fx))
    assert torch.equal(grgb, grgb2) and torch.equal(gw, gw2)
    out, opac, grgb, gw = _np(out, R), _np(opac, R), _np(grgb, n), _np(gw, n)
    rout, ropac, terms, oterms = ref.composite(rgb, w, info, bg)
    bound, obound = ref.composite_bound(info, terms, oterms, bg)
    rgrgb, rgw, G, r_g = ref.composite_grad(rgb, w, info, bg, go)
    assert (grgb[~own] == ref.SENTINEL).all() and (gw[~own] == ref.SENTINEL).all()
    assert np.isfinite(out).all() and np.isfinite(opac).all() and np.isfinite(grgb).all() and np.isfinite(gw).all()
    ref.same_bits(grgb[own], rgrgb[own].astype(f32), f"{name} {kind} grad_rgbs")
    if kind == "exact":
        ref.same_bits(out, rout.astype(f32), f"{name} exact rendered")
        ref.same_bits(opac, ropac.astype(f32), f"{name} exact opacity")
        ref.same_bits(gw[own], rgw[own].astype(f32), f"{name} exact grad_weights")
        return
    ratio = max(ref.worst_ratio(out, rout, bound, f"{name} rendered"), ref.worst_ratio(opac, ropac, obound, f"{name} opacity"))
    _note("tn_composite_fwd", ratio)
    rb = _note("tn_composite_bwd", ref.worst_ratio(gw[own], rgw[own], r_g * ref.U * G[own], f"{name} grad_weights"))
    print(f"{name} bg {with_bg}: tn_composite_fwd err / bound {ratio:.3f}, tn_composite_bwd {rb:.3f}")


# ------------------------------------------------------------------------------------------------ tn_render_rays_*
@pytest.mark.parametrize("with_bg", [True, False])
@pytest.mark.parametrize("name", ref.FIXTURES)
def test_render_rays_against_fp64(name, with_bg):
    thr = 1e-4
    fx, r = ref.fixture(name), ref.forward_ref(name, thr)
    info, n, R = fx["info"], fx["n"], fx["R"]
    bg = ref.BG if with_bg else None
    x = _Inputs(fx)
    w32 = r["w"].astype(f32)
    rgb = ref.masked_rgb(fx["rgb"], w32)
    d_rgb, d_bg, d_go = _dev(rgb), _dev(bg), _dev(fx["go"])
    own = ref.owned(info, n)
    want_gate = float((r["w"] > 0).any())
    # forward
    for gate in (None, torch.zeros(1, device=DEV)):
        w, out = _buf(n), _buf(R, 3)
        _call("tn_render_rays_fwd", _ptr(x.sig), _ptr(x.step), _ptr(d_rgb), _ptr(x.info), _ptr(d_bg), C.c_float(thr), _ptr(w), _ptr(out),
              _ptr(gate), *_sizes(fx))
        assert gate is None or float(gate) == want_gate
    got_w, got_out = _np(w, n), _np(out, R)
    worst = ref.check_weights(got_w, r, info, f"{name} tn_render_rays_fwd weights")
    rout, _, terms, oterms = ref.composite(rgb, got_w, info, bg)          # of the weights the launch wrote (their zero set is w_ref's)
    bound = ref.composite_bound(info, terms, oterms, bg)[0]
    worst = _note("tn_render_rays_fwd", max(worst, ref.worst_ratio(got_out, rout, bound, f"{name} tn_render_rays_fwd rendered")))
    if not fx["info"][:, 1].any():                          # no samples at all: the background, or nothing
        ref.same_bits(got_out, np.broadcast_to(ref.BG if with_bg else np.zeros(3, f32), (R, 3)), f"{name} all-empty rendered")
    # the fused launch is its two halves bit for bit: tn_composite_fwd on the weights it wrote, tn_weights_fwd on its inputs
    out2, w2 = _buf(R, 3), _buf(n)
    _call("tn_composite_fwd", _ptr(d_rgb), _ptr(w), _ptr(x.info), _ptr(d_bg), _ptr(out2), C.c_void_p(None), *_sizes(fx))
    _call("tn_weights_fwd", _ptr(x.sig), _ptr(x.step), _ptr(x.info), C.c_float(thr), _ptr(w2), *_sizes(fx))
    ref.same_bits(_np(out2, R), got_out, f"{name} tn_composite_fwd on tn_render_rays_fwd's weights, rendered")
    ref.same_bits(_np(w2, n), got_w, f"{name} tn_weights_fwd against tn_render_rays_fwd, weights")
    # backward, on the reference weights
    d_w = _dev(w32)
    res = {}
    for entry, extra in (("tn_render_rays_bwd", None), ("tn_render_rays_bwd_dw", fx["extra"])):
        grgb, gs = _buf(n, 3), _buf(n)
        d_extra = _dev(extra)                                   # (held in a name: the launch reads it after _ptr returns)
        tail = () if extra is None else (_ptr(d_extra),)
        _call(entry, _ptr(x.sig), _ptr(x.step), _ptr(d_rgb), _ptr(x.info), _ptr(d_bg), _ptr(d_w), _ptr(d_go), *tail, _ptr(grgb), _ptr(gs),
              *_sizes(fx))
        grgb, gs = _np(grgb, n), _np(gs, n)
        rgrgb, rgw, G, r_g = ref.composite_grad(rgb, w32, info, bg, fx["go"], extra)
        want, gbound, _ = ref.weights_grad(fx["sig"], fx["step"], info, w32, rgw, gabs=G, r_g=r_g)
        assert (grgb[~own] == ref.SENTINEL).all()
        ref.same_bits(grgb[own], rgrgb[own].astype(f32), f"{name} {entry} grad_rgbs")
        res[entry] = _note(entry, ref.check_owned(gs, want, gbound, info, f"{name} {entry} grad_sigmas"))
    print(f"{name} bg {with_bg}: tn_render_rays_fwd err / bound {worst:.3f}, _bwd {res['tn_render_rays_bwd']:.3f}, _bwd_dw {res['tn_render_rays_bwd_dw']:.3f}")


# ------------------------------------------------------------------------------------------------ tn_mse_grad / _gated
@pytest.mark.parametrize("n", ref.MSE_SIZES)
def test_mse_grad_against_fp64(n):
    r, t = ref.mse_inputs(n)
    d_r, d_t = _dev(r), _dev(t)
    start, scale = 0.75, 0.25
    worst = 0.0
    for c_dev in (None, 3.0):
        d_c = None if c_dev is None else torch.tensor([c_dev], device=DEV)
        for gate in (None, 1.0, 0.0, -1.0, float("nan")):
            grad = _buf(n + 1)                                  # one element behind the end: it keeps the sentinel
            acc = torch.tensor([start], dtype=torch.float64, device=DEV)
            if gate is None:
                _call("tn_mse_grad", _ptr(d_r), _ptr(d_t), C.c_int64(n), C.c_float(scale), _ptr(d_c), _ptr(grad), _ptr(acc))
            else:
                d_gate = torch.tensor([gate], device=DEV)
                _call("tn_mse_grad_gated", _ptr(d_r), _ptr(d_t), C.c_int64(n), C.c_float(scale), _ptr(d_c), _ptr(d_gate), _ptr(grad), _ptr(acc))
            want, s, bound = ref.mse(r, t, scale, c_dev, gate, start)
            got = grad.cpu().numpy()
            assert got[n] == ref.SENTINEL
            ref.same_bits(got[:n], want, f"mse n {n} c_dev {c_dev} gate {gate} grad")
            assert (want != 0).any() == (gate is None or gate > 0)
            worst = max(worst, ref.worst_ratio(np.array([float(acc)]), np.array([s]), np.array([bound]), f"mse n {n} sumsq"))
    _note("tn_mse_grad sumsq", worst)
    print(f"n {n}: tn_mse_grad sumsq err / bound {worst:.3f}")
