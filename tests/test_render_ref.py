"""CPU checks of the volume-rendering yardstick (tests/_render_ref.py), no GPU:

* the fp64 references agree with what the project already has: oracle.weights_fwd_vectorised, oracle.weights_bwd_fp64, and torch
  autograd in fp64 of T (1 - alpha) with thr = 0 and of the composite;
* a numpy fp32 restatement of the kernels' evaluation order (64-lane Kogge-Stone scans with carries across chunks, lane-strided
  partial sums under a 64-leaf butterfly, the register and the streaming backward) stays inside every bound on every fixture -- the
  largest err / bound per kernel is printed;
* mutants of that restatement (a dropped carry, termination off by one, a short total, a flipped bg sign, masked colours read, a
  lane left out of a wave_sum, an element the loss kernel does not visit) each break a bound, a zero set or a bit-exact comparison;
* no fixture holds a ray whose transmittance comes within the bound on T of a threshold, and the regimes are what they claim;
* the entry points reject bad arguments before any launch (the cases tests/test_abi.py and tests/test_distortion_abi.py leave)."""
import ctypes

import numpy as np
import pytest
import torch

import _render_ref as ref
from oracle import tinynerf_oracle as orc

f32, f64 = np.float32, np.float64
LANES = np.arange(64)
THR = ref.THRESHOLDS


# ------------------------------------------------------------------------------------------------ the references agree
@pytest.mark.parametrize("name", ["smooth_ladder", "smooth_gaps_permuted", "walls_short", "walls_long", "unbounded"])
def test_yardstick_agrees_with_the_oracle(name):
    fx = ref.fixture(name)
    for thr in THR:
        got = ref.forward_ref(name, thr)["w"]
        want = orc.weights_fwd_vectorised(fx["sig"], fx["step"], fx["info"], ref.thr32(thr))
        np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-60)
    w = ref.forward_ref(name, 1e-4)["w"].astype(f32)
    gs = ref.weights_grad(fx["sig"], fx["step"], fx["info"], w, fx["g"])[0]
    want = orc.weights_bwd_fp64(fx["sig"], fx["step"], fx["info"], w, fx["g"])          # (returned as fp32)
    np.testing.assert_allclose(gs, want, rtol=2.0 ** -23, atol=1e-30)


@pytest.mark.parametrize("name", ["smooth_rays9", "smooth_empties", "walls_short"])
@pytest.mark.parametrize("with_bg", [True, False])
def test_yardstick_agrees_with_autograd(name, with_bg):
    fx = ref.fixture(name)
    info, n = fx["info"], fx["n"]
    sig = torch.tensor(fx["sig"], dtype=torch.float64, requires_grad=True)
    step, g = torch.tensor(fx["step"], dtype=torch.float64), torch.tensor(fx["g"], dtype=torch.float64)
    w = torch.zeros(n, dtype=torch.float64)
    for _, s, c in ref.rays(info):
        if c:
            a = torch.exp(-sig[s:s + c] * step[s:s + c])
            T = torch.cat([torch.ones(1, dtype=torch.float64), torch.cumprod(a, 0)[:-1]])
            w = w.index_put((torch.arange(s, s + c),), T * (1 - a))
    r0 = ref.forward_ref(name, 0.0)
    np.testing.assert_allclose(w.detach().numpy(), r0["w"], rtol=1e-12, atol=1e-60)
    (w * g).sum().backward()
    gs, bound, A = ref.weights_grad(fx["sig"], fx["step"], info, w.detach().numpy(), fx["g"])
    scale = np.zeros(n)
    for r, s, c in ref.rays(info):
        scale[s:s + c] = A[r] + np.abs(fx["g"][s:s + c])
    assert (np.abs(sig.grad.numpy() - gs) <= 1e-12 * fx["step"] * scale).all()
    # composite
    bg = ref.BG if with_bg else None
    wv = r0["w"].astype(f32)
    rgb_t = torch.tensor(fx["rgb"], dtype=torch.float64, requires_grad=True)
    w_t = torch.tensor(wv, dtype=torch.float64, requires_grad=True)
    idx = torch.as_tensor(np.concatenate([np.full(c, r) for r, _, c in ref.rays(info)] + [np.zeros(0, np.int64)]).astype(np.int64))
    own = torch.as_tensor(np.concatenate([np.arange(s, s + c) for _, s, c in ref.rays(info)] + [np.zeros(0, np.int64)]).astype(np.int64))
    out = torch.zeros((fx["R"], 3), dtype=torch.float64).index_add(0, idx, (rgb_t * w_t[:, None])[own])
    opac = torch.zeros(fx["R"], dtype=torch.float64).index_add(0, idx, w_t[own])
    if with_bg:
        out = out + torch.tensor(ref.BG, dtype=torch.float64) * (1 - opac[:, None])
    want, wopac, _, _ = ref.composite(ref.masked_rgb(fx["rgb"], wv), wv, info, bg)
    np.testing.assert_allclose(out.detach().numpy(), want, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(opac.detach().numpy(), wopac, rtol=1e-12, atol=1e-14)
    go = torch.tensor(fx["go"], dtype=torch.float64)
    (out * go).sum().backward()
    grgb, gw, G, _ = ref.composite_grad(ref.masked_rgb(fx["rgb"], wv), wv, info, bg, fx["go"])
    np.testing.assert_allclose(rgb_t.grad.numpy(), grgb, rtol=1e-12, atol=1e-14)
    live = wv != 0                  # (the kernels' masked samples carry colour 0: their grad_w is -<bg, g> only)
    np.testing.assert_allclose(w_t.grad.numpy()[live], gw[live], rtol=1e-12, atol=1e-13)
    dead = ref.owned(info, n) & ~live
    for r, s, c in ref.rays(info):
        m = np.zeros(n, bool)
        m[s:s + c] = True
        np.testing.assert_allclose(gw[m & dead], -(ref.f64(ref.BG) * fx["go"][r]).sum() if with_bg else 0.0, rtol=1e-13, atol=0)


# ------------------------------------------------------------------------------------------------ fp32 restatement of the kernels
def _scan(v, op):
    """wave_scan_mul / wave_scan_add: inclusive, six shuffle-up steps"""
    v = v.copy()
    for o in (1, 2, 4, 8, 16, 32):
        up = v[:-o].copy()
        v[o:] = op(v[o:], up)
    return v


def _wave_sum(v, mut=""):
    v = v.copy()
    if mut == "skip63":
        v[63] = 0
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[LANES ^ o]
    return v[0]


def emu_weights_fwd(sig, step, info, thr, n, mut="", rgb=None, bg=None, gate=0.0):
    """weights_fwd_kernel<COMP>: -> (weights, gate, rendered or None)"""
    out = np.full(n, ref.SENTINEL, f32)
    rendered = None if rgb is None else np.full((len(info), 3), ref.SENTINEL, f32)
    thr = f32(thr)
    for r, s, c in ref.rays(info):
        acc = np.zeros((4, 64), f32)
        carry, alive = f32(1), True
        for base in range(0, c, 64):
            m = min(64, c - base)
            sl = slice(s + base, s + base + m)
            w = np.zeros(64, f32)
            if alive:
                a = np.ones(64, f32)
                a[:m] = np.exp(-sig[sl] * step[sl])
                incl = _scan(a, np.multiply)
                T = carry * np.concatenate([[f32(1)], incl[:-1]]).astype(f32)
                dead = (LANES < m) & ~(T > thr)
                first = int(np.argmax(dead)) if dead.any() else 64
                if dead.any() and mut == "late":
                    first += 1
                if dead.any() and mut == "early":
                    first = max(first - 1, 0)
                live = LANES < first
                w[live] = (T[live].astype(f64) * (1.0 - a[live].astype(f64))).astype(f32)
                if mut != "fwd_carry":
                    carry = carry * incl[63]
                alive = not dead.any()
            out[sl] = w[:m]
            if (w[:m] > 0).any():
                gate = 1.0
            if rgb is not None:
                use = (w[:m] != 0) | (mut == "read_masked")
                for ch in range(3):
                    acc[ch, :m][use] = acc[ch, :m][use] + rgb[sl, ch][use] * w[:m][use]
                acc[3, :m] = acc[3, :m] + w[:m]
        if rgb is not None:
            tot = [_wave_sum(acc[ch], mut) for ch in range(4)]
            for ch in range(3):
                v = tot[ch]
                if bg is not None:
                    v = v + bg[ch] * (f32(1) - tot[3]) if mut != "bg_sign_fwd" else v - bg[ch] * (f32(1) - tot[3])
                rendered[r, ch] = v
    return out, gate, rendered


def emu_composite_fwd(rgb, w, info, bg, mut=""):
    """composite_fwd_kernel: -> (rendered, opacity)"""
    R = len(info)
    rendered, opacity = np.full((R, 3), ref.SENTINEL, f32), np.full(R, ref.SENTINEL, f32)
    for r, s, c in ref.rays(info):
        acc = np.zeros((4, 64), f32)
        for base in range(0, c, 64):
            m = min(64, c - base)
            sl = slice(s + base, s + base + m)
            use = (w[sl] != 0) | (mut == "read_masked")
            for ch in range(3):
                acc[ch, :m][use] = acc[ch, :m][use] + rgb[sl, ch][use] * w[sl][use]
            acc[3, :m] = acc[3, :m] + w[sl]
        tot = [_wave_sum(acc[ch], mut) for ch in range(4)]
        for ch in range(3):
            v = tot[ch]
            if bg is not None:
                v = v + bg[ch] * (f32(1) - tot[3]) if mut != "bg_sign_fwd" else v - bg[ch] * (f32(1) - tot[3])
            rendered[r, ch] = v
        opacity[r] = tot[3]
    return rendered, opacity


def emu_composite_bwd(rgb, w, info, bg, go, n, extra=None, mut=""):
    """composite_bwd_kernel / the grad_weight lambda of weights_bwd_kernel<COMP>: -> (grad_rgbs, grad_weights)"""
    grgb, gw = np.full((n, 3), ref.SENTINEL, f32), np.full(n, ref.SENTINEL, f32)
    for r, s, c in ref.rays(info):
        sl = slice(s, s + c)
        g = go[r]
        gbg = f32(0) if bg is None else (bg[0] * g[0] + bg[1] * g[1]) + bg[2] * g[2]
        grgb[sl] = w[sl, None] * g[None]
        d = np.zeros(c, f32)
        use = (w[sl] != 0) | (mut == "read_masked")
        d[use] = (rgb[sl, 0][use] * g[0] + rgb[sl, 1][use] * g[1]) + rgb[sl, 2][use] * g[2]
        v = d - gbg if mut != "bg_sign_bwd" else d + gbg
        gw[sl] = v if extra is None else v + extra[sl]
    return grgb, gw


def emu_weights_bwd(sig, step, info, w, g, n, mut=""):
    """weights_bwd_kernel<16, ...>: the register path up to 1024 samples, the streaming path behind"""
    out = np.full(n, ref.SENTINEL, f32)
    for r, s, c in ref.rays(info):
        if not c:
            continue
        k = ref.nch(c)
        pad = lambda x, fill: np.concatenate([x[s:s + c], np.full(64 * k - c, fill, f32)]).astype(f32).reshape(k, 64)
        W, G, D = pad(w, 0), pad(g, 0), pad(step, 0)
        A = np.concatenate([np.exp(-sig[s:s + c] * step[s:s + c]), np.ones(64 * k - c, f32)]).astype(f32).reshape(k, 64)
        WG = W * G
        total = np.zeros(64, f32)
        if c <= 64 * ref.MAXC:                                  # registers: all MAXC slots are added, the unused ones hold 0
            for ch in range(ref.MAXC):
                total = total + (WG[ch] if ch < k else np.zeros(64, f32))
        else:
            for ch in range(ref.MAXC if mut == "total1024" else k):
                total = total + WG[ch]
        acc, T = -_wave_sum(total, mut), f32(1)
        for ch in range(k):
            m = min(64, c - 64 * ch)
            ps, pt = _scan(WG[ch], np.add), _scan(A[ch], np.multiply)
            out[s + 64 * ch:s + 64 * ch + m] = (D[ch] * ((acc + ps) + (T * pt) * G[ch]))[:m]
            if mut != "acc_carry":
                acc = acc + ps[63]
            if mut != "bwd_T_carry":
                T = T * pt[63]
    return out


def emu_mse(r, t, c, c_dev, gate, start, mut=""):
    """mse_grad_kernel: -> (grad, sumsq)"""
    n = r.size
    threads = ref.mse_blocks(n) * 256
    cc = f32(c) if c_dev is None else f32(c) * f32(c_dev)
    if gate is not None and not (f32(gate) > 0):
        cc = f32(0)
    grad = np.full(n, ref.SENTINEL, f32)
    s = np.zeros(threads, f32)
    for base in range(0, n, threads):
        if mut == "mse_one_round" and base:
            break
        m = min(threads, n - base)
        d = r[base:base + m] - t[base:base + m]
        grad[base:base + m] = d * cc
        s[:m] = (d.astype(f64) * d.astype(f64) + s[:m].astype(f64)).astype(f32)          # fmaf
    return grad, start + float(s.astype(f64).sum())


# ------------------------------------------------------------------------------------------------ one comparison per kernel
def check_fwd(name, thr, mut=""):
    fx, r = ref.fixture(name), ref.forward_ref(name, thr)
    got, gate, _ = emu_weights_fwd(fx["sig"], fx["step"], fx["info"], thr, fx["n"], mut)
    assert gate == float((r["w"] > 0).any())
    return ref.check_weights(got, r, fx["info"], f"{name} thr {thr} weights")


def check_bwd(name, mut=""):
    fx = ref.fixture(name)
    w = ref.forward_ref(name, 1e-4)["w"].astype(f32)
    got = emu_weights_bwd(fx["sig"], fx["step"], fx["info"], w, fx["g"], fx["n"], mut)
    gs, bound, _ = ref.weights_grad(fx["sig"], fx["step"], fx["info"], w, fx["g"])
    return ref.check_owned(got, gs, bound, fx["info"], f"{name} grad_sigmas")


def check_composite(name, kind, with_bg, mut=""):
    fx = ref.fixture(name)
    info, n, bg = fx["info"], fx["n"], (ref.BG if with_bg else None)
    if kind == "exact":
        w, go = fx["exact_w"], fx["exact_go"]
        rgb = ref.masked_rgb(fx["exact_rgb"], w)
    else:
        w, go = ref.forward_ref(name, 1e-4)["w"].astype(f32), fx["go"]
        rgb = ref.masked_rgb(fx["rgb"], w)
    out, opac = emu_composite_fwd(rgb, w, info, bg, mut)
    grgb, gw = emu_composite_bwd(rgb, w, info, bg, go, n, mut=mut)
    rout, ropac, terms, oterms = ref.composite(rgb, w, info, bg)
    bound, obound = ref.composite_bound(info, terms, oterms, bg)
    rgrgb, rgw, G, r_g = ref.composite_grad(rgb, w, info, bg, go)
    own = ref.owned(info, n)
    assert (grgb[~own] == ref.SENTINEL).all() and (gw[~own] == ref.SENTINEL).all()
    ref.same_bits(grgb[own], rgrgb[own].astype(f32), f"{name} {kind} grad_rgbs")
    if kind == "exact":
        ref.same_bits(out, rout.astype(f32), f"{name} exact rendered")
        ref.same_bits(opac, ropac.astype(f32), f"{name} exact opacity")
        ref.same_bits(gw[own], rgw[own].astype(f32), f"{name} exact grad_weights")
        return 0.0
    return max(ref.worst_ratio(out, rout, bound, f"{name} rendered"), ref.worst_ratio(opac, ropac, obound, f"{name} opacity"),
               ref.worst_ratio(gw[own], rgw[own], r_g * ref.U * G[own], f"{name} grad_weights"))


def check_fused(name, with_bg, with_extra, mut=""):
    fx, r = ref.fixture(name), ref.forward_ref(name, 1e-4)
    info, n, bg = fx["info"], fx["n"], (ref.BG if with_bg else None)
    w32 = r["w"].astype(f32)
    rgb = ref.masked_rgb(fx["rgb"], w32)
    got_w, _, rendered = emu_weights_fwd(fx["sig"], fx["step"], info, 1e-4, n, mut, rgb=rgb, bg=bg)
    worst = ref.check_weights(got_w, r, info, f"{name} fused weights")
    rout, _, terms, oterms = ref.composite(rgb, got_w, info, bg)          # of the weights the launch wrote (their zero set is w_ref's)
    worst = max(worst, ref.worst_ratio(rendered, rout, ref.composite_bound(info, terms, oterms, bg)[0], f"{name} fused rendered"))
    extra = fx["extra"] if with_extra else None
    grgb, gw = emu_composite_bwd(rgb, w32, info, bg, fx["go"], n, extra=extra, mut=mut)
    got = emu_weights_bwd(fx["sig"], fx["step"], info, w32, gw, n, mut)
    rgrgb, rgw, G, r_g = ref.composite_grad(rgb, w32, info, bg, fx["go"], extra)
    gs, gbound, _ = ref.weights_grad(fx["sig"], fx["step"], info, w32, rgw, gabs=G, r_g=r_g)
    own = ref.owned(info, n)
    ref.same_bits(grgb[own], rgrgb[own].astype(f32), f"{name} fused grad_rgbs")
    return max(worst, ref.check_owned(got, gs, gbound, info, f"{name} fused grad_sigmas"))


def check_mse(n, c_dev, gate, start=0.75, mut=""):
    r, t = ref.mse_inputs(n)
    grad, s = emu_mse(r, t, 0.25, c_dev, gate, start, mut)
    rgrad, rs, bound = ref.mse(r, t, 0.25, c_dev, gate, start)
    ref.same_bits(grad, rgrad, f"mse n {n} grad")
    return ref.worst_ratio(np.array([s]), np.array([rs]), np.array([bound]), f"mse n {n} sumsq")


# ------------------------------------------------------------------------------------------------ the restatement is inside
def test_restatement_stays_inside_every_bound():
    worst = {}

    def note(kernel, ratio):
        worst[kernel] = max(worst.get(kernel, 0.0), ratio)
    for name in ref.FIXTURES:
        for thr in THR:
            note("weights_fwd", check_fwd(name, thr))
        note("weights_bwd", check_bwd(name))
        for with_bg in (True, False):
            note("composite", check_composite(name, "general", with_bg))
            check_composite(name, "exact", with_bg)
            note("render_rays", check_fused(name, with_bg, False))
        note("render_rays_dw", check_fused(name, True, True))
    for n in ref.MSE_SIZES:
        for c_dev, gate in ((None, None), (3.0, 1.0), (3.0, 0.0), (None, -1.0), (None, float("nan"))):
            note("mse", check_mse(n, c_dev, gate))
    for kernel, ratio in worst.items():
        print(f"fp32 restatement, {kernel}: largest err / bound {ratio:.3f}")
    assert set(worst) == {"weights_fwd", "weights_bwd", "composite", "render_rays", "render_rays_dw", "mse"}


MUTANTS = {
    "fwd_carry": lambda m: check_fwd("smooth_ladder", 1e-4, m),
    "acc_carry": lambda m: check_bwd("smooth_ladder", m),
    "bwd_T_carry": lambda m: check_bwd("smooth_ladder", m),
    "late": lambda m: check_fwd("walls_short", 1e-4, m),
    "early": lambda m: check_fwd("walls_short", 1e-4, m),
    "total1024": lambda m: check_bwd("smooth_ladder", m),
    "bg_sign_fwd": lambda m: check_composite("smooth_ladder", "general", True, m),
    "bg_sign_bwd": lambda m: check_composite("smooth_ladder", "general", True, m),
    "read_masked": lambda m: check_composite("walls_short", "general", True, m),
    "skip63": lambda m: check_composite("smooth_ladder", "general", False, m),
    "mse_one_round": lambda m: check_mse(131073, None, None, mut=m),
}


@pytest.mark.parametrize("mut", list(MUTANTS))
def test_every_mutant_is_caught(mut):
    MUTANTS[mut]("")                                   # the same comparison passes unmutated
    with pytest.raises(AssertionError):
        MUTANTS[mut](mut)


@pytest.mark.parametrize("mut,check", [
    ("late", lambda m: check_fused("walls_long", True, False, m)),          # a wall on a chunk edge, through the fused forward
    ("early", lambda m: check_fused("walls_long", True, False, m)),
    ("fwd_carry", lambda m: check_fused("unbounded", True, True, m)),
    ("skip63", lambda m: check_bwd("smooth_rays9", m)),                     # the backward's total
    ("skip63", lambda m: check_composite("smooth_ladder", "exact", True, m)),
    ("bg_sign_fwd", lambda m: check_composite("smooth_rays3", "exact", True, m)),
    ("bg_sign_bwd", lambda m: check_fused("smooth_rays5", True, True, m)),
    ("read_masked", lambda m: check_fused("walls_short", False, False, m)),
    ("total1024", lambda m: check_fused("smooth_gaps_permuted", False, False, m)),
    ("acc_carry", lambda m: check_bwd("unbounded", m)),
])
def test_mutants_are_caught_on_the_other_fixtures_too(mut, check):
    with pytest.raises(AssertionError):
        check(mut)


# ------------------------------------------------------------------------------------------------ the fixtures are what they claim
def test_ladder_and_ray_counts():
    counts = set()
    for name in ref.FIXTURES:
        counts |= set(int(c) for c in ref.fixture(name)["info"][:, 1])
        assert ref.fixture(name)["R"] <= 300 and ref.fixture(name)["n"] <= 40000, name
    assert set(ref.LADDER) <= counts
    assert {ref.fixture(f"smooth_rays{R}")["R"] for R in (1, 3, 4, 5, 9)} == {1, 3, 4, 5, 9}
    e = ref.fixture("smooth_empties")["info"][:, 1]
    assert e[0] == 0 and e[-1] == 0 and e[4] == 0 and e[3] > 0 and e[6] > 0
    assert ref.fixture("all_empty")["n"] == 0 and ref.fixture("all_empty_gaps")["n"] > 0
    for name in ("smooth_gaps_permuted", "walls_gaps_permuted"):
        fx = ref.fixture(name)
        assert not ref.owned(fx["info"], fx["n"]).all() and (np.diff(fx["info"][:, 0]) < 0).any()


@pytest.mark.parametrize("name", ref.FIXTURES)
def test_regimes_and_zero_danger(name):
    fx = ref.fixture(name)
    info = fx["info"]
    for thr in THR:
        r = ref.forward_ref(name, thr)
        assert ref.danger_rays(r, info, thr) == [], (name, thr)
    r0, r4 = ref.forward_ref(name, 0.0), ref.forward_ref(name, 1e-4)
    own = r0["k"] >= 0
    zero_alpha = r0["a"] == 0
    for _, s, c in ref.rays(info):
        sl = slice(s, s + c)
        T, p = r0["T"][sl], r0["p"][sl]
        behind_zero = np.cumsum(zero_alpha[sl]) - zero_alpha[sl] > 0
        assert (T[~behind_zero] >= 1e-30).all() and (T[behind_zero] == 0).all()
        wall = (p >= 12) & (p <= 20)
        if fx["regime"] == "smooth":
            assert p.sum() <= 5.0 and not wall.any() and (r4["w"][sl] > 0).all()
            assert ((fx["step"][sl] >= 1e-3) & (fx["step"][sl] <= 0.08)).all()
        else:
            assert wall.sum() <= 1 and p[~wall & (p < 100)].sum() <= 5.0
            if wall.any():
                i = int(np.argmax(wall))
                assert T[i] >= 6.7e-3 and (i + 1 == c or T[i + 1] <= 6.1e-6)
        if fx["regime"] == "unbounded" and c > 1:
            assert 5.0 < fx["step"][sl].max() <= 10.0
    if name == "unbounded":                                 # the ladder twice; every non-empty ray of the second copy carries a wall
        walled = [bool(((r0["p"][s:s + c] >= 12) & (r0["p"][s:s + c] <= 20)).any()) for _, s, c in ref.rays(info)]
        L = len(ref.LADDER)
        assert not any(walled[:L]) and walled[L:] == [c > 0 for c in ref.LADDER] and sum(walled) == 12 and fx["R"] == 26
        for (_, s, c), wl in zip(ref.rays(info), walled):
            if wl and c > 2:                                # behind the wall: weights 0, so the suffix sum is 0 under a step that grows on
                assert (r4["w"][s:s + c] == 0).sum() >= c // 2
    if name == "singles":
        assert (info[:, 1] == 1).all() and fx["R"] == 67 and (r0["a"][own] >= 0.5).all()
    if name == "walls_short":
        assert ((r0["a"] == 1) & own).sum() >= 40 and zero_alpha.sum() == 2
    if fx["regime"] != "smooth":
        assert ((r4["w"] == 0) & own).any()


def test_walls_stand_on_every_listed_index():
    seen = set()
    for name in ("walls_short", "walls_long"):
        r = ref.forward_ref(name, 0.0)
        for _, s, c in ref.rays(ref.fixture(name)["info"]):
            p = r["p"][s:s + c]
            for i in np.nonzero((p >= 12) & (p <= 20))[0]:
                seen |= {int(i)} | ({-1} if i == c - 1 else set())
    assert set(ref.WALL_AT) <= seen


def test_constants_of_the_bounds():
    assert [int(ref.r_T(m)) for m in (0, 1, 2, 3, 63, 64, 65, 128)] == [0, 1, 2, 3, 7, 7, 8, 14]
    assert ref.c_add(1) == 18 and ref.c_add(1024) == 48 and ref.c_add(1025) == 50
    assert ref.EXPF_ULPS <= 4 and ref.U == 2.0 ** -24
    assert [ref.mse_blocks(n) for n in (1, 256, 257, 131072, 131073)] == [1, 1, 2, 512, 512]


# ------------------------------------------------------------------------------------------------ argument checks, no launch
@pytest.fixture(scope="module")
def lib():
    from tinynerf_amd import build
    lib = ctypes.CDLL(build.build(verbose=False))
    lib.tn_last_error_string.restype = ctypes.c_char_p
    return lib


def test_render_entry_points_reject_bad_arguments_before_launching(lib):
    i64, cf, vp = ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
    fake, odd = vp(64), vp(68)                              # never dereferenced: every call below returns before a launch
    OK, NULL, SIZE, ALIGN = 0, -1, -2, -4
    thr = cf(1e-4)

    def sizes(n, R):
        return (i64(n), i64(R), None)
    # name -> the arguments before the sizes as a function of (pointer, info)
    table = {
        "tn_weights_fwd": lambda p, i: (p, p, i, thr, p),
        "tn_weights_fwd_gate": lambda p, i: (p, p, i, thr, p, p),
        "tn_weights_bwd": lambda p, i: (p, p, i, p, p, p),
        "tn_composite_fwd": lambda p, i: (p, p, i, None, p, None),
        "tn_composite_bwd": lambda p, i: (p, p, i, None, p, p, p),
        "tn_render_rays_fwd": lambda p, i: (p, p, p, i, None, thr, p, p, None),
        "tn_render_rays_bwd": lambda p, i: (p, p, p, i, None, p, p, p, p),
    }
    for name, args in table.items():
        fn = getattr(lib, name)
        assert fn(*args(fake, fake), *sizes(-1, 4)) == SIZE, name
        assert fn(*args(fake, fake), *sizes(8, -4)) == SIZE, name
        assert fn(*args(None, fake), *sizes(8, 4)) == NULL and name.encode() in lib.tn_last_error_string(), name
        assert fn(*args(fake, None), *sizes(8, 4)) == NULL, name
        assert fn(*args(fake, odd), *sizes(8, 4)) == ALIGN and b"8-byte" in lib.tn_last_error_string(), name
        assert fn(*args(None, None), *sizes(8, 0)) == OK, name
    for name in ("tn_weights_fwd", "tn_weights_fwd_gate", "tn_weights_bwd", "tn_composite_bwd", "tn_render_rays_bwd"):
        assert getattr(lib, name)(*table[name](None, None), *sizes(0, 4)) == OK, name       # no samples: nothing to write
    # the two forwards that write per-ray outputs launch with n_samples == 0, so their per-ray pointers are still required
    assert lib.tn_composite_fwd(None, None, fake, None, None, None, *sizes(0, 4)) == NULL
    assert lib.tn_render_rays_fwd(None, None, None, fake, None, thr, fake, None, None, *sizes(0, 4)) == NULL
    assert lib.tn_weights_fwd_gate(fake, fake, fake, thr, fake, None, *sizes(8, 4)) == NULL          # the gate is the point of it
    mse, gated = lib.tn_mse_grad, lib.tn_mse_grad_gated
    assert mse(fake, fake, i64(-1), cf(1.0), None, fake, fake, None) == SIZE
    assert mse(None, None, i64(0), cf(1.0), None, None, None, None) == OK
    assert mse(fake, fake, i64(4), cf(1.0), None, fake, None, None) == NULL and b"tn_mse_grad" in lib.tn_last_error_string()
    assert mse(fake, None, i64(4), cf(1.0), None, fake, fake, None) == NULL
    assert gated(fake, fake, i64(-1), cf(1.0), None, fake, fake, fake, None) == SIZE
    assert gated(None, None, i64(0), cf(1.0), None, None, None, None, None) == OK
    assert gated(fake, fake, i64(4), cf(1.0), None, None, fake, fake, None) == NULL and b"tn_mse_grad_gated" in lib.tn_last_error_string()
