"""GPU tests of the seven kernels of csrc/planes_reg.hip (adam_kernel, adam_multi_kernel<GATED>, adam_gate_kernel,
adam_reg_multi_kernel, plane_reg_fwd_kernel, plane_reg_bwd_kernel, plane_reg_multi_kernel) through the ABI, per element against the
float64 yardstick tests/_optim_ref.py: second rounds of the grid-stride loops, every tail, chunking past TN_MULTI_MAX, the
row-sharded pass, the gate and the regularisers' edges.

Inputs.  Parameters uniform in [-1, 1]; |g| log-uniform in [1e-3, 1024] with random sign and one exact zero in eight, so g^2 (and
(wd p)^2 where g == 0) stays far above fp32 underflow.  Moments are zero at step 1; at a later step p, m, v are the yardstick's
previous step rounded to fp32.  The yardstick gets the hyper-parameters as the fp32 values the ABI receives (1 - b1 and 1 - b2 are
then exact in fp32), so what separates kernel and yardstick is the kernel's own roundings.  u = 2^-24, gamma(k) = k u / (1 - k u).

Bounds, by counting the kernel's fp32 operations (a fused multiply-add only removes a rounding).  G = |g| + |wd p|:
  gg = g + wd p                  2 roundings                                             |err| <= gamma(2) G
  m' = m + (gg - m)(1 - b1)      2 + difference, product, sum = 5                        |err| <= gamma(5) (|m| + (1 - b1)(G + |m|))
  v' = b2 v + (1 - b2) gg gg     gg twice (4) + two products + sum = 7, b2 v: 2          |err| <= gamma(7) (b2 v + (1 - b2) G^2)
  p' = p - (lr / bc1)(m' / (sqrt(v') / bc2s + eps)): no single k -- the errors of m' and v' above are carried through sqrt and the
       quotient with their condition numbers (sqrt over the interval v' +- err, the denominator no smaller than eps), and the
       kernel's own roundings are added: sqrt 1, bc2s (a float64 value cast to fp32) and the division 2, + eps 1 -> gamma(3) on the
       denominator after the sqrt; m' / denominator 1; bc1's cast, lr / bc1 and the product -> gamma(3); the last subtraction u (|p| +
       |update|).  adam_bounds() below is that propagation, term by term.  Where v' is all cancellation (g + regulariser gradient
       ~ 0 at step 1) the bound on p is honestly large; the tests print the share of such elements and hold it below 1 %
       (regularised planes) or at 0 (plain Adam).  m' and v' are bounded tightly at every element regardless.
  regulariser gradient g0 + up (2cy dy + 2cx dx + cl1 sign(p)): two differences and their combination per direction (err <= gamma(2)
       of the magnitudes |p| + |q|), times 2c (exact doubling, 1 product), sum of the directions 1, + cl1 sign 1, times up 1, + g0 1 =
       7: |err| <= gamma(7) (|g0| + _optim_ref.plane_reg_magnitude).  Inside tn_adam_reg_multi that gradient feeds Adam: kg = 7 more
       roundings on g, so gamma(5 + 7) for m' and gamma(7 + 14) for v'.
  sums: a thread adds, per float4 it visits, d0^2 + d1^2 + d2^2 + d3^2 (difference 1, square 1, three additions: 5, bounded by 6)
       resp. |v0| + ... + |v3| (3) in fp32; the single-plane forward kernel converts each such term to fp64, the multi kernels keep an
       fp32 partial over the R rounds of the thread's loop (R more additions; R <= 2 here, from the grid caps of 2048 resp. 1024
       blocks).  Above that everything is fp64 (<= n4 additions of 2^-53).  All terms are non-negative, so the sum of magnitudes is
       the sum itself: |err| <= (gamma(6 + R) + n4 2^-53) sum for the TV sums, (gamma(3 + R) + n4 2^-53) sum for L1 (R = 0 for
       tn_plane_reg_fwd).
  Row ranges: a thread's partial of the full pass is fl(a + b) where the ranges hold a and b separately, so the ranges' sums add up
       to the full pass's within (gamma(1) + n4 2^-53) sum; with one round per thread (the 13x6x8 plane) within n4 2^-53 sum.
No margin here is measured: every k above is a count.

Worst |got - ref| / bound: every test prints its own and asserts < 1 at every index.  Ratios from an MI355X are NOT recorded here yet
(these tests have not run on a device).  What is recorded is the same formulas evaluated in fp32 numpy, one rounding per operation (no
fma), put through these tests in place of the kernels -- it says the bounds leave room for a correct fp32 evaluation, not that the
kernels meet them:
  tn_adam_step                    p 0.97  m 0.66  v 0.64      (p: the last subtraction's rounding u |p'| is nearly all of the bound)
  tn_adam_multi / _gated          p 0.91  m 0.64  v 0.63
  tn_adam_reg_multi               p 0.71  m 0.34  v 0.40  sums 0.08     row-sharded: p 0.83  m 0.41  v 0.39  sums 0.05
  tn_plane_reg_fwd / _bwd         sums 0.04  gradient 0.52
  tn_plane_reg_multi              sums 0.14  gradient 0.44
  loose p bounds: 0 for plain Adam; at most 0.5 % of a plane of 1000+ elements, at most one element of a smaller one"""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import _optim_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
PAD = 8                                      # floats of sentinel behind every buffer: a tail that stores a whole float4 shows there
SENTINEL = 7.25


def f32(x):
    return float(np.float32(x))


HP = dict(lr=f32(1e-2), b1=f32(0.9), b2=f32(0.999), eps=f32(1e-15), wd=f32(1e-5))      # reference run.py:186, as the ABI sees them
COEFS = [(f32(3e-3), f32(2e-3), f32(1e-3)), (f32(2e-3), f32(5e-3), 0.0)]              # (cy, cx, cl1), the second with cl1 == 0
UP = 1024.0


def gam(k):
    return k * U / (1.0 - k * U)


def hp_args():
    return [C.c_float(HP[k]) for k in ("lr", "b1", "b2", "eps", "wd")]


# ---- inputs

def draw(rng, shape):
    p = rng.uniform(-1, 1, shape).astype(np.float32)
    mag = np.clip(np.exp2(rng.uniform(math.log2(1e-3), 10.0, shape)).astype(np.float32), np.float32(0.001000001), np.float32(1024))
    g = mag * rng.choice(np.array([-1.0, 1.0], np.float32), shape)
    g[rng.random(shape) < 0.125] = 0.0
    return p, g


@functools.lru_cache(maxsize=None)
def state(shape, seed, step=1):
    """(p, g, m, v) in fp32 as a step-`step` call finds them (read-only, shared)"""
    rng = np.random.default_rng(seed)
    p, g = draw(rng, shape)
    m, v = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
    for s in range(1, step):
        p, m, v = (a.astype(np.float32) for a in ref.adam(p, g, m, v, s, **HP))
        _, g = draw(rng, shape)
    for a in (p, g, m, v):
        a.setflags(write=False)
    return p, g, m, v


def make_plane(shape, seed):
    """uniform in [-1, 1] with exact +0.0 and -0.0 texels, all values distinct between seeds"""
    plane = np.random.default_rng(seed).uniform(-1, 1, shape).astype(np.float32)
    flat = plane.reshape(-1)
    flat[1::5] = 0.0
    flat[3::11] = -0.0
    return plane


# ---- bounds

def adam_bounds(p, g, m, v, step, g_mag=None, kg=0):
    """yardstick (p', m', v') and the bounds (ep, em, ev) of the module docstring; g is the float64 gradient that reaches Adam, g_mag
    the sum of the magnitudes of its terms and kg the fp32 roundings already in it (0: g is an input)"""
    lr, b1, b2, eps, wd = (HP[k] for k in ("lr", "b1", "b2", "eps", "wd"))
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    pn, mn, vn = ref.adam(p, g, m, v, step, **HP)
    G = (np.abs(g) if g_mag is None else g_mag) + np.abs(wd * p)
    em = gam(kg + 5) * (np.abs(m) + (1.0 - b1) * (G + np.abs(m)))
    ev = gam(2 * kg + 7) * (b2 * np.abs(v) + (1.0 - b2) * G * G)
    c2 = math.sqrt(1.0 - b2 ** step)
    A = lr / (1.0 - b1 ** step)
    s = np.sqrt(vn)
    s_hi = np.sqrt(vn + ev)
    es = np.maximum(s_hi - s, s - np.sqrt(np.maximum(vn - ev, 0.0))) + U * s_hi
    D = s / c2 + eps
    eD = (es / c2) * (1.0 + gam(3)) + gam(3) * (D + es / c2)
    D_lo = np.maximum(D - eD, eps)
    q = np.abs(mn) / D
    eq = em / D_lo + np.abs(mn) * eD / (D * D_lo) + U * (np.abs(mn) + em) / D_lo
    eu = A * eq * (1.0 + gam(3)) + gam(3) * A * q
    ep = eu + U * (np.abs(p) + A * q + eu)
    return (pn, mn, vn), (ep, em, ev)


def ratio(what, got, want, bound):
    """asserts |got - want| <= bound at EVERY index; returns the worst err / bound"""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == np.shape(want), (what, got.shape, np.shape(want))
    if got.size == 0:
        return 0.0
    assert np.isfinite(got).all(), f"{what}: non-finite values at {np.flatnonzero(~np.isfinite(got).reshape(-1))[:8]}"
    err = np.abs(got - want)
    bad = np.flatnonzero((err > bound).reshape(-1))
    r = float((err / np.maximum(bound, 1e-300)).max())
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} elements outside the bound, first at flat index {bad[:8]}, worst err / bound {r:.3g}"
    return r


def check_adam(what, got, p, g, m, v, step, g_mag=None, kg=0, loose_share=0.0):
    (pn, mn, vn), (ep, em, ev) = adam_bounds(p, g, m, v, step, g_mag, kg)
    rm, rv, rp = ratio(what + " m", got[1], mn, em), ratio(what + " v", got[2], vn, ev), ratio(what + " p", got[0], pn, ep)
    moved = np.abs(pn - np.asarray(p, dtype=np.float64))
    loose = float(np.mean(ep > 0.01 * HP["lr"])) if ep.size else 0.0       # a bound worth more than 1 % of an update says little
    assert loose <= loose_share, f"{what}: {loose:.4f} of the p bounds are loose"
    return dict(p=rp, m=rm, v=rv, loose=loose, moved=float(moved.min()) if moved.size else 0.0)


def rounds(n4, cap):
    return max(1, -(-n4 // (256 * min(-(-n4 // 256), cap))))


def sums_bound(sums, n4, r):
    s = np.abs(np.asarray(sums, dtype=np.float64))
    return np.stack([(gam(6 + r) + n4 * 2.0 ** -53) * s[..., 0], (gam(6 + r) + n4 * 2.0 ** -53) * s[..., 1],
                     (gam(3 + r) + n4 * 2.0 ** -53) * s[..., 2]], axis=-1)


def reg_grad_bound(plane, g0, cy, cx, cl1, up, rows=None):
    r0, r1 = rows or (0, plane.shape[0])
    return gam(7) * (np.abs(np.asarray(g0, dtype=np.float64)[r0:r1]) + ref.plane_reg_magnitude(plane, cy, cx, cl1, up, rows))


# ---- device plumbing

def padded(a, fill=None):
    """device buffer of a.size + PAD floats: the array (or `fill`) followed by the sentinel"""
    t = torch.full((a.size + PAD,), SENTINEL, device=DEV, dtype=torch.float32)
    if a.size:
        t[:a.size] = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(DEV) if fill is None else fill
    return t


def unpad(t, shape, what="buffer"):
    h = t.cpu().numpy()
    assert np.all(h[-PAD:] == SENTINEL), f"{what}: written past its end"
    return h[:-PAD].reshape(shape)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


class Buffers:
    """p, g, m, v of one tensor on the device"""
    def __init__(self, p, g, m, v):
        self.shape = p.shape
        self.t = [padded(a) for a in (p, g, m, v)]

    def load(self, p, g, m, v):
        for t, a in zip(self.t, (p, g, m, v)):
            if a.size:
                t[:a.size] = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(DEV)

    def host(self):
        return [unpad(t, self.shape, n) for t, n in zip(self.t, "pgmv")]


def adam_items(bufs):
    from tinynerf_amd import _lib as L
    items = (L.AdamItem * len(bufs))()
    for it, b in zip(items, bufs):
        n = int(np.prod(b.shape))
        it.param, it.grad, it.exp_avg, it.exp_avg_sq = [t.data_ptr() if n else None for t in b.t]
        it.n = n
    return items


def call_multi(form, items, count, step, zero_grad, step_dev=None, gate=None):
    from tinynerf_amd import _lib as L
    if form == "multi":
        L.call("tn_adam_multi", torch.device(DEV), items, C.c_int32(count), *hp_args(), C.c_int32(step), C.c_int32(zero_grad & 1))
    else:
        L.call("tn_adam_multi_gated", torch.device(DEV), items, C.c_int32(count), *hp_args(), L.ptr(step_dev), L.ptr(gate), C.c_int32(zero_grad))


def check_grad_buffer(what, got, before, zeroed):
    if zeroed:
        assert np.all(bits(got) == 0), f"{what}: gradient not zeroed (to +0.0) everywhere"
    else:
        assert np.array_equal(bits(got), bits(before)), f"{what}: gradient changed without zero_grad"


# ---- 1. rounds and tails

@pytest.mark.parametrize("zero_grad", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 6, 7, 1023, 2100003])
def test_adam_step_every_element_once(n, zero_grad):
    """tn_adam_step: n = 2 100 003 is 525 001 float4 -- above the 2048 x 256 threads, so the loop's second round runs, and its last
    float4 is a tail of 3"""
    from tinynerf_amd import _lib as L
    worst = {}
    for step in (1, 3):
        p, g, m, v = state((n,), 100 + n % 1000, step)
        b = Buffers(p, g, m, v)
        L.call("tn_adam_step", torch.device(DEV), *[L.ptr(t) for t in b.t], C.c_int64(n), *hp_args(), C.c_int32(step), C.c_int32(zero_grad))
        gp, gg, gm, gv = b.host()
        r = check_adam(f"tn_adam_step n={n} step={step}", (gp, gm, gv), p, g, m, v, step)
        check_grad_buffer(f"tn_adam_step n={n}", gg, g, zero_grad)
        assert step > 1 or r["moved"] > 0.9 * HP["lr"]    # the first update moves every element by lr: one left alone is far outside
        worst = {k: max(r[k], worst.get(k, 0.0)) for k in "pmv"}
    print(f"tn_adam_step n={n} zero_grad={zero_grad}: worst err / bound p {worst['p']:.3f} m {worst['m']:.3f} v {worst['v']:.3f}")


MULTI_SIZES = (1048576 + 7, 3, 2, 1, 0, 4099)


@pytest.mark.parametrize("form", ["multi", "gated"])
def test_adam_multi_second_round_in_one_item_tails_and_an_empty_item(form):
    """one launch: 262 146 float4 in item 0 against 1024 x 256 threads (second round, tail 3) while the other blocks' items are
    long finished; tails 3, 2, 1; an empty item with null pointers"""
    step = 2
    data = [state((n,), 200 + i, step) for i, n in enumerate(MULTI_SIZES)]
    bufs = [Buffers(*d) for d in data]
    step_dev = torch.tensor([step - 1, 0], dtype=torch.int32, device=DEV)
    gate = torch.tensor([0.5], device=DEV)
    call_multi(form, adam_items(bufs), len(bufs), step, 3 if form == "gated" else 1, step_dev, gate)
    worst = {}
    for n, d, b in zip(MULTI_SIZES, data, bufs):
        gp, gg, gm, gv = b.host()
        r = check_adam(f"{form} n={n}", (gp, gm, gv), *d, step)
        check_grad_buffer(f"{form} n={n}", gg, d[1], True)
        worst = {k: max(r[k], worst.get(k, 0.0)) for k in "pmv"}
    if form == "gated":
        assert step_dev.cpu().tolist() == [step, 0]
    print(f"tn_adam_{form} rounds and tails: worst err / bound p {worst['p']:.3f} m {worst['m']:.3f} v {worst['v']:.3f}")


# ---- 2. chunking past TN_MULTI_MAX

@pytest.mark.parametrize("form", ["multi", "gated"])
def test_adam_multi_seventy_items_two_steps(form):
    """70 items are three launches (32 + 32 + 6); the gated form advances the device count ONCE per call, before all of them"""
    sizes = [1 + (7 * i) % 40 for i in range(70)]
    assert min(sizes) == 1 and max(sizes) == 40
    first = [state((n,), 300 + i, 1) for i, n in enumerate(sizes)]
    second = [state((n,), 300 + i, 2) for i, n in enumerate(sizes)]
    bufs = [Buffers(*d) for d in first]
    items = adam_items(bufs)
    step_dev = torch.zeros(2, dtype=torch.int32, device=DEV)
    gate = torch.tensor([1.0], device=DEV)
    worst = {}
    for step, data in ((1, first), (2, second)):
        for b, d in zip(bufs, data):
            b.load(*d)                                    # step 2 starts from the yardstick's step 1, rounded to fp32
        call_multi(form, items, 70, step, 3 if form == "gated" else 1, step_dev, gate)
        for i, (d, b) in enumerate(zip(data, bufs)):
            gp, gg, gm, gv = b.host()
            r = check_adam(f"{form} item {i} step {step}", (gp, gm, gv), *d, step)
            check_grad_buffer(f"{form} item {i}", gg, d[1], True)
            worst = {k: max(r[k], worst.get(k, 0.0)) for k in "pmv"}
        if form == "gated":
            assert step_dev.cpu().tolist() == [step, 0]
    print(f"tn_adam_{form} 70 items: worst err / bound p {worst['p']:.3f} m {worst['m']:.3f} v {worst['v']:.3f}")


def test_plane_reg_multi_thirty_five_planes_keep_their_slots():
    from tinynerf_amd import _lib as L
    shape, n = (4, 5, 4), 35
    planes = [make_plane(shape, 400 + i) * np.float32(1 + i % 3) for i in range(n)]
    g0 = [np.random.default_rng(450 + i).uniform(-2, 2, shape).astype(np.float32) for i in range(n)]
    cy, cx, cl1 = COEFS[0]
    dp, dg = [padded(a) for a in planes], [padded(a) for a in g0]
    sums = torch.zeros((n, 3), dtype=torch.float64, device=DEV)
    items = (L.PlaneRegItem * n)()
    for it, a, b in zip(items, dp, dg):
        it.plane, it.grad, it.H, it.W, it.C, it.cy, it.cx, it.cl1 = a.data_ptr(), b.data_ptr(), *shape, cy, cx, cl1
    L.call("tn_plane_reg_multi", torch.device(DEV), items, C.c_int32(n), C.c_float(UP), L.ptr(sums))
    want = [ref.plane_reg(a, cy, cx, cl1, UP) for a in planes]
    want_sums = np.stack([s for s, _ in want])
    assert len({tuple(np.round(s, 6)) for s in want_sums}) == n          # distinct planes: a sum in the wrong slot cannot pass
    rs = ratio("35 planes' sums", sums.cpu().numpy(), want_sums, sums_bound(want_sums, 20, 1))
    rg = max(ratio(f"plane {i} gradient", unpad(dg[i], shape), g0[i].astype(np.float64) + want[i][1], reg_grad_bound(planes[i], g0[i], cy, cx, cl1, UP))
             for i in range(n))
    for i in range(n):
        assert np.array_equal(bits(unpad(dp[i], shape)), bits(planes[i]))
    print(f"tn_plane_reg_multi 35 planes: worst err / bound sums {rs:.3f} gradient {rg:.3f}")


def reg_items(entries):
    """entries: dicts with device buffers p, po, g, m, v and shape / n, slot, coef, rows"""
    from tinynerf_amd import _lib as L
    items = (L.AdamRegItem * len(entries))()
    for it, e in zip(items, entries):
        it.param, it.param_out, it.grad, it.exp_avg, it.exp_avg_sq = [e[k].data_ptr() for k in ("p", "po", "g", "m", "v")]
        if e.get("shape") is not None:
            it.H, it.W, it.C = e["shape"]
            it.n = int(np.prod(e["shape"]))
            it.cy, it.cx, it.cl1 = e["coef"]
            it.sum_slot = e.get("slot", 0)
            it.row0, it.row1 = e.get("rows") or (0, 0)
        else:
            it.n = e["n"]
    return items


def call_reg(items, count, step, zero_grad, sums):
    from tinynerf_amd import _lib as L
    L.call("tn_adam_reg_multi", torch.device(DEV), items, C.c_int32(count), *hp_args(), C.c_int32(step), C.c_int32(zero_grad), C.c_float(UP),
           L.ptr(sums))


def plane_entry(shape, seed, step, coef, slot=0, rows=None):
    """a regularised item: host inputs under "in", device buffers, param_out pre-filled with NaN"""
    n = int(np.prod(shape))
    _, g, m, v = state(shape, seed, step)
    p = make_plane(shape, seed)
    return dict(shape=shape, coef=coef, slot=slot, rows=rows, **{"in": (p, g, m, v)}, p=padded(p), po=padded(p, fill=float("nan")), g=padded(g),
                m=padded(m), v=padded(v), n=n)


def check_plane_entry(what, e, step, zero_grad, loose_share=0.01):
    """the owned rows against the yardstick, everything outside them untouched; returns the ratios and the yardstick's sums"""
    p, g, m, v = e["in"]
    shape, (cy, cx, cl1) = e["shape"], e["coef"]
    H = shape[0]
    r0, r1 = e["rows"] or (0, H)
    own = slice(r0, r1)
    sums, rg = ref.plane_reg(p, cy, cx, cl1, UP, (r0, r1))
    g_total = g[own].astype(np.float64) + rg
    g_mag = np.abs(g[own].astype(np.float64)) + ref.plane_reg_magnitude(p, cy, cx, cl1, UP, (r0, r1))
    po, gm, gv = unpad(e["po"], shape, "param_out"), unpad(e["m"], shape, "exp_avg"), unpad(e["v"], shape, "exp_avg_sq")
    r = check_adam(what, (po[own], gm[own], gv[own]), p[own], g_total, m[own], v[own], step, g_mag, kg=7,
                   loose_share=max(loose_share, 2.0 / g_total.size))
    outside = np.ones(H, bool)
    outside[own] = False
    assert np.isnan(po[outside]).all(), f"{what}: param_out written outside rows [{r0}, {r1})"
    assert np.array_equal(bits(gm[outside]), bits(m[outside])) and np.array_equal(bits(gv[outside]), bits(v[outside])), f"{what}: moments changed outside the rows"
    assert np.array_equal(bits(unpad(e["p"], shape, "param")), bits(p)), f"{what}: param (the input buffer) changed"
    check_grad_buffer(what, unpad(e["g"], shape, "grad"), g, zero_grad)
    return r, sums


def test_adam_reg_multi_twenty_planes_permuted_slots_and_plain_tensors():
    """23 items are two launches of 16 + 7; `sums` is indexed by the absolute sum_slot, here a permutation; the plain items (H == 0)
    have tails and update in place"""
    step = 2
    slots = [(7 * i + 3) % 20 for i in range(20)]
    assert sorted(slots) == list(range(20)) and slots != list(range(20))
    entries = [plane_entry((4, 5, 4), 500 + i, step, COEFS[i % 2], slot=slots[i]) for i in range(20)]
    plain_sizes = (7, 5, 1)
    plain = [state((n,), 550 + n, step) for n in plain_sizes]
    pb = [Buffers(*d) for d in plain]
    order = entries[:9] + [dict(p=b.t[0], po=b.t[0], g=b.t[1], m=b.t[2], v=b.t[3], n=n) for b, n in zip(pb, plain_sizes)] + entries[9:]
    sums = torch.zeros((20, 3), dtype=torch.float64, device=DEV)
    call_reg(reg_items(order), len(order), step, 1, sums)
    got_sums = sums.cpu().numpy()
    worst, ws = {}, 0.0
    for i, e in enumerate(entries):
        r, want = check_plane_entry(f"plane {i} (slot {slots[i]})", e, step, 1)
        ws = max(ws, ratio(f"plane {i} sums in slot {slots[i]}", got_sums[slots[i]], want, sums_bound(want, 20, 1)))
        worst = {k: max(r[k], worst.get(k, 0.0)) for k in "pmv"}
    for d, b, n in zip(plain, pb, plain_sizes):
        gp, gg, gm, gv = b.host()
        r = check_adam(f"plain item n={n}", (gp, gm, gv), *d, step)
        check_grad_buffer(f"plain item n={n}", gg, d[1], True)
        worst = {k: max(r[k], worst.get(k, 0.0)) for k in "pmv"}
    print(f"tn_adam_reg_multi 23 items: worst err / bound p {worst['p']:.3f} m {worst['m']:.3f} v {worst['v']:.3f} sums {ws:.3f}")


# ---- 3. the regulariser through all three entry points

SMALL_SHAPES = [(1, 9, 4), (9, 1, 4), (2, 2, 4), (33, 17, 32), (5, 7, 8)]
REG_CASES = [(s, c) for s in SMALL_SHAPES for c in (0, 1)]


@pytest.mark.parametrize("shape,coef", REG_CASES + [((260, 260, 32), 0)])
def test_plane_reg_fwd_and_bwd(shape, coef):
    """tn_plane_reg_fwd adds to what `sums` holds, tn_plane_reg_bwd to what `grad` holds; 260 x 260 x 8 float4 is above 2048 x 256
    threads"""
    from tinynerf_amd import _lib as L
    cy, cx, cl1 = COEFS[coef]
    H, W, Cc = shape
    n4 = H * W * Cc // 4
    assert (rounds(n4, 2048) == 2) == (shape[0] == 260)
    plane = make_plane(shape, 600 + H)
    g0 = np.random.default_rng(601 + H).uniform(-2, 2, shape).astype(np.float32)
    want_sums, want_grad = ref.plane_reg(plane, cy, cx, cl1, UP)
    dp, dg = padded(plane), padded(g0)
    init = np.array([1.5, 2.5, 3.5])
    sums = torch.from_numpy(init.copy()).to(DEV)
    up = torch.tensor([UP], device=DEV)
    L.call("tn_plane_reg_fwd", torch.device(DEV), L.ptr(dp), C.c_int(H), C.c_int(W), C.c_int(Cc), L.ptr(sums))
    L.call("tn_plane_reg_bwd", torch.device(DEV), L.ptr(dp), C.c_int(H), C.c_int(W), C.c_int(Cc), C.c_float(cy), C.c_float(cx), C.c_float(cl1),
           L.ptr(up), L.ptr(dg))
    rs = ratio("sums", sums.cpu().numpy(), init + want_sums, sums_bound(init + want_sums, n4, 0))
    got = unpad(dg, shape, "grad")
    rg = ratio("gradient", got, g0.astype(np.float64) + want_grad, reg_grad_bound(plane, g0, cy, cx, cl1, UP))
    assert np.array_equal(bits(unpad(dp, shape, "plane")), bits(plane))
    check_zero_texels(plane, cl1)
    print(f"tn_plane_reg_fwd/_bwd {shape} cl1={cl1:g}: worst err / bound sums {rs:.3f} gradient {rg:.3f}")


def check_zero_texels(plane, cl1):
    """a +0.0 and a -0.0 texel get the same L1 gradient, 0: with only the L1 term, their gradient keeps its bits"""
    zero = plane == 0
    assert np.signbit(plane[zero]).any() and not np.signbit(plane[zero]).all()
    if cl1 != 0:
        only_l1 = ref.plane_reg(plane, 0.0, 0.0, cl1, UP)[1]
        assert np.all(only_l1[zero] == 0) and np.all(np.abs(only_l1[~zero]) == abs(cl1) * UP)


@pytest.mark.parametrize("shape,coef", REG_CASES + [((192, 192, 32), 0)])
def test_plane_reg_multi_one_plane(shape, coef):
    """gradient and sums; grad == NULL leaves only the sums, sums == NULL only the gradient; 192 x 192 x 8 float4 is above 1024 x 256
    threads"""
    from tinynerf_amd import _lib as L
    cy, cx, cl1 = COEFS[coef]
    H, W, Cc = shape
    n4 = H * W * Cc // 4
    R = rounds(n4, 1024)
    assert (R == 2) == (shape[0] == 192)
    plane = make_plane(shape, 700 + H)
    g0 = np.random.default_rng(701 + H).uniform(-2, 2, shape).astype(np.float32)
    want_sums, want_grad = ref.plane_reg(plane, cy, cx, cl1, UP)
    dp = padded(plane)

    def run(with_grad, with_sums):
        dg = padded(g0)
        sums = torch.full((3,), -5.0, dtype=torch.float64, device=DEV)
        items = (L.PlaneRegItem * 1)()
        it = items[0]
        it.plane, it.grad, it.H, it.W, it.C, it.cy, it.cx, it.cl1 = dp.data_ptr(), dg.data_ptr() if with_grad else None, H, W, Cc, cy, cx, cl1
        L.call("tn_plane_reg_multi", torch.device(DEV), items, C.c_int32(1), C.c_float(UP), L.ptr(sums) if with_sums else C.c_void_p(None))
        return unpad(dg, shape, "grad"), sums.cpu().numpy() + 5.0

    both_g, both_s = run(True, True)
    rs = ratio("sums", both_s, want_sums, sums_bound(want_sums, n4, R) + 5.0 * 2.0 ** -52)
    rg = ratio("gradient", both_g, g0.astype(np.float64) + want_grad, reg_grad_bound(plane, g0, cy, cx, cl1, UP))
    g_only, s_none = run(True, False)
    assert np.array_equal(bits(g_only), bits(both_g)) and np.all(s_none == 0.0)          # the sums buffer that was not passed kept -5
    g_none, s_only = run(False, True)
    assert np.array_equal(bits(g_none), bits(g0))
    ratio("sums without a gradient", s_only, want_sums, sums_bound(want_sums, n4, R) + 5.0 * 2.0 ** -52)
    assert np.array_equal(bits(unpad(dp, shape, "plane")), bits(plane))
    check_zero_texels(plane, cl1)
    print(f"tn_plane_reg_multi {shape} cl1={cl1:g}: worst err / bound sums {rs:.3f} gradient {rg:.3f}")


@pytest.mark.parametrize("zero_grad", [0, 1])
@pytest.mark.parametrize("shape,coef", REG_CASES + [((192, 192, 32), 0)])
def test_adam_reg_multi_one_plane(shape, coef, zero_grad):
    step = 1 + coef                                       # zero moments with the first coefficients, the yardstick's step 1 with the second
    e = plane_entry(shape, 800 + shape[0], step, COEFS[coef])
    n4 = e["n"] // 4
    sums = torch.zeros(3, dtype=torch.float64, device=DEV)
    call_reg(reg_items([e]), 1, step, zero_grad, sums)
    r, want = check_plane_entry(f"adam_reg {shape}", e, step, zero_grad)
    rs = ratio("sums", sums.cpu().numpy(), want, sums_bound(want, n4, rounds(n4, 1024)))
    # sums == NULL: the same update, bit for bit
    e2 = plane_entry(shape, 800 + shape[0], step, COEFS[coef])
    call_reg(reg_items([e2]), 1, step, zero_grad, None)
    for k in ("po", "m", "v"):
        assert np.array_equal(bits(unpad(e2[k], shape)), bits(unpad(e[k], shape)))
    print(f"tn_adam_reg_multi {shape} cl1={COEFS[coef][2]:g} step={step}: worst err / bound p {r['p']:.3f} m {r['m']:.3f} v {r['v']:.3f} sums {rs:.3f}, "
          f"loose p bounds {r['loose']:.4f}")


# ---- 4. the row-sharded pass

PARTITIONS = {
    (13, 6, 8): [[(0, 13)], [(0, 1), (1, 13)], [(0, 12), (12, 13)], [(0, 4), (4, 9), (9, 13)]],
    (192, 192, 32): [[(0, 67), (67, 68), (68, 192)]],                     # three unequal ranges, one of a single row
}


@pytest.mark.parametrize("shape", sorted(PARTITIONS))
def test_row_sharded_pass_at_the_seams(shape):
    """each range is its own call on fresh copies of the same inputs (so the stencil at a seam reads the neighbour's CURRENT rows);
    the unsharded call (row0 == row1 == 0) is what every range must reproduce bit for bit inside its rows"""
    step, coef = 2, COEFS[0]
    n4 = int(np.prod(shape)) // 4
    R = rounds(n4, 1024)

    def run(rows):
        e = plane_entry(shape, 900, step, coef, rows=rows)
        sums = torch.zeros(3, dtype=torch.float64, device=DEV)
        call_reg(reg_items([e]), 1, step, 1, sums)
        return e, sums.cpu().numpy()

    full, full_sums = run(None)
    _, want_full = check_plane_entry(f"unsharded {shape}", full, step, 1)
    ratio("unsharded sums", full_sums, want_full, sums_bound(want_full, n4, R))
    full_host = {k: unpad(full[k], shape) for k in ("po", "m", "v")}
    worst, ws, wadd = {}, 0.0, 0.0
    for part in PARTITIONS[shape]:
        total = np.zeros(3)
        for rows in part:
            e, s = run(rows)
            r, want = check_plane_entry(f"rows {rows} of {shape}", e, step, 1)         # inside: the yardstick; outside: untouched, gradient zero
            ws = max(ws, ratio(f"rows {rows} sums", s, want, sums_bound(want, n4, R)))
            own = slice(*rows)
            for k in ("po", "m", "v"):
                assert np.array_equal(bits(unpad(e[k], shape)[own]), bits(full_host[k][own])), f"rows {rows}: {k} differs from the unsharded call's bits"
            total += s
            worst = {k: max(r[k], worst.get(k, 0.0)) for k in "pmv"}
        # the pair (y, y + 1) across a seam is counted by exactly one owner, |p| and the x pairs by the row's owner
        seam = ((gam(1) if R > 1 else 0.0) + (n4 + 3 * len(part)) * 2.0 ** -53) * np.abs(want_full)
        wadd = max(wadd, ratio(f"sums of the ranges {part}", total, full_sums, seam))
    print(f"row-sharded {shape}: worst err / bound p {worst['p']:.3f} m {worst['m']:.3f} v {worst['v']:.3f} sums {ws:.3f}, ranges add up to the full sums "
          f"within {wadd:.3f} of the bound")


# ---- 5. the gate

GATE_SIZES = (4099, 3, 64)


def gate_setup(step, count):
    data = [state((n,), 1000 + n, step) for n in GATE_SIZES]
    bufs = [Buffers(*d) for d in data]
    return data, bufs, adam_items(bufs), torch.tensor([count, 0], dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("zero_grad", [0, 1, 2, 3])
@pytest.mark.parametrize("gate_value", [0.0, -1.0, float("nan")])
def test_closed_gate_changes_nothing_but_the_gradients(gate_value, zero_grad):
    data, bufs, items, step_dev = gate_setup(2, 1)
    gate = torch.tensor([gate_value], device=DEV)
    call_multi("gated", items, len(bufs), None, zero_grad, step_dev, gate)
    for d, b in zip(data, bufs):
        gp, gg, gm, gv = b.host()
        for name, got, before in (("p", gp, d[0]), ("m", gm, d[2]), ("v", gv, d[3])):
            assert np.array_equal(bits(got), bits(before)), f"closed gate {gate_value}: {name} changed"
        check_grad_buffer(f"closed gate {gate_value}", gg, d[1], zero_grad & 1)
    assert step_dev.cpu().tolist() == [1, 0]


def test_gate_open_closed_closed_open_counts_open_steps():
    """the fourth call is the second update: its bias correction is that of step 2 (1 - 0.9^2 = 0.19 against 1 - 0.9^4 = 0.34: a count
    of calls moves every element by about half an update too little)"""
    first = [state((n,), 1000 + n, 1) for n in GATE_SIZES]
    second = [state((n,), 1000 + n, 2) for n in GATE_SIZES]
    bufs = [Buffers(*d) for d in first]
    items = adam_items(bufs)
    step_dev = torch.zeros(2, dtype=torch.int32, device=DEV)
    opened, closed = torch.tensor([0.25], device=DEV), torch.tensor([0.0], device=DEV)
    worst = {}
    for call, (gate, data, step) in enumerate([(opened, first, 1), (closed, second, 1), (closed, second, 1), (opened, second, 2)]):
        for b, d in zip(bufs, data):
            b.load(*d)
        call_multi("gated", items, len(bufs), None, 3, step_dev, gate)
        assert step_dev.cpu().tolist() == [step, 0], f"after call {call}"
        for n, d, b in zip(GATE_SIZES, data, bufs):
            gp, gg, gm, gv = b.host()
            check_grad_buffer(f"call {call}", gg, d[1], True)
            if gate is closed:
                assert all(np.array_equal(bits(a), bits(c)) for a, c in ((gp, d[0]), (gm, d[2]), (gv, d[3])))
            else:
                r = check_adam(f"call {call} n={n} (step {step})", (gp, gm, gv), *d, step)
                worst = {k: max(r[k], worst.get(k, 0.0)) for k in "pmv"}
    print(f"gate open, closed, closed, open: worst err / bound p {worst['p']:.3f} m {worst['m']:.3f} v {worst['v']:.3f}")


@pytest.mark.parametrize("zero_grad", [1, 3])
def test_nonfinite_flag_is_raised_by_an_infinite_gradient_only_when_asked_for(zero_grad):
    """step_dev[1] exists only under zero_grad bit 1; an inf gradient (an input value) makes that element's update NaN"""
    data, bufs, items, step_dev = gate_setup(2, 1)
    at = 2050                                             # in the middle of the 4099-element tensor
    bufs[0].t[1][at] = float("inf")
    call_multi("gated", items, len(bufs), None, zero_grad, step_dev, torch.tensor([1.0], device=DEV))
    assert step_dev.cpu().tolist() == [2, 1 if zero_grad & 2 else 0]
    keep = np.ones(GATE_SIZES[0], bool)
    keep[at] = False
    worst = {}
    for i, (d, b) in enumerate(zip(data, bufs)):
        gp, gg, gm, gv = b.host()
        sel = keep if i == 0 else slice(None)
        if i == 0:
            assert not np.isfinite(gp[at])
        r = check_adam(f"flag n={GATE_SIZES[i]}", (gp[sel], gm[sel], gv[sel]), *[a[sel] for a in d], 2)
        check_grad_buffer("flag", gg, d[1], True)
        worst = {k: max(r[k], worst.get(k, 0.0)) for k in "pmv"}
    print(f"non-finite flag zero_grad={zero_grad}: worst err / bound p {worst['p']:.3f} m {worst['m']:.3f} v {worst['v']:.3f}")
