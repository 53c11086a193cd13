"""fp64 yardstick of the volume-rendering kernels of csrc/weights.hip, the bounds an fp32 evaluation in the kernels' order is entitled
to, and the deterministic fixtures both are used on (numpy, no GPU).

Kernels: tn_weights_fwd(_gate), tn_weights_bwd, tn_composite_fwd / _bwd, tn_render_rays_fwd / _bwd / _bwd_dw, tn_mse_grad(_gated).
Inputs are taken as the fp32 values the kernels receive (the threshold included); everything behind that is fp64.

References
  weights        w_k = T_k (1 - a_k), T_k = prod_{j<k} a_j, a = exp(-sigma step); everything from the first k with !(T_k > thr) on is 0.
                 An alpha below 2^-150 (half the smallest fp32 subnormal, p > 104) is 0 here as in every fp32 evaluation.
  weights_grad   step_k (T_{k+1} g_k - sum_{j>k} w_j g_j), T unterminated, suffix sums formed directly, w as passed.
  composite      sum_k w_k rgb_k (+ bg (1 - sum_k w_k)); a sample with w == 0 contributes no colour and its rgb is never read.
  composite_grad grad_rgb = w g (one product of two fp32 numbers: exact in fp64, so the kernel's value is its fp32 rounding, bit for
                 bit), grad_w = <rgb, g> - <bg, g> (+ extra), the first term 0 where w == 0.
  mse            grad = fl(fl(r - t) fl(c c_dev)) in fp32, bit for bit, c = 0 behind a closed gate (0, negative, NaN); sumsq fp64.

Bounds.  u = 2^-24.  E = EXPF_ULPS bounds the device expf in ulps; one alpha a_j = expf(fl(-sigma_j step_j)) then has the relative
error eps_j = (p_j + 2 E) u: the product's rounding moves the exponent by p u, and E ulps are at most 2 E u of the value.

  r_T(m), the fp32 multiplications on the path of T_m (m = 64 c + l: chunk c, lane l):
    7 per finished chunk: wave_scan_mul's six steps on lane 63 (wave_scan, weights.hip:56-59) and the carry update `carry * wave_last(incl)`
    (:148; in the backward `T *= wave_last(pt)`, :209, both paths);
    inside the chunk, for l > 0, the scan steps o <= l - 1 that lane l - 1 takes part in, bit_length(l - 1) of them (:58), and
    `carry * wave_excl(incl)` (:143).  Lane 0 multiplies the carry by 1.
    The backward's T_{k+1} is `T * pt` of the INCLUSIVE scan of lane l (:207): 7 c + bit_length(l) + 1, which is r_T(k + 1).
  forward   |w - w_ref| <= T_ref a_ref eps_k + w_ref (sum_{j<k} eps_j + r_T(k) u + u): alpha's own error acts on 1 - a through T a; T
            carries the alphas before it and its multiplications; the fp64 product T (1 - a) is rounded to fp32 once (:147).
            w is exactly 0 where w_ref is.  The same sum bounds T itself: |T - T_ref| <= T_ref (sum_{j<k} eps_j + r_T(k) u), and a ray
            on which some T_ref,k lies that close to the threshold is a "danger ray" -- the fixtures hold none (danger_rays).
  backward  |gs - gs_ref| <= step_k u [c_add(count) A_ray + (sum_{j<=k} eps_j / u + r_T(k + 1) + 3) T_{k+1} |g_k|],
            A_ray = sum_j |w_j g_j|.  The 3: the product with g, the final addition and the product with the step (:207).
            c_add, the fp32 operations on the path of one term through -total + prefix, nch = ceil(count / 64):
              register path (count <= 1024): the product w g (:200) 1; the lane's partial sum (:219; its 16 - nch other additions add an
              exact 0) nch; wave_sum (tn_common.h:38) 6; wave_scan_add (:56-59) 6; `acc += wave_last(ps)` (:208) nch; `acc + ps`,
              the final addition and the product with the step (:207) 3: 2 nch + 16, nch <= 16;
              streaming path: the product and the lane's partial sum (:226) 1 + nch; wave_sum 6; wave_scan_add 6; the carry (:208) nch;
              :207 3: 2 nch + 16 with nch unbounded.
  composite (m + r) u sum|terms|.  A lane sums nch products (Composite::add, :82, in both forms) and wave_sum adds 6 levels (:90): the opacity
            has m = nch + 6, r = 0; a colour without bg m = nch + 6 and r = 1 (the product); with bg the longest path is a weight's
            through the opacity (nch + 6), `1 - o`, the product with bg and the final addition (:92): m = nch + 7, r = 2, and
            sum|terms| holds |bg| (1 + sum |w|).  grad_w: three products, two additions, the subtraction of gbg (:113-114): m = 3,
            r = 1 on sum_c |rgb_c g_c| + sum_c |bg_c g_c|; tn_render_rays_bwd_dw's extra is one more addition (:188): m = 4 and
            |extra| joins the terms.
  fused     tn_render_rays_fwd composites with its own weights: those are held to the forward bound, and `rendered` to the composite
            of the weights the launch wrote, with the composite's bound.  tn_render_rays_bwd(_dw) feeds grad_w to the backward unrounded by any store: with G_j = sum|terms| of
            grad_w_j and r_g = m + r of it (4, or 5 with extra), the backward bound holds with |g| -> G, A_ray = sum_j |w_j| G_j,
            c_add + r_g and 3 + r_g.
  sumsq     a thread adds its m = ceil(n / (blocks 256)) squares with fmaf in fp32 (:281), blocks = min(ceil(n / 256), 512) (:578);
            d = fl(r - t) is squared: r = 2.  Lanes, waves and blocks are added in fp64 (:283-289): 2^-50 (sum + |start|) on top.

EXPF_ULPS = 1.  Unverified: OCML is believed to document 1 ulp for the fp32 exp.  The constant is NOT tuned on the multi-sample
fixtures.  Every fixture stayed inside its bounds on an MI355X with E = 1 (the table in tests/test_hip_render.py), so it did not move
and the measurement the single-sample rays allow was not needed to set it.  expf_ulps_single() makes it all the same, on the
`singles` fixture (67 rays of one sample, p < ln 2): there w = fl(1 - a), so a_gpu is known to half an ulp of w, and the function
returns an interval for max |a_gpu - exp(-fl(p))| in ulps of a -- what is left beyond the rounding of w, and that plus the rounding.
It is no accuracy claim for expf: the lower end only says that no excess over the rounding of w was seen.
Note on r_T: it counts the multiplications on the PATH of T_k (the scan's depth, at most 7 per chunk), as a sum's bound counts
additions.  But relative errors of a product add over EVERY factor: the expression tree of T_k holds about k multiplications, one per
alpha, each with its own rounding u.  The form of the bound leaves those to the 2 E u that each alpha is granted for expf.  So the
forward bound is rigorous only for an expf that stays about u (half an ulp at worst) inside its E ulps; an expf that really used a
full ulp on every sample could push a CORRECT kernel past it (the fp32 restatement on the CPU, whose numpy exp errs by up to ~2 ulp
near 1, reaches 0.92 of it).  A failure of the forward bound by a small factor on long rays, with the zero set intact, is to be read
with that in mind before the kernel is blamed.

Fixtures (fixture(name), FIXTURES): deterministic, at most ~300 rays and 40 000 samples each.  Lengths 0, 1, 2, 63, 64, 65, 127, 128,
129, 1023, 1024, 1025 and 2100; ray counts 1, 3, 4, 5, 9 (WAVES_PER_BLOCK = 4: a partial last block); empty rays at the front, in the
middle and at the end; all-empty batches; starts with gaps and rays stored in permuted order (samples no ray owns keep the
sentinel the output buffers are prefilled with).  Regimes:
  smooth     sum p per ray <= 5: T >= e^-5 = 6.7e-3, no ray terminates at thr <= 1e-3; steps in [1e-3, 0.08];
  walls      smooth with one sample per ray at p in [12, 20]: T falls from >= 6.7e-3 to <= 6.1e-6 in one step, 6.7x above the
             largest threshold and 16x below the smallest non-zero one, where the bound on T is below 1e-3 of T.  The wall stands at
             0, 1, 62, 63, 64, 65, count - 1, 1023 and 1024 where the ray is long enough.  Also sigma == 0 runs (alpha exactly 1), a
             sample with p = 200 (alpha exactly 0 on both sides) and, at thr = 0, T >= 1e-30 everywhere except behind that zero;
  unbounded  smooth's p with steps growing along the ray up to 10 and sigma scaled down to match; the ladder twice, and every
             non-empty ray of the second copy carries a wall (12 of 26 rays; on a listed index that leaves samples behind it, a
             third of the way along the ray otherwise), so at least half the ray lies behind it with suffix sum 0 and the backward there is
             cancellation noise times a large step -- on every chunk-edge length.
Upstream gradients are N(0, 1), rgb uniform in [0, 1), bg None or [1, .5, .25].  The `exact` composite kind: weights k / 256,
colours k / 16, gradients integers in [-3, 3]: no product or sum rounds.  rgb = NaN at every sample with w == 0."""
import functools
import math
import zlib

import numpy as np

U = 2.0 ** -24
EXPF_ULPS = 1
WAVE, MAXC, WAVES_PER_BLOCK = 64, 16, 4
BG = np.array([1.0, 0.5, 0.25], np.float32)
SENTINEL = np.float32(-777.25)
THRESHOLDS = (1e-4, 1e-3, 0.0)
LADDER = (0, 1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2100)
WALL_AT = (0, 1, 62, 63, 64, 65, -1, 1023, 1024)           # -1: count - 1
MSE_SIZES = (1, 3, 255, 256, 257, 768, 131072, 131073)
_BITLEN = np.array([0] + [(l - 1).bit_length() + 1 for l in range(1, WAVE)], np.float64)     # in-chunk part of r_T, by lane


def f64(a):
    return np.asarray(a, np.float64)


def thr32(thr):
    return float(np.float32(thr))


def rays(info):
    for r, (start, count) in enumerate(np.asarray(info)):
        yield r, int(start), int(count)


def owned(info, n):
    m = np.zeros(n, bool)
    for _, a, c in rays(info):
        m[a:a + c] = True
    return m


def alpha(p):
    a = np.exp(-f64(p))
    return np.where(a < 2.0 ** -150, 0.0, a)


def r_T(m):
    m = np.asarray(m, np.int64)
    return 7.0 * (m // WAVE) + _BITLEN[m % WAVE]


def eps(p):
    return (f64(p) + 2.0 * EXPF_ULPS) * U


def nch(count):
    return -(-int(count) // WAVE)


def c_add(count):
    n = nch(count)
    if count <= WAVE * MAXC:
        return 1 + n + 6 + 6 + n + 3          # register path
    return (1 + n) + 6 + 6 + n + 3            # streaming path


# ------------------------------------------------------------------------------------------------ references
def weights(sig, step, info, thr):
    """-> dict: w, T (exclusive, unterminated), a, p, k (index within the ray, -1 where no ray owns the sample), S (sum_{j<k} eps_j),
    first (per ray: the first terminated index, count if none)"""
    sig, step = f64(sig), f64(step)
    thr = thr32(thr)
    n = sig.size
    p = sig * step
    out = dict(w=np.zeros(n), T=np.zeros(n), a=np.zeros(n), p=p, k=np.full(n, -1, np.int64), S=np.zeros(n),
               first=np.zeros(len(info), np.int64))
    for r, s, c in rays(info):
        sl = slice(s, s + c)
        a = alpha(p[sl])
        T = np.concatenate([[1.0], np.cumprod(a)[:-1]]) if c else np.zeros(0)
        dead = ~(T > thr)
        first = int(np.argmax(dead)) if dead.any() else c
        w = T * (1.0 - a)
        w[first:] = 0.0
        e = eps(p[sl])
        out["w"][sl], out["T"][sl], out["a"][sl], out["k"][sl] = w, T, a, np.arange(c)
        out["S"][sl] = np.cumsum(e) - e
        out["first"][r] = first
    return out


def weights_T_bound(ref):
    return ref["T"] * (ref["S"] + r_T(np.maximum(ref["k"], 0)) * U)


def weights_bound(ref):
    k = np.maximum(ref["k"], 0)
    b = ref["T"] * ref["a"] * eps(ref["p"]) + ref["w"] * (ref["S"] + r_T(k) * U + U)
    return np.where(ref["w"] == 0, 0.0, b)              # w is exactly 0 where w_ref is


def danger_rays(ref, info, thr):
    """rays on which some T_ref,k is within the forward bound on T of the threshold (a bound of 0 means T is exact on both sides)"""
    thr = thr32(thr)
    b = weights_T_bound(ref)
    near = (np.abs(ref["T"] - thr) <= b) & (b > 0)
    return [r for r, s, c in rays(info) if near[s:s + c].any()]


def weights_grad(sig, step, info, w, g, gabs=None, r_g=0):
    """-> (gs, bound, A per ray).  gabs: the sum of |terms| behind each g (the fused backward), |g| if None"""
    sig, step, w, g = f64(sig), f64(step), f64(w), f64(g)
    gabs = np.abs(g) if gabs is None else f64(gabs)
    gs, bound, A = np.zeros(sig.size), np.zeros(sig.size), np.zeros(len(info))
    for r, s, c in rays(info):
        if not c:
            continue
        sl = slice(s, s + c)
        p = sig[sl] * step[sl]
        Tn = np.cumprod(alpha(p))
        wg = w[sl] * g[sl]
        suffix = np.concatenate([np.cumsum(wg[::-1])[::-1][1:], [0.0]])
        gs[sl] = step[sl] * (Tn * g[sl] - suffix)
        A[r] = (np.abs(w[sl]) * gabs[sl]).sum()
        k = np.arange(c)
        bound[sl] = np.abs(step[sl]) * U * ((c_add(c) + r_g) * A[r] + (np.cumsum(eps(p)) / U + r_T(k + 1) + 3 + r_g) * Tn * gabs[sl])
    return gs, bound, A


def composite(rgb, w, info, bg):
    """-> (out [R, 3], opacity [R], sum|terms| of out [R, 3], sum|terms| of the opacity [R]); composite_bound turns the sums into bounds"""
    rgb, w = f64(rgb), f64(w)
    R = len(info)
    out, opac, terms, oterms = np.zeros((R, 3)), np.zeros(R), np.zeros((R, 3)), np.zeros(R)
    for r, s, c in rays(info):
        ws = w[s:s + c]
        live = ws != 0
        col = rgb[s:s + c][live] * ws[live, None]
        out[r], opac[r] = col.sum(0), ws.sum()
        terms[r], oterms[r] = np.abs(col).sum(0), np.abs(ws).sum()
        if bg is not None:
            out[r] += f64(bg) * (1.0 - opac[r])
            terms[r] += np.abs(f64(bg)) * (1.0 + oterms[r])
    return out, opac, terms, oterms


def composite_bound(info, terms, oterms, bg):
    """(m + r) u sum|terms|: [R, 3] for the colours, [R] for the opacity"""
    n = np.array([nch(c) for _, _, c in rays(info)], np.float64).reshape(-1)
    mr = n + 6 + 1 if bg is None else n + 7 + 2
    return mr[:, None] * U * terms, (n + 6) * U * oterms


def composite_grad(rgb, w, info, bg, g, extra=None):
    """-> (grad_rgb [n, 3] exact, grad_w [n], G [n] the sum of |terms| of grad_w, r_g the m + r of its bound); unowned samples 0"""
    rgb, w, g = f64(rgb), f64(w), f64(g)
    n = w.size
    grgb, gw, G = np.zeros((n, 3)), np.zeros(n), np.zeros(n)
    for r, s, c in rays(info):
        sl = slice(s, s + c)
        live = w[sl] != 0
        grgb[sl] = w[sl, None] * g[r][None]
        d, dabs = np.zeros(c), np.zeros(c)
        d[live] = (rgb[sl][live] * g[r]).sum(-1)
        dabs[live] = np.abs(rgb[sl][live] * g[r]).sum(-1)
        gbg = 0.0 if bg is None else float((f64(bg) * g[r]).sum())
        gw[sl] = d - gbg
        G[sl] = dabs + (0.0 if bg is None else float(np.abs(f64(bg) * g[r]).sum()))
        if extra is not None:
            gw[sl] += f64(extra)[sl]
            G[sl] += np.abs(f64(extra)[sl])
    return grgb, gw, G, (4 if extra is None else 5)


def mse_blocks(n):
    return min((n + 255) // 256, 512)


def mse(r, t, c, c_dev, gate, start=0.0):
    """-> (grad fp32, sumsq fp64 on top of `start`, its bound).  gate: None (no gate) or its fp32 value"""
    r, t = np.asarray(r, np.float32), np.asarray(t, np.float32)
    cc = np.float32(c) if c_dev is None else np.float32(c) * np.float32(c_dev)
    if gate is not None and not (np.float32(gate) > 0):
        cc = np.float32(0)
    grad = ((r - t) * cc).astype(np.float32)
    d = f64(r) - f64(t)
    s = float((d * d).sum())
    m = -(-r.size // (mse_blocks(r.size) * 256))
    return grad, start + s, (m + 2) * U * s + 2.0 ** -50 * (s + abs(start))


def expf_ulps_single(sig, step, info, w_got):
    """single-sample rays with a >= 1/2 (p <= ln 2): there w = fl(1 - a_gpu), so a_gpu = 1 - w to half an ulp of w.
    -> (lo, hi), the largest over those rays of |(1 - w) - exp(-fl(p))| minus / plus that half ulp, in ulps of a (lo floored at 0):
    max |a_gpu - exp(-fl(p))| lies between them.  None when the fixture holds no such ray."""
    lo = hi = None
    for _, s, c in rays(info):
        if c != 1:
            continue
        p32 = np.float32(sig[s]) * np.float32(step[s])
        a = math.exp(-float(p32))
        if a < 0.5:
            continue
        raw, half = abs((1.0 - float(w_got[s])) - a), 0.5 * float(np.spacing(np.float32(w_got[s])))
        ulp = float(np.spacing(np.float32(a)))
        lo, hi = max(lo or 0.0, max(raw - half, 0.0) / ulp), max(hi or 0.0, (raw + half) / ulp)
    return None if lo is None else (lo, hi)


# ------------------------------------------------------------------------------------------------ comparisons
def worst_ratio(got, ref, bound, what):
    """max |got - ref| / bound; where the bound is 0 the values must be equal.  Raises past 1."""
    got, ref, bound = f64(got), f64(ref), f64(bound)
    assert got.shape == ref.shape == bound.shape, (what, got.shape, ref.shape, bound.shape)
    if got.size == 0:
        return 0.0
    err = np.abs(got - ref)
    assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} non-finite values"
    zero = bound == 0
    assert not (err[zero] != 0).any(), f"{what}: {int((err[zero] != 0).sum())} values differ where the bound is 0"
    ratio = np.where(zero, 0.0, err / np.where(zero, 1.0, bound))
    i = int(np.argmax(ratio))
    assert ratio.flat[i] <= 1.0, f"{what}: |got - ref| = {err.flat[i]:.3e} is {ratio.flat[i]:.2f} x the bound {bound.flat[i]:.3e} at {i} (got {got.flat[i]!r}, ref {ref.flat[i]!r})"
    return float(ratio.flat[i])


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.int32) != want.view(np.int32)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ in their bits, first at {int(np.argmax(bad))}"


def check_weights(got, ref, info, what):
    """the zero set, the sentinel on samples no ray owns, the forward bound -> err / bound"""
    got = np.asarray(got, np.float32)
    own = ref["k"] >= 0
    assert (got[~own] == SENTINEL).all(), f"{what}: a sample no ray owns was written"
    zg, zr = got[own] == 0, ref["w"][own] == 0
    assert np.array_equal(zg, zr), f"{what}: {int((zg != zr).sum())} samples are zero on one side only"
    return worst_ratio(got[own], ref["w"][own], weights_bound(ref)[own], what)


def check_owned(got, ref, bound, info, what):
    """per-sample outputs: the sentinel outside the rays, the bound inside"""
    got = np.asarray(got)
    own = owned(info, got.shape[0])
    assert (got[~own] == SENTINEL).all(), f"{what}: a sample no ray owns was written"
    return worst_ratio(got[own], ref[own], bound[own], what)


# ------------------------------------------------------------------------------------------------ fixtures
def _layout(counts, rng, gaps=False, perm=False):
    counts = np.asarray(counts, np.int64)
    order = rng.permutation(len(counts)) if perm else np.arange(len(counts))
    info = np.zeros((len(counts), 2), np.int32)
    at = 0
    for r in order:
        at += int(rng.integers(1, 4)) if gaps else 0
        info[r] = (at, counts[r])
        at += int(counts[r])
    return info, at + (2 if gaps else 0)


def _smooth_p(c, rng):
    d = rng.uniform(0.2, 1.0, c)
    return rng.uniform(0.5, 4.9) * d / d.sum()


def _build(name, counts, regime, walls=None, gaps=False, perm=False, specials=(), single_p=None):
    """walls: per ray, the wall's index or None.  specials: (ray, kind, index) with kind "zero_run" (sigma = 0 on [index, index + 20)),
    "all_zero" or "p200" (p = 200 at index)."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    info, n = _layout(counts, rng, gaps, perm)
    p = rng.uniform(0.01, 0.2, n)
    step = rng.uniform(1e-3, 0.08, n)
    for r, s, c in rays(info):
        if not c:
            continue
        p[s:s + c] = _smooth_p(c, rng) if single_p is None else rng.uniform(*single_p, c)
        if regime == "unbounded":
            step[s:s + c] = 10.0 ** (-2.0 + 3.0 * np.arange(c) / max(c - 1, 1)) * rng.uniform(0.8, 1.0, c)
        if walls is not None and walls[r] is not None:
            p[s + walls[r]] = rng.uniform(12.05, 19.95)
    for r, kind, i in specials:
        s, c = int(info[r, 0]), int(info[r, 1])
        if kind == "zero_run":
            p[s + i:s + min(i + 20, c)] = 0.0
        elif kind == "all_zero":
            p[s:s + c] = 0.0
        elif kind == "p200":
            p[s + i] = 200.0
    step = step.astype(np.float32)
    sig = (p / step.astype(np.float64)).astype(np.float32)
    R = len(counts)
    fx = dict(name=name, regime=regime, info=info, n=n, R=R, sig=sig, step=step,
              g=rng.standard_normal(n).astype(np.float32), rgb=rng.random((n, 3)).astype(np.float32),
              go=rng.standard_normal((R, 3)).astype(np.float32), extra=(0.3 * rng.standard_normal(n)).astype(np.float32))
    # the exact composite kind on the same layout
    wk = rng.integers(0, 9, n) * (rng.random(n) > 0.3)
    fx["exact_w"] = (wk / 256.0).astype(np.float32)
    fx["exact_rgb"] = (rng.integers(0, 16, (n, 3)) / 16.0).astype(np.float32)
    fx["exact_go"] = rng.integers(-3, 4, (R, 3)).astype(np.float32)
    for v in fx.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return fx


def _wall_index(c, at):
    i = c - 1 if at < 0 else at
    return i if 0 <= i < c else None


def _walls_case(lengths):
    counts, walls = [], []
    for c in lengths:
        for i in sorted({_wall_index(c, at) for at in WALL_AT} - {None}):
            counts.append(c)
            walls.append(i)
    return counts, walls


_SHORT = (65, 1, 64, 130, 2, 63, 0, 129, 7)


def _specs():
    s = {}
    s["smooth_ladder"] = dict(counts=LADDER, regime="smooth")
    for R in (1, 3, 4, 5, 9):
        s[f"smooth_rays{R}"] = dict(counts=_SHORT[:R], regime="smooth")
    s["singles"] = dict(counts=(1,) * 67, regime="smooth", single_p=(0.01, 0.69))        # alpha >= 1/2: the expf measurement
    s["smooth_empties"] = dict(counts=(0, 0, 5, 64, 0, 0, 70, 1, 0, 0), regime="smooth")
    s["all_empty"] = dict(counts=(0,) * 5, regime="smooth")
    s["all_empty_gaps"] = dict(counts=(0,) * 6, regime="smooth", gaps=True)
    s["smooth_gaps_permuted"] = dict(counts=(64, 0, 1, 129, 65, 1025, 3, 63, 0, 128, 200), regime="smooth", gaps=True, perm=True)
    counts, walls = _walls_case((1, 2, 63, 64, 65, 127, 128, 129))
    k = len(counts)
    counts += [100, 129, 40, 70, 130, 0]
    walls += [None, 64, None, None, None, None]
    s["walls_short"] = dict(counts=counts, regime="walls", walls=walls,
                            specials=((k, "zero_run", 10), (k + 1, "zero_run", 60), (k + 2, "all_zero", 0), (k + 3, "p200", 5),
                                      (k + 4, "p200", 63)))
    counts, walls = _walls_case((1023, 1024, 1025))
    s["walls_long"] = dict(counts=counts + [2100] * 4, regime="walls", walls=walls + [0, 1023, 1024, 2099])
    s["walls_gaps_permuted"] = dict(counts=(64, 0, 65, 129, 1025, 5, 63, 0, 1), regime="walls", walls=(63, None, 64, 1, 1024, 0, 62, None, 0),
                                    gaps=True, perm=True)
    counts = list(LADDER) + list(LADDER)
    def tail_wall(c, at):          # the listed index where samples are left behind it, a third of the way along the ray otherwise
        i = _wall_index(c, at)
        return i if i is not None and i < c - 1 else c // 3
    walls = [None] * len(LADDER) + [tail_wall(c, WALL_AT[i % len(WALL_AT)]) if c else None for i, c in enumerate(LADDER)]
    walls[-1], walls[-2], walls[-3] = 1024, 512, 63            # 2100, 1025, 1024: a long noise tail behind
    s["unbounded"] = dict(counts=counts, regime="unbounded", walls=walls)
    return s


_SPECS = _specs()
FIXTURES = tuple(_SPECS)


@functools.lru_cache(maxsize=None)
def fixture(name):
    return _build(name, **_SPECS[name])


@functools.lru_cache(maxsize=None)
def forward_ref(name, thr):
    """the reference forward of a fixture: computed once, shared, read-only"""
    fx = fixture(name)
    ref = weights(fx["sig"], fx["step"], fx["info"], thr)
    for v in ref.values():
        v.setflags(write=False)
    return ref


def masked_rgb(rgb, w):
    """rgb with NaN at every sample whose weight is 0"""
    out = np.array(rgb, np.float32)
    out[np.asarray(w) == 0] = np.nan
    return out


def mse_inputs(n):
    rng = np.random.default_rng(n)
    return rng.random(n).astype(np.float32), rng.random(n).astype(np.float32)
