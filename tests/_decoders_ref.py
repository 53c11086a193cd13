"""fp64 definition of the explicit K-Planes decoders' product stage (tn_basis_dot_fwd / _bwd, csrc/kplanes.hip), of the stand-alone
encoders (tn_posenc_fwd, tn_dir_encode, csrc/mlp.hip) and of the ray tables (tn_ray_aux, csrc/weights.hip), with an absolute bound
``E_*`` next to every floating-point output.  numpy only, CPU only.  Conventions and constants are tests/_mlp_ref.py's (u = 2^-24;
E_SINCOS and R_EXP are its 2-ulp ASSUMPTION for the device library's sinf / cosf / expf -- not a measurement).

basis_dot, on the fp32 inputs exactly as the kernels receive them (f [n, C], basis [n, K, C], grad_out [n, K]):

  pre-activation  v = sum_c f b,  A = sum_c |f b|,  E_v = (C + 2) u A: C products and C additions in ANY order (the lane-strided partial
                  sums, the wave tree, fused or unfused multiply-adds).
  none            the value and its bound pass through; backward factor 1, exact.
  exp_m1          y = exp(t), t = v - 1:  E_y = y expm1(E_v + u |t|) + 5 u y  (fl(v - 1), expf's 2 ulp = 4 u, the result's rounding).
  exp             the same with t = v.
  sigmoid         s = 1 / (1 + exp(-v)):  E_y = (s (1 - s) + 0.1 E_v) E_v + s r,  r = 4 u (1 - s) + 3 u;
                  backward factor s (1 - s) from the same s: E = 0.1 E_v + s (1 - s) (r + 2 u) + s^2 r.
  exp*, backward  factor exp(clamp(t, -15, 15)), bound as for y with the clamped value: the clamp is 1-Lipschitz and continuous, so the
                  bound holds on both sides of +-15 and no sample needs rejecting there.
  gv = g fac      E_gv = |g| E_fac + u |g fac|
  grad_basis      gv f:            E = |f| E_gv + u |gv f|
  grad_f          sum_k gv_k b_k:  E = sum_k |b_k| E_gv_k + (K + 2) u sum_k |gv_k b_k|
  accumulate_f    pre-fill + grad_f, one more u |result| (the one addition of the finished sum to what was there).

Encoders: the angle is ONE fp32 product x_c * freq_f (posenc_kernel, mlp_device.h posenc_value), sin / cos of that fp32 number are taken
in fp64 and carry E_SINCOS; freqs = NULL means ldexp(float32(pi), f) (exact: a power of two times an fp32 number).  The raw direction
columns and the zero pad of tn_dir_encode are exact.  ray_aux is integers and copies: equality.

Exact fixtures (``exact_fixture``), in the manner of tests/_scatter_orders.py: f, basis in {-1, 0, 1}, integer grad_out (and pre-fill) of
small magnitude, TN_ACT_NONE.  Every term and every partial sum of out, grad_basis and grad_f is then an integer far below 2^24 in any
order, so a correct kernel returns the fp64 values bit for bit; ``assert_exact`` proves that from the sums of |terms| instead of
assuming it.
"""
from typing import Dict, NamedTuple, Optional

import numpy as np

from _mlp_ref import E_SINCOS, R_EXP, U, default_freqs      # noqa: F401  (re-exported: the tests take them from here)

ACTS = {"none": 0, "exp_m1": 1, "sigmoid": 2, "exp": 3}      # TN_ACT_* of include/tinynerf_hip.h
CLAMP = 15.0
GRID_BLOCKS, WAVES_PER_BLOCK = 2048, 4                        # tn_basis_dot_*: min(ceil(n / 4), 2048) blocks of 4 waves, persistent


def n_waves(n: int) -> int:
    """waves of the tn_basis_dot_* grid: sample i is served by wave i mod n_waves(n)"""
    return WAVES_PER_BLOCK * min((n + WAVES_PER_BLOCK - 1) // WAVES_PER_BLOCK, GRID_BLOCKS)


# ------------------------------------------------------------------------------------------------ basis_dot: fp64 + bounds
def preact(f: np.ndarray, basis: np.ndarray):
    """-> v [n, K], A = sum_c |f b|, E_v = (C + 2) u A"""
    assert f.dtype == np.float32 and basis.dtype == np.float32 and basis.ndim == 3 and basis.shape[::2] == f.shape
    f64, b64 = f.astype(np.float64), basis.astype(np.float64)
    v = np.einsum("nc,nkc->nk", f64, b64)
    A = np.einsum("nc,nkc->nk", np.abs(f64), np.abs(b64))
    return v, A, (f.shape[1] + 2) * U * A


def _exp_bound(y, Ev, t):
    return y * np.expm1(Ev + U * np.abs(t)) + R_EXP * y + U * y


def activation(act: str, v: np.ndarray, Ev: np.ndarray):
    """-> y, E_y"""
    if act == "none":
        return v, Ev
    if act == "sigmoid":
        s = 1.0 / (1.0 + np.exp(-v))
        return s, (s * (1 - s) + 0.1 * Ev) * Ev + s * (R_EXP * (1 - s) + 3 * U)
    t = v - 1.0 if act == "exp_m1" else v
    assert act in ("exp_m1", "exp"), act
    y = np.exp(t)
    return y, _exp_bound(y, Ev, t)


def act_grad(act: str, v: np.ndarray, Ev: np.ndarray):
    """d act / d v as the backward takes it -> fac, E_fac"""
    if act == "none":
        return np.ones_like(v), np.zeros_like(v)
    if act == "sigmoid":
        s = 1.0 / (1.0 + np.exp(-v))
        r = R_EXP * (1 - s) + 3 * U
        return s * (1 - s), 0.1 * Ev + s * (1 - s) * (r + 2 * U) + s * s * r
    t = v - 1.0 if act == "exp_m1" else v
    assert act in ("exp_m1", "exp"), act
    fac = np.exp(np.clip(t, -CLAMP, CLAMP))
    return fac, _exp_bound(fac, Ev, t)


def reference(f: np.ndarray, basis: np.ndarray, act: str, grad_out: Optional[np.ndarray] = None,
              prefill: Optional[np.ndarray] = None) -> Dict[str, np.ndarray]:
    """out / E_out [n, K]; with grad_out [n, K]: grad_basis / E_grad_basis [n, K, C], grad_f / E_grad_f [n, C]; with ``prefill`` [n, C]
    (what grad_f held before an accumulate_f = 1 call) also grad_f_acc / E_grad_f_acc; and the sums of |terms| A_out, A_grad_f,
    A_grad_f_acc that ``assert_exact`` takes."""
    v, A, Ev = preact(f, basis)
    y, Ey = activation(act, v, Ev)
    res = dict(v=v, E_v=Ev, out=y, E_out=Ey, A_out=A)
    if grad_out is None:
        return res
    assert grad_out.dtype == np.float32 and grad_out.shape == v.shape
    f64, b64, g = f.astype(np.float64), basis.astype(np.float64), grad_out.astype(np.float64)
    fac, Efac = act_grad(act, v, Ev)
    gv = g * fac
    Egv = np.abs(g) * Efac + (0.0 if act == "none" else U) * np.abs(gv)          # none: gv IS g, no product
    gb = gv[:, :, None] * f64[:, None, :]
    Egb = np.abs(f64)[:, None, :] * Egv[:, :, None] + U * np.abs(gb)
    terms = gv[:, :, None] * b64
    K = basis.shape[1]
    S = np.abs(terms).sum(1)
    gf = terms.sum(1)
    Egf = (np.abs(b64) * Egv[:, :, None]).sum(1) + (K + 2) * U * S
    res.update(gv=gv, E_gv=Egv, grad_basis=gb, E_grad_basis=Egb, grad_f=gf, E_grad_f=Egf, A_grad_f=S)
    if prefill is not None:
        assert prefill.dtype == np.float32 and prefill.shape == f.shape
        p64 = prefill.astype(np.float64)
        res.update(grad_f_acc=p64 + gf, E_grad_f_acc=Egf + U * np.abs(p64 + gf), A_grad_f_acc=S + np.abs(p64))
    return res


def ratios(got: Dict[str, np.ndarray], ref: Dict[str, np.ndarray], keys=("out", "grad_basis", "grad_f", "grad_f_acc")) -> Dict[str, float]:
    """{name: largest |got - ref| / bound over the elements}; <= 1 is inside.  Per element; a non-finite `got` is infinitely far."""
    out = {}
    for k in keys:
        if got.get(k) is None:
            continue
        g = np.asarray(got[k], np.float64)
        assert g.shape == ref[k].shape, (k, g.shape, ref[k].shape)
        r = np.abs(g - ref[k]) / np.maximum(ref["E_" + k], 1e-300)
        r = np.where(np.isfinite(g), r, np.inf)
        r = np.where((ref["E_" + k] == 0) & (g == ref[k]), 0.0, r)
        out[k] = float(r.max(initial=0.0))
    return out


def assert_exact(ref: np.ndarray, abs_ref: np.ndarray, name: str = "") -> None:
    """every term and every partial sum, in any order, is an integer bounded by sum |terms|: exact in fp32 when that sum stays below
    2^24; the fp64 reference must then be an integer and its own fp32 rounding (tests/_scatter_orders.assert_exact with bits = 0)"""
    ref, abs_ref = np.asarray(ref, np.float64), np.asarray(abs_ref, np.float64)
    assert float(abs_ref.max(initial=0.0)) < 2.0 ** 24, (name, float(abs_ref.max(initial=0.0)))
    assert np.array_equal(ref, np.round(ref)), name
    assert np.array_equal(ref, ref.astype(np.float32).astype(np.float64)), name


# ------------------------------------------------------------------------------------------------ basis_dot: fixtures
class Fixture(NamedTuple):
    f: np.ndarray               # [n, C]
    basis: np.ndarray           # [n, K, C]
    grad_out: np.ndarray        # [n, K]
    prefill: np.ndarray         # [n, C]: grad_f before an accumulate_f = 1 call
    act: str


def general_fixture(n: int, C: int, K: int, act: str, seed: int) -> Fixture:
    """f, basis ~ N(0, s^2) with s^2 sqrt(C) = 8 / 3, i.e. pre-activations of standard deviation 8 / 3: they span about [-8, 8].  C = 1 has
    the heavy tails of a product of two normals, so there the product is drawn uniform in [-8, 8] and split into its two factors."""
    rng = np.random.default_rng(seed)
    if C == 1:
        v = rng.uniform(-8.0, 8.0, (n, K))
        f = (rng.uniform(0.5, 2.0, (n, 1)) * rng.choice([-1.0, 1.0], (n, 1))).astype(np.float32)
        basis = (v / f.astype(np.float64))[:, :, None].astype(np.float32)
    else:
        s = (8.0 / 3.0 / np.sqrt(C)) ** 0.5
        f = (s * rng.standard_normal((n, C))).astype(np.float32)
        basis = (s * rng.standard_normal((n, K, C))).astype(np.float32)
    g = rng.standard_normal((n, K)).astype(np.float32)
    pre = rng.uniform(-2.0, 2.0, (n, C)).astype(np.float32)
    return Fixture(f, basis, g, pre, act)


def exact_fixture(n: int, C: int, K: int, seed: int) -> Fixture:
    """f, basis in {-1, 0, 1}, grad_out and the pre-fill integers in [-7, 7], TN_ACT_NONE: |out| <= C, |grad_basis| <= 7,
    |grad_f| <= 7 K (+ 7 with the pre-fill) -- integers below 2^24 whatever the order"""
    rng = np.random.default_rng(seed)
    f = rng.integers(-1, 2, (n, C)).astype(np.float32)
    basis = rng.integers(-1, 2, (n, K, C)).astype(np.float32)
    g = rng.integers(-7, 8, (n, K)).astype(np.float32)
    pre = rng.integers(-7, 8, (n, C)).astype(np.float32)
    return Fixture(f, basis, g, pre, "none")


C_VALUES = (1, 8, 24, 63, 64, 65, 96, 128, 129, 200)         # idle lanes; a full wave; ragged last trips of the lane stride at 65, 129, 200
K_VALUES = (1, 2, 3, 4)
N_VALUES = (1, 3, 4, 5, 8191, 8192, 8193, 20001)              # the persistent loop's second trip starts at 8193; 20001: waves of 2 and 3 trips
SECOND_TRIP = (8193, 20001)
REAL = ((96, 1, "exp_m1"), (96, 3, "sigmoid"))                # KPlanesExplicitOpacityDecoder(96), KPlanesExplicitColorDecoder(96, ..)


def cases():
    """(n, C, K, act) of tests/test_hip_decoders.py part A: the two real configurations at every n; every C with K = 4 at both second-trip
    sizes, the activations in turn; K = 1, 2, 3 at both second-trip sizes; K = 4 at every other n."""
    acts = ("none", "exp_m1", "sigmoid", "exp")
    out = [(n, C, K, act) for (C, K, act) in REAL for n in N_VALUES]
    for j, n in enumerate(SECOND_TRIP):
        out += [(n, C, 4, acts[(i + j) % 4]) for i, C in enumerate(C_VALUES)]
    out += [(8193, 65, 1, "none"), (8193, 129, 2, "exp"), (8193, 24, 3, "exp_m1"),
            (20001, 200, 1, "sigmoid"), (20001, 63, 2, "none"), (20001, 8, 3, "exp")]
    out += [(1, 65, 4, "exp"), (3, 200, 4, "sigmoid"), (4, 24, 4, "none"), (5, 129, 4, "exp_m1"), (8191, 1, 4, "exp"), (8192, 64, 4, "none")]
    assert len(set(out)) == len(out)
    return out


def case_seed(n: int, C: int, K: int) -> int:
    return 1000003 * n + 1009 * C + K


CLAMP_TARGETS = (-40.0, -15.5, -15.0, 15.0, 15.5, 20.0)


def clamp_fixture(act: str, at: str, C: int = 96, reps: int = 4, seed: int = 0) -> Fixture:
    """K = 1 rows of C channels whose clamped quantity sits EXACTLY at CLAMP_TARGETS (each `reps` times, different channels every row).
    ``at`` = "acc-1": sum_c f b = target + 1 (what TN_ACT_EXP_M1 clamps is the target; TN_ACT_EXP sees target + 1: "the same rows");
    "acc": sum_c f b = target (TN_ACT_EXP's own clamp edges).  f in {+-1/2, +-1, +-2}, basis multiples of 2^-6 in [-1, 1]: every product
    and partial sum is a multiple of 2^-7 below 2^9, exact in fp32 in any order; the last channel (f = 1) carries the remainder, itself
    such a multiple.  So the pre-activation is the same number in the kernel and in fp64, on either side of and AT +-15."""
    rng = np.random.default_rng(seed)
    tg = np.repeat(np.asarray(CLAMP_TARGETS), reps) + (1.0 if at == "acc-1" else 0.0)
    n = tg.size
    f = (rng.choice([0.5, 1.0, 2.0], (n, C)) * rng.choice([-1.0, 1.0], (n, C)))
    b = rng.integers(-64, 65, (n, C)) / 64.0
    f[:, -1] = 1.0
    b[:, -1] = tg - (f[:, :-1] * b[:, :-1]).sum(1)
    f32, b32 = f.astype(np.float32), b.astype(np.float32)
    assert np.array_equal(f32, f) and np.array_equal(b32, b)
    assert np.array_equal(np.einsum("nc,nc->n", f, b), tg) and float(np.abs(f * b).sum(1).max()) * 2.0 ** 7 < 2.0 ** 24
    g = rng.uniform(0.5, 2.0, (n, 1)).astype(np.float32) * rng.choice([-1.0, 1.0], (n, 1)).astype(np.float32)
    pre = rng.uniform(-2.0, 2.0, (n, C)).astype(np.float32)
    return Fixture(f32, b32[:, None, :], g, pre, act)


# ------------------------------------------------------------------------------------------------ basis_dot: fp32 evaluations (CPU)
def eval32(fx: Fixture, accumulate: bool = False, want_basis: bool = True, fault: Optional[str] = None) -> Dict[str, np.ndarray]:
    """numpy float32 evaluation in the kernel's own order: lane l sums its channels c = l, l + 64, ..., the 64 partial sums go through a
    butterfly tree, every intermediate rounded to fp32 (products and additions separately: one of the orders the bound covers).
    ``fault`` plants one error (tests/test_decoders_ref.py):
      "drop_ge64"   channels >= 64 are left out of the dot product and get no grad_f;
      "drop_tail"   the last trip of the lane stride (c >= 64 * floor((C - 1) / 64)) is left out the same way;
      "stride_c1"   basis row k is read at k * (C - 1) instead of k * C;
      "no_clamp"    the backward factor of exp / exp_m1 is exp(t) unclamped;
      "no_accum"    accumulate_f is ignored;
      "wrap_8192"   sample i >= 8192 reads and writes sample i - 8192 (rows >= 8192 keep what the buffers held: zeros here)."""
    f32 = np.float32
    f, basis, g = fx.f, fx.basis, fx.grad_out
    n, K, C = basis.shape
    act = fx.act
    if fault == "wrap_8192" and n > 8192:
        fresh = eval32(fx, False, want_basis)
        idx = np.arange(n)
        served = (idx < 8192).astype(int) + (idx + 8192 < n)        # how often row j is computed: as itself and as the image of j + 8192
        out = {k_: a * (served > 0).reshape((n,) + (1,) * (a.ndim - 1)).astype(f32) for k_, a in fresh.items()}
        if accumulate:                      # recomputing a row gives the same values -- but an accumulating backward adds them again
            a = fx.prefill
            for trip in range(2):
                a = np.where((served > trip)[:, None], (a + fresh["grad_f"]).astype(f32), a)
            out["grad_f"] = a
        return out
    if fault == "stride_c1":
        flat = basis.reshape(n, K * C)
        basis = np.stack([flat[:, k * (C - 1):k * (C - 1) + C] for k in range(K)], 1)
    live = np.ones(C, bool)
    if fault == "drop_ge64":
        live[64:] = False
    if fault == "drop_tail":
        live[64 * ((C - 1) // 64):] = False
    lanes = np.zeros((n, K, 64), f32)
    for c0 in range(0, C, 64):
        w = min(64, C - c0)
        prod = (f[:, None, c0:c0 + w] * basis[:, :, c0:c0 + w]).astype(f32) * live[c0:c0 + w].astype(f32)
        lanes[:, :, :w] = (lanes[:, :, :w] + prod).astype(f32)
    o = 32
    while o:
        lanes = (lanes[:, :, :o] + lanes[:, :, o:2 * o]).astype(f32)
        o >>= 1
    acc = lanes[:, :, 0]
    one, lim = f32(1), f32(CLAMP)
    def exp32(a):                            # a correctly rounded expf (numpy's own float32 exp promises no 2 ulp)
        assert a.dtype == f32
        with np.errstate(over="ignore"):
            return np.exp(a.astype(np.float64)).astype(f32)
    if act == "none":
        y, fac = acc, np.ones_like(acc)
    elif act == "sigmoid":
        y = (one / (one + exp32(-acc))).astype(f32)
        fac = None
    else:
        t = (acc - one).astype(f32) if act == "exp_m1" else acc
        y = exp32(t)
        fac = exp32(t if fault == "no_clamp" else np.clip(t, -lim, lim))
    if act == "sigmoid":
        gv = ((g * y).astype(f32) * (one - y).astype(f32)).astype(f32)
    elif act == "none":
        gv = g
    else:
        gv = (g * fac).astype(f32)
    gf = np.zeros((n, C), f32)
    for k in range(K):
        gf = (gf + (gv[:, k:k + 1] * basis[:, k, :]).astype(f32)).astype(f32)
    gf = gf * live.astype(f32)
    if accumulate and fault != "no_accum":
        gf = (fx.prefill + gf).astype(f32)
    res = dict(out=y.astype(f32), grad_f=gf)
    if want_basis:
        res["grad_basis"] = (gv[:, :, None] * f[:, None, :]).astype(f32)
    return res


# ------------------------------------------------------------------------------------------------ encoders
def freqs_or_default(freqs: Optional[np.ndarray], F: int) -> np.ndarray:
    """freqs = NULL: ldexp(float32(pi), f) -- exact in fp32"""
    if freqs is not None:
        assert freqs.dtype == np.float32 and freqs.shape == (F,)
        return freqs
    fr = np.ldexp(np.float32(np.pi), np.arange(F)).astype(np.float32)
    assert np.array_equal(fr.astype(np.float64), np.float64(np.float32(np.pi)) * 2.0 ** np.arange(F))
    return fr


def posenc(x: np.ndarray, freqs: Optional[np.ndarray], F: int):
    """tn_posenc_fwd: x [n, C] fp32 -> out [n, 2 F C] fp64 with out[n, c 2F + f] = sin, out[n, c 2F + F + f] = cos of the fp32 product
    x[n, c] * freqs[f]; -> (out, E) with E = E_SINCOS everywhere"""
    assert x.dtype == np.float32 and x.ndim == 2
    ang = x[:, :, None] * freqs_or_default(freqs, F)[None, None, :]
    assert ang.dtype == np.float32
    a = ang.astype(np.float64)
    out = np.concatenate([np.sin(a), np.cos(a)], -1).reshape(x.shape[0], -1)
    return out, np.full(out.shape, E_SINCOS)


def dir_encode(dirs: np.ndarray, freqs: Optional[np.ndarray], F: int, stride: int):
    """tn_dir_encode: [PE_F(d) (6F), d (3), 0 ...] per row of `stride` columns -> (table fp64, E): E_SINCOS on the PE columns, 0 on the
    direction and pad columns (compared for equality)"""
    assert dirs.dtype == np.float32 and dirs.shape[1] == 3 and stride >= 6 * F + 3
    pe, Epe = posenc(dirs, freqs, F)
    n = dirs.shape[0]
    out, E = np.zeros((n, stride)), np.zeros((n, stride))
    out[:, :6 * F], E[:, :6 * F] = pe, Epe
    out[:, 6 * F:6 * F + 3] = dirs.astype(np.float64)
    return out, E


def posenc_x(n: int, C: int, seed: int):
    """x [n, C] uniform in [-1, 1) whose last min(5, n - 1) rows hold exactly 0, +1, -1, +0.5, -0.5 in every channel (angles at
    multiples of pi / 2, where a wrong sin / cos column order or frequency index shows as a sign) -> (x, the number of such rows)"""
    x = (np.random.default_rng(seed).random((n, C)) * 2 - 1).astype(np.float32)
    special = np.array([0.0, 1.0, -1.0, 0.5, -0.5], np.float32)[:max(min(5, n - 1), 0)]
    if special.size:
        x[n - special.size:] = special[:, None]
    return x, int(special.size)


def posenc32(x: np.ndarray, freqs: Optional[np.ndarray], F: int, fault: Optional[str] = None) -> np.ndarray:
    """fp32 numpy evaluation of posenc; ``fault``: "swap" = sin / cos halves exchanged, "freq_index" = frequency F - 1 - f"""
    fr = freqs_or_default(freqs, F)
    if fault == "freq_index":
        fr = fr[::-1]
    ang = x[:, :, None] * fr[None, None, :]
    assert ang.dtype == np.float32
    parts = [np.sin(ang.astype(np.float64)), np.cos(ang.astype(np.float64))]      # correctly rounded sinf / cosf of the fp32 angle
    if fault == "swap":
        parts.reverse()
    return np.concatenate(parts, -1).reshape(x.shape[0], -1).astype(np.float32)


# ------------------------------------------------------------------------------------------------ ray_aux
def ray_aux(packed: np.ndarray, info: np.ndarray):
    """tn_ray_aux: ray_ids[i] = the ray of sample i, steps[i] = packed[i, 6], dirs[r] = packed[start_r, 3:6] (0 for an empty ray)"""
    assert packed.dtype == np.float32 and packed.shape[1] == 7 and info.dtype == np.int32 and info.shape[1] == 2
    N, R = packed.shape[0], info.shape[0]
    ray_ids = np.full(N, -1, np.int32)
    dirs = np.zeros((R, 3), np.float32)
    for r, (a, c) in enumerate(info.tolist()):
        ray_ids[a:a + c] = r
        if c > 0:
            dirs[r] = packed[a, 3:6]
    return ray_ids, packed[:, 6].copy(), dirs
