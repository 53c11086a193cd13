"""fp64 reference of the fused MLP launches (tinynerf_amd.models._FusedMLP -> csrc/mlp*.hip, heads_dx.hip) with a running worst-case
error bound per element.  numpy only, CPU only.

Given the fp32 parameters and inputs exactly as the kernels receive them, ``reference`` evaluates in fp64

* the input encoding of the descriptor (``Spec.enc``): "none"; "posenc" = PE_F(x[:, :3]) (TN_ENC_POSENC); "dircat" = cat[PE_F(d), d, x]
  (TN_ENC_DIR_CAT, and TN_ENC_AUX_CAT through the per-ray table).  The sin / cos ARGUMENT is formed as the kernel forms it
  (csrc/mlp_device.h posenc_value: ``ang = x_c * freq_f`` as one fp32 product), then sin / cos of that fp32 number are taken in fp64;
* the Linear / ReLU stack;
* the output activation ("none", "sigmoid", "exp_m1" = exp(v - 1) with the truncated exponential's clamped backward);
* the backward for a given grad_y: grad_x, every dW, every db,

and next to every quantity an absolute bound ``E_*`` on |any correct fp32 evaluation - the fp64 value|, u = 2^-24:

  forward   E_out = |W| E_in + ((K + 2) u + c_mode) A,   A = |W| |h| + |b|   (the layer on absolute values), K = the layer's fan-in.
            (K + 2) u covers K products, K additions in ANY order (gamma_K of a dot product, whatever the tree: MFMA K-order, split
            accumulators, atomics) and the bias addition.  ReLU passes E on unchanged (1-Lipschitz), so the forward bound holds whatever
            side of zero a unit lands on.
  backward  the same recurrence through W^T and the ReLU masks: E_g = |W^T| E_delta + ((K + 2) u + c_mode) |W^T| |delta|, K = the layer's
            fan-out; delta_l = g_l * mask_l, E_delta_l = E_g * mask_l (the masks are exact on tie-free samples, below).
  dW, db    product rule |delta| E_h + E_delta |h| + E_delta E_h summed over the samples, plus ((n + 2) u + c_mode) sum |delta| |h| for the
            n-term sum (db: (n + 2) u sum |delta|; it has no products).  c_mode enters dW because the header's promise is per PRODUCT and
            the weight-gradient launches of the wide stacks run on the same matrix cores as the forward.
  c_mode    what include/tinynerf_hip.h promises for the arithmetic, not a measurement: 0 for the fp32 MFMA; 2^-23 for TN_MLP_BF16X3
            ("every product good to 2^-23, the error of an fp32 product's own rounding"); 2^-21 for TN_MLP_F16X2 ("x s = hi + lo in
            fp16: 22 of fp32's 24 significand bits": each operand is good to 2^-22, a product to 2 * 2^-22).
  sinf / cosf / expf  the kernels call the device library's sinf, cosf and expf (no fast-math flag, tinynerf_amd/build.py).  Their
            accuracy is not stated anywhere in this repository, so 2 ulp is assumed: sin / cos columns carry E = 2 * 2^-24 = 2^-23 (2 ulp
            of a value in [1/2, 1); absolute, so it is generous for smaller values), expf a relative 2 * 2^-23.  Raw input columns are exact.
  sigmoid   s = 1 / (1 + expf(-v)): |s'| <= s (1 - s) + 0.1 E_v on [v - E_v, v + E_v] (|s''| < 0.1), relative rounding r = 4 u (1 - s) + 3 u
            (expf, the addition, the correctly rounded division).  Backward factor s (1 - s) evaluated from the same s:
            error <= 0.1 E_v + s (1 - s) (r + 2 u) + s^2 r.
  exp_m1    y = expf(t), t = fl(v - 1): E_y = y expm1(E_v + u |t|) + 5 u y (expf's 2 ulp = 4 u, one u of slack for the result's own rounding); the backward factor expf(clamp(t, -15, 15)) likewise (the clamp
            is 1-Lipschitz).

Ties.  A backward comparison is only meaningful for a sample in which no hidden unit has |pre| <= 2 E_pre: then every evaluation within
the bound takes the same ReLU state as the fp64 one.  ``fixture`` draws samples one at a time and rejects a draw that holds such a
unit, until it has n samples -- n and every sample's position stay exact -- and returns the rejection share.  It always uses the largest
c_mode (2^-21), so that all arithmetic modes are tested on the same samples.
"""
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

U = 2.0 ** -24
C_MODE = {"fp32": 0.0, "bf16x3": 2.0 ** -23, "f16x2": 2.0 ** -21}
C_MODE_MAX = max(C_MODE.values())
E_SINCOS = 2.0 * 2.0 ** -24          # 2 ulp of a value in [1/2, 1)
R_EXP = 2.0 * 2.0 ** -23             # 2 ulp, relative
REJECTION_CAP = 0.5


class Spec(NamedTuple):
    """enc: "none" | "posenc" | "dircat"; in_dim: width of x (posenc: 3); F: n_freqs; n_hidden: hidden -> hidden layers (models.MLP's
    hidden_layers: the stack has n_hidden + 1 ReLU layers); act: "none" | "sigmoid" | "exp_m1"."""
    enc: str
    in_dim: int
    F: int
    hidden: int
    n_hidden: int
    out: int
    act: str

    @property
    def enc_dim(self) -> int:
        return {"none": self.in_dim, "posenc": 6 * self.F, "dircat": 6 * self.F + 3 + self.in_dim}[self.enc]

    @property
    def x_cols(self) -> slice:          # where x sits in the encoded input (grad_x = those columns of the first layer's data gradient)
        return slice(6 * self.F + 3, self.enc_dim) if self.enc == "dircat" else slice(0, self.enc_dim)

    def __str__(self):
        return f"{self.enc}{self.F or ''}:{self.enc_dim}->{self.hidden}x{self.n_hidden + 1}->{self.out}:{self.act}"


def make_layers(spec: Spec, seed: int) -> List[Tuple[np.ndarray, np.ndarray]]:
    """torch's default Linear init in the order models.MLP constructs its layers: torch.manual_seed(seed); models.MLP(...) holds the same
    parameters."""
    import torch
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        dims = [spec.enc_dim] + [spec.hidden] * (spec.n_hidden + 1) + [spec.out]
        lins = [torch.nn.Linear(i, o) for i, o in zip(dims[:-1], dims[1:])]
    return [(l.weight.detach().numpy().copy(), l.bias.detach().numpy().copy()) for l in lins]


def default_freqs(F: int) -> np.ndarray:
    """models.PositionalEncoding.freqs: 2^j pi in fp32"""
    return (2.0 ** np.arange(F) * np.pi).astype(np.float32)


def _encode(spec: Spec, x: np.ndarray, aux: Optional[np.ndarray], freqs: Optional[np.ndarray], dtype):
    """-> (encoded input in `dtype`, its error bound; fp32 evaluation: no bound needed)"""
    x = np.asarray(x, np.float32)
    if spec.enc == "none":
        return x.astype(dtype), np.zeros(x.shape)
    src = x[:, :3] if spec.enc == "posenc" else np.asarray(aux, np.float32)
    ang = src[:, :, None] * np.asarray(freqs, np.float32)[None, None, :]          # one fp32 product, as posenc_value forms it
    assert ang.dtype == np.float32
    a = ang.astype(dtype)
    pe = np.concatenate([np.sin(a), np.cos(a)], -1).reshape(x.shape[0], -1)       # [c * 2F + (f | F + f)]: models.py:36-39
    if spec.enc == "posenc":
        return pe.astype(dtype), np.full(pe.shape, E_SINCOS)
    h = np.concatenate([pe.astype(dtype), src.astype(dtype), x.astype(dtype)], -1)
    return h, np.concatenate([np.full(pe.shape, E_SINCOS), np.zeros((x.shape[0], 3 + x.shape[1]))], -1)


def forward(spec: Spec, layers, x, aux=None, freqs=None, c_mode: float = 0.0) -> Dict:
    """fp64 forward with bounds: hs / E_hs (inputs of every layer), pres / E_pres, y / E_y, and ``margin`` [n] = min over the hidden units
    of |pre| - 2 E_pre (a sample is tie-free iff margin > 0)."""
    h, E = _encode(spec, x, aux, freqs, np.float64)
    hs, Ehs, pres, Epres = [], [], [], []
    margin = np.full(h.shape[0], np.inf)
    for li, (W, b) in enumerate(layers):
        W, b = np.asarray(W, np.float64), np.asarray(b, np.float64)
        K = W.shape[1]
        hs.append(h); Ehs.append(E)
        pre = h @ W.T + b
        A = np.abs(h) @ np.abs(W).T + np.abs(b)
        Epre = E @ np.abs(W).T + ((K + 2) * U + c_mode) * A
        pres.append(pre); Epres.append(Epre)
        if li + 1 < len(layers):
            margin = np.minimum(margin, (np.abs(pre) - 2.0 * Epre).min(axis=1))
            h, E = np.maximum(pre, 0.0), Epre
    v, Ev = pres[-1], Epres[-1]
    if spec.act == "none":
        y, Ey = v, Ev
    elif spec.act == "sigmoid":
        s = 1.0 / (1.0 + np.exp(-v))
        y, Ey = s, (s * (1 - s) + 0.1 * Ev) * Ev + s * (R_EXP * (1 - s) + 3 * U)
    elif spec.act == "exp_m1":
        t = v - 1.0
        y = np.exp(t)
        Ey = y * np.expm1(Ev + U * np.abs(t)) + R_EXP * y + U * y
    else:
        raise ValueError(spec.act)
    return dict(hs=hs, E_hs=Ehs, pres=pres, E_pres=Epres, y=y, E_y=Ey, margin=margin)


def reference(spec: Spec, layers, x, aux=None, freqs=None, grad_y=None, c_mode: float = 0.0) -> Dict:
    """forward() plus, for grad_y [n, out]: grad_x / E_grad_x (None for posenc: coordinates carry no gradient), dW / E_dW and db / E_db
    (lists, one per layer)."""
    out = forward(spec, layers, x, aux, freqs, c_mode)
    if grad_y is None:
        return out
    gy = np.asarray(grad_y, np.float64)
    n = gy.shape[0]
    v, Ev = out["pres"][-1], out["E_pres"][-1]
    if spec.act == "none":
        d, Ed = gy, np.zeros_like(gy)
    elif spec.act == "sigmoid":
        s = 1.0 / (1.0 + np.exp(-v))
        r = R_EXP * (1 - s) + 3 * U
        f, Ef = s * (1 - s), 0.1 * Ev + s * (1 - s) * (r + 2 * U) + s * s * r
        d, Ed = gy * f, np.abs(gy) * Ef + U * np.abs(gy * f)
    else:
        t = v - 1.0
        tc = np.clip(t, -15.0, 15.0)
        f = np.exp(tc)
        Ef = f * np.expm1(Ev + U * np.abs(t)) + R_EXP * f + U * f
        d, Ed = gy * f, np.abs(gy) * Ef + U * np.abs(gy * f)
    dW, EdW, db, Edb = [None] * len(layers), [None] * len(layers), [None] * len(layers), [None] * len(layers)
    for li in range(len(layers) - 1, -1, -1):
        W = np.asarray(layers[li][0], np.float64)
        h, Eh = out["hs"][li], out["E_hs"][li]
        S = np.abs(d).T @ np.abs(h)
        dW[li] = d.T @ h
        EdW[li] = np.abs(d).T @ Eh + Ed.T @ np.abs(h) + Ed.T @ Eh + ((n + 2) * U + c_mode) * S
        db[li] = d.sum(0)
        Edb[li] = Ed.sum(0) + (n + 2) * U * np.abs(d).sum(0)
        K = W.shape[0]
        g = d @ W
        Eg = Ed @ np.abs(W) + ((K + 2) * U + c_mode) * (np.abs(d) @ np.abs(W))
        if li > 0:
            mask = out["pres"][li - 1] > 0
            d, Ed = g * mask, Eg * mask
    out.update(dW=dW, E_dW=EdW, db=db, E_db=Edb, delta0=d, grad_x=None, E_grad_x=None)
    if spec.enc != "posenc":
        out["grad_x"], out["E_grad_x"] = g[:, spec.x_cols], Eg[:, spec.x_cols]
    return out


def eval32(spec: Spec, layers, x, aux=None, freqs=None, grad_y=None, order: str = "fwd", drop_input_col: Optional[int] = None) -> Dict:
    """The same network in numpy float32 (every intermediate rounded to fp32), in one of two summation orders: "fwd" = numpy's matmul,
    "rev" = the same with every reduction axis reversed.  Returns y, grad_x, dW, db.  ``drop_input_col``: a planted error for the mutation
    tests -- that column of the encoded input is left out of the first layer, forward and backward."""
    f32 = np.float32
    flip = (lambda a, ax: np.ascontiguousarray(np.flip(a, ax))) if order == "rev" else (lambda a, ax: a)

    def mm(a, b):                       # a [m, k] @ b [k, p] in fp32, reduction order by `order`
        return np.matmul(flip(a, 1), flip(b, 0), dtype=f32)
    h, _ = _encode(spec, x, aux, freqs, f32)
    h = h.astype(f32)
    if drop_input_col is not None:
        h = h.copy(); h[:, drop_input_col] = 0
    hs, pres = [], []
    for li, (W, b) in enumerate(layers):
        hs.append(h)
        pre = (mm(h, np.asarray(W, f32).T) + np.asarray(b, f32)).astype(f32)
        pres.append(pre)
        if li + 1 < len(layers):
            h = np.maximum(pre, f32(0))
    v = pres[-1]
    if spec.act == "none":
        y = v
    elif spec.act == "sigmoid":
        y = (f32(1) / (f32(1) + np.exp(-v))).astype(f32)
    else:
        y = np.exp(v - f32(1)).astype(f32)
    res = dict(y=y)
    if grad_y is None:
        return res
    gy = np.asarray(grad_y, f32)
    if spec.act == "none":
        d = gy
    elif spec.act == "sigmoid":
        d = (gy * (y * (f32(1) - y))).astype(f32)
    else:
        d = (gy * np.exp(np.clip(v - f32(1), f32(-15), f32(15)))).astype(f32)
    dW, db = [None] * len(layers), [None] * len(layers)
    for li in range(len(layers) - 1, -1, -1):
        dW[li] = mm(np.ascontiguousarray(d.T), hs[li])
        db[li] = flip(d, 0).sum(0, dtype=f32)
        g = mm(d, np.asarray(layers[li][0], f32))
        if li > 0:
            d = (g * (pres[li - 1] > 0)).astype(f32)
    res.update(dW=dW, db=db, grad_x=None if spec.enc == "posenc" else g[:, spec.x_cols])
    return res


def draw_inputs(spec: Spec, rng: np.random.Generator, m: int):
    """m candidate samples: randn features (posenc: coordinates uniform in [-1, 1)), unit directions"""
    if spec.enc == "posenc":
        return (rng.random((m, 3)) * 2 - 1).astype(np.float32), None
    x = rng.standard_normal((m, spec.in_dim)).astype(np.float32)
    if spec.enc == "none":
        return x, None
    d = rng.standard_normal((m, 3))
    return x, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


class Fixture(NamedTuple):
    spec: Spec
    layers: list
    freqs: Optional[np.ndarray]
    x: np.ndarray
    aux: Optional[np.ndarray]
    grad_y: np.ndarray
    rejected: float          # share of the draws that held a tie unit (0 when ties were not rejected)
    tie_free: bool


def fixture(spec: Spec, n: int, seed: int, layers=None, reject_ties: bool = True, max_draws_factor: int = 64) -> Fixture:
    """n samples for `spec` with torch-default parameters (``layers``: use these instead).  Candidates come from one generator stream,
    one at a time; with ``reject_ties`` a candidate in which some hidden unit has |pre| <= 2 E_pre (bound at the largest c_mode) is
    rejected and the next one takes its place, so n and every sample's position are exact.  ``rejected`` is the share of tie-holding
    candidates among ALL candidates evaluated (whole chunks, at least 32: at n = 1 it is not 1 - 1 / (index of the first tie-free draw),
    which two unlucky draws would push past the cap).  Raises when fewer than n of
    max_draws_factor * n candidates are tie-free (the share is then far above the cap anyway)."""
    layers = make_layers(spec, seed) if layers is None else layers
    freqs = default_freqs(spec.F) if spec.enc != "none" else None
    rng = np.random.default_rng(seed)
    xs, auxs, kept, drawn, ties = [], [], 0, 0, 0
    while kept < n:
        if drawn >= max_draws_factor * n:
            raise RuntimeError(f"{spec}: {kept} tie-free samples in {drawn} draws")
        m = max(32, min(4096, 2 * (n - kept)))
        x, aux = draw_inputs(spec, rng, m)                         # (the chunk size decides how the stream is split between features and
        ok = np.ones(m, bool)                                      # directions: the fixture is a function of (spec, n, seed), not a prefix
        if reject_ties:                                            # of one endless candidate sequence)
            ok = forward(spec, layers, x, aux, freqs, C_MODE_MAX)["margin"] > 0
        idx = np.nonzero(ok)[0][:n - kept]
        drawn += m; ties += int((~ok).sum()); kept += len(idx)
        xs.append(x[idx]); auxs.append(None if aux is None else aux[idx])
    x = np.concatenate(xs)
    aux = None if auxs[0] is None else np.concatenate(auxs)
    gy = np.random.default_rng(seed + 1).standard_normal((n, spec.out)).astype(np.float32)
    return Fixture(spec, layers, freqs, x, aux, gy, ties / drawn, reject_ties)


def compare(got: Dict[str, np.ndarray], ref: Dict, keys: Sequence[str] = ("y", "grad_x", "dW", "db")):
    """-> {name: (largest |got - ref| / bound over the elements, index of that element)}; a value <= 1 is inside the bound.  Per element,
    nothing is normalised by a tensor maximum.  Names: y, grad_x, dW0.., db0.."""
    out = {}

    def one(name, g, r, E):
        g = np.asarray(g, np.float64)
        assert g.shape == r.shape, (name, g.shape, r.shape)
        ratio = np.abs(g - r) / np.maximum(E, 1e-300)
        ratio = np.where(np.isfinite(g), ratio, np.inf)
        k = int(np.argmax(ratio))
        out[name] = (float(ratio.ravel()[k]), np.unravel_index(k, ratio.shape))
    for key in keys:
        if key not in got or got[key] is None:
            continue
        if key in ("dW", "db"):
            for li, g in enumerate(got[key]):
                if g is not None:
                    one(f"{key}{li}", g, ref[key][li], ref["E_" + key][li])
        else:
            one(key, got[key], ref[key], ref["E_" + key])
    return out


# The shallow stacks of tests/test_hip_mlp_fp64.py part A (one or two ReLU layers; deeper stacks reject every sample): name -> (Spec, the
# fixture that selects the arithmetic).  Every kernel family appears as first, hidden -> hidden and last layer: width 64 = mlp.hip /
# mlp_bwd2.hip / mlp_f2_heads.h, widths 128 and 256 = the layer kernels (mlp_bwd_layers.hip, mlp_f2_layers.hip, mlp_fused_f2.hip,
# mlp_b3_layers.hip, mlp_wgrad_rows.hip).
PART_A = {
    "mlp40_64x2_3":      (Spec("none", 40, 0, 64, 1, 3, "none"), "heads"),
    "mlp40_64x1_3":      (Spec("none", 40, 0, 64, 0, 3, "none"), "heads"),          # two-pass backward with a partial second k tile / column block
    "mlp38_64x2_6":      (Spec("none", 38, 0, 64, 1, 6, "none"), "heads"),          # in_dim % 4 != 0, six outputs: generic first layer, MFMA output layer
    "sigma96_64x1_1":    (Spec("none", 96, 0, 64, 0, 1, "exp_m1"), "heads"),        # VanillaOpacityDecoder(96)
    "sigma96_64x2_1":    (Spec("none", 96, 0, 64, 1, 1, "exp_m1"), "heads"),
    "color99_64x2_3":    (Spec("dircat", 48, 8, 64, 1, 3, "sigmoid"), "heads"),     # VanillaColorDecoder(8, 48, 64, 1)
    "color147_64x2_3":   (Spec("dircat", 96, 8, 64, 1, 3, "sigmoid"), "heads"),     # the K-Planes colour head's first layer
    "pe36_64x2_64":      (Spec("posenc", 3, 6, 64, 1, 64, "none"), "heads"),        # VanillaFeatureMLP(6, 64, 1)
    "mlp36_128x1_128":   (Spec("none", 36, 0, 128, 0, 128, "none"), "matmul"),
    "mlp36_128x2_128":   (Spec("none", 36, 0, 128, 1, 128, "none"), "matmul"),      # Cobafa's input width
    "mlp36_128x2_40":    (Spec("none", 36, 0, 128, 1, 40, "none"), "matmul"),       # output below H, not a multiple of 32
    "mlp36_128x2_37":    (Spec("none", 36, 0, 128, 1, 37, "none"), "matmul"),       # output below H, odd: the scalar y stores, a second block with 5 rows
    "mlp147_128x2_288":  (Spec("none", 147, 0, 128, 1, 288, "none"), "matmul"),     # output wider than H
    "pe60_128x2_128":    (Spec("posenc", 3, 10, 128, 1, 128, "none"), "matmul"),
    "color59_128x2_3":   (Spec("dircat", 32, 4, 128, 1, 3, "sigmoid"), "matmul"),    # VanillaColorDecoder(4, 32, 128, 1)
    "pe60_256x1_256":    (Spec("posenc", 3, 10, 256, 0, 256, "none"), "matmul"),
    "pe60_256x2_256":    (Spec("posenc", 3, 10, 256, 1, 256, "none"), "matmul"),    # the Vanilla stack's first, hidden and last layer
    "mlp24_256x2_256":   (Spec("none", 24, 0, 256, 1, 256, "none"), "matmul"),
}
