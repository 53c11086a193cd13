"""fp64 restatement of the SSIM that tn_ssim / run.ssim compute, in numpy -- the yardstick of tests/test_hip_ssim.py.

Single-scale SSIM of Wang et al. 2004 as the NeRF evaluation scripts use it: 11 x 11 window w(i,j) = g(i) g(j),
g(i) = exp(-(i-5)^2 / (2 * 1.5^2)) / sum; one value per window wholly inside the image ("valid") and per channel;
mu = sum w a, var = sum w (a - mu)^2, cov = sum w (a - mu_a)(b - mu_b) (weighted population moments); c1 = (0.01 L)^2, c2 = (0.03 L)^2;
ssim = (2 mu_a mu_b + c1)(2 cov + c2) / ((mu_a^2 + mu_b^2 + c1)(var_a + var_b + c2)); the image's value is the plain mean.

`ssim_map` is the direct 121-tap form with centred moments.  `ssim_map_separable` is the textbook form (two 1-D passes, raw moments)
in fp64, kept as an independent second evaluation.  `ssim_map_emulated` replays candidate fp32 formulations of a kernel tap by tap
(every operation rounded to float32, no fma) so that the choice between them can be re-measured on the CPU."""
import numpy as np

WIN = 11
SIGMA = 1.5


def gauss(dtype=np.float64):
    i = np.arange(WIN, dtype=np.float64)
    g = np.exp(-((i - WIN // 2) ** 2) / (2.0 * SIGMA ** 2))
    return (g / g.sum()).astype(dtype)


def _check(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.ndim == 3 and a.shape == b.shape, (a.shape, b.shape)
    assert a.shape[0] >= WIN and a.shape[1] >= WIN, "no whole window fits"
    return a, b


def _windows(x, oh, ow):
    """the 121 shifted views x[i:i+oh, j:j+ow] with their tap indices"""
    for i in range(WIN):
        for j in range(WIN):
            yield i, j, x[i:i + oh, j:j + ow]


def _combine(mua, mub, vaa, vbb, vab, data_range):
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    return ((2.0 * mua * mub + c1) * (2.0 * vab + c2)) / ((mua * mua + mub * mub + c1) * (vaa + vbb + c2))


def ssim_map(a, b, data_range=1.0):
    """[(H-10), (W-10), C] in float64: direct form, centred moments."""
    a, b = _check(a, b)
    a, b = a.astype(np.float64), b.astype(np.float64)
    g = gauss()
    oh, ow = a.shape[0] - WIN + 1, a.shape[1] - WIN + 1
    mua, mub = np.zeros((oh, ow, a.shape[2])), np.zeros((oh, ow, a.shape[2]))
    for (i, j, wa), (_, _, wb) in zip(_windows(a, oh, ow), _windows(b, oh, ow)):
        mua += g[i] * g[j] * wa
        mub += g[i] * g[j] * wb
    vaa, vbb, vab = np.zeros_like(mua), np.zeros_like(mua), np.zeros_like(mua)
    for (i, j, wa), (_, _, wb) in zip(_windows(a, oh, ow), _windows(b, oh, ow)):
        da, db = wa - mua, wb - mub
        vaa += g[i] * g[j] * da * da
        vbb += g[i] * g[j] * db * db
        vab += g[i] * g[j] * da * db
    return _combine(mua, mub, vaa, vbb, vab, float(data_range))


def ssim(a, b, data_range=1.0):
    return float(ssim_map(a, b, data_range).mean())


def _blur_valid(x, g):
    oh, ow = x.shape[0] - WIN + 1, x.shape[1] - WIN + 1
    rows = sum(g[i] * x[i:i + oh] for i in range(WIN))
    return sum(g[j] * rows[:, j:j + ow] for j in range(WIN))


def ssim_map_separable(a, b, data_range=1.0):
    """the textbook form in float64: separable blur of a, b, a^2, b^2, ab; var = E[a^2] - mu^2"""
    a, b = _check(a, b)
    a, b = a.astype(np.float64), b.astype(np.float64)
    g = gauss()
    mua, mub = _blur_valid(a, g), _blur_valid(b, g)
    vaa = _blur_valid(a * a, g) - mua * mua
    vbb = _blur_valid(b * b, g) - mub * mub
    vab = _blur_valid(a * b, g) - mua * mub
    return _combine(mua, mub, vaa, vbb, vab, float(data_range))


def ssim_map_emulated(a, b, data_range=1.0, form="centred"):
    """float32 replay of a kernel formulation: "raw" (E[a^2] - mu^2 per window), "pivot" (the same after subtracting the images'
    common mean) or "centred" (two passes, sum w (a - mu)^2)."""
    a, b = _check(a, b)
    f = np.float32
    a, b = a.astype(f), b.astype(f)
    if form == "pivot":
        p = f(0.5) * (a.mean(dtype=np.float64).astype(f) + b.mean(dtype=np.float64).astype(f))
        a, b = a - p, b - p
    g = gauss(f)
    oh, ow = a.shape[0] - WIN + 1, a.shape[1] - WIN + 1
    z = lambda: np.zeros((oh, ow, a.shape[2]), f)      # noqa: E731
    mua, mub, saa, sbb, sab = z(), z(), z(), z(), z()
    for (i, j, wa), (_, _, wb) in zip(_windows(a, oh, ow), _windows(b, oh, ow)):
        w = g[i] * g[j]
        mua += w * wa
        mub += w * wb
        if form != "centred":
            saa += w * wa * wa
            sbb += w * wb * wb
            sab += w * wa * wb
    if form == "centred":
        for (i, j, wa), (_, _, wb) in zip(_windows(a, oh, ow), _windows(b, oh, ow)):
            w = g[i] * g[j]
            da, db = wa - mua, wb - mub
            saa += w * da * da
            sbb += w * db * db
            sab += w * da * db
        vaa, vbb, vab = saa, sbb, sab
    else:
        vaa, vbb, vab = saa - mua * mua, sbb - mub * mub, sab - mua * mub
    if form == "pivot":                                  # the luminance factor needs the unshifted means
        mua, mub = mua + p, mub + p
    c1, c2 = f((0.01 * data_range) ** 2), f((0.03 * data_range) ** 2)
    out = ((f(2) * mua * mub + c1) * (f(2) * vab + c2)) / ((mua * mua + mub * mub + c1) * (vaa + vbb + c2))
    assert out.dtype == f
    return out


# ------------------------------------------------------------------------------------------------ seeded test images
def disc_on_white(h, w, c=3, seed=0):
    """a textured disc on an exactly-1.0 background (as Blender scenes have); render = truth + noise of 0.05 inside the disc and
    0.002 outside, clipped to [0, 1].  Returns (truth, render) float32 [h, w, c]."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    r = np.hypot((yy - 0.5 * (h - 1)) / (0.3 * h), (xx - 0.5 * (w - 1)) / (0.3 * w))
    inside = (r < 1.0)[..., None]
    phase = np.arange(c) * 0.7
    tex = 0.5 + 0.35 * np.sin(0.9 * xx[..., None] + phase) * np.cos(0.6 * yy[..., None] - phase)
    truth = np.where(inside, tex, 1.0)
    noise = rng.standard_normal((h, w, c)) * np.where(inside, 0.05, 0.002)
    return truth.astype(np.float32), np.clip(truth + noise, 0.0, 1.0).astype(np.float32)


def uniform_noise(h, w, c=3, seed=0):
    rng = np.random.default_rng(seed)
    return rng.random((h, w, c), dtype=np.float32), rng.random((h, w, c), dtype=np.float32)


def ramp(h, w, c=3, seed=0):
    """a smooth ramp against the ramp plus 1e-3"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    base = (0.1 + 0.8 * (xx / max(w - 1, 1) * 0.6 + yy / max(h - 1, 1) * 0.4))[..., None] * (1.0 - 0.1 * np.arange(c))
    return base.astype(np.float32), (base + 1e-3).astype(np.float32)


def clipped(h, w, c=3, seed=0):
    """a render that over- and undershoots before it is clipped to [0, 1]: flat runs of exact 0.0 and 1.0 beside texture"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    truth = 0.5 + 0.45 * np.sin(0.21 * xx + 0.13 * yy)[..., None] * np.cos(0.05 * xx[..., None] + np.arange(c))
    render = 0.5 + 1.4 * (truth - 0.5) + 0.02 * rng.standard_normal((h, w, c))
    return np.clip(truth, 0.0, 1.0).astype(np.float32), np.clip(render, 0.0, 1.0).astype(np.float32)


PATTERNS = {"disc": disc_on_white, "noise": uniform_noise, "ramp": ramp, "clipped": clipped}
