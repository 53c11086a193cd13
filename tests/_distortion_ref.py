"""fp64 yardstick of the distortion loss (tn_distortion_fwd / tn_distortion_bwd): the pairwise definition, O(n^2) per ray, numpy.

    L_r       = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 d_i
    dL_r/dw_i = 2 sum_j w_j |m_i - m_j| + (2/3) w_i d_i

with x = (t - near) / range and  m = x, d = step / range (LINEAR)  or  m = g(x), d = g'(x) step / range, g(x) = x / 2 below 1 and
1 - 1 / (2 x) from there on (UNBOUNDED).  Inputs are taken as they come (callers round them to fp32 first where the kernels' inputs
are fp32) and everything behind that is fp64."""
import numpy as np

LINEAR, UNBOUNDED = 0, 1


def g(x):
    x = np.asarray(x, dtype=np.float64)
    safe = np.where(x < 1.0, 1.0, x)
    return np.where(x < 1.0, 0.5 * x, 1.0 - 0.5 / safe)


def g_prime(x):
    x = np.asarray(x, dtype=np.float64)
    safe = np.where(x < 1.0, 1.0, x)
    return np.where(x < 1.0, 0.5, 0.5 / (safe * safe))


def f(u):
    """the unbounded marcher's map from its uniform parameter u in [0, 1) to x (reference core.py:52): g's inverse"""
    u = np.asarray(u, dtype=np.float64)
    return np.where(u < 0.5, 2.0 * u, 1.0 / (2.0 - 2.0 * u))


def warp_md(t, step, warp, near, rng):
    t, step = np.asarray(t, dtype=np.float64), np.asarray(step, dtype=np.float64)
    x = (t - float(near)) / float(rng)
    if warp == LINEAR:
        return x, step / float(rng)
    if warp == UNBOUNDED:
        return g(x), g_prime(x) * step / float(rng)
    raise ValueError(warp)


def ray_loss_and_grad(w, m, d):
    """one ray from (w, m, d): (L, dL/dw [n]), pairwise"""
    w, m, d = (np.asarray(a, dtype=np.float64) for a in (w, m, d))
    if w.size == 0:
        return 0.0, np.zeros(0)
    dist = np.abs(m[:, None] - m[None, :])
    pair = dist @ w                                  # sum_j w_j |m_i - m_j|
    loss = float(w @ pair + (w * w * d).sum() / 3.0)
    return loss, 2.0 * pair + (2.0 / 3.0) * w * d


def distortion(weights, t, steps, info, warp, near, rng):
    """packed rays: (loss [R], dloss_r/dw [N]); samples no ray owns keep gradient 0"""
    weights, t, steps = (np.asarray(a, dtype=np.float64) for a in (weights, t, steps))
    info = np.asarray(info)
    loss = np.zeros(info.shape[0])
    grad = np.zeros_like(weights)
    for r, (start, count) in enumerate(info):
        sl = slice(int(start), int(start) + int(count))
        m, d = warp_md(t[sl], steps[sl], warp, near, rng)
        loss[r], grad[sl] = ray_loss_and_grad(weights[sl], m, d)
    return loss, grad
