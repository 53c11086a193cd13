"""numpy float64 yardstick of the optimiser pass and the K-Planes plane regularisers (include/tinynerf_hip.h: tn_adam_step,
tn_adam_multi, tn_adam_multi_gated, tn_adam_reg_multi, tn_plane_reg_fwd / _bwd / _multi).  Plain formulas on whole arrays, no
kernel of the package behind them: inputs are the float32 arrays the kernels see, every operation after that is float64.

Planes are channel-last [H, W, C].  A row range (row0, row1) restricts a result to the rows a rank owns in the sharded pass: the
owner of row y counts the vertical pair (y, y + 1), the horizontal pairs and the |p| of row y; the gradient stencil of an owned
row still reads its neighbours in the full plane."""
import numpy as np


def adam(p, g, m, v, step, lr, b1, b2, eps, wd):
    """one step of torch.optim.Adam (coupled weight decay, no amsgrad): returns (p, m, v)"""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    gg = g + wd * p
    m = m + (gg - m) * (1.0 - b1)
    v = b2 * v + (1.0 - b2) * gg * gg
    bc1 = 1.0 - float(b1) ** step
    bc2 = 1.0 - float(b2) ** step
    denom = np.sqrt(v) / np.sqrt(bc2) + eps
    return p - (lr / bc1) * (m / denom), m, v


def _rows(H, rows):
    row0, row1 = (0, H) if rows is None else rows
    assert 0 <= row0 < row1 <= H, (row0, row1, H)
    return row0, row1


def _stencils(plane):
    """(dy, dx): d/dp of sum (p[y+1] - p[y])^2 / 2 and of sum (p[x+1] - p[x])^2 / 2, on the full plane"""
    q = np.asarray(plane, dtype=np.float64)
    dy, dx = np.zeros_like(q), np.zeros_like(q)
    dy[1:] += q[1:] - q[:-1]
    dy[:-1] -= q[1:] - q[:-1]
    dx[:, 1:] += q[:, 1:] - q[:, :-1]
    dx[:, :-1] -= q[:, 1:] - q[:, :-1]
    return q, dy, dx


def plane_reg(plane, cy, cx, cl1, upstream, rows=None):
    """(sums, grad): sums = [sum (dy p)^2, sum (dx p)^2, sum |p|] over the pairs / texels the rows own, grad [row1 - row0, W, C] =
    upstream * (2 cy * dy-stencil + 2 cx * dx-stencil + cl1 * sign(p)) of those rows; sign(+0) = sign(-0) = 0"""
    q, dy, dx = _stencils(plane)
    H = q.shape[0]
    row0, row1 = _rows(H, rows)
    own = q[row0:row1]
    below = q[row0 + 1:min(row1 + 1, H)] - q[row0:min(row1, H - 1)]        # pairs (y, y + 1) with y owned
    across = own[:, 1:] - own[:, :-1]
    sums = np.array([np.sum(below * below), np.sum(across * across), np.sum(np.abs(own))], dtype=np.float64)
    sign = (own > 0).astype(np.float64) - (own < 0).astype(np.float64)
    grad = upstream * (2.0 * cy * dy[row0:row1] + 2.0 * cx * dx[row0:row1] + cl1 * sign)
    return sums, grad


def plane_reg_magnitude(plane, cy, cx, cl1, upstream, rows=None):
    """the sum of the magnitudes of the terms of plane_reg's gradient, with every difference p - q counted as |p| + |q|: what a
    forward-error bound of an fp32 evaluation is relative to"""
    a = np.abs(np.asarray(plane, dtype=np.float64))
    H = a.shape[0]
    row0, row1 = _rows(H, rows)
    my, mx = np.zeros_like(a), np.zeros_like(a)
    my[1:] += a[1:] + a[:-1]
    my[:-1] += a[1:] + a[:-1]
    mx[:, 1:] += a[:, 1:] + a[:, :-1]
    mx[:, :-1] += a[:, 1:] + a[:, :-1]
    mag = abs(upstream) * (2.0 * abs(cy) * my + 2.0 * abs(cx) * mx + abs(cl1) * (a != 0))
    return mag[row0:row1]


def adam_reg(p, g, m, v, step, lr, b1, b2, eps, wd, cy, cx, cl1, upstream, rows=None):
    """tn_adam_reg_item with H > 0: g += regulariser gradient of the current plane, then adam(); everything [H, W, C], results for
    the owned rows only.  Returns (p, m, v, sums)."""
    H = np.asarray(p).shape[0]
    row0, row1 = _rows(H, rows)
    sums, rg = plane_reg(p, cy, cx, cl1, upstream, rows)
    own = slice(row0, row1)
    g_total = np.asarray(g, dtype=np.float64)[own] + rg
    po, mo, vo = adam(np.asarray(p)[own], g_total, np.asarray(m)[own], np.asarray(v)[own], step, lr, b1, b2, eps, wd)
    return po, mo, vo, sums
