"""float64 yardstick of the multiresolution hash grid (definition: include/tinynerf_hip.h).  numpy only; nothing here comes
from the kernel or from tinynerf_amd.models.

The position p = x * (N/2) + N/2 is formed in float64 from the fp32 input and rounded to fp32 ONCE -- the single rounding of the
kernel's fmaf (the float64 product of an fp32 x and N/2 is exact, the sum carries one float64 rounding far below fp32's) -- the cell i
and the fraction f are taken from that fp32 p; weights, interpolation and the scatter are float64 from there on."""
import math

import numpy as np

P1, P2 = 2654435761, 805459861          # the primes of Instant-NGP (the first axis is multiplied by 1)

SMALL = dict(n_levels=4, log2_T=8, n_min=2, n_max=32)
FINE = dict(n_levels=16, log2_T=14, n_min=16, n_max=2048)
DEFAULT = dict(n_levels=16, log2_T=19, n_min=16, n_max=2048)


def levels(n_levels, log2_T, n_min, n_max):
    """-> (res, hashed, entries, offsets), python ints / bools"""
    b = math.exp(math.log(n_max / n_min) / (n_levels - 1)) if n_levels > 1 else 1.0
    T = 1 << log2_T
    res, hashed, entries, offsets = [], [], [], []
    total = 0
    for l in range(n_levels):
        n_l = int(math.floor(n_min * b ** l + 0.5))
        nodes = (n_l + 1) ** 3
        dense = nodes <= T
        res.append(n_l)
        hashed.append(not dense)
        entries.append((nodes + 7) // 8 * 8 if dense else T)
        offsets.append(total)
        total += entries[-1]
    return res, hashed, entries, offsets


def total_entries(plan):
    return plan[3][-1] + plan[2][-1]


def cell(x, n_l):
    """x [n, 3] fp32 -> (i [n, 3] int64, f [n, 3] float64 holding fp32 values)"""
    x = np.asarray(x, np.float32)
    h = 0.5 * n_l
    with np.errstate(invalid="ignore", over="ignore"):
        p = (x.astype(np.float64) * h + h).astype(np.float32)
    p = np.where(p > 0, p, np.float32(0))                  # a NaN lands on 0
    p = np.where(p < n_l, p, np.float32(n_l)).astype(np.float32)
    i = np.minimum(p.astype(np.int64), n_l - 1)
    f = p.astype(np.float64) - i
    return i, f


def node_index(ix, iy, iz, n_l, hashed, T):
    ix, iy, iz = (np.asarray(v, np.uint64) for v in (ix, iy, iz))
    if hashed:
        m = np.uint64(0xFFFFFFFF)
        return ((ix ^ ((iy * np.uint64(P1)) & m) ^ ((iz * np.uint64(P2)) & m)) & np.uint64(T - 1)).astype(np.int64)
    s = np.uint64(n_l + 1)
    return (ix + s * (iy + s * iz)).astype(np.int64)


def corners(x, plan, l):
    """-> (rows [n, 8] int64 into the table, w [n, 8] float64)"""
    res, hashed, entries, offsets = plan
    i, f = cell(x, res[l])
    rows, ws = [], []
    for k in range(8):
        d = np.array([k & 1, (k >> 1) & 1, k >> 2])
        w = np.prod(np.where(d[None, :] == 1, f, 1.0 - f), axis=1)
        idx = node_index(i[:, 0] + d[0], i[:, 1] + d[1], i[:, 2] + d[2], res[l], hashed[l], entries[l])
        assert idx.min(initial=0) >= 0 and idx.max(initial=0) < entries[l]
        rows.append(offsets[l] + idx)
        ws.append(w)
    return np.stack(rows, 1), np.stack(ws, 1)


def forward(table, x, plan):
    """table [E, F] -> feat [n, L * F] float64"""
    table = np.asarray(table, np.float64)
    F = table.shape[1]
    n, L = len(x), len(plan[0])
    feat = np.zeros((n, L * F))
    for l in range(L):
        rows, w = corners(x, plan, l)
        feat[:, l * F:(l + 1) * F] = (w[:, :, None] * table[rows]).sum(1)
    return feat


def backward(grad_feat, x, plan, features):
    """-> (grad_table [E, F] float64, m [E] contributions per entry, abs_sum [E, F] = sum |terms|)"""
    g = np.asarray(grad_feat, np.float64)
    E, L = total_entries(plan), len(plan[0])
    grad, m, abs_sum = np.zeros((E, features)), np.zeros(E, np.int64), np.zeros((E, features))
    for l in range(L):
        rows, w = corners(x, plan, l)
        terms = w[:, :, None] * g[:, None, l * features:(l + 1) * features]
        np.add.at(grad, rows.reshape(-1), terms.reshape(-1, features))
        np.add.at(abs_sum, rows.reshape(-1), np.abs(terms).reshape(-1, features))
        np.add.at(m, rows.reshape(-1), 1)
    return grad, m, abs_sum


def sample_points(n, plan, seed):
    """n fp32 points: mostly U(-1, 1); the rest corners +-1, exact node positions, values just outside the range, and runs of 64
    points along a line (the packed-ray pattern: neighbouring lanes in one cell)"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    if n >= 31:
        x[1] = [1, 1, 1]
        x[2] = [-1, -1, -1]
        x[3] = [1, -1, 1]
        n_l = plan[0][min(1, len(plan[0]) - 1)]
        x[4:10] = (rng.integers(0, n_l + 1, (6, 3)) * (2.0 / n_l) - 1.0).astype(np.float32)          # nodes of a coarse level
        x[10] = [np.nextafter(np.float32(1), np.float32(2)), -1.0000001, 1.5]
        x[11] = [-2.0, 3.0, np.nextafter(np.float32(-1), np.float32(-2))]
        x[12] = [1e30, -1e30, 0.25]
        x[13] = [np.nan, 0.5, -np.inf]
    start = 40
    while start + 64 <= n and start < 40 + 64 * 6:
        o, d = rng.uniform(-0.6, 0.6, 3), rng.normal(size=3)
        d /= np.linalg.norm(d)
        step = [0.0005, 0.004, 0.02][(start // 64) % 3]
        x[start:start + 64] = np.clip(o + d * step * np.arange(64)[:, None], -1, 1).astype(np.float32)
        start += 64 + 5
    return x
