"""float64 yardstick of the surface normals (definition: include/tinynerf_hip.h).  numpy only; nothing here comes from the
kernels or from tinynerf_amd.

Only the quantities that choose a CELL are formed in fp32, exactly as the kernels form them, so that the yardstick differentiates
inside the cell the kernel interpolates in: ix, iy of a K-Planes lookup (one rounding per operation) and p of a hash-grid axis (one fused
rounding; tests/_hashgrid_ref.cell).  Everything after that is float64.

Every gradient comes back as (value, A): A is the sum of the absolute values of the terms of the nested sum
    grad_a = sum_j sum_c sum_taps  w2_j [h_j > 0] W1_jc * (a tap's term of df_c/dx_a),
the quantity an fp32 evaluation's error is proportional to whatever order it sums in."""
import numpy as np

import _hashgrid_ref as hg

NONE, AABB, MIP_INF, MIP_L2 = 3, 0, 1, 2          # TN_CONTRACT_*
PAIRS = ((0, 1), (0, 2), (1, 2))                  # (u, v) axes of the three planes of a scale
EPS = 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------------------ the head
def head(W1, b1, w2, f, f_abs=None):
    """f [n, F] -> (g [n, F] = dy/df, g_abs [n, F] = sum_j |W1_jc w2_j| [h_j > 0], tie [n] bool, y_hidden = h [n, 64]).
    tie: some |h_j| <= 1e-5 (sum_c |W1_jc f_c| + |b1_j|) -- a ReLU bit an fp32 evaluation may set the other way."""
    W1, b1, w2, f = (np.asarray(v, np.float64) for v in (W1, b1, w2, f))
    w2 = w2.reshape(-1)
    h = f @ W1.T + b1
    mag = np.abs(f) @ np.abs(W1).T + np.abs(b1)
    with np.errstate(invalid="ignore"):
        on = h > 0
        tie = (np.abs(h) <= 1e-5 * mag).any(1) | ~np.isfinite(h).all(1)
    a = np.where(on, w2[None, :], 0.0)
    return a @ W1, np.abs(a) @ np.abs(W1), tie, h


def y_of(W1, b1, w2, b2, f):
    f = np.asarray(f, np.float64)
    h = f @ np.asarray(W1, np.float64).T + np.asarray(b1, np.float64)
    return np.maximum(h, 0) @ np.asarray(w2, np.float64).reshape(-1) + float(b2)


# ------------------------------------------------------------------------------------------------------------------------ K-Planes
def plane_pos(u, size):
    """fp32, one rounding per operation, as tn::plane_taps: ix = ((u + 1) * 0.5) * (size - 1) -> float64 holding the fp32 value"""
    u = np.asarray(u, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        u1 = (u + np.float32(1)).astype(np.float32)
        return ((u1 * np.float32(0.5)).astype(np.float32) * np.float32(size - 1)).astype(np.float32).astype(np.float64)


def plane_lookup(plane, u, v, fp32_pos=True):
    """plane [H, W, C]; u indexes W, v indexes H -> (P, dP/du, dP/dv, |P|, |dP/du|, |dP/dv|), each [n, C] float64; the last three are the
    sums of the absolute values of the terms.  fp32_pos False: the position in float64 (the self-check differentiates THAT function)."""
    plane = np.asarray(plane, np.float64)
    H, W, C = plane.shape
    if fp32_pos:
        ix, iy = plane_pos(u, W), plane_pos(v, H)
    else:
        ix, iy = (np.asarray(u, np.float64) + 1) * 0.5 * (W - 1), (np.asarray(v, np.float64) + 1) * 0.5 * (H - 1)
    with np.errstate(invalid="ignore"):
        x0, y0 = np.floor(ix), np.floor(iy)
        fx, fy = ix - x0, iy - y0
        gx, gy = (x0 + 1) - ix, (y0 + 1) - iy

    def tap(yy, xx):
        with np.errstate(invalid="ignore"):
            ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        xi, yi = np.where(ok, xx, 0).astype(np.int64), np.where(ok, yy, 0).astype(np.int64)
        return np.where(ok[:, None], plane[yi, xi], 0.0)

    nw, ne, sw, se = tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
    c = lambda w: w[:, None]                                                                                   # noqa: E731
    P = nw * c(gx * gy) + ne * c(fx * gy) + sw * c(gx * fy) + se * c(fx * fy)
    Pa = np.abs(nw) * c(np.abs(gx * gy)) + np.abs(ne) * c(np.abs(fx * gy)) + np.abs(sw) * c(np.abs(gx * fy)) + np.abs(se) * c(np.abs(fx * fy))
    su, sv = 0.5 * (W - 1), 0.5 * (H - 1)
    dU = su * ((ne - nw) * c(gy) + (se - sw) * c(fy))
    dV = sv * ((sw - nw) * c(gx) + (se - ne) * c(fx))
    dUa = su * ((np.abs(ne) + np.abs(nw)) * c(np.abs(gy)) + (np.abs(se) + np.abs(sw)) * c(np.abs(fy)))
    dVa = sv * ((np.abs(sw) + np.abs(nw)) * c(np.abs(gx)) + (np.abs(se) + np.abs(ne)) * c(np.abs(fx)))
    return P, dU, dV, Pa, dUa, dVa


def kplanes_features(planes, x, fp32_pos=True):
    """planes[s][p] [H, W, C] -> (f [n, S C], df [3][n, S C], |f| terms, |df| terms [3][n, S C])"""
    x = np.asarray(x, np.float32 if fp32_pos else np.float64)
    f, fa, df, dfa = [], [], [[], [], []], [[], [], []]
    for scale in planes:
        L = [plane_lookup(scale[p], x[:, PAIRS[p][0]], x[:, PAIRS[p][1]], fp32_pos) for p in range(3)]
        P, U, V, Pa, Ua, Va = ([l[k] for l in L] for k in range(6))
        f.append(P[0] * P[1] * P[2])
        fa.append(Pa[0] * Pa[1] * Pa[2])
        # x0 is u of planes 0 and 1; x1 is v of plane 0 and u of plane 2; x2 is v of planes 1 and 2
        df[0].append(U[0] * P[1] * P[2] + P[0] * U[1] * P[2]); dfa[0].append(Ua[0] * Pa[1] * Pa[2] + Pa[0] * Ua[1] * Pa[2])
        df[1].append(V[0] * P[1] * P[2] + P[0] * P[1] * U[2]); dfa[1].append(Va[0] * Pa[1] * Pa[2] + Pa[0] * Pa[1] * Ua[2])
        df[2].append(P[0] * V[1] * P[2] + P[0] * P[1] * V[2]); dfa[2].append(Pa[0] * Va[1] * Pa[2] + Pa[0] * Pa[1] * Va[2])
    cat = lambda v: np.concatenate(v, 1)                                                                       # noqa: E731
    return cat(f), [cat(d) for d in df], cat(fa), [cat(d) for d in dfa]


# ----------------------------------------------------------------------------------------------------------------------- hash grid
def hashgrid_features(table, x, plan, fp32_pos=True):
    """-> (f [n, L F], df [3][n, L F], |f| terms, |df| terms): the derivative inside the cell _hashgrid_ref.cell chooses, 0 on an axis
    where the clamp acts (p = fmaf(x, N/2, N/2) < 0, > N or NaN).  fp32_pos False: p in float64 (the self-check differentiates THAT function)"""
    table = np.asarray(table, np.float64)
    x = np.asarray(x, np.float32 if fp32_pos else np.float64)
    F = table.shape[1]
    res, hashed, entries, offsets = plan
    n, L = len(x), len(res)
    f, fa = np.zeros((n, L * F)), np.zeros((n, L * F))
    df, dfa = [np.zeros((n, L * F)) for _ in range(3)], [np.zeros((n, L * F)) for _ in range(3)]
    for l in range(L):
        N = res[l]
        with np.errstate(invalid="ignore", over="ignore"):
            p = x.astype(np.float64) * (0.5 * N) + 0.5 * N
            if fp32_pos:
                i, fr = hg.cell(x, N)
                p = p.astype(np.float32)
            else:
                pc = np.clip(p, 0, N)
                i = np.minimum(np.floor(pc), N - 1).astype(np.int64)
                fr = pc - i
            live = (p >= 0) & (p <= N)
        sl = slice(l * F, (l + 1) * F)
        for k in range(8):
            d = np.array([k & 1, (k >> 1) & 1, k >> 2])
            w1 = np.where(d[None, :] == 1, fr, 1.0 - fr)                              # per-axis weights [n, 3]
            idx = hg.node_index(i[:, 0] + d[0], i[:, 1] + d[1], i[:, 2] + d[2], N, hashed[l], entries[l])
            t = table[offsets[l] + idx]
            f[:, sl] += w1.prod(1)[:, None] * t
            fa[:, sl] += w1.prod(1)[:, None] * np.abs(t)
            for a in range(3):
                others = w1[:, (a + 1) % 3] * w1[:, (a + 2) % 3]
                term = np.where(live[:, a], 0.5 * N * (1.0 if d[a] else -1.0) * others, 0.0)[:, None] * t
                df[a][:, sl] += term
                dfa[a][:, sl] += np.abs(term)
    return f, df, fa, dfa


# ------------------------------------------------------------------------------------------------------------- gradient of y w.r.t. x
def gradient(W1, b1, w2, f, df, dfa):
    """-> (grad [n, 3], A [n, 3], tie [n])"""
    g, ga, tie, _ = head(W1, b1, w2, f)
    grad = np.stack([(g * df[a]).sum(1) for a in range(3)], 1)
    A = np.stack([(ga * dfa[a]).sum(1) for a in range(3)], 1)
    return grad, A, tie


def kplanes_gradient(planes, x, W1, b1, w2):
    f, df, _, dfa = kplanes_features(planes, x)
    return gradient(W1, b1, w2, f, df, dfa)


def hashgrid_gradient(table, x, plan, W1, b1, w2):
    f, df, _, dfa = hashgrid_features(table, x, plan)
    return gradient(W1, b1, w2, f, df, dfa)


def grad_bound(A, F):
    """|fp32 - exact| <= (F + 64 + 16) 2^-24 A per element: the worst case of any summation order over the nested sum"""
    return (F + 64 + 16) * EPS * A


# ----------------------------------------------------------------------------------------------------------------- the world frame
def contract(X, order):
    """reference src/core.py:18-19 in float64"""
    X = np.asarray(X, np.float64)
    m = np.abs(X).max(-1, keepdims=True) if np.isinf(order) else np.sqrt((X * X).sum(-1, keepdims=True))
    return np.where(m <= 1, X, (2 - 1 / np.maximum(m, 1e-300)) * X / np.maximum(m, 1e-300)) / 2


def jacobian(kind, x, aabb=None, fp32_x=True):
    """J = dx/dX [n, 3, 3] from the contracted x [n, 3] alone, as the header defines it (J = 0 where v = 0 is prescribed)"""
    x = np.asarray(x, np.float32).astype(np.float64) if fp32_x else np.asarray(x, np.float64)
    n = len(x)
    eye = np.broadcast_to(np.eye(3), (n, 3, 3)).copy()
    if kind == NONE:
        return eye
    if kind == AABB:
        aabb = np.asarray(aabb, np.float32).astype(np.float64).reshape(6)
        return eye * (2.0 / (aabb[3:] - aabb[:3]))[None, None, :]
    u = 2 * x
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.abs(u).max(1) if kind == MIP_INF else np.sqrt((u * u).sum(1))
        s = np.where(np.isnan(u).any(1), np.nan, s)
        inside, dead = s <= 1, ~(s < 2)
    J = np.zeros((n, 3, 3))
    J[inside] = 0.5 * np.eye(3)
    mid = ~inside & ~dead
    if mid.any():
        um, sm = u[mid], s[mid]
        m = 1 / (2 - sm)
        X = (m / sm)[:, None] * um
        if kind == MIP_INF:
            k = np.argmax(np.abs(um) == sm[:, None], 1)                                # the lowest axis with |u_k| = s
            dm = np.zeros_like(um)
            dm[np.arange(len(um)), k] = np.sign(um[np.arange(len(um)), k])
        else:
            dm = X / m[:, None]
        A_, B_ = 2 / m - 1 / m ** 2, 2 / m ** 3 - 2 / m ** 2
        J[mid] = 0.5 * (A_[:, None, None] * np.eye(3) + B_[:, None, None] * X[:, :, None] * dm[:, None, :])
    return J


def normals(kind, x, grad, bound, aabb=None):
    """-> (n [rows, 3] unit or 0, v, bound_v [rows, 3] = |J|^T bound, ok [rows] = |v| finite and > 0 and x finite)"""
    J = jacobian(kind, x, aabb)
    with np.errstate(invalid="ignore", over="ignore"):
        v = -np.einsum("nij,ni->nj", J, np.where(np.isfinite(grad), grad, 0.0))
        bv = np.einsum("nij,ni->nj", np.abs(J), np.where(np.isfinite(bound), bound, 0.0))
        norm = np.sqrt((v * v).sum(1))
    ok = np.isfinite(norm) & (norm > 0) & np.isfinite(np.asarray(x, np.float64)).all(1) & np.isfinite(grad).all(1)
    nrm = np.where(ok[:, None], v / np.where(ok, norm, 1.0)[:, None], 0.0)
    return nrm, v, bv, ok


def ray_normals(weights, nrm, info):
    """-> (N [R, 3] = sum w n, |terms| [R, 3], counts [R])"""
    w, nrm = np.asarray(weights, np.float64), np.asarray(nrm, np.float64)
    R = len(info)
    N, A = np.zeros((R, 3)), np.zeros((R, 3))
    for r, (s, c) in enumerate(np.asarray(info)):
        N[r] = (w[s:s + c, None] * nrm[s:s + c]).sum(0)
        A[r] = np.abs(w[s:s + c, None] * nrm[s:s + c]).sum(0)
    return N, A, np.asarray(info)[:, 1].astype(np.int64)


# -------------------------------------------------------------------------------------------------------------------------- inputs
def make_head(F, seed, positive=False):
    """W1 ~ U(-0.2, 1), b1 ~ U(-0.05, 0.05), w2 ~ U(0.2, 1): about half of the hidden units are on behind features of either sign, and the
    sum over the hidden units cancels little -- with weights of either sign the bound on a NORMAL (2 bound(v) / |v|) passes 1e-2 on 3 - 7 %
    of the rows at F = 96, above the 1 % cap on rows left to the gradient comparison.  positive: every h_j > 0 for f >= 0 (the analytic
    cases)."""
    rng = np.random.default_rng(seed)
    W1 = rng.uniform(-0.2, 1, (64, F)).astype(np.float32)
    b1 = rng.uniform(-0.05, 0.05, 64).astype(np.float32)
    w2 = rng.uniform(0.2, 1, (1, 64)).astype(np.float32)
    if positive:
        W1, b1 = np.abs(W1), np.abs(b1) + np.float32(0.1)
    return W1, b1, w2, np.float32(0.25)


def make_planes(n_scales, C, sizes, seed):
    """sizes: (H, W) per scale; U(-1, 1) texels: the features are products of uniforms"""
    rng = np.random.default_rng(seed)
    return [[rng.uniform(-1, 1, (H, W, C)).astype(np.float32) for _ in range(3)] for (H, W) in sizes[:n_scales]]


def linear_hashgrid(N, features, a, seed):
    """One dense level of N cells per axis whose entry at node q holds beta_c <a, pos(q)> + gamma_c, pos = 2 q / N - 1 and beta > 0: the
    trilinear interpolant IS that linear function, so behind a head with every h_j > 0 (make_head(positive=True)) and positive w2 the
    density gradient is a positive multiple of a everywhere inside -> the normal is -a / |a|.  -> (plan, table fp32)"""
    rng = np.random.default_rng(seed)
    plan = ([N], [False], [((N + 1) ** 3 + 7) // 8 * 8], [0])
    q = np.arange(N + 1)
    iz, iy, ix = np.meshgrid(q, q, q, indexing="ij")                              # index = ix + S (iy + S iz)
    pos = np.stack([ix, iy, iz], -1).reshape(-1, 3) * (2.0 / N) - 1.0
    beta, gamma = rng.uniform(0.5, 1.5, features), rng.uniform(0.5, 1.0, features) + 2.0 * np.abs(a).sum()
    table = np.zeros((plan[2][0], features), np.float32)
    table[:len(pos)] = (pos @ np.asarray(a, np.float64))[:, None] * beta + gamma
    return plan, table


def x0_planes(n_scales, C, sizes, seed):
    """K-Planes planes that vary along x0 only and increase with it (positive values): planes 0 and 1 (u = x0 indexes W) are functions of
    the column, plane 2 (x1, x2) is constant.  Behind a positive head the density increases with x0 -> the normal is -e0."""
    rng = np.random.default_rng(seed)
    out = []
    for (H, W) in sizes[:n_scales]:
        col = lambda: np.cumsum(rng.uniform(0.1, 1.0, (W, C)), 0)                                                # noqa: E731
        out.append([np.broadcast_to(col()[None], (H, W, C)).astype(np.float32).copy() for _ in range(2)]
                   + [np.broadcast_to(rng.uniform(0.5, 1.5, C)[None, None], (H, W, C)).astype(np.float32).copy()])
    return out
