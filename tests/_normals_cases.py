"""The cases of tests/test_hip_normals.py and their float64 references (tests/_normals_ref.py), computed once per (case, n) and shared:
the CPU suite holds the seeds to the cap on skipped rows (tests/test_normals_ref.py), the GPU suite compares the kernels against them.
numpy only."""
import functools

import numpy as np

import _hashgrid_ref as hg
import _normals_ref as ref

NS = (1, 31, 32, 33, 197, 2051)
FRAMES = (ref.NONE, ref.AABB, ref.MIP_INF, ref.MIP_L2)
BOX = (-1.0, -3.0, -0.5, 2.0, 1.0, 4.0)              # the AABB frame: not a cube

# K-Planes: (H, W) per scale and channels; hash grid: a plan of tests/_hashgrid_ref.py and features
CASES = {
    "kplanes_3x32_r4_9_16": dict(field="kplanes", sizes=[(4, 4), (9, 9), (16, 16)], C=32, seed=11),
    "kplanes_2x8_6x11": dict(field="kplanes", sizes=[(6, 11), (6, 11)], C=8, seed=12),
    "kplanes_1x4": dict(field="kplanes", sizes=[(5, 5)], C=4, seed=13),
    "hashgrid_small_f2": dict(field="hashgrid", plan=hg.SMALL, features=2, seed=14),
    "hashgrid_small_f4": dict(field="hashgrid", plan=hg.SMALL, features=4, seed=15),
    "hashgrid_fine_f2": dict(field="hashgrid", plan=hg.FINE, features=2, seed=16),
}


@functools.lru_cache(maxsize=None)
def model(name):
    """the field's parameters and the head of a case (fp32 arrays)"""
    c = CASES[name]
    if c["field"] == "kplanes":
        planes = ref.make_planes(len(c["sizes"]), c["C"], c["sizes"], c["seed"])
        F = len(c["sizes"]) * c["C"]
        m = dict(field="kplanes", planes=planes, F=F)
    else:
        plan = hg.levels(**c["plan"])
        table = np.random.default_rng(c["seed"]).uniform(-1, 1, (hg.total_entries(plan), c["features"])).astype(np.float32)
        F = len(plan[0]) * c["features"]
        m = dict(field="hashgrid", plan=plan, table=table, F=F)
    m["W1"], m["b1"], m["w2"], m["b2"] = ref.make_head(F, c["seed"] + 100)
    return m


def points(name, n):
    """tests/_hashgrid_ref.sample_points: nodes, +-1, just outside, huge, NaN, runs along a line (n >= 31)"""
    plan = model(name).get("plan") or hg.levels(**hg.SMALL)
    return hg.sample_points(n, plan, CASES[name]["seed"] + n)


def gradient(m, x):
    if m["field"] == "kplanes":
        return ref.kplanes_gradient(m["planes"], x, m["W1"], m["b1"], m["w2"])
    return ref.hashgrid_gradient(m["table"], x, m["plan"], m["W1"], m["b1"], m["w2"])


@functools.lru_cache(maxsize=None)
def reference(name, n):
    """x [n,3] fp32, grad / bound [n,3] float64, tie / finite [n] bool, normals[kind] = dict(n, tol, loose, zero):
    tol = 2 bound(v) / |v_ref| + 8 2^-24 per row, loose = tol > 1e-2 (left to the gradient comparison), zero = v_ref is 0 with a zero
    bound (the kernel must give exactly 0)"""
    m = model(name)
    x = points(name, n)
    grad, A, tie = gradient(m, x)
    bound = ref.grad_bound(A, m["F"])
    finite = np.isfinite(x).all(1)
    out = dict(x=x, grad=grad, bound=bound, tie=tie, finite=finite, normals={})
    for kind in FRAMES:
        nrm, v, bv, ok = ref.normals(kind, x, grad, bound, BOX)
        vnorm = np.sqrt((v * v).sum(1))
        bvn = np.sqrt((bv * bv).sum(1))
        zero = (vnorm == 0) & (bvn == 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            tol = np.where(ok, 2 * bvn / np.where(ok, vnorm, 1.0), np.inf) + 8 * ref.EPS
        loose = ~zero & ~(tol <= 1e-2)
        out["normals"][kind] = dict(n=nrm, tol=tol, loose=loose, zero=zero)
    return out
