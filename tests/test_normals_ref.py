"""CPU checks of the surface-normal yardstick (tests/_normals_ref.py), without the kernel: its gradient equals central differences of
its own y(x), its contraction Jacobian equals central differences of the reference's contraction (src/core.py:18-19) for both norms,
two analytic cases with a known normal come out as they must, and the cases of tests/test_hip_normals.py stay under the 1 % cap on
skipped rows -- a property of the inputs alone, so it is settled here."""
import numpy as np
import pytest

import _hashgrid_ref as hg
import _normals_ref as ref
import _normals_cases as cases


def _central(fun, x, h):
    g = np.zeros_like(x)
    for a in range(3):
        e = np.zeros(3)
        e[a] = h
        g[:, a] = (fun(x + e) - fun(x - e)) / (2 * h)
    return g


def _away_from_faces(pos, margin):
    """every coordinate of `pos` (in cells) at least `margin` of a cell from a face"""
    fr = pos - np.floor(pos)
    return ((fr > margin) & (fr < 1 - margin)).all(-1)


def test_kplanes_gradient_equals_central_differences():
    rng = np.random.default_rng(1)
    sizes = [(6, 11), (9, 9)]
    planes = ref.make_planes(2, 8, sizes, 2)
    W1, b1, w2, b2 = ref.make_head(16, 3)
    x = rng.uniform(-0.98, 0.98, (4000, 3))
    h = 1e-6

    def y(xx):
        return ref.y_of(W1, b1, w2, b2, ref.kplanes_features(planes, xx, fp32_pos=False)[0])

    keep = np.ones(len(x), bool)
    for (H, W) in sizes:
        for p, (ua, va) in enumerate(ref.PAIRS):
            keep &= _away_from_faces(np.stack([(x[:, ua] + 1) * 0.5 * (W - 1), (x[:, va] + 1) * 0.5 * (H - 1)], 1), 1e-3)
    f, df, _, dfa = ref.kplanes_features(planes, x, fp32_pos=False)
    grad, A, _ = ref.gradient(W1, b1, w2, f, df, dfa)
    hid = ref.head(W1, b1, w2, f)[3]
    keep &= (np.abs(hid) > 1e-3).all(1)                       # no ReLU changes sides within the stencil
    assert keep.sum() > 1000
    fd = _central(y, x, h)
    assert np.abs(fd - grad)[keep].max() <= 1e-7 * np.abs(grad)[keep].max()
    assert (np.abs(grad) <= A * (1 + 1e-12)).all()


def test_hashgrid_gradient_equals_central_differences():
    rng = np.random.default_rng(4)
    plan = hg.levels(**hg.SMALL)
    table = rng.uniform(-1, 1, (hg.total_entries(plan), 2)).astype(np.float32)
    W1, b1, w2, b2 = ref.make_head(8, 5)
    x = rng.uniform(-0.98, 0.98, (4000, 3))

    def y(xx):
        return ref.y_of(W1, b1, w2, b2, ref.hashgrid_features(table, xx, plan, fp32_pos=False)[0])

    keep = np.ones(len(x), bool)
    for N in plan[0]:
        keep &= _away_from_faces((x + 1) * 0.5 * N, 1e-3)
    f, df, _, dfa = ref.hashgrid_features(table, x, plan, fp32_pos=False)
    grad, A, _ = ref.gradient(W1, b1, w2, f, df, dfa)
    keep &= (np.abs(ref.head(W1, b1, w2, f)[3]) > 1e-3).all(1)
    assert keep.sum() > 1000
    fd = _central(y, x, 1e-6)
    assert np.abs(fd - grad)[keep].max() <= 1e-7 * np.abs(grad)[keep].max()
    assert (np.abs(grad) <= A * (1 + 1e-12)).all()


def test_hashgrid_gradient_is_zero_where_the_clamp_acts():
    plan = hg.levels(**hg.SMALL)
    table = np.random.default_rng(0).uniform(-1, 1, (hg.total_entries(plan), 2)).astype(np.float32)
    x = np.array([[1.5, 0.2, -0.3], [0.1, -1.0000001, 0.4], [np.nan, 0.5, 0.5], [0.3, 0.3, 1e30]], np.float32)
    _, df, _, _ = ref.hashgrid_features(table, x, plan)
    for row, axis in enumerate((0, 1, 0, 2)):
        assert (df[axis][row] == 0).all() and (df[(axis + 1) % 3][row] != 0).any()


@pytest.mark.parametrize("kind,order", [(ref.MIP_INF, np.inf), (ref.MIP_L2, 2.0)])
def test_jacobian_equals_central_differences_of_the_reference_contraction(kind, order):
    rng = np.random.default_rng(7)
    X = np.concatenate([rng.uniform(-1, 1, (500, 3)), rng.standard_normal((1500, 3)) * 3, rng.standard_normal((500, 3)) * 40])
    m = np.abs(X).max(1) if np.isinf(order) else np.sqrt((X * X).sum(1))
    keep = np.abs(m - 1) > 1e-3
    if np.isinf(order):
        a = np.sort(np.abs(X), 1)
        keep &= (a[:, 2] - a[:, 1]) > 1e-3 * a[:, 2]           # no argmax tie within the stencil
    X, m = X[keep], m[keep]
    assert (m < 1).sum() > 50 and (m > 1).sum() > 500
    J = ref.jacobian(kind, ref.contract(X, order), fp32_x=False)
    fd = np.zeros_like(J)
    for j in range(3):
        h = 1e-6 * np.maximum(1.0, m)
        e = np.zeros((len(X), 3))
        e[:, j] = h
        fd[:, :, j] = (ref.contract(X + e, order) - ref.contract(X - e, order)) / (2 * h)[:, None]
    assert np.abs(J - fd).max() <= 1e-8
    rel = np.abs(J - fd).reshape(len(X), -1).max(1) / np.abs(J).reshape(len(X), -1).max(1)
    assert rel.max() <= 1e-6


def test_jacobian_edges():
    x = np.array([[0.1, 0.2, 0.3], [1.0, 0.0, 0.0], [1.2, 0.1, 0.1], [np.nan, 0, 0], [np.inf, 0, 0], [0.5, -0.5, 0.5]], np.float32)
    for kind in (ref.MIP_INF, ref.MIP_L2):
        J = ref.jacobian(kind, x)
        assert np.array_equal(J[0], 0.5 * np.eye(3))
        for row in (1, 2, 3, 4):                               # s >= 2 or not finite: v = 0
            assert (J[row] == 0).all()
    assert np.array_equal(ref.jacobian(ref.MIP_INF, x)[5], 0.5 * np.eye(3))      # s = 1 exactly: inside
    J = ref.jacobian(ref.AABB, x[:1], aabb=[-1, -2, -4, 1, 2, 4])
    assert np.array_equal(J[0], np.diag([1.0, 0.5, 0.25]))
    assert np.array_equal(ref.jacobian(ref.NONE, x[:1])[0], np.eye(3))


# ------------------------------------------------------------------------------------------------- analytic cases, no yardstick needed
def test_linear_hashgrid_has_a_constant_normal():
    a = np.array([0.3, -1.1, 0.7])
    plan, table = ref.linear_hashgrid(6, 2, a, 0)
    W1, b1, w2, _ = ref.make_head(2, 1, positive=True)
    x = np.random.default_rng(2).uniform(-0.999, 0.999, (500, 3)).astype(np.float32)
    grad, A, tie = ref.hashgrid_gradient(table, x, plan, W1, b1, w2)
    assert not tie.any()
    nrm, _, _, ok = ref.normals(ref.NONE, x, grad, ref.grad_bound(A, 2))
    assert ok.all() and np.abs(nrm + a / np.linalg.norm(a)).max() < 1e-5          # (the fp32 table rounds the linear function)


@pytest.mark.parametrize("aabb", [None, [-1.0, -3.0, -0.5, 2.0, 1.0, 4.0]])
def test_planes_that_vary_along_x0_give_e0(aabb):
    sizes = [(5, 7), (9, 4)]
    planes = ref.x0_planes(2, 4, sizes, 3)
    W1, b1, w2, _ = ref.make_head(8, 4, positive=True)
    x = np.random.default_rng(5).uniform(-0.999, 0.999, (500, 3)).astype(np.float32)
    grad, A, tie = ref.kplanes_gradient(planes, x, W1, b1, w2)
    assert not tie.any() and (grad[:, 0] > 0).all() and np.abs(grad[:, 1:]).max() <= 1e-12 * np.abs(grad[:, 0]).max()
    nrm, _, _, ok = ref.normals(ref.NONE if aabb is None else ref.AABB, x, grad, ref.grad_bound(A, 8), aabb)
    assert ok.all() and np.abs(nrm - np.array([-1.0, 0, 0])).max() < 1e-12


# ------------------------------------------------------------------------------------------------------ the GPU tests' cases, on the CPU
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_gpu_cases_stay_under_the_cap_on_skipped_rows(name):
    """at most 1 % of the finite rows of a case may be skipped for a ReLU tie, and at most 1 % of them may have a normal bound above
    1e-2 in any frame: the yardstick depends on the inputs only, so the seeds are held to it here"""
    for n in cases.NS:
        c = cases.reference(name, n)
        finite = c["finite"]
        if finite.sum() == 0:
            continue
        cap = int(0.01 * finite.sum())
        assert (c["tie"] & finite).sum() <= cap, (name, n, int((c["tie"] & finite).sum()), int(finite.sum()))
        for kind in cases.FRAMES:
            loose = c["normals"][kind]["loose"] & finite & ~c["tie"]
            assert loose.sum() <= cap, (name, n, kind, int(loose.sum()))
