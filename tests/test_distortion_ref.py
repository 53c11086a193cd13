"""CPU checks of the distortion loss' fp64 yardstick (tests/_distortion_ref.py), which the GPU tests hold the kernels against: hand
answers, torch's autograd on the same expression, shift invariance, and g as the inverse of the unbounded marcher's table."""
import numpy as np
import pytest
import torch

import _distortion_ref as ref


def test_one_sample_is_the_width_term():
    loss, grad = ref.ray_loss_and_grad([0.7], [3.0], [0.25])
    assert loss == pytest.approx(0.7 ** 2 * 0.25 / 3.0, rel=1e-15)
    assert grad[0] == pytest.approx(2.0 / 3.0 * 0.7 * 0.25, rel=1e-15)


def test_two_samples():
    w, m, d = [0.3, 0.5], [1.0, 1.4], [0.1, 0.2]
    loss, grad = ref.ray_loss_and_grad(w, m, d)
    assert loss == pytest.approx(2 * 0.3 * 0.5 * 0.4 + (0.09 * 0.1 + 0.25 * 0.2) / 3.0, rel=1e-14)
    np.testing.assert_allclose(grad, [2 * 0.5 * 0.4 + 2.0 / 3.0 * 0.3 * 0.1, 2 * 0.3 * 0.4 + 2.0 / 3.0 * 0.5 * 0.2], rtol=1e-14)


@pytest.mark.parametrize("n", [2, 7, 64])
def test_equal_weights_on_an_equispaced_ray(n):
    """w = 1 / n on n cells of width h: sum_ij |i - j| = n (n^2 - 1) / 3, so L = h (n^2 - 1) / (3 n) + h / (3 n) = n h / 3 -- a third of
    the span, the value of the continuous uniform distribution"""
    h = 0.125
    loss, _ = ref.ray_loss_and_grad(np.full(n, 1.0 / n), h * np.arange(n), np.full(n, h))
    assert loss == pytest.approx(n * h / 3.0, rel=1e-13)


def test_a_ray_without_samples_and_zero_weights():
    assert ref.ray_loss_and_grad([], [], [])[0] == 0.0
    loss, grad = ref.ray_loss_and_grad(np.zeros(5), np.arange(5.0), np.ones(5))
    assert loss == 0.0 and not grad.any()


@pytest.mark.parametrize("warp,near,rng", [(ref.LINEAR, 0.0, 5.2), (ref.UNBOUNDED, 0.1, 1.0), (ref.UNBOUNDED, 0.1, 4.0)])
def test_analytic_gradient_against_autograd(warp, near, rng):
    r = np.random.default_rng(warp + int(rng))
    n = 23
    step = np.full(n, 0.04)
    t = 0.3 + np.cumsum(step) + 0.04 * r.uniform(0, 1, n) * 0.5           # crosses x = 1 under (UNBOUNDED, 0.1, 1)
    w = r.uniform(0, 0.1, n)
    m, d = ref.warp_md(t, step, warp, near, rng)
    mt, dt = torch.from_numpy(m), torch.from_numpy(d)

    def expr(wt):
        return (wt[:, None] * wt[None, :] * (mt[:, None] - mt[None, :]).abs()).sum() + (wt * wt * dt).sum() / 3.0
    wt = torch.from_numpy(w).requires_grad_(True)
    assert torch.autograd.gradcheck(expr, (wt,), eps=1e-7, atol=1e-7)
    loss, grad = ref.distortion(w, t, step, np.array([[0, n]]), warp, near, rng)
    val = expr(wt)
    val.backward()
    assert loss[0] == pytest.approx(float(val.detach()), rel=1e-13)
    np.testing.assert_allclose(grad, wt.grad.numpy(), rtol=1e-12, atol=1e-16)


def test_packed_rays_and_unowned_samples():
    """two rays and a gap between them: per-ray values, the gap's gradient stays 0"""
    r = np.random.default_rng(5)
    w, t, s = r.uniform(0, 1, 12), np.sort(r.uniform(2, 6, 12)), np.full(12, 0.1)
    info = np.array([[0, 5], [7, 5], [12, 0]])
    loss, grad = ref.distortion(w, t, s, info, ref.LINEAR, 0.0, 2.0)
    for k, (a, c) in enumerate(info[:2]):
        lk, gk = ref.ray_loss_and_grad(w[a:a + c], t[a:a + c] / 2.0, s[a:a + c] / 2.0)
        assert loss[k] == pytest.approx(lk, rel=1e-14)
        np.testing.assert_allclose(grad[a:a + c], gk, rtol=1e-14)
    assert loss[2] == 0.0 and not grad[5:7].any()


def test_shift_invariance():
    r = np.random.default_rng(7)
    w, m, d = r.uniform(0, 1, 40), np.sort(r.uniform(0, 1, 40)), r.uniform(0, 0.1, 40)
    l0, g0 = ref.ray_loss_and_grad(w, m, d)
    l1, g1 = ref.ray_loss_and_grad(w, m + 37.5, d)
    assert l1 == pytest.approx(l0, rel=1e-12)
    np.testing.assert_allclose(g1, g0, rtol=1e-11)
    # LINEAR: a shift of t is a shift of m
    info = np.array([[0, 40]])
    la, _ = ref.distortion(w, m * 4, d, info, ref.LINEAR, 0.0, 4.0)
    lb, _ = ref.distortion(w, m * 4 + 50.0, d, info, ref.LINEAR, 0.0, 4.0)
    assert lb[0] == pytest.approx(la[0], rel=1e-11)


@pytest.mark.parametrize("S", [200, 1024])
def test_g_inverts_the_unbounded_marchers_table(S):
    """the marcher's samples are f(u) * uniform_range + near for u uniform in [0, 1 - 1 / (S + 2)] (core.py:52): g(f(u)) == u, and
    g of the marcher's own fp32 table gives u back to fp32 rounding"""
    u = np.linspace(0.0, 1.0 - 1.0 / (S + 2), S + 1)
    np.testing.assert_allclose(ref.g(ref.f(u)), u, rtol=0, atol=2e-16)
    np.testing.assert_allclose(ref.g_prime(ref.f(u)) * np.where(u < 0.5, 2.0, 2.0 * ref.f(u) ** 2), 1.0, rtol=1e-12)   # g'(f(u)) f'(u) == 1
    from tinynerf_amd.core import RayMarcherUnbounded, distortion_warp
    for near, scale in ((0.0, 1.0), (0.1, 4.0)):
        marcher = RayMarcherUnbounded(S, near, 1e5, uniform_range=scale)
        t, delta = marcher._table(torch.device("cpu"))
        warp, w_near, w_range = distortion_warp(marcher)
        assert (warp, w_near, w_range) == (ref.UNBOUNDED, near, scale)
        m, d = ref.warp_md(t.numpy(), delta.numpy(), warp, w_near, w_range)
        # fp32 t behind the knee: d u = d t / (2 x^2 range) -- an ulp of t = x range moves u by 2^-24 / x at most
        np.testing.assert_allclose(m, u[:-1], rtol=0, atol=3e-7)
        assert np.all(np.diff(m) > 0)
        # the widths are the table's own cells in u, 1 / (S + 2 ...) each, up to the curvature inside a cell
        np.testing.assert_allclose(d[: S // 2 - 1], np.diff(u)[: S // 2 - 1], rtol=2e-4)


def test_the_aabb_marchers_warp_is_the_box_diagonal():
    from tinynerf_amd.core import RayMarcherAABB, distortion_warp
    aabb = torch.tensor([[-1.5, -1.5, -1.5], [1.5, 1.5, 1.5]])
    warp, near, rng = distortion_warp(RayMarcherAABB(aabb, 1024, 0.1))
    assert warp == ref.LINEAR and near == 0.0
    assert rng == pytest.approx(3.0 * 3.0 ** 0.5, rel=1e-6)
