"""CPU checks of the float64 yardstick tests/_optim_ref.py: its Adam is torch.optim.Adam in float64, its regulariser is float64
autograd of the reference formulas (mse_loss of the shifted views, abs().mean(): models.py:115-121), and its row-restricted results
partition the unrestricted ones.  Also here, because it needs no GPU: tn_adam_reg_multi refuses a bad row range, shape or output
buffer with its documented code before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import _optim_ref as ref

TN_E_NULL, TN_E_SIZE, TN_E_CONFIG, TN_E_ALIGN = -1, -2, -3, -4
HP = dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-15, wd=1e-5)              # reference run.py:186


def test_adam_is_torch_adam_in_float64_over_five_steps():
    rng = np.random.default_rng(0)
    n = 1003
    p0 = rng.uniform(-1, 1, n).astype(np.float32)
    param = torch.nn.Parameter(torch.from_numpy(p0.astype(np.float64)))
    opt = torch.optim.Adam([param], lr=HP["lr"], betas=(HP["b1"], HP["b2"]), eps=HP["eps"], weight_decay=HP["wd"])
    p, m, v = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    for step in range(1, 6):
        g = (rng.standard_normal(n) * 1024).astype(np.float32)
        g[::7] = 0.0
        param.grad = torch.from_numpy(g.astype(np.float64))
        opt.step()
        p, m, v = ref.adam(p, g, m, v, step, **HP)
        st = opt.state[param]
        np.testing.assert_allclose(p, param.detach().numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(m, st["exp_avg"].numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(v, st["exp_avg_sq"].numpy(), rtol=1e-12, atol=0)
    assert np.abs(p - p0).max() > 1e-2                                   # (five updates of about lr each)


def make_plane(H, W, C, seed):
    rng = np.random.default_rng(seed)
    plane = rng.uniform(-1, 1, (H, W, C)).astype(np.float32)
    flat = plane.reshape(-1)
    flat[::5] = 0.0
    flat[2::11] = -0.0
    return plane


@pytest.mark.parametrize("shape", [(5, 7, 8), (33, 17, 32)])
def test_plane_reg_is_float64_autograd_of_the_reference_formulas(shape):
    H, W, C = shape
    plane = make_plane(H, W, C, 3)
    w_tv, w_l1, upstream = 0.7, 0.3, 1024.0
    p = torch.from_numpy(plane.astype(np.float64)).permute(2, 0, 1)[None].clone().requires_grad_(True)       # [1, C, H, W]
    mse_y = torch.nn.functional.mse_loss(p[:, :, 1:, :], p[:, :, :-1, :])
    mse_x = torch.nn.functional.mse_loss(p[:, :, :, 1:], p[:, :, :, :-1])
    l1 = p.abs().mean()
    (upstream * (w_tv * (mse_y + mse_x) + w_l1 * l1)).backward()
    cy, cx, cl1 = w_tv / (C * (H - 1) * W), w_tv / (C * H * (W - 1)), w_l1 / (C * H * W)
    sums, grad = ref.plane_reg(plane, cy, cx, cl1, upstream)
    want = np.array([mse_y.item() * C * (H - 1) * W, mse_x.item() * C * H * (W - 1), l1.item() * C * H * W])
    np.testing.assert_allclose(sums, want, rtol=1e-12, atol=0)
    want_grad = p.grad[0].permute(1, 2, 0).numpy()
    assert np.abs(grad - want_grad).max() <= 1e-12 * np.abs(want_grad).max()
    zero = plane == 0
    assert zero.sum() > 10 and np.signbit(plane[zero]).any() and not np.signbit(plane[zero]).all()
    _, only_l1 = ref.plane_reg(plane, 0.0, 0.0, 1.0, 1.0)
    assert np.all(only_l1[zero] == 0.0) and set(np.unique(only_l1)) == {-1.0, 0.0, 1.0}


def partitions(H, rng):
    yield [(0, H)]
    yield [(0, 1), (1, H)]
    yield [(0, H - 1), (H - 1, H)]
    yield [(y, y + 1) for y in range(H)]
    for _ in range(5):
        cuts = sorted(set(rng.integers(1, H, 3).tolist()))
        edges = [0] + cuts + [H]
        yield list(zip(edges[:-1], edges[1:]))


@pytest.mark.parametrize("shape", [(13, 6, 8), (2, 2, 4), (9, 1, 4), (33, 17, 32)])
def test_row_restricted_results_partition_the_unrestricted_ones(shape):
    H, W, C = shape
    plane = make_plane(H, W, C, 5)
    args = (3e-3, 2e-3, 1e-3, 1024.0)
    sums, grad = ref.plane_reg(plane, *args)
    mag = ref.plane_reg_magnitude(plane, *args)
    assert np.all(np.abs(grad) <= mag * (1 + 1e-12))
    for part in partitions(H, np.random.default_rng(H)):
        pieces = [ref.plane_reg(plane, *args, rows=r) for r in part]
        np.testing.assert_allclose(sum(s for s, _ in pieces), sums, rtol=1e-12, atol=0)
        assert np.array_equal(np.concatenate([g for _, g in pieces], axis=0), grad)
        assert np.array_equal(np.concatenate([ref.plane_reg_magnitude(plane, *args, rows=r) for r in part], axis=0), mag)


def test_adam_reg_is_the_regulariser_gradient_followed_by_adam():
    H, W, C = 13, 6, 8
    rng = np.random.default_rng(8)
    plane = make_plane(H, W, C, 8)
    g, m = (rng.standard_normal((H, W, C)).astype(np.float32) for _ in range(2))
    v = rng.uniform(0, 1, (H, W, C)).astype(np.float32)
    reg = (3e-3, 2e-3, 1e-3, 1024.0)
    full = ref.adam_reg(plane, g, m, v, 3, *HP.values(), *reg)
    sums, rg = ref.plane_reg(plane, *reg)
    want = ref.adam(plane, g.astype(np.float64) + rg, m, v, 3, **HP)
    assert all(np.array_equal(a, b) for a, b in zip(full[:3], want)) and np.array_equal(full[3], sums)
    rows = (4, 9)
    part = ref.adam_reg(plane, g, m, v, 3, *HP.values(), *reg, rows=rows)
    assert all(np.array_equal(a, b[4:9]) for a, b in zip(part[:3], full[:3]))
    assert np.array_equal(part[3], ref.plane_reg(plane, *reg, rows=rows)[0])


# ---- tn_adam_reg_multi: what the host refuses, before any launch (dummy pointers, never dereferenced)

@pytest.fixture(scope="module")
def lib():
    from tinynerf_amd import build
    lib = ctypes.CDLL(build.build(verbose=False))
    lib.tn_last_error_string.restype = ctypes.c_char_p
    return lib


def reg_item(**kw):
    from tinynerf_amd import _lib as L
    it = (L.AdamRegItem * 1)()
    t = it[0]
    t.param, t.param_out, t.grad, t.exp_avg, t.exp_avg_sq = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    t.H, t.W, t.C, t.n = 13, 6, 8, 13 * 6 * 8
    for k, val in kw.items():
        setattr(t, k, val)
    return it


def reg_call(lib, items, sums=0x60000):
    f = ctypes.c_float
    return lib.tn_adam_reg_multi(items, ctypes.c_int32(1), f(1e-2), f(0.9), f(0.999), f(1e-15), f(1e-5), ctypes.c_int32(1), ctypes.c_int32(1),
                                 f(1024.0), ctypes.c_void_p(sums), None)


@pytest.mark.parametrize("kw,code", [
    (dict(row0=4, row1=4), TN_E_SIZE),                       # empty range
    (dict(row0=5, row1=4), TN_E_SIZE),
    (dict(row0=3, row1=0), TN_E_SIZE),                       # row1 == 0 means every row, and then row0 must be 0
    (dict(row0=-1, row1=4), TN_E_SIZE),
    (dict(row0=0, row1=14), TN_E_SIZE),                      # row1 > H
    (dict(H=0, W=0, C=0, row0=0, row1=4), TN_E_SIZE),        # a row range on a tensor without a plane shape
    (dict(param_out=0x10000), TN_E_CONFIG),                  # a regularised plane updated in place
    (dict(n=13 * 6 * 8 + 4), TN_E_SIZE),                     # H W C != n
    (dict(n=13 * 6 * 8 - 8, H=12), TN_E_SIZE),
    (dict(C=6, W=8), TN_E_SIZE),                             # C % 4 != 0 (H W C still equals n)
    (dict(W=0), TN_E_SIZE),
    (dict(sum_slot=-1), TN_E_SIZE),
    (dict(n=-1), TN_E_SIZE),
    (dict(grad=None), TN_E_NULL),
    (dict(param_out=None), TN_E_NULL),
    (dict(exp_avg=0x40008), TN_E_ALIGN),
])
def test_adam_reg_multi_refuses_before_any_launch(lib, kw, code):
    assert reg_call(lib, reg_item(**kw)) == code and lib.tn_last_error_string()
    assert lib.tn_adam_reg_multi(reg_item(), ctypes.c_int32(1), *[ctypes.c_float(0.1)] * 5, ctypes.c_int32(0), ctypes.c_int32(1),
                                 ctypes.c_float(1.0), None, None) == TN_E_SIZE                     # step < 1
    assert lib.tn_adam_reg_multi(None, ctypes.c_int32(1), *[ctypes.c_float(0.1)] * 5, ctypes.c_int32(1), ctypes.c_int32(1),
                                 ctypes.c_float(1.0), None, None) == TN_E_NULL


def test_adam_reg_multi_accepts_nothing_to_do(lib):
    """what the refusals above are measured against: the same item with n == 0, and an empty list, return 0 without a launch"""
    assert lib.tn_adam_reg_multi(None, ctypes.c_int32(0), *[ctypes.c_float(0.1)] * 5, ctypes.c_int32(1), ctypes.c_int32(1),
                                 ctypes.c_float(1.0), None, None) == 0
    assert reg_call(lib, reg_item(H=0, W=0, C=0, n=0)) == 0
