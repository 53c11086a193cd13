"""The yardstick of tests/test_hip_decoders.py (tests/_decoders_ref.py) is right and sharp -- on the CPU.

* right: it agrees with torch autograd in fp64 on the port's own formulas (oracle.torch_port.explicit_sigma / explicit_rgb / _TruncExp),
  and an fp32 numpy evaluation in the kernel's order stays inside every bound / reproduces the exact fixtures bit for bit;
* sharp: each planted fault of ``_decoders_ref.eval32`` leaves a bound or breaks exact equality on the shapes the GPU test runs.
"""
import numpy as np
import pytest
import torch

import _decoders_ref as dr
from oracle import torch_port as tp


def _eval(fx, accumulate=False, fault=None):
    got = dr.eval32(fx, accumulate, True, fault)
    if accumulate:
        got["grad_f_acc"] = got.pop("grad_f")
    return got


def _worst(fx, accumulate=False, fault=None):
    ref = dr.reference(fx.f, fx.basis, fx.act, fx.grad_out, fx.prefill)
    return dr.ratios(_eval(fx, accumulate, fault), ref), ref


# ------------------------------------------------------------------------------------------------ the case list itself
def test_case_list_covers_every_axis_value_where_the_issue_wants_it():
    cs = dr.cases()
    for n in dr.SECOND_TRIP:
        assert dr.n_waves(n) == 8192 and n > 8192
        sub = [c for c in cs if c[0] == n]
        assert {c[1] for c in sub} == set(dr.C_VALUES) and {c[2] for c in sub} == set(dr.K_VALUES) and {c[3] for c in sub} == set(dr.ACTS)
    k4 = [c for c in cs if c[2] == 4]
    assert {c[0] for c in k4} == set(dr.N_VALUES) and {c[1] for c in k4} == set(dr.C_VALUES) and {c[3] for c in k4} == set(dr.ACTS)
    for (C, K, act) in dr.REAL:
        assert {c[0] for c in cs if c[1:] == (C, K, act)} == set(dr.N_VALUES)
    assert dr.n_waves(8192) == 8192 and dr.n_waves(8191) == 8192 and dr.n_waves(5) == 8 and dr.n_waves(1) == 4
    trips = np.bincount(np.arange(20001) % dr.n_waves(20001))
    assert set(trips.tolist()) == {2, 3}                                       # 20001: waves of two and of three trips


# ------------------------------------------------------------------------------------------------ right: torch autograd, fp64
def _as64(a):
    return torch.as_tensor(np.asarray(a, np.float64))


@pytest.mark.parametrize("C,K,act", dr.REAL)
def test_reference_agrees_with_torch_autograd_on_the_ports_formula(C, K, act, monkeypatch):
    """explicit_sigma / explicit_rgb evaluated by autograd in fp64, with the stage in front of the product (the Linear / the basis MLP)
    replaced by a leaf that holds this fixture's basis: what is differentiated is the port's own product, shift and activation"""
    fx = dr.general_fixture(257, C, K, act, seed=5)
    f = _as64(fx.f).requires_grad_(True)
    b = _as64(fx.basis).requires_grad_(True)
    if act == "exp_m1":
        monkeypatch.setattr(tp.torch.nn.functional, "linear", lambda x, w, bias=None: b[:, 0, :])
        out = tp.explicit_sigma({"net.weight": None, "net.bias": None}, f)
    else:
        monkeypatch.setattr(tp, "mlp", lambda sd, prefix, x: b.reshape(b.size(0), -1))
        out = tp.explicit_rgb({"pe.freqs": _as64(dr.default_freqs(8))}, f, _as64(np.ones((257, 3))))
    monkeypatch.undo()
    out.backward(_as64(fx.grad_out))
    ref = dr.reference(fx.f, fx.basis, act, fx.grad_out)
    np.testing.assert_allclose(out.detach().numpy(), ref["out"], rtol=1e-13, atol=0)
    np.testing.assert_allclose(f.grad.numpy(), ref["grad_f"], rtol=0, atol=1e-13 * np.abs(ref["grad_f"]).max())
    np.testing.assert_allclose(b.grad.numpy(), ref["grad_basis"], rtol=0, atol=1e-13 * np.abs(ref["grad_basis"]).max())


def test_reference_agrees_with_the_ports_truncated_exponential():
    """_TruncExp on both sides of and at the clamp: forward exp(x), backward g exp(clamp(x, -15, 15)) -- TN_ACT_EXP with C = K = 1, f = 1"""
    x = np.array([-40.0, -15.5, -15.0, -3.0, 0.0, 2.5, 15.0, 15.5, 20.0, 30.0], np.float32)
    g = np.linspace(0.5, 2.0, x.size).astype(np.float32)
    xt = _as64(x).requires_grad_(True)
    y = tp._TruncExp.apply(xt)
    y.backward(_as64(g))
    ref = dr.reference(np.ones((x.size, 1), np.float32), x.reshape(-1, 1, 1), "exp", g.reshape(-1, 1))
    np.testing.assert_allclose(y.detach().numpy(), ref["out"][:, 0], rtol=1e-15)
    np.testing.assert_allclose(xt.grad.numpy(), ref["grad_basis"][:, 0, 0], rtol=1e-15)
    for act, at in (("exp_m1", "acc-1"), ("exp", "acc-1"), ("exp", "acc")):              # the clamp fixture sits exactly where it says
        fx = dr.clamp_fixture(act, at)
        r = dr.reference(fx.f, fx.basis, act, fx.grad_out)
        t = r["v"][:, 0] - (1.0 if act == "exp_m1" else 0.0)
        want = np.repeat(dr.CLAMP_TARGETS, 4) + (1.0 if (act, at) == ("exp", "acc-1") else 0.0)
        assert np.array_equal(t, want)
        xt = _as64(t).requires_grad_(True)
        tp._TruncExp.apply(xt).backward(_as64(fx.grad_out[:, 0]))
        np.testing.assert_allclose(r["gv"][:, 0], xt.grad.numpy(), rtol=1e-15)


# ------------------------------------------------------------------------------------------------ right: fp32 in the kernel's order
SMALL = [c for c in dr.cases() if c[0] <= 5] + [(8193, 8, 4, "exp_m1"), (8193, 96, 1, "exp_m1"), (8193, 96, 3, "sigmoid"), (20001, 8, 3, "exp")]


@pytest.mark.parametrize("n,C,K,act", SMALL)
def test_fp32_evaluation_in_kernel_order_stays_inside_every_bound(n, C, K, act):
    fx = dr.general_fixture(n, C, K, act, dr.case_seed(n, C, K))
    for accumulate in (False, True):
        worst, ref = _worst(fx, accumulate)
        assert np.abs(ref["v"]).max() < 16.0
        assert max(worst.values()) <= 1.0, (accumulate, worst)
    assert np.array_equal(dr.eval32(fx, want_basis=False)["grad_f"], dr.eval32(fx)["grad_f"])


@pytest.mark.parametrize("act,at", [("exp_m1", "acc-1"), ("exp", "acc-1"), ("exp", "acc")])
def test_fp32_evaluation_stays_inside_the_bounds_on_the_clamp_rows(act, at):
    fx = dr.clamp_fixture(act, at)
    for accumulate in (False, True):
        worst, _ = _worst(fx, accumulate)
        assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("n,C,K", sorted({c[:3] for c in SMALL}))
def test_exact_fixtures_are_exact_in_any_order(n, C, K):
    """the proof (assert_exact: integers, sums of |terms| below 2^24), then the kernel-order fp32 evaluation and a reversed-order one
    reproduce the fp64 values bit for bit"""
    fx = dr.exact_fixture(n, C, K, dr.case_seed(n, C, K))
    ref = dr.reference(fx.f, fx.basis, "none", fx.grad_out, fx.prefill)
    dr.assert_exact(ref["out"], ref["A_out"], "out")
    dr.assert_exact(ref["grad_basis"], np.abs(ref["grad_basis"]), "grad_basis")
    dr.assert_exact(ref["grad_f"], ref["A_grad_f"], "grad_f")
    dr.assert_exact(ref["grad_f_acc"], ref["A_grad_f_acc"], "grad_f_acc")
    for accumulate in (False, True):
        for k, a in _eval(fx, accumulate).items():
            assert np.array_equal(a.astype(np.float64), ref[k]), k
    rev = dr.Fixture(fx.f[:, ::-1].copy(), fx.basis[:, ::-1, ::-1].copy(), fx.grad_out[:, ::-1].copy(), fx.prefill[:, ::-1].copy(), "none")
    got, ref = dr.eval32(rev), dr.reference(fx.f, fx.basis, "none", fx.grad_out)
    assert np.array_equal(got["out"][:, ::-1].astype(np.float64), ref["out"])
    assert np.array_equal(got["grad_f"][:, ::-1].astype(np.float64), ref["grad_f"])


# ------------------------------------------------------------------------------------------------ sharp: planted faults
FAULTS = {            # fault -> the (n, C, K, act) of the GPU list on which it must show, on the general AND on the exact fixture
    "drop_ge64": [(1, 65, 4, "exp"), (3, 200, 4, "sigmoid"), (5, 129, 4, "exp_m1"), (5, 96, 1, "exp_m1"), (5, 96, 3, "sigmoid")],
    "drop_tail": [(1, 65, 4, "exp"), (3, 200, 4, "sigmoid"), (5, 129, 4, "exp_m1"), (5, 96, 3, "sigmoid")],
    "stride_c1": [(3, 200, 4, "sigmoid"), (4, 24, 4, "none"), (5, 96, 3, "sigmoid")],
    "no_accum": [(5, 129, 4, "exp_m1"), (1, 96, 1, "exp_m1"), (4, 24, 4, "none")],
    "wrap_8192": [(8193, 8, 4, "exp_m1"), (8193, 96, 1, "exp_m1"), (20001, 8, 3, "exp")],
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_planted_fault_leaves_a_bound_and_breaks_exactness(fault):
    listed = set(dr.cases())
    for (n, C, K, act) in FAULTS[fault]:
        assert (n, C, K, act) in listed
        accumulate = fault in ("no_accum", "wrap_8192")
        fx = dr.general_fixture(n, C, K, act, dr.case_seed(n, C, K))
        clean, _ = _worst(fx, accumulate)
        bad, _ = _worst(fx, accumulate, fault)
        assert max(clean.values()) <= 1.0 and max(bad.values()) > 1.0, (fault, n, C, K, act, clean, bad)
        ex = dr.exact_fixture(n, C, K, dr.case_seed(n, C, K))
        ref = dr.reference(ex.f, ex.basis, "none", ex.grad_out, ex.prefill)
        good, wrong = _eval(ex, accumulate), _eval(ex, accumulate, fault)
        assert all(np.array_equal(good[k].astype(np.float64), ref[k]) for k in good)
        assert any(not np.array_equal(wrong[k].astype(np.float64), ref[k]) for k in wrong), (fault, n, C, K)
    if fault == "wrap_8192":                 # without accumulate_f the wrapped rows are recomputed to the same values: the fault is the
        fx = dr.exact_fixture(8193, 8, 4, 1)  # ONE row past 8192 that is never written -- the exact fixture still sees it
        ref = dr.reference(fx.f, fx.basis, "none", fx.grad_out)
        wrong = dr.eval32(fx, False, True, fault)
        assert not np.array_equal(wrong["grad_basis"].astype(np.float64), ref["grad_basis"])


@pytest.mark.parametrize("act,at", [("exp_m1", "acc-1"), ("exp", "acc-1"), ("exp", "acc")])
def test_omitted_clamp_leaves_the_bound_on_the_clamp_rows(act, at):
    fx = dr.clamp_fixture(act, at)
    bad, ref = _worst(fx, False, "no_clamp")
    assert bad["out"] <= 1.0 and bad["grad_f"] > 1.0 and bad["grad_basis"] > 1.0, bad
    t = ref["v"][:, 0] - (1.0 if act == "exp_m1" else 0.0)
    got = dr.eval32(fx, False, True, "no_clamp")["grad_basis"].astype(np.float64)
    outside = np.abs(got - ref["grad_basis"]) > ref["E_grad_basis"]
    assert np.array_equal(outside.any(axis=(1, 2)), np.abs(t) > 15.0)             # every row beyond +-15 sees it, no row inside or AT it


# ------------------------------------------------------------------------------------------------ encoders and ray tables
@pytest.mark.parametrize("C,F", [(1, 1), (3, 4), (5, 10), (3, 10)])
def test_posenc_definition_agrees_with_the_port_and_sees_column_faults(C, F):
    fr = dr.default_freqs(F)
    x, n_special = dr.posenc_x(257, C, 3)
    assert n_special == 5
    for freqs in (fr, None):
        ref, E = dr.posenc(x, freqs, F)
        assert ref.shape == (257, 2 * F * C) and np.all(E == dr.E_SINCOS)
        assert np.all(np.abs(dr.posenc32(x, freqs, F).astype(np.float64) - ref) <= E)
        zero = ref[257 - 5].reshape(C, 2, F)                                     # x = 0: sin = 0, cos = 1 exactly, at c 2F + f / c 2F + F + f
        assert np.all(zero[:, 0] == 0.0) and np.all(zero[:, 1] == 1.0)
        for fault in ("swap",) + (("freq_index",) if F > 1 else ()):
            assert np.any(np.abs(dr.posenc32(x, freqs, F, fault).astype(np.float64) - ref) > E), fault
    assert np.array_equal(dr.freqs_or_default(None, F), fr)                      # 2^j pi rounded once == ldexp(float32(pi), j)
    # torch_port.posenc in fp64 on inputs whose fp32 product is exact (x a power of two): the same numbers, the same column order
    xp = (2.0 ** -np.random.default_rng(1).integers(0, 6, (33, C)) * np.random.default_rng(2).choice([-1.0, 1.0], (33, C))).astype(np.float32)
    port = tp.posenc(_as64(xp), _as64(fr)).numpy()
    np.testing.assert_allclose(dr.posenc(xp, fr, F)[0], port, rtol=0, atol=1e-15)


def test_dir_encode_and_ray_aux_definitions():
    d = np.random.default_rng(0).standard_normal((65, 3)).astype(np.float32)
    tab, E = dr.dir_encode(d, None, 4, 28)
    assert np.array_equal(tab[:, :24], dr.posenc(d, None, 4)[0]) and np.array_equal(tab[:, 24:27], d.astype(np.float64))
    assert np.all(tab[:, 27:] == 0) and np.all(E[:, 24:] == 0) and np.all(E[:, :24] == dr.E_SINCOS)
    cnt = np.array([0, 1, 63, 0, 0, 64, 65, 300, 0], np.int32)
    info = np.stack([np.cumsum(cnt) - cnt, cnt], -1).astype(np.int32)
    packed = np.random.default_rng(1).random((int(cnt.sum()), 7)).astype(np.float32)
    ids, steps, dirs = dr.ray_aux(packed, info)
    assert np.array_equal(ids, np.repeat(np.arange(cnt.size), cnt)) and np.array_equal(steps, packed[:, 6])
    assert np.all(dirs[cnt == 0] == 0) and np.array_equal(dirs[7], packed[info[7, 0], 3:6])
