"""G23: the port-side yardstick of tests/test_hip_train_trace.py (oracle/make_trace_noise.py, tests/_trace_noise.py).  CPU only: the
golden is what its raw arrays say it is, the recipe still produces it, and the caps trip when they should."""
import importlib.util
import os

import numpy as np
import pytest

import _g22
import _trace_noise as tn
from conftest import ROOT, load_golden


@pytest.fixture(scope="module")
def g23():
    return load_golden("G23_trace_noise")


@pytest.fixture(scope="module")
def recipe():
    spec = importlib.util.spec_from_file_location("make_trace_noise", os.path.join(ROOT, "oracle", "make_trace_noise.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name", tn.TRACES)
def test_golden_is_what_its_raw_arrays_say(g23, name):
    g, d = _g22.trace(name), tn.load(name, g23)
    K, names, C = int(g["steps"]), [str(n) for n in g["param_names"]], len(g23["controls"])
    assert g23["controls"].tolist() == [1, 2, 3, 4, 5, 6] and float(g23["amplitude"]) == 2.0 ** -22
    assert [str(n) for n in d["param_names"]] == names
    assert d["loss"].shape == (C, K) and d["unperturbed_loss"].shape == (K,) and d["spread"].shape == (C, len(names))
    assert d["E6"].shape == d["cap_loss"].shape == (K,) and d["S6"].shape == d["cap_param"].shape == (len(names),)
    assert np.isfinite(d["loss"]).all() and np.isfinite(d["spread"]).all() and (d["spread"] >= 0).all()
    # (the unperturbed replay is one more fp32 evaluation: with another thread count than the record's it parts from it like a control)
    assert (np.maximum.accumulate(np.abs(d["unperturbed_loss"] / g["loss"] - 1)) <= np.maximum(1e-6, float(d["R"]) * d["E6"])).all()
    env = tn.control_envelopes(d["loss"], g["loss"])
    assert (np.diff(env, axis=1) >= 0).all() and (np.diff(d["E6"]) >= 0).all()
    assert d["E6"][:3].max() < 1e-3 / 8                  # the port's controls start together (test_hip_train_trace: tol[:3] < 1e-3, tol = 8 x envelope)
    again = tn.derive(d["loss"], d["spread"], g["loss"])
    for k, v in again.items():
        np.testing.assert_array_equal(v, d[k], err_msg=k)
    assert float(d["R"]) >= 1 and float(d["M"]) == 2 * float(d["R"]) and float(d["R_p"]) >= 1 and float(d["M_p"]) == 2 * float(d["R_p"])
    ahead = np.minimum(np.arange(K) + 1, K - 1)
    np.testing.assert_array_equal(d["cap_loss"], np.maximum(1e-5 / 8, float(d["M"]) * d["E6"][ahead]))
    np.testing.assert_array_equal(d["cap_param"], np.maximum(1e-5 / 8, float(d["M_p"]) * d["S6"]))
    print(name, "R", float(d["R"]), "M", float(d["M"]), "R_p", float(d["R_p"]), "M_p", float(d["M_p"]), "E6 end", d["E6"][-1], "S6 max", d["S6"].max())


def test_sampling_ratio_by_hand():
    """six controls, two columns: the split {0, 1, 2} | {3, 4, 5} gives 8 / 1 in column 0; column 1 never has both halves >= 1e-6"""
    a = np.array([[1e-5, 1e-9], [1e-5, 1e-9], [1e-5, 1e-9], [8e-5, 1e-3], [2e-5, 1e-9], [2e-5, 1e-9]])
    assert tn.sampling_ratio(a) == pytest.approx(8.0)
    assert tn.sampling_ratio(np.full((6, 4), 1e-9)) == 1.0
    assert tn.sampling_ratio(np.full((6, 4), 3e-4)) == 1.0


def test_recipe_still_produces_the_golden(g23, recipe):
    """one control of kplanes, seed 1, 3 steps through the recipe's own function"""
    losses, seen = recipe.replay("kplanes", 1, n_steps=3)
    np.testing.assert_allclose(losses, tn.load("kplanes", g23)["loss"][0, :3], rtol=1e-6)
    g = _g22.trace("kplanes")
    assert list(seen) == [str(n) for n in g["param_names"]]
    for n, a in seen.items():
        assert a.shape == (g["final/" + n] if "final/" + n in g else g["final_sub/" + n]).shape, n


def test_recipe_perturbs_by_the_rule_of_the_hip_controls(recipe):
    """every floating parameter but ``*freqs`` within 2^-23 relative (and an fp32 rounding) of the unperturbed one, not all equal to it"""
    from oracle import torch_port as tp
    base, moved = tp.initial_state("vanilla", 0), recipe.perturbed_state("vanilla", 0, 1)
    for k, v in base.items():
        if k.endswith("freqs"):
            assert (moved[k] == v).all()
            continue
        assert moved[k].dtype == v.dtype and moved[k].shape == v.shape
        rel = ((moved[k].double() - v.double()).abs() / v.double().abs().clamp_min(1e-300))[v != 0]
        assert float(rel.max()) <= 2.0 ** -23 + 2.0 ** -24 and float(rel.max()) > 0, k
    again = recipe.perturbed_state("vanilla", 0, 1)
    assert all((again[k] == moved[k]).all() for k in moved)
    other = recipe.perturbed_state("vanilla", 0, 2)
    assert any((other[k] != moved[k]).any() for k in moved)


def _synthetic(K=12, N=4):
    rng = np.random.default_rng(0)
    record = 0.1 + rng.random(K)
    growth = 1e-7 * 2.0 ** np.arange(K)                                  # controls part at a doubling rate
    loss = record[None, :] * (1 + growth[None, :] * rng.uniform(0.5, 1.0, (6, K)) * rng.choice([-1.0, 1.0], (6, K)))
    spread = rng.uniform(1e-5, 3e-5, (6, N))
    d = tn.derive(loss, spread, record)
    d["param_names"] = np.array([f"p{i}" for i in range(N)])
    return d


def _ahead(envelope):
    return np.append(envelope[1:], envelope[-1])


def test_cap_holds_an_envelope_like_the_ports():
    d = _synthetic()
    assert float(d["M"]) >= 2 and float(d["M_p"]) >= 2
    env = d["E6"].copy()                 # a three-control envelope EQUAL to the port's six-control one
    assert tn.check_loss_envelope("synthetic", _ahead(env), d)[0] == pytest.approx(1 / float(d["M"]))
    tn.check_param_spread("synthetic", dict(zip(d["param_names"].tolist(), d["S6"])), d["param_names"], d)
    tn.check_controls("synthetic", _ahead(env), dict(zip(d["param_names"].tolist(), d["S6"])), d["param_names"], d)


def test_cap_trips_on_one_late_step_and_names_it():
    d = _synthetic()
    K, M = d["E6"].shape[0], float(d["M"])
    env = d["E6"].copy()
    env[K - 1] = 4 * M * d["E6"][K - 1]                  # 4 M E6 at the last step alone
    with pytest.raises(AssertionError, match=rf"self-measured loss envelope.*at step {K - 2} the HIP controls. envelope \(read at step {K - 1}\).*steps over the cap: \[{K - 2}, {K - 1}\]"):
        tn.check_loss_envelope("synthetic", _ahead(env), d)          # (read one step ahead: the allowances of steps K-2 and K-1 hold it)
    env = d["E6"].copy()
    env[5:] = np.maximum(env[5:], 4 * M * d["E6"][5])                      # a jump at step 5 (cumulative, as a real envelope is)
    with pytest.raises(AssertionError, match=r"steps over the cap: \[4"):
        tn.check_loss_envelope("synthetic", _ahead(env), d)
    with pytest.raises(AssertionError, match="self-measured loss envelope"):
        tn.check_controls("synthetic", _ahead(env), dict(zip(d["param_names"].tolist(), d["S6"])), d["param_names"], d)


def test_cap_trips_on_a_parameter_spread():
    d = _synthetic()
    spread = dict(zip(d["param_names"].tolist(), d["S6"]))
    spread["p2"] = 1.01 * float(d["cap_param"][2])
    with pytest.raises(AssertionError, match=r"self-measured parameter spread.*p2 spreads.*over the cap: \['p2'\]"):
        tn.check_param_spread("synthetic", spread, d["param_names"], d)
    spread["p2"] = float("nan")
    with pytest.raises(AssertionError, match="p2"):
        tn.check_param_spread("synthetic", spread, d["param_names"], d)


def test_values_below_the_floor_pass():
    """a port whose controls never part (E6 = S6 = 0) leaves the 1e-5 floor of the HIP test's allowance alone: an envelope of 1e-5 / 8,
    which 8 x turns into that floor, passes whatever the port measured"""
    d = _synthetic()
    K, N = d["E6"].shape[0], d["S6"].shape[0]
    quiet = tn.derive(np.tile(np.ones(K), (6, 1)), np.zeros((6, N)), np.ones(K))
    quiet["param_names"] = d["param_names"]
    assert float(quiet["M"]) == 2 and (quiet["cap_loss"] == tn.FLOOR).all() and (quiet["cap_param"] == tn.FLOOR).all()
    env = np.full(K, tn.FLOOR)
    tn.check_controls("quiet", _ahead(env), {n: tn.FLOOR for n in d["param_names"].tolist()}, d["param_names"], quiet)
    with pytest.raises(AssertionError, match="loss envelope"):
        tn.check_loss_envelope("quiet", _ahead(env * 1.01), quiet)
    with pytest.raises(AssertionError, match="parameter spread"):
        tn.check_param_spread("quiet", {n: tn.FLOOR * 1.01 for n in d["param_names"].tolist()}, d["param_names"], quiet)
