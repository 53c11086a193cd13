"""G23: how fast fp32 trajectories of the G22 recipes part, measured on the CPU port (oracle/make_trace_noise.py), and the caps
that tests/test_hip_train_trace.py puts on the HIP trainer's own control runs from it.  Pure numpy: the recipe calls ``derive`` to
store the derived quantities, the tests call it to recompute them.

Raw arrays per trace (C = 6 controls, K steps, N recorded parameters):
``loss[c, k]``     per-step loss of control c (every floating parameter moved by 1 + 2^-22 (U - 0.5) before step 0)
``spread[c, n]``   max |control - unperturbed| / max |unperturbed| of parameter n after the last step, on what
                   ``_g22.compare_final_state`` compares
``record[k]``      the reference's own per-step loss (G22)

Derived:
``E6[k]``          max over the controls of the cumulative max over steps of |loss_c / record - 1|
``S6[n]``          max over the controls of spread[c, n]
``R``, ``R_p``     sampling ratio: over the 10 ways to split the six controls into 3 + 3 and every step (parameter) at which both
                   halves' three-control envelopes (spreads) are >= 1e-6, the largest (larger half) / (smaller half) -- how much a
                   THREE-control envelope, which is what the GPU test can afford, fluctuates from the random onset of the divergence
``M = 2 R``, ``M_p = 2 R_p``   the factor 2: the HIP trainer has one more source of ulp-sized disturbance than the port, the order of
                   its gradient atomics -- a second disturbance of the perturbation's size at most doubles the initial distance, and a
                   chaotic system carries that factor along
``cap_loss[k]``    max(1e-5 / 8, M * E6[min(k + 1, K - 1)])    (one step ahead, as the HIP test reads its own envelope)
``cap_param[n]``   max(1e-5 / 8, M_p * S6[n])"""
from itertools import combinations

import numpy as np

TRACES = ("kplanes", "vanilla", "kplanes_lr")
FLOOR = 1e-5 / 8
ONSET = 1e-6


def control_envelopes(loss, record):
    """[C, K]: per control, the cumulative |loss_c / record - 1|"""
    loss, record = np.asarray(loss, np.float64), np.asarray(record, np.float64)
    return np.maximum.accumulate(np.abs(loss / record[None, :] - 1), axis=1)


def sampling_ratio(per_control):
    """``per_control`` [C, X] (C even): largest ratio between the two halves' maxima over all balanced splits and every column at
    which both halves are >= ONSET; 1 where no column qualifies"""
    a = np.asarray(per_control, np.float64)
    C = a.shape[0]
    assert C % 2 == 0 and C >= 2
    worst = 1.0
    for half in combinations(range(C), C // 2):
        if 0 not in half:            # (each split once)
            continue
        other = [c for c in range(C) if c not in half]
        x, y = a[list(half)].max(0), a[other].max(0)
        ok = (x >= ONSET) & (y >= ONSET)
        if ok.any():
            worst = max(worst, float((np.maximum(x, y)[ok] / np.minimum(x, y)[ok]).max()))
    return worst


def derive(loss, spread, record):
    env = control_envelopes(loss, record)
    spread = np.asarray(spread, np.float64)
    K = env.shape[1]
    E6, S6 = env.max(0), spread.max(0)
    R, R_p = sampling_ratio(env), sampling_ratio(spread)
    M, M_p = 2.0 * R, 2.0 * R_p
    ahead = np.minimum(np.arange(K) + 1, K - 1)
    return {"E6": E6, "S6": S6, "R": np.float64(R), "R_p": np.float64(R_p), "M": np.float64(M), "M_p": np.float64(M_p),
            "cap_loss": np.maximum(FLOOR, M * E6[ahead]), "cap_param": np.maximum(FLOOR, M_p * S6)}


def load(name, golden):
    """the stored arrays of one trace out of ``golden`` (the loaded G23 file)"""
    return {k[len(name) + 1:]: v for k, v in golden.items() if k.startswith(name + "/")}


def check_loss_envelope(name, envelope_ahead, d):
    """``envelope_ahead[k]``: the HIP controls' cumulative envelope read one step ahead (the array test_hip_train_trace multiplies by 8
    for its allowance).  Returns (worst envelope_ahead / (M E6 one step ahead), its step)."""
    envelope_ahead = np.asarray(envelope_ahead, np.float64)
    K = envelope_ahead.shape[0]
    ahead = np.minimum(np.arange(K) + 1, d["E6"].shape[0] - 1)
    cap, M, E6 = d["cap_loss"][:K], float(d["M"]), d["E6"][ahead]
    ratio = envelope_ahead / np.maximum(M * E6, 1e-300)
    ratio[envelope_ahead <= FLOOR] = 0.0          # (below the floor nothing is asked)
    k = int(np.argmax(ratio))
    print(f"{name} loss envelope: worst HIP controls' envelope / (M x port controls' E6) = {ratio[k]:.3g} at step {k} "
          f"(both read at step {ahead[k]}: HIP {envelope_ahead[k]:.3g}, port {E6[k]:.3g}, M = {M:.3g})")
    bad = np.nonzero(~(envelope_ahead <= cap))[0]
    if bad.size:
        b = int(bad[np.argmax((envelope_ahead / cap)[bad])])
        raise AssertionError(
            f"{name}: the HIP trainer's OWN control runs part faster than the port's -- this is the self-measured loss envelope, not the "
            f"comparison with the reference's record: at step {b} the HIP controls' envelope (read at step {ahead[b]}) is {envelope_ahead[b]:.3g}, "
            f"the cap {cap[b]:.3g} = max({FLOOR:.3g}, M x E6[{ahead[b]}]), port E6 = {E6[b]:.3g}, M = {M:.3g}; steps over the cap: {bad.tolist()}")
    return float(ratio[k]), k


def check_param_spread(name, spread_hip, param_names, d):
    """``spread_hip``: name -> the HIP controls' spread of that parameter.  Returns (worst spread_hip / (M_p S6), its name)."""
    names = [str(n) for n in param_names]
    cap, M_p, S6 = d["cap_param"], float(d["M_p"]), d["S6"]
    hip = np.array([spread_hip[n] for n in names], np.float64)
    ratio = hip / np.maximum(M_p * S6, 1e-300)
    ratio[hip <= FLOOR] = 0.0
    i = int(np.argmax(ratio))
    print(f"{name} parameters: worst HIP controls' spread / (M_p x port controls' S6) = {ratio[i]:.3g} at {names[i]} "
          f"(HIP {hip[i]:.3g}, port {S6[i]:.3g}, M_p = {M_p:.3g})")
    bad = [j for j in range(len(names)) if not hip[j] <= cap[j]]
    if bad:
        j = max(bad, key=lambda q: hip[q] / cap[q])
        raise AssertionError(
            f"{name}: the HIP trainer's OWN control runs spread further than the port's -- this is the self-measured parameter spread, not "
            f"the comparison with the reference's record: {names[j]} spreads by {hip[j]:.3g} of its largest value, cap {cap[j]:.3g} = "
            f"max({FLOOR:.3g}, M_p x S6), port S6 = {S6[j]:.3g}, M_p = {M_p:.3g}; over the cap: {[names[q] for q in bad]}")
    return float(ratio[i]), names[i]


def check_controls(name, envelope_ahead, spread_hip, param_names, d):
    """both caps; every headroom figure is printed before anything is raised"""
    failures = []
    for check, args in ((check_loss_envelope, (envelope_ahead,)), (check_param_spread, (spread_hip, param_names))):
        try:
            check(name, *args, d)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)
