"""Gradient comparison "up to the state of fp32-tie ReLU units" (see oracle/torch_port.ReluControl).

A hidden unit whose pre-activation is a rounding-level tie can be on in ATen's summation order and off in the MFMA K-order
(or vice versa).  Both are correct fp32 evaluations of the reference network, but the unit's backward contribution differs,
which moves that sample's gradient by O(1 %) -- far above any fp32 tolerance.  Instead of picking seeds without such units,
the comparison lets every recorded tie unit take either state: the reference is re-evaluated with one tie unit flipped at a
time (closest ties first; flips of different units are additive to first order because they sit in different samples or
layers), a flip is accepted when the projection of (got - current) on its direction says so, and the result must match
within the stated tolerance.  With no ties, or when nothing flipped (the common cases), this is a plain comparison."""
from typing import Callable, Dict

import numpy as np

from oracle import torch_port as tp


def _flat(d: Dict[str, np.ndarray], keys) -> np.ndarray:
    return np.concatenate([np.asarray(d[k], np.float64).ravel() for k in keys])


def _check(got, ref, keys, rel, what):
    for k in keys:
        r = np.asarray(ref[k], np.float64)
        rk = rel[k] if isinstance(rel, dict) else rel
        np.testing.assert_allclose(np.asarray(got[k], np.float64), r, rtol=0, atol=rk * max(float(np.abs(r).max()), 1e-30),
                                   err_msg=f"{k} ({what}; tolerance {rk:.1e} of the largest element)")


def _matches(got, ref, keys, rel) -> bool:
    try:
        _check(got, ref, keys, rel, "")
        return True
    except AssertionError:
        return False


def assert_grads_match_up_to_relu_ties(got: Dict[str, np.ndarray], compute_ref: Callable[[], Dict[str, np.ndarray]], rel,
                                       eps: float = 2e-6, max_flips: int = 256, weights_conditioning: bool = False,
                                       golden: Dict[str, np.ndarray] = None, cond_cap: float = None, matched: dict = None) -> int:
    """``compute_ref()`` evaluates the reference gradients through oracle/torch_port.mlp (on any device) and returns
    {name: array}.  |got - ref| <= rel * max|ref| per tensor (``rel``: one number or {name: number}) for some assignment of the tie units (|pre| <= eps * sum |terms|;
    the rounding error of an fp32 dot product of K <= 307 terms is ~sqrt(K) * 6e-8 = 1e-6 of that sum).  Returns the number of
    tie units that had to be flipped.
    ``golden`` {name: gradient captured from the reference itself}: when no tie unit had to be flipped, `got` is ALSO compared
    with it directly, same tolerance -- the reference stays the oracle, the port only supplies the tie bookkeeping.
    ``cond_cap``: upper bound on any conditioning-derived tolerance (a fixture whose reference gradients are looser than this
    pins nothing and must be replaced).
    ``matched`` (a dict): receives the reference gradients `got` was finally held to (tie units in their accepted states) and, under
    the key "rel", the tolerances used -- for callers that report how much of the allowance was used."""
    if weights_conditioning:
        # render-level fixtures: the reference's fp32 weights backward (cuda.cu:49-56) is itself only this close to an exact
        # evaluation of its formula (oracle/torch_port.weights_conditioning); no other fp32 order can be held to less
        cond = tp.weights_conditioning(compute_ref)
        rel = {k: max(rel[k] if isinstance(rel, dict) else rel, 4.0 * c) for k, c in cond.items()}
    if cond_cap is not None:
        worst = max(rel.values()) if isinstance(rel, dict) else rel
        assert worst <= cond_cap, f"tolerance {worst:.1e} exceeds the cap {cond_cap:.1e}: " + str({k: f"{v:.1e}" for k, v in rel.items() if v > cond_cap} if isinstance(rel, dict) else rel)
    with tp.ReluControl(eps) as ctrl:
        base = compute_ref()
    keys = sorted(base)

    def tol(k, ref):
        return (rel[k] if isinstance(rel, dict) else rel) * max(float(np.abs(np.asarray(ref[k])).max()), 1e-30)

    def score(ref):          # worst violation in units of the tolerance; <= 1 passes
        return max(float(np.abs(np.asarray(got[k], np.float64) - np.asarray(ref[k], np.float64)).max()) / tol(k, base) for k in keys)
    if score(base) <= 1.0:
        if golden is not None:
            _check(got, golden, keys, {k: tol(k, base) / max(float(np.abs(np.asarray(golden[k])).max()), 1e-30) for k in keys},
                   "directly against the reference's golden gradients")
        if matched is not None:
            matched.update(base, rel={k: tol(k, base) / max(float(np.abs(np.asarray(base[k])).max()), 1e-30) for k in keys})
        return 0
    def dist2(ref):          # squared distance in units of the tolerances: every correct flip lowers it, whatever the others do
        return sum(float((((np.asarray(got[k], np.float64) - np.asarray(ref[k], np.float64)) / tol(k, base)) ** 2).sum()) for k in keys)
    ties = sorted(dict.fromkeys(ctrl.found), key=lambda t: ctrl.state[t][1])[:max_flips]
    cur = {k: np.asarray(v, np.float64).copy() for k, v in base.items()}
    flips = {}
    for t in ties:           # a flip is kept when it brings the reference closer to `got`
        with tp.ReluControl(eps, force={t: not ctrl.state[t][0]}):
            alt = compute_ref()
        cand = {k: cur[k] + (np.asarray(alt[k], np.float64) - np.asarray(base[k], np.float64)) for k in keys}
        if dist2(cand) < dist2(cur):
            cur, flips[t] = cand, not ctrl.state[t][0]
            if score(cur) <= 1.0:
                break
    if len(flips) > 1:                      # several flips: evaluate them together (exact, not the first-order sum)
        with tp.ReluControl(eps, force=flips):
            cur = compute_ref()
    _check(got, cur, keys, {k: tol(k, base) / max(float(np.abs(np.asarray(cur[k])).max()), 1e-30) for k in keys},
           f"{len(flips)} of {len(ties)} tie units flipped: {sorted(flips)}")
    if matched is not None:
        matched.update(cur, rel={k: tol(k, base) / max(float(np.abs(np.asarray(cur[k])).max()), 1e-30) for k in keys})
    return len(flips)
