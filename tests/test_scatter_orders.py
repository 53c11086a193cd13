"""CPU: the sample-order families of _scatter_orders.py do what test_hip_scatter.py relies on them for.

* every phase-B branch of kp_scatter_scale (same cell, x+-1, y+-1, the four diagonals, flush, the false row-wrap neighbour, the
  ragged tail) occurs in the K-Planes streams, in every plane pair of every scale of every case;
* the Cobafa streams hold runs that cross a 64-sample wave boundary and waves that end mid-run, in every lookup;
* the exact fixtures are exact: the fp64 reference is its own fp32 rounding and no partial sum can round in fp32;
* the numpy restatement of the cell arithmetic classifies a hand-built stream as intended.
"""
import numpy as np
import pytest

import _scatter_orders as so

FAMS = list(so.FAMILIES)


def _kp_counts(cases, name, n):
    C, shapes, single = cases[name]
    tot = {}
    for f in FAMS:
        x = so.kp_fixture(cases, name, f, n, seed=so.seed_of(name, f))[0]
        for s, (H, W) in enumerate(shapes):
            for p in range(1 if single else 3):
                c = so.kplanes_classes(x, H, W, p)
                for k, v in c.items():
                    tot[(s, p, k)] = tot.get((s, p, k), 0) + v
    return tot


@pytest.mark.parametrize("name", list(so.KP_GENERAL))
def test_kplanes_general_streams_hit_every_branch(name):
    C, shapes, single = so.KP_GENERAL[name]
    tot = _kp_counts(so.KP_GENERAL, name, so.N_GENERAL)
    for s in range(len(shapes)):
        for p in range(1 if single else 3):
            miss = [k for k in so.KP_CLASSES if tot[(s, p, k)] == 0]
            assert not miss, (name, s, p, miss)


@pytest.mark.parametrize("name", list(so.KP_EXACT))
def test_kplanes_exact_streams_hit_every_branch(name):
    """exact coordinates sit on the half-texel grid of the coarsest side, so a finer axis moves several texels at once: every
    branch in every plane pair, on at least one scale"""
    C, shapes, single = so.KP_EXACT[name]
    tot = _kp_counts(so.KP_EXACT, name, so.N_EXACT)
    for p in range(1 if single else 3):
        miss = [k for k in so.KP_CLASSES if k != "tile_end" and all(tot[(s, p, k)] == 0 for s in range(len(shapes)))]
        assert not miss, (name, p, miss)


def test_classifier_on_a_hand_built_stream():
    """one plane pair (x, y) of a 9 x 9 plane: a walk whose moves are known"""
    H = W = 9
    h = so.cell_width(W)
    cells = [(0, 0), (0, 0), (1, 0), (0, 0), (0, 1), (0, 0), (1, 1), (0, 0), (-1, 1), (0, 0), (1, -1), (0, 0), (-1, -1),
             (0, 0), (5, 5), (W + 1, 2), (-2, 3)]
    x = np.array([[-1.0 + h * (cx + 0.5) if -1 <= cx < W else (3.0 if cx > 0 else -3.0), -1.0 + h * (cy + 0.5), 0.0]
                  for cx, cy in cells])
    x[:, :2] += 2 * h                                     # away from the border, except the clamped columns
    x[-2, 0], x[-1, 0] = 7.0, -7.0
    c = so.kplanes_classes(so.snap(x), H, W, 0)
    # every diagonal twice (out and back); x+ once for real and once across the row wrap
    want = {"same": 1, "x+": 1 + 1, "x-": 1, "y+": 1, "y-": 1, "++": 2, "-+": 2, "+-": 2, "--": 2, "flush": 2, "false_wrap": 1,
            "tail": 1, "tile_end": 0}
    assert c == want, c


@pytest.mark.parametrize("cases,name", [(so.CB_GENERAL, k) for k in so.CB_GENERAL] + [(so.CB_EXACT, k) for k in so.CB_EXACT])
def test_cobafa_streams_cross_waves(cases, name):
    cres, levels = cases[name]
    for look in [(cres, 0.0)] + [(r, f) for r, f, _ in levels]:
        tot = {"cross_wave": 0, "merged": 0, "end_mid_run": 0}
        for f in FAMS:
            x = so.cb_fixture(cases, name, f, so.N_COBAFA, seed=so.seed_of(name, f))[0]
            r = so.cobafa_runs(x, [look])
            for k in tot:
                tot[k] += r[k]
        assert tot["cross_wave"] > 0 and tot["merged"] > 0 and tot["end_mid_run"] > 0, (name, look, tot)


@pytest.mark.parametrize("name", list(so.KP_EXACT))
@pytest.mark.parametrize("family", FAMS)
def test_kplanes_exact_fixture_precondition(name, family):
    x, planes, g, exact = so.kp_fixture(so.KP_EXACT, name, family, so.N_EXACT, seed=7)
    assert exact
    shapes = so.KP_EXACT[name][1]
    fb, tb = so.kp_exact_bits(x, shapes, planes, g)
    feat, afeat, grads, agrads = so.kplanes_ref(x, planes, g)
    so.assert_exact(feat, afeat, fb, "features")
    for i, (r, a) in enumerate(zip(grads, agrads)):
        if r is not None:
            so.assert_exact(r, a, tb, f"plane {i}")
            assert np.count_nonzero(r) > 0, i


@pytest.mark.parametrize("name", list(so.CB_EXACT))
@pytest.mark.parametrize("family", FAMS)
def test_cobafa_exact_fixture_precondition(name, family):
    x, coef, basis, freqs, g, exact = so.cb_fixture(so.CB_EXACT, name, family, so.N_COBAFA, seed=7)
    cres, levels = so.CB_EXACT[name]
    fb, tb = so.cb_exact_bits(x, cres, levels, g)
    feat, afeat, grads, agrads = so.cobafa_ref(x, coef, basis, freqs, g)
    so.assert_exact(feat, afeat, fb, "features")
    for i, (r, a) in enumerate(zip(grads, agrads)):
        so.assert_exact(r, a, tb, f"grid {i}")
