"""The hash grid's float64 yardstick (tests/_hashgrid_ref.py) pinned on closed forms, on the CPU: trilinear interpolation is exact on
affine data, a node returns its entry, hand-computed hashes, clamping at and beyond the boundary, forward and scatter adjoint."""
import numpy as np
import pytest

import _hashgrid_ref as ref


def dense_plan(n_l):
    """one dense level of resolution n_l"""
    return ref.levels(1, 30, n_l, n_l)


def affine_table(plan, coef):
    """entry of node (ix, iy, iz) of a dense one-level plan = a0 + a . node position in [-1, 1]^3, F = 2 (second channel negated)"""
    n_l, E = plan[0][0], ref.total_entries(plan)
    s = n_l + 1
    idx = np.arange(s ** 3)
    node = np.stack([idx % s, idx // s % s, idx // (s * s)], 1) * (2.0 / n_l) - 1.0
    t = np.zeros((E, 2))
    t[:s ** 3, 0] = coef[0] + node @ coef[1:]
    t[:s ** 3, 1] = -t[:s ** 3, 0]
    return t


def test_level_plan_of_the_small_and_the_default_configuration():
    res, hashed, entries, offsets = ref.levels(**ref.SMALL)
    assert res == [2, 5, 13, 32] and hashed == [False, False, True, True]
    assert entries == [32, 216, 256, 256] and offsets == [0, 32, 248, 504]           # 27 nodes padded to 32; 6^3 = 216
    res, hashed, entries, offsets = ref.levels(**ref.DEFAULT)
    assert res[0] == 16 and res[-1] == 2048 and len(res) == 16 and all(a < b for a, b in zip(res, res[1:]))
    assert hashed == [False] * 5 + [True] * 11                                       # 59^3 <= 2^19 < 82^3
    assert entries[0] == (17 ** 3 + 7) // 8 * 8 and entries[5:] == [1 << 19] * 11 and all(e % 8 == 0 for e in entries)
    assert offsets == [sum(entries[:l]) for l in range(16)]
    assert ref.levels(1, 8, 7, 7)[0] == [7]                                          # L = 1: b = 1


@pytest.mark.parametrize("n_l", [1, 2, 7, 32])
def test_affine_data_is_reproduced_exactly(n_l):
    plan = dense_plan(n_l)
    coef = np.array([0.3, -1.25, 0.5, 2.0])
    rng = np.random.default_rng(n_l)
    x = rng.uniform(-1, 1, (500, 3)).astype(np.float32)
    feat = ref.forward(affine_table(plan, coef), x, plan)
    # the interpolant is affine in the fp32 position p the yardstick derives, so compare at the point p stands for
    i, f = ref.cell(x, n_l)
    xp = (i + f) * (2.0 / n_l) - 1.0
    want = coef[0] + xp @ coef[1:]
    assert np.abs(feat[:, 0] - want).max() <= 1e-13 and np.abs(feat[:, 1] + want).max() <= 1e-13
    assert np.abs(xp - x).max() <= 2.0 ** -23 * 2                                    # ... which is x to fp32 rounding of p


def test_at_a_node_the_output_is_the_entry():
    plan = ref.levels(**ref.SMALL)
    rng = np.random.default_rng(0)
    table = rng.uniform(-1, 1, (ref.total_entries(plan), 2))
    for l, n_l in enumerate(plan[0]):
        if n_l not in (2, 32):               # node positions 2 k / N - 1 that fp32 holds exactly
            continue
        k = rng.integers(0, n_l + 1, (50, 3))
        x = (k * (2.0 / n_l) - 1.0).astype(np.float32)
        idx = ref.node_index(k[:, 0], k[:, 1], k[:, 2], n_l, plan[1][l], plan[2][l])
        got = ref.forward(table, x, plan)[:, 2 * l:2 * l + 2]
        assert np.array_equal(got, table[plan[3][l] + idx])


def test_hashes_of_hand_computed_nodes():
    for log2_T in (8, 14, 19):
        T = 1 << log2_T
        assert ref.node_index(1, 0, 0, 99, True, T) == 1
        assert ref.node_index(0, 1, 0, 99, True, T) == 2654435761 % T
        assert ref.node_index(0, 0, 1, 99, True, T) == 805459861 % T
        assert ref.node_index(3, 5, 7, 99, True, T) == (3 ^ (5 * 2654435761 % 2 ** 32) ^ (7 * 805459861 % 2 ** 32)) % T
    assert ref.node_index(2, 3, 4, 5, False, 0) == 2 + 6 * (3 + 6 * 4)


def test_boundary_and_outside_points_clamp_to_the_boundary_nodes():
    n_l = 5
    plan = dense_plan(n_l)
    table = affine_table(plan, np.array([0.0, 1.0, 10.0, 100.0]))
    big = np.float32(3e38)
    x = np.array([[1, 1, 1], [-1, -1, -1], [1.5, -7, big], [-big, np.inf, -np.inf], [np.nan, np.nan, np.nan]], np.float32)
    i, f = ref.cell(x, n_l)
    assert np.array_equal(i[0], [4, 4, 4]) and np.array_equal(f[0], [1, 1, 1])       # the last cell, fraction 1: the node N
    assert np.array_equal(i[1], [0, 0, 0]) and np.array_equal(f[1], [0, 0, 0])
    assert np.array_equal(i[4], [0, 0, 0]) and np.array_equal(f[4], [0, 0, 0])       # a NaN lands on 0
    got = ref.forward(table, x, plan)[:, 0]
    assert np.allclose(got, [111, -111, 1 - 10 + 100, -1 + 10 - 100, -111], atol=1e-12)


@pytest.mark.parametrize("cfg,features", [(ref.SMALL, 2), (ref.SMALL, 4), (ref.FINE, 2)])
def test_forward_and_scatter_are_adjoint(cfg, features):
    plan = ref.levels(**cfg)
    rng = np.random.default_rng(7)
    x = ref.sample_points(300, plan, 3)
    table = rng.uniform(-1, 1, (ref.total_entries(plan), features))
    g = rng.uniform(-1, 1, (300, len(plan[0]) * features))
    grad, m, abs_sum = ref.backward(g, x, plan, features)
    lhs, rhs = (ref.forward(table, x, plan) * g).sum(), (table * grad).sum()
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))
    assert m.sum() == 300 * 8 * len(plan[0]) and np.all(abs_sum >= np.abs(grad) - 1e-15)
    assert np.all(grad[m == 0] == 0)
