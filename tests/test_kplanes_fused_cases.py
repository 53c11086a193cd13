"""CPU: the sizes, planted samples and exact fixture of _kplanes_fused_cases.py are what its docstring says (the GPU tests of the
fused K-Planes launches, tests/test_hip_kplanes_fused.py, rely on them)."""
import numpy as np
import pytest

import _kplanes_fused_cases as kc
import _scatter_orders as so


def test_grid_restatement_matches_the_documented_launches():
    assert kc.grid_blocks(1, 8, 256) == 1 and kc.grid_blocks(257, 8, 256) == 2 and kc.grid_blocks(1 << 20, 8, 256) == 256
    assert kc.per_cu_max(8) == 4 and kc.per_cu_max(12) == 2 and kc.per_cu_max(16) == 2
    assert kc.grid_per_cu(1 << 22, 8, 100 * 1024) == 256 and kc.grid_per_cu(1 << 22, 8, 50 * 1024) == 3 * 256
    assert kc.grid_per_cu(1 << 22, 8, 1024) == 4 * 256 and kc.grid_per_cu(1 << 22, 12, 1024) == 2 * 256
    assert kc.grid_per_cu(1 << 22, 12, 200 * 1024) == 256
    assert [kc.second_round_n(k) for k in ("train_f16x2", "train_fp32", "chain")] == [65573, 98341, 65573]
    assert [kc.second_round_n(k) for k in ("infer_pair_f16x2", "infer_pair_fp32", "infer_sigma")] == [262181, 196645, 196645]
    assert kc.ROUND_EDGES == (65536, 98304, 131072, 196608, 262144)
    # the heads' staged weights as lay_out_lds / plan_f2 lay them out, and the blocks per CU that follow
    assert [kc.lds_bytes(kc.HEAD_DIMS[h], f2) for h in ("colour", "sigma") for f2 in (False, True)] == [94016, 100336, 26144, 27312]
    assert [kc.per_cu(k) for k in kc.LAUNCHES] == [1, 1, 1, 1, 1, 2]


@pytest.mark.parametrize("launch", list(kc.LAUNCHES))
def test_every_size_list_has_its_first_round_edge_and_second_round_sizes(launch):
    waves, per_cu = kc.LAUNCHES[launch]
    ns = kc.sizes(launch)
    assert len(ns) == len(kc.SIZE_KEYS) and [kc.size_of(launch, k) for k in kc.SIZE_KEYS] == ns
    assert {1, 31, 32, 33} <= set(ns)
    assert {32 * waves - 1, 32 * waves, 32 * waves + 1} <= set(ns)
    # one block with a ragged last wave, one full block, a second block of one sample
    assert [kc.grid_blocks(n, waves, 256) for n in (32 * waves - 1, 32 * waves, 32 * waves + 1)] == [1, 1, 2]
    big = ns[-1]
    tiles = (big + 31) // 32
    for pc in ([per_cu] if per_cu is not None else range(1, kc.per_cu_max(waves) + 1)):      # whatever per_cu is:
        blocks = kc.grid_blocks(big, waves, 256 * pc)
        rs = blocks * waves * 32                                   # samples per round
        assert blocks == 256 * pc and big > rs, "the grid is at its cap and a later round is reached"
        assert rs in kc.ROUND_EDGES                                # the first round's end is a planted edge
    rs = 256 * kc.per_cu(launch) * waves * 32                      # at the derived per_cu a round opens at round_samples(launch) ...
    assert kc.round_samples(launch) % rs == 0
    assert tiles - kc.round_samples(launch) // 32 == 2 and big % 32 == 5        # ... with two tiles, the second ragged
    assert all(n <= kc.round_samples(launch) for n in ns[:-1])     # the others stay inside the first round


@pytest.mark.parametrize("n", sorted({n for k in kc.LAUNCHES for n in kc.sizes(k)}))
def test_planted_samples_sit_at_the_tile_and_round_edges(n):
    pos = kc.planted_positions(n)
    last = (n - 1) // 32 * 32
    want = {0, min(31, n - 1)} | set(range(last, n))
    for e in kc.ROUND_EDGES:
        if e < n:
            want |= set(range(e - 32, min(e + 32, n)))
    assert set(pos.tolist()) == want
    for name in kc.FIXTURES:
        x, planes, exact = kc.fixture(name, n)
        shapes = kc.shapes_of(name)
        assert x.shape == (n, 3) and x.dtype == np.float32 and len(planes) == 9 and all(p.shape[2] == 32 for p in planes)
        ppos, coord, val = kc.planted_values(n)
        assert np.array_equal(ppos, pos) and np.array_equal(coord, np.arange(len(pos)) % 3) and np.isin(val, so._EDGES).all()
        snapped = so.exact_coords(val, [s for hw in shapes for s in hw]) if exact else so.snap(val)
        assert np.array_equal(x[pos, coord], snapped), "planted values"
        cls = kc.tap_classes(x, shapes)
        # the samples at the borders of tile 0 and of the last tile -- what kplanes_classes calls tile_end and tail -- are planted ones
        # and read outside a plane; +-3 empties the whole row
        for border in (0, min(31, n - 1), n - 1):
            assert border in want and cls[border] >= 1, (name, n, border)
        assert np.all(cls[pos[np.abs(val) == 3.0]] == 2)
        # wherever a whole tile is planted both kinds of out-of-range sample occur
        for t0 in {last} | {e + d for e in kc.ROUND_EDGES if e < n for d in (-32, 0)}:
            t1 = min(t0 + 32, n)
            if t1 - t0 >= 24:
                assert {1, 2} <= set(cls[t0:t1].tolist()), (name, n, t0)
    # 24 consecutive planted samples of either half take every (coordinate, value) pair once
    if len(pos) >= 48:
        for sl in (slice(0, 24), slice(len(pos) - 24, len(pos))):
            assert len(set(zip(coord[sl].tolist(), val[sl].tolist()))) == 24


def test_tap_classes_on_hand_made_points():
    shapes = [(17, 17)] * 3
    x = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [-1.0 - 2.0 ** -10, 0.0, 0.0], [0.0, 3.0, 0.0], [-1.0, -1.0, -1.0],
                  [1.0 - 2.0 ** -10, 0.5, 0.5]], np.float32)
    assert kc.tap_classes(x, shapes).tolist() == [0, 1, 1, 2, 0, 0]


def test_probe_positions():
    assert kc.probes(1).tolist() == [0]
    assert kc.probes(33).tolist() == [0, 31, 32]
    assert kc.probes(257).tolist() == [0, 31, 32, 256]
    assert kc.probes(255).tolist() == [0, 31, 32, 239, 254]
    assert kc.probes(65573).tolist() == [0, 31, 32, 65535, 65536, 65570, 65572]


@pytest.mark.parametrize("n", [33, 257, 65573])
def test_exact_fixture_is_exact(n):
    """every feature of the exact fixture is a dyadic number that fp32 holds whatever the order of the products: the fp64 reference is
    its own fp32 rounding (checked on the reference alone, as _scatter_orders.assert_exact does for the stand-alone kernels)"""
    x, planes, exact = kc.fixture("exact", n)
    assert exact
    shapes = kc.shapes_of("exact")
    fb, _ = so.kp_exact_bits(x, shapes, planes, np.zeros((1, 1)))
    ref, aref = kc.reference("exact", n)
    so.assert_exact(ref, aref, fb, f"exact n={n}")
    assert fb <= 6


def test_forward_only_reference_equals_the_autograd_one():
    x, planes, _ = kc.fixture("nonsquare", 385)
    ref, aref = kc.features_fp64(x, planes)
    full = so.kplanes_ref(x, list(planes), np.ones((385, 96), np.float32))
    assert np.array_equal(ref, full[0]) and np.array_equal(aref, full[1])
    cls = kc.tap_classes(x, kc.shapes_of("nonsquare"))
    assert np.all(aref[cls == 2].min(1) == 0.0) and np.all(aref[cls == 0] >= 0.0)
