"""CPU checks of the mesh-smoothing yardstick: tests/_mesh_smooth_ref.py on hand-checked tiny meshes, and the properties the
definition was chosen for, on the yardstick's own Surface Nets meshes -- ten Taubin iterations take the staircase out of a binary
sphere without shrinking it where plain Laplacian steps lose a tenth of its volume, an open mesh's rim stays where it is, and the
normals of the faces agree with the extractor's."""
import numpy as np
import pytest

import _mesh_ref as mref
import _mesh_smooth_ref as ref

TETRA = np.int32([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]])     # counter-clockwise from outside for the corners below
TETRA_P = np.float64([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])


def test_one_triangle_by_hand():
    offsets, pairs, pinned, stats = ref.adjacency([[4, 1, 2]], 6)
    assert offsets.tolist() == [0, 0, 1, 2, 2, 3, 3] and pairs.tolist() == [[2, 4], [4, 1], [1, 2]]      # (b,v,a) -> (a,b); (a,b,v); (v,a,b)
    assert pinned.tolist() == [1] * 6 and stats == (1, 0, 1)
    assert offsets.dtype == np.int32 and pairs.dtype == np.int32 and pinned.dtype == np.uint8


def test_tetrahedron_by_hand():
    offsets, pairs, pinned, stats = ref.adjacency(TETRA, 4)
    assert offsets.tolist() == [0, 3, 6, 9, 12] and stats == (4, 4, 3) and not pinned.any()
    assert pairs[:3].tolist() == [[2, 1], [1, 3], [3, 2]]          # vertex 0: faces 0, 1, 3 in that order
    assert pairs[9:].tolist() == [[0, 1], [1, 2], [2, 0]]          # vertex 3: faces 1, 2, 3
    # one pass: every neighbour counted twice -> the mean of the other three corners
    out, bound = ref.smooth_pass(TETRA_P, offsets, pairs, pinned, 0.5)
    assert np.allclose(out[0], 0.5 * np.float64([1, 1, 1]) / 3) and np.allclose(out[3], [1 / 6, 1 / 6, 0.5]) and (bound >= 0).all()
    n, g, nb = ref.vertex_normals(TETRA_P, offsets, pairs)
    assert np.allclose(n[0], -np.ones(3) / np.sqrt(3)) and np.allclose(g[0], [-1, -1, -1])       # three right triangles of area 1/2, summed twice
    assert (np.einsum("ij,ij->i", n, TETRA_P - TETRA_P.mean(0)) > 0).all() and np.isfinite(nb).all()


@pytest.mark.parametrize("faces,V,want_pinned,want_stats", [
    ([[1, 2, 3], [3, 2, 4]], 5, [1, 1, 1, 1, 1], (2, 0, 2)),                                     # two triangles on an edge: all on the rim
    ([[0, 1, 2], [0, 1, 3], [0, 1, 4]], 5, [1, 1, 1, 1, 1], (3, 0, 3)),                          # three on one edge: non-manifold and rim
    ([[0, 1, 2], [2, 3, 5], [3, -1, 4], [-1, -1, -1], [4, 3, 3], [1, 0, 2]], 5, [0, 0, 0, 1, 1], (2, 3, 2)),      # invalid rows take no part; a two-sided triangle is closed
    (np.zeros((0, 3)), 3, [1, 1, 1], (0, 0, 0)),
    (np.zeros((0, 3)), 0, [], (0, 0, 0)),
])
def test_boundaries_non_manifold_edges_and_invalid_rows(faces, V, want_pinned, want_stats):
    offsets, pairs, pinned, stats = ref.adjacency(faces, V)
    assert pinned.tolist() == want_pinned and stats == want_stats and offsets[-1] == 3 * stats[0] == pairs.shape[0]


def test_a_fan_frees_its_hub_alone_and_twice_the_same_face_pins():
    faces, V = ref.fan(7)
    offsets, pairs, pinned, stats = ref.adjacency(faces, V)
    assert pinned.tolist() == [0] + [1] * 7 and stats == (7, 1, 7)
    assert pairs[:7].tolist() == [[1 + i, 1 + (i + 1) % 7] for i in range(7)]
    # the tetrahedron with one face twice: that face's corners see ids four times
    offsets, pairs, pinned, stats = ref.adjacency(np.concatenate([TETRA, TETRA[:1]]), 4)
    assert pinned.tolist() == [1, 1, 1, 0] and stats == (5, 1, 4)


def test_the_sorted_and_the_looped_adjacency_agree():
    rng = np.random.default_rng(3)
    cases = [(rng.integers(-1, 9, (40, 3)), 8), (ref.fan(5)[0], 6), (ref.binary_sphere()[2], 590), (ref.tilted_plane()[2], ref.tilted_plane()[0].shape[0])]
    for faces, V in cases:
        a, b = ref.adjacency(faces, V), ref.adjacency_loop(faces, V)
        assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def test_a_pass_leaves_pinned_and_bare_vertices_alone_and_nan_propagates():
    faces, V = ref.fan(5)
    offsets, pairs, pinned, _ = ref.adjacency(faces, V + 1)        # one isolated vertex
    p = np.random.default_rng(0).standard_normal((V + 1, 3))
    out, _ = ref.smooth_pass(p, offsets, pairs, pinned, 0.5)
    assert np.array_equal(out[1:], p[1:]) and np.allclose(out[0], 0.5 * p[0] + 0.5 * p[1:6].mean(0))
    free, _ = ref.smooth_pass(p, offsets, pairs, None, 0.5)
    assert not np.array_equal(free[1:6], p[1:6]) and np.array_equal(free[6], p[6])
    p[2, 1] = np.nan
    out, _ = ref.smooth_pass(p, offsets, pairs, pinned, 0.5)
    assert np.isnan(out[0, 1]) and np.isfinite(out[0, [0, 2]]).all()
    assert np.array_equal(ref.taubin(p, offsets, pairs, pinned, 0)[0], p, equal_nan=True)


def test_taubin_smooths_the_binary_sphere_without_shrinking_it():
    vert, _, faces = ref.binary_sphere()
    assert vert.shape == (590, 3) and faces.shape == (1176, 3) and mref.edge_report(faces)[:2] == (True, True)
    offsets, pairs, pinned, stats = ref.adjacency(faces, 590)
    assert stats == (1176, 590, 12)
    out, bound = ref.taubin(vert, offsets, pairs, pinned, 10)
    ratio = ref.radial_std(out, ref.BINARY_CENTRE) / ref.radial_std(vert, ref.BINARY_CENTRE)
    v0, v1 = mref.signed_volume(vert, faces), mref.signed_volume(out, faces)
    print(f"radial std {ref.radial_std(vert, ref.BINARY_CENTRE):.5f} -> {ref.radial_std(out, ref.BINARY_CENTRE):.5f} (ratio {ratio:.3f}), "
          f"volume {v0:.4f} -> {v1:.4f} ({(v1 - v0) / v0:+.2%}), carried bound {bound.max():.2e}")
    assert ratio < 0.8 and abs(v1 - v0) / v0 < 0.02
    lap = vert
    for _ in range(10):                                            # the same number of plain Laplacian steps (lambda alone)
        lap, _ = ref.smooth_pass(lap, offsets, pairs, pinned, ref.LAMBDA)
    v2 = mref.signed_volume(lap, faces)
    print(f"10 Laplacian steps: volume {v2:.4f} ({(v2 - v0) / v0:+.2%})")
    assert (v0 - v2) / v0 > 0.10
    # the carried bound grows by |1 - mu| + |mu| = 2.06 per iteration (no cancellation assumed): still a hundredth of a cell (0.125)
    assert bound.max() < 2e-3


def test_the_tilted_planes_rim_does_not_move_and_it_stays_a_plane():
    vert, _, faces = ref.tilted_plane()
    offsets, pairs, pinned, stats = ref.adjacency(faces, vert.shape[0])
    print(f"tilted plane: {vert.shape[0]} vertices, {int(pinned.sum())} pinned, stats {stats}")
    assert (vert.shape[0], int(pinned.sum()), stats) == (141, 42, (238, 99, 6))
    out, _ = ref.taubin(vert, offsets, pairs, pinned, 10)
    assert np.array_equal(out[pinned == 1], vert[pinned == 1]) and not np.array_equal(out[pinned == 0], vert[pinned == 0])

    def off_plane(p):                                              # the largest distance from the least-squares plane
        q = p - p.mean(0)
        return float(np.abs(q @ np.linalg.svd(q)[2][2]).max())

    print(f"distance from the least-squares plane: {off_plane(vert):.2e} before, {off_plane(out):.2e} after")
    assert off_plane(out) < 2e-8                                   # float64 passes over vertices computed from float32 node values


def test_face_normals_agree_with_the_extractors():
    vert, normals, faces = ref.binary_sphere()
    offsets, pairs, _, _ = ref.adjacency(faces, 590)
    n, g, bound = ref.vertex_normals(vert, offsets, pairs)
    dots = np.einsum("ij,ij->i", n, normals)
    print(f"binary sphere: smallest dot product with the extractor's normals {dots.min():.3f}")
    assert dots.min() > 0.8 and np.allclose(np.linalg.norm(n, axis=1), 1) and bound.max() < 1e-3
    # fallback: a vertex without faces, and a fan of zero area
    faces, V = ref.fan(4)
    offsets, pairs, _, _ = ref.adjacency(faces, V + 1)
    flat = np.zeros((V + 1, 3))
    flat[:, 0] = np.arange(V + 1)                                  # all on one line: every cross product is 0
    fb = np.arange(3 * (V + 1), dtype=np.float64).reshape(-1, 3)
    n, _, bound = ref.vertex_normals(flat, offsets, pairs, fb)
    assert np.array_equal(n, fb) and np.isinf(bound).all()
    assert not ref.vertex_normals(flat, offsets, pairs)[0].any()
