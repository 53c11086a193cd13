"""GPU tests of the mesh-component filter: tn_mesh_components and tn_mesh_filter through the C ABI against the sequential
union-find of tests/_mesh_components_ref.py -- labels, face counts, stats, counts, src, renumbered faces and attribute rows, all for
equality --, on tiny meshes, long chains, many components around the scan's trip edge, Surface Nets meshes with floaters, the
capacity contract, two calls giving the same bytes, and export_clean_mesh / train(mesh_keep_fraction=...) end to end."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

import _mesh_components_ref as ref
import _mesh_ref as mref

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL_F, SENTINEL_I, SENTINEL_B, TAIL = -7.25, -12345, 0xA5, 5
EDGE = 256 * 1024                                                  # 1024 workgroups of 256: the scan's trip edge


# ------------------------------------------------------------------------------------------------------------ the calls
def _dev(a, dtype):
    return torch.from_numpy(np.array(a, dtype=dtype)).to(DEV)     # (a copy: the shared cases are read only)


def run_components(faces, V):
    """tn_mesh_components through the C ABI, 64 guard bytes behind the workspace -> (labels, face_counts, stats) as numpy / tuple"""
    from tinynerf_amd import _lib as L
    dev = torch.device(DEV)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    F = faces.shape[0]
    f = _dev(faces, np.int32)
    nbytes = C.c_int64(0)
    L.call_plain("tn_mesh_components_workspace_bytes", C.c_int64(V), C.c_int64(F), C.byref(nbytes))
    work = torch.full((nbytes.value + 64,), 0x5A, dtype=torch.uint8, device=dev)
    labels = torch.full((V + TAIL,), SENTINEL_I, dtype=torch.int32, device=dev)
    counts = torch.full((V + TAIL,), SENTINEL_I, dtype=torch.int32, device=dev)
    stats = torch.full((3,), -1, dtype=torch.int64, device=dev)
    L.call("tn_mesh_components", dev, L.ptr(f) if F else None, C.c_int64(V), C.c_int64(F), L.ptr(labels), L.ptr(counts), L.ptr(stats), L.ptr(work))
    torch.cuda.synchronize()
    assert bool((work[nbytes.value:] == 0x5A).all()), "the workspace was overrun"
    assert bool((labels[V:] == SENTINEL_I).all()) and bool((counts[V:] == SENTINEL_I).all())
    return labels[:V].cpu().numpy(), counts[:V].cpu().numpy(), tuple(stats.tolist())


def run_filter(vert, nrm, rgb, faces, labels, face_counts, T, vcap, fcap, null_outputs=False, guard=(0, 64), spare=0):
    """tn_mesh_filter through the C ABI on sentinel-filled outputs with TAIL rows behind the capacities ->
    (counts, vertices, normals, colors, src, faces) as numpy, ALL allocated rows.  The workspace is
    tn_mesh_filter_workspace_bytes + `spare` bytes with `guard` bytes of a fixed pattern before and behind it."""
    from tinynerf_amd import _lib as L
    dev = torch.device(DEV)
    V, F = vert.shape[0], faces.shape[0]
    d_v, d_f, d_l, d_c = _dev(vert, np.float32), _dev(faces, np.int32), _dev(labels, np.int32), _dev(face_counts, np.int32)
    d_n = None if nrm is None else _dev(nrm, np.float32)
    d_rgb = None if rgb is None else _dev(rgb, np.uint8)
    nbytes = C.c_int64(0)
    L.call_plain("tn_mesh_filter_workspace_bytes", C.c_int64(V), C.c_int64(F), C.byref(nbytes))
    first, last = guard[0], guard[0] + nbytes.value + spare
    work = torch.full((last + guard[1],), 0x5A, dtype=torch.uint8, device=dev)
    o_v = torch.full((vcap + TAIL, 3), SENTINEL_F, dtype=torch.float32, device=dev)
    o_n = torch.full((vcap + TAIL, 3), SENTINEL_F, dtype=torch.float32, device=dev)
    o_c = torch.full((vcap + TAIL, 3), SENTINEL_B, dtype=torch.uint8, device=dev)
    o_s = torch.full((vcap + TAIL,), SENTINEL_I, dtype=torch.int32, device=dev)
    o_f = torch.full((fcap + TAIL, 3), SENTINEL_I, dtype=torch.int32, device=dev)
    counts = torch.full((2,), -1, dtype=torch.int64, device=dev)
    outs = (None,) * 5 if null_outputs else (L.ptr(o_v), L.ptr(o_n), L.ptr(o_c), L.ptr(o_s), L.ptr(o_f))
    L.call("tn_mesh_filter", dev, L.ptr(d_f) if F else None, L.ptr(d_l), L.ptr(d_c), C.c_int64(T), L.ptr(d_v), L.ptr(d_n), L.ptr(d_rgb),
           C.c_int64(V), C.c_int64(F), C.c_int64(vcap), C.c_int64(fcap), *outs, L.ptr(counts), L.ptr(work[first:]))
    torch.cuda.synchronize()
    assert bool((work[:first] == 0x5A).all()) and bool((work[last:] == 0x5A).all()), "the workspace was overrun"
    return tuple(counts.tolist()), o_v.cpu().numpy(), o_n.cpu().numpy(), o_c.cpu().numpy(), o_s.cpu().numpy(), o_f.cpu().numpy()


def attributes(V, seed=0):
    """positions, normals and colours with every row distinct -- and a NaN, a signed zero, a subnormal: rows are copied, not computed"""
    rng = np.random.default_rng([V, seed])
    vert, nrm = rng.standard_normal((V, 3)).astype(np.float32), rng.standard_normal((V, 3)).astype(np.float32)
    if V:
        vert[0], nrm[V - 1] = [np.nan, -0.0, np.float32(1e-42)], [np.inf, -0.0, np.nan]
    return vert, nrm, rng.integers(0, 256, (V, 3)).astype(np.uint8)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def check_components(faces, V):
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    want = ref.components(faces, V)
    labels, counts, stats = run_components(faces, V)
    assert stats == want[2], (stats, want[2])
    assert np.array_equal(labels, want[0]) and np.array_equal(counts, want[1])
    return want


def check_filter(vert, nrm, rgb, faces, want_components, T, caps="exact"):
    """one threshold at capacities exact / one short / 0: counts, src, faces, rows equal to the yardstick's first rows; the tail untouched"""
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    labels, face_counts, _ = want_components
    w_v, w_n, w_c, w_f, w_src, w_counts = ref.filter_mesh(vert, nrm, rgb, faces, T, labels, face_counts)
    nv, nf = w_counts
    vcap, fcap = {"exact": (nv, nf), "short": (max(nv - 1, 0), max(nf - 1, 0)), "zero": (0, 0)}[caps]
    counts, o_v, o_n, o_c, o_s, o_f = run_filter(vert, nrm, rgb, faces, labels, face_counts, T, vcap, fcap, null_outputs=caps == "zero")
    assert counts == w_counts, (T, caps, counts, w_counts)
    assert np.array_equal(o_s[:vcap], w_src[:vcap]) and np.array_equal(o_f[:fcap], w_f[:fcap]), (T, caps)
    assert np.array_equal(bits(o_v[:vcap]), bits(w_v[:vcap])), (T, caps)
    if nrm is not None:
        assert np.array_equal(bits(o_n[:vcap]), bits(w_n[:vcap])), (T, caps)
    if rgb is not None:
        assert np.array_equal(o_c[:vcap], w_c[:vcap]), (T, caps)
    keep_n, keep_c = (vcap if nrm is not None else 0), (vcap if rgb is not None else 0)            # an attribute not given is not written at all
    assert (o_v[vcap:] == np.float32(SENTINEL_F)).all() and (o_n[keep_n:] == np.float32(SENTINEL_F)).all() and (o_c[keep_c:] == SENTINEL_B).all(), (T, caps)
    assert (o_s[vcap:] == SENTINEL_I).all() and (o_f[fcap:] == SENTINEL_I).all(), (T, caps)
    return w_v, w_n, w_c, w_f, w_src, w_counts


def check_mesh(faces, V, thresholds, seed=0):
    vert, nrm, rgb = attributes(V, seed)
    want = check_components(faces, V)
    for T in thresholds:
        check_filter(vert, nrm, rgb, faces, want, T)
    return want


@pytest.mark.parametrize("V,F", [(1, 0), (5, 300), (300, 5), (257, 257)])
def test_the_filter_workspace_is_what_the_size_function_says(V, F):
    """V != F: the workgroup count is the larger one's, and the lanes past the shorter list still store ballots and counts -- inside
    the layout: a workspace of exactly tn_mesh_filter_workspace_bytes in the middle of a larger buffer leaves the bytes around it
    alone (`run_filter` asserts that) and gives the outputs of a generous one"""
    faces = np.random.default_rng([V, F]).integers(0, V, (F, 3)).astype(np.int32)
    vert, nrm, rgb = attributes(V)
    labels, face_counts, _ = ref.components(faces, V)
    for T in (0, 1):
        nv, nf = ref.filter_mesh(vert, nrm, rgb, faces, T, labels, face_counts)[5]
        tight = run_filter(vert, nrm, rgb, faces, labels, face_counts, T, nv, nf, guard=(256, 256))
        generous = run_filter(vert, nrm, rgb, faces, labels, face_counts, T, nv, nf, guard=(256, 256), spare=4096)
        assert tight[0] == (nv, nf), (T, tight[0])
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(tight[1:], generous[1:])), T


# ------------------------------------------------------------------------------------------------------------ tiny cases
TINY = {
    "V=1 F=0": (np.zeros((0, 3), np.int32), 1),
    "isolated vertices": (np.zeros((0, 3), np.int32), 7),
    "one triangle": ([[0, 1, 2]], 3),
    "one triangle among isolated vertices": ([[4, 1, 2]], 6),
    "two triangles sharing nothing": ([[0, 1, 2], [3, 4, 5]], 6),
    "two triangles sharing a vertex": ([[4, 1, 2], [2, 3, 0]], 5),
    "two triangles sharing an edge": ([[1, 2, 3], [3, 2, 4]], 5),
    "degenerate (a,a,b)": ([[3, 3, 1], [0, 0, 0], [2, 4, 2]], 6),
    "invalid -1, V, 2^31-1": ([[0, 1, 2], [2, 3, 5], [3, -1, 4], [3, 4, 2 ** 31 - 1], [-1, -1, -1], [4, 3, 3], [-2 ** 31, 0, 1]], 5),
}


@pytest.mark.parametrize("name", TINY)
def test_tiny_cases(name):
    faces, V = TINY[name]
    want = check_mesh(faces, V, (0, 1, 2, 3))
    if name == "invalid -1, V, 2^31-1":
        assert want[2] == (2, 2, 1) and want[0].tolist() == [0, 0, 0, 3, 3]
    for T in (0, 1):                                               # without normals / without colours / without both
        vert, nrm, rgb = attributes(V)
        check_filter(vert, None, rgb, faces, want, T)
        check_filter(vert, nrm, None, faces, want, T)
        check_filter(vert, None, None, faces, want, T)


def test_no_vertices():
    from tinynerf_amd import _lib as L
    dev = torch.device(DEV)
    stats = torch.full((3,), -1, dtype=torch.int64, device=dev)
    counts = torch.full((2,), -1, dtype=torch.int64, device=dev)
    bad = torch.full((4, 3), 9, dtype=torch.int32, device=dev)    # four faces over no vertices: all invalid
    for faces, F in ((None, 0), (bad, 4)):
        stats.fill_(-1), counts.fill_(-1)
        L.call("tn_mesh_components", dev, L.ptr(faces), C.c_int64(0), C.c_int64(F), None, None, L.ptr(stats), None)
        L.call("tn_mesh_filter", dev, L.ptr(faces), None, None, C.c_int64(0), None, None, None, C.c_int64(0), C.c_int64(F), C.c_int64(0), C.c_int64(0),
               None, None, None, None, None, L.ptr(counts), None)
        assert stats.tolist() == [0, 0, 0] and counts.tolist() == [0, 0]
    from tinynerf_amd import mesh as M
    e3 = torch.empty((0, 3), device=dev)
    assert M.components(bad, 0)[2] == (0, 0, 0)
    v, n, c, f, src = M.filter_components(e3, e3, None, bad, min_faces=1, return_src=True)
    assert v.shape == (0, 3) and n.shape == (0, 3) and c is None and f.shape == (0, 3) and src.shape == (0,)


# ------------------------------------------------------------------------------------------------------------ chains
def chain(order, n=5000):
    """a strip of n triangles over n + 2 vertices, triangle i = (p[i], p[i+1], p[i+2]) with p the ids in `order`"""
    V = n + 2
    p = {"ascending": np.arange(V), "descending": np.arange(V)[::-1], "permuted": np.random.default_rng(11).permutation(V)}[order]
    i = np.arange(n)
    return np.stack([p[i], p[i + 1], p[i + 2]], 1).astype(np.int32), V


@pytest.mark.parametrize("order", ["ascending", "descending", "permuted"])
def test_a_long_chain_ends_with_one_root(order):
    faces, V = chain(order)
    want = check_mesh(faces, V, (0, 5000, 5001))
    assert want[2] == (1, 1, 5000) and not want[0].any()


# ------------------------------------------------------------------------------------------------------------ many components
@functools.lru_cache(maxsize=None)
def disjoint_triangles(n, V):
    """n triangles over the first 3n of a fixed permutation of V ids (the rest isolated), the faces shuffled"""
    rng = np.random.default_rng([n, V])
    faces = rng.permutation(V)[:3 * n].reshape(n, 3).astype(np.int32)
    rng.shuffle(faces)
    faces.setflags(write=False)
    return faces


@pytest.mark.parametrize("n,V", [(EDGE // 3, EDGE - 1), (EDGE // 3, EDGE), (EDGE // 3 + 1, EDGE + 2),                    # vertices around the edge
                                 (EDGE - 1, 3 * EDGE - 3), (EDGE, 3 * EDGE), (EDGE + 1, 3 * EDGE + 3)])                  # faces around the edge
def test_many_components_around_the_scan_trip_edge(n, V):
    faces = disjoint_triangles(n, V)
    want = check_components(faces, V)
    assert want[2] == (V - 2 * n, n, 1)
    vert, nrm, rgb = attributes(V)
    assert check_filter(vert, nrm, rgb, faces, want, 1)[5] == (3 * n, n)            # the isolated vertices go
    assert check_filter(vert, None, None, faces, want, 0)[5] == (V, n)
    assert check_filter(vert, None, None, faces, want, 2)[5] == (0, 0)


def test_a_mix_of_component_sizes_filtered_at_several_thresholds():
    strips, first = [], 0
    for _ in range(4):
        for k in range(1, 51):                                     # a strip of k triangles over k + 2 vertices
            i = first + np.arange(k)
            strips.append(np.stack([i, i + 1, i + 2], 1))
            first += k + 2
    V = first + 9                                                  # and nine isolated vertices
    rng = np.random.default_rng(5)
    faces = rng.permutation(V)[np.concatenate(strips)].astype(np.int32)
    rng.shuffle(faces)
    vert, nrm, rgb = attributes(V)
    want = check_components(faces, V)
    assert want[2] == (200 + 9, 200, 50)
    kept = {T: check_filter(vert, nrm, rgb, faces, want, T)[5] for T in (0, 1, 2, 25, 50, 51)}
    assert kept[0] == (V, 5100) and kept[1] == (V - 9, 5100) and kept[2] == (V - 9 - 4 * 3, 5100 - 4)
    assert kept[25] == (4 * sum(k + 2 for k in range(25, 51)), 4 * sum(range(25, 51))) and kept[50] == (4 * 52, 200) and kept[51] == (0, 0)


# ------------------------------------------------------------------------------------------------------------ Surface Nets meshes
DIMS = (32, 32, 32)                                                # 33 x 33 x 33 nodes
BIG, SMALL = ([0.42, -0.05, 0.45], 0.36), ([-0.45, 0.1, -0.4], 0.25)


def _sphere(s, centre, radius):
    return radius - np.linalg.norm(s - np.float64(centre), axis=-1)


@functools.lru_cache(maxsize=None)
def field(name):
    """float32 node values [33,33,33], level 0: `big` / `small` -- one sphere alone; `spheres` -- both; `specks` -- both and 40 single
    nodes set above the level, each at least 3 cells from either sphere, from the box and from one another; `plane` -- tilted,
    reaching the box"""
    lo, h = mref.grid(DIMS)
    x = mref.node_positions(DIMS, lo, h)
    s = mref._unit(x, (-1.0, -0.75, -1.25), (1.0, 0.75, 1.25))
    if name == "plane":
        f = s @ np.float64([0.3, 0.5, -0.4]) + 0.013
    elif name in ("big", "small"):
        f = _sphere(s, *(BIG if name == "big" else SMALL))
    else:
        f = np.maximum(_sphere(s, *BIG), _sphere(s, *SMALL))
        if name == "specks":
            rng = np.random.default_rng(3)
            taken = np.zeros(f.shape, bool)
            placed = 0
            for k, j, i in rng.integers(3, 30, (4000, 3)).tolist():
                if placed < 40 and f[k - 3:k + 4, j - 3:j + 4, i - 3:i + 4].max() < 0 and not taken[k - 3:k + 4, j - 3:j + 4, i - 3:i + 4].any():
                    taken[k, j, i] = True
                    placed += 1
            assert placed == 40
            f = np.where(taken, 0.05, f)
    f = f.astype(np.float32)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def surface(name, half=False):
    """(vertices, normals, colours, faces) as numpy: mesh.extract on the device; `half`: extract(capacity=(V // 2, F)) -- the faces
    still name the full mesh's vertices, so about half of them are invalid"""
    from tinynerf_amd import mesh as M
    lo, h = mref.grid(DIMS)
    values = torch.from_numpy(np.array(field(name))).to(DEV)
    v, n, f = M.extract(values, lo, h, 0.0)
    if half:
        v, n, f = M.extract(values, lo, h, 0.0, capacity=(v.size(0) // 2, f.size(0)))
    out = (v.cpu().numpy(), n.cpu().numpy(), attributes(v.size(0))[2], f.cpu().numpy())
    for a in out:
        a.setflags(write=False)
    return out


def closed_pieces(faces, V):
    """[(vertices, faces)] of every component with a face, after asserting each closed, consistently oriented and of Euler number 2"""
    out = []
    for f in ref.pieces(faces, V).values():
        twice, paired, edges = mref.edge_report(f)
        n_v = np.unique(f).size
        assert twice and paired and n_v - edges + f.shape[0] == 2
        out.append((n_v, f.shape[0]))
    return sorted(out)


@pytest.mark.parametrize("name,half", [("spheres", False), ("specks", False), ("plane", False), ("specks", True)])
def test_surface_nets_meshes_against_the_yardstick(name, half):
    vert, nrm, rgb, faces = surface(name, half)
    V = vert.shape[0]
    want = check_components(faces, V)
    largest = want[2][2]
    if half:
        invalid = int((~ref.valid_faces(faces, V)).sum())
        assert 0.3 * faces.shape[0] < invalid < 0.7 * faces.shape[0]
    for T in (0, 1, 13, largest, largest + 1):
        got = check_filter(vert, nrm, rgb, faces, want, T)
        if T == 0 and not half:                                    # the identity, bit for bit
            assert np.array_equal(bits(got[0]), bits(vert)) and np.array_equal(bits(got[1]), bits(nrm)) and np.array_equal(got[2], rgb)
            assert np.array_equal(got[3], faces) and np.array_equal(got[4], np.arange(V))
    if name == "spheres":
        assert want[2][:2] == (2, 2)
    if name == "plane":
        assert want[2] == (1, 1, faces.shape[0])


def test_floaters_leave_and_the_spheres_stay():
    from tinynerf_amd import mesh as M
    vert, nrm, rgb, faces = surface("specks")
    big, small = surface("big"), surface("small")
    n_big, n_small = big[3].shape[0], small[3].shape[0]
    want = ref.components(faces, vert.shape[0])
    assert want[2] == (42, 42, n_big) and n_small < n_big and sorted(want[1][want[1] > 0].tolist()) == [12] * 40 + [n_small, n_big]
    dv, dn, dc, df = (torch.from_numpy(np.array(a)).to(DEV) for a in (vert, nrm, rgb, faces))
    # keep_fraction = 1: the larger sphere's mesh, as extracting that sphere alone gives it
    v, n, c, f, src = M.filter_components(dv, dn, dc, df, keep_fraction=1.0, return_src=True)
    assert np.array_equal(bits(v.cpu().numpy()), bits(big[0])) and np.array_equal(bits(n.cpu().numpy()), bits(big[1])) and np.array_equal(f.cpu().numpy(), big[3])
    w = ref.filter_mesh(vert, nrm, rgb, faces, n_big)
    assert np.array_equal(src.cpu().numpy(), w[4]) and np.array_equal(c.cpu().numpy(), w[2]) and np.array_equal(f.cpu().numpy(), w[3])
    assert closed_pieces(f.cpu().numpy(), v.size(0)) == [(big[0].shape[0], n_big)]
    # min_faces = the smaller sphere's count: both spheres, no speck
    v, n, c, f = M.filter_components(dv, dn, None, df, min_faces=n_small)
    assert c is None and closed_pieces(f.cpu().numpy(), v.size(0)) == sorted([(small[0].shape[0], n_small), (big[0].shape[0], n_big)])
    w = ref.filter_mesh(vert, nrm, None, faces, n_small)
    assert np.array_equal(bits(v.cpu().numpy()), bits(w[0])) and np.array_equal(bits(n.cpu().numpy()), bits(w[1])) and np.array_equal(f.cpu().numpy(), w[3])
    # both options: the larger threshold wins; one face more than the largest component has: nothing
    assert M.filter_components(dv, None, None, df, min_faces=n_small, keep_fraction=1.0)[3].size(0) == n_big
    assert M.filter_components(dv, None, None, df, min_faces=n_big + 1)[0].shape == (0, 3)
    # every piece of the unfiltered mesh is closed too: 40 specks of 8 vertices and 12 faces
    assert closed_pieces(faces, vert.shape[0])[:40] == [(8, 12)] * 40
    labels, face_counts, stats = M.components(df, vert.shape[0])
    assert stats == want[2] and labels.dtype == face_counts.dtype == torch.int32
    assert np.array_equal(labels.cpu().numpy(), want[0]) and np.array_equal(face_counts.cpu().numpy(), want[1])


@pytest.mark.parametrize("caps", ["exact", "short", "zero"])
def test_capacities(caps):
    vert, nrm, rgb, faces = surface("specks")
    want = ref.components(faces, vert.shape[0])
    for T in (0, 13, want[2][2]):
        check_filter(vert, nrm, rgb, faces, want, T, caps)
    # one side alone: vertices without faces, faces without vertices (the other outputs NULL with their capacity 0)
    if caps == "exact":
        from tinynerf_amd import _lib as L
        w = ref.filter_mesh(vert, nrm, rgb, faces, 13, *want[:2])
        full = run_filter(vert, nrm, rgb, faces, want[0], want[1], 13, *w[5])
        v_only = run_filter(vert, nrm, rgb, faces, want[0], want[1], 13, w[5][0], 0)
        f_only = run_filter(vert, None, None, faces, want[0], want[1], 13, 0, w[5][1])
        assert v_only[0] == f_only[0] == w[5]
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(v_only[1:5], full[1:5])) and (v_only[5] == SENTINEL_I).all()
        assert np.array_equal(f_only[5], full[5]) and (f_only[4] == SENTINEL_I).all() and (f_only[1] == np.float32(SENTINEL_F)).all()


def test_two_calls_give_the_same_bytes():
    for faces, V in (chain("permuted"), (surface("specks")[3], surface("specks")[0].shape[0])):
        vert, nrm, rgb = attributes(V)
        runs = []
        for _ in range(2):
            labels, counts, stats = run_components(faces, V)
            out = run_filter(vert, nrm, rgb, faces, labels, counts, 13, V, faces.shape[0])
            runs.append((labels, counts, np.int64(stats), np.int64(out[0])) + out[1:])
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(*runs))


# ------------------------------------------------------------------------------------------------------------ end to end
def _scene_on_disk(root):
    """the 48 x 48 synthetic ball in Blender format: three training views, the first of them as the test split"""
    from PIL import Image
    from tinynerf_amd import rays
    o, d, rgb, K, cams = rays.synthetic_scene(n_views=3, res=48, seed=5, device="cpu")
    imgs = (rgb.reshape(3, 48, 48, 3) * 255).to(torch.uint8).numpy()
    (root / "train").mkdir()
    frames = []
    for i in range(3):
        Image.fromarray(imgs[i]).save(root / "train" / f"r_{i}.png")
        frames.append({"file_path": f"./train/r_{i}", "transform_matrix": cams[i].tolist()})
    for split in ("train", "test"):
        json.dump({"camera_angle_x": 0.6911112070083618, "frames": frames[:3 if split == "train" else 1]},
                  open(root / f"transforms_{split}.json", "w"))


def test_export_clean_mesh_and_train_end_to_end(tmp_path):
    from tinynerf_amd import data, mesh as M
    from tinynerf_amd.run import TrainConfig, train
    _scene_on_disk(tmp_path)
    dev = torch.device(DEV)
    train_rays = data.RaysDataset(data.parse_nerf_synthetic(tmp_path, "train"), dev)
    test_set = data.PoseDataset(data.parse_nerf_synthetic(tmp_path, "test"), dev)

    def go(name, **more):
        out = tmp_path / name
        out.mkdir()
        cfg = TrainConfig(method="kplanes", batch_size=512, n_samples=64, occupancy_res=32, seed=3, kplanes_resolutions=(16, 32, 64))
        return out, train(cfg, train_rays, None, test_set, out, max_steps=20, log_every=50, **more)[0]

    out, tr = go("plain")
    # both options 0: export_mesh's file, byte for byte
    a = M.export_mesh(tr, out / "a.ply", resolution=24)
    b = M.export_clean_mesh(tr, out / "b.ply", resolution=24)
    assert open(out / "a.ply", "rb").read() == open(out / "b.ply", "rb").read() and all(torch.equal(x, y) for x, y in zip(a, b))
    # a level low enough that the young model's surface has several pieces
    from tinynerf_amd.points import default_crop
    crop = default_crop(tr.cfg)
    lo, h, dims = M.grid_dims(crop, 24)
    values = M.density_grid(tr, crop, dims)[0]
    level = None
    for q in (0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.98):
        sigma = float(torch.exp(values.flatten().float().kthvalue(int(q * values.numel())).values))
        v, n, f = M.extract(values, lo, h, float(np.log(sigma)))
        stats = M.components(f, v.size(0))[2]
        print(f"quantile {q}: sigma {sigma:.4g}, {v.size(0)} vertices, {f.size(0)} faces, components {stats}")
        if stats[1] >= 2:
            level = sigma
            break
    if level is None:
        pytest.skip("the model trained for 20 steps has fewer than two components with a face at every level tried")
    v, n, c, f = (t.cpu().numpy() for t in M.export_mesh(tr, out / "full.ply", resolution=24, level=level))
    kept = M.export_clean_mesh(tr, out / "clean.ply", resolution=24, level=level, keep_fraction=1.0)
    got = M.read_mesh_ply(out / "clean.ply")
    labels, face_counts, stats = ref.components(f, v.shape[0])
    w_v, w_n, _, w_f, w_src, w_counts = ref.filter_mesh(v, n, c, f, stats[2], labels, face_counts)
    assert 0 < w_counts[0] < v.shape[0] and 0 < w_counts[1] < f.shape[0]
    assert np.array_equal(bits(got[0]), bits(w_v)) and np.array_equal(bits(got[1]), bits(w_n)) and np.array_equal(got[3], w_f)
    colours = M.vertex_colors(tr, torch.from_numpy(w_v).to(dev), torch.from_numpy(w_n).to(dev)).cpu().numpy()
    assert np.array_equal(got[2], colours) and np.array_equal(kept[2].cpu().numpy(), colours)
    print(f"kept {w_counts} of {(v.shape[0], f.shape[0])}; colours equal to the unfiltered export's rows: {np.array_equal(colours, c[w_src])}")
    sizes = [p.shape[0] for p in ref.pieces(got[3], got[0].shape[0]).values()]
    assert sizes and all(s == stats[2] for s in sizes)             # the largest piece alone (ties all kept)
    # min_faces through the same path; no colours
    m = M.export_clean_mesh(tr, None, resolution=24, level=level, min_faces=stats[2], colors=False)
    assert torch.equal(m[0], kept[0]) and torch.equal(m[3], kept[3]) and not m[2].any()
    # train(): the keywords reach export_clean_mesh; one of them alone is enough
    out2, _ = go("clean", mesh=24, mesh_level=level, mesh_keep_fraction=1.0)
    vert2, _, _, faces2 = M.read_mesh_ply(out2 / "mesh.ply")
    sizes = [p.shape[0] for p in ref.pieces(faces2, vert2.shape[0]).values()]
    assert len(set(sizes)) <= 1 and (not sizes or np.unique(faces2).size == vert2.shape[0])      # one size of piece, no vertex outside a face
