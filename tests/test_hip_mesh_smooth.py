"""GPU tests of the mesh smoothing: tn_mesh_adjacency, tn_mesh_smooth_pass, tn_mesh_smooth and tn_mesh_vertex_normals
through the C ABI against tests/_mesh_smooth_ref.py -- the adjacency for equality, passes and normals within the per-element fp32
bounds of the float64 restatement applied to the device's own fp32 input --, on tiny meshes, a fan of degree 1 000, invalid rows,
Surface Nets meshes, strips around the scan's trip edge, and the exporters / train(mesh_smooth=...) end to end.

Largest observed error over bound (MI355X): see DESIGN 6l."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

import _mesh_ref as mref
import _mesh_smooth_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL_F, SENTINEL_I, SENTINEL_B, TAIL = -7.25, -12345, 0xA5, 5
EDGE = 256 * 1024                                                  # 1024 workgroups of 256: the scan's trip edge
TETRA = np.int32([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]])


# ------------------------------------------------------------------------------------------------------------ the calls
def _dev(a, dtype):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(DEV)     # (a C-ordered copy: the shared cases are read only, the yardstick's faces strided)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def run_adjacency(faces, V, fill=0x5A, guard=64):
    """tn_mesh_adjacency through the C ABI on sentinel-filled outputs with TAIL rows behind them, `guard` bytes of `fill` before and
    behind a workspace filled with `fill` -> (offsets [V+1], pairs ALL 3F + TAIL rows, pinned [V], stats) as numpy / tuple"""
    from tinynerf_amd import _lib as L
    dev = torch.device(DEV)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    F = faces.shape[0]
    f = _dev(faces, np.int32)
    nbytes = C.c_int64(0)
    L.call_plain("tn_mesh_adjacency_workspace_bytes", C.c_int64(V), C.c_int64(F), C.byref(nbytes))
    work = torch.full((guard + nbytes.value + guard,), fill, dtype=torch.uint8, device=dev)
    offsets = torch.full((V + 1 + TAIL,), SENTINEL_I, dtype=torch.int32, device=dev)
    pairs = torch.full((3 * F + TAIL, 2), SENTINEL_I, dtype=torch.int32, device=dev)
    pinned = torch.full((V + TAIL,), SENTINEL_B, dtype=torch.uint8, device=dev)
    stats = torch.full((3,), -1, dtype=torch.int64, device=dev)
    L.call("tn_mesh_adjacency", dev, L.ptr(f) if F else None, C.c_int64(V), C.c_int64(F), L.ptr(offsets), L.ptr(pairs), L.ptr(pinned), L.ptr(stats),
           L.ptr(work[guard:]))
    torch.cuda.synchronize()
    assert bool((work[:guard] == fill).all()) and bool((work[guard + nbytes.value:] == fill).all()), "the workspace was overrun"
    if V:
        assert bool((offsets[V + 1:] == SENTINEL_I).all()) and bool((pinned[V:] == SENTINEL_B).all())
    return offsets[:V + 1].cpu().numpy(), pairs.cpu().numpy(), pinned[:V].cpu().numpy(), tuple(stats.tolist())


def check_adjacency(faces, V):
    """equality with the yardstick, rows beyond offsets[V] untouched, and the same bytes from a workspace pre-filled with other bytes"""
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    want = ref.adjacency(faces, V)
    got = run_adjacency(faces, V)
    again = run_adjacency(faces, V, fill=0xC3)
    assert got[3] == want[3], (got[3], want[3])
    if V == 0:
        return want
    n = int(want[0][V])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1][:n], want[1]) and np.array_equal(got[2], want[2])
    assert (got[1][n:] == SENTINEL_I).all(), "pairs beyond offsets[V] were written"
    assert all(np.array_equal(a, b) for a, b in zip(got[:3], again[:3])) and got[3] == again[3]
    return want


class Device:
    """a mesh's adjacency (the yardstick's, uploaded) and fp32 positions on the device, for the pass / smooth / normals calls"""

    def __init__(self, positions, faces, V=None):
        self.p = np.ascontiguousarray(positions, np.float32)
        self.V = self.p.shape[0] if V is None else V
        self.faces = np.asarray(faces, np.int32).reshape(-1, 3)
        self.offsets, self.pairs, self.pinned, self.stats = ref.adjacency(self.faces, self.V)
        self.d_p, self.d_off = _dev(self.p, np.float32), _dev(self.offsets, np.int32)
        self.d_pairs = _dev(np.concatenate([self.pairs, np.full((1, 2), SENTINEL_I, np.int32)]), np.int32)
        self.d_pin = _dev(self.pinned, np.uint8)

    def out(self):
        return torch.full((self.V + TAIL, 3), SENTINEL_F, dtype=torch.float32, device=DEV)

    def done(self, o):
        torch.cuda.synchronize()
        assert bool((o[self.V:] == SENTINEL_F).all()), "rows behind the output were written"
        return o[:self.V].cpu().numpy()

    def one_pass(self, src, f, pin=True):
        from tinynerf_amd import _lib as L
        o = self.out()
        L.call("tn_mesh_smooth_pass", torch.device(DEV), L.ptr(src), L.ptr(self.d_off), L.ptr(self.d_pairs), L.ptr(self.d_pin) if pin else None,
               C.c_int64(self.V), C.c_float(f), L.ptr(o))
        return o

    def smooth(self, N, lam=ref.LAMBDA, mu=ref.MU, pin=True):
        from tinynerf_amd import _lib as L
        o, scratch = self.out(), self.out()
        L.call("tn_mesh_smooth", torch.device(DEV), L.ptr(self.d_p), L.ptr(self.d_off), L.ptr(self.d_pairs), L.ptr(self.d_pin) if pin else None,
               C.c_int64(self.V), C.c_int32(N), C.c_float(lam), C.c_float(mu), L.ptr(scratch), L.ptr(o))
        torch.cuda.synchronize()
        assert bool((scratch[self.V:] == SENTINEL_F).all())
        return self.done(o)

    def normals(self, fallback=None):
        from tinynerf_amd import _lib as L
        o = self.out()
        fb = None if fallback is None else _dev(fallback, np.float32)
        L.call("tn_mesh_vertex_normals", torch.device(DEV), L.ptr(self.d_p), L.ptr(self.d_off), L.ptr(self.d_pairs), C.c_int64(self.V), L.ptr(fb), L.ptr(o))
        return self.done(o)


@functools.lru_cache(maxsize=None)
def surface(name, dims=(16, 16, 16)):
    """(vertices float32, normals float32, faces int32) of the yardstick's Surface Nets mesh of a field: computed once, read only"""
    want = mref.case(name, dims)[4]
    out = want["vertices"].astype(np.float32), want["normals"].astype(np.float32), want["faces"]
    for a in out:
        a.setflags(write=False)
    return out


def binary():
    v, n, f = ref.binary_sphere()
    return v.astype(np.float32), n.astype(np.float32), f


# ------------------------------------------------------------------------------------------------------------ adjacency
TINY = {
    "one triangle": ([[0, 1, 2]], 3),
    "one triangle among isolated vertices": ([[4, 1, 2]], 6),
    "a tetrahedron": (TETRA, 4),
    "two triangles on an edge": ([[1, 2, 3], [3, 2, 4]], 5),
    "three triangles on one edge": ([[0, 1, 2], [0, 1, 3], [0, 1, 4]], 5),
    "a face twice": (np.concatenate([TETRA, TETRA[:1]]), 4),
    "-1 rows, out of range, repeated": ([[0, 1, 2], [2, 3, 5], [3, -1, 4], [3, 4, 2 ** 31 - 1], [-1, -1, -1], [4, 3, 3], [0, 0, 0], [2, 4, 2],
                                         [-2 ** 31, 0, 1], [1, 0, 2], [3, 4, 0]], 5),
    "isolated vertices": (np.zeros((0, 3), np.int32), 7),
    "V=1 F=0": (np.zeros((0, 3), np.int32), 1),
    "only invalid faces": ([[0, 0, 1], [-1, -1, -1], [5, 6, 7]], 3),
}


@pytest.mark.parametrize("name", TINY)
def test_adjacency_tiny_cases(name):
    faces, V = TINY[name]
    want = check_adjacency(faces, V)
    if name == "a tetrahedron":
        assert want[3] == (4, 4, 3) and not want[2].any()
    if name == "three triangles on one edge":
        assert want[2].all()
    if name in ("isolated vertices", "V=1 F=0", "only invalid faces"):
        assert want[2].all() and want[3] == (0, 0, 0) and not want[0].any()


def test_adjacency_no_vertices():
    from tinynerf_amd import _lib as L, mesh as M
    dev = torch.device(DEV)
    stats = torch.full((3,), -1, dtype=torch.int64, device=dev)
    bad = torch.full((4, 3), 9, dtype=torch.int32, device=dev)    # four faces over no vertices: none takes part
    for faces, F in ((None, 0), (bad, 4)):
        stats.fill_(-1)
        L.call("tn_mesh_adjacency", dev, L.ptr(faces), C.c_int64(0), C.c_int64(F), None, None, None, L.ptr(stats), None)
        assert stats.tolist() == [0, 0, 0]
    offsets, pairs, pinned, st = M.adjacency(bad, 0)
    assert offsets.tolist() == [0] and pinned.numel() == 0 and st == (0, 0, 0)
    e3 = torch.empty((0, 3), device=dev)
    v, n = M.smooth_mesh(e3, e3, bad, 2)
    assert v.shape == (0, 3) and n.shape == (0, 3)


def test_adjacency_of_a_fan_of_1000_faces():
    faces, V = ref.fan(1000)
    want = check_adjacency(faces, V)
    assert want[3] == (1000, 1, 1000) and want[2].tolist() == [0] + [1] * 1000
    # the same fan with its faces shuffled, and closed into a double cone: every vertex free, two hubs of degree 1000
    rng = np.random.default_rng(4)
    check_adjacency(faces[rng.permutation(1000)], V)
    other = faces[:, [0, 2, 1]].copy()
    other[:, 0] = V
    want = check_adjacency(np.concatenate([faces, other])[rng.permutation(2000)], V + 1)
    assert want[3] == (2000, 1002, 1000)


@pytest.mark.parametrize("dims", [(16, 16, 16), (17, 9, 33)])
@pytest.mark.parametrize("name", ["sphere", "torus", "two_spheres", "plane", "noise"])
def test_adjacency_of_surface_nets_meshes(name, dims):
    vert, _, faces = surface(name, dims)
    want = check_adjacency(faces, vert.shape[0])
    if name in mref.CLOSED:
        assert want[3][:2] == (faces.shape[0], vert.shape[0]) and want[3][2] <= 12      # closed: nothing pinned


@pytest.mark.parametrize("V", [EDGE, EDGE + 1])
def test_adjacency_of_a_strip_around_the_scans_trip_edge(V):
    faces, V = ref.strip(V)
    want = check_adjacency(faces, V)
    assert want[3] == (V - 2, 0, 3) and int(want[0][V]) == 3 * (V - 2)


def test_the_host_layer_returns_the_same_adjacency():
    from tinynerf_amd import mesh as M
    vert, _, faces = surface("noise")
    want = ref.adjacency(faces, vert.shape[0])
    offsets, pairs, pinned, stats = M.adjacency(_dev(faces, np.int32), vert.shape[0])
    assert stats == want[3] and pairs.shape == (3 * faces.shape[0], 2)
    assert np.array_equal(offsets.cpu().numpy(), want[0]) and np.array_equal(pairs.cpu().numpy()[:want[0][-1]], want[1])
    assert np.array_equal(pinned.cpu().numpy(), want[2])


# ------------------------------------------------------------------------------------------------------------ one pass
def pass_cases():
    """(name, positions, faces): Surface Nets meshes (closed, open, noise), the fan with isolated vertices, a NaN row and a signed zero"""
    out = [(n, surface(n)[0], surface(n)[2]) for n in ("sphere", "plane", "noise")] + [("torus 17x9x33", surface("torus", (17, 9, 33))[0], surface("torus", (17, 9, 33))[2])]
    faces, V = ref.fan(1000)
    rng = np.random.default_rng(7)
    p = rng.standard_normal((V + 3, 3)).astype(np.float32) * 3
    p[5], p[V + 1], p[V] = [np.nan, 1.0, -0.0], [np.nan, -0.0, np.float32(1e-42)], [-0.0, np.inf, 2.0]     # a rim vertex; two isolated ones
    out.append(("fan 1000 + isolated", p, faces))
    return out


@pytest.mark.parametrize("pin", [True, False])
@pytest.mark.parametrize("f", [0.5, -0.53])
def test_one_pass_against_float64(f, pin):
    worst = 0.0
    for name, p, faces in pass_cases():
        m = Device(p, faces)
        got = m.done(m.one_pass(m.d_p, f, pin))
        want, bound = ref.smooth_pass(m.p, m.offsets, m.pairs, m.pinned if pin else None, np.float64(np.float32(f)))
        move = ref.moves(m.offsets, m.pinned if pin else None)
        assert np.array_equal(bits(got[~move]), bits(m.p[~move])), name                               # not moved: bit for bit, NaN and -0 included
        err = np.abs(got[move].astype(np.float64) - want[move])
        fin = np.isfinite(want[move])
        assert np.array_equal(np.isnan(got[move]), np.isnan(want[move])), name                        # NaN propagates, and only where it must
        ratio = float((err[fin] / np.maximum(bound[move][fin], 1e-300)).max()) if fin.any() else 0.0
        print(f"pass f={f} pinned={pin} {name}: {int(move.sum())} of {m.V} move, largest error / bound {ratio:.3f}")
        assert (err[fin] <= bound[move][fin]).all(), (name, ratio)
        worst = max(worst, ratio)
    print(f"largest error over bound, f={f} pinned={pin}: {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------ tn_mesh_smooth
@pytest.mark.parametrize("N", [0, 1, 2, 5])
def test_smooth_is_the_chained_passes_bit_for_bit(N):
    for name, p, faces in pass_cases()[1:]:
        for pin in (True, False):
            m = Device(p, faces)
            x = m.d_p
            for _ in range(N):
                x = m.one_pass(x, ref.LAMBDA, pin)[:m.V].contiguous()
                x = m.one_pass(x, ref.MU, pin)[:m.V].contiguous()
            torch.cuda.synchronize()
            assert np.array_equal(bits(m.smooth(N, pin=pin)), bits(x.cpu().numpy())), (name, pin)


def test_smooth_ten_iterations_within_the_carried_bound_and_the_sphere_keeps_its_volume():
    from tinynerf_amd import mesh as M
    lam, mu = np.float64(np.float32(ref.LAMBDA)), np.float64(np.float32(ref.MU))
    for name, p, faces in [("binary sphere", binary()[0], binary()[2])] + pass_cases()[:4]:
        m = Device(p, faces)
        got = m.smooth(10)
        want, bound = ref.taubin(m.p, m.offsets, m.pairs, m.pinned, 10, lam, mu)
        err = np.abs(got.astype(np.float64) - want)
        print(f"smooth N=10 {name}: largest error {err.max():.3e}, largest error / carried bound {float((err / np.maximum(bound, 1e-300)).max()):.4f}")
        assert (err <= bound).all(), name
        assert np.array_equal(bits(got[m.pinned == 1]), bits(m.p[m.pinned == 1])), name
        if name == "binary sphere":
            ratio = ref.radial_std(got, ref.BINARY_CENTRE) / ref.radial_std(m.p, ref.BINARY_CENTRE)
            v0, v1 = mref.signed_volume(m.p, faces), mref.signed_volume(got, faces)
            print(f"  radial std ratio {ratio:.3f}, volume {v0:.4f} -> {v1:.4f}")
            assert ratio < 0.8 and abs(v1 - v0) / v0 < 0.02
            # the host layer: the same bytes, with and without a prebuilt adjacency; pin_boundary=False is the same on a closed mesh
            dv, df = _dev(m.p, np.float32), _dev(faces, np.int32)
            adj = M.adjacency(df, m.V)
            for out in (M.smooth(dv, df, 10), M.smooth(dv, df, 10, adjacency=adj), M.smooth(dv, df, 10, pin_boundary=False)):
                assert np.array_equal(bits(out.cpu().numpy()), bits(got))
            assert M.smooth(dv, df, 0) is dv


# ------------------------------------------------------------------------------------------------------------ normals
@pytest.mark.parametrize("name", ["sphere", "torus", "two_spheres", "plane", "noise", "binary sphere", "binary sphere smoothed"])
def test_vertex_normals_against_float64(name):
    if name.startswith("binary"):
        p, extractor, faces = binary()
    else:
        p, extractor, faces = surface(name)
    m = Device(p, faces)
    if name.endswith("smoothed"):
        m = Device(m.smooth(10), faces)
    fallback = np.random.default_rng(1).standard_normal((m.V, 3)).astype(np.float32)
    got = m.normals(fallback)
    want, g, bound = ref.vertex_normals(m.p, m.offsets, m.pairs, fallback)
    taken = np.isinf(bound)                                        # the fallback row: d == 0 or |g| == 0
    assert np.array_equal(bits(got[taken]), bits(fallback[taken]))
    checked = ~taken & (bound <= 1e-3)
    err = np.abs(got.astype(np.float64) - want).max(1)
    print(f"normals {name}: {int(checked.sum())} of {m.V} rows checked, {int(taken.sum())} fallback, largest error / bound "
          f"{float((err[checked] / bound[checked]).max()) if checked.any() else 0.0:.3f}")
    assert (err[checked] <= bound[checked]).all()
    if name in ("sphere", "torus", "two_spheres"):
        assert checked.all()                                       # no row may be skipped
    if name in ("sphere", "binary sphere", "binary sphere smoothed"):
        assert (np.einsum("ij,ij->i", got.astype(np.float64), extractor.astype(np.float64)) > 0).all()
    assert np.array_equal(bits(m.normals(None)[~taken]), bits(got[~taken])) and not m.normals(None)[taken].any()


def test_vertex_normals_fall_back_without_faces_and_on_a_fan_of_zero_area():
    from tinynerf_amd import mesh as M
    faces, V = ref.fan(6)
    p = np.zeros((V + 2, 3), np.float32)
    p[:, 0] = np.arange(V + 2)                                     # all on one line: every cross product is 0; two isolated vertices
    fallback = np.arange(3 * (V + 2), dtype=np.float32).reshape(-1, 3) - 4
    m = Device(p, faces)
    assert np.array_equal(bits(m.normals(fallback)), bits(fallback)) and not m.normals(None).any()
    p2 = p.copy()
    p2[1:V + 1, 1], p2[1:V + 1, 2] = np.cos(np.arange(V)), np.sin(np.arange(V))      # now the fan has area; the isolated two still fall back
    m = Device(p2, faces)
    got = m.normals(fallback)
    assert np.array_equal(got[V:], fallback[V:]) and np.allclose(np.linalg.norm(got[:V], axis=1), 1, atol=1e-6)
    n = M.vertex_normals(_dev(p2, np.float32), _dev(faces, np.int32), fallback=_dev(fallback, np.float32))
    assert np.array_equal(bits(n.cpu().numpy()), bits(got))
    v, n2 = M.smooth_mesh(_dev(p2, np.float32), _dev(fallback, np.float32), _dev(faces, np.int32), 0)
    assert np.array_equal(bits(n2.cpu().numpy()), bits(got)) and np.array_equal(bits(v.cpu().numpy()), bits(p2))


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


def _datasets(root):
    from tinynerf_amd import data
    _scene_on_disk(root)
    dev = torch.device(DEV)
    return data.RaysDataset(data.parse_nerf_synthetic(root, "train"), dev), data.PoseDataset(data.parse_nerf_synthetic(root, "test"), dev)


def _trainer(root, train_rays, test_set, name, steps, **more):
    from tinynerf_amd.run import TrainConfig, train
    out = root / name
    out.mkdir()
    cfg = TrainConfig(method="kplanes", batch_size=512, n_samples=64, occupancy_res=32, seed=3, kplanes_resolutions=(16, 32, 64))
    return out, train(cfg, train_rays, None, test_set, out, max_steps=steps, log_every=1000, **more)[0]


def check_smoothed_export(plain, smoothed, path, iterations=3):
    """a smoothing export against the plain one: faces and colours unchanged, positions smooth(...) of the plain ones, normals those of
    the smoothed faces with the plain ones as fallback, the PLY a round trip; returns the number of vertices that moved"""
    from tinynerf_amd import mesh as M
    assert plain[0].size(0) > 0 and plain[3].size(0) > 0
    assert torch.equal(plain[3], smoothed[3]) and torch.equal(plain[2], smoothed[2])
    moved = M.smooth(plain[0], plain[3], iterations)
    assert torch.equal(moved, smoothed[0])
    assert torch.equal(M.vertex_normals(moved, plain[3], fallback=plain[1]), smoothed[1])
    got = M.read_mesh_ply(path)
    for x, y in zip(got, smoothed):
        assert np.array_equal(bits(x), bits(y.cpu().numpy()))
    n = int((moved != plain[0]).any(1).sum())
    print(f"{path.name}: {plain[0].size(0)} vertices, {plain[3].size(0)} faces, {n} moved")
    assert n > 0
    return n


def test_density_exports_and_train_end_to_end(tmp_path):
    from tinynerf_amd import mesh as M
    from tinynerf_amd.points import default_crop
    from tinynerf_amd.run import TrainConfig, train
    train_rays, test_set = _datasets(tmp_path)
    out, tr = _trainer(tmp_path, train_rays, test_set, "plain", 20)
    # a level at which the young model has a surface: the density one node in ten exceeds
    crop = default_crop(tr.cfg)
    lo, h, dims = M.grid_dims(crop, 24)
    values = M.density_grid(tr, crop, dims)[0]
    level = float(torch.exp(values.flatten().float().kthvalue(int(0.9 * values.numel())).values))
    # smooth=0: the bytes export_clean_mesh writes
    a = M.export_clean_mesh(tr, out / "a.ply", resolution=24, level=level, min_faces=4)
    b = M.export_smooth_mesh(tr, out / "b.ply", resolution=24, level=level, min_faces=4, smooth=0)
    assert open(out / "a.ply", "rb").read() == open(out / "b.ply", "rb").read() and all(torch.equal(x, y) for x, y in zip(a, b))
    # smooth=3, with and without the component filter
    check_smoothed_export(a, M.export_smooth_mesh(tr, out / "s.ply", resolution=24, level=level, min_faces=4, smooth=3), out / "s.ply")
    check_smoothed_export(M.export_mesh(tr, None, resolution=24, level=level), M.export_smooth_mesh(tr, out / "m.ply", resolution=24, level=level, smooth=3),
                          out / "m.ply")
    # train(): the keyword reaches the exporter
    out2, tr2 = _trainer(tmp_path, train_rays, test_set, "smooth", 20, mesh=24, mesh_level=level, mesh_smooth=3)
    M.export_smooth_mesh(tr2, out2 / "again.ply", resolution=24, level=level, smooth=3)
    assert open(out2 / "again.ply", "rb").read() == open(out2 / "mesh.ply", "rb").read()
    check_smoothed_export(M.export_mesh(tr2, None, resolution=24, level=level), M.export_smooth_mesh(tr2, out2 / "t.ply", resolution=24, level=level, smooth=3),
                          out2 / "t.ply")
    with pytest.raises(ValueError):
        train(TrainConfig(method="kplanes"), train_rays, None, test_set, tmp_path, max_steps=1, mesh=24, mesh_smooth=-1)


TSDF_STEPS = 200                                                   # 6j's tiny K-Planes scene: 148 TSDF vertices after 200 steps, none after 20


def test_tsdf_exports_and_train_end_to_end(tmp_path, monkeypatch):
    from tinynerf_amd import mesh as M, tsdf
    train_rays, test_set = _datasets(tmp_path)
    # train(): tsdf_mesh.ply smoothed, its colours fused from the renders
    out, tr = _trainer(tmp_path, train_rays, test_set, "fused", TSDF_STEPS, tsdf_mesh=24, tsdf_colors="fused", mesh_smooth=3)
    plain = {c: tsdf.export_tsdf_mesh(tr, test_set, out / f"plain_{c}.ply", resolution=24, colors=c) for c in (True, "fused")}
    assert plain[True][0].size(0) > 50 and bool((plain[True][2] != plain["fused"][2]).any())
    for c in (True, "fused"):
        # smooth=0: the old exporter's bytes
        zero = tsdf.export_smooth_tsdf_mesh(tr, test_set, out / f"zero_{c}.ply", resolution=24, colors=c, smooth=0)
        assert open(out / f"zero_{c}.ply", "rb").read() == open(out / f"plain_{c}.ply", "rb").read() and all(torch.equal(x, y) for x, y in zip(zero, plain[c]))
        # smooth=3: the decoder and the colour volume are asked at the EXTRACTED positions, with the extracted normals
        asked, sampled = [], []
        decoder, sampler = M.vertex_colors, tsdf.sample_colors
        monkeypatch.setattr(M, "vertex_colors", lambda trainer, v, n, *a, **k: (asked.append((v.clone(), n.clone())), decoder(trainer, v, n, *a, **k))[1])
        monkeypatch.setattr(tsdf, "sample_colors", lambda *a: (sampled.append(a[-1].clone()), sampler(*a))[1])
        smoothed = tsdf.export_smooth_tsdf_mesh(tr, test_set, out / f"smooth_{c}.ply", resolution=24, colors=c, smooth=3)
        monkeypatch.setattr(M, "vertex_colors", decoder)
        monkeypatch.setattr(tsdf, "sample_colors", sampler)
        check_smoothed_export(plain[c], smoothed, out / f"smooth_{c}.ply")
        if c is True:
            assert len(asked) == 1 and not sampled and torch.equal(asked[0][0], plain[c][0]) and torch.equal(asked[0][1], plain[c][1])
        else:
            assert len(sampled) == 1 and torch.equal(sampled[0], plain[c][0])
            for v, n in asked:                                     # the bare vertices, if any: rows of the extracted mesh
                bare = (v[:, None, :] == plain[c][0][None]).all(2).any(1)
                assert bool(bare.all())
    assert open(out / "smooth_fused.ply", "rb").read() == open(out / "tsdf_mesh.ply", "rb").read()      # what train() wrote
    # the fallback for bare vertices: every third vertex without fused colour takes the decoder's, asked at its extracted position
    sampler = tsdf.sample_colors

    def thinned(*a):
        colour, den = sampler(*a)
        den[::3] = 0.0
        return colour, den
    asked = []
    decoder = M.vertex_colors
    monkeypatch.setattr(tsdf, "sample_colors", thinned)
    monkeypatch.setattr(M, "vertex_colors", lambda trainer, v, n, *a, **k: (asked.append((v.clone(), n.clone())), decoder(trainer, v, n, *a, **k))[1])
    mixed = tsdf.export_smooth_tsdf_mesh(tr, test_set, out / "mixed.ply", resolution=24, colors="fused", smooth=3)
    monkeypatch.setattr(tsdf, "sample_colors", sampler)
    monkeypatch.setattr(M, "vertex_colors", decoder)
    assert len(asked) == 1 and torch.equal(asked[0][0], plain["fused"][0][::3]) and torch.equal(asked[0][1], plain["fused"][1][::3])
    assert torch.equal(mixed[2][::3], plain[True][2][::3]) and torch.equal(mixed[2][1::3], plain["fused"][2][1::3])
    assert torch.equal(mixed[2][2::3], plain["fused"][2][2::3])
    check_smoothed_export(plain["fused"][:2] + (mixed[2],) + plain["fused"][3:], mixed, out / "mixed.ply")
    # train() with the decoder's colours
    out2, tr2 = _trainer(tmp_path, train_rays, test_set, "decoder", TSDF_STEPS, tsdf_mesh=24, mesh_smooth=3)
    tsdf.export_smooth_tsdf_mesh(tr2, test_set, out2 / "again.ply", resolution=24, smooth=3)
    assert open(out2 / "again.ply", "rb").read() == open(out2 / "tsdf_mesh.ply", "rb").read()
    assert M.read_mesh_ply(out2 / "tsdf_mesh.ply")[0].shape[0] > 50
    with pytest.raises(ValueError, match="export_smooth_tsdf_mesh"):
        tsdf.export_smooth_tsdf_mesh(tr2, test_set, None, resolution=24, colors="nonsense", smooth=1)
