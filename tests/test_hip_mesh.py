"""GPU tests of the mesh export: tn_mesh_extract through the C ABI against the numpy restatement of its definition
(tests/_mesh_ref.py) -- counts, active cells and every face index exactly, positions and normals within the bounds derived from
the float32 arithmetic --, the capacity contract, the device mesh's own closedness, tn_grid_nodes bit for bit, mesh.extract_mesh
on an analytic density, and train(mesh=16) end to end on a scene on disk."""
import ctypes as C
import json
import sys

import numpy as np
import pytest
import torch

import _mesh_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (nx, ny, nz): one cell -- a vertex and no face can exist; the first grid with a face; odd, unequal dims -- a wave spans rows and
# slices; ragged last wave and last workgroup; exactly 1024 workgroups -- the scan's trip edge; a second scan trip with a carry
SHAPES = ((1, 1, 1), (2, 2, 2), (3, 5, 7), (17, 9, 33), (64, 64, 64), (65, 64, 64))
CLOSED_SHAPES = SHAPES[3:]                                         # where tests/test_mesh_host.py shows the yardstick's surfaces closed
SENTINEL_F, SENTINEL_I, TAIL = -7.25, -12345, 5


# ------------------------------------------------------------------------------------------------------------ the call
def run(values, lo, h, level, vcap, fcap, alloc=None, null_outputs=False, normals=True, guard=(0, 64), spare=0):
    """tn_mesh_extract through the C ABI on sentinel-filled outputs of `alloc` = (vertex rows, face rows) >= the capacities ->
    (counts, vertices, normals, faces, cell -> vertex id map) as numpy, ALL allocated rows.  The workspace is
    tn_mesh_workspace_bytes + `spare` bytes with `guard` bytes of a fixed pattern before and behind it."""
    from tinynerf_amd import _lib as L
    dev = torch.device(DEV)
    v = torch.from_numpy(np.array(values, np.float32)).to(dev)              # (a copy: the shared case is read only)
    nz, ny, nx = (s - 1 for s in values.shape)
    cells = nx * ny * nz
    va, fa = (vcap, fcap) if alloc is None else alloc
    assert va >= vcap and fa >= fcap
    lo_c, h_c, dims_c = (C.c_float * 3)(*np.float32(lo).tolist()), (C.c_float * 3)(*np.float32(h).tolist()), (C.c_int32 * 3)(nx, ny, nz)
    nbytes = C.c_int64(0)
    L.call_plain("tn_mesh_workspace_bytes", C.c_int32(nx), C.c_int32(ny), C.c_int32(nz), C.byref(nbytes))
    first, last = guard[0], guard[0] + nbytes.value + spare
    work = torch.full((last + guard[1],), 0x5A, dtype=torch.uint8, device=dev)
    vert = torch.full((va, 3), SENTINEL_F, dtype=torch.float32, device=dev)
    nrm = torch.full((va, 3), SENTINEL_F, dtype=torch.float32, device=dev)
    faces = torch.full((fa, 3), SENTINEL_I, dtype=torch.int32, device=dev)
    counts = torch.full((2,), -1, dtype=torch.int64, device=dev)
    outs = (None, None, None) if null_outputs else (L.ptr(vert), L.ptr(nrm) if normals else None, L.ptr(faces))
    L.call("tn_mesh_extract", dev, L.ptr(v), dims_c, lo_c, h_c, C.c_float(level), C.c_int64(vcap), C.c_int64(fcap), *outs, L.ptr(counts),
           L.ptr(work[first:]))
    torch.cuda.synchronize()
    assert bool((work[:first] == 0x5A).all()) and bool((work[last:] == 0x5A).all()), "the workspace was overrun"
    g = -(-cells // 256)
    vid = work[first + 144 * g:first + 144 * g + 4 * cells].cpu().numpy().view(np.int32)      # the documented layout: ballots, counts, then the ids
    return counts.cpu().numpy(), vert.cpu().numpy(), nrm.cpu().numpy(), faces.cpu().numpy(), vid


def check_against_yardstick(name, dims):
    """one (field, grid) case: capacities exact, too small and 0 -> (V, F, worst position ratio, worst normal ratio, normal rows skipped)"""
    values, lo, h, level, want = ref.case(name, dims)
    V, F = want["vertices"].shape[0], want["faces"].shape[0]
    tag = (name, dims)
    # capacity 0, null outputs: the counts alone
    counts = run(values, lo, h, level, 0, 0, null_outputs=True)[0]
    assert counts.tolist() == [V, F], (tag, counts, V, F)
    # exact capacities, TAIL sentinel rows behind them
    counts, vert, nrm, faces, vid = run(values, lo, h, level, V, F, alloc=(V + TAIL, F + TAIL))
    assert counts.tolist() == [V, F], tag
    if V == 0 and F == 0:                                          # both capacities 0: two launches, no map -- ask with room for rows
        counts, vert, nrm, faces, vid = run(values, lo, h, level, TAIL, TAIL)
        assert counts.tolist() == [0, 0], tag
    active = np.flatnonzero(vid >= 0)
    assert np.array_equal(active, want["cells"]), tag                              # the set of active cells ...
    assert np.array_equal(vid[active], np.arange(V)) and (vid[vid < 0] == -1).all(), tag      # ... and their order
    assert np.array_equal(faces[:F], want["faces"]), tag                           # every index
    assert (vert[V:] == np.float32(SENTINEL_F)).all() and (nrm[V:] == np.float32(SENTINEL_F)).all() and (faces[F:] == SENTINEL_I).all(), tag
    ratio = np.abs(vert[:V].astype(np.float64) - want["vertices"]) / want["vertex_bound"] if V else np.zeros(1)
    print(f"{name} {dims}: V {V} F {F}, worst position error / bound {ratio.max():.4f}")
    assert ratio.max() <= 1.0, (tag, ratio.max())
    zero = (want["normals"] == 0).all(1)
    assert (nrm[:V][zero] == 0).all(), tag                                         # n_ref = 0 (a corner that is not finite): exactly 0
    n_ratio, skipped = 0.0, 0
    if name in ref.CLOSED and V:
        keep = want["normal_bound"] <= 1e-3
        skipped = int((~keep).sum())
        assert skipped <= 0.01 * V, (tag, skipped, V)
        err = np.abs(nrm[:V].astype(np.float64) - want["normals"]).max(1)
        n_ratio = float((err[keep] / want["normal_bound"][keep]).max())
        print(f"{name} {dims}: worst normal error / bound {n_ratio:.4f}, rows skipped {skipped}")
        assert n_ratio <= 1.0, (tag, n_ratio)
    # capacities too small (an odd number of face rows: half a quad): the counts unchanged, the first rows the same, the tail untouched
    if V or F:
        vcap, fcap = V // 2, (min((F // 2) | 1, F - 1) if F else 0)
        c2, vert2, nrm2, faces2, _ = run(values, lo, h, level, vcap, fcap, alloc=(V + TAIL, F + TAIL))
        assert c2.tolist() == [V, F], tag
        assert np.array_equal(vert2[:vcap].view(np.uint32), vert[:vcap].view(np.uint32)) and np.array_equal(nrm2[:vcap].view(np.uint32), nrm[:vcap].view(np.uint32)), tag
        assert np.array_equal(faces2[:fcap], faces[:fcap]), tag
        assert (vert2[vcap:] == np.float32(SENTINEL_F)).all() and (nrm2[vcap:] == np.float32(SENTINEL_F)).all() and (faces2[fcap:] == SENTINEL_I).all(), tag
    return V, F, float(ratio.max()), n_ratio, skipped, vert[:V], faces[:F]


# ------------------------------------------------------------------------------------------------------------ against the yardstick
@pytest.mark.parametrize("dims", SHAPES)
@pytest.mark.parametrize("name", ref.FIELDS)
def test_counts_cells_faces_exact_positions_and_normals_within_bounds(name, dims):
    V, F, _, _, _, vert, faces = check_against_yardstick(name, dims)
    if name in ("all_inside", "all_outside"):
        assert V == 0 and F == 0
    if dims == (1, 1, 1):
        assert F == 0 and V <= 1
        if name in ("noise", "plane"):
            assert V == 1                                          # a vertex and no face
    if dims == (2, 2, 2) and name == "sphere":
        assert (V, F) == (8, 12)                                   # the first grid with a face: the centre node alone is inside
    if name in ref.CLOSED and dims in CLOSED_SHAPES:
        # the device mesh itself: closed, consistently oriented, outward, the yardstick's volume
        twice, paired, edges = ref.edge_report(faces)
        assert twice and paired and V - edges + F == ref.CLOSED[name]
        want = ref.case(name, dims)[4]
        vol, vol_ref = ref.signed_volume(vert, faces), ref.signed_volume(want["vertices"], want["faces"])
        assert vol > 0 and abs(vol - vol_ref) <= 1e-5 * vol_ref, (vol, vol_ref)


@pytest.mark.parametrize("dims", [(1, 1, 1), (3, 5, 7), (17, 9, 33)])
def test_the_workspace_is_what_the_size_function_says(dims):
    """every ballot, count and id lands inside the layout: a workspace of exactly tn_mesh_workspace_bytes in the middle of a larger
    buffer leaves the bytes around it alone (`run` asserts that) and gives the outputs, the id map included, of a generous one"""
    for name in ("noise", "sphere"):
        values, lo, h, level, want = ref.case(name, dims)
        V, F = want["vertices"].shape[0], want["faces"].shape[0]
        tight = run(values, lo, h, level, V, F, alloc=(V + TAIL, F + TAIL), guard=(256, 256))
        generous = run(values, lo, h, level, V, F, alloc=(V + TAIL, F + TAIL), guard=(256, 256), spare=4096)
        assert tight[0].tolist() == [V, F], (name, dims)
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(tight, generous)), (name, dims)


def test_two_calls_give_the_same_bytes_and_normals_are_optional():
    values, lo, h, level, want = ref.case("specks", (65, 64, 64))
    V, F = want["vertices"].shape[0], want["faces"].shape[0]
    a = run(values, lo, h, level, V, F)
    b = run(values, lo, h, level, V, F)
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))
    c = run(values, lo, h, level, V, F, normals=False)
    assert np.array_equal(c[1].view(np.uint32), a[1].view(np.uint32)) and np.array_equal(c[3], a[3]) and (c[2] == np.float32(SENTINEL_F)).all()
    # vertices alone, faces alone: the other output may be NULL with its capacity 0
    from tinynerf_amd import mesh as M
    vt = torch.from_numpy(np.array(values)).to(DEV)
    v_only = M.extract(vt, lo, h, float(level), capacity=(V, 0))
    f_only = M.extract(vt, lo, h, float(level), normals=False, capacity=(0, F))
    assert v_only[2].shape == (0, 3) and np.array_equal(v_only[0].cpu().numpy().view(np.uint32), a[1].view(np.uint32))
    assert f_only[0].shape == (0, 3) and f_only[1] is None and np.array_equal(f_only[2].cpu().numpy(), a[3])
    # the host layer's two-call form returns the same mesh
    vert, nrm, faces = M.extract(vt, lo, h, float(level))
    assert np.array_equal(vert.cpu().numpy().view(np.uint32), a[1].view(np.uint32)) and np.array_equal(nrm.cpu().numpy().view(np.uint32), a[2].view(np.uint32))
    assert np.array_equal(faces.cpu().numpy(), a[3]) and faces.dtype == torch.int32


def test_an_empty_grid_writes_zero_counts():
    from tinynerf_amd import _lib as L
    counts = torch.full((2,), -1, dtype=torch.int64, device=DEV)
    z = (C.c_float * 3)(0, 0, 0)
    L.call("tn_mesh_extract", torch.device(DEV), None, (C.c_int32 * 3)(4, 0, 4), z, z, C.c_float(0.0), C.c_int64(0), C.c_int64(0), None, None, None,
           L.ptr(counts), None)
    assert counts.tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------------------ nodes, host layer
def test_grid_nodes_are_bit_exact():
    from tinynerf_amd import mesh as M
    dims, lo, h = (65, 33, 17), np.float32([-1.1, 0.3, 7.7]), np.float32([0.03, 0.11, 0.007])
    want = ref.node_positions(dims, lo, h).reshape(-1, 3)
    n = want.shape[0]
    got = M.grid_nodes(lo, h, dims, 0, n, DEV).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    for first, m in ((0, 1), (n - 1, 1), (66 * 34 - 3, 700), (12345, 257)):        # ranges across rows and slices
        part = M.grid_nodes(lo, h, dims, first, m, DEV).cpu().numpy()
        assert np.array_equal(part.view(np.uint32), want[first:first + m].view(np.uint32))


def test_extract_mesh_is_extract_on_the_values_at_the_grid_nodes():
    from tinynerf_amd import core, mesh as M
    dev = torch.device(DEV)
    aabb = torch.tensor([[-1.5, -1.5, -1.5], [1.5, 1.5, 1.5]], device=dev)
    contraction = core.ContractionAABB(aabb)

    def sigma_fn(x):                                               # a blob in contracted coordinates: sigma = 5 on an ellipsoid
        r = ((x[:, 0] - 0.05) ** 2 + (1.3 * x[:, 1]) ** 2 + (0.8 * x[:, 2] + 0.1) ** 2).sqrt()
        return 5.0 * torch.exp(8.0 * (0.5 - r))

    box = [-1.2, -0.9, -1.4, 1.2, 0.9, 1.0]                        # the blob lies strictly inside
    vert, nrm, faces = M.extract_mesh(sigma_fn, box, 24, level=5.0, contraction=contraction)
    lo, h, dims = M.grid_dims(box, 24)
    assert dims == (24, 18, 24)
    n = 25 * 19 * 25
    x = M.grid_nodes(lo, h, dims, 0, n, dev)
    values = torch.log(sigma_fn(contraction(x)[0]).clamp_min(1e-30)).view(25, 19, 25)
    v2, n2, f2 = M.extract(values, lo, h, float(np.log(5.0)))
    assert vert.size(0) > 100 and faces.size(0) > 200
    assert torch.equal(vert, v2) and torch.equal(nrm, n2) and torch.equal(faces, f2)
    # chunked node evaluation changes nothing
    v3, n3, f3 = M.extract_mesh(sigma_fn, box, 24, level=5.0, contraction=contraction, chunk=1000)
    assert torch.equal(vert, v3) and torch.equal(nrm, n3) and torch.equal(faces, f3)
    twice, paired, edges = ref.edge_report(faces.cpu().numpy())
    assert twice and paired and vert.size(0) - edges + faces.size(0) == 2
    # against the yardstick on the same values
    want = ref.surface_nets(values.cpu().numpy(), lo, h, np.float32(np.log(5.0)))
    assert np.array_equal(faces.cpu().numpy(), want["faces"])
    assert (np.abs(vert.cpu().numpy().astype(np.float64) - want["vertices"]) <= want["vertex_bound"]).all()
    # the default level: ln 2 / max(h)
    v4, _, _ = M.extract_mesh(sigma_fn, box, 24, contraction=contraction)
    v5, _, _ = M.extract_mesh(sigma_fn, box, 24, level=M.default_level(h), contraction=contraction)
    assert v4.size(0) > 0 and torch.equal(v4, v5)


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


def _decoder_bytes(tr, vertices, normals):
    """the colour decoder called by the test at the vertices, view direction -n ((0,0,-1) where n = 0), to bytes as tn_points_compact"""
    x, n = torch.from_numpy(vertices).to(DEV), torch.from_numpy(normals).to(DEV)
    d = -n
    d[(n == 0).all(1)] = torch.tensor([0.0, 0.0, -1.0], device=DEV)
    with torch.no_grad():
        tr.renderer.eval()
        c = tr.renderer.rgb_decoder(tr.renderer.feature_module(tr.ray_provider.contraction(x)[0]), d.contiguous()).cpu().numpy()
    c = np.where(c > 0, np.minimum(c, 1.0), 0.0).astype(np.float32)                # NaN -> 0
    return (c.astype(np.float64) * 255.0 + 0.5).astype(np.float32).astype(np.uint8)


@pytest.mark.parametrize("method", ["kplanes", "hashgrid"])
def test_train_writes_a_mesh(tmp_path, method):
    from tinynerf_amd import data, mesh as M
    from tinynerf_amd.run import TrainConfig, train
    _scene_on_disk(tmp_path)
    dev = torch.device(DEV)
    train_rays = data.RaysDataset(data.parse_nerf_synthetic(tmp_path, "train"), dev)
    test_set = data.PoseDataset(data.parse_nerf_synthetic(tmp_path, "test"), dev)
    kw = dict(hashgrid_log2_table_size=14) if method == "hashgrid" else dict(kplanes_resolutions=(16, 32, 64))

    def go(name, **more):
        out = tmp_path / name
        out.mkdir()
        cfg = TrainConfig(method=method, batch_size=512, n_samples=64, occupancy_res=32, seed=3, **kw)
        return out, train(cfg, train_rays, None, test_set, out, max_steps=20, log_every=50, **more)[0]

    out, tr = go("on", mesh=16)
    vert, nrm, rgb, faces = M.read_mesh_ply(out / "mesh.ply")
    V, F = vert.shape[0], faces.shape[0]
    direct = M.export_mesh(tr, None, resolution=16)
    assert (direct[0].size(0), direct[3].size(0)) == (V, F)        # the same trainer, the same counts
    print(f"{method}: mesh.ply has {V} vertices, {F} triangles")
    assert ((faces >= 0) & (faces < max(V, 1))).all() and np.isfinite(vert).all() and (np.abs(vert) <= 1.5).all()      # the default crop
    assert np.array_equal(rgb, _decoder_bytes(tr, vert, nrm))
    # a level inside the density's range, so that there is a surface whatever 20 steps have learnt; a crop that is not the default
    crop = [-1.0, -1.2, -0.8, 1.0, 0.4, 0.8]
    lo, h, dims = M.grid_dims(crop, 16)
    values = M.density_grid(tr, crop, dims)[0]
    level = float(torch.exp(values.flatten().float().kthvalue(int(0.7 * values.numel())).values))
    v, n, c, f = M.export_mesh(tr, out / "level.ply", resolution=16, level=level, crop=crop)
    assert v.size(0) > 0 and f.size(0) > 0 and int(f.max()) < v.size(0) and int(f.min()) >= 0
    p = v.cpu().numpy()
    assert (p >= np.float32(crop[:3]) - 1e-6).all() and (p <= np.float32(crop[3:]) + 1e-6).all()
    got = M.read_mesh_ply(out / "level.ply")
    assert np.array_equal(got[0].view(np.uint32), p.view(np.uint32)) and np.array_equal(got[3], f.cpu().numpy())
    assert np.array_equal(got[2], _decoder_bytes(tr, got[0], got[1])) and np.array_equal(got[2], c.cpu().numpy())
    length = np.linalg.norm(got[1].astype(np.float64), axis=1)
    assert (np.abs(length[length > 0] - 1.0) < 1e-5).all()
    no_colors = M.export_mesh(tr, None, resolution=16, level=level, crop=crop, colors=False)
    assert torch.equal(no_colors[0], v) and not no_colors[2].any()
    if method == "kplanes":
        # mesh=0: nothing of it is imported or written
        sys.modules.pop("tinynerf_amd.mesh", None)
        out0, _ = go("off", mesh=0)
        assert "tinynerf_amd.mesh" not in sys.modules and not (out0 / "mesh.ply").exists()
        import tinynerf_amd.mesh                                   # noqa: F401  (back for the tests that follow)
