"""CPU checks of the TSDF fusion: the yardstick (tests/_tsdf_ref.py) on hand-worked nodes, its margins, the face mask and
the mesh field; the host layer's argument checks without a device; the new flags and keywords of train.py and run.train."""
import importlib.util
import inspect
import os

import numpy as np
import pytest
import torch

import _tsdf_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- yardstick
def plane_view(depth_value=2.0, w=8, h=6):
    """one pinhole at the origin looking down -z (the identity pose), f = 4 px, centre (4.25, 3.25); every pixel holds `depth_value`"""
    c2w = np.eye(4)[:3][None]
    lens = np.float64([[4.0, 4.0, 4.25, 3.25, 0, 0, 0, 0, 0, 0]])
    return c2w, np.int64([0]), lens, np.int64([[w, h]]), np.full(w * h, depth_value, np.float32)


def test_nodes_in_front_of_on_and_behind_a_surface():
    # a 1 x 1 x 4 grid: nodes at x, y in {0, 0.5}, z = -1, -1.5, -2, -2.5, -3.  On the axis |p| = -z and the depth is 2 everywhere.
    c2w, models, lens, sizes, depth = plane_view()
    dims, lo, h = (1, 1, 4), np.float32([0, 0, -1]), np.float32([0.5, 0.5, -0.5])
    out = ref.integrate(dims, lo, h, c2w, models, lens, sizes, depth, None, 0.5, 0.5)
    S, W = out["S"].reshape(5, 2, 2), out["W"].reshape(5, 2, 2)
    # axis nodes (x = y = 0): sdf = 2 - |z| = 1, 0.5, 0, -0.5, -1 -> s = min(sdf / 0.5, 1) = 1, 1, 0, -1, and the last is hidden
    assert S[:, 0, 0].tolist() == [1.0, 1.0, 0.0, -1.0, 0.0] and W[:, 0, 0].tolist() == [1.0, 1.0, 1.0, 1.0, 0.0]
    # the node (0.5, 0.5, -2): |p| = sqrt(4.5), sdf = 2 - 2.1213 = -0.1213 -> s = -0.2426; it lands in pixel (5, 2): u = 5.25, v = 2.25
    assert abs(S[2, 1, 1] - (2.0 - np.sqrt(4.5)) / 0.5) < 1e-15 and W[2, 1, 1] == 1.0
    pr = ref.project(ref.nodes(dims, lo, h), c2w[0], 0, lens[0])
    k = 2 * 4 + 3
    assert abs(pr["u"][k] - 5.25) < 1e-15 and abs(pr["v"][k] - 2.25) < 1e-15 and pr["z"][k] == 2.0       # y up in the camera is v DOWN in the image
    assert out["margin_pixel"][k] == 0.25 and np.isinf(out["margin_guard"]).all()
    # the node on the truncation edge, sdf = -trunc exactly, is kept and has a zero margin; its neighbour's margin is 0.5 / |p|
    assert out["margin_trunc"][3 * 4] == 0.0 and abs(out["margin_trunc"][4 * 4] - 0.5 / 3.0) < 1e-15
    assert ref.field(S, W)[:, 0, 0].tolist() == [-1.0, -1.0, 0.0, 1.0, -1.0]                             # empty where nothing was seen


def test_gates_views_in_order_and_a_range_continued():
    c2w, models, lens, sizes, depth = plane_view()
    dims, lo, h = (1, 1, 4), np.float32([0, 0, -1]), np.float32([0.5, 0.5, -0.5])
    # nodes behind the camera: the same grid mirrored to z > 0
    behind = ref.integrate(dims, np.float32([0, 0, 1]), np.float32([0.5, 0.5, 0.5]), c2w, models, lens, sizes, depth, None, 0.5, 0.5)
    assert not behind["W"].any() and (behind["margin_z"] > 0.5).all()
    # bad depths and low opacities switch a pixel off
    for bad in (0.0, -2.0, np.nan, np.inf, -np.inf):
        out = ref.integrate(dims, lo, h, c2w, models, lens, sizes, np.full_like(depth, bad), None, 0.5, 0.5)
        assert not out["W"].any() and not out["S"].any()
    for op, votes in ((0.5, True), (0.49, False), (np.nan, False), (1.0, True)):
        out = ref.integrate(dims, lo, h, c2w, models, lens, sizes, depth, np.full_like(depth, op), 0.5, 0.5)
        assert bool(out["W"].any()) == votes
    # two views: a range continued from a state is the whole, and W counts both
    two = (np.concatenate([c2w, c2w]), np.int64([0, 0]), np.concatenate([lens, lens]), np.concatenate([sizes, sizes]), np.concatenate([depth, depth + 0.25]))
    whole = ref.integrate(dims, lo, h, *two, None, 0.5, 0.5)
    first = ref.integrate(dims, lo, h, *two, None, 0.5, 0.5, views=(0, 1))
    rest = ref.integrate(dims, lo, h, *two, None, 0.5, 0.5, views=(1, 1), state=(first["S"], first["W"]))
    assert np.array_equal(rest["S"], whole["S"]) and np.array_equal(rest["W"], whole["W"]) and whole["W"].max() == 2.0
    assert whole["S"].reshape(5, 2, 2)[2, 0, 0] == 0.5             # 0 from the first view, 0.25 / 0.5 from the second


def test_pixel_edges_and_the_guard():
    c2w, models, lens, sizes, depth = plane_view()
    # nodes on the plane z = -1: u = 4 x + 4.25 -- x = -1.0625 is the image's left edge u = 0 (inside), x = 0.9375 its right edge u = 8 (outside)
    lo, h = np.float32([-1.0625, 0.0, -1.0]), np.float32([2.0, 1.0, 1.0])
    out = ref.integrate((1, 0, 0), lo, h, c2w, models, lens, sizes, depth, None, 0.5, 5.0)
    assert out["W"].tolist() == [1.0, 0.0] and out["margin_pixel"].tolist() == [0.0, 0.0]
    assert ref._edge_distance(np.float64([-3.0, 0.2, 7.9, 8.0, 11.5]), 8).tolist() == pytest.approx([3.0, 0.2, 0.1, 0.0, 3.5])
    # a lens whose radial map turns back at r^2 = 4.97 (k1 = 1/16, k2 = -1/64, exact in float32: 1 + 3 k1 s + 5 k2 s^2): the guard passes
    # r = 1.9 and stops r = 2.5
    L = lens.copy()
    L[0, 4:6] = [0.0625, -0.015625]
    x = np.float64([[1.9, 0.0, -1.0], [2.5, 0.0, -1.0], [0.0, 0.0, -1.0]])
    pr = ref.project(x, c2w[0], ref.OPENCV, L[0])
    assert pr["guard"][0] > 0 > pr["guard"][1] and pr["guard"][2] == 1.0
    s = 1.9 ** 2
    assert abs(pr["guard"][0] - (1 + 0.1875 * s - 0.078125 * s * s)) < 1e-12
    assert abs(pr["u"][0] - (4.0 * 1.9 * (1 + 0.0625 * s - 0.015625 * s * s) + 4.25)) < 1e-12
    # the fisheye maps a point 45 degrees off the axis to theta = pi / 4, and the axis to the principal point
    fe = ref.project(np.float64([[1.0, 0.0, -1.0], [0.0, 0.0, -2.0]]), c2w[0], ref.FISHEYE, lens[0])
    assert abs(fe["u"][0] - (4.0 * np.pi / 4 + 4.25)) < 1e-12 and fe["u"][1] == 4.25 and fe["v"][1] == 3.25


def test_mask_faces_yardstick():
    W = np.ones((2, 2, 3))                                         # 2 x 1 x 1 cells
    W[0, 0, 0] = 0
    got = ref.mask_faces(W, (2, 1, 1), [0, 1], 2, [[0, 1, 1], [1, 1, 1], [1, 2, 1], [-1, 1, 1]])
    assert got.tolist() == [[-1] * 3, [1, 1, 1], [-1] * 3, [-1] * 3]


# ---------------------------------------------------------------------------------------------------------------- host layer
def test_host_layer_checks_its_arguments_without_a_device():
    from tinynerf_amd import tsdf

    class Table:
        n_img, n_rays = 2, 10
        c2w = torch.zeros((2, 3, 4))
    box = [-1.0] * 3 + [1.0] * 3
    depth = torch.zeros(10)
    for kw in (dict(trunc=0.0), dict(trunc=float("nan")), dict(trunc=float("inf")), dict(views=(1, 2)), dict(views=(-1, 1)), dict(dims=(4, 4)),
               dict(dims=(4, -1, 4)), dict(box=[0.0] * 6), dict(depth=torch.zeros(9)), dict(depth=depth.double()), dict(opacity=torch.zeros(3))):
        args = dict(cams=Table(), depth=depth, opacity=None, box=box, dims=(4, 4, 4), trunc=0.1)
        args.update(kw)
        with pytest.raises(ValueError):
            tsdf.integrate(**args)
    with pytest.raises(RuntimeError):                              # no CPU path
        tsdf.integrate(Table(), depth, None, box, (4, 4, 4), 0.1)
    f = torch.zeros((1, 3), dtype=torch.int32)
    with pytest.raises(RuntimeError):
        tsdf.mask_faces(torch.ones(27), (2, 2, 2), torch.zeros(8, dtype=torch.int32), 3, f)
    for args in ((torch.ones(26), (2, 2, 2), torch.zeros(8, dtype=torch.int32), 3, f), (torch.ones(27), (2, 2, 2), torch.zeros(7, dtype=torch.int32), 3, f),
                 (torch.ones(27), (2, 2, 2), torch.zeros(8, dtype=torch.int32), 3, f.long()), (torch.ones(27), (2, 2, 2), torch.zeros(8, dtype=torch.int32), -1, f)):
        with pytest.raises(ValueError):
            tsdf.mask_faces(*args)
    S, W = torch.tensor([2.0, -1.0, 0.0, 3.0]), torch.tensor([2.0, 4.0, 0.0, 3.0])
    assert tsdf.field(S, W).tolist() == [-1.0, 0.25, -1.0, -1.0]

    class TwoRanks:
        world = 2
    with pytest.raises(ValueError, match="world_size"):
        tsdf.export_tsdf_mesh(TwoRanks(), None)

    class Anything:
        world = 1
    for kw in (dict(min_faces=-1), dict(keep_fraction=1.5), dict(depth="nearest")):
        with pytest.raises(ValueError):
            tsdf.export_tsdf_mesh(Anything(), None, **kw)


def test_pose_dataset_keeps_its_cameras_and_makes_a_pose_only_table():
    from tinynerf_amd import data, rays
    cams = rays.look_at_origin_poses(3, seed=2)
    K = rays.Intrinsics(20.0, 21.0, 8.3, 5.9, 16, 12)
    ds = data.PoseDataset(data.NerfData(cams, K, None, None), "cpu")
    assert torch.equal(ds.cameras, cams) and len(ds) == 3


def test_signatures_and_defaults():
    from tinynerf_amd import mesh as M, run, tsdf
    sig = inspect.signature(tsdf.integrate)
    assert list(sig.parameters) == ["cams", "depth", "opacity", "box", "dims", "trunc", "min_opacity", "state", "views"]
    assert sig.parameters["min_opacity"].default == 0.5 and sig.parameters["state"].default is None and sig.parameters["views"].default is None
    assert list(inspect.signature(tsdf.field).parameters) == ["S", "W"]
    assert list(inspect.signature(tsdf.mask_faces).parameters) == ["W", "dims", "cell_ids", "n_vertices", "faces"]
    sig = inspect.signature(tsdf.export_tsdf_mesh)
    assert list(sig.parameters) == ["trainer", "dataset", "path", "resolution", "trunc", "crop", "indices", "min_faces", "keep_fraction", "depth", "colors"]
    want = dict(path=None, resolution=256, trunc=None, crop=None, indices=None, min_faces=0, keep_fraction=0.0, depth="expected", colors=True)
    assert {k: sig.parameters[k].default for k in want} == want
    assert list(inspect.signature(M.extract_with_cells).parameters) == list(inspect.signature(M.extract).parameters)
    sig = inspect.signature(run.train)
    assert sig.parameters["tsdf_mesh"].default == 0 and sig.parameters["tsdf_trunc"].default is None


def test_train_cli_tsdf_flags():
    spec = importlib.util.spec_from_file_location("tinynerf_train_cli", os.path.join(ROOT, "train.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    base = ["--data", "d", "--datatype", "synthetic", "--output", "o", "--method", "kplanes"]
    args = cli.parse_args(base)
    assert args.export_tsdf_mesh == 0 and args.tsdf_trunc is None
    args = cli.parse_args(base + ["--export_tsdf_mesh", "128"])
    assert args.export_tsdf_mesh == 128 and args.tsdf_trunc is None and args.export_mesh == 0
    args = cli.parse_args(base + ["--export_tsdf_mesh", "128", "--tsdf_trunc", "0.05", "--mesh_min_faces", "50", "--mesh_keep_fraction", "0.5",
                                  "--mesh_crop", "-1", "-1", "-1", "1", "1", "1"])
    assert args.tsdf_trunc == 0.05 and args.mesh_min_faces == 50 and args.mesh_keep_fraction == 0.5 and args.mesh_crop == [-1, -1, -1, 1, 1, 1]
    for extra in (["--tsdf_trunc", "0.1"], ["--export_tsdf_mesh", "0", "--tsdf_trunc", "0.1"], ["--export_tsdf_mesh", "64", "--tsdf_trunc", "0"],
                  ["--export_tsdf_mesh", "64", "--tsdf_trunc", "-1"], ["--export_tsdf_mesh", "64", "--tsdf_trunc", "nan"],
                  ["--export_tsdf_mesh", "64", "--tsdf_trunc", "inf"], ["--export_tsdf_mesh", "-1"], ["--mesh_min_faces", "5"]):
        with pytest.raises(SystemExit):
            cli.parse_args(base + extra)
    assert "--export_tsdf_mesh" in open(os.path.join(ROOT, "train.py")).read().split("FLAGS = (")[0]      # the FLAGS comment names it
