"""CPU checks of the TSDF colour fusion: the yardstick (tests/_tsdf_color_ref.py) on hand-worked nodes and points, the host
layer's argument checks without a device, the new keyword of run.train and the new flag of train.py."""
import importlib.util
import inspect
import os

import numpy as np
import pytest
import torch

import _tsdf_color_ref as cref
from test_tsdf_host import plane_view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# a 1 x 1 x 4 grid under plane_view(): nodes at x, y in {0, 0.5}, z = -1, -1.5, -2, -2.5, -3; on the axis |p| = -z, the depth is 2
DIMS, LO, H = (1, 1, 4), np.float32([0, 0, -1]), np.float32([0.5, 0.5, -0.5])


def axis(C):
    return C.reshape(5, 2, 2, 4)[:, 0, 0]


# ---------------------------------------------------------------------------------------------------------------- integrate_color
def test_the_weight_is_triangular_over_the_band():
    c2w, models, lens, sizes, depth = plane_view()
    rgb = np.tile(np.float32([0.25, 0.5, 1.0]), (depth.size, 1))
    # trunc = 1: sdf = 1, 0.5, 0, -0.5, -1 -> the nodes at +-trunc get w = 0, half a band in front and behind 0.5, on the surface 1
    out = cref.integrate_color(DIMS, LO, H, c2w, models, lens, sizes, depth, None, 0.5, rgb, None, 1.0)
    assert axis(out["C"])[:, 3].tolist() == [0.0, 0.5, 1.0, 0.5, 0.0]
    assert axis(out["C"])[:, :3].tolist() == [[0.0] * 3, [0.125, 0.25, 0.5], [0.25, 0.5, 1.0], [0.125, 0.25, 0.5], [0.0] * 3]
    assert out["n_views"].reshape(5, 2, 2)[:, 0, 0].tolist() == [1.0] * 5         # the edges are inside the band: w is 0 there, not missing
    # trunc = 0.25: the nodes in free space (sdf = 1, 0.5) and those hidden behind the surface (sdf = -0.5, -1) get nothing
    out = cref.integrate_color(DIMS, LO, H, c2w, models, lens, sizes, depth, None, 0.5, rgb, None, 0.25)
    assert axis(out["C"]).tolist() == [[0.0] * 4, [0.0] * 4, [0.25, 0.5, 1.0, 1.0], [0.0] * 4, [0.0] * 4]
    assert out["n_views"].reshape(5, 2, 2)[:, 0, 0].tolist() == [0.0, 0.0, 1.0, 0.0, 0.0]
    # the node (0.5, 0.5, -2) off the axis: |p| = sqrt(4.5), sdf = -0.1213, w = 1 - 0.1213 / 0.25
    assert abs(out["C"].reshape(5, 2, 2, 4)[2, 1, 1, 3] - (1.0 - (np.sqrt(4.5) - 2.0) / 0.25)) < 1e-15


def test_the_background_is_taken_out_again_and_bad_colours_are_clamped():
    c2w, models, lens, sizes, depth = plane_view()
    n = depth.size
    bg = np.float32([0.25, 0.75, 0.5])
    true = np.float64([0.5, 0.125, 1.0])
    opacity = np.full(n, 0.8, np.float32)
    op = np.float64(opacity[0])
    rgb = np.tile((op * true + (1.0 - op) * bg).astype(np.float32), (n, 1))       # composited over bg at opacity 0.8
    out = cref.integrate_color(DIMS, LO, H, c2w, models, lens, sizes, depth, opacity, 0.5, rgb, bg, 0.25)
    got = axis(out["C"])[2]
    assert got[3] == 1.0 and np.abs(got[:3] - true).max() < 2e-7                  # the float32 rounding of rgb, over 0.8
    leaked = axis(cref.integrate_color(DIMS, LO, H, c2w, models, lens, sizes, depth, opacity, 0.5, rgb, None, 0.25)["C"])[2]
    assert np.abs(leaked[:3] - true).max() > 0.05                                 # without bg the background stays in the colour
    # the gate is tn_tsdf_integrate's: below min_opacity and NaN say nothing
    for bad in (0.49, np.nan):
        assert not cref.integrate_color(DIMS, LO, H, c2w, models, lens, sizes, depth, np.full(n, bad, np.float32), 0.5, rgb, bg, 0.25)["C"].any()
    # NaN -> 0, below 0 -> 0, above 1 -> 1; the weight is added all the same
    for value, want in ((np.nan, 0.0), (-0.3, 0.0), (1.7, 1.0), (0.625, 0.625)):
        out = cref.integrate_color(DIMS, LO, H, c2w, models, lens, sizes, depth, None, 0.5, np.full((n, 3), value, np.float32), bg, 0.25)
        assert axis(out["C"])[2].tolist() == [want, want, want, 1.0]
    col, raw = cref.uncomposite(np.float64([[0.5, 2.0, np.nan]]), np.float64([0.5]), np.float64([1.0, 0.0, 0.0]))
    assert col.tolist() == [[0.0, 1.0, 0.0]] and raw[0, :2].tolist() == [0.0, 4.0]


def test_views_in_order_a_range_continued_and_the_margins():
    c2w, models, lens, sizes, depth = plane_view()
    n = depth.size
    two = (np.concatenate([c2w, c2w]), np.int64([0, 0]), np.concatenate([lens, lens]), np.concatenate([sizes, sizes]), np.concatenate([depth, depth + 0.25]))
    rgb = np.concatenate([np.full((n, 3), 0.25, np.float32), np.full((n, 3), 0.75, np.float32)])
    whole = cref.integrate_color(DIMS, LO, H, *two, None, 0.5, rgb, None, 0.5, margins=True)
    first = cref.integrate_color(DIMS, LO, H, *two, None, 0.5, rgb, None, 0.5, views=(0, 1))
    rest = cref.integrate_color(DIMS, LO, H, *two, None, 0.5, rgb, None, 0.5, views=(1, 1), state=first["C"])
    assert np.array_equal(rest["C"], whole["C"])
    # the node on the first view's surface: w = 1 there and 0.5 from the second, whose surface is 0.25 behind it
    assert axis(whole["C"])[2].tolist() == [0.25 + 0.5 * 0.75] * 3 + [1.5]
    assert whole["margin_trunc"].shape == (20,) and np.isinf(whole["margin_guard"]).all()


# ---------------------------------------------------------------------------------------------------------------- sample_colors
def volume():
    """2 x 1 x 1 cells, 3 x 2 x 2 nodes: the nodes at i = 0 and 1 coloured by their index with the weight 2, those at i = 2 uncoloured"""
    C = np.zeros((2, 2, 3, 4), np.float32)
    for k in range(2):
        for j in range(2):
            for i in range(2):
                colour = np.float32([0.125 * (i + 1), 0.25 * j, 0.5 * k])
                C[k, j, i] = np.concatenate([2.0 * colour, [2.0]])
    return C, (2, 1, 1), np.float32([0.0, 0.0, 0.0]), np.float32([0.5, 1.0, 1.0])


def test_sample_colors_yardstick():
    C, dims, lo, h = volume()
    points = np.float32([[0.5, 1.0, 1.0],                          # the node (1, 1, 1): its own colour
                         [0.25, 0.5, 0.5],                         # the centre of cell 0: the mean of its 8 corners
                         [0.75, 0.5, 0.5],                         # the centre of cell 1: four corners uncoloured -- the mean of the coloured four
                         [1.0, 0.25, 0.5],                         # on the uncoloured face: den = 0
                         [-3.0, 0.5, 0.5], [0.0, 0.5, 0.5],        # outside the grid: clamped onto its face
                         [0.25, 7.0, -2.0], [0.25, 1.0, 0.0],
                         [np.nan, 0.5, 0.5], [0.25, np.inf, 0.5]])
    out = cref.sample_colors(C.reshape(-1, 4), dims, lo, h, points)
    rgb, den = out["rgb"], out["den"]
    assert rgb[0].tolist() == [0.25, 0.25, 0.5] and den[0] == 2.0
    assert rgb[1].tolist() == [0.1875, 0.125, 0.25] and den[1] == 2.0
    assert rgb[2].tolist() == [0.25, 0.125, 0.25] and den[2] == 1.0              # not darkened: half the weight, the coloured corners' mean
    assert rgb[3].tolist() == [0.0] * 3 and den[3] == 0.0
    assert rgb[4].tolist() == rgb[5].tolist() == [0.125, 0.125, 0.25] and den[4] == den[5] == 2.0
    assert rgb[6].tolist() == rgb[7].tolist() and den[6] == den[7] == 2.0
    assert not rgb[8:].any() and not den[8:].any() and out["finite"].tolist() == [True] * 8 + [False] * 2
    assert out["near_face"][:3].tolist() == [True, False, False] and out["spread"][1].tolist() == [0.25, 0.5, 1.0, 0.0]
    assert out["spread"][0].tolist() == [0.5, 0.5, 1.0, 2.0] and out["size"][2].tolist() == [0.5, 0.5, 1.0, 2.0]      # on a node: the neighbours too
    nothing = cref.sample_colors(np.zeros_like(C).reshape(-1, 4), dims, lo, h, points)
    assert not nothing["rgb"].any() and not nothing["den"].any()


# ---------------------------------------------------------------------------------------------------------------- host layer
def test_host_layer_checks_its_arguments_without_a_device():
    from tinynerf_amd import tsdf

    class Table:
        n_img, n_rays = 2, 10
        c2w = torch.zeros((2, 3, 4))
    box = [-1.0] * 3 + [1.0] * 3
    depth, rgb = torch.zeros(10), torch.zeros((10, 3))
    for kw in (dict(trunc=0.0), dict(trunc=float("nan")), dict(trunc=float("inf")), dict(views=(1, 2)), dict(views=(-1, 1)), dict(dims=(4, 4)),
               dict(dims=(4, -1, 4)), dict(box=[0.0] * 6), dict(depth=torch.zeros(9)), dict(depth=depth.double()), dict(opacity=torch.zeros(3)),
               dict(rgb=torch.zeros((9, 3))), dict(rgb=torch.zeros(10)), dict(rgb=rgb.double()), dict(bg=torch.zeros(4)), dict(bg=torch.zeros(3).double()),
               dict(opacity=torch.ones(10), min_opacity=0.0), dict(opacity=torch.ones(10), min_opacity=float("nan"))):
        args = dict(cams=Table(), depth=depth, opacity=None, rgb=rgb, bg=None, box=box, dims=(4, 4, 4), trunc=0.1)
        args.update(kw)
        with pytest.raises(ValueError):
            tsdf.integrate_color(**args)
    with pytest.raises(RuntimeError):                              # no CPU path
        tsdf.integrate_color(Table(), depth, None, rgb, None, box, (4, 4, 4), 0.1)
    vol, points = torch.zeros((3, 3, 3, 4)), torch.zeros((5, 3))
    with pytest.raises(RuntimeError):
        tsdf.sample_colors(vol, box, (2, 2, 2), points)
    for args in ((vol, box, (2, 2, 3), points), (vol.double(), box, (2, 2, 2), points), (vol[..., :3], box, (2, 2, 2), points),
                 (vol, box, (2, 2, 2), points.double()), (vol, box, (2, 2, 2), torch.zeros((5, 4))), (vol, [0.0] * 6, (2, 2, 2), points),
                 (vol, box, (2, 2), points)):
        with pytest.raises(ValueError):
            tsdf.sample_colors(*args)

    class Anything:
        world = 1
    for bad in ("nonsense", "decoder", "Fused", ""):
        with pytest.raises(ValueError, match="colors"):
            tsdf.export_tsdf_mesh(Anything(), None, colors=bad)

    class TwoRanks:
        world = 2
    with pytest.raises(ValueError, match="world_size"):
        tsdf.export_tsdf_mesh(TwoRanks(), None, colors="fused")


def test_signatures_and_defaults():
    from tinynerf_amd import run, tsdf
    sig = inspect.signature(tsdf.integrate_color)
    assert list(sig.parameters) == ["cams", "depth", "opacity", "rgb", "bg", "box", "dims", "trunc", "min_opacity", "state", "views"]
    assert sig.parameters["min_opacity"].default == 0.5 and sig.parameters["state"].default is None and sig.parameters["views"].default is None
    assert list(inspect.signature(tsdf.sample_colors).parameters) == ["C", "box", "dims", "points"]
    assert inspect.signature(tsdf.export_tsdf_mesh).parameters["colors"].default is True
    sig = inspect.signature(run.train)
    assert sig.parameters["tsdf_colors"].default == "decoder" and sig.parameters["tsdf_mesh"].default == 0
    with pytest.raises(ValueError, match="tsdf_colors"):
        run.train(None, None, tsdf_colors="vertex")


def test_train_cli_tsdf_colors_flag():
    spec = importlib.util.spec_from_file_location("tinynerf_train_cli", os.path.join(ROOT, "train.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    base = ["--data", "d", "--datatype", "synthetic", "--output", "o", "--method", "kplanes"]
    assert cli.parse_args(base).tsdf_colors == "decoder"
    assert cli.parse_args(base + ["--export_tsdf_mesh", "64"]).tsdf_colors == "decoder"
    assert cli.parse_args(base + ["--export_tsdf_mesh", "64", "--tsdf_colors", "decoder"]).tsdf_colors == "decoder"
    assert cli.parse_args(base + ["--tsdf_colors", "decoder"]).tsdf_colors == "decoder"      # the default, spelled out, asks for nothing
    args = cli.parse_args(base + ["--export_tsdf_mesh", "64", "--tsdf_colors", "fused"])
    assert args.tsdf_colors == "fused" and args.export_tsdf_mesh == 64
    assert dict(cli.FLAGS)["--tsdf_colors"]["choices"] == ["decoder", "fused"]
    for extra in (["--tsdf_colors", "fused"], ["--export_tsdf_mesh", "0", "--tsdf_colors", "fused"], ["--export_mesh", "64", "--tsdf_colors", "fused"],
                  ["--export_tsdf_mesh", "64", "--tsdf_colors", "vertex"]):
        with pytest.raises(SystemExit):
            cli.parse_args(base + extra)
    assert "--tsdf_colors" in open(os.path.join(ROOT, "train.py")).read().split("FLAGS = (")[0]      # the FLAGS comment names it
