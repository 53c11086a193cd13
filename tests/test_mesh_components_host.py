"""CPU checks of the mesh-component filter: the yardstick (tests/_mesh_components_ref.py) on hand-worked meshes, the
threshold arithmetic and the argument checks of the host layer without a device, and the new flags and keywords of train.py and
run.train."""
import importlib.util
import inspect
import os

import numpy as np
import pytest
import torch

import _mesh_components_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- yardstick
def test_two_triangles_sharing_nothing():
    labels, counts, stats = ref.components([[0, 1, 2], [3, 4, 5]], 6)
    assert labels.tolist() == [0, 0, 0, 3, 3, 3] and counts.tolist() == [1, 0, 0, 1, 0, 0] and stats == (2, 2, 1)


def test_two_triangles_sharing_one_vertex_or_one_edge():
    labels, counts, stats = ref.components([[4, 1, 2], [2, 3, 0]], 5)              # vertex 2 joins them; the root is the minimum, 0
    assert labels.tolist() == [0] * 5 and counts.tolist() == [2, 0, 0, 0, 0] and stats == (1, 1, 2)
    labels, counts, stats = ref.components([[1, 2, 3], [3, 2, 4]], 5)              # edge 2-3; vertex 0 is in no face
    assert labels.tolist() == [0, 1, 1, 1, 1] and counts.tolist() == [0, 2, 0, 0, 0] and stats == (2, 1, 2)


def test_isolated_vertices_invalid_and_degenerate_faces():
    labels, counts, stats = ref.components(np.zeros((0, 3), np.int32), 3)
    assert labels.tolist() == [0, 1, 2] and counts.tolist() == [0, 0, 0] and stats == (3, 0, 0)
    assert ref.components(np.zeros((0, 3), np.int32), 0)[2] == (0, 0, 0)
    # an invalid face joins nothing and counts nowhere -- not even the two valid indices it names
    faces = [[0, 1, 2], [2, 3, 5], [3, -1, 4], [3, 4, 2 ** 31 - 1]]
    labels, counts, stats = ref.components(faces, 5)
    assert labels.tolist() == [0, 0, 0, 3, 4] and counts.tolist() == [1, 0, 0, 0, 0] and stats == (3, 1, 1)
    assert ref.valid_faces(faces, 5).tolist() == [True, False, False, False]
    # a degenerate face (a, a, b) is an ordinary face: it joins a and b and counts
    labels, counts, stats = ref.components([[3, 3, 1], [0, 0, 0]], 4)
    assert labels.tolist() == [0, 1, 2, 1] and counts.tolist() == [1, 1, 0, 0] and stats == (3, 2, 1)


def test_filter_on_a_hand_worked_mesh():
    # components: {0, 2, 5} with 1 face, {1, 3, 4, 6} with 2 faces, {7} alone; one invalid face
    faces = np.int32([[5, 2, 0], [1, 3, 4], [4, 3, 6], [7, 8, 0]])
    vert = np.arange(24, dtype=np.float32).reshape(8, 3)
    rgb = np.arange(24, dtype=np.uint8).reshape(8, 3)
    v, n, c, f, src, counts = ref.filter_mesh(vert, None, rgb, faces, 2)
    assert src.tolist() == [1, 3, 4, 6] and counts == (4, 2) and n is None
    assert f.tolist() == [[0, 1, 2], [2, 1, 3]] and np.array_equal(v, vert[[1, 3, 4, 6]]) and np.array_equal(c, rgb[[1, 3, 4, 6]])
    v, _, _, f, src, counts = ref.filter_mesh(vert, None, None, faces, 1)
    assert src.tolist() == [0, 1, 2, 3, 4, 5, 6] and f.tolist() == [[5, 2, 0], [1, 3, 4], [4, 3, 6]] and counts == (7, 3)
    v, _, _, f, src, counts = ref.filter_mesh(vert, None, None, faces, 0)              # T = 0: every vertex, every VALID face
    assert src.tolist() == list(range(8)) and f.tolist() == faces[:3].tolist() and counts == (8, 3)
    assert ref.filter_mesh(vert, None, None, faces, 3)[5] == (0, 0)
    assert sorted(ref.pieces(faces, 8)) == [0, 1] and ref.pieces(faces, 8)[1].tolist() == [[1, 3, 4], [4, 3, 6]]


# ---------------------------------------------------------------------------------------------------------------- host layer
def test_threshold_arithmetic():
    from tinynerf_amd.mesh import component_threshold as T
    assert T(0, 0.0, 1000) == 0 and T(7, 0.0, 1000) == 7 and T(0, 1.0, 1000) == 1000 and T(2000, 1.0, 1000) == 2000
    assert T(0, 0.5, 1001) == 501 and T(0, 0.5, 1000) == 500 and T(500, 0.5, 1000) == 500 and T(501, 0.5, 1000) == 501
    assert T(0, 0.25, 3) == 1 and T(0, 1e-9, 5) == 1 and T(0, 1.0, 0) == 0 and T(0, 0.5, 0) == 0
    # exact: the float 0.1 is a little above 1/10, so a tenth of 10 faces rounds up to 2; 1.0 of a count beyond 2^53 is that count
    assert T(0, 0.1, 10) == 2 and T(0, 0.125, 16) == 2 and T(0, 1.0, 2 ** 31 - 2) == 2 ** 31 - 2
    assert T(0, np.float32(0.5), np.int64(11)) == 6 and isinstance(T(np.int64(3), 0.0, 5), int)


@pytest.mark.parametrize("kw", [dict(min_faces=-1), dict(keep_fraction=-0.01), dict(keep_fraction=1.0001), dict(keep_fraction=float("nan")),
                                dict(keep_fraction=float("inf")), dict(min_faces=1.5)])
def test_bad_options_raise_value_error_before_any_device_work(kw):
    from tinynerf_amd import mesh as M
    with pytest.raises(ValueError):
        M.component_threshold(kw.get("min_faces", 0), kw.get("keep_fraction", 0.0), 10)
    z, f = torch.zeros((3, 3)), torch.zeros((1, 3), dtype=torch.int32)             # CPU tensors: the options are checked first
    with pytest.raises(ValueError):
        M.filter_components(z, None, None, f, **kw)

    class Anything:
        world = 1
    with pytest.raises(ValueError):
        M.export_clean_mesh(Anything(), None, **kw)


def test_host_layer_has_no_cpu_path_and_checks_shapes():
    from tinynerf_amd import mesh as M
    z, f = torch.zeros((3, 3)), torch.zeros((1, 3), dtype=torch.int32)
    with pytest.raises(RuntimeError):
        M.components(f, 3)
    with pytest.raises(RuntimeError):
        M.filter_components(z, None, None, f, min_faces=1)
    with pytest.raises(ValueError):
        M.components(f.long(), 3)
    with pytest.raises(ValueError):
        M.components(f, -1)
    with pytest.raises(ValueError):
        M.filter_components(z, torch.zeros((2, 3)), None, f)
    with pytest.raises(ValueError):
        M.filter_components(z, None, torch.zeros((3, 3)), f)                       # colours are bytes

    class TwoRanks:
        world = 2
    with pytest.raises(ValueError, match="world_size"):
        M.export_clean_mesh(TwoRanks(), None, min_faces=1)


def test_signatures_and_defaults():
    from tinynerf_amd import mesh as M, run
    sig = inspect.signature(M.components)
    assert list(sig.parameters) == ["faces", "n_vertices"]
    sig = inspect.signature(M.filter_components)
    assert list(sig.parameters) == ["vertices", "normals", "colors", "faces", "min_faces", "keep_fraction", "return_src"]
    assert sig.parameters["min_faces"].default == 0 and sig.parameters["keep_fraction"].default == 0.0 and sig.parameters["return_src"].default is False
    sig = inspect.signature(M.export_clean_mesh)
    assert list(sig.parameters) == ["trainer", "path", "resolution", "level", "crop", "colors", "min_faces", "keep_fraction"]
    assert sig.parameters["resolution"].default == 256 and sig.parameters["colors"].default is True
    assert sig.parameters["min_faces"].default == 0 and sig.parameters["keep_fraction"].default == 0.0
    assert list(inspect.signature(M.export_mesh).parameters) == ["trainer", "path", "resolution", "level", "crop", "colors"]      # untouched
    sig = inspect.signature(run.train)
    assert sig.parameters["mesh_min_faces"].default == 0 and sig.parameters["mesh_keep_fraction"].default == 0.0
    assert sig.parameters["mesh"].default == 0


def test_train_cli_component_flags():
    spec = importlib.util.spec_from_file_location("tinynerf_train_cli", os.path.join(ROOT, "train.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    base = ["--data", "d", "--datatype", "synthetic", "--output", "o", "--method", "kplanes"]
    args = cli.parse_args(base)
    assert args.mesh_min_faces == 0 and args.mesh_keep_fraction == 0.0 and isinstance(args.mesh_keep_fraction, float)
    args = cli.parse_args(base + ["--export_mesh", "64"])
    assert args.mesh_min_faces == 0 and args.mesh_keep_fraction == 0.0
    args = cli.parse_args(base + ["--export_mesh", "64", "--mesh_min_faces", "100", "--mesh_keep_fraction", "0.25"])
    assert args.export_mesh == 64 and args.mesh_min_faces == 100 and args.mesh_keep_fraction == 0.25
    for extra in (["--mesh_min_faces", "5"], ["--mesh_keep_fraction", "1.0"], ["--export_mesh", "0", "--mesh_min_faces", "5"],
                  ["--export_mesh", "64", "--mesh_min_faces", "-1"], ["--export_mesh", "64", "--mesh_keep_fraction", "1.5"],
                  ["--export_mesh", "64", "--mesh_keep_fraction", "nan"]):
        with pytest.raises(SystemExit):
            cli.parse_args(base + extra)
