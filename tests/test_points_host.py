"""CPU checks of the point-cloud export: the PLY writer and reader round trip bit for bit in the one dialect they speak, the header
declares tn_points_compact / tn_points_workspace_bytes and still says ABI 6, the library sizes the workspace and rejects bad
arguments before any launch, the yardstick (tests/_points_ref.py) and the input generator of the GPU tests do what they promise,
and train.py carries the two flags."""
import ctypes
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest
import torch

import _points_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tinynerf_hip.h")
NEW = ("tn_points_compact", "tn_points_workspace_bytes")
PLY_HEADER = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")


@pytest.fixture(scope="module")
def lib():
    from tinynerf_amd import build
    lib = ctypes.CDLL(build.build(verbose=False))
    lib.tn_last_error_string.restype = ctypes.c_char_p
    return lib


# ---------------------------------------------------------------------------------------------------------------- PLY
@pytest.mark.parametrize("m", [0, 1, 1000])
def test_ply_round_trip_is_bit_exact(tmp_path, m):
    from tinynerf_amd import points as P
    rng = np.random.default_rng(m)
    xyz = rng.standard_normal((m, 3)).astype(np.float32)
    if m:
        xyz[0] = [-0.0, np.float32(1e-42), np.float32(np.finfo(np.float32).max)]          # signed zero, a subnormal, the largest
    rgb = rng.integers(0, 256, (m, 3)).astype(np.uint8)
    path = tmp_path / "cloud.ply"
    P.write_ply(path, xyz, rgb)
    raw = open(path, "rb").read()
    head = (PLY_HEADER % m).encode("ascii")
    assert raw.startswith(head) and len(raw) == len(head) + 15 * m
    body = np.frombuffer(raw[len(head):], np.uint8).reshape(m, 15)
    assert np.array_equal(body[:, :12].copy().view("<f4").view(np.uint32), xyz.view(np.uint32))     # x y z, then the three bytes
    assert np.array_equal(body[:, 12:], rgb)
    got_xyz, got_rgb = P.read_ply(path)
    assert got_xyz.dtype == np.float32 and got_xyz.shape == (m, 3) and got_rgb.dtype == np.uint8 and got_rgb.shape == (m, 3)
    assert np.array_equal(got_xyz.view(np.uint32), xyz.view(np.uint32)) and np.array_equal(got_rgb, rgb)
    P.write_ply(path, torch.from_numpy(xyz), torch.from_numpy(rgb))                       # tensors write the same file
    assert open(path, "rb").read() == raw


def test_read_ply_refuses_other_dialects(tmp_path):
    from tinynerf_amd import points as P
    path = tmp_path / "cloud.ply"
    P.write_ply(path, np.zeros((2, 3), np.float32), np.zeros((2, 3), np.uint8))
    raw = open(path, "rb").read()
    for bad in (raw.replace(b"binary_little_endian", b"ascii"), raw.replace(b"property uchar red\n", b""), raw[:-1], raw + b"\0",
                raw.replace(b"end_header\n", b"")):
        open(path, "wb").write(bad)
        with pytest.raises(ValueError):
            P.read_ply(path)
    with pytest.raises(ValueError):
        P.write_ply(path, np.zeros((2, 3), np.float32), np.zeros((3, 3), np.uint8))


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_header_declares_the_points_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
    assert re.search(r"#define TN_ABI_VERSION 6\b", src)


def test_library_exports_and_the_guide_names_the_points_entry_points(lib):
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert re.search(r"\b" + name + r"\b", text), name
    from tinynerf_amd import build
    assert build.SOURCES["points.hip"] == build.SOURCES["cameras.hip"]


WORKSPACE_N = list(range(0, 1100)) + [4099, 65536 + 257, 640000, 2 ** 20 + 13, 2 ** 31 - 1]


def test_workspace_bytes(lib):
    q, i64 = lib.tn_points_workspace_bytes, ctypes.c_int64
    out = i64(-1)
    prev = 0
    for n in WORKSPACE_N:
        assert q(i64(n), ctypes.byref(out)) == 0
        assert out.value >= 8 * -(-n // 64) + 8 * -(-n // 256) and out.value >= prev and out.value % 8 == 0
        prev = out.value
    assert out.value < 2 ** 31 - 1                                 # 5/32 of a byte per ray
    assert q(i64(0), ctypes.byref(out)) == 0 and out.value == 0
    assert q(i64(8), None) == -1 and b"tn_points_workspace_bytes" in lib.tn_last_error_string()
    assert q(i64(-1), ctypes.byref(out)) == -2
    assert q(i64(2 ** 31), ctypes.byref(out)) == -2


def test_workspace_bytes_are_the_shared_layout(lib):
    """per workgroup of 256 rays 4 waves x 1 ballot and 1 count of 8 B each: the layout the mesh and filter workspaces start with"""
    out = ctypes.c_int64(-1)
    for n in WORKSPACE_N:
        assert lib.tn_points_workspace_bytes(ctypes.c_int64(n), ctypes.byref(out)) == 0
        assert out.value == 40 * -(-n // 256), n


def test_compact_rejects_bad_arguments_before_launching(lib):
    """every call below returns before a launch: the pointers are never dereferenced and no device is touched"""
    i64, f32, vp = ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
    fake = vp(64)

    def call(n=4, capacity=4, min_opacity=0.5, inputs=(fake,) * 5, outputs=(fake,) * 3, count=fake, work=fake, bg=None, box=None):
        return lib.tn_points_compact(*inputs, bg, box, f32(min_opacity), i64(n), i64(capacity), *outputs, count, work, None)

    # null required pointers: each input, each output with capacity > 0, count, the workspace
    for k in range(5):
        assert call(inputs=(fake,) * k + (None,) + (fake,) * (4 - k)) == -1, k
        assert b"tn_points_compact" in lib.tn_last_error_string() and b"null" in lib.tn_last_error_string()
    for k in range(3):
        assert call(outputs=(fake,) * k + (None,) + (fake,) * (2 - k)) == -1, k
    assert call(count=None) == -1
    assert call(n=0, count=None) == -1                             # count is written for n == 0 too
    assert call(work=None) == -1
    # sizes
    assert call(n=-1) == -2
    assert call(capacity=-1) == -2
    assert call(n=2 ** 31) == -2 and b"2^31" in lib.tn_last_error_string()
    assert call(n=-1, inputs=(None,) * 5, outputs=(None,) * 3, count=None, work=None) == -2         # as tn_weights_fwd: the size first
    # min_opacity must be > 0: the colour is divided by the opacity
    for bad in (0.0, -0.0, -0.5, float("nan"), float("-inf")):
        assert call(min_opacity=bad) == -3, bad
        assert b"min_opacity must be > 0" in lib.tn_last_error_string()
    # alignment, as the other entry points with 8-byte items
    assert call(work=vp(68)) == -4
    assert call(count=vp(68)) == -4


# ---------------------------------------------------------------------------------------------------------------- yardstick
def test_yardstick_on_hand_computed_rays():
    o = np.zeros((6, 3), np.float32)
    d = np.tile(np.float32([1, 0, 0]), (6, 1))
    depth = np.float32([0.5, 0.5, 0.75, np.nan, -1.0, 0.25])
    opacity = np.float32([0.5, 0.25, 1.0, 1.0, 1.0, np.nan])
    rgb = np.tile(np.float32([0.75, 0.5, 1.0]), (6, 1))
    box = [-1, -1, -1, 0.5, 1, 1]
    src, p, col, val = ref.compact(o, d, rgb, opacity, depth, [1, 1, 1], box, 0.5)
    assert src.tolist() == [0] and p.tolist() == [[0.5, 0.0, 0.0]]                 # 1: opacity; 2: beyond hi_x; 3, 4: depth; 5: NaN opacity
    assert col.tolist() == [[128, 0, 255]]                                         # (0.75 - 0.5) / 0.5 = 0.5 -> 128; (0.5 - 0.5) / 0.5; 1
    src, p, col, _ = ref.compact(o, d, rgb, opacity, depth, None, None, 0.25)
    assert src.tolist() == [0, 1, 2] and col[1].tolist() == [255, 255, 255] and col[2].tolist() == [191, 128, 255]
    big = np.float32([1e30])
    assert not ref.keep_mask(np.zeros((1, 3), np.float32), np.float32([[1e30, 0, 0]]), np.float32([1]), big, None, 0.5)[0]      # inf in fp32


def test_gpu_test_inputs_stay_clear_of_every_threshold():
    """the generator of tests/test_hip_points.py: no point within 1e-4 of a box face, no opacity within 1e-6 of min_opacity -- the
    fp32 and the fp64 predicate cannot differ through rounding -- and each keep pattern is what its name says"""
    import test_hip_points as T
    for n in (1, 63, 257, 4099):
        for pattern in T.PATTERNS:
            c = T.make_case(n, pattern, seed=n)
            p = ref.points64(c["rays_o"], c["rays_d"], c["depth"])
            face = np.minimum(np.abs(p - np.float64(T.BOX[:3])), np.abs(p - np.float64(T.BOX[3:])))
            assert face.min() > 1e-4 and np.abs(c["opacity"].astype(np.float64) - T.MIN_OPACITY).min() > 1e-6
            keep = ref.keep_mask(c["rays_o"], c["rays_d"], c["opacity"], c["depth"], T.BOX, T.MIN_OPACITY)
            assert np.array_equal(keep, c["want"]), (n, pattern)
            want = {"all": n, "none": 0, "first": 1, "last": 1, "alternating": (n + 1) // 2}.get(pattern)
            if want is not None:
                assert keep.sum() == want
            if n == 4099 and pattern.startswith("random"):
                frac = keep.mean()
                assert (0.4 < frac < 0.6) if pattern == "random50" else (0.002 < frac < 0.03)
            # rays are dropped for either reason: some by the opacity, some by the box
            if pattern == "random50" and n == 4099:
                inside = ((p >= T.BOX[:3]) & (p <= T.BOX[3:])).all(1)
                assert (~inside).any() and (c["opacity"] < T.MIN_OPACITY).any() and (inside & (c["opacity"] < T.MIN_OPACITY)).any()


# ---------------------------------------------------------------------------------------------------------------- Python layers, CLI
def test_python_layers_take_the_new_keywords():
    from tinynerf_amd import points as P, run
    sig = inspect.signature(P.compact_points)
    assert list(sig.parameters) == ["rays_o", "rays_d", "maps", "bg", "box", "min_opacity", "depth", "capacity"]
    assert sig.parameters["min_opacity"].default == 0.5 and sig.parameters["depth"].default == "expected" and sig.parameters["capacity"].default is None
    sig = inspect.signature(P.export_pointcloud)
    assert list(sig.parameters) == ["trainer", "dataset", "indices", "path", "n_points", "min_opacity", "depth", "crop", "seed", "rendered"]
    assert sig.parameters["n_points"].default == 1_000_000 and sig.parameters["crop"].default is None and sig.parameters["seed"].default == 0
    sig = inspect.signature(run.train)
    assert sig.parameters["pointcloud"].default == 0 and sig.parameters["pointcloud_crop"].default is None


def test_host_layer_checks_its_arguments_without_a_gpu():
    from tinynerf_amd import points as P
    o = torch.zeros(4, 3)
    maps = {"rgb": torch.zeros(4, 3), "opacity": torch.ones(4), "depth": torch.ones(4), "median_depth": torch.ones(4)}
    with pytest.raises(RuntimeError):
        P.compact_points(o, o, maps, None)                         # no CPU path
    with pytest.raises(ValueError):
        P.compact_points(o, o, maps, None, depth="mean")
    with pytest.raises(ValueError):
        P.compact_points(o, o, maps, None, min_opacity=0.0)
    with pytest.raises(RuntimeError):
        P.compact_points(o, o[:3], maps, None)

    class TwoRanks:
        world = 2
    with pytest.raises(ValueError, match="world_size"):
        P.export_pointcloud(TwoRanks(), [])


def test_default_crop_is_the_marchers_uniform_box():
    from tinynerf_amd import points as P
    from tinynerf_amd.run import TrainConfig
    assert P.default_crop(TrainConfig(method="kplanes", scene_type="aabb")) == [-1.5] * 3 + [1.5] * 3
    assert P.default_crop(TrainConfig(method="kplanes", scene_type="unbounded", scene_scale=2.5)) == [-2.5] * 3 + [2.5] * 3


def test_train_cli_pointcloud_flags():
    spec = importlib.util.spec_from_file_location("tinynerf_train_cli", os.path.join(ROOT, "train.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    base = ["--data", "d", "--datatype", "synthetic", "--output", "o", "--method", "kplanes"]
    args = cli.parse_args(base)
    assert args.export_pointcloud == 0 and args.pointcloud_crop is None
    args = cli.parse_args(base + ["--export_pointcloud", "5000", "--pointcloud_crop", "-1", "-1", "-0.5", "1", "1", "0.5"])
    assert args.export_pointcloud == 5000 and args.pointcloud_crop == [-1.0, -1.0, -0.5, 1.0, 1.0, 0.5]
    with pytest.raises(SystemExit):
        cli.parse_args(base + ["--pointcloud_crop", "0", "1"])
