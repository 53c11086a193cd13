"""CPU checks of the nerfstudio path: the float64 yardstick (tests/_camera_ref.py) pins itself, the header declares tn_camera_rays and
still says ABI 6, the library exports it and rejects bad arguments before any launch, the ctypes mirror of tn_camera_table has gcc's
layout, INTEGRATION.md names the symbol; data.parse_nerfstudio on captures written to tmp_path (intrinsics, models, image formats,
downscale routes, split rules, pose normalisation); CameraRays refuses 2^31 pixels; train.py carries the new flags and loads a capture
into the two camera-table dataset types."""
import ctypes
import importlib.util
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import _camera_ref as ref
from oracle import tinynerf_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tinynerf_hip.h")


@pytest.fixture(scope="module")
def lib():
    from tinynerf_amd import build
    lib = ctypes.CDLL(build.build(verbose=False))
    lib.tn_last_error_string.restype = ctypes.c_char_p
    return lib


# ------------------------------------------------------------------------------------------------ 1. the yardstick pins itself
@pytest.mark.parametrize("name", sorted(ref.FIXTURES))
def test_fixture_lenses_are_invertible_on_their_image(name):
    """distort(undistort(p)) == p on EVERY pixel of the 1296 x 968 image: a condition on the fixture -- a lens that misses it may not
    be used to judge the kernel"""
    model, L = ref.FIXTURES[name]
    err = ref.round_trip_error(model, L, ref.W, ref.H, step=1)
    print(f"{name}: round trip {err:.3g}")
    assert err <= 1e-12


@pytest.mark.parametrize("name", ["opencv_a", "opencv_b", "opencv_c", "fisheye"])
@pytest.mark.parametrize("w,h", [(648, 484), (324, 242), (640, 478), (96, 64)])
def test_scaled_fixture_lenses_are_invertible(name, w, h):
    model, L = ref.scaled(ref.FIXTURES[name], w, h)
    assert ref.round_trip_error(model, L, w, h) <= 1e-12


def test_the_not_invertible_lens_is_not_a_fixture():
    assert ref.round_trip_error(*ref.NOT_INVERTIBLE, ref.W, ref.H, step=4) > 1e-3


def test_yardstick_iteration_has_converged_long_before_it_stops():
    for name in ("opencv_a", "opencv_b", "opencv_c", "fisheye"):
        model, L = ref.FIXTURES[name]
        u, v = np.meshgrid(np.arange(0, ref.W, 9), np.arange(0, ref.H, 9), indexing="xy")
        xd, yd = ref.normalised(L, u, v)
        a, b = ref.undistort(model, L, xd, yd, iters=8), ref.undistort(model, L, xd, yd, iters=ref.ITERS)
        assert max(np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max()) <= 1e-14


def test_yardstick_without_distortion_is_the_reference_pinhole(monkeypatch):
    """zero coefficients, pinhole and OpenCV: oracle.tinynerf_oracle.generate_rays (the restatement of data.py:48-73 that G12 pins to the
    reference's own output).  The oracle evaluates in float32, so the 1e-12 comparison runs its formula with the float type switched
    to float64 (its only use of the type), and its float32 result is held to float32's own error beside that."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "G12_rays_fixture.npz"))
    fx, fy, cx, cy, w, h = float(g["fx"]), float(g["fy"]), float(g["cx"]) + 1.25, float(g["cy"]) - 0.5, 40, 30
    L = np.array([fx, fy * 1.1, cx / 5, cy / 5, 0, 0, 0, 0, 0, 0], np.float64)
    u, v = np.meshgrid(np.arange(w), np.arange(h), indexing="xy")
    for cam in g["cameras"]:
        o32, d32 = orc.generate_rays(cam, L[0], L[1], L[2], L[3], w, h)
        with monkeypatch.context() as m:
            m.setattr(orc, "f32", np.float64)
            o64, d64 = orc.generate_rays(cam, L[0], L[1], L[2], L[3], w, h)
        assert d64.dtype == np.float64
        for model in (ref.PINHOLE, ref.OPENCV):
            o, d = ref.rays(cam, model, L, u, v)
            assert np.abs(d - d64).max() <= 1e-12 and np.abs(o - o64).max() <= 1e-12, model
            assert np.abs(d - d32).max() <= 1e-6 and np.array_equal(o.astype(np.float32), o32)
    # the fisheye without coefficients is the equidistant lens, not the pinhole: the angle to the axis IS |(xd, yd)|
    d = ref.camera_dirs(ref.FISHEYE, L, u, v)
    xd, yd = ref.normalised(L, u, v)
    assert np.abs(np.arccos(-d[..., 2]) - np.hypot(xd, yd)).max() <= 1e-12 and np.abs(np.linalg.norm(d, axis=-1) - 1.0).max() <= 1e-15
    assert np.abs(d[..., 0] * yd + d[..., 1] * xd).max() <= 1e-15            # same azimuth as the pixel, y flipped


def test_table_rays_walks_images_row_major():
    cams = np.tile(np.eye(4)[None], (3, 1, 1))
    cams[:, :3, 3] = [[1, 2, 3], [4, 5, 6], [7, 8, 9]]
    sizes = [[4, 3], [2, 5], [3, 3]]
    lenses = [ref.lens(10., w=w, h=h) for w, h in sizes]
    o, d, img = ref.table_rays(cams, [0, 0, 0], lenses, sizes, np.arange(12 + 10 + 9))
    assert img.tolist() == [0] * 12 + [1] * 10 + [2] * 9
    assert np.array_equal(o[12], [4, 5, 6]) and np.array_equal(o[-1], [7, 8, 9])
    want = np.array([(1 + 0.5 - 1.0) / 10., -(2 + 0.5 - 2.5) / 10., -1.])            # image 1, pixel 5: u = 1, v = 2
    assert np.abs(d[12 + 5] - want / np.linalg.norm(want)).max() <= 1e-15


# ------------------------------------------------------------------------------------------------ 2. the C ABI
def test_header_declares_the_camera_entry_point():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+tn_camera_rays\s*\(", src)
    assert re.search(r"\btn_camera_table\b", src)
    assert re.search(r"#define TN_ABI_VERSION 6\b", src)


def test_library_exports_the_camera_entry_point(lib):
    assert hasattr(lib, "tn_camera_rays")
    assert hasattr(lib, "tn_gather_rays")
    assert lib.tn_abi_version() == 6


def test_integration_guide_names_the_camera_entry_point():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"\btn_camera_rays\b", text) and re.search(r"\btn_camera_table\b", text)


def test_build_compiles_the_camera_kernels():
    from tinynerf_amd import build
    assert "cameras.hip" in build.sources()


def test_ctypes_table_matches_the_compilers_layout(tmp_path):
    from tinynerf_amd import _lib as L
    fields = [name for name, _ in L.CameraTable._fields_]
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tinynerf_hip.h"\nint main(void) {\n'
                    '    printf("%zu", sizeof(tn_camera_table));\n'
                    + "".join(f'    printf(" %zu", offsetof(tn_camera_table, {f}));\n' for f in fields) + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == ctypes.sizeof(L.CameraTable) == 64
    assert got[1:] == [getattr(L.CameraTable, f).offset for f in fields]
    assert (L.LENS_PINHOLE, L.LENS_OPENCV, L.LENS_FISHEYE) == (0, 1, 2)


def test_camera_rays_rejects_bad_arguments_before_launching(lib):
    from tinynerf_amd import _lib as L
    i64, vp = ctypes.c_int64, ctypes.c_void_p
    fake = 64                                               # never dereferenced: every call below returns before a launch

    def table(n_img=2, n_pixels=100, **kw):
        f = dict(c2w=fake, lens=fake, model=fake, size=fake, pixel_offset=fake, rgb=fake)
        f.update(kw)
        return L.CameraTable(f["c2w"], f["lens"], f["model"], f["size"], f["pixel_offset"], f["rgb"], n_pixels, n_img, 0)

    def call(t=None, idx=None, first=0, stride=1, n=10, o=vp(fake), d=vp(fake), rgb=vp(fake), null_table=False):
        t = table() if t is None else t
        return lib.tn_camera_rays(None if null_table else ctypes.byref(t), idx, i64(first), i64(stride), i64(n), o, d, rgb, None)

    assert call(n=0) == 0                                   # nothing to do: no launch, whatever else is passed
    assert call(n=0, null_table=True) == 0
    assert call(n=-1) == -2                                 # negative size
    assert b"tn_camera_rays" in lib.tn_last_error_string()
    assert call(null_table=True) == -1                      # null pointers
    assert call(o=None) == -1
    assert call(d=None) == -1
    for key in ("c2w", "lens", "model", "size", "pixel_offset"):
        assert call(t=table(**{key: None})) == -1, key
    assert call(t=table(rgb=None)) == -1                    # colours asked for, none in the table
    assert b"tn_camera_rays" in lib.tn_last_error_string()
    assert call(t=table(n_img=0)) == -2                     # empty table
    assert call(t=table(n_img=-3)) == -2
    assert call(t=table(n_pixels=0)) == -2
    # idx == NULL: the whole range is known on the host and must lie inside the table of 100 pixels
    assert call(first=91, n=10) == -2
    assert call(first=100, n=1) == -2
    assert call(first=-1, n=1) == -2
    assert call(first=3, stride=4, n=26) == -2              # 3 + 4 * 25 = 103
    assert call(first=99, stride=-10, n=11) == -2           # walks below 0
    assert call(first=0, stride=2 ** 62, n=3) == -2         # overflows int64
    assert b"outside the table" in lib.tn_last_error_string()


# ------------------------------------------------------------------------------------------------ 3. the loader
def _poses(n, seed=0):
    """cameras somewhere in space, looking roughly at a common point, up roughly along a tilted axis"""
    from tinynerf_amd import rays
    rng = np.random.default_rng(seed)
    c2w = rays.look_at_origin_poses(n, radius=3.0, seed=seed).double().numpy()
    for M in c2w:                                            # (made in float32: orthonormal to 1e-7 only)
        U, _, Vt = np.linalg.svd(M[:3, :3])
        M[:3, :3] = U @ Vt
    tilt = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    tilt *= np.sign(np.linalg.det(tilt))
    world = np.eye(4)
    world[:3, :3] = tilt
    world[:3, 3] = [5.0, -2.0, 11.0]
    return world @ c2w


def _write_capture(root, n=5, size=(24, 16), top=None, per_frame=None, suffix=".png", mode="RGB", extra=None, sizes=None, seed=0):
    from PIL import Image
    rng = np.random.default_rng(seed)
    (root / "images").mkdir(parents=True, exist_ok=True)
    poses = _poses(n, seed)
    frames, pixels = [], []
    for i in range(n):
        w, h = sizes[i] if sizes else size
        px = rng.integers(0, 256, (h, w, 4 if mode == "RGBA" else 3), dtype=np.uint8)
        name = f"images/frame_{i:03d}{suffix}"
        Image.fromarray(px, mode).save(root / name, **({"quality": 95} if suffix != ".png" else {}))
        pixels.append(px)
        frame = {"file_path": name, "transform_matrix": poses[i].tolist()}
        frame.update((per_frame or {}).get(i, {}))
        frames.append(frame)
    meta = {"fl_x": 30.0, "fl_y": 31.0, "cx": size[0] / 2 + 0.25, "cy": size[1] / 2 - 0.5, "w": size[0], "h": size[1]}
    if top is not None:
        meta = dict(top)
    meta["frames"] = frames
    meta.update(extra or {})
    json.dump(meta, open(root / "transforms.json", "w"))
    return poses, pixels


def test_parse_nerfstudio_shared_intrinsics_and_the_holdout_rule(tmp_path):
    from tinynerf_amd import data
    poses, pixels = _write_capture(tmp_path, n=10)
    tr = data.parse_nerfstudio(tmp_path, "train", orient=False)
    va = data.parse_nerfstudio(tmp_path, "val", orient=False)
    te = data.parse_nerfstudio(tmp_path, "test", orient=False)
    assert va.names == te.names == ["images/frame_000.png", "images/frame_008.png"]           # index % 8 == 0
    assert tr.names == [f"images/frame_{i:03d}.png" for i in (1, 2, 3, 4, 5, 6, 7, 9)]
    assert data.parse_nerfstudio(tmp_path, "val", holdout_every=3, orient=False).names == [f"images/frame_{i:03d}.png" for i in (0, 3, 6, 9)]
    assert isinstance(tr.intrinsics, list) and len(tr.intrinsics) == tr.n_img == 8
    K = tr.intrinsics[3]
    assert (K.fx, K.fy, K.cx, K.cy, K.w, K.h) == (30.0, 31.0, 12.25, 7.5, 24, 16)
    assert tr.models == [0] * 8 and tr.lens.shape == (8, 6) and not tr.lens.any()             # no coefficients, no model: PINHOLE
    assert tr.imgs[0].dtype == torch.uint8 and np.array_equal(tr.imgs[0].numpy(), pixels[1])  # kept as bytes
    np.testing.assert_array_equal(tr.cameras.numpy(), poses[[1, 2, 3, 4, 5, 6, 7, 9]].astype(np.float32))
    assert torch.equal(tr.bg_color, torch.ones(3))
    # the json file itself is accepted too; an unsorted frame list is sorted by file_path first
    meta = json.load(open(tmp_path / "transforms.json"))
    meta["frames"] = meta["frames"][::-1]
    json.dump(meta, open(tmp_path / "reversed.json", "w"))
    assert data.parse_nerfstudio(tmp_path / "reversed.json", "val", orient=False).names == va.names
    with pytest.raises(ValueError):
        data.parse_nerfstudio(tmp_path, "nonsense")


def test_parse_nerfstudio_split_lists(tmp_path):
    from tinynerf_amd import data
    names = [f"images/frame_{i:03d}.png" for i in range(6)]
    _write_capture(tmp_path, n=6, extra={"train_filenames": names[:4], "val_filenames": [names[4]], "test_filenames": names[4:]})
    assert data.parse_nerfstudio(tmp_path, "train").names == names[:4]
    assert data.parse_nerfstudio(tmp_path, "val").names == [names[4]]
    assert data.parse_nerfstudio(tmp_path, "test").names == names[4:]
    meta = json.load(open(tmp_path / "transforms.json"))
    del meta["val_filenames"]
    json.dump(meta, open(tmp_path / "transforms.json", "w"))
    with pytest.raises(ValueError, match="val"):
        data.parse_nerfstudio(tmp_path, "val")               # the json lists its splits and has nothing for this one


def test_parse_nerfstudio_per_frame_cameras_and_the_default_model_rule(tmp_path):
    from tinynerf_amd import data
    per_frame = {
        0: {"fl_x": 40.0, "fl_y": 41.0, "cx": 9.0, "cy": 5.0, "w": 20, "h": 12, "camera_model": "OPENCV_FISHEYE", "k1": 0.01, "k4": -0.002},
        1: {"k2": 0.03, "p2": 1e-3},                                       # coefficients, no model of its own -> inherits the top level's
        2: {"camera_model": "PINHOLE"},
        3: {"camera_model": "SIMPLE_RADIAL", "k1": -0.05},
    }
    top = {"fl_x": 30.0, "fl_y": 30.5, "cx": 12.0, "cy": 8.0, "w": 24, "h": 16, "camera_model": "OPENCV", "k1": 0.1, "p1": 2e-3}
    _write_capture(tmp_path, n=5, top=top, per_frame=per_frame, sizes=[(20, 12)] + [(24, 16)] * 4, extra={"train_filenames": [f"images/frame_{i:03d}.png" for i in range(5)]})
    nd = data.parse_nerfstudio(tmp_path, "train")
    assert nd.models == [2, 1, 0, 1, 1]
    K0, K1 = nd.intrinsics[0], nd.intrinsics[1]
    assert (K0.fx, K0.fy, K0.cx, K0.cy, K0.w, K0.h) == (40.0, 41.0, 9.0, 5.0, 20, 12)
    assert (K1.fx, K1.fy, K1.cx, K1.cy, K1.w, K1.h) == (30.0, 30.5, 12.0, 8.0, 24, 16)
    assert nd.imgs[0].shape == (12, 20, 3) and nd.imgs[1].shape == (16, 24, 3)              # mixed sizes in one split
    lens = nd.lens.double().numpy()
    np.testing.assert_allclose(lens[0], [0.01, 0, 0, -0.002, 2e-3, 0], atol=1e-9)           # k1, k4 its own; p1 from the top level
    np.testing.assert_allclose(lens[1], [0.1, 0.03, 0, 0, 2e-3, 1e-3], atol=1e-9)
    np.testing.assert_allclose(lens[3], [-0.05, 0, 0, 0, 2e-3, 0], atol=1e-9)
    # no camera_model anywhere: OPENCV exactly where a coefficient is non-zero
    sub = tmp_path / "defaults"
    _write_capture(sub, n=3, top={"fl_x": 30.0, "w": 24, "h": 16}, per_frame={1: {"k3": 1e-4}, 2: {"p1": 0.0}},
                   extra={"train_filenames": [f"images/frame_{i:03d}.png" for i in range(3)]})
    nd = data.parse_nerfstudio(sub, "train")
    assert nd.models == [0, 1, 0]
    K = nd.intrinsics[0]
    assert (K.fx, K.fy, K.cx, K.cy) == (30.0, 30.0, 12.0, 8.0)                              # fl_y = fl_x, centre of the image
    # the split becomes a camera table: per-image rows
    src = nd.camera_rays("cpu")
    assert (src.n_img, src.n_rays) == (3, 3 * 24 * 16) and src.lens.shape == (3, 10) and src.rgb.shape == (3 * 24 * 16, 3)
    assert src.model.tolist() == [0, 1, 0] and src.size.tolist() == [[24, 16]] * 3 and src.pixel_offset.tolist() == [0, 384, 768, 1152]
    assert abs(float(src.lens[1, 6]) - 1e-4) < 1e-10 and src.table.n_pixels == 1152 and src.table.n_img == 3


def test_parse_nerfstudio_unknown_model_raises_its_name(tmp_path):
    from tinynerf_amd import data
    _write_capture(tmp_path, n=3, per_frame={2: {"camera_model": "EQUIRECTANGULAR"}})
    with pytest.raises(NotImplementedError, match="EQUIRECTANGULAR"):
        data.parse_nerfstudio(tmp_path, "train")
    with pytest.raises(NotImplementedError, match="EQUIRECTANGULAR"):
        data.parse_nerfstudio(tmp_path, "val")              # (frame 2 is not in this split: the capture as a whole is refused)


def test_parse_nerfstudio_image_formats(tmp_path):
    from PIL import Image
    from tinynerf_amd import data
    # RGBA over a colour: exactly the synthetic loader's compositing
    _, pixels = _write_capture(tmp_path / "rgba", n=2, mode="RGBA", extra={"train_filenames": ["images/frame_000.png", "images/frame_001.png"]})
    bg = (255, 128, 0)
    nd = data.parse_nerfstudio(tmp_path / "rgba", "train", bg_color=bg)
    with Image.open(tmp_path / "rgba" / "images" / "frame_001.png") as img:
        want = data._composite_over(img, bg)
    assert nd.imgs[1].dtype == torch.uint8
    assert torch.equal(data._as_float(nd.imgs[1]), want)                  # the same float32 bits once divided by 255
    assert torch.equal(nd.bg_color, torch.tensor(bg, dtype=torch.float) / 255.)
    # JPEG, and a file_path without its suffix
    _write_capture(tmp_path / "jpeg", n=2, suffix=".jpg", extra={"train_filenames": ["images/frame_000", "images/frame_001"]})
    meta = json.load(open(tmp_path / "jpeg" / "transforms.json"))
    for f in meta["frames"]:
        f["file_path"] = f["file_path"][:-4]
    json.dump(meta, open(tmp_path / "jpeg" / "transforms.json", "w"))
    nd = data.parse_nerfstudio(tmp_path / "jpeg", "train")
    with Image.open(tmp_path / "jpeg" / "images" / "frame_000.jpg") as img:
        assert np.array_equal(nd.imgs[0].numpy(), np.asarray(img.convert("RGB")))
    # an image that is not the size the json states is refused at full resolution
    _write_capture(tmp_path / "wrong", n=2, sizes=[(24, 16), (20, 16)], extra={"train_filenames": ["images/frame_000.png", "images/frame_001.png"]})
    with pytest.raises(ValueError, match="20 x 16"):
        data.parse_nerfstudio(tmp_path / "wrong", "train")


def test_parse_nerfstudio_downscale_routes(tmp_path):
    from PIL import Image
    from tinynerf_amd import data
    names = [f"images/frame_{i:03d}.png" for i in range(2)]
    _, pixels = _write_capture(tmp_path, n=2, size=(48, 32), extra={"train_filenames": names})
    full = data.parse_nerfstudio(tmp_path, "train")
    # 1. no images_2/: box filter of the decoded image
    nd = data.parse_nerfstudio(tmp_path, "train", downscale=2)
    K, K1 = nd.intrinsics[0], full.intrinsics[0]
    assert (K.w, K.h) == (24, 16) and nd.imgs[0].shape == (16, 24, 3)
    assert (K.fx, K.fy, K.cx, K.cy) == (K1.fx / 2, K1.fy / 2, K1.cx / 2, K1.cy / 2)
    assert np.array_equal(nd.imgs[0].numpy(), np.asarray(Image.fromarray(pixels[0]).reduce(2)))
    # 2. images_4/ exists: its files are taken as they are, w and h from them (a folder that rounds the size its own way)
    (tmp_path / "images_4").mkdir()
    rng = np.random.default_rng(7)
    small = [rng.integers(0, 256, (8, 13, 3), dtype=np.uint8) for _ in range(2)]
    for i in range(2):
        Image.fromarray(small[i]).save(tmp_path / "images_4" / f"frame_{i:03d}.png")
    nd = data.parse_nerfstudio(tmp_path, "train", downscale=4)
    K = nd.intrinsics[1]
    assert (K.w, K.h) == (13, 8) and np.array_equal(nd.imgs[1].numpy(), small[1])
    assert (K.fx, K.fy, K.cx, K.cy) == (K1.fx / 4, K1.fy / 4, K1.cx / 4, K1.cy / 4)
    with pytest.raises(ValueError):
        data.parse_nerfstudio(tmp_path, "train", downscale=0)


def test_orient_poses_closed_forms(tmp_path):
    from tinynerf_amd import data
    poses = _poses(9, seed=3)
    out = data.orient_poses(poses)
    t = out[:, :3, 3]
    assert np.abs(t.mean(0)).max() <= 1e-12                              # mean position 0
    assert abs(np.abs(t).max() - 1.0) <= 1e-12                           # largest coordinate 1
    up = out[:, :3, 1].mean(0)
    assert np.abs(up / np.linalg.norm(up) - [0., 0., 1.]).max() <= 1e-12  # mean up = +z
    for M in out:                                                        # still rotations
        assert np.abs(M[:3, :3] @ M[:3, :3].T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(M[:3, :3]) - 1.0) <= 1e-12
        assert np.array_equal(M[3], [0., 0., 0., 1.])
    # ONE similarity: relative rotations are unchanged, relative positions scale by one factor
    scale = 1.0 / np.abs((poses[:, :3, 3] - poses[:, :3, 3].mean(0)) @ np.eye(3)).max()
    for i in range(1, 9):
        rel_in = poses[0, :3, :3].T @ poses[i, :3, :3]
        rel_out = out[0, :3, :3].T @ out[i, :3, :3]
        assert np.abs(rel_in - rel_out).max() <= 1e-12
        # position of camera i in camera 0's frame
        p_in = poses[0, :3, :3].T @ (poses[i, :3, 3] - poses[0, :3, 3])
        p_out = out[0, :3, :3].T @ (out[i, :3, 3] - out[0, :3, 3])
        ratio = np.linalg.norm(p_out) / np.linalg.norm(p_in)
        assert np.abs(p_out - ratio * p_in).max() <= 1e-12
        if i == 1:
            first = ratio
        assert abs(ratio - first) <= 1e-12
    # cameras hanging upside down (mean up = -z): half a turn, not a division by zero
    flipped = poses.copy()
    flipped[:, :3, :3] = np.diag([1., -1., -1.]) @ data.orient_poses(poses)[:, :3, :3]
    flipped[:, :3, 3] = data.orient_poses(poses)[:, :3, 3] @ np.diag([1., -1., -1.])
    again = data.orient_poses(flipped)
    up = again[:, :3, 1].mean(0)
    assert np.isfinite(again).all() and np.abs(up / np.linalg.norm(up) - [0., 0., 1.]).max() <= 1e-9
    del scale


def test_parse_nerfstudio_orients_once_over_all_frames(tmp_path):
    from tinynerf_amd import data
    poses, _ = _write_capture(tmp_path, n=10)
    want = data.orient_poses(poses)                                      # all ten frames, not the split's
    tr, va = data.parse_nerfstudio(tmp_path, "train"), data.parse_nerfstudio(tmp_path, "val")
    np.testing.assert_array_equal(tr.cameras.numpy(), want[[1, 2, 3, 4, 5, 6, 7, 9]].astype(np.float32))
    np.testing.assert_array_equal(va.cameras.numpy(), want[[0, 8]].astype(np.float32))
    assert "applied_transform" in inspect.getdoc(data.parse_nerfstudio) and "mask" in inspect.getdoc(data.parse_nerfstudio)


def test_synthetic_loader_and_nerfdata_defaults_are_unchanged():
    from tinynerf_amd import data, rays
    nd = data.NerfData(cameras=rays.look_at_origin_poses(2), intrinsics=rays.Intrinsics(20., 20., 4., 3., 8, 6))
    assert nd.lens is None and nd.models is None and nd.names is None
    o, d = nd.generate_rays()
    assert o.shape == (2, 6, 8, 3)
    assert data.PoseDataset(nd).img_intrinsics(1) is nd.intrinsics
    per_image = data.NerfData(cameras=nd.cameras, intrinsics=[nd.intrinsics, nd.intrinsics])
    with pytest.raises(ValueError, match="CameraRaysDataset"):
        per_image.generate_rays()


# ------------------------------------------------------------------------------------------------ 4. CameraRays and the command line
def test_camera_rays_refuses_two_to_the_31_pixels():
    """a faked size table: the check runs before anything is allocated"""
    from tinynerf_amd import rays
    sizes = [[65536, 16384]] * 2                            # 2 x 2^30 pixels
    with pytest.raises(ValueError, match="--downscale"):
        rays.CameraRays(None, None, None, sizes, None, "cpu")
    with pytest.raises(ValueError, match="--downscale"):
        rays.CameraRays(None, None, None, [[46341, 46341]], None, "cpu")       # 46341^2 = 2^31 + 4633
    assert rays.CameraRays.MAX_PIXELS == 2 ** 31


def test_camera_rays_checks_its_table_without_a_gpu():
    from tinynerf_amd import rays
    c2w, lens = torch.eye(4)[None], torch.tensor([[10., 10., 2., 2., 0, 0, 0, 0, 0, 0]])
    src = rays.CameraRays(c2w, lens, [0], [[4, 4]], None, "cpu")
    assert (src.n_img, src.n_rays, src.rgb) == (1, 16, None) and src.c2w.shape == (1, 3, 4)
    with pytest.raises(ValueError):
        rays.CameraRays(c2w, lens, [3], [[4, 4]], None, "cpu")                   # no such model
    with pytest.raises(ValueError):
        rays.CameraRays(c2w, lens, [0], [[4, 4]], [torch.zeros(4, 5, 3, dtype=torch.uint8)], "cpu")
    with pytest.raises(ValueError):
        rays.CameraRays(c2w, lens, [0], [[4, 0]], None, "cpu")
    with pytest.raises(RuntimeError, match="CUDA"):                              # no CPU path
        src.gather(None, torch.zeros(16, 3), torch.zeros(16, 3), n=16)
    with pytest.raises(ValueError, match="no colours"):
        src.image_rgb(0)


def test_trainer_signature_keeps_its_positional_arguments():
    from tinynerf_amd import run
    params = inspect.signature(run.Trainer.__init__).parameters
    assert list(params)[:9] == ["self", "cfg", "rays_o", "rays_d", "rgbs", "bg_color", "device", "rank", "world_size"]
    assert params["ray_source"].kind is inspect.Parameter.KEYWORD_ONLY and params["ray_source"].default is None


def _train_cli():
    spec = importlib.util.spec_from_file_location("tinynerf_train_cli", os.path.join(ROOT, "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_cli_loads_a_capture_into_camera_tables(tmp_path):
    from tinynerf_amd import data
    cli = _train_cli()
    base = ["--data", str(tmp_path), "--datatype", "nerfstudio", "--output", "o", "--method", "kplanes"]
    args = cli.parse_args(base)
    assert (args.downscale, args.holdout_every) == (1, 8)
    args = cli.parse_args(base + ["--downscale", "2", "--holdout_every", "4"])
    assert (args.downscale, args.holdout_every) == (2, 4)
    _write_capture(tmp_path, n=9, size=(48, 32))
    train_rays, eval_set, test_set = cli.load_datasets(args, "cpu")
    assert type(train_rays) is data.CameraRaysDataset and type(eval_set) is data.CameraPoseDataset and type(test_set) is data.CameraPoseDataset
    assert len(train_rays) == 6 * 24 * 16 and len(eval_set) == len(test_set) == 3           # frames 0, 4, 8 held out; images halved
    assert train_rays.source.n_rays == len(train_rays) and bool(test_set.rgbs) and len(test_set.rgbs) == 3
    K = test_set.img_intrinsics(2)
    assert (K.w, K.h, K.fx) == (24, 16, 15.0)
    assert torch.equal(train_rays.bg_color, torch.ones(3)) and np.isfinite(train_rays.scene_scale)
    pose_only = data.CameraPoseDataset(data.NerfData(cameras=torch.eye(4).repeat(2, 1, 1), intrinsics=K), "cpu")
    assert not pose_only.rgbs and len(pose_only) == 2
