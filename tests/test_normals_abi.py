"""CPU checks of the surface-normal feature's boundary: the header declares the three entry points and tn_normal_frame and still says
ABI 6, the library exports them and rejects every bad argument before any launch (no GPU is touched), INTEGRATION.md names them, the
Python layers and the command line carry the keyword with its default off, and the PLY dialect with normals round-trips bit for bit."""
import ctypes
import importlib.util
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tinynerf_hip.h")
NEW = ("tn_kplanes_normals", "tn_hashgrid_normals", "tn_ray_normals")
PLY_HEADER_N = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                "property float nx\nproperty float ny\nproperty float nz\n"
                "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")


@pytest.fixture(scope="module")
def lib():
    from tinynerf_amd import build
    lib = ctypes.CDLL(build.build(verbose=False))
    lib.tn_last_error_string.restype = ctypes.c_char_p
    return lib


def test_header_declares_the_entry_points_and_keeps_the_abi_version():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
    assert re.search(r"#define TN_ABI_VERSION 6\b", src)
    assert re.search(r"TN_CONTRACT_NONE\s*=\s*3\b", src) and re.search(r"\btn_normal_frame\b", src)


def test_library_exports_and_the_guide_names_the_entry_points(lib):
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert re.search(r"\b" + name + r"\b", text), name
    from tinynerf_amd import build
    assert build.SOURCES["normals.hip"] == build.FAST                      # kplanes.hip's flags without the atomics flag
    assert build.SOURCES["kplanes.hip"] == build.FAST + ["-munsafe-fp-atomics"]


def test_normal_frame_has_the_c_layout(tmp_path):
    from tinynerf_amd import _lib as L
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tinynerf_hip.h"\n'
                    'int main(){printf("%zu %zu %zu %zu %d\\n", sizeof(tn_normal_frame), offsetof(tn_normal_frame, contraction),'
                    'offsetof(tn_normal_frame, reserved), offsetof(tn_normal_frame, aabb), (int)TN_CONTRACT_NONE);return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(L.NormalFrame), L.NormalFrame.contraction.offset, L.NormalFrame.reserved.offset, L.NormalFrame.aabb.offset,
                   L.CONTRACT_NONE]
    assert got[0] == 32


# ------------------------------------------------------------------------------------------------------------ argument checks
FAKE = 64                                   # a 16-byte aligned address that is never dereferenced


def _head(F, **kw):
    from tinynerf_amd import _lib as L
    d = L.MlpDesc()
    d.n_layers, d.in_dim, d.encoding = 2, F, L.ENC_NONE
    d.dims[0], d.dims[1], d.dims[2] = F, 64, 1
    d.weights[0] = d.weights[1] = d.biases[0] = d.biases[1] = FAKE
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _kplanes(n_scales=3, channels=32, missing=None, plane=FAKE):
    from tinynerf_amd import _lib as L
    d = L.KPlanesDesc()
    d.n_scales, d.channels = n_scales, channels
    for s in range(min(n_scales, 4)):
        d.height[s] = d.width[s] = 8
        for p in range(3):
            d.planes[s][p] = None if missing == (s, p) else plane
    return d


def _hashgrid(features=2, table=FAKE):
    from tinynerf_amd import _lib as L
    d = L.HashGridDesc()
    d.n_levels, d.features = 2, features
    d.res[0], d.res[1] = 2, 4
    d.entries[0], d.entries[1] = 32, 128
    d.offset[0], d.offset[1] = 0, 32
    d.table = table
    return d


def _frame(kind=3, box=(-1, -1, -1, 1, 1, 1)):
    from tinynerf_amd import _lib as L
    f = L.NormalFrame(contraction=kind)
    for i in range(6):
        f.aabb[i] = box[i]
    return f


def _call(lib, fn, desc, head, frame=None, x=FAKE, stride=7, n=40, gate=None, normals=FAKE, grad=FAKE):
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    return getattr(lib, fn)(None if desc is None else ctypes.byref(desc), vp(x), i64(stride), i64(n),
                            None if head is None else ctypes.byref(head), None if frame is None else ctypes.byref(frame), vp(gate),
                            vp(normals), vp(grad), None)


def test_sample_entry_points_reject_bad_arguments_before_launching(lib):
    """every call below returns before a launch: the pointers are never dereferenced and no device is touched"""
    for fn, desc, F in (("tn_kplanes_normals", _kplanes(), 96), ("tn_hashgrid_normals", _hashgrid(), 4)):
        ok_head = _head(F)
        # n == 0: TN_OK without a launch, whatever the data pointers are
        assert _call(lib, fn, desc, ok_head, _frame(), x=None, n=0, normals=None, grad=None) == 0
        assert _call(lib, fn, desc, ok_head, None, n=0) == 0                                  # a NULL frame is the none frame
        # null pointers
        assert _call(lib, fn, None, ok_head) == -1
        assert _call(lib, fn, desc, None) == -1
        assert _call(lib, fn, desc, ok_head, x=None) == -1
        assert _call(lib, fn, desc, ok_head, normals=None, grad=None) == -1 and b"normals" in lib.tn_last_error_string()
        bad = _head(F)
        bad.weights[1] = None
        assert _call(lib, fn, desc, bad) == -1
        # sizes
        assert _call(lib, fn, desc, ok_head, n=-1) == -2
        assert _call(lib, fn, desc, ok_head, stride=2) == -2
        # the head
        for kw in (dict(n_layers=3), dict(n_layers=1), dict(encoding=1), dict(in_dim=F + 4)):
            assert _call(lib, fn, desc, _head(F, **kw)) == -3, kw
        for dims in ((F + 4, 64, 1), (F, 32, 1), (F, 64, 3)):
            h = _head(F)
            h.dims[0], h.dims[1], h.dims[2] = dims
            assert _call(lib, fn, desc, h) == -3, dims
        assert b"64" in lib.tn_last_error_string()
        flagged = _head(F, flags=64 | 512, out_activation=2)                                   # flags and the activation are ignored
        assert _call(lib, fn, desc, flagged, n=0) == 0
        # the frame
        assert _call(lib, fn, desc, ok_head, _frame(4)) == -3 and _call(lib, fn, desc, ok_head, _frame(-1)) == -3
        assert _call(lib, fn, desc, ok_head, _frame(0, (-1, -1, -1, 1, -1, 1))) == -3          # hi == lo on an axis
        assert _call(lib, fn, desc, ok_head, _frame(0, (-1, -1, -1, 1, float("nan"), 1))) == -3
        for kind in (0, 1, 2, 3):
            assert _call(lib, fn, desc, ok_head, _frame(kind), n=0) == 0
    # K-Planes configurations
    assert _call(lib, "tn_kplanes_normals", _kplanes(missing=(1, 2)), _head(96)) == -3 and b"three planes" in lib.tn_last_error_string()
    assert _call(lib, "tn_kplanes_normals", _kplanes(channels=12), _head(36)) == -3
    assert _call(lib, "tn_kplanes_normals", _kplanes(n_scales=5), _head(160)) == -3
    assert _call(lib, "tn_kplanes_normals", _kplanes(plane=72), _head(96)) == -4
    assert _call(lib, "tn_kplanes_normals", _kplanes(1, 4), _head(4), n=0) == 0
    assert _call(lib, "tn_kplanes_normals", _kplanes(2, 8), _head(16), n=0) == 0
    assert _call(lib, "tn_kplanes_normals", _kplanes(2, 8), _head(96)) == -3                   # F is the field's width
    # hash-grid configurations: as tn_hashgrid_fwd
    assert _call(lib, "tn_hashgrid_normals", _hashgrid(features=3), _head(6)) == -3
    assert _call(lib, "tn_hashgrid_normals", _hashgrid(table=None), _head(4)) == -1
    assert _call(lib, "tn_hashgrid_normals", _hashgrid(table=72), _head(4)) == -4
    assert _call(lib, "tn_hashgrid_normals", _hashgrid(features=4), _head(8), n=0) == 0


def test_ray_normals_rejects_bad_arguments_before_launching(lib):
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    f = lib.tn_ray_normals
    assert f(None, None, None, i64(0), None, None) == 0
    assert f(vp(FAKE), vp(FAKE), vp(FAKE), i64(-1), vp(FAKE), None) == -2
    for k in range(4):
        args = [vp(FAKE)] * 4
        args[k] = None
        assert f(args[0], args[1], args[2], i64(3), args[3], None) == -1 and b"tn_ray_normals" in lib.tn_last_error_string()
    assert f(vp(FAKE), vp(FAKE), vp(FAKE + 4), i64(3), vp(FAKE), None) == -4


# --------------------------------------------------------------------------------------------------------------- Python layers
def test_keywords_and_defaults():
    from tinynerf_amd import core, points as P, run
    sig = inspect.signature(core.NerfRenderer.render_maps)
    assert list(sig.parameters)[1:] == ["packed_samples", "packing_info", "t", "early_termination_threshold", "normals"]
    assert sig.parameters["normals"].default is False
    for fn in (run.Trainer.render_rays, run.infer, run.train):
        params = inspect.signature(fn).parameters
        assert list(params)[-1] == "normals" and params["normals"].default is False, fn
    sig = inspect.signature(core.sample_normals)
    assert list(sig.parameters) == ["renderer", "packed", "gate", "return_grad"]
    assert sig.parameters["gate"].default is None and sig.parameters["return_grad"].default is False
    assert list(inspect.signature(P.export_oriented_pointcloud).parameters) == list(inspect.signature(P.export_pointcloud).parameters)
    assert list(inspect.signature(P.write_ply).parameters) == ["path", "points", "colors", "normals"]
    assert inspect.signature(P.write_ply).parameters["normals"].default is None
    assert inspect.signature(P.read_ply).parameters["normals"].default is False


def test_renderer_frame_defaults_to_none_and_the_helper_mirrors_the_contractions():
    from tinynerf_amd import _lib as L, core, models
    r = core.NerfRenderer(models.HashGridFeatureField(2, 2, 8, 2, 4), models.VanillaOpacityDecoder(4), models.VanillaColorDecoder(2, 4, 64, 1))
    assert r.normal_frame is None
    assert core.normal_frame(None).contraction == L.CONTRACT_NONE
    assert core.normal_frame(core.ContractionMip360()).contraction == L.CONTRACT_MIP360_INF
    assert core.normal_frame(core.ContractionMip360(2)).contraction == L.CONTRACT_MIP360_L2
    f = core.normal_frame(core.ContractionAABB(torch.tensor([[-1., -2., -3.], [1., 2., 4.]])))
    assert f.contraction == L.CONTRACT_AABB and list(f.aabb) == [-1, -2, -3, 1, 2, 4]


def test_sample_normals_names_why_a_model_has_no_normals():
    from tinynerf_amd import core, models
    packed = torch.zeros(4, 7)
    vanilla = core.NerfRenderer(models.VanillaFeatureMLP(2, 64, 2), models.VanillaOpacityDecoder(64), models.VanillaColorDecoder(2, 64, 64, 1))
    with pytest.raises(NotImplementedError, match="VanillaFeatureMLP"):
        core.sample_normals(vanilla, packed)
    cobafa = core.NerfRenderer(models.CobafaFeatureField(basis_res=[4, 4], coef_res=4, freqs=[2., 4.], channels=[4, 4], mlp_hidden_dim=16), models.VanillaOpacityDecoder(16),
                               models.VanillaColorDecoder(2, 16, 64, 1))
    with pytest.raises(NotImplementedError, match="CobafaFeatureField"):
        core.sample_normals(cobafa, packed)
    field = models.HashGridFeatureField(2, 2, 8, 2, 4)
    explicit = core.NerfRenderer(field, models.KPlanesExplicitOpacityDecoder(4), models.VanillaColorDecoder(2, 4, 64, 1))
    with pytest.raises(NotImplementedError, match="KPlanesExplicitOpacityDecoder"):
        core.sample_normals(explicit, packed)
    wide = core.NerfRenderer(field, models.VanillaOpacityDecoder(8), models.VanillaColorDecoder(2, 4, 64, 1))
    with pytest.raises(NotImplementedError, match="4 -> 64 -> 1"):
        core.sample_normals(wide, packed)
    good = core.NerfRenderer(field, models.VanillaOpacityDecoder(4), models.VanillaColorDecoder(2, 4, 64, 1))
    with pytest.raises(RuntimeError, match="no CPU path"):
        core.sample_normals(good, packed)


def _train_cli():
    spec = importlib.util.spec_from_file_location("train_cli_normals", os.path.join(ROOT, "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_command_line(capsys):
    cli = _train_cli()
    base = ["--data", "d", "--datatype", "synthetic", "--output", "o"]
    assert cli.parse_args(base + ["--method", "kplanes"]).normals is False
    assert cli.parse_args(base + ["--method", "kplanes", "--normals"]).normals is True
    assert cli.parse_args(base + ["--method", "hashgrid", "--normals", "--export_pointcloud", "1000"]).normals is True
    for method in ("vanilla", "cobafa"):
        with pytest.raises(SystemExit):
            cli.parse_args(base + ["--method", method, "--normals"])
        assert "--normals" in capsys.readouterr().err


@pytest.mark.parametrize("method", ["vanilla", "cobafa"])
def test_train_rejects_methods_without_normals_before_any_step(method):
    from tinynerf_amd import run

    class Boom:
        def __getattr__(self, name):
            raise AssertionError("train() touched its data before rejecting the method")

    with pytest.raises(ValueError, match=method):
        run.train(run.TrainConfig(method=method), Boom(), normals=True)


# ------------------------------------------------------------------------------------------------------------------------- PLY
@pytest.mark.parametrize("m", [0, 1, 1000])
def test_ply_with_normals_round_trips_bit_for_bit(tmp_path, m):
    from tinynerf_amd import points as P
    rng = np.random.default_rng(m)
    xyz = rng.standard_normal((m, 3)).astype(np.float32)
    nrm = rng.standard_normal((m, 3)).astype(np.float32)
    if m:
        nrm[0] = [-0.0, np.float32(1e-42), np.float32(np.finfo(np.float32).max)]
    rgb = rng.integers(0, 256, (m, 3)).astype(np.uint8)
    path = tmp_path / "cloud.ply"
    P.write_ply(path, xyz, rgb, nrm)
    raw = open(path, "rb").read()
    head = (PLY_HEADER_N % m).encode("ascii")
    assert raw.startswith(head) and len(raw) == len(head) + 27 * m
    body = np.frombuffer(raw[len(head):], np.uint8).reshape(m, 27)
    assert np.array_equal(body[:, :12].copy().view("<f4").view(np.uint32), xyz.view(np.uint32))
    assert np.array_equal(body[:, 12:24].copy().view("<f4").view(np.uint32), nrm.view(np.uint32))
    assert np.array_equal(body[:, 24:], rgb)
    got = P.read_ply(path, normals=True)
    assert len(got) == 3 and got[2].dtype == np.float32 and got[2].shape == (m, 3)
    assert np.array_equal(got[0].view(np.uint32), xyz.view(np.uint32)) and np.array_equal(got[1], rgb)
    assert np.array_equal(got[2].view(np.uint32), nrm.view(np.uint32))
    P.write_ply(path, torch.from_numpy(xyz), torch.from_numpy(rgb), torch.from_numpy(nrm))
    assert open(path, "rb").read() == raw


def test_read_ply_refuses_the_other_dialect(tmp_path):
    from tinynerf_amd import points as P
    xyz, rgb, nrm = np.zeros((2, 3), np.float32), np.zeros((2, 3), np.uint8), np.ones((2, 3), np.float32)
    plain, oriented = tmp_path / "plain.ply", tmp_path / "oriented.ply"
    P.write_ply(plain, xyz, rgb)
    P.write_ply(oriented, xyz, rgb, nrm)
    assert len(P.read_ply(plain)) == 2 and len(P.read_ply(oriented, normals=True)) == 3
    with pytest.raises(ValueError):
        P.read_ply(plain, normals=True)
    with pytest.raises(ValueError):
        P.read_ply(oriented)
    with pytest.raises(ValueError):
        P.write_ply(plain, xyz, rgb, np.zeros((3, 3), np.float32))
    raw = open(oriented, "rb").read()
    for bad in (raw[:-1], raw + b"\0", raw.replace(b"property float nz\n", b"")):
        open(oriented, "wb").write(bad)
        with pytest.raises(ValueError):
            P.read_ply(oriented, normals=True)


def test_oriented_export_needs_rendered_normals():
    from tinynerf_amd import points as P

    class Trainer:
        world = 1
    with pytest.raises(ValueError, match="normal"):
        P.export_oriented_pointcloud(Trainer(), [None], indices=[0], rendered=[{"rgb": 0, "opacity": 0, "depth": 0, "median_depth": 0}])
