"""CPU checks of the depth / opacity maps feature: the header declares tn_sample_pack_t and tn_ray_maps, the library exports
them and rejects bad arguments before any launch, INTEGRATION.md names them, and the Python layers take the new keywords."""
import ctypes
import importlib.util
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tinynerf_hip.h")
NEW = ("tn_sample_pack_t", "tn_ray_maps")


@pytest.fixture(scope="module")
def lib():
    from tinynerf_amd import build
    lib = ctypes.CDLL(build.build(verbose=False))
    lib.tn_last_error_string.restype = ctypes.c_char_p
    return lib


def test_header_declares_the_map_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
    assert re.search(r"#define TN_ABI_VERSION 6\b", src)


def test_library_exports_the_map_entry_points(lib):
    for name in NEW:
        assert hasattr(lib, name), name


def test_integration_guide_names_the_map_entry_points():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert re.search(r"\b" + name + r"\b", text), name


def test_ray_maps_rejects_bad_arguments_before_launching(lib):
    i64, vp = ctypes.c_int64, ctypes.c_void_p
    fake = vp(64)                                           # never dereferenced: every call below returns before a launch
    assert lib.tn_ray_maps(None, None, None, i64(-1), fake, None, None, None) == -2
    assert lib.tn_ray_maps(None, None, None, i64(4), None, None, None, None) == 0        # no output asked for
    assert lib.tn_ray_maps(None, None, None, i64(0), fake, fake, fake, None) == 0        # no rays
    assert lib.tn_ray_maps(None, fake, fake, i64(4), fake, None, None, None) == -1       # weights missing
    assert b"tn_ray_maps" in lib.tn_last_error_string()
    assert lib.tn_ray_maps(fake, None, fake, i64(4), None, fake, None, None) == -1       # depth without t
    assert lib.tn_ray_maps(fake, None, fake, i64(4), None, None, fake, None) == -1       # median without t
    assert lib.tn_ray_maps(fake, fake, vp(68), i64(4), fake, None, None, None) == -4     # info not 8-byte aligned
    assert lib.tn_sample_pack_t(None, None, None, i64(4), None, None, None, None, None, None, None, i64(8), None) == -1


def test_python_layers_take_the_new_keywords():
    from tinynerf_amd import core, run
    assert inspect.signature(core.RayProvider.__call__).parameters["return_t"].default is False
    assert list(inspect.signature(core.NerfRenderer.render_maps).parameters)[1:4] == ["packed_samples", "packing_info", "t"]
    assert inspect.signature(run.Trainer.render_rays).parameters["maps"].default is False
    assert inspect.signature(run.infer).parameters["maps"].default is False
    assert inspect.signature(run.train).parameters["render_maps"].default is False


def _train_cli():
    spec = importlib.util.spec_from_file_location("tinynerf_train_cli", os.path.join(ROOT, "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_cli_render_maps_flag():
    cli = _train_cli()
    base = ["--data", "d", "--datatype", "synthetic", "--output", "o", "--method", "kplanes"]
    assert cli.parse_args(base + ["--render_maps"]).render_maps is True
    assert cli.parse_args(base).render_maps is False


def test_render_maps_refuses_a_graph():
    """The maps carry no gradient: with grad enabled on parameters that require it, render_maps raises before any launch."""
    from tinynerf_amd import core, models
    r = core.NerfRenderer(models.KPlanesFeatureField(32, (8, 8, 8)), models.VanillaOpacityDecoder(96),
                          models.VanillaColorDecoder(8, 96, 64, 3), None)
    with pytest.raises(RuntimeError, match="inference only"):
        r.render_maps(torch.zeros(4, 7), torch.zeros(1, 2, dtype=torch.int32), torch.zeros(4))
