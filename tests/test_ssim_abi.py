"""CPU checks of the SSIM feature: the fp64 yardstick (tests/_ssim_ref.py) pins itself on closed forms, the header declares
tn_ssim / tn_ssim_workspace_bytes and still says ABI 6, the library exports them and rejects bad arguments before any launch,
INTEGRATION.md names them, and the Python layers and the command line carry the feature with its default off."""
import ctypes
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest

import _ssim_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tinynerf_hip.h")
NEW = ("tn_ssim", "tn_ssim_workspace_bytes")


@pytest.fixture(scope="module")
def lib():
    from tinynerf_amd import build
    lib = ctypes.CDLL(build.build(verbose=False))
    lib.tn_last_error_string.restype = ctypes.c_char_p
    return lib


# ------------------------------------------------------------------------------------------------ 1. the yardstick pins itself
def test_window_is_the_normalised_gaussian():
    g = ref.gauss()
    assert g.shape == (11,) and abs(g.sum() - 1.0) < 1e-15 and np.array_equal(g, g[::-1])
    assert abs(g[5] / g[4] - np.exp(1.0 / 4.5)) < 1e-14 and abs(g[5] / g[0] - np.exp(25.0 / 4.5)) < 1e-12


@pytest.mark.parametrize("data_range", [1.0, 255.0])
@pytest.mark.parametrize("p,q", [(0.0, 0.0), (1.0, 1.0), (0.25, 0.75), (1.0, 0.0), (0.5, 0.501)])
def test_reference_on_constant_images_is_the_closed_form(p, q, data_range):
    """variances are 0, the second factor is 1: (2pq + c1) / (p^2 + q^2 + c1) in every entry"""
    a = np.full((19, 23, 3), p * data_range)
    b = np.full((19, 23, 3), q * data_range)
    c1 = (0.01 * data_range) ** 2
    want = (2 * a[0, 0, 0] * b[0, 0, 0] + c1) / (a[0, 0, 0] ** 2 + b[0, 0, 0] ** 2 + c1)
    m = ref.ssim_map(a, b, data_range)
    assert m.shape == (9, 13, 3)
    assert np.abs(m - want).max() <= 1e-12
    assert abs(ref.ssim(a, b, data_range) - want) <= 1e-12


def test_reference_on_identical_images_is_one():
    a, _ = ref.uniform_noise(30, 41, 4, seed=1)
    m = ref.ssim_map(a, a)
    assert m.shape == (20, 31, 4) and np.abs(m - 1.0).max() <= 1e-12


def test_reference_on_an_11_x_11_input_has_one_window_per_channel():
    a, b = ref.uniform_noise(11, 11, 3, seed=2)
    m = ref.ssim_map(a, b)
    assert m.shape == (1, 1, 3)
    g = ref.gauss()
    w = np.outer(g, g)[..., None]
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    mua, mub = (w * a64).sum((0, 1)), (w * b64).sum((0, 1))
    vaa, vbb = (w * (a64 - mua) ** 2).sum((0, 1)), (w * (b64 - mub) ** 2).sum((0, 1))
    vab = (w * (a64 - mua) * (b64 - mub)).sum((0, 1))
    want = (2 * mua * mub + 1e-4) * (2 * vab + 9e-4) / ((mua ** 2 + mub ** 2 + 1e-4) * (vaa + vbb + 9e-4))
    assert np.abs(m[0, 0] - want).max() <= 1e-14
    with pytest.raises(AssertionError):
        ref.ssim_map(a[:10], b[:10])


@pytest.mark.parametrize("pattern", sorted(ref.PATTERNS))
def test_reference_direct_and_separable_forms_agree(pattern):
    a, b = ref.PATTERNS[pattern](37, 52, 3, seed=3)
    d, s = ref.ssim_map(a, b), ref.ssim_map_separable(a, b)
    assert np.abs(d - s).max() <= 1e-10
    d, s = ref.ssim_map(a * 255.0, b * 255.0, 255.0), ref.ssim_map_separable(a * 255.0, b * 255.0, 255.0)
    assert np.abs(d - s).max() <= 1e-10


def test_fp32_centred_moments_hold_the_bound_where_raw_moments_do_not():
    """the numerical choice of the kernel, replayed in float32 on the disc-on-white pair: the centred form stays within the
    1e-5 parity bound of the fp64 map, the textbook E[a^2] - mu^2 misses it on the flat background (c2 = 9e-4 is the whole
    denominator there)"""
    a, b = ref.disc_on_white(96, 96, 3, seed=0)
    exact = ref.ssim_map(a, b)
    centred = np.abs(ref.ssim_map_emulated(a, b, form="centred") - exact).max()
    raw = np.abs(ref.ssim_map_emulated(a, b, form="raw") - exact).max()
    print(f"fp32 emulation, worst map entry vs fp64: centred {centred:.3g}, raw moments {raw:.3g}")
    assert centred <= 1e-5
    assert raw > 1e-5


# ------------------------------------------------------------------------------------------------ 2. the C ABI
def test_header_declares_the_ssim_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
    assert re.search(r"#define TN_ABI_VERSION 6\b", src)


def test_library_exports_the_ssim_entry_points(lib):
    for name in NEW:
        assert hasattr(lib, name), name
    assert lib.tn_abi_version() == 6


def test_integration_guide_names_the_ssim_entry_points():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert re.search(r"\b" + name + r"\b", text), name


def test_workspace_query_works_without_a_gpu(lib):
    i64, i32 = ctypes.c_int64, ctypes.c_int32
    q = lib.tn_ssim_workspace_bytes
    n = i64(-1)
    assert q(i64(11), i64(11), i32(3), ctypes.byref(n)) == 0 and n.value > 0 and n.value % 8 == 0
    one = n.value
    assert q(i64(800), i64(800), i32(3), ctypes.byref(n)) == 0 and one < n.value <= 1 << 20
    big = n.value
    assert q(i64(800), i64(800), i32(1), ctypes.byref(n)) == 0 and n.value <= big
    assert q(i64(800), i64(800), i32(3), None) == -1
    assert b"tn_ssim_workspace_bytes" in lib.tn_last_error_string()
    assert q(i64(-1), i64(800), i32(3), ctypes.byref(n)) == -2
    assert q(i64(10), i64(800), i32(3), ctypes.byref(n)) == -3
    assert q(i64(800), i64(10), i32(3), ctypes.byref(n)) == -3
    assert q(i64(800), i64(800), i32(0), ctypes.byref(n)) == -3
    assert q(i64(800), i64(800), i32(5), ctypes.byref(n)) == -3


def test_ssim_rejects_bad_arguments_before_launching(lib):
    i64, i32, f32, vp = ctypes.c_int64, ctypes.c_int32, ctypes.c_float, ctypes.c_void_p
    fake = vp(64)                                           # never dereferenced: every call below returns before a launch
    n = i64(0)
    assert lib.tn_ssim_workspace_bytes(i64(43), i64(75), i32(3), ctypes.byref(n)) == 0
    ws = i64(n.value)

    def call(a=fake, b=fake, H=43, W=75, C=3, L=1.0, smap=fake, work=fake, nbytes=ws, mean=fake):
        return lib.tn_ssim(a, b, i64(H), i64(W), i32(C), f32(L), smap, work, nbytes, mean, None)

    assert call(a=None) == -1                               # null pointers
    assert b"tn_ssim" in lib.tn_last_error_string()
    assert call(b=None) == -1
    assert call(work=None) == -1
    assert call(mean=None) == -1
    assert call(H=-43) == -2                                # negative sizes
    assert call(W=-1) == -2
    assert call(C=-3) == -2
    assert call(nbytes=i64(-8)) == -2
    assert call(H=10) == -3                                 # no whole window
    assert b"tn_ssim" in lib.tn_last_error_string()
    assert call(W=10) == -3
    assert call(H=0, W=0) == -3                             # not an empty result
    assert call(C=0) == -3
    assert call(C=5) == -3
    assert call(L=0.0) == -3                                # data_range
    assert call(L=-1.0) == -3
    assert call(L=float("nan")) == -3
    assert call(L=float("inf")) == -3
    assert call(nbytes=i64(n.value - 1)) == -3              # a workspace one byte short
    assert call(nbytes=i64(0)) == -3
    assert call(a=vp(66)) == -4                             # misaligned
    assert call(b=vp(65)) == -4
    assert call(smap=vp(66)) == -4
    assert call(mean=vp(67)) == -4
    assert call(work=vp(68)) == -4                          # fp64 partial sums: 8-byte aligned
    assert b"tn_ssim" in lib.tn_last_error_string()


# ------------------------------------------------------------------------------------------------ 3. Python and the command line
def test_python_layers_carry_the_feature_with_its_default_off():
    from tinynerf_amd import run
    sig = inspect.signature(run.ssim)
    assert list(sig.parameters) == ["x", "y", "data_range", "return_map"]
    assert sig.parameters["data_range"].default == 1.0 and sig.parameters["return_map"].default is False
    sig = inspect.signature(run.evaluate)
    assert list(sig.parameters) == ["dataset", "rendered", "indices", "ssim"] and sig.parameters["ssim"].default is False
    assert inspect.signature(run.train).parameters["ssim"].default is False
    assert run.EvalMetrics().ssim == 0.0
    assert callable(run.psnr)


def test_ssim_wrapper_checks_its_arguments_without_a_gpu():
    import torch
    from tinynerf_amd import run
    x = torch.rand(16, 16, 3)
    with pytest.raises(RuntimeError, match="CUDA"):
        run.ssim(x, x)                                       # no CPU path
    with pytest.raises(RuntimeError, match="float32"):
        run.ssim(x.double(), x.double())
    with pytest.raises(RuntimeError, match="same shape"):
        run.ssim(x, x[:, :12])
    with pytest.raises(RuntimeError, match="same shape"):
        run.ssim(x[..., 0], x[..., 0])


def _train_cli():
    spec = importlib.util.spec_from_file_location("tinynerf_train_cli", os.path.join(ROOT, "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_cli_ssim_flag():
    cli = _train_cli()
    base = ["--data", "d", "--datatype", "synthetic", "--output", "o", "--method", "kplanes"]
    assert cli.parse_args(base).ssim is False
    assert cli.parse_args(base + ["--ssim"]).ssim is True
