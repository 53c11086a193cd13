"""CPU checks of the TSDF colour entry points' boundary: the header declares the two and still says ABI 6, the library
exports them and INTEGRATION.md names them, and every bad argument is rejected in the stated order before any launch (no device
pointer is dereferenced, no GPU is touched)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tinynerf_hip.h")
NEW = ("tn_tsdf_integrate_color", "tn_tsdf_sample_colors")
i32, i64, f32, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
FAKE, ODD, WORD = vp(64), vp(66), vp(68)                           # 16-byte aligned; not 4-byte aligned; 4- but not 16-byte aligned
OK, E_NULL, E_SIZE, E_CONFIG, E_ALIGN = 0, -1, -2, -3, -4


@pytest.fixture(scope="module")
def lib():
    from tinynerf_amd import build
    lib = ctypes.CDLL(build.build(verbose=False))
    lib.tn_last_error_string.restype = ctypes.c_char_p
    return lib


def test_header_declares_the_entry_points_and_keeps_the_abi_version():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
    assert re.search(r"#define TN_ABI_VERSION 6\b", src)
    assert "w = 1 - |sdf| / trunc" in text and "fmaf(-(1 - opacity[g]), bg_c, rgb[g][c]) / opacity[g]" in text      # the definition is in the comment


def test_library_exports_and_the_guide_names_the_entry_points(lib):
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert re.search(r"\b" + name + r"\b", text), name
    assert lib.tn_abi_version() == 6


def _table(n_img=4, **null):
    from tinynerf_amd import _lib as L
    fields = dict(c2w=64, lens=64, model=64, size=64, pixel_offset=64, rgb=None)
    fields.update(null)
    return L.CameraTable(fields["c2w"], fields["lens"], fields["model"], fields["size"], fields["pixel_offset"], fields["rgb"], 1000, n_img, 0)


def test_integrate_color_rejects_bad_arguments_before_launching(lib):
    err = lib.tn_last_error_string
    keep = []

    def call(dims=(4, 3, 2), first=0, count=4, trunc=0.1, min_opacity=0.5, cams="table", depth=FAKE, opacity=FAKE, rgb=FAKE, bg=FAKE, vol=FAKE,
             lo=True, h=True, **table):
        t = _table(**table)
        d, l3, h3 = (i32 * 3)(*dims) if dims is not None else None, (f32 * 3)(0, 0, 0), (f32 * 3)(1, 1, 1)
        keep.append((t, d, l3, h3))
        return lib.tn_tsdf_integrate_color(ctypes.byref(t) if cams == "table" else None, depth, opacity, f32(min_opacity), rgb, bg, d,
                                           l3 if lo else None, h3 if h else None, f32(trunc), i32(first), i32(count), vol, None)

    for kw in ({"cams": None}, {"dims": None}, {"lo": False}, {"h": False}, {"depth": None}, {"rgb": None}, {"vol": None}, {"c2w": None}, {"lens": None},
               {"model": None}, {"size": None}, {"pixel_offset": None}):
        assert call(**kw) == E_NULL, kw
        assert b"tn_tsdf_integrate_color" in err() and b"null" in err()
    for kw in ({"dims": (-1, 3, 2)}, {"dims": (4, -3, 2)}, {"dims": (4, 3, -2)}, {"count": -1}, {"first": -1}, {"first": 1}, {"first": 4, "count": 1},
               {"count": 5}, {"first": 2 ** 31 - 1, "count": 2 ** 31 - 1}, {"dims": (2047, 1023, 1023)}, {"dims": (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)},
               {"n_img": -1, "count": 0}):
        assert call(**kw) == E_SIZE, kw
    assert call(dims=(2046, 1023, 1023), depth=None) == E_NULL     # 2^31 - 2^21 nodes: the size passes
    for trunc in (0.0, -1.0, float("nan"), float("inf")):
        assert call(trunc=trunc) == E_CONFIG and b"trunc" in err()
    for m in (0.0, -0.5, float("nan")):                            # the division by the opacity must stay defined
        assert call(min_opacity=m) == E_CONFIG and b"min_opacity" in err()
        assert call(min_opacity=m, opacity=None, depth=None) == E_NULL      # without a map min_opacity is not used: the next check speaks
    # the order: null cams / dims / lo / h, sizes, configuration, the other pointers, alignment
    assert call(cams=None, dims=(-1, 1, 1), trunc=0.0) == E_NULL
    assert call(dims=(-1, 1, 1), trunc=0.0, depth=None, vol=ODD) == E_SIZE
    assert call(trunc=0.0, depth=None, vol=ODD) == E_CONFIG
    assert call(min_opacity=0.0, depth=None, vol=ODD) == E_CONFIG
    assert call(depth=None, vol=ODD) == E_NULL
    for kw in ({"depth": ODD}, {"opacity": ODD}, {"rgb": ODD}, {"bg": ODD}):
        assert call(**kw) == E_ALIGN, kw
        assert b"4-byte aligned" in err()
    for bad in (ODD, WORD, vp(72)):
        assert call(vol=bad) == E_ALIGN and b"16-byte aligned" in err()
    assert call(depth=WORD, opacity=WORD, rgb=WORD, bg=WORD, first=4, count=0) == OK
    # nothing to do: TN_OK without a launch, whatever the pointers
    assert call(count=0, depth=None, rgb=None, vol=None) == OK and call(first=4, count=0) == OK
    for dims in ((0, 3, 2), (4, 0, 2), (4, 3, 0)):
        assert call(dims=dims, depth=None, rgb=None, vol=None, c2w=None) == OK
    assert call(count=0, trunc=0.0) == E_CONFIG                    # (the checks come first)
    assert call(opacity=None, bg=None, depth=None) == E_NULL       # opacity and bg are optional, depth is not
    assert call(rgb=vp(0), c2w=None) == E_NULL


def test_sample_colors_rejects_bad_arguments_before_launching(lib):
    err = lib.tn_last_error_string

    def call(dims=(4, 3, 2), n=10, vol=FAKE, points=FAKE, out=FAKE, lo=True, h=True):
        l3, h3 = (f32 * 3)(0, 0, 0), (f32 * 3)(1, 1, 1)
        return lib.tn_tsdf_sample_colors(vol, (i32 * 3)(*dims) if dims is not None else None, l3 if lo else None, h3 if h else None, points, i64(n),
                                         out, None)

    for kw in ({"dims": None}, {"lo": False}, {"h": False}, {"vol": None}, {"points": None}, {"out": None}):
        assert call(**kw) == E_NULL, kw
        assert b"tn_tsdf_sample_colors" in err() and b"null" in err()
    for kw in ({"dims": (-1, 3, 2)}, {"dims": (4, 3, -2)}, {"n": -1}, {"n": 2 ** 31}, {"dims": (2047, 1023, 1023)}):
        assert call(**kw) == E_SIZE, kw
    assert call(dims=None, n=-1) == E_NULL and call(n=-1, vol=None, out=ODD) == E_SIZE and call(vol=None, out=ODD) == E_NULL
    assert call(points=ODD) == E_ALIGN and b"4-byte aligned" in err()
    for kw in ({"vol": WORD}, {"out": WORD}, {"vol": ODD}, {"out": vp(72)}):
        assert call(**kw) == E_ALIGN and b"16-byte aligned" in err(), kw
    assert call(points=WORD, n=0) == OK
    assert call(n=0, vol=None, points=None, out=None) == OK
    for dims in ((0, 3, 2), (4, 0, 2), (4, 3, 0)):
        assert call(dims=dims, vol=None, points=None, out=None) == OK
