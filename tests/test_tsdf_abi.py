"""CPU checks of the TSDF entry points' boundary: the header declares the two and still says ABI 6, the library exports them
and INTEGRATION.md names them, tsdf.hip is built with mesh.hip's flags after mesh_components.hip, and every bad argument is rejected
before any launch (no device pointer is dereferenced, no GPU is touched)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tinynerf_hip.h")
NEW = ("tn_tsdf_integrate", "tn_tsdf_mask_faces")
i32, i64, f32, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
FAKE, ODD = vp(64), vp(66)
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
    assert "LIMIT" in text and "the guard is local" in text        # the definition states the guard's limit


def test_library_exports_and_the_guide_names_the_entry_points(lib):
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert re.search(r"\b" + name + r"\b", text), name
    assert lib.tn_abi_version() == 6
    from tinynerf_amd import build
    assert build.SOURCES["tsdf.hip"] == build.SOURCES["mesh.hip"]
    names = list(build.SOURCES)
    assert names.index("tsdf.hip") > names.index("mesh_components.hip")      # behind it: the objects before link where they did


def _table(n_img=4, **null):
    from tinynerf_amd import _lib as L
    fields = dict(c2w=64, lens=64, model=64, size=64, pixel_offset=64, rgb=None)
    fields.update(null)
    return L.CameraTable(fields["c2w"], fields["lens"], fields["model"], fields["size"], fields["pixel_offset"], fields["rgb"], 1000, n_img, 0)


def test_integrate_rejects_bad_arguments_before_launching(lib):
    err = lib.tn_last_error_string
    keep = []

    def call(dims=(4, 3, 2), first=0, count=4, trunc=0.1, cams="table", depth=FAKE, opacity=FAKE, S=FAKE, W=FAKE, lo=True, h=True, **table):
        t = _table(**table)
        d, l3, h3 = (i32 * 3)(*dims) if dims is not None else None, (f32 * 3)(0, 0, 0), (f32 * 3)(1, 1, 1)
        keep.append((t, d, l3, h3))
        return lib.tn_tsdf_integrate(ctypes.byref(t) if cams == "table" else None, depth, opacity, f32(0.5), d, l3 if lo else None, h3 if h else None,
                                     f32(trunc), i32(first), i32(count), S, W, None)

    for kw in ({"cams": None}, {"dims": None}, {"lo": False}, {"h": False}, {"depth": None}, {"S": None}, {"W": None}, {"c2w": None}, {"lens": None},
               {"model": None}, {"size": None}, {"pixel_offset": None}):
        assert call(**kw) == E_NULL, kw
        assert b"tn_tsdf_integrate" in err() and b"null" in err()
    for kw in ({"dims": (-1, 3, 2)}, {"dims": (4, -3, 2)}, {"dims": (4, 3, -2)}, {"count": -1}, {"first": -1}, {"first": 1}, {"first": 4, "count": 1},
               {"count": 5}, {"first": 2 ** 31 - 1, "count": 2 ** 31 - 1}, {"dims": (2047, 1023, 1023)}, {"dims": (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)},
               {"n_img": -1, "count": 0}):
        assert call(**kw) == E_SIZE, kw
    assert call(dims=(2046, 1023, 1023), depth=None) == E_NULL     # 2^31 - 2^21 nodes: the size passes
    for trunc in (0.0, -1.0, float("nan"), float("inf")):
        assert call(trunc=trunc) == E_CONFIG and b"trunc" in err()
    # the order: sizes, configuration, pointers, alignment
    assert call(dims=(-1, 1, 1), trunc=0.0, depth=None, S=ODD) == E_SIZE
    assert call(trunc=0.0, depth=None, S=ODD) == E_CONFIG
    assert call(depth=None, S=ODD) == E_NULL
    for kw in ({"depth": ODD}, {"opacity": ODD}, {"S": ODD}, {"W": ODD}):
        assert call(**kw) == E_ALIGN, kw
    assert b"4-byte aligned" in err()
    # nothing to do: TN_OK without a launch, whatever the pointers
    assert call(count=0, depth=None, S=None, W=None) == OK and call(first=4, count=0) == OK
    for dims in ((0, 3, 2), (4, 0, 2), (4, 3, 0)):
        assert call(dims=dims, depth=None, S=None, W=None, c2w=None) == OK
    assert call(count=0, trunc=0.0) == E_CONFIG                    # (the checks come first)
    assert call(opacity=None, depth=None) == E_NULL                # opacity is optional, depth is not


def test_mask_faces_rejects_bad_arguments_before_launching(lib):
    err = lib.tn_last_error_string

    def call(dims=(4, 3, 2), V=10, F=5, W=FAKE, ids=FAKE, faces=FAKE, observed=FAKE):
        return lib.tn_tsdf_mask_faces(W, (i32 * 3)(*dims) if dims is not None else None, ids, i64(V), faces, i64(F), observed, None)

    for kw in ({"dims": None}, {"W": None}, {"ids": None}, {"faces": None}, {"observed": None}):
        assert call(**kw) == E_NULL, kw
        assert b"tn_tsdf_mask_faces" in err() and b"null" in err()
    for kw in ({"dims": (-1, 3, 2)}, {"dims": (4, 3, -2)}, {"V": -1}, {"F": -1}, {"V": 2 ** 31}, {"F": 2 ** 31}, {"dims": (2047, 1023, 1023)}):
        assert call(**kw) == E_SIZE, kw
    assert call(V=-1, faces=None, W=ODD) == E_SIZE and call(faces=None, W=ODD) == E_NULL
    for kw in ({"W": ODD}, {"ids": ODD}, {"faces": ODD}):
        assert call(**kw) == E_ALIGN, kw
    assert b"4-byte aligned" in err()
    assert call(F=0, W=None, ids=None, faces=None, observed=None) == OK
