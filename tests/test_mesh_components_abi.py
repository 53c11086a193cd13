"""CPU checks of the mesh-component entry points' boundary: the header declares the four and still says ABI 6, the library
exports them and INTEGRATION.md names them, the workspace sizes are the documented ones -- monotone, multiples of 8 B --, and every bad
argument is rejected before any launch (no device pointer is dereferenced, no GPU is touched)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tinynerf_hip.h")
NEW = ("tn_mesh_components_workspace_bytes", "tn_mesh_components", "tn_mesh_filter_workspace_bytes", "tn_mesh_filter")
i64, vp = ctypes.c_int64, ctypes.c_void_p
FAKE, ODD = vp(64), vp(68)
OK, E_NULL, E_SIZE, E_CONFIG, E_ALIGN = 0, -1, -2, -3, -4


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


def test_library_exports_and_the_guide_names_the_entry_points(lib):
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert re.search(r"\b" + name + r"\b", text), name
    assert lib.tn_abi_version() == 6
    from tinynerf_amd import build
    assert build.SOURCES["mesh_components.hip"] == build.SOURCES["mesh.hip"]


def test_workspace_sizes_are_documented_monotone_and_multiples_of_8(lib):
    out = i64(-1)
    sizes = [0, 1, 2, 3, 255, 256, 257, 1000, 256 * 1024 - 1, 256 * 1024, 256 * 1024 + 1, 10 ** 7, 2 ** 31 - 1]
    for name, want in (("tn_mesh_components_workspace_bytes", lambda v, f: 24 * -(-v // 256)),
                       ("tn_mesh_filter_workspace_bytes", lambda v, f: 80 * -(-max(v, f) // 256) + 8 * -(-v // 2))):
        q = getattr(lib, name)
        got = {}
        for v in sizes:
            for f in sizes:
                assert q(i64(v), i64(f), ctypes.byref(out)) == OK, (name, v, f)
                assert out.value == want(v, f) and out.value % 8 == 0 and out.value >= 0, (name, v, f, out.value)
                got[v, f] = out.value
        for (v, f), b in got.items():                              # monotone in each argument
            assert all(got[v2, f] >= b for v2 in sizes if v2 >= v) and all(got[v, f2] >= b for f2 in sizes if f2 >= f), (name, v, f)
        assert got[0, 0] == 0
        assert q(i64(1), i64(1), None) == E_NULL and name.encode() in lib.tn_last_error_string()
        for v, f in [(-1, 0), (0, -1), (2 ** 31, 0), (0, 2 ** 31), (2 ** 40, 2 ** 40)]:
            assert q(i64(v), i64(f), ctypes.byref(out)) == E_SIZE, (name, v, f)


def test_components_rejects_bad_arguments_before_launching(lib):
    err = lib.tn_last_error_string

    def call(V=6, F=2, faces=FAKE, labels=FAKE, face_counts=FAKE, stats=FAKE, work=FAKE):
        return lib.tn_mesh_components(faces, i64(V), i64(F), labels, face_counts, stats, work, None)

    for kw in ({"faces": None}, {"labels": None}, {"face_counts": None}, {"stats": None}, {"work": None}, {"V": 0, "stats": None}):
        assert call(**kw) == E_NULL, kw
        assert b"tn_mesh_components" in err() and b"null" in err()
    for kw in ({"V": -1}, {"F": -1}, {"V": 2 ** 31}, {"F": 2 ** 31}):
        assert call(**kw) == E_SIZE, kw
    assert b"2^31" in err()
    assert call(V=-1, faces=None, labels=None, face_counts=None, stats=None, work=None) == E_SIZE          # the size before the pointers
    assert call(work=ODD) == E_ALIGN and call(stats=ODD) == E_ALIGN and b"8-byte aligned" in err()
    assert call(labels=None, work=ODD) == E_NULL                                                       # the pointers before the alignment


def test_filter_rejects_bad_arguments_before_launching(lib):
    err = lib.tn_last_error_string

    def call(V=6, F=2, T=1, vcap=4, fcap=4, faces=FAKE, labels=FAKE, face_counts=FAKE, vertices=FAKE, normals=FAKE, colors=FAKE, out_vertices=FAKE,
             out_normals=FAKE, out_colors=FAKE, src=FAKE, out_faces=FAKE, counts=FAKE, work=FAKE):
        return lib.tn_mesh_filter(faces, labels, face_counts, i64(T), vertices, normals, colors, i64(V), i64(F), i64(vcap), i64(fcap), out_vertices,
                                  out_normals, out_colors, src, out_faces, counts, work, None)

    for kw in ({"faces": None}, {"labels": None}, {"face_counts": None}, {"vertices": None}, {"out_vertices": None}, {"src": None},
               {"out_normals": None}, {"out_colors": None}, {"out_faces": None}, {"counts": None}, {"work": None}, {"V": 0, "counts": None}):
        assert call(**kw) == E_NULL, kw
        assert b"tn_mesh_filter" in err() and b"null" in err()
    for kw in ({"V": -1}, {"F": -1}, {"V": 2 ** 31}, {"F": 2 ** 31}, {"vcap": -1}, {"fcap": -1}):
        assert call(**kw) == E_SIZE, kw
    assert call(T=-1) == E_CONFIG and b"threshold" in err()
    assert call(T=-2 ** 40) == E_CONFIG
    assert call(V=-1, T=-1, counts=None) == E_SIZE                 # the order: size, configuration, pointers, alignment
    assert call(T=-1, counts=None, work=ODD) == E_CONFIG
    assert call(labels=None, work=ODD) == E_NULL
    assert call(work=ODD) == E_ALIGN and call(counts=ODD) == E_ALIGN and b"8-byte aligned" in err()
