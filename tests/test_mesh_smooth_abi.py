"""CPU checks of the mesh-smoothing entry points' boundary: the header declares the five and still says ABI 6, the library
exports them and INTEGRATION.md names them, the new source sits behind tsdf.hip with mesh.hip's flags, the workspace size is the
documented one, every bad argument is rejected before any launch (no device pointer is dereferenced, no GPU is touched), the host
layer raises ValueError before it touches a device, and train.py knows --mesh_smooth."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tinynerf_hip.h")
NEW = ("tn_mesh_adjacency_workspace_bytes", "tn_mesh_adjacency", "tn_mesh_smooth_pass", "tn_mesh_smooth", "tn_mesh_vertex_normals")
i64, i32, f32, vp = ctypes.c_int64, ctypes.c_int32, ctypes.c_float, ctypes.c_void_p
FAKE, FAKE2, FAKE3, ODD, ODD8 = vp(64), vp(128), vp(192), vp(66), vp(68)
OK, E_NULL, E_SIZE, E_CONFIG, E_ALIGN = 0, -1, -2, -3, -4
NAN, INF = float("nan"), float("inf")


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
    assert "QUADRATIC in" in text                                  # the header says what the row ranking costs


def test_library_exports_and_the_guide_names_the_entry_points(lib):
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert re.search(r"\b" + name + r"\b", text), name
    assert lib.tn_abi_version() == 6
    from tinynerf_amd import build
    names = list(build.SOURCES)
    assert build.SOURCES["mesh_smooth.hip"] == build.SOURCES["mesh.hip"]
    assert names.index("mesh_smooth.hip") == names.index("tsdf.hip") + 1 == len(names) - 1      # behind tsdf.hip: the objects before it link where they did


def test_no_floating_point_atomics_in_the_source():
    src = open(os.path.join(ROOT, "tinynerf_amd", "csrc", "mesh_smooth.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert set(re.findall(r"\batomic\w+", code)) == {"atomicAdd"}
    for call in re.findall(r"atomicAdd\(([^;]*);", code):
        assert "cursor" in call, call                              # the int32 degrees / cursors and nothing else


def test_workspace_size_is_documented_monotone_and_a_multiple_of_8(lib):
    out = i64(-1)
    q = lib.tn_mesh_adjacency_workspace_bytes
    sizes = [0, 1, 2, 3, 255, 256, 257, 1000, 256 * 1024 - 1, 256 * 1024, 256 * 1024 + 1, 10 ** 7, (2 ** 31 - 1) // 3]
    got = {}
    for v in sizes + [2 ** 31 - 1]:
        for f in sizes:
            assert q(i64(v), i64(f), ctypes.byref(out)) == OK, (v, f)
            assert out.value == 24 * -(-v // 256) + 8 * -(-v // 2) + 8 * -(-3 * f // 2) and out.value % 8 == 0, (v, f, out.value)
            got[v, f] = out.value
    for (v, f), b in got.items():
        assert all(got[v2, f] >= b for v2 in sizes if v2 >= v) and all(got[v, f2] >= b for f2 in sizes if f2 >= f), (v, f)
    assert got[0, 0] == 0
    assert q(i64(1), i64(1), None) == E_NULL and b"tn_mesh_adjacency_workspace_bytes" in lib.tn_last_error_string()
    for v, f in [(-1, 0), (0, -1), (2 ** 31, 0), (0, 2 ** 31), (0, (2 ** 31 - 1) // 3 + 1), (2 ** 40, 2 ** 40)]:
        assert q(i64(v), i64(f), ctypes.byref(out)) == E_SIZE, (v, f)


def test_adjacency_rejects_bad_arguments_before_launching(lib):
    err = lib.tn_last_error_string

    def call(V=6, F=2, faces=FAKE, offsets=FAKE, pairs=FAKE, pinned=FAKE, stats=FAKE, work=FAKE):
        return lib.tn_mesh_adjacency(faces, i64(V), i64(F), offsets, pairs, pinned, stats, work, None)

    for kw in ({"faces": None}, {"offsets": None}, {"pairs": None}, {"pinned": None}, {"stats": None}, {"work": None}, {"V": 0, "stats": None}):
        assert call(**kw) == E_NULL, kw
        assert b"tn_mesh_adjacency" in err() and b"null" in err()
    for kw in ({"V": -1}, {"F": -1}, {"V": 2 ** 31}, {"F": 2 ** 31}, {"F": (2 ** 31 - 1) // 3 + 1}):
        assert call(**kw) == E_SIZE, kw
    assert b"2^31" in err()
    assert call(V=-1, faces=None, offsets=None, pairs=None, pinned=None, stats=None, work=None) == E_SIZE      # the size before the pointers
    assert call(work=ODD8) == E_ALIGN and call(stats=ODD8) == E_ALIGN and b"8-byte aligned" in err()
    assert call(offsets=ODD) == E_ALIGN and call(pairs=ODD) == E_ALIGN and call(faces=ODD) == E_ALIGN
    assert call(offsets=None, work=ODD8) == E_NULL                                                         # the pointers before the alignment


def test_smooth_pass_rejects_bad_arguments_before_launching(lib):
    err = lib.tn_last_error_string

    def call(V=6, f=0.5, src=FAKE, offsets=FAKE, pairs=FAKE, pinned=None, out=FAKE2):
        return lib.tn_mesh_smooth_pass(src, offsets, pairs, pinned, i64(V), f32(f), out, None)

    for kw in ({"src": None}, {"offsets": None}, {"pairs": None}, {"out": None}):
        assert call(**kw) == E_NULL, kw
        assert b"tn_mesh_smooth_pass" in err() and b"null" in err()
    assert call(V=-1) == E_SIZE and call(V=2 ** 31) == E_SIZE
    for f in (NAN, INF, -INF):
        assert call(f=f) == E_CONFIG and b"finite" in err()
    assert call(out=FAKE) == E_CONFIG and b"alias" in err()
    assert call(V=-1, f=NAN, src=None) == E_SIZE and call(f=NAN, src=None) == E_CONFIG                     # size, configuration, pointers, alignment
    assert call(src=ODD) == E_ALIGN and call(out=ODD) == E_ALIGN and call(offsets=ODD) == E_ALIGN
    assert call(V=0, src=None, offsets=None, pairs=None, out=None) == OK


def test_smooth_rejects_bad_arguments_before_launching(lib):
    err = lib.tn_last_error_string

    def call(V=6, N=2, lam=0.5, mu=-0.53, src=FAKE, offsets=FAKE, pairs=FAKE, pinned=None, scratch=FAKE2, out=FAKE3):
        return lib.tn_mesh_smooth(src, offsets, pairs, pinned, i64(V), i32(N), f32(lam), f32(mu), scratch, out, None)

    for kw in ({"src": None}, {"offsets": None}, {"pairs": None}, {"scratch": None}, {"out": None}):
        assert call(**kw) == E_NULL, kw
        assert b"tn_mesh_smooth" in err() and b"null" in err()
    assert call(V=-1) == E_SIZE and call(V=2 ** 31) == E_SIZE and call(N=-1) == E_SIZE and b"iterations" in err()
    for kw in ({"lam": NAN}, {"mu": NAN}, {"lam": INF}, {"mu": -INF}):
        assert call(**kw) == E_CONFIG, kw
    for kw in ({"out": FAKE}, {"scratch": FAKE}, {"scratch": FAKE3}):
        assert call(**kw) == E_CONFIG and b"alias" in err(), kw
    assert call(N=-1, lam=NAN) == E_SIZE and call(lam=NAN, src=None) == E_CONFIG and call(src=None, out=ODD) == E_NULL
    assert call(scratch=ODD) == E_ALIGN and call(out=ODD) == E_ALIGN
    assert call(V=0, src=None, offsets=None, pairs=None, scratch=None, out=None) == OK


def test_vertex_normals_rejects_bad_arguments_before_launching(lib):
    err = lib.tn_last_error_string

    def call(V=6, src=FAKE, offsets=FAKE, pairs=FAKE, fallback=None, out=FAKE2):
        return lib.tn_mesh_vertex_normals(src, offsets, pairs, i64(V), fallback, out, None)

    for kw in ({"src": None}, {"offsets": None}, {"pairs": None}, {"out": None}):
        assert call(**kw) == E_NULL, kw
        assert b"tn_mesh_vertex_normals" in err() and b"null" in err()
    assert call(V=-1) == E_SIZE and call(V=2 ** 31) == E_SIZE
    assert call(src=ODD) == E_ALIGN and call(fallback=ODD) == E_ALIGN and call(out=ODD) == E_ALIGN
    assert call(V=0, src=None, offsets=None, pairs=None, out=None) == OK


def test_the_host_layer_checks_its_arguments_before_any_device_work():
    import torch
    from tinynerf_amd import mesh as M
    v, f = torch.zeros((4, 3)), torch.zeros((2, 3), dtype=torch.int32)
    for fn in (M.adjacency, M.smooth, M.vertex_normals, M.smooth_mesh, M.check_smooth):
        assert callable(fn)
    bad = [lambda: M.smooth(v, f, -1), lambda: M.smooth(v, f, 1.5), lambda: M.smooth(v, f, 1, lam=NAN), lambda: M.smooth(v, f, 1, mu=INF),
           lambda: M.smooth(v.double(), f, 1), lambda: M.smooth(v[:, :2], f, 1), lambda: M.smooth(v, f.long(), 1), lambda: M.smooth(v, f[:, :2], 1),
           lambda: M.vertex_normals(v, f, fallback=v[:3]), lambda: M.vertex_normals(v, f.long()), lambda: M.smooth_mesh(v, v[:2], f, 1),
           lambda: M.smooth_mesh(v, v, f, -2), lambda: M.adjacency(f.long(), 4), lambda: M.adjacency(f, -1),
           lambda: M.export_smooth_mesh(None, smooth=-1), lambda: M.export_smooth_mesh(None, smooth=1, smooth_mu=NAN)]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    assert M.smooth(v, f, 0) is v                                  # the identity: no launch, the input returned
    from tinynerf_amd import tsdf
    with pytest.raises(ValueError):
        tsdf.export_smooth_tsdf_mesh(None, None, smooth=-1)
    import inspect
    from tinynerf_amd.run import train
    for fn in (M.export_smooth_mesh, tsdf.export_smooth_tsdf_mesh):
        p = inspect.signature(fn).parameters
        assert p["smooth"].default == 0 and p["smooth_lambda"].default == 0.5 and p["smooth_mu"].default == -0.53
    assert inspect.signature(train).parameters["mesh_smooth"].default == 0


def test_train_py_knows_the_flag(capsys):
    sys.path.insert(0, ROOT)
    try:
        import train as cli
    finally:
        sys.path.remove(ROOT)
    base = ["--data", "d", "--datatype", "synthetic", "--output", "o", "--method", "kplanes"]
    assert cli.parse_args(base).mesh_smooth == 0
    assert cli.parse_args(base + ["--export_mesh", "64", "--mesh_smooth", "5"]).mesh_smooth == 5
    assert cli.parse_args(base + ["--export_tsdf_mesh", "64", "--mesh_smooth", "2"]).mesh_smooth == 2
    for extra, word in ((["--mesh_smooth", "3"], "--export_mesh"), (["--export_mesh", "64", "--mesh_smooth", "-1"], ">= 0"),
                        (["--export_tsdf_mesh", "64", "--mesh_smooth", "-2"], ">= 0")):
        with pytest.raises(SystemExit):
            cli.parse_args(base + extra)
        assert word in capsys.readouterr().err
    comment = "".join(line for line in open(os.path.join(ROOT, "train.py")).read().split("FLAGS = (")[0].splitlines(True) if line.startswith("#"))
    assert "--mesh_smooth" in comment
