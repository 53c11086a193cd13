"""CPU checks of the host-only answers of the wide-stack (layer-by-layer) MLP path: tn_mlp_bwd_workspace_bytes,
tn_mlp_fwd_workspace_bytes, tn_mlp_rows_view and tn_mlp_rows_view_hidden for the shapes that path takes, under every arithmetic
and the flags that shape its workspace.  tests/golden/mlp_wide_workspace.json holds what the library answered before these answers
came from one plan (csrc/mlp_bwd_layers.hip); the only entries allowed to differ are the training workspaces that cannot run the
cross-layer f16x2 forms, which no longer carry the chain's gradient slabs and the packed weight stream."""
import ctypes as C
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mlp_wide_workspace.json")

ENC_NONE, ENC_POSENC, ENC_DIR_CAT = 0, 1, 2
BF16X3, F16X2, ROWS_ONLY, SKIP_LAST, LAYERWISE = 32, 64, 128, 1024, 2048

# name: (encoding, in_dim, n_freqs, dims)
CONFIGS = {
    "vanilla": (ENC_POSENC, 3, 10, [60] + [256] * 10),                  # 60 -> 256 x 9 -> 256
    "cobafa": (ENC_NONE, 36, 0, [36] + [128] * 7),                      # 36 -> 128 x 6 -> 128
    "mlp100": (ENC_NONE, 100, 0, [100] + [256] * 5),                    # MLP(100, 256, 3, 256): general-shape first layer
    "dircat": (ENC_DIR_CAT, 32, 4, [59] + [128] * 4),                   # 32 features + PE(dir) + dir -> 128 x 3 -> 128
    "narrow_out": (ENC_POSENC, 3, 10, [60, 256, 256, 256, 128]),        # out < H
    "h64": (ENC_NONE, 32, 0, [32, 64, 64, 16]),                         # width 64, 3 layers (not a two-pass shape)
}
FLAGS = {"fp32": 0, "bf16x3": BF16X3, "f16x2": F16X2, "f16x2_layerwise": F16X2 | LAYERWISE,
         "f16x2_skip_rows": F16X2 | SKIP_LAST | ROWS_ONLY}
NS = [1, 32, 1000, 1 << 20]


class Desc(C.Structure):          # tn_mlp_desc (include/tinynerf_hip.h; test_abi checks tinynerf_amd._lib's mirror)
    _fields_ = [
        ("n_layers", C.c_int32), ("in_dim", C.c_int32), ("dims", C.c_int32 * 13),
        ("encoding", C.c_int32), ("n_freqs", C.c_int32), ("out_activation", C.c_int32), ("flags", C.c_int32),
        ("freqs", C.c_void_p), ("weights", C.c_void_p * 12), ("biases", C.c_void_p * 12),
        ("aux_index", C.c_void_p), ("aux_stride", C.c_int32), ("reserved", C.c_int32), ("row_gate", C.c_void_p),
        ("x_rows", C.c_void_p), ("grad_x_rows", C.c_void_p), ("x_rows_tile_stride", C.c_int64), ("grad_x_rows_tile_stride", C.c_int64),
        ("grad_x_mask_rows", C.c_void_p), ("grad_x_mask_tile_stride", C.c_int64),
    ]


def make_desc(cfg, flags):
    enc, in_dim, n_freqs, dims = CONFIGS[cfg]
    d = Desc()
    d.n_layers, d.in_dim, d.encoding, d.n_freqs, d.flags = len(dims) - 1, in_dim, enc, n_freqs, flags
    for i, v in enumerate(dims):
        d.dims[i] = v
    for l in range(len(dims) - 1):          # (never dereferenced by these host-only calls)
        d.weights[l] = d.biases[l] = 256
    return d


def query(lib, cfg, flags, n):
    d = make_desc(cfg, flags)
    out = {"bwd_bytes": lib.tn_mlp_bwd_workspace_bytes(C.byref(d), C.c_int64(n)),
           "fwd_bytes": lib.tn_mlp_fwd_workspace_bytes(C.byref(d), C.c_int64(n))}
    v = [C.c_int64(-7) for _ in range(4)]
    rc = lib.tn_mlp_rows_view(C.byref(d), C.c_int64(n), C.byref(v[0]), C.byref(v[1]), C.byref(v[2]))
    out["rows_view"] = [rc] + ([x.value for x in v[:3]] if rc == 0 else [])
    v = [C.c_int64(-7) for _ in range(4)]
    rc = lib.tn_mlp_rows_view_hidden(C.byref(d), C.c_int64(n), *[C.byref(x) for x in v])
    out["rows_view_hidden"] = [rc] + ([x.value for x in v] if rc == 0 else [])
    return out


@pytest.fixture(scope="module")
def lib():
    from tinynerf_amd import build
    lib = C.CDLL(build.build(verbose=False))
    lib.tn_mlp_bwd_workspace_bytes.restype = C.c_int64
    lib.tn_mlp_fwd_workspace_bytes.restype = C.c_int64
    return lib


def expected_bwd_bytes(cfg, flags, n, golden):
    """The training workspace: a 256-byte tail behind the rows, and the L - 1 gradient slabs of the data-gradient chain plus the
    packed weight stream only where the chain (and the cross-layer training forward) can run: slab layout, f16x2 without
    TN_MLP_LAYERWISE, output as wide as the hidden layers.  Every other wide stack keeps exactly the rows it uses."""
    n_tiles = (n + 31) // 32
    chain = flags & F16X2 and not flags & LAYERWISE
    if cfg in ("vanilla", "cobafa", "narrow_out") and not (chain and cfg != "narrow_out"):
        # slab layout: L - 1 activations, buffers A and B, one slab shared by the 64 input rows and the ReLU bit rows
        # (Vanilla 64 + 9 x 16, Cobafa 64 + 6 x 8, narrow_out 64 + 3 x 16 rows <= H)
        H, L = {"vanilla": (256, 10), "cobafa": (128, 7), "narrow_out": (256, 4)}[cfg]
        return (L + 2) * n_tiles * H * 128 + 256
    if cfg == "mlp100":           # tile-major: 4 x 256 activation rows, 2 x 256 gradient rows, 4 x 16 bit rows per tile
        return n_tiles * (4 * 256 + 2 * 256 + 4 * 16) * 128 + 256
    if cfg == "dircat":           # tile-major: 3 x 128 activations, 32 PE rows, 2 x 128 gradient rows, 3 x 8 bit rows
        return n_tiles * (3 * 128 + 32 + 2 * 128 + 3 * 8) * 128 + 256
    return golden


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_wide_stack_workspace_answers(lib, cfg):
    golden = json.load(open(GOLDEN))
    for fname, flags in FLAGS.items():
        for n in NS:
            key = "%s/%s/%d" % (cfg, fname, n)
            got, want = query(lib, cfg, flags, n), dict(golden[key])
            want["bwd_bytes"] = expected_bwd_bytes(cfg, flags, n, want["bwd_bytes"])
            assert got == want, key



# ---- the width-64 heads (two-pass form, csrc/mlp_bwd2.hip) ----
HEADS_GOLDEN = os.path.join(ROOT, "tests", "golden", "mlp_heads_workspace.json")
ENC_AUX_CAT = 3
STASHED, CHAIN_ONLY, WGRAD_ONLY, X_FROM_ROWS, LEAN = 2, 4, 8, 256, 512
PTR = 1 << 20           # a 16-byte aligned address that no call below dereferences
HEAD_FLAGS = {"fp32": 0, "bf16x3": BF16X3, "f16x2": F16X2, "f16x2_lean": F16X2 | LEAN}


def head_shapes():
    """the heads fused.py builds for K-Planes (F = 96), Vanilla (256) and Cobafa (128), and shapes that are not two-pass"""
    s = {}
    for name, F in (("kplanes", 96), ("vanilla", 256), ("cobafa", 128)):
        s[name + "_colour_aux"] = (ENC_AUX_CAT, F, 8, [F + 51, 64, 64, 64, 64, 3], 56)
        s[name + "_colour_dir"] = (ENC_DIR_CAT, F, 8, [F + 51, 64, 64, 64, 64, 3], 0)
        s[name + "_sigma"] = (ENC_NONE, F, 0, [F, 64, 1], 0)
    s["three_layers"] = (ENC_NONE, 96, 0, [96, 64, 64, 1], 0)
    s["width32"] = (ENC_NONE, 96, 0, [96, 32, 1], 0)
    s["five_outputs"] = (ENC_NONE, 96, 0, [96, 64, 64, 64, 64, 5], 0)
    return s


def head_desc(shape, flags=0, **kw):
    enc, in_dim, n_freqs, dims, aux_stride = head_shapes()[shape] if isinstance(shape, str) else shape
    d = Desc()
    d.n_layers, d.in_dim, d.encoding, d.n_freqs, d.flags, d.aux_stride = len(dims) - 1, in_dim, enc, n_freqs, flags, aux_stride
    d.out_activation = 0
    for i, v in enumerate(dims):
        d.dims[i] = v
    for l in range(len(dims) - 1):          # (never dereferenced: every call below is refused or host-only)
        d.weights[l] = d.biases[l] = PTR
    d.freqs = PTR
    d.aux_index = PTR if enc == ENC_AUX_CAT else None
    for k, v in kw.items():
        setattr(d, k, v)
    return d


LEAN_PAIRS = {          # (desc shape, partner shape, desc flags, partner flags, desc aux_stride override)
    "kplanes_f16x2": ("kplanes_colour_aux", "kplanes_sigma", F16X2, F16X2, None),
    "kplanes_f16x2_stride60": ("kplanes_colour_aux", "kplanes_sigma", F16X2, F16X2, 60),
    "kplanes_f16x2_stride58": ("kplanes_colour_aux", "kplanes_sigma", F16X2, F16X2, 58),
    "kplanes_f16x2_stride52": ("kplanes_colour_aux", "kplanes_sigma", F16X2, F16X2, 52),
    "kplanes_fp32": ("kplanes_colour_aux", "kplanes_sigma", 0, 0, None),
    "kplanes_partner_fp32": ("kplanes_colour_aux", "kplanes_sigma", F16X2, 0, None),
    "kplanes_dir": ("kplanes_colour_dir", "kplanes_sigma", F16X2, F16X2, None),
    "vanilla_f16x2": ("vanilla_colour_aux", "vanilla_sigma", F16X2, F16X2, None),
    "cobafa_f16x2": ("cobafa_colour_aux", "cobafa_sigma", F16X2, F16X2, None),
    "swapped": ("kplanes_sigma", "kplanes_colour_aux", F16X2, F16X2, None),
    "kplanes_three_layers": ("kplanes_colour_aux", "three_layers", F16X2, F16X2, None),
}


def lean_pair(name):
    a, b, fa, fb, stride = LEAN_PAIRS[name]
    da = head_desc(a, fa)
    if stride is not None:
        da.aux_stride = stride
    return da, head_desc(b, fb)


def test_head_workspace_answers(lib):
    """tn_mlp_bwd_workspace_bytes of the heads and tn_mlp_lean_supported, as the library answered before the heads' launches came
    from one plan"""
    golden = json.load(open(HEADS_GOLDEN))
    for shape in head_shapes():
        for fname, flags in HEAD_FLAGS.items():
            for n in NS:
                key = "%s/%s/%d" % (shape, fname, n)
                assert lib.tn_mlp_bwd_workspace_bytes(C.byref(head_desc(shape, flags)), C.c_int64(n)) == golden["bwd_bytes"][key], key
    for name in LEAN_PAIRS:
        da, db = lean_pair(name)
        assert lib.tn_mlp_lean_supported(C.byref(da), C.byref(db)) == golden["lean_supported"][name], name


class KDesc(C.Structure):         # tn_kplanes_desc
    _fields_ = [("n_scales", C.c_int32), ("channels", C.c_int32), ("height", C.c_int32 * 4), ("width", C.c_int32 * 4),
                ("planes", (C.c_void_p * 3) * 4)]


def kdesc(n_scales=3, channels=32, plane=PTR):
    k = KDesc()
    k.n_scales, k.channels = n_scales, channels
    for s in range(4):
        k.height[s] = k.width[s] = 64
        for p in range(3):
            k.planes[s][p] = PTR
    k.planes[1][2] = plane
    return k


def grads(n, null_at=None):
    g = (C.c_void_p * 12)(*([PTR] * 12))
    if null_at is not None:
        g[null_at] = None
    return g


WS = 1 << 40                      # workspace bytes: large enough for every n below


def call(lib, entry, shape="kplanes_colour_aux", partner="kplanes_sigma", flags=STASHED, pflags=STASHED, n=1000, kd=None,
         coord_stride=7, x=PTR, ws=PTR, y=PTR, py=PTR, gx=PTR, gw=None, pgw=None, feat=PTR, pkw=None, **kw):
    d = head_desc(shape, flags, **kw) if shape else None
    p = head_desc(partner, pflags, **(pkw or {})) if partner else None
    k = kd if kd is not None else kdesc()
    gw, pgw = gw or grads(5), pgw or grads(2)
    gp = ((C.c_void_p * 3) * 4)()
    D, P, K, n = (C.byref(d) if d else None), (C.byref(p) if p else None), C.byref(k), C.c_int64(n)
    if entry == "tn_mlp_fwd":
        return lib.tn_mlp_fwd(D, x, PTR, n, y, None, None)
    if entry == "tn_mlp_fwd_stash":
        return lib.tn_mlp_fwd_stash(D, x, PTR, n, y, ws, C.c_int64(WS), None)
    if entry == "tn_mlp_fwd_stash_pair":
        return lib.tn_mlp_fwd_stash_pair(D, P, x, PTR, n, y, py, ws, C.c_int64(WS), ws, C.c_int64(WS), None)
    if entry == "tn_kplanes_mlp_fwd":
        return lib.tn_kplanes_mlp_fwd(K, x, C.c_int64(coord_stride), D, n, PTR, y, None)
    if entry == "tn_kplanes_mlp_fwd_pair":
        return lib.tn_kplanes_mlp_fwd_pair(K, x, C.c_int64(coord_stride), D, P, PTR, n, feat, y, py, ws, C.c_int64(WS), ws, C.c_int64(WS), None)
    if entry == "tn_mlp_bwd":
        return lib.tn_mlp_bwd(D, x, PTR, PTR, n, gw, gw, gx, ws, C.c_int64(WS), None)
    if entry == "tn_mlp_bwd_pair":
        return lib.tn_mlp_bwd_pair(D, P, x, PTR, PTR, PTR, n, gw, gw, pgw, pgw, gx, ws, C.c_int64(WS), ws, C.c_int64(WS), None)
    if entry == "tn_kplanes_mlp_bwd_pair":
        return lib.tn_kplanes_mlp_bwd_pair(K, x, C.c_int64(coord_stride), gp, D, P, PTR, PTR, PTR, PTR, n, gw, gw, pgw, pgw, gx, ws,
                                           C.c_int64(WS), ws, C.c_int64(WS), None)
    raise KeyError(entry)


E_NULL, E_SIZE, E_CONFIG, E_ALIGN = -1, -2, -3, -4
F2S, F2L = F16X2 | STASHED, F16X2 | STASHED | LEAN
# (entry, expected TN_E_*, keyword arguments of call()).  Rows marked "moved" were refused by the parent only after a kernel had run.
REFUSALS = [
    ("tn_mlp_fwd", E_NULL, dict(shape=None)),
    ("tn_mlp_fwd", E_SIZE, dict(shape="kplanes_sigma", n=-1)),
    ("tn_mlp_fwd", E_NULL, dict(shape="kplanes_sigma", x=None)),
    ("tn_mlp_fwd", E_ALIGN, dict(shape="kplanes_sigma", x=PTR + 4)),
    ("tn_mlp_fwd", E_CONFIG, dict(shape="kplanes_sigma", flags=F16X2 | X_FROM_ROWS)),
    ("tn_mlp_fwd", E_CONFIG, dict(shape=(ENC_NONE, 96, 0, [96, 48, 1], 0))),
    ("tn_mlp_fwd_stash", E_NULL, dict(shape=None)),
    ("tn_mlp_fwd_stash", E_SIZE, dict(shape="kplanes_sigma", n=-1)),
    ("tn_mlp_fwd_stash", E_NULL, dict(shape="kplanes_sigma", ws=None)),
    ("tn_mlp_fwd_stash", E_ALIGN, dict(shape="kplanes_sigma", ws=PTR + 4)),
    ("tn_mlp_fwd_stash", E_CONFIG, dict(shape="kplanes_sigma", flags=X_FROM_ROWS)),
    ("tn_mlp_fwd_stash", E_CONFIG, dict(shape="kplanes_sigma", flags=F16X2 | LEAN)),
    ("tn_mlp_fwd_stash_pair", E_NULL, dict(partner=None)),
    ("tn_mlp_fwd_stash_pair", E_CONFIG, dict(shape="kplanes_colour_dir")),
    ("tn_mlp_fwd_stash_pair", E_SIZE, dict(n=-1)),
    ("tn_mlp_fwd_stash_pair", E_NULL, dict(ws=None)),
    ("tn_mlp_fwd_stash_pair", E_ALIGN, dict(ws=PTR + 4)),
    ("tn_mlp_fwd_stash_pair", E_NULL, dict(py=None)),
    ("tn_mlp_fwd_stash_pair", E_CONFIG, dict(flags=LEAN, pflags=LEAN)),
    ("tn_mlp_fwd_stash_pair", E_CONFIG, dict(flags=X_FROM_ROWS)),
    ("tn_kplanes_mlp_fwd", E_NULL, dict(shape=None)),
    ("tn_kplanes_mlp_fwd", E_CONFIG, dict(shape="kplanes_colour_aux")),
    ("tn_kplanes_mlp_fwd", E_SIZE, dict(shape="kplanes_sigma", n=-1)),
    ("tn_kplanes_mlp_fwd", E_CONFIG, dict(shape="kplanes_sigma", kd=kdesc(n_scales=2))),
    ("tn_kplanes_mlp_fwd", E_SIZE, dict(shape="kplanes_sigma", coord_stride=2)),
    ("tn_kplanes_mlp_fwd", E_NULL, dict(shape="kplanes_sigma", x=None)),
    ("tn_kplanes_mlp_fwd", E_NULL, dict(shape="kplanes_sigma", kd=kdesc(plane=None))),
    ("tn_kplanes_mlp_fwd", E_ALIGN, dict(shape="kplanes_sigma", kd=kdesc(plane=PTR + 4))),
    ("tn_kplanes_mlp_fwd", E_ALIGN, dict(shape="kplanes_sigma", y=None)),
    ("tn_kplanes_mlp_fwd", E_CONFIG, dict(shape="kplanes_sigma", flags=X_FROM_ROWS)),
    ("tn_kplanes_mlp_fwd_pair", E_NULL, dict(partner=None)),
    ("tn_kplanes_mlp_fwd_pair", E_CONFIG, dict(kd=kdesc(n_scales=2))),
    ("tn_kplanes_mlp_fwd_pair", E_CONFIG, dict(shape="vanilla_colour_aux")),
    ("tn_kplanes_mlp_fwd_pair", E_SIZE, dict(coord_stride=2)),
    ("tn_kplanes_mlp_fwd_pair", E_SIZE, dict(n=-1)),
    ("tn_kplanes_mlp_fwd_pair", E_NULL, dict(x=None)),
    ("tn_kplanes_mlp_fwd_pair", E_NULL, dict(kd=kdesc(plane=None))),
    ("tn_kplanes_mlp_fwd_pair", E_ALIGN, dict(kd=kdesc(plane=PTR + 4))),
    ("tn_kplanes_mlp_fwd_pair", E_NULL, dict(py=None)),
    ("tn_kplanes_mlp_fwd_pair", E_ALIGN, dict(y=PTR + 4)),
    ("tn_kplanes_mlp_fwd_pair", E_CONFIG, dict(shape="kplanes_colour_dir")),
    ("tn_kplanes_mlp_fwd_pair", E_CONFIG, dict(flags=LEAN, pflags=LEAN)),
    # the inference pair form (both workspaces NULL): the dummy operand line lies in the coordinates when there are no feature rows
    ("tn_kplanes_mlp_fwd_pair", E_ALIGN, dict(ws=None, x=PTR + 4)),
    ("tn_kplanes_mlp_fwd_pair", E_ALIGN, dict(ws=None, x=PTR + 4, feat=None)),
    ("tn_kplanes_mlp_fwd_pair", E_SIZE, dict(ws=None, feat=None, n=1, coord_stride=3)),
    ("tn_kplanes_mlp_fwd_pair", E_CONFIG, dict(ws=None, row_gate=PTR)),
    ("tn_kplanes_mlp_fwd_pair", E_CONFIG, dict(ws=None, pkw=dict(row_gate=PTR))),
    ("tn_kplanes_mlp_fwd_pair", E_CONFIG, dict(ws=None, feat=None, row_gate=PTR)),
    ("tn_mlp_bwd", E_NULL, dict(shape=None)),
    ("tn_mlp_bwd", E_CONFIG, dict(shape=(ENC_AUX_CAT, 96, 8, [147, 64, 64, 64, 3], 56))),
    ("tn_mlp_bwd", E_NULL, dict(ws=None)),
    ("tn_mlp_bwd", E_NULL, dict(x=None)),
    ("tn_mlp_bwd", E_ALIGN, dict(ws=PTR + 4)),
    ("tn_mlp_bwd", E_NULL, dict(gw=grads(5, null_at=3))),
    ("tn_mlp_bwd", E_CONFIG, dict(shape=(ENC_AUX_CAT, 96, 8, [147, 64, 3], 56))),                                    # moved
    ("tn_mlp_bwd_pair", E_NULL, dict(partner=None)),
    ("tn_mlp_bwd_pair", E_CONFIG, dict(pflags=0)),
    ("tn_mlp_bwd_pair", E_CONFIG, dict(partner="three_layers")),
    ("tn_mlp_bwd_pair", E_CONFIG, dict(shape="vanilla_colour_aux")),
    ("tn_mlp_bwd_pair", E_NULL, dict(ws=None)),
    ("tn_mlp_bwd_pair", E_NULL, dict(gx=None)),
    ("tn_mlp_bwd_pair", E_NULL, dict(pgw=grads(2, null_at=1))),
    ("tn_mlp_bwd_pair", E_CONFIG, dict(flags=STASHED | CHAIN_ONLY | WGRAD_ONLY)),
    ("tn_mlp_bwd_pair", E_CONFIG, dict(flags=F2L, pflags=F2S)),
    ("tn_mlp_bwd_pair", E_CONFIG, dict(flags=STASHED | LEAN, pflags=STASHED | LEAN)),                                 # moved
    ("tn_mlp_bwd_pair", E_CONFIG, dict(shape="vanilla_colour_aux", partner="vanilla_sigma", flags=F2L, pflags=F2L)),
    ("tn_mlp_bwd_pair", E_CONFIG, dict(shape="cobafa_colour_aux", partner="cobafa_sigma", flags=F2L, pflags=F2L)),          # moved
    ("tn_kplanes_mlp_bwd_pair", E_NULL, dict(partner=None)),
    ("tn_kplanes_mlp_bwd_pair", E_CONFIG, dict(kd=kdesc(n_scales=2))),
    ("tn_kplanes_mlp_bwd_pair", E_CONFIG, dict(shape="kplanes_colour_dir")),
    ("tn_kplanes_mlp_bwd_pair", E_SIZE, dict(coord_stride=2)),
    ("tn_kplanes_mlp_bwd_pair", E_NULL, dict(x=None)),
    ("tn_kplanes_mlp_bwd_pair", E_NULL, dict(kd=kdesc(plane=None))),
    ("tn_kplanes_mlp_bwd_pair", E_CONFIG, dict(partner="three_layers")),
    ("tn_kplanes_mlp_bwd_pair", E_NULL, dict(ws=None)),
    ("tn_kplanes_mlp_bwd_pair", E_CONFIG, dict(flags=F2L, pflags=F2S)),
    ("tn_kplanes_mlp_bwd_pair", E_CONFIG, dict(flags=STASHED | LEAN, pflags=STASHED | LEAN)),                         # moved
]


def test_head_refusals_come_before_any_launch(lib):
    """Every call below is refused before the first HIP call: on a host without a GPU, a call that launched first would return the
    HIP error of that launch instead.  (Skipped where a GPU exists: a regression would launch on dummy pointers there.)"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("refusal table runs on dummy pointers: host without a GPU only")
    for i, (entry, want, kw) in enumerate(REFUSALS):
        assert call(lib, entry, **kw) == want, (i, entry, kw)
