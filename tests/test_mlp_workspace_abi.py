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

