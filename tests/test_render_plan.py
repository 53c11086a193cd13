"""CPU golden of the fused render nodes' launches (tinynerf_amd/fused.py): K-Planes, Vanilla and Cobafa renderers, forward and
backward, under the three arithmetics and the f16x2 path's switches.  ``_lib.call`` is replaced by a recorder and ``_lib.require_cuda``
by a stub, so nothing runs on a device; the host-only answers (workspace bytes, lean support, row views) come from the real library.
Every launch is recorded with its entry point, each MLP descriptor's flags and null / non-null row_gate, x_rows and grad_x_rows, and
every pointer argument as null or not.  tests/golden/render_node_launches.json holds the sequences the nodes launched before they were
driven from host-side plans; they must be reproduced exactly.

Regenerate (only when a change of the launches is intended): python tests/test_render_plan.py --write"""
import ctypes as C
import itertools
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "render_node_launches.json")

from tinynerf_amd import _lib as L, build, config, core, fused, models  # noqa: E402


def _arg(a):
    obj = getattr(a, "_obj", None)              # C.byref(...)
    if isinstance(obj, L.MlpDesc):
        return "mlp(flags=%d,row_gate=%d,x_rows=%d,grad_x_rows=%d)" % (obj.flags, bool(obj.row_gate), bool(obj.x_rows), bool(obj.grad_x_rows))
    if isinstance(obj, L.KPlanesDesc):
        return "kplanes(%d x %d)" % (obj.n_scales, obj.channels)
    if isinstance(a, C.c_void_p):
        return "ptr" if a.value else "null"
    if isinstance(a, (C.c_int64, C.c_int32, C.c_int)):
        return str(a.value)
    if isinstance(a, C.c_float):
        return "float"
    if isinstance(a, C.Array):
        return "array[%d]" % len(a)
    return type(a).__name__


class _Slot:
    """a measurement of the inference live fraction still in flight (no pinned copy, no event: nothing here needs a device)"""

    def query(self):
        return False


def _in_flight(value, pair_on=False):
    return {"slots": [{"pinned": torch.ones(1), "event": _Slot(), "seq": k + 1} for k in range(4)], "seq": 4, "seen": 0,
            "value": value, "pair_on": pair_on}


def _batch(R=6, per_ray=11):
    torch.manual_seed(0)
    cnt = torch.full((R,), per_ray, dtype=torch.int32)
    info = torch.stack([torch.cumsum(cnt, 0, dtype=torch.int32) - cnt, cnt], -1)
    packed = torch.rand(int(cnt.sum()), 7)
    return packed, info


def _hint(packed, info, planes_ready=None):
    n, R = packed.size(0), info.size(0)
    return {"key": (packed.data_ptr(), n, R), "ray_ids": torch.zeros(n, dtype=torch.int32), "steps": torch.zeros(n),
            "dirs": torch.zeros(R, 3), "planes_ready": planes_ready, "gate": torch.zeros(1)}


def _kplanes(channels=32, scales=3):
    field = models.KPlanesFeatureField(channels, [8 + 4 * s for s in range(scales)])
    F = channels * scales
    return core.NerfRenderer(field, models.VanillaOpacityDecoder(F), models.VanillaColorDecoder(8, F, 64, 3), torch.ones(3))


def _wide(kind):
    if kind == "vanilla":
        fm = models.VanillaFeatureMLP(10, 256, 8)
    else:                   # Cobafa's 36 -> 128 x 6 stack; the grids' own launches are not the render node's, their features are a leaf here
        fm = models.CobafaFeatureField([4] * 6, 4, [2.0] * 6, [8, 8, 8, 4, 4, 4], 128)
        leaf = torch.zeros(1024, 36, requires_grad=True)
        fm.features = lambda x: leaf[:x.size(0)]
    dim = fm.feature_dim
    return core.NerfRenderer(fm, models.VanillaOpacityDecoder(dim), models.VanillaColorDecoder(8, dim, 64, 3), torch.ones(3))


def _trainer_style(r):
    """what run.Trainer sets up: gradient buffers, accumulation into them, the arena and the wide stacks' scratch with the row link"""
    for p in r.parameters():
        p.grad = torch.zeros_like(p)
    r.accumulate_into_grad = r.reuse_buffers = True
    arena = fused.Arena()
    for i, m in enumerate(mod for mod in r.feature_module.modules() if isinstance(mod, models.MLP)):
        m.__dict__["scratch"] = (arena, f"mlp_ws{i}", {}, True, {})
    return r


# name: (field, arithmetic, switches, train, options)
_KP = {"fuse_gather": True, "fuse_scatter": True}


def _scenarios():
    s = {}
    for mm in config.MATMULS:
        s[f"kplanes/{mm}/train"] = ("kplanes", mm, {}, True, {"trainer": True})
        s[f"kplanes/{mm}/infer"] = ("kplanes", mm, {}, False, {})
        for kind in ("vanilla", "cobafa"):
            s[f"{kind}/{mm}/train_link"] = (kind, mm, {}, True, {"trainer": True, "steps": 2})
            s[f"{kind}/{mm}/train"] = (kind, mm, {}, True, {})
            s[f"{kind}/{mm}/infer"] = (kind, mm, {}, False, {})
    f2 = "f16x2"
    s["kplanes/f16x2/train/no_fuse_gather"] = ("kplanes", f2, {"fuse_gather": False}, True, {"trainer": True})
    s["kplanes/f16x2/train/no_fuse_scatter"] = ("kplanes", f2, {"fuse_scatter": False}, True, {"trainer": True})
    s["kplanes/f16x2/train/no_fuse"] = ("kplanes", f2, {"fuse_gather": False, "fuse_scatter": False}, True, {"trainer": True})
    s["kplanes/f16x2/train/no_lean"] = ("kplanes", f2, {"kp_lean": False}, True, {"trainer": True})
    s["kplanes/f16x2/train/no_lean/no_fuse"] = ("kplanes", f2, {"kp_lean": False, "fuse_gather": False, "fuse_scatter": False}, True,
                                                {"trainer": True})
    s["kplanes/f16x2/train/planes_ready"] = ("kplanes", f2, {}, True, {"trainer": True, "planes_ready": True})
    s["kplanes/f16x2/train/planes_ready/no_fuse_scatter"] = ("kplanes", f2, {"fuse_scatter": False}, True,
                                                            {"trainer": True, "planes_ready": True})
    s["kplanes/f16x2/train/no_hint"] = ("kplanes", f2, {}, True, {})
    s["kplanes/f16x2/train/frozen_planes"] = ("kplanes", f2, {}, True, {"trainer": True, "frozen_planes": True})
    s["kplanes/f16x2/infer/hint"] = ("kplanes", f2, {}, False, {"hint": True})
    s["kplanes/f16x2/infer/no_fuse_gather"] = ("kplanes", f2, {"fuse_gather": False}, False, {"live": (0.9, False)})
    for label, live in (("landed_above", (0.9, False)), ("in_band_on", (0.5, True)), ("in_band_off", (0.5, False)),
                        ("landed_below", (0.1, True))):
        s[f"kplanes/f16x2/infer/{label}"] = ("kplanes", f2, {}, False, {"live": live})
        s[f"kplanes/f16x2/infer/{label}/no_infer_pair"] = ("kplanes", f2, {"infer_pair": False}, False, {"live": live})
    s["kplanes/f16x2/infer/not_landed"] = ("kplanes", f2, {}, False, {"live": (None, False)})
    for shape, (ch, sc) in (("c16x3", (16, 3)), ("c32x2", (32, 2))):
        s[f"kplanes_{shape}/f16x2/train"] = ("kplanes", f2, {}, True, {"trainer": True, "shape": (ch, sc)})
        s[f"kplanes_{shape}/f16x2/train/planes_ready"] = ("kplanes", f2, {}, True, {"trainer": True, "shape": (ch, sc), "planes_ready": True})
        s[f"kplanes_{shape}/f16x2/train/no_hint"] = ("kplanes", f2, {}, True, {"shape": (ch, sc)})
        s[f"kplanes_{shape}/f16x2/infer"] = ("kplanes", f2, {}, False, {"shape": (ch, sc), "live": (0.9, False)})
        s[f"kplanes_{shape}/fp32/train"] = ("kplanes", "fp32", {}, True, {"trainer": True, "shape": (ch, sc)})
    for kind in ("vanilla", "cobafa"):
        for sw in ("heads_pair", "rows_handoff", "merge_last"):
            s[f"{kind}/f16x2/train_link/no_{sw}"] = (kind, f2, {sw: False}, True, {"trainer": True, "steps": 2})
        s[f"{kind}/f16x2/train_link/no_heads_pair/no_merge_last"] = (kind, f2, {"heads_pair": False, "merge_last": False}, True,
                                                                     {"trainer": True, "steps": 2})
        s[f"{kind}/f16x2/infer_trainer"] = (kind, f2, {}, False, {"trainer": True})
    return s


def run_scenario(name, spec, mp):
    kind, mm, switches, train, opt = spec
    cfg = config.Config(matmul=mm, **{k: v for k, v in switches.items() if k not in _KP}).validate()
    mp.setattr(models, "MATMUL", cfg.matmul)
    for attr, val in (("ROWS_HANDOFF", cfg.rows_handoff), ("MERGE_LAST", cfg.merge_last), ("HEADS_PAIR_BACKWARD", cfg.heads_pair),
                      ("KP_LEAN", cfg.kp_lean), ("INFER_PAIR", cfg.infer_pair), ("FUSE_GATHER", switches.get("fuse_gather", True)),
                      ("FUSE_SCATTER", switches.get("fuse_scatter", True))):
        mp.setattr(fused, attr, val)
    seq = []

    def call(fn, dev, *args):
        seq.append("%s(%s)" % (fn, ", ".join(_arg(a) for a in args)))

    def require(*ts):
        return next(t.device for t in ts if t is not None)
    mp.setattr(L, "call", call)
    mp.setattr(L, "require_cuda", require)
    torch.manual_seed(1)
    r = _kplanes(*opt.get("shape", (32, 3))) if kind == "kplanes" else _wide(kind)
    if opt.get("frozen_planes"):
        for p in r.feature_module.plane_tensors():
            p.requires_grad_(False)
    if opt.get("trainer"):
        _trainer_style(r)
    packed, info = _batch()
    ready = (lambda grads: seq.append("planes_ready(%d)" % len(grads))) if opt.get("planes_ready") else None
    if opt.get("trainer") or opt.get("hint"):
        r._batch_aux = _hint(packed, info, ready)
    r.__dict__["_stats"] = {"infer_live": _in_flight(*opt.get("live", (None, False)))}
    for step in range(opt.get("steps", 1)):
        seq.append("-- step %d forward" % step)
        if train:
            out = fused.render(r, packed, info, 1e-4, r.accumulate_into_grad)
            seq.append("-- backward")
            out.sum().backward()
        else:
            with torch.no_grad():
                fused.render(r, packed, info, 1e-4, r.accumulate_into_grad)
    if getattr(r, "_arena", None) is not None:
        seq.append("-- arena " + ", ".join("%s:%s" % (k, v.numel()) for k, v in sorted(r._arena.buf.items())))
    return seq


@pytest.fixture(scope="module")
def library():
    path = build.build(verbose=False)
    assert path == L.LIB_PATH or os.path.samefile(path, L.LIB_PATH)
    return L.lib()


def record_all():
    out = {}
    for name, spec in _scenarios().items():
        with pytest.MonkeyPatch.context() as mp:
            out[name] = run_scenario(name, spec, mp)
    return out


@pytest.mark.parametrize("name", list(_scenarios()))
def test_render_node_launches(library, name, monkeypatch):
    golden = json.load(open(GOLDEN))
    assert run_scenario(name, _scenarios()[name], monkeypatch) == golden[name]


def test_lean_forward_implies_paired_backward(library, monkeypatch):
    """a K-Planes plan never pairs a lean forward (no hidden activations stashed) with a backward that would need them"""
    paired = (fused._KpBwd.SCATTER_CHAIN, fused._KpBwd.PAIR_SPLIT, fused._KpBwd.PAIR)
    seen = set()
    for mm in config.MATMULS:
        monkeypatch.setattr(models, "MATMUL", mm)
        for (ch, sc), sigma_layers in itertools.product(((32, 3), (16, 3), (32, 2), (16, 2), (32, 1)), (0, 1)):
            r = _kplanes(ch, sc)
            F = ch * sc
            sig_p = models.MLP(F, 64, sigma_layers, 1).params()
            rgb_p = r.rgb_decoder.net.params()
            kdesc, keep = models._kplanes_desc(r.feature_module.plane_tensors())
            table, ray_ids = torch.zeros(6, 56), torch.zeros(66, dtype=torch.int32)
            rdesc, sdesc = fused._head_descs(sig_p, rgb_p, F, 8, r.rgb_decoder.pe.freqs, ray_ids, table)
            sb, rb = fused._workspace(sdesc, 66, torch.device("cpu"))[1], fused._workspace(rdesc, 66, torch.device("cpu"))[1]
            for lean, gather, scatter, ready in itertools.product((True, False), repeat=4):
                monkeypatch.setattr(fused, "KP_LEAN", lean)
                monkeypatch.setattr(fused, "FUSE_GATHER", gather)
                monkeypatch.setattr(fused, "FUSE_SCATTER", scatter)
                plan = fused._plan_kplanes(kdesc, keep, rdesc, sdesc, sig_p, rgb_p, True, sb, rb, True, ready, None)
                assert not plan.lean or plan.bwd in paired, (mm, ch, sc, sigma_layers, plan)
                seen.add((plan.lean, plan.bwd))
    assert (True, fused._KpBwd.SCATTER_CHAIN) in seen and (False, fused._KpBwd.SEPARATE) in seen


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_render_plan.py --write")
    build.build(verbose=False)
    with open(GOLDEN, "w") as f:
        json.dump(record_all(), f, indent=1, sort_keys=True)
        f.write("\n")
