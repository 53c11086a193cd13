"""Fused K-Planes render path: the whole of ``NerfRenderer.forward`` (reference core.py:225-267) as one
autograd node that drives the C-ABI kernels back to back on the current stream.

The module-by-module path in ``core.NerfRenderer`` mirrors the reference's data flow, including its
boolean gather of the samples with w > 0 (a host sync, a [M,96] gather, an index_copy and their autograd
counterparts).  Here every sample goes through the colour head in place -- samples with w == 0 contribute
exactly 0 to the composite in both directions, as in the reference -- so there is no sync, no gather and
no intermediate autograd graph: forward = gather+sigma -> weights scan -> colour -> composite,
backward = composite -> colour head -> weights -> sigma head -> plane scatter, 9 launches in total.
Parameter gradients are accumulated straight into ``param.grad`` when it exists (the harness keeps the
gradient buffers allocated), which saves two passes over the 126 MiB of plane gradients per step.
"""
from __future__ import annotations

import ctypes as C
import enum
from dataclasses import dataclass
from typing import Any, Callable, List, Optional, Sequence, Tuple

import torch
from torch.autograd import Function

from . import _lib as L
from .arena import Arena
from .config import CONFIG
from .models import _empty_rows, _hwc, _kplanes_desc, _mlp_desc


# Heads behind a wide stack take their first-layer operands from the stack's workspace rows, and the stack stops writing the row-major
# copy (TN_MLP_ROWS_ONLY / TN_MLP_X_FROM_ROWS; f16x2 heads only).  TN_ROWS_HANDOFF=0: row-major as before (A/B runs, tests).
ROWS_HANDOFF = CONFIG.rows_handoff


def MATMUL_F16X2() -> bool:
    from . import models
    return ROWS_HANDOFF and models.MATMUL == "f16x2"


FUSE_GATHER = True        # the K-Planes gather inside the heads' forward launch (tn_kplanes_mlp_fwd_pair, tn_kplanes_mlp_fwd)
FUSE_SCATTER = True       # backward: the plane scatter inside the data-gradient chain launch (tn_kplanes_mlp_bwd_pair)
# behind the wide stacks (_RenderHeads; round 5): tn_mlp_bwd_pair takes both heads' first-layer weight gradients over the x
# columns in ONE launch (x rows read once) and, where both first layers fit LDS (128-wide stack), both data gradients in one pass; "0": off
HEADS_PAIR_BACKWARD = CONFIG.heads_pair
# round 5 (TN_MLP_SKIP_LAST): behind a wide stack whose last layer is a plain Linear (Vanilla 256 -> 256, Cobafa 128 -> 128: reference
# models.py:59-68,239-247) the heads' first layers are Linear too -- the harness merges the two (W_head W_last, W_head b_last + b_head: five
# small torch matmuls per step, differentiable, so the original parameters get their gradients by the chain rule) and the stack stops at its
# last hidden activation: one layer launch less in the forward pass, two less in the backward pass, the feature tensor never exists
MERGE_LAST = CONFIG.merge_last
# round 5 (TN_MLP_LEAN): the paired f16x2 training forward writes masks / pre-activations / feature rows only, the weight-gradient launches
# rebuild the hidden activations from the feature rows (csrc/mlp_wgrad_rc.hip) -- 2.7 GB less workspace traffic per K-Planes step.
# TN_KP_LEAN=0: the stash-everything form of rounds 1-4 (A/B runs; always taken by the fp32 / bf16x3 head forms)
KP_LEAN = CONFIG.kp_lean


def _alloc(arena: Optional[Arena], name: str, shape, dev: torch.device, dtype=torch.float32) -> torch.Tensor:
    return arena.get(name, shape, dev, dtype) if arena is not None else torch.empty(tuple(shape), device=dev, dtype=dtype)


def _workspace(desc: L.MlpDesc, n: int, dev: torch.device, arena: Optional[Arena] = None, name: str = "ws"):
    fn = L.lib().tn_mlp_bwd_workspace_bytes
    fn.restype = C.c_int64
    nbytes = int(fn(C.byref(desc), C.c_int64(n)))
    if not nbytes:
        return None, 0
    return _alloc(arena, name, (nbytes // 4,), dev), nbytes


def _covered(hint: Optional[dict], packed: torch.Tensor, R: int) -> bool:
    """the trainer's sampler wrote ray ids, steps and ray directions for exactly this batch and covers every sample"""
    return hint is not None and hint.get("key") == (packed.data_ptr(), packed.size(0), R)


def _ray_aux(packed: torch.Tensor, info: torch.Tensor, freqs: torch.Tensor, n_freqs: int, arena: Optional[Arena], hint: Optional[dict]):
    """Per-ray inputs of the colour head (models.py:87: cat[PE(d), d]): evaluated once per ray into a table
    (tn_dir_encode) that the MLP kernels index through the ray id of every sample, instead of 48 sin/cos per sample.
    Returns (table, ray_ids, steps).  ``hint``: ray ids / steps / ray directions the sampler already wrote out
    for exactly this batch (run.Trainer.build_batch); otherwise they are rebuilt from (packed, info)."""
    dev = packed.device
    n, R = packed.size(0), info.size(0)
    stride = (6 * n_freqs + 3 + 7) & ~7
    table = _alloc(arena, "aux_table", (R, stride), dev)
    if _covered(hint, packed, R):
        ray_ids, steps, dirs_ray = hint["ray_ids"], hint["steps"], hint["dirs"]
    else:
        ray_ids = _alloc(arena, "ray_ids", (n,), dev, torch.int32)
        steps = _alloc(arena, "steps", (n,), dev)
        dirs_ray = _alloc(arena, "dirs_ray", (R, 3), dev)
        L.call("tn_ray_aux", dev, L.ptr(packed), L.ptr(info), C.c_int64(R), L.ptr(ray_ids), L.ptr(steps), L.ptr(dirs_ray))
    if n > 0:
        L.call("tn_dir_encode", dev, L.ptr(dirs_ray), C.c_int64(R), L.ptr(freqs), C.c_int(n_freqs), L.ptr(table), C.c_int(stride))
    return table, ray_ids, steps


def _gate_slot(hint: Optional[dict], wanted: bool) -> Optional[torch.Tensor]:
    """the trainer's "Empty iteration" flag slot for this batch (the weights kernel only ever RAISES it): fresh -- zeroed by the
    ring's lap -- for the first forward on a batch, cleared here for any further forward on the same batch (another threshold,
    other parameters), which would otherwise inherit the earlier forward's 1.0"""
    if not wanted or hint is None or hint.get("gate") is None:
        return None
    if hint.get("gate_used"):
        hint["gate"].zero_()
    hint["gate_used"] = True
    return hint["gate"]


INFER_PAIR = CONFIG.infer_pair       # (TN_INFER_PAIR=0: always the gated inference form -- A/B, debugging)
INFER_PAIR_MIN_LIVE = 0.6       # the pair form is taken at >= this live fraction ...
INFER_PAIR_HYSTERESIS = 0.15    # ... and kept until the fraction falls below MIN_LIVE - HYSTERESIS (chunks of an image alternate between background
                                # and object: without the band the form -- not the result -- would flip from chunk to chunk)


def _infer_prefers_pair(stats: Optional[dict]) -> bool:
    """live-sample fraction (w > 0) of the most recent inference call on this renderer whose measurement has LANDED, read without
    a host sync: the values travel to a small ring of pinned slots, each behind its own event.  Until one has landed the gated
    form runs: on a trained scene (most samples behind a terminated ray) it is 4 x faster than the pair form (48 against 188 ms
    per 800 x 800 image), on a field that is alive everywhere only 1.4 x slower -- the cheap mistake is the default."""
    st = None if stats is None else stats.get("infer_live")
    if st is None:
        return False
    for slot in st["slots"]:
        if slot["seq"] > st["seen"] and slot["event"].query():
            st["seen"], st["value"] = slot["seq"], float(slot["pinned"][0])
    if st["value"] is None:
        return False
    on = st.get("pair_on", False)
    on = st["value"] >= (INFER_PAIR_MIN_LIVE - INFER_PAIR_HYSTERESIS if on else INFER_PAIR_MIN_LIVE)
    st["pair_on"] = on
    return on


def _note_live_fraction(stats: dict, weights: torch.Tensor) -> None:
    st = stats.get("infer_live")
    if st is None:
        st = stats["infer_live"] = {"slots": [{"pinned": torch.ones(1, pin_memory=True), "event": torch.cuda.Event(), "seq": 0} for _ in range(4)],
                                    "seq": 0, "seen": 0, "value": None}
    if not weights.numel():
        return
    for slot in st["slots"]:                      # a slot whose previous measurement has landed (or that was never used)
        if slot["seq"] == 0 or (slot["seq"] <= st["seen"]) or slot["event"].query():
            if slot["seq"] > st["seen"]:          # landed but not read yet: read it before it is overwritten
                st["seen"], st["value"] = slot["seq"], float(slot["pinned"][0])
            st["seq"] += 1
            slot["seq"] = st["seq"]
            # (one reduction launch + one 4-byte copy; the count is divided on the host side of the pinned slot)
            slot["pinned"].copy_((torch.count_nonzero(weights) / float(weights.numel())).reshape(1).float(), non_blocking=True)
            slot["event"].record(torch.cuda.current_stream(weights.device))
            return
    # every slot still in flight: skip this measurement


@dataclass
class _Call:
    """A render node's inputs that are not tensors (render())."""
    thr: float
    n_freqs: int
    n_planes: int               # the parameters: K-Planes' planes (none for _RenderHeads), the sigma head's, the colour head's
    n_sigma: int
    accumulate: bool            # weight gradients go straight into param.grad where it exists (the trainer keeps it allocated)
    arena: Optional[Arena]
    train: bool
    hint: Optional[dict]        # run.Trainer.build_batch's _batch_aux
    stats: Optional[dict]       # the renderer's _stats
    link: Optional[dict] = None     # _RenderHeads: row views offered by the wide stack that produced feat
    # NerfRenderer.render_with_distortion: {"t": [n], "warp": (warp, near, range)} -- the node hands out the per-ray distortion loss of
    # its weights as a second output; the trainer adds {"sum": fp64 [1] accumulator, "scale": constant upstream gradient}
    dist: Optional[dict] = None

    def split(self, params: Sequence[torch.Tensor]) -> Tuple[List[torch.Tensor], List[torch.Tensor], List[torch.Tensor]]:
        k = self.n_planes + self.n_sigma
        return list(params[:self.n_planes]), [p.contiguous() for p in params[self.n_planes:k]], [p.contiguous() for p in params[k:]]


# eligibility rules of the paired and fused launch forms, each written once
def _heads64(sig_p: Sequence[torch.Tensor], rgb_p: Sequence[torch.Tensor]) -> bool:
    """both heads 64 wide: the width of every paired head launch"""
    return sig_p[0].size(0) == 64 and rgb_p[0].size(0) == 64


def _planes_3x32(kdesc: L.KPlanesDesc, keep: Sequence[torch.Tensor]) -> bool:
    """the plane set the fused gather and scatter take: 3 scales x 32 channels, all nine planes present"""
    return kdesc.n_scales == 3 and kdesc.channels == 32 and len(keep) == 9


def _stack_pair_bwd(F: int, sig_p: Sequence[torch.Tensor], rgb_p: Sequence[torch.Tensor]) -> bool:
    """behind a wide stack: both heads' backward in one tn_mlp_bwd_pair"""
    return F % 64 == 0 and len(sig_p) // 2 == 2 and len(rgb_p) // 2 == 5 and _heads64(sig_p, rgb_p)


class _KpFwd(enum.Enum):
    INFER_PAIR = "gather + both heads of every sample in one launch, nothing stashed (tn_kplanes_mlp_fwd_pair)"
    INFER_GATHER_SIGMA = "gather + sigma head in one launch (tn_kplanes_mlp_fwd), the colour head gated by the weights"
    INFER_PLAIN = "tn_kplanes_fwd, the sigma head, the colour head gated by the weights"
    TRAIN_GATHER_PAIR = "gather + both heads in one launch, stashed (tn_kplanes_mlp_fwd_pair)"
    TRAIN_PAIR = "tn_kplanes_fwd, then both heads in one launch (tn_mlp_fwd_stash_pair)"
    TRAIN_STASH = "tn_kplanes_fwd, then each head on its own, stashed where it has a workspace"


class _KpBwd(enum.Enum):
    SCATTER_CHAIN = "tn_kplanes_mlp_bwd_pair: data gradients + plane scatter, [planes_ready], then the weight gradients"
    PAIR_SPLIT = "tn_mlp_bwd_pair data gradients, tn_kplanes_bwd, planes_ready, tn_mlp_bwd_pair weight gradients"
    PAIR = "tn_mlp_bwd_pair, then tn_kplanes_bwd"
    SEPARATE = "one tn_mlp_bwd per head, then tn_kplanes_bwd"


@dataclass(frozen=True)
class _KPlanesPlan:
    fwd: _KpFwd
    bwd: Optional[_KpBwd]       # None: inference
    lean: bool                  # TN_MLP_LEAN on both heads: no hidden activations stashed, the weight-gradient launches rebuild them
    note_live: bool             # measure the live fraction for the next inference call's form
    covered: bool
    sb: int                     # workspace bytes of the sigma and the colour head (0: none)
    rb: int

    @property
    def rays_fwd(self) -> bool:
        """both heads are done before the weights: weights and composite as one launch per ray (tn_render_rays_fwd)"""
        return self.fwd in (_KpFwd.INFER_PAIR, _KpFwd.TRAIN_GATHER_PAIR, _KpFwd.TRAIN_PAIR)

    @property
    def flags(self) -> int:
        return L.MLP_LEAN if self.lean else 0


def _plan_kplanes(kdesc, keep, rdesc, sdesc, sig_p, rgb_p, train: bool, sb: int, rb: int, covered: bool, planes_ready: bool,
                  stats: Optional[dict]) -> _KPlanesPlan:
    F = kdesc.n_scales * kdesc.channels
    planes = _planes_3x32(kdesc, keep)
    pair_fwd = bool(sb and rb) and F % 4 == 0 and _heads64(sig_p, rgb_p)
    pair_bwd = bool(sb and rb) and F % 32 == 0 and len(sig_p) // 2 == 2 and _heads64(sig_p, rgb_p)
    # TN_MLP_LEAN: only the paired backward rebuilds the hidden activations (csrc/mlp_wgrad_rc.hip)
    lean = pair_fwd and pair_bwd and KP_LEAN and bool(L.lib().tn_mlp_lean_supported(C.byref(rdesc), C.byref(sdesc)))
    gather_sigma = not train and FUSE_GATHER and F % 4 == 0 and sig_p[0].size(0) == 64 and planes
    bwd = None
    if train:
        fwd = _KpFwd.TRAIN_GATHER_PAIR if pair_fwd and FUSE_GATHER and planes else _KpFwd.TRAIN_PAIR if pair_fwd else _KpFwd.TRAIN_STASH
        if not pair_bwd:
            bwd = _KpBwd.SEPARATE
        elif FUSE_SCATTER and planes:
            bwd = _KpBwd.SCATTER_CHAIN
        else:       # N > 1: the plane gradients go on the wire between the data and the weight gradients
            bwd = _KpBwd.PAIR_SPLIT if planes_ready else _KpBwd.PAIR
    # inference, two forms with identical results (a sample with w == 0 contributes exactly 0 either way, core.py:243-249):
    #   gated: gather + sigma head -> weights -> colour head on the 32-sample tiles that hold a weight -> composite;
    #   pair:  gather + BOTH heads of every sample in one launch (no feature rows, nothing stashed) -> weights + composite.
    # The pair wins while most tiles are alive (an untrained or half-trained field: 0.6 against 0.9 ms per 2^20 samples), the
    # gated form once early termination has emptied most of them; the choice follows the live fraction of the previous call
    elif gather_sigma and INFER_PAIR and rgb_p[0].size(0) == 64 and len(rgb_p) == 10 and _infer_prefers_pair(stats):
        fwd = _KpFwd.INFER_PAIR
    else:
        fwd = _KpFwd.INFER_GATHER_SIGMA if gather_sigma else _KpFwd.INFER_PLAIN
    return _KPlanesPlan(fwd, bwd, lean, gather_sigma and INFER_PAIR and stats is not None, covered, sb, rb)


@dataclass(frozen=True)
class _HeadsPlan:
    rows_fwd: bool              # the heads' forwards read x from the wide stack's workspace rows (f16x2 heads) ...
    x_from_rows: bool           # ... and only there: the stack wrote no row-major copy (TN_MLP_ROWS_ONLY)
    pair_bwd: bool              # both heads' backward in one tn_mlp_bwd_pair
    covered: bool
    sb: int
    rb: int


def _plan_heads(F: int, sig_p, rgb_p, train: bool, link: Optional[dict], sb: int, rb: int, covered: bool) -> _HeadsPlan:
    if train and not (sb and rb):
        raise RuntimeError("tinynerf_amd: these decoder shapes are outside the fused render node (use renderer.fused = False)")
    # f16x2 heads read their first-layer operands from the stack's row view (128-byte rows instead of 16 bytes per lane and
    # sample); once a forward has done so the stack stops writing the row-major feat (TN_MLP_ROWS_ONLY / TN_MLP_X_FROM_ROWS)
    rows_fwd = link is not None and MATMUL_F16X2()
    pair_bwd = link is not None and HEADS_PAIR_BACKWARD and _stack_pair_bwd(F, sig_p, rgb_p)
    return _HeadsPlan(rows_fwd, rows_fwd and bool(link.get("rows_only")), pair_bwd, covered, sb, rb)


def _head_descs(sig_p, rgb_p, F: int, n_freqs: int, freqs, ray_ids, table, rflags: int = 0, sflags: int = 0) -> Tuple[L.MlpDesc, L.MlpDesc]:
    """the colour and the sigma head.  The colour head's input is cat[PE(d), d, x] (models.py:87): PE(d) from the per-ray table
    through the ray id of every sample where there is one (TN_ENC_AUX_CAT), otherwise evaluated per sample (TN_ENC_DIR_CAT)"""
    enc, stride = (L.ENC_AUX_CAT, table.size(1)) if ray_ids is not None else (L.ENC_DIR_CAT, 0)
    rdesc = _mlp_desc(rgb_p, F, enc, n_freqs, L.ACT_SIGMOID, freqs, rflags, ray_ids, stride)
    sdesc = _mlp_desc(sig_p, F, L.ENC_NONE, 0, L.ACT_EXP_M1, None, sflags)
    return rdesc, sdesc


def _head_fwd(dev: torch.device, desc: L.MlpDesc, x, aux, n: int, y, ws, nbytes: int, gate: Optional[torch.Tensor] = None) -> None:
    """one head's forward: stashed for the backward where it has a workspace; otherwise only on the 32-sample tiles where
    `gate` (the weights) is not 0 (core.py:246-251)"""
    if ws is not None:
        L.call("tn_mlp_fwd_stash", dev, C.byref(desc), L.ptr(x), L.ptr(aux), C.c_int64(n), L.ptr(y), L.ptr(ws), C.c_int64(nbytes))
        return
    desc.row_gate = None if gate is None else gate.data_ptr()
    L.call("tn_mlp_fwd", dev, C.byref(desc), L.ptr(x), L.ptr(aux), C.c_int64(n), L.ptr(y), C.c_void_p(None))
    desc.row_gate = None


def _composite(ctx: Any, a: _Call, covered: bool, dev: torch.device, sigma, steps, rgbs, info, bg, colour: Optional[Callable], rays: bool):
    """weights scan and composite behind the sigma head, -> (out, weights).  `rays`: `colour(weights)` if given, then weights and
    composite as one launch per ray (tn_render_rays_fwd, bit-identical to the two); otherwise weights -> colour(weights) -> composite"""
    n, R = sigma.size(0), info.size(0)
    weights = _alloc(a.arena, "weights", (n,), dev)
    if not covered:
        weights.zero_()          # cuda.cu:84 (zeros_like): samples outside every (start, count) keep weight 0
    # harness: a zeroed [1] slot that the weights kernel raises when any weight is > 0 (instead of a reduction launch), and an
    # upstream gradient that arrives gated (tn_mse_grad_gated) -- see the "Empty iteration" note below
    gate_slot = _gate_slot(a.hint, covered and a.train)
    out = torch.empty((R, 3), device=dev)
    if rays:
        if colour is not None:
            colour(weights)
        L.call("tn_render_rays_fwd", dev, L.ptr(sigma), L.ptr(steps), L.ptr(rgbs), L.ptr(info), L.ptr(bg), C.c_float(a.thr), L.ptr(weights),
               L.ptr(out), L.ptr(gate_slot), C.c_int64(n), C.c_int64(R))
    else:
        gate = (L.ptr(gate_slot),) if gate_slot is not None else ()
        L.call("tn_weights_fwd_gate" if gate else "tn_weights_fwd", dev, L.ptr(sigma), L.ptr(steps), L.ptr(info), C.c_float(a.thr),
               L.ptr(weights), *gate, C.c_int64(n), C.c_int64(R))
        colour(weights)
        L.call("tn_composite_fwd", dev, L.ptr(rgbs), L.ptr(weights), L.ptr(info), L.ptr(bg), L.ptr(out), C.c_void_p(None),
               C.c_int64(n), C.c_int64(R))
    # core.py:246-254: when EVERY sample is masked (w == 0 everywhere) the reference renders the background from constants
    # that carry no graph, i.e. no parameter receives a gradient from the image loss; here the upstream gradient is gated
    # (a [1] tensor kept outside save_for_backward: with N > 1 the trainer all-reduces it in place right after this forward
    # (run.Trainer.step_on_batch) -- the single-GPU step on the union of the ranks' rays is only "empty" when every
    # rank's is -- so the backward already reads the all-rank value)
    ctx.gate_in_slot, ctx.stats = gate_slot is not None, a.stats
    ctx.gate = gate_slot if gate_slot is not None else (weights.amax().reshape(1) if a.train else None)
    if a.stats is not None:
        a.stats["gate"] = ctx.gate
        a.stats["pre_gated"] = ctx.gate_in_slot        # the caller MAY hand in a gated gradient (and must then say so)
        a.stats["upstream_gated"] = False
        if a.stats.get("maps_handout") is not None:   # NerfRenderer.render_maps: the weights this forward composited with
            a.stats["maps_handout"]["weights"] = weights
    return out, weights


def _distortion(ctx: Any, a: _Call, dev: torch.device, weights, steps, info):
    """the node's second output (a.dist): per-ray distortion loss of the weights the composite used, one launch (tn_distortion_fwd)"""
    ctx.set_materialize_grads(False)          # an output the caller never uses sends None, not a tensor of zeros, to the backward
    R = info.size(0)
    loss = torch.empty(R, device=dev)
    warp, near, rng = a.dist["warp"]
    L.call("tn_distortion_fwd", dev, L.ptr(weights), L.ptr(a.dist["t"]), L.ptr(steps), L.ptr(info), C.c_int64(R), C.c_int32(warp),
           C.c_float(near), C.c_float(rng), L.ptr(loss), L.ptr(a.dist.get("sum")))
    return loss


def _grad_buffers(ctx: Any, params: Sequence[torch.Tensor]) -> Tuple[List[torch.Tensor], List[Optional[torch.Tensor]]]:
    """where the kernels write each parameter's gradient -- param.grad itself when the caller accumulates into it and it has the
    parameter's layout, a zeroed tensor otherwise -- and what the backward returns to autograd (None for the former)"""
    refs: Sequence[Optional[torch.Tensor]] = ctx.param_refs if ctx.param_refs is not None else [None] * len(params)
    in_place = [r is not None and r.is_leaf and r.grad is not None and r.grad.stride() == p.stride() for p, r in zip(params, refs)]
    bufs = [r.grad if ip else torch.zeros_like(p) for p, r, ip in zip(params, refs, in_place)]
    return bufs, [None if ip else g for g, ip in zip(bufs, in_place)]


def _grad_ptrs(g_sig: Sequence[torch.Tensor], g_rgb: Sequence[torch.Tensor]):
    """the heads' weight and bias gradient pointers, in the kernels' argument order (gw_r, gb_r, gw_s, gb_s)"""
    return tuple((C.c_void_p * len(gs))(*[g.data_ptr() for g in gs]) for gs in (g_rgb[0::2], g_rgb[1::2], g_sig[0::2], g_sig[1::2]))


def _heads_bwd(dev: torch.device, pair: bool, rdesc, sdesc, feat, table, g_rgbs, g_sigma, gw, g_feat, ws_r, rb: int, ws_s, sb: int):
    """both heads' backward: one tn_mlp_bwd_pair, or one tn_mlp_bwd per head"""
    n = C.c_int64(feat.size(0))
    if pair:
        L.call("tn_mlp_bwd_pair", dev, C.byref(rdesc), C.byref(sdesc), L.ptr(feat), L.ptr(table), L.ptr(g_rgbs), L.ptr(g_sigma), n, *gw,
               L.ptr(g_feat), L.ptr(ws_r), C.c_int64(rb), L.ptr(ws_s), C.c_int64(sb))
        return
    L.call("tn_mlp_bwd", dev, C.byref(rdesc), L.ptr(feat), L.ptr(table), L.ptr(g_rgbs), n, *gw[:2], L.ptr(g_feat), L.ptr(ws_r), C.c_int64(rb))
    L.call("tn_mlp_bwd", dev, C.byref(sdesc), L.ptr(feat), C.c_void_p(None), L.ptr(g_sigma), n, *gw[2:], L.ptr(g_feat), L.ptr(ws_s), C.c_int64(sb))


def _rays_bwd(ctx: Any, grad_out: Optional[torch.Tensor], sigma, steps, rgbs, info, bg, weights,
              grad_dist: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """composite -> (rgbs, weights) and weights -> sigma as one launch per ray (the weights' gradient needs only the composite's).
    With a distortion output in use its gradient w.r.t. the weights (tn_distortion_bwd) joins the composite's inside that launch
    (tn_render_rays_bwd_dw)."""
    if grad_out is None:                     # (only the distortion output was used)
        grad_out = torch.zeros((info.size(0), 3), device=sigma.device)
    g_out = grad_out.contiguous()
    # "Empty iteration": zero gradients, as on the module-by-module path.  Applied here unless the caller has DECLARED the upstream
    # gradient gated (run.Trainer.step_on_batch sets stats["upstream_gated"] around tn_mse_grad_gated): any other loss on a
    # trainer-built batch -- a test, a custom loop -- then still gets the reference's zero gradients in an all-masked step (core.py:251-254)
    if ctx.gate is not None and not (ctx.gate_in_slot and ctx.stats is not None and ctx.stats.get("upstream_gated")):
        g_out = g_out * (ctx.gate > 0).to(g_out.dtype)
    dev, n, R = sigma.device, sigma.size(0), info.size(0)
    g_rgbs = _alloc(ctx.call.arena, "g_rgbs", (n, 3), dev)
    g_sigma = _alloc(ctx.call.arena, "g_sigma", (n,), dev)
    if not ctx.plan.covered:     # samples no ray owns: zero gradient, not whatever the arena held (the kernel writes every
        g_rgbs.zero_(); g_sigma.zero_()      # sample a ray owns)
    dist = ctx.call.dist
    scale = dist.get("scale") if dist is not None else None       # the trainer's hand-written upstream gradient: a constant per ray
    if dist is None or (scale is None and grad_dist is None):
        L.call("tn_render_rays_bwd", dev, L.ptr(sigma), L.ptr(steps), L.ptr(rgbs), L.ptr(info), L.ptr(bg), L.ptr(weights),
               L.ptr(g_out), L.ptr(g_rgbs), L.ptr(g_sigma), C.c_int64(n), C.c_int64(R))
        return g_rgbs, g_sigma
    # (in an "Empty iteration" every w is 0 and so is d L / d w: no gate here)
    g_extra = _alloc(ctx.call.arena, "g_weights_dist", (n,), dev)
    if not ctx.plan.covered:
        g_extra.zero_()
    warp, near, rng = dist["warp"]
    g_dist = None if scale is not None else grad_dist.contiguous()
    L.call("tn_distortion_bwd", dev, L.ptr(weights), L.ptr(dist["t"]), L.ptr(steps), L.ptr(info), C.c_int64(R), C.c_int32(warp),
           C.c_float(near), C.c_float(rng), L.ptr(g_dist), C.c_float(1.0 if scale is None else scale), C.c_void_p(None), L.ptr(g_extra))
    L.call("tn_render_rays_bwd_dw", dev, L.ptr(sigma), L.ptr(steps), L.ptr(rgbs), L.ptr(info), L.ptr(bg), L.ptr(weights),
           L.ptr(g_out), L.ptr(g_extra), L.ptr(g_rgbs), L.ptr(g_sigma), C.c_int64(n), C.c_int64(R))
    return g_rgbs, g_sigma


class _RenderKPlanes(Function):
    @staticmethod
    def forward(ctx: Any, a: _Call, packed: torch.Tensor, info: torch.Tensor, bg: Optional[torch.Tensor], freqs: torch.Tensor,
                *params: torch.Tensor) -> torch.Tensor:  # type: ignore
        planes, sig_p, rgb_p = a.split(params)
        dev = L.require_cuda(packed, info, *sig_p, *rgb_p)
        n, R = packed.size(0), info.size(0)
        kdesc, keep = _kplanes_desc(planes)
        F = kdesc.n_scales * kdesc.channels
        feat = _alloc(a.arena, "feat", (n, F), dev)
        table, ray_ids, steps = _ray_aux(packed, info, freqs, a.n_freqs, a.arena, a.hint)
        rdesc, sdesc = _head_descs(sig_p, rgb_p, F, a.n_freqs, freqs, ray_ids, table)
        # training forward: activations go to the backward's workspace, nothing is recomputed
        ws_s, sb = _workspace(sdesc, n, dev, a.arena, "ws_sigma") if a.train else (None, 0)
        ws_r, rb = _workspace(rdesc, n, dev, a.arena, "ws_rgb") if a.train else (None, 0)
        ready = a.hint.get("planes_ready") if (a.hint is not None and a.accumulate) else None
        p = _plan_kplanes(kdesc, keep, rdesc, sdesc, sig_p, rgb_p, a.train, sb, rb, _covered(a.hint, packed, R), ready is not None,
                          a.stats)
        rdesc.flags, sdesc.flags = rdesc.flags | p.flags, sdesc.flags | p.flags
        sigma = _alloc(a.arena, "sigma", (n,), dev)
        rgbs = _alloc(a.arena, "rgbs", (n, 3), dev)
        kp = (C.byref(kdesc), L.ptr(packed), C.c_int64(7))
        if p.fwd in (_KpFwd.INFER_PAIR, _KpFwd.TRAIN_GATHER_PAIR):
            # the feature rows go from the texel lines to the MFMA operands
            L.call("tn_kplanes_mlp_fwd_pair", dev, *kp, C.byref(rdesc), C.byref(sdesc), L.ptr(table), C.c_int64(n), L.ptr(feat), L.ptr(rgbs),
                   L.ptr(sigma), L.ptr(ws_r), C.c_int64(rb), L.ptr(ws_s), C.c_int64(sb))
        elif p.fwd is _KpFwd.INFER_GATHER_SIGMA:
            L.call("tn_kplanes_mlp_fwd", dev, *kp, C.byref(sdesc), C.c_int64(n), L.ptr(feat), L.ptr(sigma))
        else:
            L.call("tn_kplanes_fwd", dev, *kp, C.c_int64(n), L.ptr(feat))
            if p.fwd is _KpFwd.TRAIN_PAIR:      # both heads in one launch: the feature rows are read from HBM once
                L.call("tn_mlp_fwd_stash_pair", dev, C.byref(rdesc), C.byref(sdesc), L.ptr(feat), L.ptr(table), C.c_int64(n), L.ptr(rgbs),
                       L.ptr(sigma), L.ptr(ws_r), C.c_int64(rb), L.ptr(ws_s), C.c_int64(sb))
            else:
                _head_fwd(dev, sdesc, feat, None, n, sigma, ws_s, sb)
        colour = None if p.rays_fwd else lambda w: _head_fwd(dev, rdesc, feat, table, n, rgbs, ws_r, rb, w)
        out, weights = _composite(ctx, a, p.covered, dev, sigma, steps, rgbs, info, bg, colour, rays=p.rays_fwd)
        if p.note_live:
            _note_live_fraction(a.stats, weights)
        ctx.save_for_backward(packed, info, bg, freqs, feat, sigma, steps, table, ray_ids, weights, rgbs, ws_s, ws_r, *params)
        ctx.call, ctx.plan, ctx.planes_ready = a, p, ready
        ctx.param_refs = params if a.accumulate else None
        if a.dist is not None:
            return out, _distortion(ctx, a, dev, weights, steps, info)
        return out

    @staticmethod
    def backward(ctx: Any, grad_out: torch.Tensor, grad_dist: Optional[torch.Tensor] = None):  # type: ignore
        packed, info, bg, freqs, feat, sigma, steps, table, ray_ids, weights, rgbs, ws_s, ws_r, *params = ctx.saved_tensors
        a, p = ctx.call, ctx.plan
        planes, sig_p, rgb_p = a.split(params)
        dev, n, F = packed.device, packed.size(0), feat.size(1)
        g_rgbs, g_sigma = _rays_bwd(ctx, grad_out, sigma, steps, rgbs, info, bg, weights, grad_dist)
        grads, returned = _grad_buffers(ctx, params)
        g_planes, k = grads[:a.n_planes], a.n_planes + a.n_sigma
        gw = _grad_ptrs(grads[a.n_planes:k], grads[k:])
        g_feat = _alloc(a.arena, "g_feat", (n, F), dev)
        kdesc, _ = _kplanes_desc(planes)
        gp = ((C.c_void_p * 3) * L.TN_KPLANES_MAX_SCALES)(*[tuple(_hwc(g).data_ptr() for g in g_planes[3 * s:3 * s + 3])
                                                              for s in range(kdesc.n_scales)])
        if p.bwd is _KpBwd.SEPARATE:          # g_feat += d sigma / d feat
            rflags, sflags = L.MLP_STASHED if ws_r is not None else 0, L.MLP_ACCUM_GRAD_X | (L.MLP_STASHED if ws_s is not None else 0)
        else:                                 # both heads in one data-gradient pass: d / d feat is written once as the sum of the two
            rflags = sflags = L.MLP_STASHED | p.flags
        rdesc, sdesc = _head_descs(sig_p, rgb_p, F, a.n_freqs, freqs, ray_ids, table, rflags, sflags)
        rb, sb = p.rb, p.sb
        if ws_r is None:                      # (a head whose forward had no workspace: SEPARATE only)
            ws_r, rb = _workspace(rdesc, n, dev, a.arena, "ws_rgb")
        if ws_s is None:
            ws_s, sb = _workspace(sdesc, n, dev, a.arena, "ws_sigma")
        base_flags = rdesc.flags              # (STASHED + the matrix-mode bit + LEAN: the phase bits are OR-ed in, nothing is dropped)
        # SCATTER_CHAIN and PAIR_SPLIT: two calls, data gradients (+ plane scatter) then weight gradients -- the same launches as one
        # call makes, but the plane gradients are final in between: with N > 1 their all-reduce starts there and travels under the
        # weight-gradient kernels, and each half can be timed on its own (bench.py)
        for phase in (0,) if p.bwd in (_KpBwd.SEPARATE, _KpBwd.PAIR) else (L.MLP_CHAIN_ONLY, L.MLP_WGRAD_ONLY):
            rdesc.flags = base_flags | phase
            if p.bwd is _KpBwd.SCATTER_CHAIN:       # d loss / d features stays in registers
                L.call("tn_kplanes_mlp_bwd_pair", dev, C.byref(kdesc), L.ptr(packed), C.c_int64(7), gp, C.byref(rdesc), C.byref(sdesc),
                       L.ptr(feat), L.ptr(table), L.ptr(g_rgbs), L.ptr(g_sigma), C.c_int64(n), *gw, C.c_void_p(None), L.ptr(ws_r),
                       C.c_int64(rb), L.ptr(ws_s), C.c_int64(sb))
            else:
                _heads_bwd(dev, p.bwd is not _KpBwd.SEPARATE, rdesc, sdesc, feat, table, g_rgbs, g_sigma, gw, g_feat, ws_r, rb, ws_s, sb)
                if phase != L.MLP_WGRAD_ONLY:
                    L.call("tn_kplanes_bwd", dev, C.byref(kdesc), L.ptr(packed), C.c_int64(7), C.c_int64(n), L.ptr(g_feat), gp)
            if phase == L.MLP_CHAIN_ONLY and ctx.planes_ready is not None:
                ctx.planes_ready(g_planes)
        return (None, None, None, None, None, *returned)


class _MergeLast(Function):
    """(W_c[:, x] W_last, b_c + W_c[:, x] b_last, W_s W_last, b_s + W_s b_last) and the chain rule back to the six original tensors: one
    small launch each way (merge.hip) -- the same five matmuls through torch and autograd were ~35 launches, 0.26 ms per step."""

    @staticmethod
    def forward(ctx: Any, accumulate: bool, pe: int, wc: torch.Tensor, bc: torch.Tensor, ws: torch.Tensor, bs: torch.Tensor,
                w_last: torch.Tensor, b_last: torch.Tensor):  # type: ignore
        dev = L.require_cuda(wc, bc, ws, bs, w_last, b_last)
        ps = [t.contiguous() for t in (wc, bc, ws, bs, w_last, b_last)]
        F = w_last.size(0)
        outs = [torch.empty_like(t) for t in ps[:4]]
        heads = (L.MergeHead * 2)()
        for k, col0 in ((0, pe), (1, 0)):
            heads[k].weight, heads[k].bias = ps[2 * k].data_ptr(), ps[2 * k + 1].data_ptr()
            heads[k].rows, heads[k].ld, heads[k].col0 = ps[2 * k].size(0), ps[2 * k].size(1), col0
            heads[k].out_weight, heads[k].out_bias = outs[2 * k].data_ptr(), outs[2 * k + 1].data_ptr()
        L.call("tn_linear_merge_fwd", dev, C.c_int32(2), heads, L.ptr(ps[4]), L.ptr(ps[5]), C.c_int32(F))
        ctx.save_for_backward(*ps)
        ctx.cfg = (accumulate, pe)
        ctx.refs = (wc, bc, ws, bs, w_last, b_last) if accumulate else None
        return tuple(outs)

    @staticmethod
    def backward(ctx: Any, g_wc: torch.Tensor, g_bc: torch.Tensor, g_ws: torch.Tensor, g_bs: torch.Tensor):  # type: ignore
        ps = ctx.saved_tensors
        accumulate, pe = ctx.cfg
        dev = ps[0].device
        gm = [g.contiguous() if g is not None else torch.zeros_like(p) for g, p in zip((g_wc, g_bc, g_ws, g_bs), ps[:4])]
        refs = ctx.refs if ctx.refs is not None else [None] * 6
        in_place = [r is not None and r.is_leaf and r.grad is not None and r.grad.is_contiguous() and r.grad.dtype == p.dtype
                    for r, p in zip(refs, ps)]
        grads = [r.grad if ip else torch.zeros_like(p) for r, p, ip in zip(refs, ps, in_place)]
        heads = (L.MergeHead * 2)()
        for k, col0 in ((0, pe), (1, 0)):
            heads[k].weight, heads[k].bias = ps[2 * k].data_ptr(), ps[2 * k + 1].data_ptr()
            heads[k].rows, heads[k].ld, heads[k].col0 = ps[2 * k].size(0), ps[2 * k].size(1), col0
            heads[k].out_weight, heads[k].out_bias = grads[2 * k].data_ptr(), grads[2 * k + 1].data_ptr()
            heads[k].grad_merged_weight, heads[k].grad_merged_bias = gm[2 * k].data_ptr(), gm[2 * k + 1].data_ptr()
        L.call("tn_linear_merge_bwd", dev, C.c_int32(2), heads, L.ptr(ps[4]), L.ptr(ps[5]), C.c_int32(ps[4].size(0)), L.ptr(grads[4]), L.ptr(grads[5]))
        return (None, None, *[None if ip else g for g, ip in zip(grads, in_place)])


class _RenderHeads(Function):
    """The part of NerfRenderer.forward behind the feature module (core.py:239-267) for ANY field with the Vanilla decoders
    (Vanilla NeRF, Cobafa): sigma head -> weights scan -> colour head -> composite as one autograd node; ``feat`` is an
    ordinary differentiable input, so the field's own backward (width-256 / 128 stacks, grid scatters) follows through
    autograd.  Replaces the module-by-module path's ``mask.any()`` host sync, boolean gather / index_copy pair and their
    autograd counterparts: every sample goes through the colour head in place -- samples with w == 0 contribute exactly 0 to
    the composite in both directions, as in the reference (core.py:243-249)."""

    @staticmethod
    def forward(ctx: Any, a: _Call, feat: torch.Tensor, packed: torch.Tensor, info: torch.Tensor, bg: Optional[torch.Tensor],
                freqs: torch.Tensor, *params: torch.Tensor) -> torch.Tensor:  # type: ignore
        _, sig_p, rgb_p = a.split(params)
        feat = feat.contiguous()
        # `a.link`: row views of the wide stack that produced `feat` (models._FusedMLP.forward, harness only): feat^T as
        # [feature][32-sample] rows in that stack's workspace and the slot where it takes d loss / d feat in the same layout
        link = a.link if (a.link and a.train and a.link.get("n") == feat.size(0) and a.link.get("y_ptr") == feat.data_ptr()
                          and a.link.get("width") == feat.size(1) and feat.size(1) in (128, 256)) else None
        if link is None and a.link and a.link.get("rows_only"):
            raise RuntimeError("tinynerf_amd: the feature stack left its output as workspace rows only (TN_MLP_ROWS_ONLY) but this render "
                               "node cannot read them")
        dev = L.require_cuda(feat, packed, info, *sig_p, *rgb_p)
        n, R, F = packed.size(0), info.size(0), feat.size(1)
        covered = _covered(a.hint, packed, R)
        if link is not None:
            # cat[PE(d), d] (models.py:87) once per RAY as a table the kernels index through the ray id of every sample
            # (TN_ENC_AUX_CAT, as in the K-Planes node): the colour head then takes the plain-column first layer.  Its weight
            # gradient over a 256-wide x needs the row-operand kernel, hence only with row views
            table, ray_ids, steps = _ray_aux(packed, info, freqs, a.n_freqs, a.arena, a.hint)
        else:
            steps = a.hint["steps"] if covered else _alloc(a.arena, "steps", (n,), dev).copy_(packed[:, 6])
            table = _alloc(a.arena, "dirs", (n, 3), dev).copy_(packed[:, 3:6])
            ray_ids = None
        rdesc, sdesc = _head_descs(sig_p, rgb_p, F, a.n_freqs, freqs, ray_ids, table)
        ws_s, sb = _workspace(sdesc, n, dev, a.arena, "ws_sigma") if a.train else (None, 0)
        ws_r, rb = _workspace(rdesc, n, dev, a.arena, "ws_rgb") if a.train else (None, 0)
        p = _plan_heads(F, sig_p, rgb_p, a.train, link, sb, rb, covered)
        sigma = _alloc(a.arena, "sigma", (n,), dev)
        rgbs = _alloc(a.arena, "rgbs", (n, 3), dev)
        if p.rows_fwd:
            for d in (rdesc, sdesc):
                d.x_rows, d.x_rows_tile_stride = link["y_rows"], link["stride"]
                d.flags |= L.MLP_X_FROM_ROWS if p.x_from_rows else 0
        _head_fwd(dev, sdesc, feat, None, n, sigma, ws_s, sb)
        # training: the colour head runs on every sample, weights and composite of a ray behind it in one launch
        out, weights = _composite(ctx, a, covered, dev, sigma, steps, rgbs, info, bg,
                                  lambda w: _head_fwd(dev, rdesc, feat, table, n, rgbs, ws_r, rb, w), rays=a.train)
        ctx.save_for_backward(feat, info, bg, freqs, sigma, steps, table, ray_ids, weights, rgbs, ws_s, ws_r, *params)
        ctx.call, ctx.plan, ctx.link = a, p, link
        ctx.param_refs = params if a.accumulate else None
        if a.dist is not None:
            return out, _distortion(ctx, a, dev, weights, steps, info)
        return out

    @staticmethod
    def backward(ctx: Any, grad_out: torch.Tensor, grad_dist: Optional[torch.Tensor] = None):  # type: ignore
        feat, info, bg, freqs, sigma, steps, table, ray_ids, weights, rgbs, ws_s, ws_r, *params = ctx.saved_tensors
        a, p, link = ctx.call, ctx.plan, ctx.link
        _, sig_p, rgb_p = a.split(params)
        dev, (n, F) = feat.device, feat.shape
        g_rgbs, g_sigma = _rays_bwd(ctx, grad_out, sigma, steps, rgbs, info, bg, weights, grad_dist)
        grads, returned = _grad_buffers(ctx, params)
        gw = _grad_ptrs(grads[:a.n_sigma], grads[a.n_sigma:])
        # with row views the heads write d loss / d feat straight into the feature stack's workspace (rows) and read feat^T from
        # there for their first layers' weight gradients; autograd gets a placeholder of the right shape (no memory behind it)
        g_feat = _empty_rows(n, F, dev) if link is None else None      # handed to autograd (the field's backward): not an arena view
        rdesc, sdesc = _head_descs(sig_p, rgb_p, F, a.n_freqs, freqs, ray_ids, table, L.MLP_STASHED,
                                   L.MLP_STASHED | (0 if p.pair_bwd else L.MLP_ACCUM_GRAD_X))      # unpaired: g_feat += d sigma / d feat
        if link is not None:
            for d in (rdesc, sdesc):
                d.x_rows, d.grad_x_rows = link["y_rows"], link["grad_rows"]
                d.x_rows_tile_stride = d.grad_x_rows_tile_stride = link["stride"]
                if link.get("skipped_last"):     # x is the producer's last HIDDEN activation: d / d (its pre-activation) = relu' * ...
                    d.grad_x_mask_rows, d.grad_x_mask_tile_stride = link["mask_rows"], link["stride"]
        # pair: both heads' first layers' x-column weight gradients share a launch (and the x rows), and behind the 128-wide stack
        # d loss / d feat is written once as the sum of the two data gradients (mlp_bwd2.hip, bwd_pair_common)
        _heads_bwd(dev, p.pair_bwd, rdesc, sdesc, feat, table, g_rgbs, g_sigma, gw, g_feat, ws_r, p.rb, ws_s, p.sb)
        if link is not None:
            link["delivered"] = True
            g_feat = torch.empty(1, device=dev).expand(n, F)
        return (None, g_feat, None, None, None, None, *returned)


def _mergeable(producer, sig_p, rgb_p) -> bool:
    """the producer stack's last layer is a square Linear without activation feeding nothing but the two heads' first layers"""
    ps = producer.params()
    if len(ps) < 6 or ps[-2].dim() != 2 or ps[-2].size(0) != ps[-2].size(1) or ps[-2].size(0) not in (128, 256):
        return False
    F = ps[-2].size(0)
    if not (sig_p[0].size(1) == F and rgb_p[0].size(1) > F and all(p.requires_grad for p in (ps[-2], ps[-1], sig_p[0], sig_p[1], rgb_p[0], rgb_p[1]))):
        return False
    # ... and the kernel side can actually stop this stack at its last hidden activation (slab-eligible f16x2 stack: positional encoding with
    # <= 64 slots or <= 64 plain inputs, out == H): asked of the library itself (host-only, no launch) with the descriptor of the
    # stack's previous forward -- shapes alone would arm TN_MLP_SKIP_LAST for stacks that then fail with TN_E_CONFIG mid-step
    sc = producer.__dict__.get("scratch")
    cfg = sc[4].get("last_cfg") if sc is not None and len(sc) > 4 else None
    if cfg is None:
        return False
    in_dim, encoding, n_freqs, out_act = cfg
    desc = _mlp_desc([p.contiguous() for p in ps], in_dim, encoding, n_freqs, out_act, None, flags=L.MLP_SKIP_LAST | L.MLP_ROWS_ONLY)
    a, b, c, d = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
    return L.lib().tn_mlp_rows_view_hidden(C.byref(desc), C.c_int64(32), C.byref(a), C.byref(b), C.byref(c), C.byref(d)) == 0


def _vanilla_decoders(renderer) -> bool:
    from .models import VanillaColorDecoder, VanillaOpacityDecoder
    sd, cd = renderer.sigma_decoder, renderer.rgb_decoder
    return type(sd) is VanillaOpacityDecoder and type(cd) is VanillaColorDecoder and sd.net.net[0].out_features == 64 and \
        cd.net.net[0].out_features == 64 and len(cd.net.params()) == 10 and sd.net.net[0].in_features % 4 == 0


def supports(renderer) -> bool:
    """K-Planes field (whole render as one node, gather / scatter inside the MLP launches) or any other field in front of the
    Vanilla decoders of run.py:133-134,138-139,149-150 (heads + scan + composite as one node)."""
    from .models import KPlanesFeatureField
    fm = renderer.feature_module
    if not _vanilla_decoders(renderer):
        return False
    if isinstance(fm, KPlanesFeatureField):
        return fm.dropout.p == 0.0
    return True


def render(renderer, packed: torch.Tensor, info: torch.Tensor, thr: float, accumulate_into_grad: bool = False, dist: Optional[dict] = None):
    """Fused forward of ``renderer`` on packed samples (see supports()).  ``dist`` (NerfRenderer.render_with_distortion): t and the
    warp -- the result is then (rgb, per-ray distortion loss)."""
    from .models import KPlanesFeatureField
    fm, sd, cd = renderer.feature_module, renderer.sigma_decoder, renderer.rgb_decoder
    sig_p, rgb_p = sd.net.params(), cd.net.params()
    bg = renderer._bg(packed.device)
    arena = None
    if getattr(renderer, "reuse_buffers", False):
        arena = renderer.__dict__.setdefault("_arena", Arena())
    hint, stats = getattr(renderer, "_batch_aux", None), renderer.__dict__.setdefault("_stats", {})
    if dist is not None:
        train_side = stats.get("dist_train")       # the trainer's accumulator slot and constant upstream gradient
        if train_side is not None:
            dist = {**dist, **train_side}
            train_side["taken"] = True
    if isinstance(fm, KPlanesFeatureField):
        planes = fm.plane_tensors()
        train = torch.is_grad_enabled() and any(p.requires_grad for p in (*planes, *sig_p, *rgb_p))
        a = _Call(float(thr), cd.n_freqs, len(planes), len(sig_p), accumulate_into_grad, arena, train, hint, stats, dist=dist)
        return _RenderKPlanes.apply(a, packed.contiguous(), info.contiguous(), bg, cd.pe.freqs, *planes, *sig_p, *rgb_p)
    # harness: the stack whose row view this node matched last time may leave its output as rows only (TN_MLP_ROWS_ONLY) -- armed for
    # exactly this forward; _RenderHeads fails loudly if it then cannot read the rows
    producer = renderer.__dict__.get("_rows_producer")
    armed = None
    if producer is not None and arena is not None and torch.is_grad_enabled() and MATMUL_F16X2():
        sc = producer.__dict__.get("scratch")
        if sc is not None and len(sc) > 4:
            sc[4]["rows_only"] = True
            armed = sc[4]
            if MERGE_LAST and _mergeable(producer, sig_p, rgb_p):
                sc[4]["skip_last"] = True
    try:
        feat = fm(packed[:, :3])
    finally:
        # the flag is for exactly THIS forward: if the producer stack did not run (an exception, a feature module that skipped it) it must
        # not stay armed for an unrelated forward, whose row-major output would then silently stay unwritten
        if armed is not None:
            armed.pop("skip_last", None)
        if armed is not None and armed.pop("rows_only", False):
            import warnings
            warnings.warn("tinynerf_amd.fused: TN_MLP_ROWS_ONLY was armed but the feature stack did not consume it; disarmed", RuntimeWarning)
    train = torch.is_grad_enabled() and (feat.requires_grad or any(p.requires_grad for p in (*sig_p, *rgb_p)))
    link = None
    if train and arena is not None:          # harness: the stack that produced `feat` may offer row views of its workspace
        from .models import MLP
        for mod in fm.modules():
            sc = mod.__dict__.get("scratch") if isinstance(mod, MLP) else None
            if sc is not None and len(sc) > 2 and sc[2].get("y_ptr") == feat.data_ptr():
                link = sc[2]
                if feat.size(1) in (128, 256) and sc[2].get("n") == feat.size(0):
                    renderer.__dict__["_rows_producer"] = mod
    if link is not None and link.get("skipped_last"):
        # the stack stopped at its last hidden activation h (rows): heads on h with the last layer folded into their first layers
        w_last, b_last = producer.params()[-2:]
        pe = rgb_p[0].size(1) - feat.size(1)                        # torch column order of the colour head: [PE(d), d, x] (models.py:87)
        wc, bc, ws_, bs_ = _MergeLast.apply(accumulate_into_grad, pe, rgb_p[0], rgb_p[1], sig_p[0], sig_p[1], w_last, b_last)
        rgb_p = [wc, bc, *rgb_p[2:]]
        sig_p = [ws_, bs_, *sig_p[2:]]
    a = _Call(float(thr), cd.n_freqs, 0, len(sig_p), accumulate_into_grad, arena, train, hint, stats, link, dist)
    return _RenderHeads.apply(a, feat, packed.contiguous(), info.contiguous(), bg, cd.pe.freqs, *sig_p, *rgb_p)
