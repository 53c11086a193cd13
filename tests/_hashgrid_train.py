"""What the hash grid's training tests share (tests/test_hip_training.py, test_hip_refresh.py, test_hip_hashgrid.py): the small
configuration, its level plan from the yardstick, the scaled starting state, and the per-level view of the table's gradient.

``python tests/_hashgrid_train.py`` repeats, with the CPU port alone (no GPU), the runs behind the choices the GPU tests document:
the learning rate of the trajectory test, the designed state of the refresh test, and the sensitivity of the per-level comparison.
The starting state built here on the CPU is the trainer's own: run.Trainer constructs its modules from the CPU generator behind
``torch.manual_seed(cfg.seed)`` before it moves them to the device (the GPU tests assert the equality)."""
import os
import sys

import numpy as np
import torch

import _hashgrid_ref as hg

LOG2_T = 14
PLAN = hg.levels(16, LOG2_T, 16, 2048)                  # two dense levels, fourteen hashed ones, ~0.25 M entries
TABLE = "feature_module.table"
TABLE_SCALE = 1e4                                       # the recipe's U(+-1e-4) table -> U(+-1): features the heads can see
# The free-running test's seed.  The recipe's lr 1e-2 lets the density of most starting states die within a dozen steps (seeds 0, 2, 4,
# 5, 6, 8 of 0..9, in the port alone); such a run renders the background, and on the rows of the image that ARE background its loss is
# rounding noise squared (seed 5: 0, 4.6e-18, 0, 0 at steps 13..16), which no relative bound can hold.  Seeds 3, 7 and 9 keep every
# one of the 24 losses above 6e-4; 9 has the largest smallest loss (2.9e-3).
FREE_RUN_SEED = 9


def config(**kw):
    from tinynerf_amd.run import TrainConfig
    base = dict(method="hashgrid", hashgrid_log2_table_size=LOG2_T, scene_type="aabb", batch_size=256, n_samples=32, seed=5,
                occupancy_res=32, deterministic=True)
    base.update(kw)
    return TrainConfig(**base)


def scene():
    from tinynerf_amd import rays
    o, d, rgb, _, _ = rays.synthetic_scene(n_views=2, res=64, seed=3, device="cpu")
    return o.contiguous(), d.contiguous(), rgb.contiguous()


def scale_table(renderer):
    """in place, before the starting state is taken"""
    with torch.no_grad():
        renderer.feature_module.table.mul_(TABLE_SCALE)


def cpu_start_state(cfg):
    """the state dict run.Trainer(cfg, ...) starts from, with the scaled table, built without a device"""
    from tinynerf_amd.run import build_renderer
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(cfg.seed)
        renderer, _, _ = build_renderer(cfg, torch.ones(3), torch.device("cpu"))
    scale_table(renderer)
    return {k: v.detach().clone() for k, v in renderer.state_dict().items()}


def split_levels(grads, plan=PLAN):
    """{..., TABLE: [E, F]} -> the same dict with the table's entry replaced by one entry per level (views)"""
    out = {k: v for k, v in grads.items() if k != TABLE}
    _, _, entries, offsets = plan
    for l, (e, o) in enumerate(zip(entries, offsets)):
        out[f"{TABLE}.level{l:02d}"] = grads[TABLE][o:o + e]
    return out


def level_ratios(got, ref, rel, plan=PLAN):
    """per level: max |got - ref| / (rel * max |ref|)"""
    g, r = split_levels({TABLE: np.asarray(got, np.float64)}, plan), split_levels({TABLE: np.asarray(ref, np.float64)}, plan)
    return [float(np.abs(g[k] - r[k]).max() / (rel * max(float(np.abs(r[k]).max()), 1e-30))) for k in sorted(r)]


def port_grads(sd, packed, info, target, bg, grad_scale, plan=PLAN):
    """d (grad_scale * MSE) / d parameter through the port, table split by level"""
    from oracle import torch_port as tp
    pk, inf_, tg = (torch.from_numpy(np.asarray(a)) if not isinstance(a, torch.Tensor) else a for a in (packed, info, target))
    grads, loss = tp.grads_of(sd, lambda p: grad_scale * torch.nn.functional.mse_loss(tp.render(p, pk, inf_, bg, hashgrid=plan), tg))
    return (split_levels(grads, plan) if grads else grads), loss


def forward_conditioning(cur, packed, info, target, grad_scale):
    """How well the reference's fp32 weights FORWARD determines each gradient tensor, relative to its largest element: the port's
    gradients with w = T (1 - expf(-sigma delta)) as the reference forms it in fp32 against the same formula evaluated in float64.
    expf(-sigma delta) is an fp32 number next to 1, so 1 - expf carries an absolute error of 2^-24: where the density has died
    (sigma delta ~ 1e-6) the weights, and every gradient behind them, are only percent-level determined by ANY fp32 evaluation.
    (oracle/torch_port.weights_conditioning probes the backward's suffix sums only.)"""
    import unittest.mock as mock
    from oracle import torch_port as tp
    base, _ = port_grads(cur, packed, info, target, torch.ones(3), grad_scale)
    exact = lambda s, d, i, thr: tp.orc.weights_fwd_vectorised(s, d, i, thr).astype(np.float32)
    with mock.patch.object(tp.orc, "weights_fwd", exact):
        alt, _ = port_grads(cur, packed, info, target, torch.ones(3), grad_scale)
    return {k: float(np.abs(alt[k] - base[k]).max() / max(float(np.abs(base[k]).max()), 1e-30)) for k in base}


def _trajectory(lr, n_steps=8):
    """the port alone along the trajectory of test_gradients_along_the_reference_trajectory[hashgrid]"""
    from oracle import torch_port as tp
    cfg = config()
    o, d, rgb = scene()
    sd0 = cpu_start_state(cfg)
    rows = []

    def on_step(step, sd, packed, info, target):
        cur = {k: v.detach().clone() for k, v in sd.items()}
        grads, _ = port_grads(cur, packed, info, target, torch.ones(3), cfg.grad_scale)
        rows.append((step, packed.shape[0], info.shape[0], bool(grads),
                     [float(np.abs(grads[k]).max()) for k in sorted(grads) if k.startswith(TABLE)] if grads else [],
                     max(forward_conditioning(cur, packed, info, target, cfg.grad_scale).values()) if grads else 0.0))
        if step == 0:
            rows[-1] += (cur, packed, info, target)
    losses, _, _ = tp.reference_training(sd0, o.numpy(), d.numpy(), rgb.numpy(), method="hashgrid", batch_size=256, n_samples=32,
                                         n_steps=n_steps, occupancy_res=32, on_step=on_step, lr=lr, hashgrid=PLAN)
    return losses, rows


def _free_run(seed, n_steps=24):
    """the port alone on the run of test_hashgrid_training_matches_cpu_port"""
    from oracle import torch_port as tp
    cfg = config(seed=seed)
    o, d, rgb = scene()
    return tp.reference_training(cpu_start_state(cfg), o.numpy(), d.numpy(), rgb.numpy(), method="hashgrid", batch_size=256, n_samples=32,
                                 n_steps=n_steps, occupancy_res=32, hashgrid=PLAN)[0]


def _sensitivity(cur, packed, info, target):
    """scale one hashed level's slice of the table gradient by 1.01, and drop the last lane (sample) of every wave from one
    level's scatter: either must leave the 1e-4 allowance at that level and at no other"""
    grads, _ = port_grads(cur, packed, info, target, torch.ones(3), config().grad_scale)
    ref = np.concatenate([grads[k] for k in sorted(grads) if k.startswith(TABLE)])
    _, _, entries, offsets = PLAN
    level = 9
    a = ref.copy()
    a[offsets[level]:offsets[level] + entries[level]] *= 1.01
    print("sensitivity, level 9 scaled by 1.01: error / allowance per level =", [f"{r:.2g}" for r in level_ratios(a, ref, 1e-4)])
    from oracle import torch_port as tp
    leaf = {k: v for k, v in cur.items()}
    table = cur[TABLE].clone().requires_grad_(True)
    leaf[TABLE] = table
    pk, inf_, tg = torch.from_numpy(packed), torch.from_numpy(info), torch.from_numpy(target)
    feat = tp.hashgrid_features(leaf, pk[:, :3], PLAN)
    # d loss / d feat of the step, then the scatter with lane 63 of every wave left out at one level
    feat_leaf = feat.detach().clone().requires_grad_(True)
    import unittest.mock as mock
    with mock.patch.object(tp, "features", lambda *a_, **k_: feat_leaf):
        loss = config().grad_scale * torch.nn.functional.mse_loss(tp.render(leaf, pk, inf_, torch.ones(3), hashgrid=PLAN), tg)
    loss.backward()
    g = feat_leaf.grad.clone()
    g[63::64, 2 * level:2 * level + 2] = 0.0
    feat.backward(g)
    print("sensitivity, lane 63 dropped at level 9:  error / allowance per level =",
          [f"{r:.2g}" for r in level_ratios(table.grad.numpy(), ref, 1e-4)])


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    first = None
    for lr in (1e-2, 1e-3):
        losses, rows = _trajectory(lr)
        real = sum(1 for r in rows if r[3] and r[5] <= 2.5e-5)
        print(f"lr {lr:g}: {sum(1 for r in rows if r[3])} of {len(rows)} steps have a gradient at all, {real} one that the reference's fp32 "
              f"forward determines to a quarter of the 1e-4 rule; losses {[f'{v:.5f}' for v in losses]}")
        for r in rows:
            print(f"  step {r[0]}: {r[1]} samples, {r[2]} rays, forward conditioning {r[5]:.1e}, largest |table gradient| per level "
                  f"{[f'{v:.2g}' for v in r[4]]}")
        first = first or rows[0]
    _sensitivity(*first[6:])
    for seed in range(10) if "seeds" in sys.argv[1:] else (5, FREE_RUN_SEED):
        losses = _free_run(seed)
        print(f"free run, seed {seed}: smallest of 24 losses {min(losses):.3e}; {[f'{v:.1e}' for v in losses]}")
    if "refresh" in sys.argv[1:]:
        import test_hip_refresh
        test_hip_refresh.design_report("hashgrid")
