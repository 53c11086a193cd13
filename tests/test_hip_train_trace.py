"""G22 on the GPU: the HIP harness against the record of the reference's OWN ``train()`` (oracle/make_train_trace.py ran
``src.run.train`` on the reference's hotdog fixture with regenerable random streams; tests/test_oracle_train_trace.py holds the CPU
port to the same record, bit for bit).

The test body is the reference's loop (run.py:205-261) with the HIP objects in place of the reference's: loader batches walked as
``DataLoader(shuffle=True)`` walks a permutation (partial last batch, fresh permutation per epoch), ``RayProvider`` per loader batch
with the recorded jitter stream, the projection rule, ``Trainer.step_on_batch`` for everything behind the batch (refresh, render,
loss, TV, scaled-never-unscaled backward, Adam, MultiStepLR).  Nothing of the reference is needed at run time: the golden carries
what it did."""
import numpy as np
import pytest
import torch

import _g22
import _trace_noise
from conftest import load_golden
from oracle import tinynerf_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _loader(M, B, seed):
    """run.py:116-122,221-225 with the trace's permutation stream (oracle/make_train_trace.py LoaderRec)"""
    gen = torch.Generator().manual_seed(seed * 1000003 + 1)
    while True:
        perm = torch.randperm(M, generator=gen, dtype=torch.int32).to(torch.int64)
        for b0 in range(0, M, B):
            yield perm[b0:b0 + B]


def _run(name, n_steps=None, perturb=0):
    from tinynerf_amd.run import TrainConfig, Trainer, jitter_seed
    g = _g22.trace(name)
    o, d, rgbs, bg = _g22.ray_table()
    method, seed, B, S = str(g["method"]), int(g["seed"]), int(g["batch_size"]), int(g["n_samples"])
    K = int(g["steps"]) if n_steps is None else n_steps
    dev = torch.device(DEV)
    o_t, d_t, rgb_t = (torch.from_numpy(a).to(dev) for a in (o, d, rgbs))
    cfg = TrainConfig(method=method, scene_type="aabb", batch_size=B, n_samples=S, seed=seed)
    tr = Trainer(cfg, o_t, d_t, rgb_t, torch.from_numpy(bg).to(dev), dev)
    assert tr.steps == int(g["total_steps"])
    if perturb:                          # the control runs: every parameter moved by a few ulps (see _check)
        gen = torch.Generator(device=dev).manual_seed(perturb)
        with torch.no_grad():
            for p in tr.renderer.parameters():
                p.mul_(1.0 + 2.0 ** -22 * (torch.rand(p.shape, device=dev, generator=gen) - 0.5))
    stream = _loader(o.shape[0], B, seed)
    target_size = B * S
    ladder = _g22.decay_ladder()
    losses, lrs, counts, flips, occ = [], [], [], [], []
    for step in range(K):
        refresh = step % tr.occupancy_grid_updates == 0
        # ---- run.py:215-244, literally ----
        current_size, projected_size, tmp_count = 0, 0, 0
        acc_info, acc_samples, acc_rgbs = [], [], []
        while projected_size < target_size:
            idx = next(stream).to(dev)
            r0 = tmp_count * B
            ctr = np.arange(r0, r0 + idx.numel(), dtype=np.uint64)[:, None] * np.uint64(S) + np.arange(S, dtype=np.uint64)[None, :]
            jit = torch.from_numpy(orc.uniform01(jitter_seed(seed, step), ctr)).to(dev)          # the trace's stand-in for core.py:173
            samples, info = tr.ray_provider(o_t[idx], d_t[idx], training=True, jitter=jit)
            info = info.clone()
            info[:, 0] += current_size
            acc_info.append(info); acc_samples.append(samples); acc_rgbs.append(rgb_t[idx])
            current_size += samples.size(0)
            tmp_count += 1
            projected_size = int(current_size * (1 + 1 / tmp_count))
        packed, target, info = torch.cat(acc_samples, 0), torch.cat(acc_rgbs, 0), torch.cat(acc_info, 0)
        counts.append((packed.size(0), info.size(0), tmp_count))
        tr.renderer._batch_aux = None            # (a hand-built batch: the fused node derives ray ids / steps itself)
        tr.step_on_batch(packed, info, target, tmp_count, prefetch=False)
        losses.append(tr.loss_value())
        lrs.append(float(tr.optimizer.param_groups[0]["lr"]))
        occ.append(tr.occupancy_grid.occupancy())
        if refresh:
            i = int(np.nonzero(g["grid_steps"] == step)[0][0])
            got = tr.occupancy_grid.grid.cpu().numpy()
            flips.append(float((got != ladder[g["grid_decays"][i]]).mean()))
            if not perturb:              # (a control run may have left the record's trajectory by now; a flipped cell moves the mean by < 1 / cells)
                assert abs(tr.occupancy_grid.mean - g["grid_means"][i]) <= flips[-1] + 1e-6
    return g, K, tr, np.array(losses), lrs, counts, flips, occ


def _check(name, n_exact, flip_bound=2e-3):
    """Tolerances by construction.  Adam at lr 1e-2 with eps 1e-15 turns rounding-level differences of a gradient into lr-sized
    differences of a parameter wherever |g| is itself rounding noise, and the recipe is run at the edge of stability (the reference's
    own Vanilla trace has loss spikes at steps 1 and 11): any two fp32 evaluations of the trajectory part ways at a rate that depends
    on the method and the step.  That rate is MEASURED, twice.  Here: three control runs of the same HIP trainer whose initial
    parameters are moved by +- 2^-23 relative (what a different summation order does to one gradient) give, per step, how far fp32
    trajectories of this recipe are apart from each other; the HIP trainer may be 8 x that far from the reference's record (the envelope
    is cumulative: once trajectories have parted they do not rejoin), and never less than 1e-5 -- the north-star figure -- is asked.
    And on the reference's side, by arithmetic that is not under test: oracle/make_trace_noise.py perturbs the CPU port -- which replays
    the same record to 1e-6 -- by the same rule, six controls per trace (golden G23), and the HIP controls' own envelope and spreads
    must stay under M x the port's (tests/_trace_noise.py: M = 2 x the measured fluctuation of a three-control envelope, nothing of it
    taken from the GPU).  A HIP trainer that became more sensitive to rounding can therefore no longer widen its own allowance.
    Batch structure, learning rates and refresh steps are compared exactly."""
    g, K, tr, losses, lrs, counts, flips, occ = _run(name)
    ref = g["loss"][:K]
    # batch structure: bit-exact sampler + rule on the same rays / jitter, for as long as the occupancy grids agree cell for cell
    # (a cell whose alpha sits within rounding of the threshold may flip: then a handful of samples differ)
    np.testing.assert_array_equal([c[0] for c in counts[:n_exact]], g["n_samples_per_step"][:n_exact])
    np.testing.assert_array_equal([c[1] for c in counts], g["n_rays_per_step"][:K])          # rays and loader batches: always
    np.testing.assert_array_equal([c[2] for c in counts], g["loader_batches_per_step"][:K])
    assert np.abs(np.array([c[0] for c in counts]) / g["n_samples_per_step"][:K] - 1).max() < 2e-3
    np.testing.assert_array_equal(lrs, g["lr_after_step"][:K])                               # run.py:188-199
    assert max(flips) <= flip_bound, flips
    np.testing.assert_allclose(occ, g["occupancy"][:K], atol=2e-3)
    np.testing.assert_allclose(losses[0], ref[0], rtol=1e-5)
    sd = {k: v.detach().cpu().contiguous().numpy() for k, v in tr.renderer.state_dict().items()}
    envelope = np.zeros(K)
    spread = {}
    for seed in (1, 2, 3):
        _, _, tr_c, losses_c, _, _, _, _ = _run(name, perturb=seed)
        envelope = np.maximum(envelope, np.maximum.accumulate(np.abs(losses_c / losses - 1)))
        for k, v in tr_c.renderer.state_dict().items():
            d = float(np.abs(v.detach().cpu().contiguous().numpy() - sd[k]).max() / max(float(np.abs(sd[k]).max()), 1e-30))
            spread[k] = max(spread.get(k, 0.0), d)
        del tr_c
    # (the ONSET of the divergence is itself random -- one control may leave a step before the record's run does: the envelope is read one
    #  step ahead)
    envelope_ahead = np.append(envelope[1:], envelope[-1])
    tol = np.maximum(1e-5, 8.0 * envelope_ahead)
    np.set_printoptions(linewidth=200, precision=2)
    # that allowance is capped from the reference's side: the port's controls under the same perturbation (golden G23)
    noise = _trace_noise.load(name, load_golden("G23_trace_noise"))
    assert [str(n) for n in noise["param_names"]] == [str(n) for n in g["param_names"]] and noise["E6"].shape[0] >= K
    _trace_noise.check_controls(name, envelope_ahead, spread, g["param_names"], noise)
    rel = np.abs(losses / ref - 1)
    print(name, "loss: |HIP / reference - 1| per step", rel)
    print(name, "loss: allowed (8 x the control runs' distance, cumulative, read one step ahead)", tol, "flips", flips)
    assert (rel <= tol).all(), (rel, tol)
    assert tol[:3].max() < 1e-3                                  # the controls themselves start together
    worst = {}
    for n in g["param_names"]:
        n = str(n)
        worst.update(_g22.compare_final_state({**g, "param_names": np.array([n])}, sd, max(1e-5, 8.0 * spread[n]), "tinynerf_amd.run.Trainer"))
    print(name, "parameters after", K, "steps: largest (difference / largest value) =", max(worst.values()), "allowed there",
          max(1e-5, 8.0 * spread[max(worst, key=worst.get)]))


def test_hip_trainer_follows_the_reference_train_loop_kplanes():
    _check("kplanes", n_exact=21)


def test_hip_trainer_follows_the_reference_train_loop_vanilla(matmul):
    _check("vanilla", n_exact=21)


def test_hip_trainer_follows_the_reference_across_refreshes_and_an_lr_milestone():
    """B = 65536: 128 recipe steps, a refresh EVERY step (run.py:103: int(16 * 4096 / B) = 1) -- the first cells cross the threshold
    after 16 of them -- and the first MultiStepLR milestone at step 64 (run.py:188-199)"""
    _check("kplanes_lr", n_exact=16)
