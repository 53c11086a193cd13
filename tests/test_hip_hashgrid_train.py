"""method="hashgrid" trains: 200 steps on the rays of golden G22 against the same run with method="kplanes" (unchanged code, the
measure): the hash grid's mean training MSE over the last 20 steps is finite and at most 2 x K-Planes' (a 3 dB margin: two different
fields do not converge at the same rate, while a wrong or missing table gradient leaves the loss near its starting value, which is 17 x
the gate: LABNOTES 9.7); the parameters round-trip through state_dict() into a fresh Trainer; infer returns a finite image."""
import numpy as np
import pytest
import torch

import _g22

pytestmark = pytest.mark.gpu
DEV = "cuda"
STEPS, TAIL = 200, 20


def run(method):
    from tinynerf_amd.run import TrainConfig, Trainer
    o, d, rgbs, bg = (torch.from_numpy(a).to(DEV) for a in _g22.ray_table())
    cfg = TrainConfig(method=method, batch_size=256, n_samples=64, seed=1)
    tr = Trainer(cfg, o, d, rgbs, bg, torch.device(DEV))
    mses = []
    for s in range(STEPS):
        tr.step()
        if s == 0 or s >= STEPS - TAIL:
            acc, inv, _, _ = tr._loss_parts                  # [0]: the step's sum of squared errors; inv = 1 / (3 rays)
            mses.append(float(acc[0].item()) * inv)
    return tr, cfg, mses[0], float(np.mean(mses[1:])), (o, d, rgbs, bg)


def test_hashgrid_trains_as_well_as_kplanes_within_3_db():
    from tinynerf_amd.models import HashGridFeatureField
    from tinynerf_amd.run import Trainer, infer
    tr, cfg, first, tail, (o, d, rgbs, bg) = run("hashgrid")
    _, _, kp_first, kp_tail, _ = run("kplanes")
    print(f"training MSE, first step -> mean of the last {TAIL} of {STEPS}: hashgrid {first:.5f} -> {tail:.5f}, kplanes {kp_first:.5f} -> {kp_tail:.5f}")
    assert isinstance(tr.renderer.feature_module, HashGridFeatureField) and tr.renderer.feature_module.table.shape[1] == 2
    assert np.isfinite(tail)
    assert tail <= 2.0 * kp_tail
    # state_dict round trip into a fresh Trainer
    sd = {k: v.detach().clone() for k, v in tr.renderer.state_dict().items()}
    assert "feature_module.table" in sd
    fresh = Trainer(cfg, o, d, rgbs, bg, torch.device(DEV))
    assert not torch.equal(fresh.renderer.feature_module.table, tr.renderer.feature_module.table)
    fresh.renderer.load_state_dict(sd)
    for k, v in fresh.renderer.state_dict().items():
        assert torch.equal(v, sd[k]), k
    H, W = 40, 50
    ds = [{"rays_o": o[:H * W].reshape(H, W, 3), "rays_d": d[:H * W].reshape(H, W, 3)}]
    img = infer(tr, ds, [0])[0]
    assert img.shape == (H, W, 3) and torch.isfinite(img).all()
