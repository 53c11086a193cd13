"""bench.py's --dump-outputs: what the last timed step computed, as .npy files of a bounded size, and --steps as the number of
timed steps."""
import importlib.util
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    bench.torch = torch
    return bench


def test_dump_outputs_of_the_headline_model(tmp_path):
    """the headline K-Planes model on the CPU behind a stand-in trainer: every parameter, loss, batch counts and the grid land as
    float32 / float64 .npy files under 64 MB; a plane larger than 2^20 entries is the documented seeded sample of its logical order"""
    from tinynerf_amd.run import TrainConfig, build_renderer
    bench = _bench()
    cfg = TrainConfig(method="kplanes", scene_type="aabb", batch_size=1024, n_samples=1024, seed=0)
    torch.manual_seed(0)
    renderer, grid, _ = build_renderer(cfg, torch.ones(3), torch.device("cpu"))
    tr = types.SimpleNamespace(renderer=renderer, occupancy_grid=grid, last={"n_samples": 1048000.0, "n_rays": 2100.0, "k": 3.0},
                               loss_device=lambda: torch.tensor([0.125]))
    bench.dump_outputs(tr, str(tmp_path), 0)
    files = sorted(os.listdir(tmp_path))
    names = {"loss", "batch", "occupancy_grid"} | {"param." + n for n, _ in renderer.named_parameters()}
    assert files == sorted(n + ".npy" for n in names)
    arrays = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(os.path.getsize(os.path.join(tmp_path, f)) for f in files) <= 64 << 20
    assert arrays["loss"].tolist() == [0.125] and arrays["batch"].tolist() == [1048000.0, 2100.0, 3.0]
    small = renderer.feature_module.planes[0][1].plane
    np.testing.assert_array_equal(arrays["param.feature_module.planes.0.1.plane"], small.detach().numpy())
    big = renderer.feature_module.planes[2][1].plane.detach()
    idx = np.sort(np.random.default_rng(0).choice(big.numel(), 1 << 20, replace=False))
    np.testing.assert_array_equal(arrays["param.feature_module.planes.2.1.plane"], big.reshape(-1).numpy()[idx])


@pytest.mark.gpu
def test_bench_steps_and_dump(tmp_path):
    """`--warmup 1 --steps 2`: the trainer ends on step 3, and the dump holds that step's loss, the one the JSON line reports"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--views", "2",
                        "--no-cpu-baseline", "--no-stages", "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=500)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["windows"]["n"] == 1 and line["psnr_at_step"]["step"] == 3
    loss = np.load(os.path.join(tmp_path, "loss.npy"))
    batch = np.load(os.path.join(tmp_path, "batch.npy"))
    assert loss.dtype == np.float64 and float(np.float32(loss[0])) == line["loss"]
    assert 0.9 * 2 ** 20 < batch[0] < 1.3 * 2 ** 20 and batch[1] > 0
    from tinynerf_amd.run import TrainConfig, build_renderer
    cfg = TrainConfig(method="kplanes", scene_type="aabb", batch_size=1024, n_samples=1024, seed=0)
    names = sorted("param." + n + ".npy" for n, _ in build_renderer(cfg, torch.ones(3), torch.device("cpu"))[0].named_parameters())
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("param.")) == names          # every parameter of the headline model
    assert all(np.isfinite(np.load(os.path.join(tmp_path, f))).all() for f in names)


def test_replay_walks_to_a_golden_step():
    """the PSNR replay of a timed run goes on to the first step of G21 at or after the run's last one: the driver's --warmup 5 --steps 20
    ends on 25 and is replayed to 30, the defaults end on 30, --windows 3 on 65"""
    bench = _bench()
    assert [bench.replay_step(s) for s in (0, 1, 25, 30, 31, 65, 66, 70)] == [0, 30, 30, 30, 65, 65, 70, 70]
    assert bench.replay_step(71) is None
