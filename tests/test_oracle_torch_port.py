"""Pin the differentiable CPU port (oracle/torch_port.py) to G9, captured from the reference's
NerfRenderer.forward / backward."""
import functools

import numpy as np
import pytest
import torch

import _hashgrid_ref as hg
from conftest import load_golden
from oracle import torch_port as tp


def test_port_matches_reference_renderer():
    g = load_golden("G9_renderer_kplanes")
    sd = {k[3:]: torch.as_tensor(v) for k, v in g.items() if k.startswith("sd.")}
    packed, info = torch.as_tensor(g["packed"]), torch.as_tensor(g["info"])
    bg, target = torch.as_tensor(g["bg"]), torch.as_tensor(g["target"])
    out = tp.render(sd, packed, info, bg)
    np.testing.assert_allclose(out.numpy(), g["rendered"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(tp.render(sd, packed, info, None).numpy(), g["rendered_nobg"], rtol=0, atol=1e-6)
    grads, loss = tp.grads_of(sd, lambda p: torch.nn.functional.mse_loss(tp.render(p, packed, info, bg), target))
    np.testing.assert_allclose(loss, float(g["loss"]), rtol=1e-6)
    for k, v in grads.items():
        np.testing.assert_allclose(v, g["grad." + k], rtol=1e-4, atol=1e-9, err_msg=k)
    assert len(grads) == sum(1 for k in g if k.startswith("grad."))


# ---------------------------------------------------------------------------------------------------------------------------------
# The hash grid's port (tp.hashgrid_features) against the float64 yardstick tests/_hashgrid_ref.py: the port is what the GPU
# training tests hold the HIP field to, the yardstick what the two ABI calls are pinned to per entry -- two restatements of one
# definition, written independently (torch index / autograd there, numpy add.at here).
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _hashgrid_case(name):
    cfg = {"small": hg.SMALL, "fine": hg.FINE}[name]
    plan = hg.levels(**cfg)
    n, F = 4099, 2
    rng = np.random.default_rng(77 + len(name))
    x = hg.sample_points(n, plan, seed=n)
    table = rng.uniform(-1, 1, (hg.total_entries(plan), F))
    g = rng.uniform(-1, 1, (n, len(plan[0]) * F))
    feat = hg.forward(table, x, plan)
    grad, m, _ = hg.backward(g, x, plan, F)
    return plan, x, table, g, feat, grad, m


@pytest.mark.parametrize("name", ["small", "fine"])
def test_hashgrid_port_matches_the_fp64_yardstick(name):
    """fp64 port: features and the table gradient (autograd) within 1e-12 of the yardstick's largest element -- room for the order of
    an fp64 sum and nothing else; entries that no sample touches get exactly 0; the fp32 port's features within the project's forward
    bound 1e-5."""
    plan, x, table, g, feat, grad, m = _hashgrid_case(name)
    t64 = torch.from_numpy(table).requires_grad_(True)
    got = tp.hashgrid_features({"feature_module.table": t64}, torch.from_numpy(x), plan)
    assert got.dtype == torch.float64 and got.shape == feat.shape
    err_f = float(np.abs(got.detach().numpy() - feat).max())
    got.backward(torch.from_numpy(g))
    got_grad = t64.grad.numpy()
    err_g = float(np.abs(got_grad - grad).max())
    print(f"hash-grid port {name}: features differ by {err_f:.3e} (largest {np.abs(feat).max():.3f}), "
          f"table gradient by {err_g:.3e} (largest {np.abs(grad).max():.3f})")
    assert err_f <= 1e-12 * float(np.abs(feat).max())
    assert err_g <= 1e-12 * float(np.abs(grad).max())
    assert (m == 0).any() and (m > 0).any()
    assert np.all(got_grad[m == 0] == 0.0)
    t32 = torch.from_numpy(table.astype(np.float32))
    got32 = tp.hashgrid_features({"feature_module.table": t32}, torch.from_numpy(x), plan)
    assert got32.dtype == torch.float32
    ref32 = hg.forward(table.astype(np.float32), x, plan)
    assert float(np.abs(got32.numpy().astype(np.float64) - ref32).max()) <= 1e-5


def test_hashgrid_port_threads_through_features_and_render():
    """``hashgrid=plan`` selects the field in ``features`` / ``render`` as ``cobafa_freqs`` does; ``reference_training`` wants the
    method and the plan together."""
    plan, x, table, *_ = _hashgrid_case("small")
    sd = {"feature_module.table": torch.from_numpy(table.astype(np.float32))}
    xs = torch.from_numpy(x[:64])
    assert torch.equal(tp.features(sd, xs, hashgrid=plan), tp.hashgrid_features(sd, xs, plan))
    with pytest.raises(ValueError):
        tp.reference_training(sd, None, None, None, method="hashgrid", batch_size=256, n_samples=32, n_steps=1)
