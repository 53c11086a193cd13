"""GPU tests of the SSIM metric: tn_ssim / run.ssim against the fp64 restatement of the definition (tests/_ssim_ref.py) on the same
float32 inputs -- map and mean --, closed forms, determinism, argument checks, and evaluate(ssim=True) / train(ssim=True) end to end."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import _ssim_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
# the project's fp32 parity level (SURVEY, tests/test_hip_maps.py TOL): every map entry and the mean, absolute, no case excluded.
# Measured on one MI355X over the 105 cases below: worst map entry 1.83e-6 (disc, 800 x 800 x 3, data_range 255), worst mean 5.19e-7
# (disc, 11 x 11 x 1: one window, the mean IS the entry; over the 800 x 800 cases the worst mean is 2.1e-8 = one fp32 rounding of it).
TOL = 1e-5
TOL_MEAN = 2.1e-6       # 4 x the worst measured mean error, never looser than TOL
assert TOL_MEAN <= TOL

TW, TH = 32, 8          # the kernel's tile of windows (csrc/metrics.hip): T + 10, T + 11 and 2 T + 10 in both directions are below
SIZES = [(11, 11), (11, 64), (12, 37), (43, 75), (TH + 10, TW + 10), (TH + 11, TW + 11), (2 * TH + 10, 2 * TW + 10), (TH + 10, 2 * TW + 10),
         (2 * TH + 10, TW + 11), (200, 200), (800, 800)]
PATTERNS = sorted(ref.PATTERNS)


def _cases():
    out = [(p, h, w, 3, 1.0) for (h, w) in SIZES for p in PATTERNS]
    out += [(p, h, w, c, 1.0) for (h, w) in [(11, 11), (12, 37), (43, 75), (2 * TH + 10, 2 * TW + 10), (200, 200)] for p in PATTERNS for c in (1, 4)]
    out += [("ramp", 800, 800, 1, 1.0), ("clipped", 800, 800, 4, 1.0), ("disc", 200, 200, 2, 1.0)]
    out += [(p, h, w, 3, 255.0) for (h, w) in [(11, 11), (43, 75), (200, 200), (800, 800)] for p in PATTERNS]
    out += [("disc", 43, 75, 1, 255.0), ("disc", 43, 75, 4, 255.0)]
    return out


def _pair(pattern, h, w, c, data_range, seed=0):
    a, b = ref.PATTERNS[pattern](h, w, c, seed=seed)
    if data_range != 1.0:
        a, b = a * np.float32(data_range), b * np.float32(data_range)
    return np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)


@pytest.mark.parametrize("pattern,h,w,c,data_range", _cases())
def test_ssim_map_and_mean_against_fp64(pattern, h, w, c, data_range):
    """every map entry within TOL of the fp64 definition on the same float32 inputs, the mean within TOL_MEAN.  "disc" is the case
    raw fp32 moments fail 50-fold (flat 1.0 background: c2 = 9e-4 is the whole denominator of the second factor)."""
    from tinynerf_amd import run
    a, b = _pair(pattern, h, w, c, data_range)
    want = ref.ssim_map(a, b, data_range)
    mean, smap = run.ssim(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), data_range, return_map=True)
    assert mean.shape == () and mean.dtype == torch.float32 and mean.is_cuda
    assert smap.shape == (h - 10, w - 10, c) and smap.dtype == torch.float32 and smap.is_contiguous()
    got = smap.cpu().numpy().astype(np.float64)
    err_map = float(np.abs(got - want).max())
    err_mean = abs(float(mean.item()) - float(want.mean()))
    print(f"ssim {pattern} {h}x{w}x{c} L={data_range:g}: value {want.mean():.6f} map err {err_map:.3g} mean err {err_mean:.3g}")
    assert np.isfinite(got).all()
    assert err_map <= TOL
    assert err_mean <= TOL_MEAN


@pytest.mark.parametrize("data_range", [1.0, 255.0])
@pytest.mark.parametrize("p,q", [(0.0, 0.0), (1.0, 1.0), (0.25, 0.75), (1.0, 0.0), (0.5, 0.501)])
def test_constant_images_give_the_closed_form(p, q, data_range):
    """variances are 0 and the second factor 1: (2pq + c1) / (p^2 + q^2 + c1) in every entry"""
    from tinynerf_amd import run
    a = torch.full((27, 50, 3), p * data_range, device=DEV)
    b = torch.full((27, 50, 3), q * data_range, device=DEV)
    pa, qb = float(a[0, 0, 0]), float(b[0, 0, 0])
    c1 = (0.01 * data_range) ** 2
    want = (2 * pa * qb + c1) / (pa * pa + qb * qb + c1)
    mean, smap = run.ssim(a, b, data_range, return_map=True)
    assert np.abs(smap.cpu().numpy().astype(np.float64) - want).max() <= TOL
    assert abs(mean.item() - want) <= TOL


@pytest.mark.parametrize("pattern", PATTERNS)
def test_identical_images_give_one(pattern):
    from tinynerf_amd import run
    a, _ = _pair(pattern, 61, 45, 3, 1.0, seed=4)
    x = torch.from_numpy(a).to(DEV)
    mean, smap = run.ssim(x, x.clone(), return_map=True)
    assert np.abs(smap.cpu().numpy().astype(np.float64) - 1.0).max() <= TOL
    assert abs(mean.item() - 1.0) <= TOL


@pytest.mark.parametrize("h,w,c", [(43, 75, 3), (800, 800, 3), (200, 200, 4)])
def test_mean_is_the_same_bits_on_every_call_and_without_the_map(h, w, c):
    from tinynerf_amd import run
    a, b = _pair("disc", h, w, c, 1.0, seed=7)
    x, y = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    m0 = run.ssim(x, y)
    m1 = run.ssim(x, y)
    m2, smap = run.ssim(x, y, return_map=True)
    m3, smap3 = run.ssim(x, y, return_map=True)
    bits = [int(m.view(torch.int32).item()) for m in (m0, m1, m2, m3)]
    assert len(set(bits)) == 1, bits
    assert torch.equal(smap, smap3)
    assert isinstance(m0, torch.Tensor) and m0.dim() == 0


def test_entry_point_refuses_a_short_workspace_and_leaves_the_outputs_alone():
    from tinynerf_amd import _lib as L
    h, w, c = 43, 75, 3
    a, b = _pair("noise", h, w, c, 1.0)
    x, y = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    n = C.c_int64(0)
    L.call_plain("tn_ssim_workspace_bytes", C.c_int64(h), C.c_int64(w), C.c_int32(c), C.byref(n))
    assert n.value > 0
    ws = torch.zeros(n.value, dtype=torch.uint8, device=DEV)
    mean = torch.full((1,), -7.0, device=DEV)
    args = (L.ptr(x), L.ptr(y), C.c_int64(h), C.c_int64(w), C.c_int32(c), C.c_float(1.0), C.c_void_p(None), L.ptr(ws))
    rc = L.lib().tn_ssim(*args, C.c_int64(n.value - 1), L.ptr(mean), L.stream(torch.device(DEV, 0)))
    assert rc == -3 and b"tn_ssim" in L.lib().tn_last_error_string()
    torch.cuda.synchronize()
    assert mean.item() == -7.0
    L.call("tn_ssim", torch.device(DEV, 0), *args, C.c_int64(n.value), L.ptr(mean))
    assert abs(mean.item() - ref.ssim(a, b)) <= TOL


def test_wrapper_refuses_what_the_kernel_cannot_read():
    from tinynerf_amd import run
    x = torch.rand(40, 40, 3, device=DEV)
    with pytest.raises(RuntimeError, match="contiguous"):
        run.ssim(x.transpose(0, 1), x.transpose(0, 1))
    with pytest.raises(RuntimeError, match="contiguous"):
        run.ssim(x[:, ::2], x[:, ::2])
    with pytest.raises(RuntimeError, match="float32"):
        run.ssim(x.double(), x.double())
    with pytest.raises(RuntimeError, match="CUDA"):
        run.ssim(x.cpu(), x.cpu())
    with pytest.raises(RuntimeError, match="CUDA"):
        run.ssim(x, x.cpu())
    with pytest.raises(RuntimeError, match="same shape"):
        run.ssim(x, x[:30].contiguous())
    with pytest.raises(RuntimeError, match="11"):
        run.ssim(x[:10].contiguous(), x[:10].contiguous())
    with pytest.raises(RuntimeError, match="C <= 4"):
        run.ssim(torch.rand(20, 20, 5, device=DEV), torch.rand(20, 20, 5, device=DEV))
    with pytest.raises(ValueError, match="data_range"):
        run.ssim(x, x, data_range=0.0)
    with pytest.raises(ValueError, match="data_range"):
        run.ssim(x, x, data_range=float("nan"))


# ------------------------------------------------------------------------------------------------ evaluate() / train() end to end
def _scene_on_disk(root, res=48):
    """a Blender-format scene of three views of the synthetic ball; the test split is the first view"""
    from PIL import Image
    from tinynerf_amd import rays
    o, d, rgb, K, cams = rays.synthetic_scene(n_views=3, res=res, seed=5, device="cpu")
    imgs = (rgb.reshape(3, res, res, 3) * 255).to(torch.uint8).numpy()
    (root / "train").mkdir()
    frames = []
    for i in range(3):
        Image.fromarray(imgs[i]).save(root / "train" / f"r_{i}.png")
        frames.append({"file_path": f"./train/r_{i}", "transform_matrix": cams[i].tolist()})
    for split in ("train", "test"):
        json.dump({"camera_angle_x": 0.6911112070083618, "frames": frames[:3 if split == "train" else 2]},
                  open(root / f"transforms_{split}.json", "w"))


def test_train_writes_the_ssim_of_the_float_renders(tmp_path):
    from tinynerf_amd import data
    from tinynerf_amd.run import TrainConfig, evaluate, infer, train
    _scene_on_disk(tmp_path)
    dev = torch.device(DEV)
    train_rays = data.RaysDataset(data.parse_nerf_synthetic(tmp_path, "train"), dev)
    test_set = data.PoseDataset(data.parse_nerf_synthetic(tmp_path, "test"), dev)
    eval_set = data.PoseDataset(data.parse_nerf_synthetic(tmp_path, "test"), dev)

    def cfg():
        return TrainConfig(method="kplanes", batch_size=512, n_samples=64, occupancy_res=32, kplanes_resolutions=(16, 32, 64), seed=3)

    out = tmp_path / "on"; out.mkdir()
    tr, _, evalm, testm = train(cfg(), train_rays, eval_set, test_set, out, eval_every=20, max_steps=40, log_every=50, ssim=True)
    written = json.load(open(out / "metrics_test.json"))
    assert written == testm and len(written) == 2 and set(written[0]) == {"mse_loss", "psnr", "ssim"}
    idx = [0, 1]
    renders = infer(tr, test_set, idx)                      # the float images the metrics were computed on (inference is deterministic)
    plain = evaluate(test_set, renders, idx)                # ssim=False
    for i, (m, p, img) in enumerate(zip(written, plain, renders)):
        want = ref.ssim(test_set[i]["rgbs"].cpu().numpy(), img.cpu().numpy())
        print(f"train(ssim=True) image {i}: ssim {m['ssim']:.6f} fp64 {want:.6f} psnr {m['psnr']:.3f}")
        assert abs(m["ssim"] - want) <= TOL
        assert 0.0 < m["ssim"] <= 1.0
        assert m["mse_loss"] == p.mse_loss and m["psnr"] == p.psnr
        assert p.ssim == 0.0
    with_ssim = evaluate(test_set, renders, idx, ssim=True)
    assert [m.ssim for m in with_ssim] == [m["ssim"] for m in written]
    assert [(m.mse_loss, m.psnr) for m in with_ssim] == [(m.mse_loss, m.psnr) for m in plain]
    periodic = json.load(open(out / "metrics_eval.json"))   # steps 20 and 40, one image each
    assert len(periodic) == 2 and all(0.0 < m["ssim"] <= 1.0 for m in periodic)

    off = tmp_path / "off"; off.mkdir()
    train(cfg(), train_rays, eval_set, test_set, off, eval_every=20, max_steps=40, log_every=50)
    assert [m["ssim"] for m in json.load(open(off / "metrics_test.json"))] == [0.0, 0.0]
    assert [m["ssim"] for m in json.load(open(off / "metrics_eval.json"))] == [0.0, 0.0]
