"""tn_camera_rays on the GPU, through the C ABI and through rays.CameraRays: directions against the float64 yardstick
(tests/_camera_ref.py) for the three lens models, the reference's own pinhole rays (G12), the ranks' shares, the lens that cannot be
inverted, the trainer on a camera source against the trainer on ray tables, train() on captures written to disk, and infer / evaluate
on a set with two image sizes.  Bound on a direction component: 1e-5 absolute, the project's floating-point parity bound (README)."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import _camera_ref as ref
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOUND = 1e-5


def _poses(n, seed=0):
    from tinynerf_amd import rays
    return rays.look_at_origin_poses(n, radius=3.0, seed=seed).numpy()


def _mixed_table():
    """eight images of four sizes, every fixture lens, all three models -- 5.5 M pixels, enough for 3 + 4 * (2^20 + 12)"""
    F = ref.FIXTURES
    cams = [(F["opencv_a"], ref.W, ref.H), (F["fisheye"], ref.W, ref.H), (F["pinhole"], 200, 200), (F["opencv_b"], ref.W, ref.H),
            (ref.scaled(F["opencv_c"], 648, 484), 648, 484), (F["opencv_c"], ref.W, ref.H), (ref.scaled(F["fisheye"], 324, 242), 324, 242),
            (ref.scaled(F["opencv_a"], 648, 484), 648, 484)]
    models = [m for (m, _), _, _ in cams]
    lenses = np.stack([L for (_, L), _, _ in cams])
    sizes = [[w, h] for _, w, h in cams]
    return _poses(len(cams), seed=7), models, lenses, sizes


@pytest.fixture(scope="module")
def mixed():
    from tinynerf_amd import rays
    c2w, models, lenses, sizes = _mixed_table()
    rng = np.random.default_rng(5)
    rgb = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for w, h in sizes]
    src = rays.CameraRays(torch.from_numpy(c2w), torch.from_numpy(lenses), models, sizes, rgb, DEV)
    # the yardstick sees what the kernel is given: the float32 table
    host = dict(c2w=src.c2w.cpu().double().numpy(), lenses=src.lens.cpu().double().numpy(), models=models, sizes=sizes,
                rgb=torch.cat([im.reshape(-1, 3) for im in rgb]).numpy())
    return src, host


def _check(src, host, g, o, d, rgb, worst):
    o, d = o.cpu().numpy(), d.cpu().numpy()
    want_o, want_d, img = ref.table_rays(host["c2w"], host["models"], host["lenses"], host["sizes"], g)
    assert np.isfinite(d).all()
    err = np.abs(d - want_d).max(-1)
    for m in (0, 1, 2):
        sel = np.asarray(host["models"])[img] == m
        if sel.any():
            worst[m] = max(worst.get(m, 0.0), float(err[sel].max()))
    assert err.max() <= BOUND, (err.max(), g[err.argmax()])
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=-1) - 1.0).max() <= BOUND
    assert np.array_equal(o, want_o.astype(np.float32))                         # origins: the table's, bit for bit
    if rgb is not None:
        assert np.array_equal(rgb.cpu().numpy(), host["rgb"][g].astype(np.float32) / np.float32(255))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, 2 ** 20 + 13])
def test_directions_match_the_float64_yardstick(mixed, n):
    """mixed table, random idx (through CameraRays.gather) and idx = NULL (through the C ABI), (first, stride) in {(0, 1), (3, 4)}"""
    from tinynerf_amd import _lib as L
    src, host = mixed
    dev = torch.device(DEV)
    worst = {}
    rng = np.random.default_rng(n)
    for first, stride in ((0, 1), (3, 4)):
        limit = (src.n_rays - first + stride - 1) // stride
        assert limit >= n
        idx = rng.integers(0, limit, n).astype(np.int32)
        if n >= 64:
            idx[:3] = [0, limit - 1, limit // 2]
        o, d, rgb = (torch.full((n + 7, 3), 7.0, device=DEV) for _ in range(3))
        src.gather(torch.from_numpy(idx).to(DEV), o, d, rgb, first=first, stride=stride)
        _check(src, host, first + stride * idx.astype(np.int64), o[:n], d[:n], rgb[:n], worst)
        for t in (o, d, rgb):
            assert bool((t[n:] == 7.0).all())                                    # nothing written past n
        # idx = NULL, raw ABI, no colours; the range starts where an image border falls inside it
        start = first + stride * ((src.offsets[1] - first) // stride - min(n, 40) // 2) if n > 1 else first
        start = max(first, min(start, first + stride * (limit - n)))
        o2, d2 = torch.full((n + 7, 3), 7.0, device=DEV), torch.full((n + 7, 3), 7.0, device=DEV)
        L.call("tn_camera_rays", dev, C.byref(src.table), C.c_void_p(None), C.c_int64(start), C.c_int64(stride), C.c_int64(n), L.ptr(o2), L.ptr(d2),
               C.c_void_p(None))
        _check(src, host, start + stride * np.arange(n, dtype=np.int64), o2[:n], d2[:n], None, worst)
        assert bool((o2[n:] == 7.0).all()) and bool((d2[n:] == 7.0).all())
    print(f"n = {n}: worst |d - fp64| pinhole {worst.get(0, 0):.3g}, OpenCV {worst.get(1, 0):.3g}, fisheye {worst.get(2, 0):.3g}")


@pytest.mark.parametrize("name", sorted(ref.FIXTURES))
def test_whole_images_per_fixture_lens(name):
    """every pixel of the 1296 x 968 image of each fixture lens, through CameraRays.image()"""
    from tinynerf_amd import rays
    model, L = ref.FIXTURES[name]
    c2w = _poses(2, seed=11)[1:]
    src = rays.CameraRays(torch.from_numpy(c2w), torch.from_numpy(L)[None], [model], [[ref.W, ref.H]], None, DEV)
    o, d = src.image_rays(0)
    assert o.shape == d.shape == (ref.H, ref.W, 3)
    u, v = np.meshgrid(np.arange(ref.W), np.arange(ref.H), indexing="xy")
    want_o, want_d = ref.rays(src.c2w[0].cpu().double().numpy(), model, src.lens[0].cpu().double().numpy(), u, v)
    err = np.abs(d.cpu().numpy() - want_d).max()
    print(f"{name}: worst |d - fp64| over the image {err:.3g}")
    assert err <= BOUND
    assert np.array_equal(o.cpu().numpy(), want_o.astype(np.float32))


def test_pinhole_matches_the_references_own_rays():
    """G12: rays of the reference's hotdog fixture cameras, generated by the reference -- tolerances of tests/test_data.py"""
    from tinynerf_amd import rays
    g = load_golden("G12_rays_fixture")
    w, h = int(g["w"]), int(g["h"])
    lens = torch.tensor([[float(g["fx"]), float(g["fy"]), float(g["cx"]), float(g["cy"]), 0, 0, 0, 0, 0, 0]] * 2, dtype=torch.float64)
    src = rays.CameraRays(torch.as_tensor(g["cameras"]), lens, [0, 0], [[w, h]] * 2, None, DEV)
    (o0, d0), (_, d1) = src.image_rays(0), src.image_rays(1)
    np.testing.assert_allclose(d0[::25, ::25].cpu().numpy(), g["rays_d_0"], atol=1e-6)
    np.testing.assert_allclose(d1[::25, ::25].cpu().numpy(), g["rays_d_1"], atol=1e-6)
    np.testing.assert_allclose(o0[::25, ::25].cpu().numpy(), g["rays_o_0"], atol=0)


def test_the_four_shares_of_a_table_are_the_table():
    """first = rank, stride = 4: every pixel once.  The colour carries the flat pixel index."""
    from tinynerf_amd import rays
    sizes = [[37, 21], [16, 16], [50, 9]]
    n_px = sum(w * h for w, h in sizes)
    code = torch.arange(n_px, dtype=torch.int64)
    flat = torch.stack([code % 256, (code // 256) % 256, code // 65536], -1).to(torch.uint8)
    rgb, off = [], 0
    for w, h in sizes:
        rgb.append(flat[off:off + w * h].reshape(h, w, 3))
        off += w * h
    lens = torch.tensor([[30., 30., w / 2, h / 2, 0, 0, 0, 0, 0, 0] for w, h in sizes])
    src = rays.CameraRays(torch.from_numpy(_poses(3)), lens, [0, 0, 0], sizes, rgb, DEV)
    seen = []
    for rank in range(4):
        n = len(range(rank, n_px, 4))
        o, d, c = (torch.empty((n, 3), device=DEV) for _ in range(3))
        src.gather(torch.arange(n, dtype=torch.int32, device=DEV), o, d, c, first=rank, stride=4)
        b = torch.round(c * 255).long().cpu()
        seen.append(b[:, 0] + 256 * b[:, 1] + 65536 * b[:, 2])
        assert torch.equal(seen[-1], torch.arange(rank, n_px, 4))
    assert torch.equal(torch.sort(torch.cat(seen)).values, torch.arange(n_px))


def test_a_lens_that_cannot_be_inverted_still_gives_finite_unit_rays():
    from tinynerf_amd import rays
    model, L = ref.NOT_INVERTIBLE
    wild = L.copy()
    wild[4:8] = [-3.0, 40.0, -500.0, 9000.0]                 # and one whose Newton steps leave float32's range
    src = rays.CameraRays(torch.from_numpy(_poses(3, seed=2)), torch.from_numpy(np.stack([L, wild, wild])), [model, model, 2],
                          [[ref.W, ref.H]] * 3, None, DEV)
    for i in range(3):
        o, d = src.image_rays(i)
        assert bool(torch.isfinite(d).all()) and bool(torch.isfinite(o).all())
        assert float((d.double().norm(dim=-1) - 1.0).abs().max()) <= BOUND


def _ball_colours(o, d):
    """rays.synthetic_scene's analytic ball (radius .75 at the origin, white behind it) on any rays, in float64"""
    b = (o * d).sum(-1)
    c = (o * o).sum(-1) - 0.75 ** 2
    disc = b * b - c
    t = -b - np.sqrt(np.clip(disc, 0, None))
    col = 0.5 + 0.5 * np.sin(4.0 * (o + d * t[..., None]))
    return np.where((disc > 0)[..., None], col, 1.0)


def test_trainer_on_a_camera_source_draws_the_rays_of_the_tables():
    from tinynerf_amd import data, rays
    from tinynerf_amd.run import TrainConfig, Trainer
    o, d, rgb, K, cams = rays.synthetic_scene(n_views=3, res=48, seed=5, device="cpu")
    imgs = [im for im in (rgb.reshape(3, 48, 48, 3) * 255).to(torch.uint8)]
    nd = data.NerfData(cameras=cams, intrinsics=K, imgs=imgs, bg_color=torch.ones(3))
    table_set, camera_set = data.RaysDataset(nd, DEV), data.CameraRaysDataset(nd, DEV)
    assert len(table_set) == len(camera_set) == 3 * 48 * 48
    dev = torch.device(DEV)

    def cfg():
        return TrainConfig(method="kplanes", batch_size=256, n_samples=32, occupancy_res=32, kplanes_resolutions=(16, 32, 64), seed=3, deterministic=True)

    a = Trainer(cfg(), table_set.rays_o, table_set.rays_d, table_set.rgbs, torch.ones(3, device=DEV), dev)
    b = Trainer(cfg(), None, None, None, torch.ones(3, device=DEV), dev, ray_source=camera_set.source)
    assert a.n_rays == b.n_rays == 3 * 48 * 48
    for _ in range(3):
        a._launch_plan(n_b=4)
        b._launch_plan(n_b=4)
        torch.cuda.synchronize()
        pa, pb = a._pending, b._pending
        assert torch.equal(pa["idx"], pb["idx"])
        assert torch.equal(pa["o"], pb["o"])                                     # origins exact
        assert torch.equal(pa["rgb"], pb["rgb"])                                 # colours exact: both from the same bytes
        assert float((pa["d"] - pb["d"]).abs().max()) <= 1e-6
        a._pending = b._pending = None
        a._cursor = b._cursor = a._cursor + 1000
    for _ in range(5):                                                           # and it steps
        st = b.step()
    assert np.isfinite(b.loss_value()) and st["n_rays"] > 0
    with pytest.raises(ValueError):
        Trainer(cfg(), table_set.rays_o, table_set.rays_d, table_set.rgbs, None, dev, ray_source=camera_set.source)


def _write_capture(root, cams, images, lens_keys, f, size):
    from PIL import Image
    (root / "images").mkdir(parents=True)
    names = []
    for i, im in enumerate(images):
        names.append(f"images/frame_{i:03d}.png")
        Image.fromarray(im).save(root / names[-1])
    meta = {"fl_x": f, "fl_y": f, "cx": size / 2, "cy": size / 2, "w": size, "h": size, **lens_keys,
            "frames": [{"file_path": n, "transform_matrix": np.asarray(cams[i]).tolist()} for i, n in enumerate(names)],
            "train_filenames": names, "test_filenames": names[:1], "val_filenames": names[:1]}
    json.dump(meta, open(root / "transforms.json", "w"))


def _train_capture(root, out):
    from tinynerf_amd import data
    from tinynerf_amd.run import TrainConfig, train
    dev = torch.device(DEV)
    train_rays = data.CameraRaysDataset(data.parse_nerfstudio(root, "train", orient=False), dev)
    test_set = data.CameraPoseDataset(data.parse_nerfstudio(root, "test", orient=False), dev)
    out.mkdir()
    cfg = TrainConfig(method="kplanes", batch_size=512, n_samples=64, occupancy_res=32, kplanes_resolutions=(16, 32, 64), seed=3)
    tr, tm, em, testm = train(cfg, train_rays, None, test_set, out, max_steps=150, log_every=50)
    assert (out / "model.pt").exists() and (out / "metrics_train.json").exists() and (out / "metrics_test.json").exists()
    assert (out / "test_full_0000.png").exists()
    logged = json.load(open(out / "metrics_train.json"))
    assert len(logged) == 151 and set(logged[0]) == {"loss", "occupancy"}
    assert np.isfinite(logged[-1]["loss"]) and logged[-1]["loss"] < logged[0]["loss"]
    return testm[0]["psnr"]


def test_train_on_a_pinhole_capture_on_disk(tmp_path):
    """the twin of test_hip_training.test_train_entry_point_on_a_scene_on_disk: same scene, TrainConfig, seed and budget, written as a
    nerfstudio capture -- same gate"""
    from tinynerf_amd import rays
    o, d, rgb, K, cams = rays.synthetic_scene(n_views=3, res=48, seed=5, device="cpu")
    imgs = (rgb.reshape(3, 48, 48, 3) * 255).to(torch.uint8).numpy()
    _write_capture(tmp_path / "scene", cams, imgs, {}, K.fx, 48)
    p = _train_capture(tmp_path / "scene", tmp_path / "out")
    print(f"pinhole capture: held-out PSNR {p:.2f} dB")
    assert p > 18.0


def test_train_on_a_distorted_capture_on_disk(tmp_path):
    """the same ball photographed through the first OpenCV fixture lens (colours from the analytic scene on the YARDSTICK's rays, focal
    scaled to the image width); the run with the coefficients deleted from the json is reported beside it, not asserted"""
    from tinynerf_amd import rays
    cams = rays.look_at_origin_poses(3, seed=5).double().numpy()
    model, L = ref.scaled(ref.FIXTURES["opencv_a"], 48, 48 * ref.H // ref.W)
    L[3] = 24.0                                              # a square 48 x 48 image: taller than the fixture's -- checked right here
    assert ref.round_trip_error(model, L, 48, 48) <= 1e-12
    u, v = np.meshgrid(np.arange(48), np.arange(48), indexing="xy")
    imgs = []
    for cam in cams:
        o, d = ref.rays(cam, model, L, u, v)
        imgs.append((np.clip(_ball_colours(o, d), 0, 1) * 255).astype(np.uint8))
    coeffs = dict(zip(("k1", "k2", "k3", "k4", "p1", "p2"), L[4:].tolist()))
    _write_capture(tmp_path / "lens", cams, imgs, {"camera_model": "OPENCV", **coeffs}, float(L[0]), 48)
    _write_capture(tmp_path / "nolens", cams, imgs, {}, float(L[0]), 48)
    p = _train_capture(tmp_path / "lens", tmp_path / "out_lens")
    q = _train_capture(tmp_path / "nolens", tmp_path / "out_nolens")
    print(f"OpenCV capture: held-out PSNR {p:.2f} dB with its lens, {q:.2f} dB with the coefficients deleted")
    assert np.isfinite(p) and np.isfinite(q)


def test_infer_and_evaluate_on_two_image_sizes():
    from tinynerf_amd import data, rays
    from tinynerf_amd.run import TrainConfig, Trainer, evaluate, infer
    cams = rays.look_at_origin_poses(2, seed=5)
    sizes = [(40, 28), (24, 36)]
    Ks = [rays.Intrinsics(50., 50., w / 2, h / 2, w, h) for w, h in sizes]
    rng = np.random.default_rng(0)
    imgs = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for w, h in sizes]
    nd = data.NerfData(cameras=cams, intrinsics=Ks, imgs=imgs, bg_color=torch.ones(3), lens=torch.tensor([[0.05, 0, 0, 0, 0, 0], [0.0] * 6]), models=[1, 0])
    ds = data.CameraPoseDataset(nd, DEV)
    assert len(ds) == 2 and ds.rgbs and ds.img_intrinsics(1) is Ks[1]
    item = ds[1]
    assert item["rays_o"].shape == item["rays_d"].shape == item["rgbs"].shape == (36, 24, 3)
    assert torch.equal(item["rgbs"].cpu(), data._as_float(imgs[1])) and torch.equal(ds.rgbs[0].cpu(), data._as_float(imgs[0]))
    train_set = data.CameraRaysDataset(nd, DEV)
    batch = train_set[torch.tensor([0, 40 * 28, 40 * 28 + 25])]
    assert torch.equal(batch["rgbs"].cpu(), torch.stack([data._as_float(imgs[0])[0, 0], data._as_float(imgs[1])[0, 0], data._as_float(imgs[1])[1, 1]]))
    cfg = TrainConfig(method="kplanes", batch_size=128, n_samples=32, occupancy_res=32, kplanes_resolutions=(16, 32, 64), seed=1)
    tr = Trainer(cfg, None, None, None, torch.ones(3, device=DEV), torch.device(DEV), ray_source=train_set.source)
    tr.step()
    rendered = infer(tr, ds, [0, 1])
    assert [tuple(r.shape) for r in rendered] == [(28, 40, 3), (36, 24, 3)]
    metrics = evaluate(ds, rendered, [0, 1], ssim=True)
    assert len(metrics) == 2 and all(np.isfinite(m.psnr) and -1.0 <= m.ssim <= 1.0 and m.ssim != 0.0 for m in metrics)
