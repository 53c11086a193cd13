#!/usr/bin/env python3
"""Time the TSDF fusion on a K-Planes model trained for a few steps: tn_tsdf_integrate over the test views of the small
scene at several numbers of views per launch, the mask, the colour pass (tn_tsdf_integrate_color over the same views, tn_tsdf_sample_colors
at the mesh's vertices), and the whole export -- decoder and fused colours -- next to export_mesh at the same resolution.

    python scripts/tsdf_time.py [--resolution 256] [--views 100] [--res 200] [--steps 50] [--calls 7]

HIP events, median of --calls, allocations outside the window.  The views are rendered once; the timed call is the integration of all
of them into zeroed S and W (the memsets are inside the window: 8 B per node).  Every number of views per launch gives the same bytes
(checked here before timing), so the host layer's VIEWS_PER_LAUNCH is a matter of these times alone."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tinynerf_amd import mesh as M, rays, tsdf  # noqa: E402
from tinynerf_amd.points import default_crop  # noqa: E402
from tinynerf_amd.run import TrainConfig, Trainer  # noqa: E402


def median_us(fn, calls):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


class Views:
    """the pose dataset of the synthetic scene's cameras: what export_tsdf_mesh needs of a data.PoseDataset"""

    def __init__(self, cams, K, device):
        self.cameras, self.K = cams.cpu(), K
        self.rays_o, self.rays_d = rays.generate_rays(cams.to(device), K)

    def img_intrinsics(self, i):
        return self.K

    def __len__(self):
        return self.rays_o.size(0)

    def __getitem__(self, i):
        return {"rays_o": self.rays_o[i], "rays_d": self.rays_d[i]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--res", type=int, default=200)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--calls", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    o, d, rgb, _, _ = rays.synthetic_scene(n_views=4, res=args.res, seed=0, device=dev)
    tr = Trainer(TrainConfig(method="kplanes", batch_size=4096, seed=0), o, d, rgb, torch.ones(3, device=dev), dev)
    for _ in range(args.steps):
        tr.step()
    torch.cuda.synchronize()
    K = rays.blender_intrinsics(args.res)
    views = Views(rays.look_at_origin_poses(args.views, seed=1), K, dev)
    crop = default_crop(tr.cfg)
    lo, h, dims = M.grid_dims(crop, args.resolution)
    nodes = (dims[0] + 1) * (dims[1] + 1) * (dims[2] + 1)
    trunc = 4.0 * float(h.max())
    cams = tsdf.camera_table(views, None, dev)
    depth = torch.empty(cams.n_rays, dtype=torch.float32, device=dev)
    opacity = torch.empty_like(depth)
    rgb = torch.empty((cams.n_rays, 3), dtype=torch.float32, device=dev)
    t0 = time.perf_counter()
    for i in range(len(views)):
        maps = tr.render_rays(views.rays_o[i].reshape(-1, 3), views.rays_d[i].reshape(-1, 3), maps=True)
        depth[cams.offsets[i]:cams.offsets[i + 1]] = maps["depth"]
        opacity[cams.offsets[i]:cams.offsets[i + 1]] = maps["opacity"]
        rgb[cams.offsets[i]:cams.offsets[i + 1]] = maps["rgb"].reshape(-1, 3)
    torch.cuda.synchronize()
    print(f"{len(views)} views of {args.res} x {args.res} rendered in {(time.perf_counter() - t0) * 1e3:.0f} ms; {nodes} nodes "
          f"({dims[0]} x {dims[1]} x {dims[2]} cells), trunc {trunc:.4f}; {float((opacity >= 0.5).float().mean()) * 100:.1f} % of the pixels pass the opacity gate")
    S, W = torch.zeros((dims[2] + 1, dims[1] + 1, dims[0] + 1), device=dev), torch.zeros((dims[2] + 1, dims[1] + 1, dims[0] + 1), device=dev)

    def run(per_launch):
        tsdf.VIEWS_PER_LAUNCH = per_launch
        S.zero_(), W.zero_()
        tsdf.integrate(cams, depth, opacity, crop, dims, trunc, state=(S, W))

    default = tsdf.VIEWS_PER_LAUNCH                                # (before run() changes it)
    run(len(views))
    want = (S.clone(), W.clone())
    print(f"votes: {int(W.sum())} ({float(W.sum()) / nodes / len(views) * 100:.1f} % of node x view), {float((W > 0).float().mean()) * 100:.1f} % of the nodes observed")
    for per_launch in sorted({1, 4, 8, 16, 32, len(views)}):
        if per_launch > len(views):
            continue
        run(per_launch)
        assert torch.equal(S, want[0]) and torch.equal(W, want[1]), per_launch
        t = median_us(lambda: run(per_launch), args.calls)
        launches = -(-len(views) // per_launch)
        print(f"integrate, {per_launch:4d} views per launch ({launches:3d} launches): {t[0]:9.0f} us (median of {args.calls}; {t[1]:.0f} - {t[2]:.0f})"
              f"  = {t[0] * 1e6 / (nodes * len(views)):.2f} ps per node and view")
    tsdf.VIEWS_PER_LAUNCH = default
    values = tsdf.field(S, W)
    vert, nrm, faces, cells = M.extract_with_cells(values, lo, h, 0.0)
    t = median_us(lambda: tsdf.mask_faces(W, dims, cells, vert.size(0), faces), args.calls)
    masked = tsdf.mask_faces(W, dims, cells, vert.size(0), faces)
    print(f"mask_faces, {vert.size(0)} vertices, {faces.size(0)} faces ({int((masked[:, 0] < 0).sum())} masked): {t[0]:.0f} us ({t[1]:.0f} - {t[2]:.0f})")
    # the colour pass (6k): the same views into a zeroed colour volume (its memset, 16 B per node, inside the window), then the volume
    # sampled at the vertices that survive mask and filter
    bg = tr.renderer._bg(dev)
    volume = torch.zeros((dims[2] + 1, dims[1] + 1, dims[0] + 1, 4), device=dev)

    def run_color(per_launch):
        tsdf.VIEWS_PER_LAUNCH = per_launch
        volume.zero_()
        tsdf.integrate_color(cams, depth, opacity, rgb, bg, crop, dims, trunc, state=volume)

    run_color(len(views))
    want_volume = volume.clone()
    for per_launch in sorted({1, 8, default, 32, len(views)}):
        if per_launch > len(views):
            continue
        run_color(per_launch)
        assert torch.equal(volume, want_volume), per_launch
        t = median_us(lambda: run_color(per_launch), args.calls)
        print(f"integrate_color, {per_launch:4d} views per launch: {t[0]:9.0f} us (median of {args.calls}; {t[1]:.0f} - {t[2]:.0f})"
              f"  = {t[0] * 1e6 / (nodes * len(views)):.2f} ps per node and view")
    tsdf.VIEWS_PER_LAUNCH = default
    print(f"{float((volume[..., 3] > 0).float().mean()) * 100:.1f} % of the nodes coloured, sum of the weights {float(volume[..., 3].sum()):.0f}")
    kept = M.filter_components(vert, nrm, None, masked, min_faces=1)[0]
    t = median_us(lambda: tsdf.sample_colors(volume, crop, dims, kept), args.calls)
    den = tsdf.sample_colors(volume, crop, dims, kept)[1]
    print(f"sample_colors, {kept.size(0)} vertices ({int((den == 0).sum())} without colour): {t[0]:.0f} us ({t[1]:.0f} - {t[2]:.0f})")
    for name, fn in (("export_tsdf_mesh (render + integrate + extract + mask + filter + colours, no file)",
                      lambda: tsdf.export_tsdf_mesh(tr, views, None, resolution=args.resolution)),
                     ("export_tsdf_mesh, colors='fused' (the same with the colour volume instead of the decoder)",
                      lambda: tsdf.export_tsdf_mesh(tr, views, None, resolution=args.resolution, colors="fused")),
                     ("export_mesh at the same resolution (density query + extract + colours, no file)",
                      lambda: M.export_mesh(tr, None, resolution=args.resolution))):
        whole = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            whole.append(time.perf_counter() - t0)
        print(f"{name}, host clock: {sorted(whole)[1] * 1e3:.1f} ms (median of 3); {out[0].size(0)} vertices, {out[3].size(0)} faces")


if __name__ == "__main__":
    main()
