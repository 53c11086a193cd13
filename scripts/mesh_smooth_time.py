#!/usr/bin/env python3
"""Time the mesh smoothing: tn_mesh_adjacency, one tn_mesh_smooth_pass, tn_mesh_smooth and tn_mesh_vertex_normals on the
mesh DESIGN 6h measured -- a K-Planes model trained for a few steps, extracted at the density 1 node in 200 exceeds -- and on the TSDF
mesh of the same model at the same resolution.

    python scripts/mesh_smooth_time.py [--resolution 256] [--steps 50] [--tsdf_steps 200] [--calls 7] [--views 100] [--res 200] [--iterations 10]

The density mesh is taken after --steps steps (DESIGN 6h's mesh), the TSDF mesh after --tsdf_steps in all: a model too young renders
too little opacity for the fusion to observe any cell, and an empty mesh would leave nothing to time.

HIP events, median of --calls, allocations outside the window; the entry points enqueue their launches themselves, so the events go
around whole calls.  Beside each time: the bytes the call moves by the definition (every input and output once; the gathers as the
definition counts them: 8 d bytes of ids and 24 d bytes of positions per vertex) and what they take at 6.3 TB/s."""
import argparse
import ctypes as C
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tinynerf_amd import _lib as L, mesh as M, rays, tsdf  # noqa: E402
from tinynerf_amd.points import default_crop  # noqa: E402
from tinynerf_amd.run import TrainConfig, Trainer  # noqa: E402

HBM = 6.3e12


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


def line(what, t, moved):
    floor = moved / HBM * 1e6
    print(f"  {what:<44s} {t[0]:8.1f} us ({t[1]:.1f} - {t[2]:.1f});  {moved} B by the definition = {floor:.2f} us at 6.3 TB/s: {t[0] / floor:.1f} x")


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


def time_mesh(name, vert, nrm, faces, calls, iterations):
    dev = vert.device
    V, F = vert.size(0), faces.size(0)
    if V == 0 or F == 0:
        print(f"{name}: an empty mesh ({V} vertices, {F} triangles): nothing to time")
        return
    nbytes = C.c_int64(0)
    L.call_plain("tn_mesh_adjacency_workspace_bytes", C.c_int64(V), C.c_int64(F), C.byref(nbytes))
    work = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    offsets, pairs = torch.empty(V + 1, dtype=torch.int32, device=dev), torch.empty((3 * F, 2), dtype=torch.int32, device=dev)
    pinned, stats = torch.empty(V, dtype=torch.uint8, device=dev), torch.zeros(3, dtype=torch.int64, device=dev)
    scratch, out, normals = torch.empty_like(vert), torch.empty_like(vert), torch.empty_like(vert)

    def adjacency():
        L.call("tn_mesh_adjacency", dev, L.ptr(faces), C.c_int64(V), C.c_int64(F), L.ptr(offsets), L.ptr(pairs), L.ptr(pinned), L.ptr(stats), L.ptr(work))

    def one_pass(pin):
        L.call("tn_mesh_smooth_pass", dev, L.ptr(vert), L.ptr(offsets), L.ptr(pairs), L.ptr(pinned) if pin else None, C.c_int64(V), C.c_float(0.5), L.ptr(out))

    def smooth():
        L.call("tn_mesh_smooth", dev, L.ptr(vert), L.ptr(offsets), L.ptr(pairs), L.ptr(pinned), C.c_int64(V), C.c_int32(iterations), C.c_float(0.5),
               C.c_float(-0.53), L.ptr(scratch), L.ptr(out))

    def vertex_normals():
        L.call("tn_mesh_vertex_normals", dev, L.ptr(out), L.ptr(offsets), L.ptr(pairs), C.c_int64(V), L.ptr(nrm), L.ptr(normals))

    t_adj = median_us(adjacency, calls)
    taking_part, free, largest = stats.tolist()
    rows = 3 * taking_part
    print(f"{name}: {V} vertices, {F} triangles, {taking_part} take part, {free} vertices free, largest degree {largest}, mean {rows / V:.2f}")
    # adjacency: the faces in, offsets, the rows and pinned out; the construction reads the faces three times more, the rows twice
    line("tn_mesh_adjacency (memset + 9 launches)", t_adj, 12 * F + 4 * (V + 1) + 8 * rows + V + 24)
    gather = 8 * rows + 24 * rows                                  # per vertex 8 d of ids and 24 d of positions
    line("tn_mesh_smooth_pass, pinned given", median_us(lambda: one_pass(True), calls), 8 * V + V + 12 * V + gather * free // max(V, 1) + 12 * V)
    line("tn_mesh_smooth_pass, pinned NULL", median_us(lambda: one_pass(False), calls), 8 * V + 12 * V + gather + 12 * V)
    t = median_us(smooth, calls)
    print(f"  tn_mesh_smooth, {iterations} iterations ({2 * iterations} passes){'':<8s} {t[0]:8.1f} us ({t[1]:.1f} - {t[2]:.1f}) = {t[0] / (2 * iterations):.1f} us a pass")
    line("tn_mesh_vertex_normals (with a fallback)", median_us(vertex_normals, calls), 8 * V + 12 * V + gather + 12 * V)
    whole = median_us(lambda: M.smooth_mesh(vert, nrm, faces, iterations), 3)
    print(f"  mesh.smooth_mesh({iterations}), allocations and the read-back of stats included: {whole[0]:.0f} us (median of 3)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--tsdf_steps", type=int, default=200, help="steps in all before the TSDF mesh is fused")
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--res", type=int, default=200)
    ap.add_argument("--iterations", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    o, d, rgb, _, _ = rays.synthetic_scene(n_views=4, res=args.res, seed=0, device=dev)
    tr = Trainer(TrainConfig(method="kplanes", batch_size=4096, seed=0), o, d, rgb, torch.ones(3, device=dev), dev)
    for _ in range(args.steps):
        tr.step()
    torch.cuda.synchronize()
    crop = default_crop(tr.cfg)
    lo, h, dims = M.grid_dims(crop, args.resolution)
    values = M.density_grid(tr, crop, dims)[0]
    level = math.log(M.default_level(h))
    vert, nrm, faces = M.extract(values, lo, h, level)
    if vert.size(0) == 0:
        # as scripts/mesh_time.py: a model this young has no surface at the default level -- the density 1 node in 200 exceeds
        level = float(values.flatten().kthvalue(int(0.995 * values.numel())).values)
        print(f"no surface at the default level sigma = {M.default_level(h):.2f}: timing at sigma = {math.exp(level):.2f} instead")
        vert, nrm, faces = M.extract(values, lo, h, level)
    del values
    time_mesh(f"K-Planes, {args.steps} steps, resolution {args.resolution}", vert, nrm, faces, args.calls, args.iterations)
    for _ in range(max(0, args.tsdf_steps - args.steps)):
        tr.step()
    torch.cuda.synchronize()
    views = Views(rays.look_at_origin_poses(args.views, seed=1), rays.blender_intrinsics(args.res), dev)
    vert, nrm, _, faces = tsdf.export_tsdf_mesh(tr, views, None, resolution=args.resolution, colors=False)
    time_mesh(f"TSDF mesh of the same model after {max(args.steps, args.tsdf_steps)} steps, {args.views} views of {args.res} x {args.res}, resolution {args.resolution}", vert.contiguous(), nrm.contiguous(),
              faces.contiguous(), args.calls, args.iterations)


if __name__ == "__main__":
    main()
