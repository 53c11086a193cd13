#!/usr/bin/env python3
"""Time the mesh-component filter: tn_mesh_components and tn_mesh_filter on the mesh DESIGN 6h measured -- a K-Planes model
trained for a few steps, extracted at the density 1 node in 200 exceeds -- and on disjoint triangles with shuffled ids and faces.

    python scripts/mesh_components_time.py [--resolution 256] [--steps 50] [--calls 7] [--triangles 1000000]

HIP events, median of --calls, allocations outside the window.  Both entry points enqueue their launches themselves, so the events go
around whole calls: tn_mesh_components; tn_mesh_filter as the count-only call (mark + scan), with vertices only (+ the vertex launch)
and with everything (+ the face launch) -- the vertex and face launches are differences.  The filter is timed at threshold 0 (every
row is copied: its worst case) and at the largest component's face count.  Also printed: the bytes every call moves by the definition
(each input and output once; the union-find's walks come on top and depend on the mesh) and what they take at 6.3 TB/s."""
import argparse
import ctypes as C
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tinynerf_amd import _lib as L, mesh as M, rays  # noqa: E402
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


def fmt(t):
    return f"{t[0]:.1f} us ({t[1]:.1f} - {t[2]:.1f})"


def time_mesh(name, vert, nrm, rgb, faces, calls):
    dev = vert.device
    V, F = vert.size(0), faces.size(0)
    nbytes = C.c_int64(0)
    L.call_plain("tn_mesh_components_workspace_bytes", C.c_int64(V), C.c_int64(F), C.byref(nbytes))
    work_c = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    L.call_plain("tn_mesh_filter_workspace_bytes", C.c_int64(V), C.c_int64(F), C.byref(nbytes))
    work_f = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    labels, face_counts = torch.empty(V, dtype=torch.int32, device=dev), torch.empty(V, dtype=torch.int32, device=dev)
    stats, counts = torch.zeros(3, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
    out_v, out_n = torch.empty_like(vert), torch.empty_like(nrm)
    out_c, src, out_f = torch.empty_like(rgb), torch.empty(V, dtype=torch.int32, device=dev), torch.empty_like(faces)

    def comp():
        L.call("tn_mesh_components", dev, L.ptr(faces), C.c_int64(V), C.c_int64(F), L.ptr(labels), L.ptr(face_counts), L.ptr(stats), L.ptr(work_c))

    def filt(T, vcap, fcap):
        L.call("tn_mesh_filter", dev, L.ptr(faces), L.ptr(labels), L.ptr(face_counts), C.c_int64(T), L.ptr(vert), L.ptr(nrm), L.ptr(rgb), C.c_int64(V),
               C.c_int64(F), C.c_int64(vcap), C.c_int64(fcap), L.ptr(out_v) if vcap else None, L.ptr(out_n) if vcap else None,
               L.ptr(out_c) if vcap else None, L.ptr(src) if vcap else None, L.ptr(out_f) if fcap else None, L.ptr(counts), L.ptr(work_f))

    t_comp = median_us(comp, calls)
    n_comp, n_faced, largest = stats.tolist()
    print(f"{name}: {V} vertices, {F} triangles, {n_comp} components, {n_faced} with a face, the largest {largest} triangles")
    groups_v, groups = -(-V // 256), -(-max(V, F) // 256)
    # components: labels and counts written by init, every face read by hook and count, labels rewritten by flatten and read by count
    # (one per face) and stats, counts read by stats, the partials out and in
    b_comp = 8 * V + 2 * 12 * F + 8 * V + 4 * F + 8 * V + 2 * 24 * groups_v
    print(f"  tn_mesh_components (6 launches):        {fmt(t_comp)};  {b_comp} B by the definition = {b_comp / 6.3e12 * 1e6:.2f} us at 6.3 TB/s")
    for T, what in ((0, "threshold 0: everything kept"), (largest, f"threshold {largest}: the largest alone")):
        filt(T, 0, 0)
        kv, kf = counts.tolist()
        t_count = median_us(lambda: filt(T, 0, 0), calls)
        t_vert = median_us(lambda: filt(T, kv, 0), calls)
        t_all = median_us(lambda: filt(T, kv, kf), calls)
        # mark: a label and its count per vertex, 3 ids + a label + its count per face, ballots and counts out; scan: both columns in and
        # out; vertices: ballots + offsets in, the map out, per kept vertex 27 B in and 31 B out; faces: ballots + offsets, per kept face
        # 12 B of ids, 12 B of map entries, 12 B out
        moved = {"mark": 8 * V + 20 * F + 80 * groups, "scan": 32 * groups + 16, "vertices": 24 * groups_v + 4 * V + 58 * kv,
                 "faces": 24 * -(-F // 256) + 36 * kf}
        total = sum(moved.values())
        print(f"  tn_mesh_filter, {what}: {kv} vertices, {kf} triangles kept")
        print(f"    mark + scan (count-only call):        {fmt(t_count)}")
        print(f"    + vertices:                           {fmt(t_vert)}  -> vertex launch {t_vert[0] - t_count[0]:.1f} us")
        print(f"    + faces (all four launches):          {fmt(t_all)}  -> face launch {t_all[0] - t_vert[0]:.1f} us")
        print("    bytes by the definition: " + ", ".join(f"{k} {b}" for k, b in moved.items()) + f"; all four {total} B = {total / 6.3e12 * 1e6:.2f} us at 6.3 TB/s")
    whole = median_us(lambda: M.filter_components(vert, nrm, rgb, faces, keep_fraction=1.0), 3)
    print(f"  mesh.filter_components(keep_fraction=1.0), allocations and both read-backs included: {whole[0]:.0f} us (median of 3)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--triangles", type=int, default=1000000, help="disjoint triangles of the many-components case")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    o, d, rgb, _, _ = rays.synthetic_scene(n_views=4, res=200, seed=0, device=dev)
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
    colours = M.vertex_colors(tr, vert, nrm)
    time_mesh(f"K-Planes, {args.steps} steps, resolution {args.resolution}", vert, nrm, colours, faces, args.calls)
    del values
    n = args.triangles
    g = torch.Generator(device="cpu").manual_seed(0)
    tri = torch.randperm(3 * n, generator=g).to(torch.int32).view(n, 3)[torch.randperm(n, generator=g)].contiguous().to(dev)
    xyz = torch.randn((3 * n, 3), generator=g).to(dev)
    time_mesh("disjoint triangles, ids and faces shuffled", xyz, xyz.flip(0).contiguous(), torch.zeros((3 * n, 3), dtype=torch.uint8, device=dev), tri,
              args.calls)


if __name__ == "__main__":
    main()
