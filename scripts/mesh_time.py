#!/usr/bin/env python3
"""Time the mesh export on a K-Planes model trained for a few steps: the density query at the grid nodes, the launches of
tn_mesh_extract and the whole export.

    python scripts/mesh_time.py [--resolution 256] [--steps 50] [--calls 7]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 scripts/mesh_time.py      (kernel times, a run of its own)

HIP events, median of --calls, allocations outside the window.  tn_mesh_extract enqueues its launches itself, so the events go
around its three call forms -- counts only (mark + scan), vertices without faces (+ the vertex launch), everything (+ the face
launch) -- and the vertex and face launches are the differences; the kernel trace above times each kernel alone.  Also printed: the
bytes every launch moves by the definition and what they take at 6.3 TB/s, and the whole export_mesh on the host clock."""
import argparse
import ctypes as C
import math
import os
import sys
import time

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--calls", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    o, d, rgb, _, _ = rays.synthetic_scene(n_views=4, res=200, seed=0, device=dev)
    tr = Trainer(TrainConfig(method="kplanes", batch_size=4096, seed=0), o, d, rgb, torch.ones(3, device=dev), dev)
    for _ in range(args.steps):
        tr.step()
    torch.cuda.synchronize()
    crop = default_crop(tr.cfg)
    lo, h, dims = M.grid_dims(crop, args.resolution)
    nodes = (dims[0] + 1) * (dims[1] + 1) * (dims[2] + 1)
    cells = dims[0] * dims[1] * dims[2]
    level = math.log(M.default_level(h))

    q = median_us(lambda: M.density_grid(tr, crop, dims), args.calls)
    print(f"density query, {nodes} nodes ({dims[0]} x {dims[1]} x {dims[2]} cells): {q[0]:.0f} us (median of {args.calls}; {q[1]:.0f} - {q[2]:.0f})")
    values = M.density_grid(tr, crop, dims)[0]
    lo_c, h_c, dims_c = M._grid(lo, h, dims)
    nbytes = C.c_int64(0)
    L.call_plain("tn_mesh_workspace_bytes", dims_c[0], dims_c[1], dims_c[2], C.byref(nbytes))
    work = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)

    def call(vcap, fcap, vert=None, nrm=None, faces=None):
        L.call("tn_mesh_extract", dev, L.ptr(values), dims_c, lo_c, h_c, C.c_float(level), C.c_int64(vcap), C.c_int64(fcap), L.ptr(vert), L.ptr(nrm),
               L.ptr(faces), L.ptr(counts), L.ptr(work))

    call(0, 0)
    V, F = counts.tolist()
    if V == 0:
        # a model this young has no surface at the default level: take the density 1 node in 200 exceeds, so that launches 3 and 4 have work
        level = float(values.flatten().kthvalue(int(0.995 * values.numel())).values)
        print(f"no surface at the default level sigma = {M.default_level(h):.2f}: timing at the 99.5th percentile of the node densities instead")
        call(0, 0)
        V, F = counts.tolist()
    vert, nrm = torch.empty((max(V, 1), 3), device=dev), torch.empty((max(V, 1), 3), device=dev)
    faces = torch.empty((max(F, 1), 3), dtype=torch.int32, device=dev)
    t_count = median_us(lambda: call(0, 0), args.calls)
    t_vert = median_us(lambda: call(V, 0, vert, nrm), args.calls)
    t_all = median_us(lambda: call(V, F, vert, nrm, faces), args.calls)
    groups = -(-cells // 256)
    # mark: every node value once, 4 x 4 ballots + 2 counts per workgroup out; scan: both count columns in and out; vertices: the
    # active ballots + offset per workgroup, an id per cell out, per vertex 8 corner values in and 2 rows out; faces: the quad
    # ballots + offset per workgroup, per quad the lower node's value and 4 ids in, 2 rows out
    moved = {"mark": 4 * nodes + 144 * groups, "scan": 32 * groups + 16, "vertices": 40 * groups + 4 * cells + V * (32 + 24),
             "faces": 104 * groups + F // 2 * (4 + 16 + 24)}
    print(f"{V} vertices, {F} triangles at sigma = {math.exp(level):.2f}")
    print(f"mark + scan (count-only call):  {t_count[0]:.1f} us ({t_count[1]:.1f} - {t_count[2]:.1f})")
    print(f"+ vertices:                     {t_vert[0]:.1f} us ({t_vert[1]:.1f} - {t_vert[2]:.1f})  -> vertex launch {t_vert[0] - t_count[0]:.1f} us")
    print(f"+ faces (all four launches):    {t_all[0]:.1f} us ({t_all[1]:.1f} - {t_all[2]:.1f})  -> face launch {t_all[0] - t_vert[0]:.1f} us")
    for name, b in moved.items():
        print(f"  {name:9s} moves {b} B by the definition = {b / 6.3e12 * 1e6:.2f} us at 6.3 TB/s")
    print(f"  all four: {sum(moved.values())} B = {sum(moved.values()) / 6.3e12 * 1e6:.2f} us at 6.3 TB/s")
    whole = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        M.export_mesh(tr, None, resolution=args.resolution)
        torch.cuda.synchronize()
        whole.append(time.perf_counter() - t0)
    print(f"export_mesh (query + extract + colours, no file), host clock: {sorted(whole)[1] * 1e3:.1f} ms (median of 3)")


if __name__ == "__main__":
    main()
