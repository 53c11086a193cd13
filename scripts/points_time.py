#!/usr/bin/env python3
"""Time tn_points_compact on one view: H x W rays looking at a sphere, `keep` of them with opacity above the bound.

    python scripts/points_time.py [--size 800] [--keep 0.5] [--calls 40]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 scripts/points_time.py      (kernel times, a run of its own)

Prints the HIP-event time per call (three launches, allocations outside the window) and the bytes the definition moves: 44 B in per
ray, 19 B out per kept ray."""
import argparse
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tinynerf_amd import _lib as L  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--keep", type=float, default=0.5)
    ap.add_argument("--calls", type=int, default=40)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = args.size * args.size
    gen = torch.Generator(device=dev).manual_seed(0)
    d = torch.nn.functional.normalize(torch.randn(n, 3, device=dev, generator=gen), dim=-1)
    o = -3.0 * d + 0.1 * torch.randn(n, 3, device=dev, generator=gen)
    depth = 2.0 + torch.rand(n, device=dev, generator=gen)
    opacity = torch.where(torch.rand(n, device=dev, generator=gen) < args.keep, 0.9, 0.1) * torch.ones(n, device=dev)
    rgb = torch.rand(n, 3, device=dev, generator=gen)
    bg = torch.ones(3, device=dev)
    box = torch.tensor([-1.5] * 3 + [1.5] * 3, device=dev)
    nbytes = C.c_int64(0)
    L.call_plain("tn_points_workspace_bytes", C.c_int64(n), C.byref(nbytes))
    work = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    points = torch.empty((n, 3), device=dev)
    colors = torch.empty((n, 3), dtype=torch.uint8, device=dev)
    src = torch.empty(n, dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)

    def call():
        L.call("tn_points_compact", dev, L.ptr(o), L.ptr(d), L.ptr(rgb), L.ptr(opacity), L.ptr(depth), L.ptr(bg), L.ptr(box), C.c_float(0.5),
               C.c_int64(n), C.c_int64(n), L.ptr(points), L.ptr(colors), L.ptr(src), L.ptr(count), L.ptr(work))

    for _ in range(5):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    times.sort()
    kept = int(count.item())
    moved = 44 * n + 19 * kept
    print(f"{args.size} x {args.size} = {n} rays, kept {kept}: {times[len(times) // 2]:.1f} us per call (median of {args.calls}; "
          f"{times[0]:.1f} - {times[-1]:.1f}); {moved} B by the definition = {moved / 6.3e12 * 1e6:.2f} us at 6.3 TB/s")


if __name__ == "__main__":
    main()
