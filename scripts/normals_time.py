#!/usr/bin/env python3
"""Time the surface-normal pass on one view: a K-Planes and a hash-grid model, a size x size view in 2^16-ray chunks,
rendered with and without `normals`.

    python scripts/normals_time.py [--size 800] [--n_samples 256] [--repeats 7] [--steps 50]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 scripts/normals_time.py --repeats 2   (kernel times, a run of its own)

Per method it prints: the whole-image time of Trainer.render_rays(maps=True) and of (maps=True, normals=True), alternated, median of
`repeats` after a warm-up of both, a host clock around work that ends in a device synchronise, and their ratio; and the HIP-event time
of the two launches of the pass alone (tn_*_normals gated by the weights, tn_ray_normals) on the view's first chunk, with its sample
count, the share of samples with a non-zero weight and of 32-row tiles that are evaluated.  The model is trained for `steps` steps on
the synthetic ball first, so that the occupancy grid and the weights look like a scene's and not like noise."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tinynerf_amd import core, rays  # noqa: E402
from tinynerf_amd.run import TrainConfig, Trainer  # noqa: E402


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--n_samples", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--methods", nargs="+", default=["kplanes", "hashgrid"])
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    o, d, rgb, _, _ = rays.synthetic_scene(n_views=4, res=200, seed=0, device=dev)
    vo, vd, _, _, _ = rays.synthetic_scene(n_views=1, res=args.size, seed=1, device=dev, with_colors=False)
    for method in args.methods:
        cfg = TrainConfig(method=method, batch_size=4096, n_samples=args.n_samples, seed=0)
        tr = Trainer(cfg, o, d, rgb, torch.ones(3, device=dev), dev)
        for _ in range(args.steps):
            tr.step()
        torch.cuda.synchronize()

        def image(normals):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = tr.render_rays(vo, vd, 1 << 16, maps=True, normals=True) if normals else tr.render_rays(vo, vd, 1 << 16, maps=True)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, out

        for flag in (False, True):
            image(flag)
        plain, full = [], []
        for _ in range(args.repeats):
            plain.append(image(False)[0])
            full.append(image(True)[0])
        a, b = median(plain), median(full)
        print(f"{method}: {args.size} x {args.size} view, S = {args.n_samples}: maps {a:.2f} ms ({min(plain):.2f} - {max(plain):.2f}), "
              f"maps + normals {b:.2f} ms ({min(full):.2f} - {max(full):.2f}), ratio {b / a:.3f} (median of {args.repeats}, alternated)")
        # the pass alone on the first chunk
        packed, info, t = tr.ray_provider(vo[:1 << 16], vd[:1 << 16], training=False, return_t=True)
        stats = tr.renderer.__dict__.setdefault("_stats", {})
        handout = {}
        stats["maps_handout"] = handout
        with torch.no_grad():
            tr.renderer(packed, info)
        stats.pop("maps_handout", None)
        w = handout["weights"].detach()
        n = packed.size(0)
        live = float((w != 0).float().mean()) if n else 0.0
        pad = (-n) % 32
        tiles = torch.nn.functional.pad((w != 0), (0, pad)).reshape(-1, 32).any(1).float().mean().item() if n else 0.0
        times = [[], []]
        for k in range(5 + args.repeats * 3):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            sn = core.sample_normals(tr.renderer, packed, gate=w)
            ev[1].record()
            core.ray_normals(w, sn, info)
            ev[2].record()
            ev[2].synchronize()
            if k >= 5:
                times[0].append(ev[0].elapsed_time(ev[1]) * 1e3)
                times[1].append(ev[1].elapsed_time(ev[2]) * 1e3)
        print(f"{method}: first chunk, {n} samples of {1 << 16} rays, {100 * live:.1f} % with w != 0, {100 * tiles:.1f} % of the tiles evaluated: "
              f"sample normals {median(times[0]):.1f} us ({min(times[0]):.1f} - {max(times[0]):.1f}, allocation of the output included), "
              f"ray normals {median(times[1]):.1f} us ({min(times[1]):.1f} - {max(times[1]):.1f})")


if __name__ == "__main__":
    main()
