#!/usr/bin/env python3
"""Command line of the reference (train.py:8-46) on the MI355X hot path.

    python train.py --data data/lego --datatype synthetic --output out --method kplanes \\
                    --batch_size 1024 --n_samples 1024 --scene_type aabb
    python train.py --data captures/garden --datatype nerfstudio --output out --method kplanes \\
                    --scene_type unbounded --downscale 4
"""
import argparse
import os
import random
import uuid
from pathlib import Path

# (flag, keyword arguments) -- same names, defaults and choices as the reference's parser, plus --max_steps, --render_maps, --distortion_weight, --ssim,
# --downscale, --holdout_every, --export_pointcloud, --pointcloud_crop, --normals, --export_mesh, --mesh_level, --mesh_crop, --mesh_min_faces, --mesh_keep_fraction,
# --export_tsdf_mesh, --tsdf_trunc, --tsdf_colors and --mesh_smooth
FLAGS = (
    ("--data", dict(type=str, required=True, help="path to the data folder")),
    ("--datatype", dict(type=str, required=True, choices=["synthetic", "nerfstudio"])),
    ("--output", dict(type=str, required=True, help="path to the output folder")),
    ("--method", dict(type=str, required=True, choices=["vanilla", "kplanes", "cobafa", "hashgrid"])),
    ("--scene_type", dict(type=str, default="aabb", choices=["aabb", "unbounded"])),
    ("--batch_size", dict(type=int, default=2048)),
    ("--n_samples", dict(type=int, default=400, help="number of samples per ray")),
    ("--eval", dict(action="store_true")),
    ("--eval_every", dict(type=int, default=None, help="number of train steps between evaluations")),
    ("--eval_n", dict(type=int, default=1, help="number of images to evaluate on")),
    ("--max_steps", dict(type=int, default=None, help="stop early (the recipe's step count is 2048*4096/batch_size)")),
    ("--render_maps", dict(action="store_true", help="the final test render also writes depth / opacity maps")),
    ("--distortion_weight", dict(type=float, default=0.0, help="weight of the Mip-NeRF 360 distortion loss (0: off; 1e-3 .. 1e-2 is usual)")),
    ("--ssim", dict(action="store_true", help="metrics_eval.json / metrics_test.json also carry each image's SSIM (else 0.0)")),
    ("--downscale", dict(type=int, default=1, help="nerfstudio: load the images N times smaller (images_N/ if present, else box-filtered)")),
    ("--holdout_every", dict(type=int, default=8, help="nerfstudio captures without split lists: every N-th frame is val / test")),
    ("--export_pointcloud", dict(type=int, default=0, metavar="N", help="write pointcloud.ply: at most N coloured surface points of the test views (0: off)")),
    ("--pointcloud_crop", dict(type=float, nargs=6, default=None, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"),
                               help="box the exported points must lie in (default: the box the marcher samples uniformly)")),
    ("--normals", dict(action="store_true", help="kplanes / hashgrid: the final test render also writes normal maps (implies --render_maps) "
                                                 "and pointcloud.ply carries normals")),
    ("--export_mesh", dict(type=int, default=0, metavar="R", help="write mesh.ply: the density's surface as a triangle mesh, R cells on the longest axis of the box (0: off)")),
    ("--mesh_level", dict(type=float, default=None, metavar="SIGMA", help="density of the exported surface (default: ln 2 / cell size, opacity 0.5 across a cell)")),
    ("--mesh_crop", dict(type=float, nargs=6, default=None, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"),
                         help="box the mesh is extracted in (default: the box the marcher samples uniformly)")),
    ("--mesh_min_faces", dict(type=int, default=0, metavar="N", help="with --export_mesh: drop the connected pieces of the mesh with fewer than N triangles (0: keep all)")),
    ("--mesh_keep_fraction", dict(type=float, default=0.0, metavar="F", help="with --export_mesh: drop the pieces with fewer than F x the largest piece's triangles "
                                                                               "(1.0: the largest piece alone; 0: keep all)")),
    ("--export_tsdf_mesh", dict(type=int, default=0, metavar="R", help="write tsdf_mesh.ply: the test views' depth maps fused into a truncated signed distance "
                                                                        "field, its zero level as a triangle mesh, R cells on the longest axis of the box (0: off); "
                                                                        "--mesh_crop, --mesh_min_faces and --mesh_keep_fraction apply to it too")),
    ("--tsdf_trunc", dict(type=float, default=None, metavar="T", help="with --export_tsdf_mesh: the truncation distance (default: 4 cells)")),
    ("--tsdf_colors", dict(type=str, default="decoder", choices=["decoder", "fused"],
                           help="with --export_tsdf_mesh: vertex colours from the colour decoder at the vertex, or fused from the test views' renders")),
    ("--mesh_smooth", dict(type=int, default=0, metavar="N", help="with --export_mesh / --export_tsdf_mesh: N Taubin smoothing iterations over the mesh before it is "
                                                                  "written, its normals recomputed from the smoothed faces (0: off)")),
)


def parse_args(argv=None):
    parser = argparse.ArgumentParser(prog="tinynerf", description="Train nerf (MI355X HIP path)")
    for flag, kw in FLAGS:
        parser.add_argument(flag, **kw)
    args = parser.parse_args(argv)
    if args.normals and args.method not in ("kplanes", "hashgrid"):
        parser.error(f"--normals needs --method kplanes or hashgrid: {args.method} has no analytic density gradient")
    if (args.mesh_min_faces or args.mesh_keep_fraction) and not (args.export_mesh or args.export_tsdf_mesh):
        parser.error("--mesh_min_faces and --mesh_keep_fraction filter the mesh of --export_mesh R or --export_tsdf_mesh R: give one of them too")
    if args.mesh_min_faces < 0 or not 0.0 <= args.mesh_keep_fraction <= 1.0:
        parser.error("--mesh_min_faces must be >= 0 and --mesh_keep_fraction lie in [0, 1]")
    if args.tsdf_trunc is not None and not args.export_tsdf_mesh:
        parser.error("--tsdf_trunc is the truncation of --export_tsdf_mesh R: give that too")
    if args.tsdf_colors == "fused" and not args.export_tsdf_mesh:
        parser.error("--tsdf_colors fused colours the mesh of --export_tsdf_mesh R: give that too")
    if args.export_tsdf_mesh < 0 or (args.tsdf_trunc is not None and not 0.0 < args.tsdf_trunc < float("inf")):
        parser.error("--export_tsdf_mesh must be >= 0 and --tsdf_trunc finite and > 0")
    if args.mesh_smooth < 0:
        parser.error("--mesh_smooth must be >= 0")
    if args.mesh_smooth and not (args.export_mesh or args.export_tsdf_mesh):
        parser.error("--mesh_smooth smooths the mesh of --export_mesh R or --export_tsdf_mesh R: give one of them too")
    return args


def fresh_run_dir(root: Path, args) -> Path:
    """<output>/<8 hex>_<method>_<scene_type>_<n_samples>, never an existing directory (train.py:36-41)."""
    for _ in range(1000):
        candidate = root / f"{uuid.uuid4().hex[:8]}_{args.method}_{args.scene_type}_{args.n_samples}"
        if not candidate.is_dir():
            candidate.mkdir(parents=True)
            return candidate
    raise RuntimeError("could not find a free experiment directory")


def load_split(data, root: Path, split: str, device, rays: bool):
    if not (root / f"transforms_{split}.json").exists():
        return None
    scene = data.parse_nerf_synthetic(root, split)
    return data.RaysDataset(scene, device) if rays else data.PoseDataset(scene, device)


def load_datasets(args, device):
    """args -> (train rays, eval set, test set); host work only (files, poses, uploads): no kernel runs here.  A synthetic scene becomes
    ray tables (RaysDataset / PoseDataset), a nerfstudio capture camera tables (CameraRaysDataset / CameraPoseDataset)."""
    from tinynerf_amd import data
    root = Path(args.data)
    if args.datatype == "synthetic":
        train_rays = load_split(data, root, "train", device, rays=True)
        if train_rays is None:
            raise FileNotFoundError(root / "transforms_train.json")
        return train_rays, load_split(data, root, "val", device, rays=False), load_split(data, root, "test", device, rays=False)
    if args.datatype == "nerfstudio":
        def split(name):
            return data.parse_nerfstudio(root, name, downscale=args.downscale, holdout_every=args.holdout_every)
        return (data.CameraRaysDataset(split("train"), device), data.CameraPoseDataset(split("val"), device),
                data.CameraPoseDataset(split("test"), device))
    raise NotImplementedError(args.datatype)


def main(argv=None):
    args = parse_args(argv)

    import numpy as np
    import torch
    from tinynerf_amd.run import TrainConfig, train

    seed = int(os.environ.get("SEED", 0))
    if seed:
        for seeder in (torch.manual_seed, np.random.seed, random.seed):
            seeder(seed)
    device = torch.device("cuda")
    train_rays, eval_set, test_set = load_datasets(args, device)
    run_dir = fresh_run_dir(Path(args.output), args)
    print(f"Experiment saved to {run_dir}")
    cfg = TrainConfig(method=args.method, scene_type=args.scene_type, batch_size=args.batch_size, n_samples=args.n_samples, seed=seed,
                      distortion_weight=args.distortion_weight)
    train(cfg, train_rays, eval_set, test_set, run_dir, args.eval_every, args.eval_n, args.max_steps, render_maps=args.render_maps, ssim=args.ssim,
          pointcloud=args.export_pointcloud, pointcloud_crop=args.pointcloud_crop, normals=args.normals,
          mesh=args.export_mesh, mesh_level=args.mesh_level, mesh_crop=args.mesh_crop, mesh_min_faces=args.mesh_min_faces,
          mesh_keep_fraction=args.mesh_keep_fraction, tsdf_mesh=args.export_tsdf_mesh, tsdf_trunc=args.tsdf_trunc,
          tsdf_colors=args.tsdf_colors, mesh_smooth=args.mesh_smooth)


if __name__ == "__main__":
    main()
