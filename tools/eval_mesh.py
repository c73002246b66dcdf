#!/usr/bin/env python3
"""Score a triangle mesh PLY as a surface on the GPU: against a ground-truth scan, or against another mesh (mp-mvs_amd/mesh.py:
evaluate_mesh, compare; csrc/pm_surface.hpp).

    python tools/eval_mesh.py --mesh M.ply --ground_truth scan.ply [--tolerances t1,t2,...] [--spacing S] [--voxel V] [--transform T.txt]
    python tools/eval_mesh.py --mesh M.ply --reference_mesh R.ply --radius R [--spacing S]

With --ground_truth: accuracy is the share of the mesh's surface samples within each tolerance of the scan, completeness the share of
the scan's points within it of the mesh's SURFACE (point-to-triangle distance, not the vertices); the keys are those of
tools/eval_ply.py.  --spacing is the distance of the samples (default: the smallest tolerance, so that no point of the surface is
farther than two thirds of it from a sample; an untuned starting value); --voxel resamples the samples on a voxel grid first;
--transform is a 4 x 4 text matrix that takes the mesh into the scan's frame, applied in fp64 and rounded to fp32.
With --reference_mesh: the samples of each mesh against the surface of the other within --radius: per direction n, beyond, max, mean
and rms, and the capped Hausdorff distance; this is what says how far tools/simplify_mesh.py moved a surface.  --spacing defaults to
half the radius there (untuned).
Prints one JSON line: the score or the comparison, device ms and wall seconds per stage."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _positive(name, v):
    if not (v > 0.0 and v < float("inf")):
        raise SystemExit(f"{name} must be finite and positive")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mesh", required=True)
    ap.add_argument("--ground_truth", help="a point cloud PLY: score the mesh against it")
    ap.add_argument("--reference_mesh", help="a mesh PLY: compare the two surfaces")
    ap.add_argument("--tolerances", default="0.01,0.02,0.05,0.1,0.2,0.5")
    ap.add_argument("--radius", type=float, help="with --reference_mesh: the cap of the distances")
    ap.add_argument("--spacing", type=float, help="distance of the surface samples (default: the smallest tolerance, or half the radius; untuned starting values)")
    ap.add_argument("--voxel", type=float, help="with --ground_truth: resample the mesh's samples on a voxel grid of this edge first")
    ap.add_argument("--transform", help="with --ground_truth: 4 x 4 text matrix that takes the mesh into the scan's frame")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    if (args.ground_truth is None) == (args.reference_mesh is None):
        raise SystemExit("give either --ground_truth or --reference_mesh")
    if args.reference_mesh is not None:
        if args.radius is None:
            raise SystemExit("--reference_mesh needs --radius")
        _positive("--radius", args.radius)
        if args.voxel is not None or args.transform is not None:
            raise SystemExit("--voxel and --transform belong to --ground_truth")
        args.tolerances = None
    else:
        if args.radius is not None:
            raise SystemExit("--radius belongs to --reference_mesh")
        try:
            args.tolerances = [float(t) for t in args.tolerances.split(",")]
        except ValueError:
            raise SystemExit("--tolerances needs numbers separated by commas") from None
        for t in args.tolerances:
            _positive("every tolerance", t)
    for name in ("spacing", "voxel"):
        if getattr(args, name) is not None:
            _positive("--" + name, getattr(args, name))
    if args.spacing is None:
        args.spacing = min(args.tolerances) if args.tolerances else 0.5 * args.radius
    return args


def load(args):
    """(the mesh, the scan's points or the reference mesh, the head of the result line); no device is touched"""
    mesh = importlib.import_module("mp-mvs_amd.mesh")
    cloud = importlib.import_module("mp-mvs_amd.cloud")
    try:
        m = mesh.read_ply_mesh(args.mesh)
        if args.transform:
            T = np.asarray(np.loadtxt(args.transform), np.float64)
            if T.shape != (4, 4) or not np.isfinite(T).all():
                raise ValueError(f"--transform needs a finite 4 x 4 matrix, got shape {T.shape}")
            m["xyz"] = (m["xyz"].astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
        other = cloud.read_ply(args.ground_truth)["xyz"] if args.ground_truth else mesh.read_ply_mesh(args.reference_mesh)
    except (ValueError, OSError) as e:
        raise SystemExit(str(e)) from None
    head = {"mesh": args.mesh, "n": int(len(m["xyz"])), "m": int(len(m["tri"])), "spacing": args.spacing}
    head.update({"ground_truth": args.ground_truth, "tolerances": args.tolerances} if args.ground_truth else {"reference_mesh": args.reference_mesh, "radius": args.radius})
    return m, other, head


def main(argv=None):
    args = parse_args(argv)
    import torch  # noqa: F401  (the HIP runtime torch bundles, before our library: engine.load)
    mesh = importlib.import_module("mp-mvs_amd.mesh")
    t0 = time.perf_counter()
    m, other, res = load(args)
    t1 = time.perf_counter()
    try:
        if args.ground_truth:
            timings = {}
            res["score"] = mesh.evaluate_mesh(m, other, args.tolerances, spacing=args.spacing, voxel=args.voxel, device=args.device, timings=timings)
            res["device_ms"] = {k: round(v, 4) for k, v in timings.pop("device_ms").items()}
            res["seconds"] = {k: round(v, 4) for k, v in timings.items()}
        else:
            res["comparison"] = mesh.compare(m, other, args.spacing, args.radius, device=args.device)
            res["seconds"] = {}
    except (ValueError, OSError, RuntimeError) as e:
        raise SystemExit(str(e)) from None
    t2 = time.perf_counter()
    res["seconds"].update(read=round(t1 - t0, 4), wall=round(t2 - t0, 4))
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
