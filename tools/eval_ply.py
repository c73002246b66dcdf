#!/usr/bin/env python3
"""Accuracy, completeness and F1 of a fused cloud against a ground-truth scan at a list of distance tolerances, on the GPU
(mp-mvs_amd/cloud.py: evaluate).

    python tools/eval_ply.py --reconstruction MPMVS_model.ply --ground_truth scan.ply [--tolerances 0.01,0.02,0.05,0.1,0.2,0.5]
                             [--transform T.txt] [--crop xmin,ymin,zmin,xmax,ymax,zmax] [--voxel V] [--device 0]
                             [--refine [--refine_radii r1,r2,...] [--refine_no_scale] [--refine_iters 30] [--save_transform OUT.txt]]

--transform: a 4 x 4 text matrix that takes the reconstruction into the ground truth's frame; applied in fp64 and rounded to
fp32.  --crop: an axis-aligned box (in the ground truth's frame, after the transform) applied to both clouds.
--refine: the transform (identity if absent) is only a starting guess and is refined before the score, as the Tanks and Temples
protocol does: point-to-point ICP of the reconstruction to the ground truth on the GPU (mp-mvs_amd/cloud.py: align; DESIGN.md
section 15), one round per radius of --refine_radii in descending order (default: 8, 4 and 2 times the largest tolerance), with
a scale unless --refine_no_scale, at most --refine_iters passes per round.  The crop is applied after the refined transform,
and the JSON line gains "refine": {"rounds": [{radius, passes, inliers, rmse}], "matrix": 4 x 4, "seconds"}.
--save_transform writes the refined 4 x 4 matrix as text: a later run's --transform (tools/eval_depth.py takes its inverse: there
the matrix carries the scan into the cameras' frame).
--voxel V: both clouds are resampled on a voxel grid of edge V on the GPU (mp-mvs_amd/cloud.py: voxel_downsample; DESIGN.md
section 16) before they are registered and measured, so that a surface does not count by how densely it was sampled; Tanks and
Temples uses half its tolerance.  The order is then: --transform, --crop, the resampling of both clouds, --refine on the resampled
clouds (starting from the identity; the matrix reported and saved is the refined one times --transform), the score.  The JSON
line gains "voxel", the point counts before the resampling ("n_reconstruction_in", "n_ground_truth_in"; "n_reconstruction" and
"n_ground_truth" are the counts after it) and the seconds it took.
This is the plain two-way nearest-neighbour measure (Tanks-and-Temples style); ETH3D's official program additionally masks
unobserved space, which is not available here, so the numbers compare our own builds and settings, not leaderboard entries.
Prints one JSON line: the dictionary of evaluate() plus seconds per stage (read, upload + build, query)."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401,E402

cloud = importlib.import_module("mp-mvs_amd.cloud")


def apply_transform(xyz, T):
    T = np.asarray(T, np.float64)
    if T.shape != (4, 4) or not np.isfinite(T).all():
        raise ValueError(f"--transform needs a finite 4 x 4 matrix, got shape {T.shape}")
    p = xyz.astype(np.float64)
    h = p @ T[:3, :3].T + T[:3, 3]
    w = p @ T[3, :3] + T[3, 3]
    return (h / w[:, None]).astype(np.float32)


def crop(xyz, box):
    lo, hi = np.asarray(box[:3], np.float32), np.asarray(box[3:], np.float32)
    with np.errstate(invalid="ignore"):
        keep = ((xyz >= lo) & (xyz <= hi)).all(1) | ~np.isfinite(xyz).all(1)   # non-finite points stay, to be counted by evaluate
    return xyz[keep]


def main_voxel(args, tol):
    """the run with --voxel: transform, crop, resample both clouds, refine on the resampled clouds, score"""
    t0 = time.perf_counter()
    rec = cloud.read_ply(args.reconstruction)["xyz"]
    gt = cloud.read_ply(args.ground_truth)["xyz"]
    T0 = np.loadtxt(args.transform) if args.transform else np.eye(4)
    if args.transform:
        rec = apply_transform(rec, T0)
    if args.crop:
        box = [float(v) for v in args.crop.split(",")]
        if len(box) != 6:
            raise SystemExit("--crop needs xmin,ymin,zmin,xmax,ymax,zmax")
        rec, gt = crop(rec, box), crop(gt, box)
    t1 = time.perf_counter()
    rec, drop_r = cloud.drop_nonfinite(rec)
    gt, drop_g = cloud.drop_nonfinite(gt)
    n_in = (len(rec), len(gt))
    rec = cloud.voxel_downsample(rec, args.voxel, device=args.device)["xyz"]
    gt = cloud.voxel_downsample(gt, args.voxel, device=args.device)["xyz"]
    t2 = time.perf_counter()
    refine = None
    if args.refine:
        radii = [float(r) for r in args.refine_radii.split(",") if r.strip()] if args.refine_radii else [8 * max(tol), 4 * max(tol), 2 * max(tol)]
        with cloud.Cloud(gt, args.device) as c_gt:
            T, rounds = cloud.align(rec, c_gt, None, radii=radii, with_scale=not args.refine_no_scale, max_iter=args.refine_iters)
        rec = apply_transform(rec, T)
        T = T @ np.asarray(T0, np.float64)
        refine = {"rounds": rounds, "matrix": T.tolist(), "seconds": round(time.perf_counter() - t2, 4)}
        if args.save_transform:
            np.savetxt(args.save_transform, T, fmt="%.17g")
    timings = {}
    res = cloud.evaluate(rec, gt, tol, device=args.device, timings=timings)
    res["dropped_reconstruction"], res["dropped_ground_truth"] = drop_r, drop_g
    res["voxel"], res["n_reconstruction_in"], res["n_ground_truth_in"] = float(args.voxel), n_in[0], n_in[1]
    res["seconds"] = {"read": round(t1 - t0, 4), "voxel": round(t2 - t1, 4), "upload_build": round(timings["upload_build_s"], 4),
                      "query": round(timings["query_s"], 4)}
    if refine is not None:
        res["refine"] = refine
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reconstruction", required=True)
    ap.add_argument("--ground_truth", required=True)
    ap.add_argument("--tolerances", default="0.01,0.02,0.05,0.1,0.2,0.5")
    ap.add_argument("--transform")
    ap.add_argument("--crop")
    ap.add_argument("--voxel", type=float, help="resample both clouds on a voxel grid of this edge before --refine and the score "
                    "(Tanks and Temples uses half its tolerance)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--refine", action="store_true")
    ap.add_argument("--refine_radii")
    ap.add_argument("--refine_no_scale", action="store_true")
    ap.add_argument("--refine_iters", type=int, default=30)
    ap.add_argument("--save_transform")
    args = ap.parse_args()
    if not args.refine and (args.refine_radii or args.refine_no_scale or args.save_transform):
        raise SystemExit("--refine_radii, --refine_no_scale and --save_transform need --refine")
    if args.voxel is not None and not (np.isfinite(args.voxel) and args.voxel > 0):
        raise SystemExit("--voxel needs a finite positive edge length")
    tol = [float(t) for t in args.tolerances.split(",") if t.strip()]
    if args.voxel is not None:
        return main_voxel(args, tol)
    t0 = time.perf_counter()
    rec = cloud.read_ply(args.reconstruction)["xyz"]
    gt = cloud.read_ply(args.ground_truth)["xyz"]
    refine = None
    if args.refine:
        T0 = np.loadtxt(args.transform) if args.transform else np.eye(4)
        radii = [float(r) for r in args.refine_radii.split(",") if r.strip()] if args.refine_radii else [8 * max(tol), 4 * max(tol), 2 * max(tol)]
        t_r = time.perf_counter()
        with cloud.Cloud(cloud.drop_nonfinite(gt)[0], args.device) as c_gt:
            T, rounds = cloud.align(rec, c_gt, T0, radii=radii, with_scale=not args.refine_no_scale, max_iter=args.refine_iters)
        refine = {"rounds": rounds, "matrix": T.tolist(), "seconds": round(time.perf_counter() - t_r, 4)}
        if args.save_transform:
            np.savetxt(args.save_transform, T, fmt="%.17g")
        rec = apply_transform(rec, T)
    elif args.transform:
        rec = apply_transform(rec, np.loadtxt(args.transform))
    if args.crop:
        box = [float(v) for v in args.crop.split(",")]
        if len(box) != 6:
            raise SystemExit("--crop needs xmin,ymin,zmin,xmax,ymax,zmax")
        rec, gt = crop(rec, box), crop(gt, box)
    t1 = time.perf_counter()
    timings = {}
    res = cloud.evaluate(rec, gt, tol, device=args.device, timings=timings)
    res["seconds"] = {"read": round(t1 - t0, 4), "upload_build": round(timings["upload_build_s"], 4), "query": round(timings["query_s"], 4)}
    if refine is not None:
        res["refine"] = refine
    print(json.dumps(res))


if __name__ == "__main__":
    main()
