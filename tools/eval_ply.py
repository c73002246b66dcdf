#!/usr/bin/env python3
"""Accuracy, completeness and F1 of a fused cloud against a ground-truth scan at a list of distance tolerances, on the GPU
(mp-mvs_amd/cloud.py: evaluate).

    python tools/eval_ply.py --reconstruction MPMVS_model.ply --ground_truth scan.ply [--tolerances 0.01,0.02,0.05,0.1,0.2,0.5]
                             [--transform T.txt] [--crop xmin,ymin,zmin,xmax,ymax,zmax] [--voxel V] [--device 0]
                             [--refine [--refine_radii r1,r2,...] [--refine_no_scale] [--refine_iters 30] [--save_transform OUT.txt]
                                       [--refine_method point|plane [--refine_normal_radius R] [--refine_normal_k 16]]]
                             [--scanners S.txt | --scan_alignment scans.mlp (in place of --ground_truth)]
                             [--face_size 1024] [--window 1] [--free_rel 0.02] [--free_abs 0]

--transform: a 4 x 4 text matrix that takes the reconstruction into the ground truth's frame; applied in fp64 and rounded to
fp32.  --crop: an axis-aligned box (in the ground truth's frame, after the transform) applied to both clouds.
--refine: the transform (identity if absent) is only a starting guess and is refined before the score, as the Tanks and Temples
protocol does: point-to-point ICP of the reconstruction to the ground truth on the GPU (mp-mvs_amd/cloud.py: align; DESIGN.md
section 15), one round per radius of --refine_radii in descending order (default: 8, 4 and 2 times the largest tolerance), with
a scale unless --refine_no_scale, at most --refine_iters passes per round.  The crop is applied after the refined transform,
and the JSON line gains "refine": {"rounds": [{radius, passes, inliers, rmse}], "matrix": 4 x 4, "seconds"}.
--refine_method plane: point-to-plane ICP instead: a pair counts by its distance along the ground truth's
normal, so the reconstruction may slide along a surface that the scan sampled at other points -- the case of every real pair of
clouds, where point-to-point ICP settles about a sample spacing off.  The normals are the ground-truth file's own (nx ny nz) when
it has them and no --refine_normal_radius is given; otherwise they are estimated on the cloud that is registered against (after
--voxel, if given) from the --refine_normal_k nearest neighbours within --refine_normal_radius (mp-mvs_amd/cloud.py:
Cloud.normals).  Its default is the smallest refine radius: an untuned starting value; a good radius holds
a dozen neighbours on one surface.  The rounds gain "rmse_plane" and "refine" gains "method" (also for point) and "normals".  The
default method stays point.
--save_transform writes the refined 4 x 4 matrix as text: a later run's --transform (tools/eval_depth.py takes its inverse: there
the matrix carries the scan into the cameras' frame).
--voxel V: both clouds are resampled on a voxel grid of edge V on the GPU (mp-mvs_amd/cloud.py: voxel_downsample; DESIGN.md
section 16) before they are registered and measured, so that a surface does not count by how densely it was sampled; Tanks and
Temples uses half its tolerance.  The order is then: --transform, --crop, the resampling of both clouds, --refine on the resampled
clouds (starting from the identity; the matrix reported and saved is the refined one times --transform), the score.  The JSON
line gains "voxel", the point counts before the resampling ("n_reconstruction_in", "n_ground_truth_in"; "n_reconstruction" and
"n_ground_truth" are the counts after it) and the seconds it took.
--scanners FILE: the scanner positions of the ground truth, in its frame (they stay there: --transform and --refine move the
reconstruction), as text with one `x y z` per line, `#` starting a comment.  The accuracy is then also given over the space the
scanners observed (mp-mvs_amd/cloud.py: Observer, evaluate(scanners=...)): per scanner a range cube map of
the ground truth with faces of --face_size pixels and a --window minimum; a reconstruction point farther than the tolerance from
the scan counts as wrong only where some scanner saw through it (its range + --free_abs below (1 - --free_rel) x the map's), and
leaves the denominator otherwise.  Every tolerance row gains "n_free_inaccurate", "n_unobserved", "accuracy_observed" and
"f1_observed", the line "observed" and the seconds of it.  The maps come from the ground truth after --crop and before --voxel.
--scan_alignment FILE.mlp instead of --ground_truth: the MeshLab project ETH3D ships with its scans; the ground truth is the union
of the PLYs it lists (read relative to the file), each taken into the common frame by its matrix, and each scan's points count for
its own scanner only, which sits at the scan's origin.  The format is restated from its description: no real ETH3D file has been
read with it here.  --face_size 1024, --window 1, --free_rel 0.02 and --free_abs 0 are starting values, not tuned on a real scan.
The plain keys are the two-way nearest-neighbour measure (Tanks-and-Temples style); ETH3D's official program additionally masks
unobserved space: the observed-space keys do that in our own formulation, not verified against ETH3D's program, so the numbers
compare our own builds and settings, not leaderboard entries.
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


def crop_keep(xyz, box):
    lo, hi = np.asarray(box[:3], np.float32), np.asarray(box[3:], np.float32)
    with np.errstate(invalid="ignore"):
        return ((xyz >= lo) & (xyz <= hi)).all(1) | ~np.isfinite(xyz).all(1)   # non-finite points stay, to be counted by evaluate


def crop(xyz, box):
    return xyz[crop_keep(xyz, box)]


def read_scanners(path):
    """--scanners: a text file with one `x y z` per line, `#` starts a comment -> float32 [m, 3]"""
    rows = []
    with open(path) as f:
        for no, line in enumerate(f, 1):
            w = line.split("#", 1)[0].split()
            if not w:
                continue
            try:
                row = [float(v) for v in w]
            except ValueError:
                row = None
            if row is None or len(row) != 3 or not np.isfinite(row).all():
                raise SystemExit(f"{path}:{no}: a scanner position needs three finite numbers, got {line.strip()!r}")
            rows.append(row)
    if not rows:
        raise SystemExit(f"{path}: no scanner position")
    return np.asarray(rows, np.float32)


def read_aligned_scans(path):
    """--scan_alignment: the union of the PLYs the project file lists (relative to it), each taken into the common frame by its
    matrix -> (xyz float32 [n, 3], owner int32 [n]: the number of the scan a point is from, scanners float32 [m, 3]: their origins)"""
    xyz, owner, scanners = [], [], []
    for k, (name, T) in enumerate(cloud.read_scan_alignment(path)):
        p = cloud.read_ply(os.path.join(os.path.dirname(os.path.abspath(path)), name))["xyz"]
        xyz.append(apply_transform(p, T))
        owner.append(np.full(len(p), k, np.int32))
        scanners.append(T[:3, 3] / T[3, 3])
    return np.concatenate(xyz), np.concatenate(owner), np.asarray(scanners, np.float32)


def load_ground_truth(args):
    """(the ground-truth file as read_ply gives it, owner or None, scanners or None) for --ground_truth [--scanners] or --scan_alignment"""
    if args.scan_alignment:
        xyz, owner, scanners = read_aligned_scans(args.scan_alignment)
        return {"xyz": xyz}, owner, scanners
    return cloud.read_ply(args.ground_truth), None, read_scanners(args.scanners) if args.scanners else None


def observed_args(args, scanners, owner):
    """the keyword arguments of cloud.evaluate for the observed-space keys; none without --scanners / --scan_alignment"""
    if scanners is None:
        return {}
    return {"scanners": scanners, "owner": owner, "face_size": args.face_size, "window": args.window, "free_rel": args.free_rel, "free_abs": args.free_abs}


def file_normals_wanted(args, gt):
    """the ground-truth file's own normals serve --refine_method plane unless a radius asks for estimated ones"""
    return args.refine and args.refine_method == "plane" and args.refine_normal_radius is None and "normals" in gt


def refine_method(args, radii, normals):
    """(the keyword arguments of cloud.align for --refine_method, what "refine" reports of them); normals: the file's, in the
    order of the cloud that is registered against, or None"""
    if args.refine_method == "point":
        return {}, {"method": "point"}
    if normals is not None:
        return {"method": "plane", "target_normals": normals}, {"method": "plane", "normals": "ground truth file"}
    r = args.refine_normal_radius if args.refine_normal_radius is not None else min(radii)
    return ({"method": "plane", "normal_radius": r, "normal_k": args.refine_normal_k},
            {"method": "plane", "normals": "estimated", "normal_radius": r, "normal_k": args.refine_normal_k})


def main_voxel(args, tol):
    """the run with --voxel: transform, crop, resample both clouds, refine on the resampled clouds, score"""
    t0 = time.perf_counter()
    rec = cloud.read_ply(args.reconstruction)["xyz"]
    gt_file, owner, scanners = load_ground_truth(args)
    gt = gt_file["xyz"]
    gt_n = gt_file["normals"] if file_normals_wanted(args, gt_file) else None   # they follow their points through every step
    T0 = np.loadtxt(args.transform) if args.transform else np.eye(4)
    if args.transform:
        rec = apply_transform(rec, T0)
    if args.crop:
        box = [float(v) for v in args.crop.split(",")]
        if len(box) != 6:
            raise SystemExit("--crop needs xmin,ymin,zmin,xmax,ymax,zmax")
        gt_n = gt_n[crop_keep(gt, box)] if gt_n is not None else None
        owner = owner[crop_keep(gt, box)] if owner is not None else None
        rec, gt = crop(rec, box), crop(gt, box)
    t1 = time.perf_counter()
    rec, drop_r = cloud.drop_nonfinite(rec)
    gt_n = gt_n[np.isfinite(gt).all(1)] if gt_n is not None else None
    owner = owner[np.isfinite(gt).all(1)] if owner is not None else None
    gt, drop_g = cloud.drop_nonfinite(gt)
    n_in = (len(rec), len(gt))
    obs, t_obs = None, 0.0
    if scanners is not None:   # the range maps come from the scan as it is, before the resampling
        with cloud.Cloud(gt, args.device) as c_scan:
            obs = cloud.Observer(c_scan, scanners, owner, args.face_size, args.window)
        t_obs = time.perf_counter() - t1
    rec = cloud.voxel_downsample(rec, args.voxel, device=args.device)["xyz"]
    gt_v = cloud.voxel_downsample(gt, args.voxel, normals=gt_n, device=args.device)
    gt, gt_n = gt_v["xyz"], gt_v.get("normals")
    t2 = time.perf_counter()
    refine = None
    if args.refine:
        radii = [float(r) for r in args.refine_radii.split(",") if r.strip()] if args.refine_radii else [8 * max(tol), 4 * max(tol), 2 * max(tol)]
        how, said = refine_method(args, radii, gt_n)
        with cloud.Cloud(gt, args.device) as c_gt:
            T, rounds = cloud.align(rec, c_gt, None, radii=radii, with_scale=not args.refine_no_scale, max_iter=args.refine_iters, **how)
        rec = apply_transform(rec, T)
        T = T @ np.asarray(T0, np.float64)
        refine = {"rounds": rounds, "matrix": T.tolist(), "seconds": round(time.perf_counter() - t2, 4), **said}
        if args.save_transform:
            np.savetxt(args.save_transform, T, fmt="%.17g")
    timings = {}
    if obs is None:
        res = cloud.evaluate(rec, gt, tol, device=args.device, timings=timings)
    else:
        with obs:
            res = cloud.evaluate(rec, gt, tol, device=args.device, timings=timings, scanners=obs, free_rel=args.free_rel, free_abs=args.free_abs)
    res["dropped_reconstruction"], res["dropped_ground_truth"] = drop_r, drop_g
    res["voxel"], res["n_reconstruction_in"], res["n_ground_truth_in"] = float(args.voxel), n_in[0], n_in[1]
    res["seconds"] = {"read": round(t1 - t0, 4), "voxel": round(t2 - t1 - t_obs, 4), "upload_build": round(timings["upload_build_s"], 4),
                      "query": round(timings["query_s"], 4)}
    if obs is not None:
        res["seconds"]["observe"] = round(t_obs + timings["observe_s"], 4)
    if refine is not None:
        res["refine"] = refine
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reconstruction", required=True)
    ap.add_argument("--ground_truth")
    ap.add_argument("--scanners", help="text file of scanner positions in the ground truth's frame, one `x y z` per line: adds the observed-space keys")
    ap.add_argument("--scan_alignment", help="MeshLab project (.mlp) of the scans: the ground truth is the union of its PLYs, each with its scanner")
    ap.add_argument("--face_size", type=int, default=1024, help="cube-map face of a scanner's range image (an untuned starting value)")
    ap.add_argument("--window", type=int, default=1, help="a pixel's range is the nearest of the (2 window + 1)^2 around it (untuned)")
    ap.add_argument("--free_rel", type=float, default=0.02, help="a point is in free space below (1 - free_rel) x the range (untuned)")
    ap.add_argument("--free_abs", type=float, default=0.0, help="... after adding this to its own range")
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
    ap.add_argument("--refine_method", choices=("point", "plane"), default="point")
    ap.add_argument("--refine_normal_radius", type=float, help="estimate the ground truth's normals within this radius (default: its file's own "
                    "normals, else the smallest refine radius, an untuned starting value)")
    ap.add_argument("--refine_normal_k", type=int, default=16)
    args = ap.parse_args()
    if not args.refine and (args.refine_radii or args.refine_no_scale or args.save_transform or args.refine_method != "point"):
        raise SystemExit("--refine_radii, --refine_no_scale, --refine_method and --save_transform need --refine")
    if args.refine_method != "plane" and (args.refine_normal_radius is not None or args.refine_normal_k != 16):
        raise SystemExit("--refine_normal_radius and --refine_normal_k need --refine_method plane")
    if bool(args.ground_truth) == bool(args.scan_alignment):
        raise SystemExit("give the ground truth as either --ground_truth or --scan_alignment")
    if args.scanners and args.scan_alignment:
        raise SystemExit("--scanners and --scan_alignment exclude each other: the project file names the scanners")
    if not (args.scanners or args.scan_alignment) and (args.face_size, args.window, args.free_rel, args.free_abs) != (1024, 1, 0.02, 0.0):
        raise SystemExit("--face_size, --window, --free_rel and --free_abs need --scanners or --scan_alignment")
    if args.voxel is not None and not (np.isfinite(args.voxel) and args.voxel > 0):
        raise SystemExit("--voxel needs a finite positive edge length")
    tol = [float(t) for t in args.tolerances.split(",") if t.strip()]
    if args.voxel is not None:
        return main_voxel(args, tol)
    t0 = time.perf_counter()
    rec = cloud.read_ply(args.reconstruction)["xyz"]
    gt_file, owner, scanners = load_ground_truth(args)
    gt = gt_file["xyz"]
    refine = None
    if args.refine:
        T0 = np.loadtxt(args.transform) if args.transform else np.eye(4)
        radii = [float(r) for r in args.refine_radii.split(",") if r.strip()] if args.refine_radii else [8 * max(tol), 4 * max(tol), 2 * max(tol)]
        how, said = refine_method(args, radii, gt_file["normals"][np.isfinite(gt).all(1)] if file_normals_wanted(args, gt_file) else None)
        t_r = time.perf_counter()
        with cloud.Cloud(cloud.drop_nonfinite(gt)[0], args.device) as c_gt:
            T, rounds = cloud.align(rec, c_gt, T0, radii=radii, with_scale=not args.refine_no_scale, max_iter=args.refine_iters, **how)
        refine = {"rounds": rounds, "matrix": T.tolist(), "seconds": round(time.perf_counter() - t_r, 4), **said}
        if args.save_transform:
            np.savetxt(args.save_transform, T, fmt="%.17g")
        rec = apply_transform(rec, T)
    elif args.transform:
        rec = apply_transform(rec, np.loadtxt(args.transform))
    if args.crop:
        box = [float(v) for v in args.crop.split(",")]
        if len(box) != 6:
            raise SystemExit("--crop needs xmin,ymin,zmin,xmax,ymax,zmax")
        owner = owner[crop_keep(gt, box)] if owner is not None else None
        rec, gt = crop(rec, box), crop(gt, box)
    t1 = time.perf_counter()
    timings = {}
    res = cloud.evaluate(rec, gt, tol, device=args.device, timings=timings, **observed_args(args, scanners, owner))
    res["seconds"] = {"read": round(t1 - t0, 4), "upload_build": round(timings["upload_build_s"], 4), "query": round(timings["query_s"], 4)}
    if scanners is not None:
        res["seconds"]["observe"] = round(timings["observe_s"], 4)
    if refine is not None:
        res["refine"] = refine
    print(json.dumps(res))


if __name__ == "__main__":
    main()
