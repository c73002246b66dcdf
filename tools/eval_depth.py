#!/usr/bin/env python3
"""Score the depth maps of a result folder per view against ground-truth depth maps (mp-mvs_amd/depthmap.py: score;
DESIGN.md section 14).

    python tools/eval_depth.py --dense_folder D [--result_folder R] [--map depths.dmb] [--tolerances 0.01,0.02,0.05,0.1] [--relative]
                               --ground_truth scan.ply [--transform T.txt] [--splat 1] [--occl 0.02] [--device 0]
    python tools/eval_depth.py --dense_folder D ... --gt_depth_dir DIR --gt_format eth3d|colmap|dmb [--gt_pattern PATTERN]
    python tools/eval_depth.py --dense_folder D ... --ground_truth_mesh mesh.ply [--transform T.txt]

D holds cams/, images/ and pair.txt; the results are R/2333_<id>/<map> with R = D/MPMVS unless --result_folder names another
root.  Every view that has a result folder with the map is scored.  The ground truth is either
  * a scan (--ground_truth, a PLY file) rendered into every view's camera on the GPU (cloud.Cloud.render_depth): a z-buffer
    with a visibility test.  --transform: a 4 x 4 text matrix that takes the scan into the frame of the cameras (fp64, rounded
    to fp32).  tools/eval_ply.py --refine --save_transform feeds it: that file takes the reconstruction (the cameras' frame)
    into the scan's frame, so its inverse (numpy.linalg.inv of the loaded matrix) is what --transform expects here.
    --splat / --occl: a point is hidden when a point within `splat` pixels is nearer by more than the factor
    1 + occl.  The slope rule: a slanted surface hides itself once occl is below splat x the relative change of depth per
    pixel, so raise --occl with --splat on steep or close scenes.  The defaults are starting values from the synthetic scene,
    not tuned on a real scan.  The map is rendered at the estimate's size with the camera rescaled as fusion does; or
  * a triangle mesh (--ground_truth_mesh, a PLY file as mesh.write_ply_mesh writes it: someone's ground-truth surface, or our own
    tools/mesh_ply.py output) rasterised into every view's camera on the GPU (mesh.Mesh.render_depth), all views in one call: the
    depth of the nearest surface along each pixel's ray, with no parameter, so --splat and --occl are refused with it.  --transform
    as for a scan.  Against our own mesh this measures how far each depth map lies from the surface they were all integrated into; or
  * one depth-map file per view (--gt_depth_dir): eth3d = raw little-endian fp32 of the estimate's size, colmap = COLMAP's
    "W&H&C&" maps, dmb = our own (with a second result root as DIR this is the A/B of two of our own builds).  --gt_pattern is
    a format string of the file name with {id} (defaults: "{id:08d}.JPG", "{id:08d}.jpg.geometric.bin",
    "2333_{id:08d}/depths.dmb").  A map of another size than the estimate is refused; nothing is resampled.
--tolerances are absolute depth errors, or shares of the ground-truth depth with --relative.
Prints one JSON line: the score per view and pooled, seconds per stage, and the render's device ms."""
import argparse
import glob
import importlib
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

depthmap = importlib.import_module("mp-mvs_amd.depthmap")
hostlib = importlib.import_module("mp-mvs_amd.hostlib")

GT_PATTERNS = {"eth3d": "{id:08d}.JPG", "colmap": "{id:08d}.jpg.geometric.bin", "dmb": "2333_{id:08d}/depths.dmb"}


def result_views(root, map_name):
    """sorted [(id, path of the map)] of the 2333_<id> folders under root that hold the map"""
    out = []
    for d in glob.glob(os.path.join(root, "2333_*")):
        m = re.fullmatch(r"2333_(\d{8})", os.path.basename(d))
        path = os.path.join(d, map_name)
        if m and os.path.isfile(path):
            out.append((int(m.group(1)), path))
    return sorted(out)


def image_size(dense_folder, view_id):
    """(width, height) of images/<id>.*"""
    files = sorted(glob.glob(os.path.join(dense_folder, "images", f"{view_id:08d}.*")))
    if not files:
        raise SystemExit(f"no image of view {view_id:08d} under {dense_folder}/images")
    h, w = hostlib.read_image(files[0]).shape[:2]
    return w, h


def apply_transform(xyz, T):
    T = np.asarray(T, np.float64)
    if T.shape != (4, 4) or not np.isfinite(T).all():
        raise SystemExit(f"--transform needs a finite 4 x 4 matrix, got shape {T.shape}")
    p = xyz.astype(np.float64)
    h = p @ T[:3, :3].T + T[:3, 3]
    w = p @ T[3, :3] + T[3, 3]
    return (h / w[:, None]).astype(np.float32)


def read_gt_file(path, fmt, est_shape):
    H, W = est_shape
    if fmt == "eth3d":
        return depthmap.read_eth3d_depth(path, W, H)   # refuses a file that does not hold W * H values, naming both
    gt = depthmap.read_colmap_map(path) if fmt == "colmap" else hostlib.read_dmb(path)
    if gt.ndim != 2:
        raise ValueError(f"{path}: {gt.shape[2]} channels, a depth map has one")
    if gt.shape != (H, W):
        raise ValueError(f"{path}: the ground-truth map is {gt.shape[1]} x {gt.shape[0]}, the estimate {W} x {H}; maps are not resampled")
    return gt


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--dense_folder", required=True)
    ap.add_argument("--result_folder")
    ap.add_argument("--map", default="depths.dmb")
    ap.add_argument("--ground_truth", help="a scan (PLY), rendered into every view on the GPU")
    ap.add_argument("--transform", help="4 x 4 text matrix: the scan into the cameras' frame")
    ap.add_argument("--ground_truth_mesh", help="a triangle mesh (PLY), rasterised into every view on the GPU; takes no --splat / --occl")
    ap.add_argument("--splat", type=int, default=None, help="visibility window radius in pixels (0: plain z-buffer)")
    ap.add_argument("--occl", type=float, default=None,
                    help="a point is hidden when one within --splat pixels is nearer by more than the factor 1 + occl; a slanted surface hides "
                         "itself once occl < splat x the relative depth change per pixel (defaults: --splat 1 --occl 0.02)")
    ap.add_argument("--gt_depth_dir")
    ap.add_argument("--gt_format", choices=sorted(GT_PATTERNS))
    ap.add_argument("--gt_pattern")
    ap.add_argument("--tolerances", default="0.01,0.02,0.05,0.1")
    ap.add_argument("--relative", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    if bool(args.ground_truth) + bool(args.gt_depth_dir) + bool(args.ground_truth_mesh) != 1:
        raise SystemExit("give exactly one of --ground_truth (a scan), --ground_truth_mesh (a mesh) and --gt_depth_dir (depth maps)")
    if args.ground_truth_mesh and (args.splat is not None or args.occl is not None):
        raise SystemExit("--ground_truth_mesh takes no --splat / --occl: a rasterised mesh has no gaps to close")
    splat, occl = (1 if args.splat is None else args.splat), (0.02 if args.occl is None else args.occl)
    if args.gt_depth_dir and not args.gt_format:
        raise SystemExit("--gt_depth_dir needs --gt_format eth3d|colmap|dmb")
    try:
        tol = [float(t) for t in args.tolerances.split(",") if t.strip()]
    except ValueError:
        raise SystemExit("--tolerances needs numbers separated by commas") from None
    if not tol or not all(np.isfinite(t) and t > 0 for t in tol):
        raise SystemExit("--tolerances must be finite and positive")
    for sub in ("cams", "images", "pair.txt"):
        if not os.path.exists(os.path.join(args.dense_folder, sub)):
            raise SystemExit(f"{args.dense_folder}: no {sub}")
    root = args.result_folder or os.path.join(args.dense_folder, "MPMVS")
    views = result_views(root, args.map)
    if not views:
        raise SystemExit(f"no 2333_<id>/{args.map} under {root}")

    t0 = time.perf_counter()
    est = {}
    for vid, path in views:
        a = hostlib.read_dmb(path)
        if a.ndim != 2:
            raise SystemExit(f"{path}: {a.shape[2]} channels, a depth map has one")
        est[vid] = a
    t1 = time.perf_counter()
    render_ms, render_counts = None, None
    try:
        if args.ground_truth or args.ground_truth_mesh:
            import torch  # noqa: F401  (the HIP runtime torch bundles, before our library: engine.load)
            cloud = importlib.import_module("mp-mvs_amd.cloud")
            if args.ground_truth:
                scan = cloud.read_ply(args.ground_truth)["xyz"]
            else:
                mesh = importlib.import_module("mp-mvs_amd.mesh")
                surface = mesh.read_ply_mesh(args.ground_truth_mesh)
                scan = surface["xyz"]
            if args.transform:
                scan = apply_transform(scan, np.loadtxt(args.transform))
            cams = []
            for vid, _ in views:
                cam = hostlib.read_camera(os.path.join(args.dense_folder, "cams", f"{vid:08d}_cam.txt"))
                iw, ih = image_size(args.dense_folder, vid)
                H, W = est[vid].shape
                cams.append(depthmap.camera_at_size(cam, iw, ih, W, H))
            if args.ground_truth:
                with cloud.Cloud(scan, args.device) as c:
                    maps = c.render_depth(cams, splat=splat, occl_rel=occl)
                    render_ms = c.render_ms()[0]
            else:
                with mesh.Mesh(scan, surface["tri"], None, args.device) as h:
                    maps = h.render_depth(cams)
                    render_ms, render_counts = h.render_ms()[0], h.last_render_counts
            gt = {vid: m for (vid, _), m in zip(views, maps)}
        else:
            pattern = args.gt_pattern or GT_PATTERNS[args.gt_format]
            gt = {vid: read_gt_file(os.path.join(args.gt_depth_dir, pattern.format(id=vid)), args.gt_format, est[vid].shape) for vid, _ in views}
    except (ValueError, OSError, RuntimeError) as e:
        raise SystemExit(str(e)) from None
    t2 = time.perf_counter()
    per_view = {f"{vid:08d}": depthmap.score(est[vid], gt[vid], tol, args.relative) for vid, _ in views}
    t3 = time.perf_counter()
    res = {"views": per_view, "pooled": depthmap.pool(per_view.values()), "ground_truth": "rendered" if args.ground_truth else ("rendered_mesh" if args.ground_truth_mesh else args.gt_format),
           "seconds": {"read": round(t1 - t0, 4), "ground_truth": round(t2 - t1, 4), "score": round(t3 - t2, 4)}, "render_device_ms": render_ms}
    if args.ground_truth_mesh:
        res["render_counts"] = render_counts
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
