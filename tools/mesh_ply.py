#!/usr/bin/env python3
"""A triangle mesh from the depth maps of a dense folder: the maps are integrated into a dense TSDF volume on the GPU and the zero
level set is extracted by marching tetrahedra (mp-mvs_amd/mesh.py; csrc/pm_tsdf.hpp).

    python tools/mesh_ply.py --dense_folder D --output mesh.ply --voxel V [--trunc 4V] [--min_weight 2]
                             [--bbox x0 y0 z0 x1 y1 z1 | --bbox_from MPMVS_model.ply --bbox_percentile 1]
                             [--sparse [--pad 1.0] [--max_bricks N]]
                             [--min_component N] [--largest K] [--simplify C [--simplify_placement mean|quadric]] [--normals]

Reads cams/<id>_cam.txt, images/<id>.* and <result_folder>/2333_<id>/depths.dmb (result_folder: D/MPMVS) with the readers of
mp-mvs_amd/hostlib.py; a camera is rescaled to the size of its depth map as the fusion does, and the image is sampled at the map's
pixels for the colours (--no_color: a volume without colour, 8 instead of 24 bytes per voxel).  The views go through
mpmvs_tsdf_integrate in batches of --batch, so only one batch of maps is in host memory at a time.  The box is --bbox, or the
--bbox_percentile .. 100 - --bbox_percentile range per axis of the points of --bbox_from (default: <result_folder>/MPMVS_model.ply),
grown by the truncation distance.  The volume is dense: (box / voxel)^3 voxels, refused above --max_voxels.
--trunc (4 voxels) and --min_weight (2) are untuned starting values, not tuned on any real scene.
--sparse: a brick-sparse volume (mesh.SparseVolume): the views are read twice, first to allocate the bricks of
8 x 8 x 8 voxels within --pad voxels (default 1.0, an untuned starting value) of the samples along every depth pixel's ray through the
truncation band, at most --max_bricks of them (default: the whole brick grid, at most 2^21), then to integrate; the box is virtual
and --max_voxels does not apply.  The mesh is a sub-mesh of the dense one: the same vertices, the triangles whose corners all exist.
--min_component N (triangles; 0 = off, the default) and --largest K drop the small detached pieces of the mesh on the GPU
(mesh.remove_small_components): the connected components with fewer than N triangles go, and all but the K
largest; vertices no triangle names go with them.  --normals writes area-weighted vertex normals (nx ny nz after z).  The mesh is
cleaned first, then shaded.  N has not been tuned on any real scene.
--simplify C (scene units; off by default) clusters the vertices on a grid of edge C after the cleaning and before --normals
(mesh.simplify): one vertex per occupied cell, placed by plane quadrics (--simplify_placement quadric, the
default) or at the mean; collapsed and duplicate triangles and the vertices no triangle names any more go.  The result line then
holds simplified = {vertices_in, triangles_in, clusters, non_finite, collapsed, duplicates, placed}.
Prints one JSON line: n_vox, views, vertices, triangles, device ms per pass, wall seconds; with --sparse also bricks, brick_share and
device_bytes; with the cleaning flags also components, largest_component and removed_triangles, with --normals normals_defined, and
the device ms of their passes."""
import argparse
import glob
import importlib
import json
import math
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def result_views(root):
    out = []
    for d in glob.glob(os.path.join(root, "2333_*")):
        m = re.fullmatch(r"2333_(\d{8})", os.path.basename(d))
        path = os.path.join(d, "depths.dmb")
        if m and os.path.isfile(path):
            out.append((int(m.group(1)), path))
    return sorted(out)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--dense_folder", required=True)
    ap.add_argument("--result_folder")
    ap.add_argument("--output", required=True)
    ap.add_argument("--voxel", type=float, required=True, help="lattice spacing in scene units")
    ap.add_argument("--trunc", type=float, help="truncation distance; default 4 voxels, an untuned starting value")
    ap.add_argument("--min_weight", type=int, default=2, help="observations a lattice point needs to take part; 2 is an untuned starting value")
    ap.add_argument("--bbox", type=float, nargs=6, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"))
    ap.add_argument("--bbox_from", help="a PLY whose points give the box (default: <result_folder>/MPMVS_model.ply)")
    ap.add_argument("--bbox_percentile", type=float, default=1.0)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--no_color", action="store_true")
    ap.add_argument("--max_voxels", type=int, default=1 << 30)
    ap.add_argument("--sparse", action="store_true", help="a brick-sparse volume: allocate from all views, then integrate")
    ap.add_argument("--pad", type=float, default=1.0, help="--sparse: voxels around a ray sample whose bricks are allocated; 1.0 is an untuned starting value")
    ap.add_argument("--max_bricks", type=int, help="--sparse: the cap on allocated bricks (default: the whole brick grid, at most 2^21)")
    ap.add_argument("--min_component", type=int, default=0, help="drop connected components with fewer triangles; 0 = off; untuned on real scenes")
    ap.add_argument("--largest", type=int, help="keep only the K largest components by triangle count")
    ap.add_argument("--simplify", type=float, help="cluster the vertices on a grid of this edge (scene units) after the cleaning; off by default")
    ap.add_argument("--simplify_placement", choices=("mean", "quadric"), default="quadric")
    ap.add_argument("--normals", action="store_true", help="write area-weighted vertex normals")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    if args.min_component < 0 or (args.largest is not None and args.largest < 1):
        raise SystemExit("--min_component must not be negative and --largest must be at least 1")
    if args.simplify is not None and not (0.0 < args.simplify < float("inf")):
        raise SystemExit("--simplify must be finite and positive")
    if not args.sparse and (args.pad != 1.0 or args.max_bricks is not None):
        raise SystemExit("--pad and --max_bricks go with --sparse")
    if not (math.isfinite(args.voxel) and args.voxel > 0):
        raise SystemExit("--voxel must be finite and positive")
    trunc = 4.0 * args.voxel if args.trunc is None else args.trunc
    if not (math.isfinite(trunc) and trunc > 0):
        raise SystemExit("--trunc must be finite and positive")
    if args.min_weight < 1 or args.batch < 1:
        raise SystemExit("--min_weight and --batch must be at least 1")
    if args.bbox and args.bbox_from:
        raise SystemExit("give --bbox or --bbox_from, not both")
    root = args.result_folder or os.path.join(args.dense_folder, "MPMVS")
    views = result_views(root)
    if not views:
        raise SystemExit(f"no 2333_<id>/depths.dmb under {root}")

    import torch  # noqa: F401  (the HIP runtime torch bundles, before our library: engine.load)
    hostlib = importlib.import_module("mp-mvs_amd.hostlib")
    depthmap = importlib.import_module("mp-mvs_amd.depthmap")
    cloud = importlib.import_module("mp-mvs_amd.cloud")
    mesh = importlib.import_module("mp-mvs_amd.mesh")

    t0 = time.perf_counter()
    if args.bbox:
        lo, hi = np.array(args.bbox[:3], np.float64), np.array(args.bbox[3:], np.float64)
    else:
        path = args.bbox_from or os.path.join(root, "MPMVS_model.ply")
        if not os.path.isfile(path):
            raise SystemExit(f"no --bbox, and no point cloud at {path} to take the box from")
        if not 0.0 <= args.bbox_percentile < 50.0:
            raise SystemExit("--bbox_percentile must lie in [0, 50)")
        pts = cloud.read_ply(path)["xyz"]
        pts = pts[np.isfinite(pts).all(1)]
        if not len(pts):
            raise SystemExit(f"{path}: no finite point")
        lo = np.percentile(pts, args.bbox_percentile, axis=0) - trunc
        hi = np.percentile(pts, 100.0 - args.bbox_percentile, axis=0) + trunc
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi > lo).all()):
        raise SystemExit(f"the box {lo.tolist()} .. {hi.tolist()} is empty or not finite")
    dims = [int(math.ceil((hi[a] - lo[a]) / args.voxel)) + 1 for a in range(3)]
    n_vox = dims[0] * dims[1] * dims[2]
    if not args.sparse and n_vox > min(args.max_voxels, 1 << 30):
        raise SystemExit(f"{dims[0]} x {dims[1]} x {dims[2]} = {n_vox} voxels exceed --max_voxels {min(args.max_voxels, 1 << 30)}: raise --voxel or shrink the box")

    def load(vid, path):
        d = hostlib.read_dmb(path)
        if d.ndim != 2:
            raise SystemExit(f"{path}: {d.shape[2]} channels, a depth map has one")
        files = sorted(glob.glob(os.path.join(args.dense_folder, "images", f"{vid:08d}.*")))
        if not files:
            raise SystemExit(f"no image of view {vid:08d} under {args.dense_folder}/images")
        img = hostlib.read_image(files[0], 3)
        ih, iw = img.shape[:2]
        H, W = d.shape
        cam = depthmap.camera_at_size(hostlib.read_camera(os.path.join(args.dense_folder, "cams", f"{vid:08d}_cam.txt")), iw, ih, W, H)
        if (ih, iw) != (H, W):   # the image at the map's pixel centres, nearest
            ys = np.minimum(((np.arange(H) + 0.5) * ih / H).astype(np.int64), ih - 1)
            xs = np.minimum(((np.arange(W) + 0.5) * iw / W).astype(np.int64), iw - 1)
            img = img[ys][:, xs]
        return cam, d, np.ascontiguousarray(img)

    device_ms = {"integrate": 0.0}
    sparse = None
    try:
        if args.sparse:
            volume = mesh.SparseVolume(lo.astype(np.float32), args.voxel, dims, trunc, color=not args.no_color, pad=args.pad, max_bricks=args.max_bricks,
                                       device=args.device)
        else:
            volume = mesh.Volume(lo.astype(np.float32), args.voxel, dims, trunc, color=not args.no_color, device=args.device)
        with volume as vol:
            if args.sparse:
                device_ms.update({"allocate_mark": 0.0, "allocate_commit": 0.0})
                for b in range(0, len(views), args.batch):
                    cams, depths, _ = zip(*(load(vid, path) for vid, path in views[b:b + args.batch]))
                    vol.allocate(cams, depths)
                    st = vol.stats()
                    device_ms["allocate_mark"] += st["allocate_mark"]
                    device_ms["allocate_commit"] += st["allocate_commit"]
                sparse = {k: vol.stats()[k] for k in ("bricks", "brick_share", "device_bytes")}
            for b in range(0, len(views), args.batch):
                cams, depths, images = zip(*(load(vid, path) for vid, path in views[b:b + args.batch]))
                vol.integrate(cams, depths, None if args.no_color else images)
                device_ms["integrate"] += vol.pass_ms()["integrate"]
            t1 = time.perf_counter()
            m = vol.mesh(args.min_weight)
            ms = vol.pass_ms()
            device_ms.update({k: ms[k] for k in ("mark", "scan", "vertices", "triangles")})
        t2 = time.perf_counter()
        if args.simplify is None:
            extra, normals = mesh.clean_and_shade(m, args.min_component, args.largest, args.normals, device=args.device)
            m = extra.pop("mesh")
            device_ms.update(extra.pop("device_ms"))
        else:   # cleaned, simplified, then shaded
            extra, _ = mesh.clean_and_shade(m, args.min_component, args.largest, False, device=args.device)
            m = extra.pop("mesh")
            device_ms.update(extra.pop("device_ms"))
            s = mesh.simplify(m, args.simplify, args.simplify_placement, drop_unreferenced=True, normals=args.normals, device=args.device)
            extra["simplified"] = dict(vertices_in=int(len(m["xyz"])), triangles_in=int(len(m["tri"])), clusters=int(len(s["count"])),
                                       placed=[int((s["placed"] == p).sum()) for p in range(3)], **s["counts"])
            device_ms.update({(k if k.startswith("normals_") else "simplify_" + k): v for k, v in s["device_ms"].items()})   # its select is not the cleaning's
            m, normals = {"xyz": s["xyz"], "rgb": s["rgb"], "tri": s["tri"]}, s["normals"]
            if args.normals:
                extra["normals_defined"] = s["normals_defined"]
    except (ValueError, OSError, RuntimeError) as e:
        raise SystemExit(str(e)) from None
    t2b = time.perf_counter()
    if normals is None:
        mesh.write_ply_mesh(args.output, m["xyz"], m["tri"], m["rgb"])
    else:
        mesh.write_ply_mesh(args.output, m["xyz"], m["tri"], m["rgb"], normals=normals)
    t3 = time.perf_counter()
    res = {"n_vox": n_vox, "dims": dims, "origin": [float(v) for v in lo.astype(np.float32)], "voxel": args.voxel, "trunc": trunc, "min_weight": args.min_weight,
           "views": len(views), "vertices": int(len(m["xyz"])), "triangles": int(len(m["tri"])),
           "device_ms": {k: round(v, 4) for k, v in device_ms.items()},
           "seconds": {"integrate": round(t1 - t0, 4), "mesh": round(t2 - t1, 4), "write": round(t3 - t2b, 4), "wall": round(t3 - t0, 4)}, "output": args.output}
    if sparse is not None:
        res.update(sparse)
    if extra:
        res["seconds"]["clean"] = round(t2b - t2, 4)
        res.update(extra)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
