#!/usr/bin/env python3
"""The ICP pass (mp-mvs_amd/cloud.py: Aligner; csrc/pm_align.hpp) on the two synthetic clouds of tools/bench_cloud.py
(--points each, default 2 M): the "reconstruction" is the moving cloud, the "ground truth" the target.

Per radius (default: the three tolerances of bench_cloud.py), medians and min .. max of --reps repetitions after --warmup:
  pass ms       device time of one point-to-point pass (HIP events: binning + kernel), at the identity transform
  plane ms      device time of one point-to-plane pass (csrc/pm_align_plane.hpp) on the same handle, in the same repetition, with
                the target's normals from Cloud.normals(radius, 16); plane/pass is the ratio of the two medians
  query ms      device time of mpmvs_cloud_nearest's query passes for the same points and radius, in the same process
  resident wall wall time of one ICP iteration on the resident cloud: Aligner.sums + solve
  composed wall wall time of the iteration a user composes without the Aligner: Cloud.nearest(want_idx=True) on the points
                transformed with numpy, and the moments of the matched pairs in numpy (float sums: not bit-reproducible)
  cKDTree wall  the same iteration with scipy.spatial.cKDTree (16 workers; the tree is built once, outside the timing), where scipy
                is importable
--trace: two repetitions only and no k-d tree, for `rocprofv3 --kernel-trace --stats -- python tools/bench_align.py --trace`
(never together with counters).  Prints a table and one JSON line."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: F401,E402

from bench_cloud import make_clouds  # noqa: E402

cloud = importlib.import_module("mp-mvs_amd.cloud")
WORKERS = 16


def stat(xs, scale=1.0):
    a = np.asarray(xs, np.float64) * scale
    return {"median": round(float(np.median(a)), 4), "min": round(float(a.min()), 4), "max": round(float(a.max()), 4), "n": int(a.size)}


def moments(y, p):
    """the float moments Umeyama needs, from matched pairs"""
    return len(y), y.mean(0), p.mean(0), (p - p.mean(0)).T @ (y - y.mean(0)) / len(y), ((y - y.mean(0)) ** 2).sum() / len(y)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--radii", default="0.01,0.02,0.05")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--no-kdtree", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    radii = sorted(float(r) for r in args.radii.split(","))
    reps, warmup = (2, 0) if args.trace else (args.reps, args.warmup)
    src, gt = make_clouds(args.points, radii)
    M = np.eye(4)
    out = {"points": args.points, "reps": reps, "warmup": warmup, "bin": os.environ.get("MPMVS_CLOUD_BIN", "1"), "radii": []}
    tree = None
    if not args.no_kdtree and not args.trace:
        try:
            from scipy.spatial import cKDTree
            tree = cKDTree(gt)
        except ImportError:
            print("scipy is not importable: no k-d tree yardstick")
    print(f"{'radius':>7} {'matched':>9} {'pass ms':>18} {'plane ms':>18} {'plane/pass':>10} {'query ms':>18} {'pass/query':>10} {'resident ms':>12} "
          f"{'composed ms':>12} {'cKDTree ms':>11}")
    with cloud.Cloud(gt, args.device) as c, cloud.Aligner(c, src) as al:
        for r in radii:
            pass_ms, plane_ms, query_ms, res_wall, comp_wall, kd_wall = [], [], [], [], [], []
            al.set_normals(c.normals(r, 16, want_curvature=False)[0])
            for k in range(warmup + reps):
                t0 = time.perf_counter()
                sums, frame = al.sums(r, M)
                cloud.solve(sums, frame, M, True)
                t1 = time.perf_counter()
                p_ms = al.ms()
                psums, _ = al.plane_sums(r, M)
                pl_ms = al.ms()
                t1b = time.perf_counter()
                y = (src.astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)
                d2, idx = c.nearest(y, r, want_idx=True)
                hit = idx >= 0
                moments(y[hit].astype(np.float64), gt[idx[hit]].astype(np.float64))
                t2 = time.perf_counter()
                if k >= warmup:
                    pass_ms.append(p_ms)
                    plane_ms.append(pl_ms)
                    query_ms.append(c.kernel_ms()[0])
                    res_wall.append(t1 - t0)
                    comp_wall.append(t2 - t1b)
            if tree is not None:
                for k in range(3):
                    t0 = time.perf_counter()
                    y = (src.astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)
                    d, idx = tree.query(y, k=1, distance_upper_bound=r, workers=WORKERS)
                    hit = np.isfinite(d)
                    moments(y[hit].astype(np.float64), gt[idx[hit]].astype(np.float64))
                    kd_wall.append(time.perf_counter() - t0)
            row = {"radius": r, "matched": int(sums[0]), "pass_ms": stat(pass_ms), "plane_matched": int(psums[0]), "plane_ms": stat(plane_ms),
                   "plane_over_pass": round(float(np.median(plane_ms) / np.median(pass_ms)), 4), "query_ms": stat(query_ms),
                   "pass_over_query": round(float(np.median(pass_ms) / np.median(query_ms)), 4),
                   "resident_iteration_wall_ms": stat(res_wall, 1e3), "composed_iteration_wall_ms": stat(comp_wall, 1e3),
                   "ckdtree_iteration_wall_ms": stat(kd_wall, 1e3) if kd_wall else None}
            out["radii"].append(row)
            f = lambda s: f"{s['median']:.3f} ({s['min']:.3f}..{s['max']:.3f})"   # noqa: E731
            print(f"{r:7.4g} {row['matched']:9d} {f(row['pass_ms']):>18} {f(row['plane_ms']):>18} {row['plane_over_pass']:10.3f} {f(row['query_ms']):>18} "
                  f"{row['pass_over_query']:10.3f} "
                  f"{row['resident_iteration_wall_ms']['median']:12.2f} {row['composed_iteration_wall_ms']['median']:12.2f} "
                  f"{row['ckdtree_iteration_wall_ms']['median'] if kd_wall else float('nan'):11.1f}", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
