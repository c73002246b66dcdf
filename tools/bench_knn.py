#!/usr/bin/env python3
"""The k-nearest-neighbour search and the outlier filter on top of it (mp-mvs_amd/cloud.py: Cloud.knn_self, remove_outliers;
csrc/pm_knn.hpp) on the two synthetic clouds of tools/bench_cloud.py (--points points each, default 2 M, spacing about 0.004) at
three radii (default: bench_cloud's tolerances).

Per cloud and radius: the candidates per point (mean of `within`), the grid-build ms, the device ms (HIP events, the query binning
included) of knn_self at k = 1, 8, 16 and 32 with d2 and idx, and beside the k = 1 figure the query ms of mpmvs_cloud_nearest for
the same points as explicit queries at the same radius, measured in the same process, alternating with it: what the list machinery
costs where it is not needed (knn_self additionally skips the query's own index, which nearest finds at d2 = 0).  Then
remove_outliers(k = 16, std_ratio = 2): device ms (build + query passes) and wall ms (upload, build, kernel, downloads and the
host's statistics), and beside it the wall time of scipy.spatial.cKDTree(points).query(points, k + 1, distance_upper_bound = radius,
workers = 16), build included: the neighbour search alone, which the CPU filters spend their time in.
Medians of --reps repetitions after --warmup.  --trace: two repetitions only and no k-d tree, for
`rocprofv3 --kernel-trace --stats -- python tools/bench_knn.py --trace` (never together with counters).
Prints a table and one JSON line."""
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

cloud = importlib.import_module("mp-mvs_amd.cloud")
from bench_cloud import WORKERS, make_clouds, med  # noqa: E402

KS = (1, 8, 16, 32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--radii", default="0.01,0.02,0.05")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--k", type=int, default=16, help="k of the remove_outliers rows")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--no-kdtree", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    radii = sorted(float(r) for r in args.radii.split(","))
    reps, warmup = (2, 0) if args.trace else (args.reps, args.warmup)
    rec, gt = make_clouds(args.points, [0.01, 0.02, 0.05])
    out = {"points": args.points, "reps": reps, "warmup": warmup, "bin": os.environ.get("MPMVS_CLOUD_BIN", "1"), "rows": []}
    cKDTree = None
    if not args.no_kdtree and not args.trace:
        try:
            from scipy.spatial import cKDTree
        except ImportError:
            print("scipy is not importable: no k-d tree yardstick")
    print(f"{'cloud':>5} {'radius':>7} {'within':>7} {'build ms':>8} " + " ".join(f"{'k=' + str(k):>8}" for k in KS) + f" {'nearest':>8} {'k1/near':>7} "
          f"{'filt dev':>8} {'filt wall':>9} {'kept':>8} {'kdtree ms':>9}")
    for name, pts in (("gt", gt), ("rec", rec)):
        with cloud.Cloud(pts, args.device) as c:
            for radius in radii:
                _, _, within = c.knn_self(radius, 1, want_within=True)   # builds the grid of this radius
                build_ms = c.knn_ms()[1]
                ms = {k: [] for k in KS}
                near = []
                for r in range(warmup + reps):
                    for k in KS:   # interleaved rounds in one process
                        c.knn_self(radius, k)
                        if r >= warmup:
                            ms[k].append(c.knn_ms()[0])
                        if k == 1:
                            c.nearest(pts, radius)
                            if r >= warmup:
                                near.append(c.kernel_ms()[0])
                dev, wall = [], []
                for r in range(warmup + reps):
                    t0 = time.perf_counter()
                    res = cloud.remove_outliers(pts, radius, k=args.k, device=args.device)
                    t1 = time.perf_counter()
                    if r >= warmup:
                        wall.append(t1 - t0)
                        dev.append(cloud.last_outliers_ms())
                row = {"cloud": name, "radius": radius, "n": len(pts), "mean_within": round(float(within.mean()), 2), "build_ms": round(build_ms, 4),
                       "knn_self_ms": {str(k): round(med(ms[k]), 4) for k in KS}, "nearest_query_ms": round(med(near), 4),
                       "k1_over_nearest": round(med(ms[1]) / med(near), 3) if med(near) > 0 else None,
                       "outliers": {"k": args.k, "device_ms": round(med(dev), 4), "wall_ms": round(med(wall) * 1e3, 3), "counts": [int(v) for v in res["counts"]]}}
                if cKDTree is not None:
                    times = []
                    for r in range(3):
                        t0 = time.perf_counter()
                        cKDTree(pts).query(pts, k=args.k + 1, distance_upper_bound=radius, workers=WORKERS)
                        times.append(time.perf_counter() - t0)
                    row["ckdtree_wall_ms"] = round(med(times) * 1e3, 2)
                    row["ckdtree_workers"] = WORKERS
                out["rows"].append(row)
                print(f"{name:>5} {radius:7.4g} {row['mean_within']:7.1f} {build_ms:8.3f} " + " ".join(f"{med(ms[k]):8.3f}" for k in KS) +
                      f" {med(near):8.3f} {row['k1_over_nearest'] or 0:7.2f} {med(dev):8.3f} {med(wall) * 1e3:9.2f} {int(res['counts'][2]):8d} "
                      f"{row.get('ckdtree_wall_ms', float('nan')):9.1f}", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
