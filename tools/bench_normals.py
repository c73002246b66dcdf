#!/usr/bin/env python3
"""The normal estimation (mp-mvs_amd/cloud.py: Cloud.normals; csrc/pm_normals.hpp) on the two synthetic clouds of
tools/bench_cloud.py (--points points each, default 2 M, spacing about 0.004) at three radii (default 0.01, 0.02, 0.05) and
k = 8, 16 and 32.

Per cloud, radius and k, all from one process with the calls alternating: the device ms (HIP events, the binning included, the grid
cached) of Cloud.normals, of knn_self at the same k (the list variant, which writes 8 k bytes per point), and of remove_outliers (the
reducing kernel k_knn_reduce: the same search, 8 bytes written per point; its figure includes the grid build of its own handle,
which is printed beside it), and on the host the wall time of scipy.spatial.cKDTree(points).query(points, k + 1,
distance_upper_bound = radius, workers = 16) plus a batched np.linalg.eigh over the scatter matrices: the same job on the CPU.
Medians of --reps repetitions after --warmup.  --trace: two repetitions only and no host yardstick, for
`rocprofv3 --kernel-trace --stats -- python tools/bench_normals.py --trace` (never together with counters).
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

KS = (8, 16, 32)


def host_normals(cKDTree, pts, radius, k):
    """the k-d tree query and a batched eigh over the scatter matrices of the neighbours found (and the point): wall seconds"""
    t0 = time.perf_counter()
    _, idx = cKDTree(pts).query(pts, k=k + 1, distance_upper_bound=radius, workers=WORKERS)
    for b in range(0, len(pts), 1 << 18):   # in blocks: the gathered neighbours of 2 M points at k = 32 would take gigabytes
        ib = idx[b:b + (1 << 18)]
        found = ib < len(pts)
        nb = pts[np.where(found, ib, 0)].astype(np.float64)
        w = found[:, :, None].astype(np.float64)
        cnt = np.maximum(found.sum(1), 1)[:, None, None]
        d = (nb - (nb * w).sum(1, keepdims=True) / cnt) * w
        np.linalg.eigh(np.einsum("nka,nkb->nab", d, d))
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--radii", default="0.01,0.02,0.05")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    radii = sorted(float(r) for r in args.radii.split(","))
    reps, warmup = (2, 0) if args.trace else (args.reps, args.warmup)
    rec, gt = make_clouds(args.points, [0.01, 0.02, 0.05])
    out = {"points": args.points, "reps": reps, "warmup": warmup, "bin": os.environ.get("MPMVS_CLOUD_BIN", "1"), "rows": []}
    cKDTree = None
    if not args.no_host and not args.trace:
        try:
            from scipy.spatial import cKDTree
        except ImportError:
            print("scipy is not importable: no host yardstick")
    print(f"{'cloud':>5} {'radius':>7} {'k':>3} {'within':>7} {'defined':>8} {'normals':>8} {'knn_self':>8} {'reduce':>8} {'(build)':>8} {'n/reduce':>8} {'host ms':>9}")
    cloud.estimate_normals(gt[:4096], radii[0], KS[0], device=args.device)   # the first launches of the process: not in the first row's build ms
    for name, pts in (("gt", gt), ("rec", rec)):
        with cloud.Cloud(pts, args.device) as c:
            for radius in radii:
                _, curv, within = c.normals(radius, KS[0], want_within=True)   # builds the grid of this radius
                build_ms = c.normals_ms()[1]
                for k in KS:
                    nm, kn, red = [], [], []
                    for r in range(warmup + reps):   # the three calls alternate
                        _, curv = c.normals(radius, k)
                        if r >= warmup:
                            nm.append(c.normals_ms()[0])
                        c.knn_self(radius, k)
                        if r >= warmup:
                            kn.append(c.knn_ms()[0])
                        cloud.remove_outliers(pts, radius, k=k, device=args.device)
                        if r >= warmup:
                            red.append(cloud.last_outliers_ms())
                    reduce_ms = med(red) - build_ms   # remove_outliers builds the grid of its own handle every time
                    row = {"cloud": name, "radius": radius, "k": k, "n": len(pts), "mean_within": round(float(within.mean()), 2),
                           "defined": int(np.isfinite(curv).sum()), "build_ms": round(build_ms, 4), "normals_ms": round(med(nm), 4),
                           "knn_self_ms": round(med(kn), 4), "outliers_device_ms": round(med(red), 4), "reduce_ms_less_build": round(reduce_ms, 4),
                           "normals_over_reduce": round(med(nm) / reduce_ms, 3) if reduce_ms > 0 else None}
                    if cKDTree is not None:
                        row["host_wall_ms"] = round(host_normals(cKDTree, pts, radius, k) * 1e3, 1)
                        row["host_workers"] = WORKERS
                    out["rows"].append(row)
                    print(f"{name:>5} {radius:7.4g} {k:3d} {row['mean_within']:7.1f} {row['defined']:8d} {med(nm):8.3f} {med(kn):8.3f} {reduce_ms:8.3f} "
                          f"{build_ms:8.3f} {row['normals_over_reduce'] or 0:8.2f} {row.get('host_wall_ms', float('nan')):9.1f}", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
