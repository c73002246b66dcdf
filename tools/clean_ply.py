#!/usr/bin/env python3
"""Removes the "flying" points of a fused cloud on the GPU: a statistical outlier removal (the mean distance to the k nearest
neighbours against mean + std_ratio x sigma over the cloud) and a radius outlier removal (at least min_within neighbours within
the radius), in one pass over the k nearest neighbours (mp-mvs_amd/cloud.py: remove_outliers).

    python tools/clean_ply.py --input A.ply --output B.ply --radius R [--k 16 --std_ratio 2.0 --min_within 0 --device 0]
                              [--cluster_radius C --min_cluster N [--largest K]]

The neighbours are searched within --radius only: a point with fewer than k of them is isolated and removed.  Reads positions,
normals and colours of the `vertex` element (cloud.read_ply) and writes the kept points, in input order, in the reference's 27-byte
records (cloud.write_ply: x y z nx ny nz red green blue); normals or colours the input lacks are written as zeros.
--cluster_radius C --min_cluster N adds the cluster filter (cloud.py: remove_small_clusters) AFTER the outlier
filter, on the points that filter kept: the connected components of "two points are neighbours iff they are within C", of which
those with fewer than N points are dropped, and with --largest K all but the K largest.  It removes the small detached clusters
(a scrap of sky, a reflection) that the outlier rules keep, because inside such a cluster every point has close neighbours.
--std_ratio inf --min_within 0 --k 1 with these flags runs the cluster filter alone (the outlier pass then drops only the points
without any neighbour within --radius).
The last line printed is one JSON line: n, kept, isolated, the mean, sigma and threshold of the mean distances, device ms of the
kernels and wall seconds per stage; with the cluster filter also clusters, largest_cluster, removed_by_cluster and
cluster_device_ms, and kept counts what both filters kept."""
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--input", required=True)
    ap.add_argument("--output", required=True)
    ap.add_argument("--radius", type=float, required=True, help="search radius of the neighbours, in the cloud's units")
    ap.add_argument("--k", type=int, default=16, help="neighbours per point (1 .. 32)")
    ap.add_argument("--std_ratio", type=float, default=2.0, help="threshold = mean + std_ratio x sigma of the mean distances; inf: no statistical test")
    ap.add_argument("--min_within", type=int, default=0, help="neighbours a point needs within the radius; 0: no radius rule")
    ap.add_argument("--cluster_radius", type=float, default=None, help="neighbour radius of the cluster filter; needs --min_cluster")
    ap.add_argument("--min_cluster", type=int, default=None, help="points a connected component needs to stay; needs --cluster_radius")
    ap.add_argument("--largest", type=int, default=None, help="keep only the K largest components (with the cluster filter)")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if not (np.isfinite(args.radius) and args.radius > 0):
        raise SystemExit("--radius needs a finite positive length")
    clusters = args.cluster_radius is not None
    if clusters != (args.min_cluster is not None) or (args.largest is not None and not clusters):
        raise SystemExit("the cluster filter needs --cluster_radius and --min_cluster together; --largest belongs to it")
    if clusters and not (np.isfinite(args.cluster_radius) and args.cluster_radius > 0 and args.min_cluster >= 1 and (args.largest is None or args.largest >= 1)):
        raise SystemExit("--cluster_radius needs a finite positive length, --min_cluster and --largest at least 1")
    t0 = time.perf_counter()
    src = cloud.read_ply(args.input)
    t1 = time.perf_counter()
    res = cloud.remove_outliers(src["xyz"], args.radius, k=args.k, std_ratio=args.std_ratio, min_within=args.min_within, device=args.device)
    keep = res["keep"]
    extra = {}
    if clusters:   # on the points the outlier filter kept
        at = np.flatnonzero(keep)
        cl = cloud.remove_small_clusters(src["xyz"][at], args.cluster_radius, min_size=args.min_cluster, largest=args.largest, device=args.device)
        keep = keep.copy()
        keep[at] = cl["keep"]
        extra = {"clusters": int(cl["counts"][1]), "largest_cluster": int(cl["counts"][2]), "removed_by_cluster": int(len(at) - cl["keep"].sum()),
                 "cluster_device_ms": round(cloud.last_clusters_ms(), 4), "cluster_radius": args.cluster_radius, "min_cluster": args.min_cluster,
                 "largest": args.largest}
    t2 = time.perf_counter()
    sys.stdout.flush()
    cloud.write_ply(args.output, src["xyz"][keep], src["normals"][keep] if "normals" in src else None, src["colors"][keep] if "colors" in src else None)
    t3 = time.perf_counter()
    finite, dense, kept = (int(v) for v in res["counts"])
    kept = int(keep.sum())
    mean, sigma, threshold = (float(v) for v in res["stats"])
    print(json.dumps({"n": int(len(keep)), "kept": kept, "isolated": finite - dense, "nonfinite": int(len(keep)) - finite, "mean": mean, "sigma": sigma,
                      "threshold": threshold if np.isfinite(threshold) else None, "radius": args.radius, "k": args.k, "std_ratio": args.std_ratio if np.isfinite(args.std_ratio) else None,
                      "min_within": args.min_within, "device_ms": round(cloud.last_outliers_ms(), 4),
                      **extra,
                      "seconds": {"read": round(t1 - t0, 4), "filter": round(t2 - t1, 4), "write": round(t3 - t2, 4), "total": round(t3 - t0, 4)}}),
          flush=True)


if __name__ == "__main__":
    main()
