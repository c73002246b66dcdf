#!/usr/bin/env python3
"""The connected components of a cloud (mp-mvs_amd/cloud.py: Cloud.components; csrc/pm_components.hpp) on the two synthetic clouds
of tools/bench_cloud.py (--points points each, default 2 M, spacing about 0.004) at three radii (default: bench_cloud's tolerances).

Per cloud and radius: the neighbours per point (mean of `within`), the grid-build ms, the device ms (HIP events) of the three passes
-- hook (the initialisation, the binning and the union-find pass over the edges), flatten, size -- and their sum, the components
found and the largest one, and beside them the device ms of knn_self(k = 1, want_within = True) at the same radius, measured in the
same process, alternating with it: the same 27-cell walk over the same candidates without the union-find.  Then, where scipy is
importable, the host wall ms of the same answer from scipy.spatial.cKDTree(points).query_pairs(radius) and
scipy.sparse.csgraph.connected_components, build included, once, and a check that both find the same partition -- only where the
cloud has at most --kdtree-max-pairs adjacent pairs (default 30 M): the list of pairs takes 16 bytes each.
Medians of --reps repetitions after --warmup.  --trace: two repetitions only and no k-d tree, for
`rocprofv3 --kernel-trace --stats -- python tools/bench_components.py --trace` (never together with counters).
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
from bench_cloud import make_clouds, med  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--radii", default="0.01,0.02,0.05")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--no-kdtree", action="store_true")
    ap.add_argument("--kdtree-max-pairs", type=float, default=3.0e7)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    radii = sorted(float(r) for r in args.radii.split(","))
    reps, warmup = (2, 0) if args.trace else (args.reps, args.warmup)
    rec, gt = make_clouds(args.points, [0.01, 0.02, 0.05])
    out = {"points": args.points, "reps": reps, "warmup": warmup, "bin": os.environ.get("MPMVS_CLOUD_BIN", "1"), "rows": []}
    have_scipy = False
    if not args.no_kdtree and not args.trace:
        try:
            from scipy.sparse import coo_matrix
            from scipy.sparse.csgraph import connected_components
            from scipy.spatial import cKDTree
            have_scipy = True
        except ImportError:
            print("scipy is not importable: no k-d tree yardstick")
    print(f"{'cloud':>5} {'radius':>7} {'within':>7} {'build ms':>8} {'hook':>8} {'flatten':>8} {'size':>8} {'total':>8} {'knn k=1':>8} {'hook/knn':>8} "
          f"{'components':>10} {'largest':>8} {'kdtree ms':>9}")
    for name, pts in (("gt", gt), ("rec", rec)):
        with cloud.Cloud(pts, args.device) as c:
            for radius in radii:
                _, _, within = c.knn_self(radius, 1, want_idx=False, want_within=True)   # builds the grid of this radius
                build_ms = c.knn_ms()[1]
                ms = {"hook": [], "flatten": [], "size": [], "total": [], "knn": []}
                for r in range(warmup + reps):   # interleaved rounds in one process
                    label, _, counts = c.components(radius)
                    total, _, passes = c.components_ms(passes=True)
                    c.knn_self(radius, 1, want_idx=False, want_within=True)
                    if r >= warmup:
                        for k, v in passes.items():
                            ms[k].append(v)
                        ms["total"].append(total)
                        ms["knn"].append(c.knn_ms()[0])
                m = {k: med(v) for k, v in ms.items()}
                pairs = int(within.astype(np.int64).sum()) // 2
                row = {"cloud": name, "radius": radius, "n": len(pts), "mean_within": round(float(within.mean()), 2), "pairs": pairs, "build_ms": round(build_ms, 4),
                       "hook_ms": round(m["hook"], 4), "flatten_ms": round(m["flatten"], 4), "size_ms": round(m["size"], 4), "total_ms": round(m["total"], 4),
                       "knn_self_k1_ms": round(m["knn"], 4), "hook_over_knn": round(m["hook"] / m["knn"], 3) if m["knn"] > 0 else None,
                       "components": int(counts[1]), "largest": int(counts[2])}
                if have_scipy and pairs <= args.kdtree_max_pairs:
                    t0 = time.perf_counter()
                    e = cKDTree(pts).query_pairs(radius, output_type="ndarray")
                    n = len(pts)
                    ncomp, lab = connected_components(coo_matrix((np.ones(len(e), np.int8), (e[:, 0], e[:, 1])), shape=(n, n)), directed=False)
                    row["kdtree_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                    # the tree measures in fp64: a pair within rounding of the radius can differ, so the partitions are compared, not assumed
                    first = np.full(ncomp, n, np.int64)
                    np.minimum.at(first, lab, np.arange(n))
                    row["kdtree_components"] = int(ncomp)
                    row["kdtree_labels_differ"] = int((first[lab] != label).sum())
                out["rows"].append(row)
                print(f"{name:>5} {radius:7.4g} {row['mean_within']:7.1f} {build_ms:8.3f} {m['hook']:8.3f} {m['flatten']:8.3f} {m['size']:8.3f} {m['total']:8.3f} "
                      f"{m['knn']:8.3f} {row['hook_over_knn'] or 0:8.2f} {row['components']:10d} {row['largest']:8d} {row.get('kdtree_wall_ms', float('nan')):9.1f}", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
