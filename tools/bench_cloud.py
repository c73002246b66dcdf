#!/usr/bin/env python3
"""The cloud score (mp-mvs_amd/cloud.py: evaluate; csrc/pm_cloud.hpp) on two synthetic clouds sampled from synth.height_field.

Workload: --points points each (default 2 M), spacing about 0.4 x the smallest tolerance; the second cloud ("reconstruction") is
sampled at other positions, displaced by Gaussian noise of half the middle tolerance per axis, and 2 % of its points are uniform
outliers in the bounding box -- the queries that find nothing.

Per level of the cascade (reconstruction -> ground truth): grid build ms and query ms (HIP events; the query figure includes the
binning of the queries), queries per second, occupied cells and the fullest cell, the bytes the query kernel must at least move
(per query 12 read + 4 written + the 4-byte order entry, and the 16-byte record of every target once) and their share of the
8 TB/s HBM peak.  Then the wall time of evaluate() (both directions, uploads and downloads included) and, where scipy is
importable, the same distances from scipy.spatial.cKDTree with 16 workers (the CPU quota of the GPU machines) and a check that
both agree.  Medians of --reps repetitions after --warmup.  --trace: two repetitions only, for
`rocprofv3 --kernel-trace --stats -- python tools/bench_cloud.py --trace` (never together with counters).
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
import torch  # noqa: F401,E402

cloud = importlib.import_module("mp-mvs_amd.cloud")
synth = importlib.import_module("mp-mvs_amd.synth")

HBM_PEAK = 8.0e12   # bytes / s
WORKERS = 16


def make_clouds(n, tol, seed=1):
    rng = np.random.default_rng(seed)
    side = np.sqrt(n) * 0.4 * min(tol)
    mid = sorted(tol)[len(tol) // 2]

    def sample(m):
        x, y = rng.uniform(0, side, m), rng.uniform(0, side, m)
        return np.stack([x, y, synth.height_field(x, y)], 1)

    gt = sample(n)
    n_out = n // 50
    rec = sample(n - n_out) + rng.normal(0, 0.5 * mid, (n - n_out, 3))
    lo, hi = gt.min(0), gt.max(0)
    rec = np.concatenate([rec, rng.uniform(lo, hi, (n_out, 3))])
    return rec[rng.permutation(n)].astype(np.float32), gt.astype(np.float32)


def med(xs):
    return float(np.median(np.asarray(xs, np.float64)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--tolerances", default="0.01,0.02,0.05")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--no-kdtree", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    tol = sorted(float(t) for t in args.tolerances.split(","))
    reps, warmup = (2, 0) if args.trace else (args.reps, args.warmup)
    rec, gt = make_clouds(args.points, tol)
    out = {"points": args.points, "tolerances": tol, "reps": reps, "warmup": warmup, "bin": os.environ.get("MPMVS_CLOUD_BIN", "1"), "levels": []}

    # the cascade of one direction, level by level
    rows = {t: {"build_ms": [], "query_ms": []} for t in tol}
    for r in range(warmup + reps):
        def on_level(t, nq, cl):
            q_ms, b_ms = cl.kernel_ms()
            if r >= warmup:
                rows[t]["build_ms"].append(b_ms)
                rows[t]["query_ms"].append(q_ms)
            rows[t]["n_queries"] = nq
            rows[t]["stats"] = cl.stats()
        with cloud.Cloud(gt, args.device) as c:   # a fresh handle per repetition: a handle keeps its grids, and a kept grid has build ms 0
            d_rec = cloud.distances(rec, c, tol, on_level)
    print(f"{'tolerance':>9} {'queries':>9} {'build ms':>9} {'query ms':>9} {'Mq/s':>8} {'cells':>9} {'fullest':>7} {'MB needed':>9} {'HBM share':>9}")
    for t in tol:
        row = rows[t]
        if "stats" not in row:
            continue
        st, nq = row["stats"], row["n_queries"]
        q_ms, b_ms = med(row["query_ms"]), med(row["build_ms"])
        need = nq * 20 + 16 * st["finite"]
        lvl = {"tolerance": t, "n_queries": nq, "build_ms": round(b_ms, 4), "query_ms": round(q_ms, 4), "queries_per_s": round(nq / (q_ms * 1e-3)) if q_ms > 0 else None,
               "cells": st["cells"], "fullest": st["fullest"], "slots": st["slots"], "bytes_needed": need,
               "hbm_share": round(need / (q_ms * 1e-3) / HBM_PEAK, 5) if q_ms > 0 else None}
        out["levels"].append(lvl)
        print(f"{t:9.4g} {nq:9d} {b_ms:9.3f} {q_ms:9.3f} {nq / q_ms / 1e3 if q_ms > 0 else 0:8.1f} {st['cells']:9d} {st['fullest']:7d} {need / 1e6:9.1f} "
              f"{100 * (lvl['hbm_share'] or 0):8.2f}%", flush=True)

    wall = []
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        res = cloud.evaluate(rec, gt, tol, device=args.device)
        if r >= warmup:
            wall.append(time.perf_counter() - t0)
    out["evaluate_wall_s"] = round(med(wall), 4)
    out["score"] = [{k: (round(v, 5) if isinstance(v, float) else v) for k, v in row.items()} for row in res["tolerances"]]
    print(f"evaluate(): {med(wall) * 1e3:.1f} ms wall (median of {len(wall)}); F1 " + ", ".join(f"{r['f1']:.4f} @ {r['tolerance']:g}" for r in res["tolerances"]))

    if not args.no_kdtree and not args.trace:
        try:
            from scipy.spatial import cKDTree
        except ImportError:
            cKDTree = None
            print("scipy is not importable: no k-d tree yardstick")
        if cKDTree is not None:
            times = []
            for r in range(3):
                t0 = time.perf_counter()
                d_a, _ = cKDTree(gt).query(rec, k=1, distance_upper_bound=tol[-1], workers=WORKERS)
                d_b, _ = cKDTree(rec).query(gt, k=1, distance_upper_bound=tol[-1], workers=WORKERS)
                times.append(time.perf_counter() - t0)
            out["ckdtree_wall_s"] = round(med(times), 4)
            out["ckdtree_workers"] = WORKERS
            # the tree works on the fp32 coordinates in fp64: distances agree to fp32 rounding, and "found" agrees off the boundary
            both = np.isfinite(d_a) & np.isfinite(d_rec)
            out["ckdtree_max_abs_diff"] = float(np.abs(d_a[both] - d_rec[both]).max()) if both.any() else 0.0
            out["ckdtree_found_mismatch"] = int((np.isfinite(d_a) != np.isfinite(d_rec)).sum())
            print(f"cKDTree, {WORKERS} workers, both directions (build + query): {med(times) * 1e3:.1f} ms wall (median of {len(times)}); "
                  f"max |difference| {out['ckdtree_max_abs_diff']:.2e}, found / not found differs for {out['ckdtree_found_mismatch']} queries")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
