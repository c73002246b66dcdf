#!/usr/bin/env python3
"""The range cube maps of a scan's scanners and the classification of points against them (cloud.Observer; csrc/pm_observe.hpp;
DESIGN.md section 21) on the synthetic scan of tools/bench_cloud.py.

Workload: the --points (default 2 M) ground-truth points of bench_cloud.make_clouds as the scan, --scanners (default 8) positions
spread over it between the surface and the origin, --face 1024, --window 1, and the reconstruction of make_clouds (as many points,
noisy, 2 % outliers) as the queries, at rel 0.02 / abs 0.

Reports device ms per pass (z-min and window minimum of the constructor, classify; HIP events), (point, scanner) atomicMin per
second of the z-min pass beside the 26.5 G/s of the render's z-min pass, (query, scanner) lookups per second
of the classify pass, the bytes each pass must at least move (z-min: 12 per point, 4 per atomic, 4 per pixel to initialise; window
minimum: 4 read and 4 written per pixel; classify: 12 per query, 4 per lookup, 8 written per query) and their share of the 8 TB/s
HBM peak, the wall time of the constructor and of classify() (uploads and downloads included), and the numpy statement
(tests/observe_common.py) on the same input, once, with a check that maps and counts agree bit for bit.  Medians of --reps
repetitions after --warmup.  --trace: two repetitions and no statement, for
`rocprofv3 --kernel-trace --stats -- python tools/bench_observe.py --trace` (never together with counters).
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: F401,E402

import observe_common as oc  # noqa: E402
from bench_cloud import HBM_PEAK, make_clouds, med  # noqa: E402

cloud = importlib.import_module("mp-mvs_amd.cloud")

RENDER_ZMIN_ATOMICS_PER_S = 26.5e9   # DESIGN.md section 14, "Measured"


def make_scanners(scan, m, seed=2):
    """m positions over the middle of the scan's footprint, 40 % to 60 % of the way from the surface to z = 0"""
    rng = np.random.default_rng(seed)
    lo, hi = scan.min(0).astype(np.float64), scan.max(0).astype(np.float64)
    xy = rng.uniform(lo[:2] + 0.25 * (hi[:2] - lo[:2]), hi[:2] - 0.25 * (hi[:2] - lo[:2]), (m, 2))
    z = rng.uniform(0.4, 0.6, m) * lo[2]
    return np.concatenate([xy, z[:, None]], 1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--scanners", type=int, default=8)
    ap.add_argument("--face", type=int, default=1024)
    ap.add_argument("--window", type=int, default=1)
    ap.add_argument("--rel", type=float, default=0.02)
    ap.add_argument("--abs", type=float, default=0.0, dest="abs_margin")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--no-statement", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    reps, warmup = (2, 0) if args.trace else (args.reps, args.warmup)
    q, scan = make_clouds(args.points, [0.01, 0.02, 0.05])
    scanners = make_scanners(scan, args.scanners)
    n, ns, R = len(scan), args.scanners, args.face
    pixels = ns * 6 * R * R
    out = {"points": n, "queries": len(q), "scanners": ns, "face_size": R, "window": args.window, "rel": args.rel, "abs": args.abs_margin, "reps": reps,
           "warmup": warmup}

    ms = {"zmin": [], "near": [], "classify": []}
    wall = {"create": [], "classify": []}
    with cloud.Cloud(scan, args.device) as c:
        for r in range(warmup + reps):
            t0 = time.perf_counter()
            obs = cloud.Observer(c, scanners, None, R, args.window)
            t1 = time.perf_counter()
            free, cov = obs.classify(q, args.rel, args.abs_margin)
            t2 = time.perf_counter()
            if r >= warmup:
                k_ms, build = obs.ms()
                ms["zmin"].append(build["zmin"]), ms["near"].append(build["near"]), ms["classify"].append(k_ms)
                wall["create"].append(t1 - t0), wall["classify"].append(t2 - t1)
            if r + 1 < warmup + reps:
                obs.close()
    stats = obs.stats()
    maps = [obs.near_map(j) for j in range(ns)] if not (args.trace or args.no_statement) else None
    obs.close()

    # what the passes did, counted on the host: the (point, scanner) pairs that take part, and the same of the queries
    pairs = sum(int(oc.locate(scan, S, R)[0].sum()) for S in scanners)
    lookups = sum(int(oc.locate(q, S, R)[0].sum()) for S in scanners)
    need = {"zmin": 12 * n + 4 * pairs + 4 * pixels, "near": 8 * pixels, "classify": 12 * len(q) + 4 * lookups + 8 * len(q)}
    m = {k: med(v) for k, v in ms.items()}
    out.update({"ms": {k: round(v, 4) for k, v in m.items()}, "wall_s": {k: round(med(v), 4) for k, v in wall.items()}, **stats,
                "pairs": pairs, "lookups": lookups, "bytes_needed": need,
                "zmin_atomics_per_s": round(pairs / (m["zmin"] * 1e-3)) if m["zmin"] > 0 else None,
                "render_zmin_atomics_per_s": RENDER_ZMIN_ATOMICS_PER_S,
                "lookups_per_s": round(lookups / (m["classify"] * 1e-3)) if m["classify"] > 0 else None,
                "hbm_share": {k: (round(need[k] / (m[k] * 1e-3) / HBM_PEAK, 5) if m[k] > 0 else None) for k in need},
                "free_share": round(float((free >= 1).mean()), 4), "covered_share": round(float((cov >= 1).mean()), 4)})
    print(f"{n} scan points, {ns} scanners, faces of {R} x {R}, window {args.window}: {pairs} pairs, "
          f"{100 * stats['covered_pixels'] / pixels:.2f} % of {pixels} pixels hold a range; {len(q)} queries, {lookups} lookups, "
          f"{100 * out['covered_share']:.1f} % covered, {100 * out['free_share']:.1f} % in free space")
    print(f"{'pass':>9} {'ms':>9} {'MB needed':>10} {'HBM share':>9}")
    for k in ("zmin", "near", "classify"):
        print(f"{k:>9} {m[k]:9.3f} {need[k] / 1e6:10.1f} {100 * (out['hbm_share'][k] or 0):8.2f}%")
    print(f"z-min: {pairs / m['zmin'] / 1e6 if m['zmin'] > 0 else 0:.2f} G atomicMin / s (render: {RENDER_ZMIN_ATOMICS_PER_S / 1e9:.1f}); "
          f"classify: {lookups / m['classify'] / 1e6 if m['classify'] > 0 else 0:.2f} G lookups / s")
    print(f"Observer(): {med(wall['create']) * 1e3:.1f} ms wall, classify(): {med(wall['classify']) * 1e3:.1f} ms wall (medians of {len(wall['create'])})")

    if maps is not None:
        t0 = time.perf_counter()
        Zn = oc.maps(scan, scanners, R, args.window)[1]
        t1 = time.perf_counter()
        wf, wc = oc.classify(q, scanners, Zn, args.rel, args.abs_margin)
        t2 = time.perf_counter()
        same = all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(maps, Zn)) and np.array_equal(free, wf) and np.array_equal(cov, wc)
        out.update({"statement_wall_s": {"maps": round(t1 - t0, 4), "classify": round(t2 - t1, 4)}, "equals_statement": bool(same)})
        print(f"numpy statement, one thread: maps {1e3 * (t1 - t0):.1f} ms, classify {1e3 * (t2 - t1):.1f} ms wall; bit for bit equal: {same}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
