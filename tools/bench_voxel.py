#!/usr/bin/env python3
"""The voxel-grid downsampling (mp-mvs_amd/cloud.py: voxel_downsample; csrc/pm_voxel.hpp) on the two synthetic clouds of
tools/bench_cloud.py (--points points each, default 2 M, spacing about 0.004) at three voxel sizes (default: half of bench_cloud's
tolerances, as Tanks and Temples takes half its tolerance).

Per cloud and voxel size: m, device ms per pass (HIP events: insert, first, flag + scan, number, accumulate, finish) and their sum,
the bytes the passes must at least move and their share of the 8 TB/s HBM peak over that sum, the 64-bit integer atomics per
second of the accumulate pass (three per finite point: the clouds carry no normals or colours), the wall time of the call (uploads
and downloads included), the grid-build ms of mpmvs_cloud_nearest for the same cloud with radius = voxel (it shares its first
pass with the downsampling), and the wall time of the numpy statement (tests/voxel_common.py) with a check that both agree in
every bit.  Medians of --reps repetitions after --warmup.  --trace: two repetitions only and no statement, for
`rocprofv3 --kernel-trace --stats -- python tools/bench_voxel.py --trace` (never together with counters).
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: F401,E402

cloud = importlib.import_module("mp-mvs_amd.cloud")
from bench_cloud import HBM_PEAK, make_clouds, med  # noqa: E402

PASSES = ("insert", "first", "scan", "number", "accumulate", "finish")


def bytes_needed(n, m):
    """the least each pass moves for n finite points in m voxels, no normals or colours, no map"""
    return {"insert": 16 * n + 12 * m,        # xyz read, slot_of written; a key and a count per occupied slot
            "first": 4 * n + 4 * m,           # slot_of read; first per slot
            "scan": 28 * n,                   # slot_of and first read, the flag written; flags read, numbers written; numbers read and written
            "number": 8 * n + 20 * m,         # flag and number read; per leader slot_of, count, vox_of_slot, out_first, out_count
            "accumulate": 20 * n + 24 * n,    # xyz, slot_of, vox_of_slot read; three 64-bit atomics
            "finish": 56 * m}                 # S, first, count, the leader's xyz read; out_xyz written


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--voxels", default="0.005,0.01,0.025")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--no-statement", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    voxels = sorted(float(v) for v in args.voxels.split(","))
    reps, warmup = (2, 0) if args.trace else (args.reps, args.warmup)
    rec, gt = make_clouds(args.points, [0.01, 0.02, 0.05])
    out = {"points": args.points, "reps": reps, "warmup": warmup, "rows": []}
    print(f"{'cloud':>5} {'voxel':>7} {'m':>8} " + " ".join(f"{p[:6]:>7}" for p in PASSES) + f" {'sum ms':>7} {'MB':>7} {'HBM':>6} {'Gatom/s':>7} {'wall ms':>8} "
          f"{'build ms':>8} {'numpy s':>8}")
    for name, pts in (("gt", gt), ("rec", rec)):
        for v in voxels:
            ms = {p: [] for p in PASSES}
            wall = []
            for r in range(warmup + reps):
                t0 = time.perf_counter()
                res = cloud.voxel_downsample(pts, v, device=args.device)
                t1 = time.perf_counter()
                if r >= warmup:
                    wall.append(t1 - t0)
                    for p, x in cloud.last_voxel_ms(passes=True)[1].items():
                        ms[p].append(x)
            m, n = len(res["xyz"]), len(pts)
            pm = {p: med(ms[p]) for p in PASSES}
            total = sum(pm.values())
            need = bytes_needed(n, m)
            with cloud.Cloud(pts, args.device) as c:   # a fresh handle: a kept grid has build ms 0
                c.nearest(pts[:1], v, want_idx=False)
                build_ms = c.kernel_ms()[1]
            row = {"cloud": name, "voxel": v, "n": n, "m": m, "pass_ms": {p: round(pm[p], 4) for p in PASSES}, "sum_ms": round(total, 4),
                   "bytes_needed": sum(need.values()), "hbm_share": round(sum(need.values()) / (total * 1e-3) / HBM_PEAK, 5) if total > 0 else None,
                   "pass_hbm_share": {p: round(need[p] / (pm[p] * 1e-3) / HBM_PEAK, 5) if pm[p] > 0 else None for p in PASSES},
                   "atomics_per_s": round(3 * n / (pm["accumulate"] * 1e-3)) if pm["accumulate"] > 0 else None, "wall_ms": round(med(wall) * 1e3, 3),
                   "nearest_build_ms": round(build_ms, 4)}
            if not args.trace and not args.no_statement:
                from voxel_common import assert_same, statement
                t0 = time.perf_counter()
                want = statement(pts, v)
                row["statement_s"] = round(time.perf_counter() - t0, 3)
                want.pop("voxel_of")
                assert_same(res, want, f"{name} at {v}")
                row["equal_bits"] = True
            out["rows"].append(row)
            print(f"{name:>5} {v:7.4g} {m:8d} " + " ".join(f"{pm[p]:7.3f}" for p in PASSES) + f" {total:7.3f} {sum(need.values()) / 1e6:7.1f} "
                  f"{100 * (row['hbm_share'] or 0):5.1f}% {(row['atomics_per_s'] or 0) / 1e9:7.2f} {row['wall_ms']:8.2f} {build_ms:8.3f} "
                  f"{row.get('statement_s', float('nan')):8.3f}", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
