#!/usr/bin/env python3
"""The z-buffer render of a cloud into cameras (cloud.Cloud.render_depth; csrc/pm_render.hpp) on a
synthetic scan of synth.height_field.

Workload: --points points (default 2 M) sampled uniformly over the footprint of the cameras, --views cameras (default 8, the
neighbours of the 3 x 3 grid of synth.make_problem_scene) of --size (default 1600x1200), --splat 1, --occl 0.02, with index maps
(--no-idx: without).

Reports device ms per pass (z-min, index, resolve; HIP events), (point, view) pairs per second through the z-min pass, the
integer atomics per second of the z-min pass (one per in-view pair) and of the index pass (one per point whose z is its
pixel's minimum), the bytes each pass must at least move (z-min: 12 per point, 4 per atomic, 4 per pixel to initialise;
index: 12 per point, 4 read per in-view pair, 4 per atomic, 4 per pixel to initialise; resolve: 4 read and 4 written per
pixel, 4 more per hidden or empty pixel with index maps) and their share of the 8 TB/s HBM peak, the wall time of the call
(downloads of the maps included), and the numpy statement (tests/render_common.py) on the same input, once, with a check that
both agree bit for bit.  Medians of --reps repetitions after --warmup.  --trace: two repetitions and no statement, for
`rocprofv3 --kernel-trace --stats -- python tools/bench_render.py --trace` (never together with counters).
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
import torch  # noqa: F401,E402

import render_common as rc  # noqa: E402

cloud = importlib.import_module("mp-mvs_amd.cloud")
synth = importlib.import_module("mp-mvs_amd.synth")

HBM_PEAK = 8.0e12   # bytes / s


def med(xs):
    return float(np.median(np.asarray(xs, np.float64)))


def make_input(n, views, w, h, spacing=0.15, seed=1):
    rng = np.random.default_rng(seed)
    centers = [(spacing * dx, spacing * dy, 0.0) for dx, dy in synth._RING[:views]]
    while len(centers) < views:   # more than the ring holds: a second ring further out
        k = len(centers)
        centers.append((spacing * 2 * np.cos(k), spacing * 2 * np.sin(k), 0.0))
    cams = synth.scene_cameras(w, h, centers)
    half_x, half_y = 0.5 * w / (0.9 * w) * 5.6 + spacing, 0.5 * h / (0.9 * w) * 5.6 + spacing   # the footprint at the field's depth
    x, y = rng.uniform(-half_x, half_x, n), rng.uniform(-half_y, half_y, n)
    return np.stack([x, y, synth.height_field(x, y)], 1).astype(np.float32), cams


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--size", default="1600x1200")
    ap.add_argument("--splat", type=int, default=1)
    ap.add_argument("--occl", type=float, default=0.02)
    ap.add_argument("--no-idx", action="store_true")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--no-statement", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    w, h = (int(v) for v in args.size.lower().split("x"))
    reps, warmup = (2, 0) if args.trace else (args.reps, args.warmup)
    want_idx = not args.no_idx
    xyz, cams = make_input(args.points, args.views, w, h)
    pixels = args.views * w * h
    out = {"points": args.points, "views": args.views, "size": [w, h], "splat": args.splat, "occl_rel": args.occl, "idx": want_idx, "reps": reps, "warmup": warmup}

    ms = {"zmin": [], "index": [], "resolve": [], "total": []}
    wall = []
    with cloud.Cloud(xyz, args.device) as c:
        for r in range(warmup + reps):
            t0 = time.perf_counter()
            got = c.render_depth(cams, args.splat, args.occl, want_idx=want_idx)
            t1 = time.perf_counter()
            if r >= warmup:
                total, passes = c.render_ms()
                wall.append(t1 - t0)
                ms["total"].append(total)
                for k, v in passes.items():
                    ms[k].append(v)
    depths, idxs = got if want_idx else (got, None)
    covered = sum(int((d != 0).sum()) for d in depths)
    out.update({"ms": {k: round(med(v), 4) for k, v in ms.items()}, "wall_s": round(med(wall), 4), "covered_share": round(covered / pixels, 4)})

    # what the passes did, counted on the host: in-view pairs, and the points whose z is the minimum of their pixel
    pairs = winners = 0
    for cam in cams:
        ok, px, py, z = rc.project(cam, xyz)
        pix = py[ok] * w + px[ok]
        zb = rc.bits(z)[ok]
        zc = np.full(w * h, rc.INF_BITS, np.uint32)
        np.minimum.at(zc, pix, zb)
        pairs += int(ok.sum())
        winners += int((zb == zc[pix]).sum())
    n = args.points
    need = {"zmin": 12 * n + 4 * pairs + 4 * pixels,
            "index": (12 * n + 4 * pairs + 4 * winners + 4 * pixels) if want_idx else 0,
            "resolve": 8 * pixels + (4 * (pixels - covered) if want_idx else 0)}
    z_ms, i_ms = med(ms["zmin"]), med(ms["index"])
    out.update({"in_view_pairs": pairs, "index_atomics": winners if want_idx else 0, "bytes_needed": need,
                "pairs_per_s": round(n * args.views / (z_ms * 1e-3)) if z_ms > 0 else None,
                "zmin_atomics_per_s": round(pairs / (z_ms * 1e-3)) if z_ms > 0 else None,
                "index_atomics_per_s": round(winners / (i_ms * 1e-3)) if want_idx and i_ms > 0 else None,
                "hbm_share": {k: (round(need[k] / (med(ms[k]) * 1e-3) / HBM_PEAK, 5) if med(ms[k]) > 0 else None) for k in need}})
    print(f"{args.points} points x {args.views} views of {w} x {h}, splat {args.splat}, occl_rel {args.occl:g}, idx {want_idx}: "
          f"{pairs} pairs in view, {100 * covered / pixels:.2f} % of the pixels covered")
    print(f"{'pass':>8} {'ms':>9} {'MB needed':>10} {'HBM share':>9}")
    for k in ("zmin", "index", "resolve"):
        print(f"{k:>8} {med(ms[k]):9.3f} {need[k] / 1e6:10.1f} {100 * (out['hbm_share'][k] or 0):8.2f}%")
    print(f"z-min: {n * args.views / z_ms / 1e6 if z_ms > 0 else 0:.1f} G (point, view) pairs / s, {pairs / z_ms / 1e6 if z_ms > 0 else 0:.2f} G atomicMin / s; "
          f"index: {winners / i_ms / 1e6 if want_idx and i_ms > 0 else 0:.2f} G atomicMin / s")
    print(f"render_depth(): {med(wall) * 1e3:.1f} ms wall (median of {len(wall)}), {med(ms['total']):.3f} ms of it in kernels")

    if not args.trace and not args.no_statement:
        t0 = time.perf_counter()
        wd, wi = rc.render_statement(xyz, cams, args.splat, args.occl)
        out["statement_wall_s"] = round(time.perf_counter() - t0, 4)
        same = all(np.array_equal(rc.bits(a), rc.bits(b)) for a, b in zip(depths, wd)) and (idxs is None or all(np.array_equal(a, b) for a, b in zip(idxs, wi)))
        out["equals_statement"] = bool(same)
        print(f"numpy statement, one thread: {out['statement_wall_s'] * 1e3:.1f} ms wall; bit for bit equal: {same}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
