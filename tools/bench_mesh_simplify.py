#!/usr/bin/env python3
"""Device and wall times of simplifying a mesh on the GPU by vertex clustering (mp-mvs_amd/mesh.py: Mesh.simplify;
csrc/pm_simplify.hpp), on the mesh of tools/bench_tsdf.py's synthetic height field.

    python tools/bench_mesh_simplify.py [--sizes 256,512] [--cells 2,4,8] [--views 8] [--size 1600x1200] [--reps 5] [--warmup 1] [--trace]

Per size n the views are integrated into an n^3 volume and meshed (about 0.5 M triangles at 256, 2.0 M at 512).  Then, per cell of
--cells voxels and per placement (mean, quadric), --reps times after --warmup (medians): Mesh.simplify on one resident handle.
Reported: device ms per pass (HIP events), n' / n and m' / m, the clusters by `placed`, the 64-bit integer terms per second of the
quadric pass (the statement's 30 per triangle -- ten sums at each of three corners -- counted whether a term is 0 and skipped or
merged with another corner's in the thread), the wall ms of the call (with its downloads).  Beside them, on the host, once per size and cell: the numpy statement of tests/mesh_simplify_common.py
for the quadric placement, its seconds, and whether the device result equals it bit for bit.
--trace: two repetitions and no host statement, for `rocprofv3 --kernel-trace --stats -- python tools/bench_mesh_simplify.py --trace`
(never together with counters).  Prints the table and one JSON line.  There is no target figure."""
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

import mesh_simplify_common as msc  # noqa: E402

mesh = importlib.import_module("mp-mvs_amd.mesh")
synth = importlib.import_module("mp-mvs_amd.synth")


def med(xs):
    return float(np.median(np.asarray(xs, np.float64)))


def surface(n, cams, depths, device, side=5.6, centre=(0.0, 0.0, 5.0)):
    voxel = side / (n - 1)
    with mesh.Volume(tuple(c - 0.5 * side for c in centre), voxel, (n, n, n), 4 * voxel, device=device) as v:
        v.integrate(cams, depths)
        return v.mesh(1), voxel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--cells", default="2,4,8", help="cell edges in voxels")
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--size", default="1600x1200")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    w, h = (int(v) for v in args.size.lower().split("x"))
    reps, warmup = (2, 0) if args.trace else (args.reps, args.warmup)
    if not 1 <= args.views <= 9:
        raise SystemExit("--views must lie in 1..9")
    scene = synth.make_problem_scene(w, h, n_src=max(args.views - 1, 1), quantize=True)
    views = scene.views[:args.views]
    cams, depths = [v.cam for v in views], [v.gt_depth for v in views]
    out = {"views": args.views, "size": [w, h], "reps": reps, "warmup": warmup, "sizes": {}}
    print(f"{'n':>5} {'cell':>5} {'placement':>9} " + " ".join(f"{p[:9]:>9}" for p in mesh.SIMPLIFY_PASSES) + f" {'sum ms':>8} {'wall ms':>8} {'n_out/n':>8} {'m_out/m':>8}")
    for n in (int(s) for s in args.sizes.split(",") if s.strip()):
        m, voxel = surface(n, cams, depths, args.device)
        nv, nt = len(m["xyz"]), len(m["tri"])
        res = {"vertices": nv, "triangles": nt, "cells": {}}
        with mesh.Mesh(m["xyz"], m["tri"], m.get("rgb"), device=args.device) as hd:
            hd.components(want_verts=False, want_tris=False)   # the upload of the mesh is not part of any timed call
            for cells in (float(s) for s in args.cells.split(",") if s.strip()):
                cell = float(np.float32(cells * voxel))
                per = {}
                for placement in ("mean", "quadric"):
                    ms, wall, got = {k: [] for k in mesh.SIMPLIFY_PASSES}, [], None
                    for r in range(warmup + reps):
                        t0 = time.perf_counter()
                        got = hd.simplify(cell, placement)
                        t1 = time.perf_counter()
                        p = hd.simplify_ms()
                        if r >= warmup:
                            wall.append(t1 - t0)
                            for k in ms:
                                ms[k].append(p[k])
                    ms = {k: med(v) for k, v in ms.items()}
                    total = sum(ms.values())
                    atomics = 30 * nt / (ms["quadric_accumulate"] * 1e-3) if ms["quadric_accumulate"] > 0 else None
                    per[placement] = {"ms": {k: round(v, 4) for k, v in ms.items()}, "device_ms": round(total, 4), "wall_ms": round(1e3 * med(wall), 3),
                                      "clusters": int(len(got["xyz"])), "triangles_out": int(len(got["tri"])), "counts": got["counts"],
                                      "placed": [int((got["placed"] == q).sum()) for q in range(3)], "quadric_atomics_per_s": round(atomics) if atomics else None}
                    print(f"{n:>5} {cells:>5g} {placement:>9} " + " ".join(f"{ms[k]:9.4f}" for k in mesh.SIMPLIFY_PASSES)
                          + f" {total:8.3f} {1e3 * med(wall):8.2f} {len(got['xyz']) / nv:8.4f} {len(got['tri']) / max(nt, 1):8.4f}")
                    if placement == "quadric":
                        print(f"{'':>21} placed {per[placement]['placed']}, counts {got['counts']}, {(atomics or 0) / 1e9:.2f} G terms / s in the quadric pass")
                        if not args.trace:
                            t0 = time.perf_counter()
                            want = msc.statement(m, cell, 1)
                            t_host = time.perf_counter() - t0
                            try:
                                msc.assert_same(got, want, f"{n} {cells}")
                                equal = True
                            except AssertionError as e:
                                equal = False
                                print(e)
                            per["host"] = {"numpy_statement_s": round(t_host, 2), "equal": equal}
                            print(f"{'':>21} host: the numpy statement takes {t_host:.2f} s; the device result equals it: {equal}")
                res["cells"][f"{cells:g}"] = per
        out["sizes"][str(n)] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
