#!/usr/bin/env python3
"""Device time of mpmvs_surface_render_depth (mesh.Mesh.render_depth; csrc/pm_raster.hpp).

    python tools/bench_mesh_render.py [--sizes 256,512] [--views 8] [--size 1600x1200] [--reps 3] [--warmup 1] [--cell 4]
                                      [--sweep 0,16,64,128,256,512,1024,4096,1073741824] [--statement-triangles 3000] [--trace]

The meshes are those of tools/bench_tsdf.py: the synthetic height field seen by --views cameras of --size, integrated into a dense
TSDF volume of n^3 voxels and meshed; and their simplifications (mesh.simplify on a grid of --cell voxels).  Each is rendered into the
same cameras.  Per mesh: the device ms of the four passes (medians of --reps runs after --warmup), (triangle, view) pairs per second,
the pixels of the boxes the pairs were tested in and the atomic minima issued (the kernels' own counters, Mesh.render_work), atomics
per second, the pixels covered, and the pairs that took the large path.
Beside it mpmvs_cloud_render_depth on the same mesh's vertices (splat 1, occl 0.02): the neighbouring number.  --sweep: the threshold
MPMVS_RASTER_LARGE over the given values on every mesh.  One triangle that fills the image is timed on its own.  The numpy statement
renders the first --statement-triangles triangles of the smallest simplified mesh into the first camera at 160 x 120; the device's
maps are compared with it bit for bit (the statement is tests/mesh_render_common.py, as tools/bench_tsdf.py takes its own from tests/;
without that folder the bench runs with --statement-triangles 0).  --trace: two repetitions, no sweep and no statement, for
`rocprofv3 --kernel-trace --stats -- python tools/bench_mesh_render.py --trace` (never together with counters).
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

mesh = importlib.import_module("mp-mvs_amd.mesh")
cloud = importlib.import_module("mp-mvs_amd.cloud")
synth = importlib.import_module("mp-mvs_amd.synth")
depthmap = importlib.import_module("mp-mvs_amd.depthmap")

PASSES = ("init", "small", "large", "resolve")


def med(xs):
    return float(np.median(np.asarray(xs, np.float64)))


def box(n, side=5.6, centre=(0.0, 0.0, 5.0)):
    voxel = side / (n - 1)
    return tuple(c - 0.5 * side for c in centre), voxel


def timed(h, cams, reps, warmup, want_tri=True):
    ms = {k: [] for k in PASSES + ("total",)}
    wall = []
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        h.render_depth(cams, want_tri=want_tri)
        t1 = time.perf_counter()
        total, p = h.render_ms()
        if r >= warmup:
            for k in PASSES:
                ms[k].append(p[k])
            ms["total"].append(total)
            wall.append(t1 - t0)
    return {k: round(med(v), 4) for k, v in ms.items()}, round(med(wall), 4), dict(h.last_render_counts, **h.render_work())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--size", default="1600x1200")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cell", type=float, default=4.0, help="the simplification's cell in voxels")
    ap.add_argument("--sweep", default="0,16,64,128,256,512,1024,4096,1073741824")
    ap.add_argument("--statement-triangles", type=int, default=3000)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    w, h = (int(v) for v in args.size.lower().split("x"))
    sizes = [int(s) for s in args.sizes.split(",") if s.strip()]
    sweep = [] if args.trace else [int(s) for s in args.sweep.split(",") if s.strip()]
    reps, warmup = (2, 0) if args.trace else (max(args.reps, 3), args.warmup)
    if not 1 <= args.views <= 9:
        raise SystemExit("--views must lie in 1..9")
    os.environ.pop("MPMVS_RASTER_LARGE", None)
    sc = synth.make_problem_scene(w, h, n_src=max(args.views - 1, 1), quantize=True)
    views = sc.views[:args.views]
    cams, depths = [v.cam for v in views], [v.gt_depth for v in views]
    out = {"views": args.views, "size": [w, h], "reps": reps, "warmup": warmup, "meshes": {}, "sweep": {}}
    meshes = {}
    for n in sizes:
        origin, voxel = box(n)
        with mesh.Volume(origin, voxel, (n, n, n), 4 * voxel, device=args.device) as v:
            v.integrate(cams, depths)
            full = v.mesh(1)
        meshes[f"{n} full"] = full
        simp = mesh.simplify(full, args.cell * voxel, device=args.device)
        meshes[f"{n} simplified"] = {"xyz": simp["xyz"], "tri": simp["tri"], "rgb": None}
    print(f"{args.views} views of {w} x {h}; medians of {reps} runs after {warmup} warm-up; threshold {os.environ.get('MPMVS_RASTER_LARGE', 'default')}")
    print(f"{'mesh':>16} {'triangles':>10} {'init':>8} {'small':>8} {'large':>8} {'resolve':>8} {'total':>8} {'Mpairs/s':>9} {'large pairs':>12} {'covered':>10} {'points ms':>10} {'box Mpix':>9} {'Matomics':>9}")
    for name, m in meshes.items():
        with mesh.Mesh(m["xyz"], m["tri"], device=args.device) as hm:
            ms, wall, counts = timed(hm, cams, reps, warmup)
            rows = {}
            for T in sweep:
                os.environ["MPMVS_RASTER_LARGE"] = str(T)
                rows[str(T)] = dict(timed(hm, cams, reps, warmup)[0], large_pairs=hm.last_render_counts["large_pairs"])
            os.environ.pop("MPMVS_RASTER_LARGE", None)
        pts = []
        with cloud.Cloud(m["xyz"], args.device) as c:
            for r in range(warmup + reps):
                c.render_depth(cams, 1, 0.02, want_idx=True)
                if r >= warmup:
                    pts.append(c.render_ms()[0])
        rate = counts["pairs"] / (ms["total"] * 1e-3) if ms["total"] > 0 else None
        out["meshes"][name] = {"vertices": len(m["xyz"]), "triangles": len(m["tri"]), "ms": ms, "wall_s": wall, "counts": counts,
                               "pairs_per_s": round(rate) if rate else None, "atomics_per_s": round(counts["atomics"] / (ms["total"] * 1e-3)) if ms["total"] > 0 else None,
                               "cloud_render_ms": round(med(pts), 4)}
        out["sweep"][name] = rows
        print(f"{name:>16} {len(m['tri']):>10} {ms['init']:8.3f} {ms['small']:8.3f} {ms['large']:8.3f} {ms['resolve']:8.3f} {ms['total']:8.3f} "
              f"{(rate or 0) / 1e6:9.1f} {counts['large_pairs']:>12} {counts['covered']:>10} {med(pts):10.3f} {counts['box_pixels'] / 1e6:9.1f} {counts['atomics'] / 1e6:9.2f}")
        for T, r in rows.items():
            print(f"{'T = ' + T:>16} {'':>10} {r['init']:8.3f} {r['small']:8.3f} {r['large']:8.3f} {r['resolve']:8.3f} {r['total']:8.3f} {'':>9} {r['large_pairs']:>12}")
    # one triangle that fills every image: in front of the first camera, far larger than its view
    R, t = np.array(cams[0].R[:], np.float64).reshape(3, 3), np.array(cams[0].t[:], np.float64)
    big = (np.linalg.inv(R) @ (np.array([[-400.0, -400.0, 5.0], [400.0, -400.0, 5.0], [0.0, 800.0, 5.0]]) - t).T).T
    with mesh.Mesh(big.astype(np.float32), [[0, 1, 2]], device=args.device) as hm:
        ms, wall, counts = timed(hm, cams, reps, warmup)
    out["one_triangle"] = {"ms": ms, "counts": counts}
    print(f"{'one triangle':>16} {1:>10} {ms['init']:8.3f} {ms['small']:8.3f} {ms['large']:8.3f} {ms['resolve']:8.3f} {ms['total']:8.3f} {'':>9} "
          f"{counts['large_pairs']:>12} {counts['covered']:>10}")
    if not args.trace and args.statement_triangles > 0:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import mesh_render_common as mr
        name = f"{min(sizes)} simplified"
        m = meshes[name]
        sub = {"xyz": m["xyz"], "tri": m["tri"][:args.statement_triangles]}
        cam = [depthmap.camera_at_size(cams[0], w, h, 160, 120)]
        with mesh.Mesh(sub["xyz"], sub["tri"], device=args.device) as hm:
            got_d, got_t = hm.render_depth(cam, want_tri=True)
            got_c = hm.last_render_counts
        t0 = time.perf_counter()
        want_d, want_t, want_c = mr.statement(sub["xyz"], sub["tri"], cam)
        t1 = time.perf_counter()
        equal = mr.same_bits(got_d[0], want_d[0]) and np.array_equal(got_t[0], want_t[0]) and [got_c["pairs"], got_c["covered"]] == want_c.tolist()
        out["statement"] = {"mesh": name, "triangles": len(sub["tri"]), "size": [160, 120], "numpy_s": round(t1 - t0, 3), "covered": int(want_c[1]), "equal": bool(equal)}
        print(f"statement: {len(sub['tri'])} triangles of {name} into 160 x 120: numpy {t1 - t0:.2f} s, {int(want_c[1])} pixels covered, device equal: {equal}")
    print(json.dumps(out))
    return 0 if out.get("statement", {}).get("equal", True) else 1


if __name__ == "__main__":
    sys.exit(main())
