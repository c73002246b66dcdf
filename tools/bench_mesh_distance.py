#!/usr/bin/env python3
"""Device and wall times of measuring a mesh as a surface on the GPU (mp-mvs_amd/mesh.py: Mesh.distance, Mesh.sample;
csrc/pm_surface.hpp), on the mesh of tools/bench_tsdf.py's synthetic height field and its simplification.

    python tools/bench_mesh_distance.py [--sizes 256,512] [--radii 0.5,1,2] [--points 2000000] [--larges 64,512,4096] [--views 8]
                                        [--size 1600x1200] [--reps 5] [--warmup 1] [--statement-points 500] [--trace]

Per size n the views are integrated into an n^3 volume and meshed (about 0.5 M triangles at 256, 2.0 M at 512), and the mesh is
simplified with a cell of 4 voxels.  Then, per radius of --radii voxels, --reps times after --warmup (medians):
  1. a scan -- up to --points of the mesh's own vertices, jittered by up to half a voxel -- against the full mesh and against the
     simplified one (large triangles against a dense scan: the large-triangle path);
  2. the samples of the simplified mesh (Mesh.sample at a spacing of one voxel) against the full mesh.
Reported: device ms per pass (HIP events), the cloud's grid build, points per second, the share of points with a candidate, samples per
second of Mesh.sample, the wall ms of a call.  Beside them Cloud.nearest of the same points against the mesh's VERTICES, the nearest
thing the project could do before, with the mean of distance-to-surface / distance-to-vertex where both exist.
--larges: the scan against the simplified mesh at the smallest radius (where its triangles span the most cells) again with the large-triangle threshold (MPMVS_SURFACE_LARGE, in
cells) at each of these values: the measurement the default is chosen from.  Also there: surface_distances as a cascade over the radii
against one call at the largest.  --statement-points: the numpy statement of tests/mesh_distance_common.py on that many points of
direction 1 against the simplified mesh, its seconds, and whether the device result equals it bit for bit (0: skip).
--trace: two repetitions, no host statement and no sweeps, for `rocprofv3 --kernel-trace --stats -- python tools/bench_mesh_distance.py
--trace` (never together with counters).  Prints the table and one JSON line.  There is no target figure."""
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

mesh = importlib.import_module("mp-mvs_amd.mesh")
cloud = importlib.import_module("mp-mvs_amd.cloud")
synth = importlib.import_module("mp-mvs_amd.synth")


def med(xs):
    return float(np.median(np.asarray(xs, np.float64)))


def surface(n, cams, depths, device, side=5.6, centre=(0.0, 0.0, 5.0)):
    voxel = side / (n - 1)
    with mesh.Volume(tuple(c - 0.5 * side for c in centre), voxel, (n, n, n), 4 * voxel, device=device) as v:
        v.integrate(cams, depths)
        return v.mesh(1), voxel


def timed_distance(h, c, radius, reps, warmup):
    """medians over reps of one resident pair: passes, wall, the grid build of the first call, the counts"""
    ms, wall, build = {k: [] for k in ("init", "scatter", "finish", "total")}, [], None
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        d2 = h.distance(c, radius, want_tri=False)
        t1 = time.perf_counter()
        if build is None:
            build = c.kernel_ms()[1]
        if r >= warmup:
            wall.append(t1 - t0)
            for k, v in h.distance_ms().items():
                ms[k].append(v)
    return {k: med(v) for k, v in ms.items()}, 1e3 * med(wall), build, d2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--radii", default="0.5,1,2", help="in voxels")
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--larges", default="64,512,4096")
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--size", default="1600x1200")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--statement-points", type=int, default=500)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    w, hgt = (int(v) for v in args.size.lower().split("x"))
    reps, warmup = (2, 0) if args.trace else (args.reps, args.warmup)
    if not 1 <= args.views <= 9:
        raise SystemExit("--views must lie in 1..9")
    scene = synth.make_problem_scene(w, hgt, n_src=max(args.views - 1, 1), quantize=True)
    views = scene.views[:args.views]
    cams, depths = [v.cam for v in views], [v.gt_depth for v in views]
    radii = [float(s) for s in args.radii.split(",") if s.strip()]
    out = {"views": args.views, "size": [w, hgt], "reps": reps, "warmup": warmup, "sizes": {}}
    head = f"{'n':>5} {'pair':>22} {'radius':>6} {'init':>8} {'scatter':>9} {'finish':>8} {'sum ms':>8} {'build':>7} {'wall ms':>8} {'Mpts/s':>8} {'found':>6}"
    print(head)
    for n in (int(s) for s in args.sizes.split(",") if s.strip()):
        full, voxel = surface(n, cams, depths, args.device)
        simp = mesh.simplify(full, float(np.float32(4 * voxel)), device=args.device)
        rng = np.random.default_rng(n)
        pick = rng.permutation(len(full["xyz"]))[:args.points]
        scan = (full["xyz"][pick] + rng.uniform(-0.5, 0.5, (len(pick), 3)) * voxel).astype(np.float32)
        res = {"vertices": len(full["xyz"]), "triangles": len(full["tri"]), "simplified_vertices": len(simp["xyz"]), "simplified_triangles": len(simp["tri"]),
               "scan_points": len(scan), "rows": []}
        with mesh.Mesh(full["xyz"], full["tri"], device=args.device) as h_full, mesh.Mesh(simp["xyz"], simp["tri"], device=args.device) as h_simp:
            t0 = time.perf_counter()
            smp = h_simp.sample(float(np.float32(voxel)))["xyz"]
            t_sample = time.perf_counter() - t0
            for _ in range(reps):
                h_simp.sample(float(np.float32(voxel)))
            sms = h_simp.sample_ms()
            res["sample"] = {"samples": len(smp), "device_ms": {k: round(v, 4) for k, v in sms.items()}, "first_wall_ms": round(1e3 * t_sample, 2),
                             "samples_per_s": round(len(smp) / (sms["total"] * 1e-3)) if sms["total"] > 0 else None}
            print(f"{n:>5} sample of the simplified mesh at one voxel: {len(smp)} samples, count {sms['count']:.4f} scan {sms['scan']:.4f} emit {sms['emit']:.4f} ms, "
                  f"{len(smp) / max(sms['total'], 1e-9) / 1e6:.1f} G samples / s")
            pairs = (("scan -> full mesh", scan, h_full, full), ("scan -> simplified", scan, h_simp, simp), ("samples -> full mesh", smp, h_full, full))
            for name, pts, h, m in pairs:
                with cloud.Cloud(pts, args.device) as c, cloud.Cloud(m["xyz"], args.device) as verts:
                    for rv in radii:
                        radius = float(np.float32(rv * voxel))
                        ms, wall, build, d2 = timed_distance(h, c, radius, reps, warmup)
                        found = float(np.isfinite(d2).mean())
                        t0 = time.perf_counter()
                        dv, _ = verts.nearest(pts, radius, want_idx=False)
                        t_near = time.perf_counter() - t0
                        near_ms = verts.kernel_ms()
                        both = np.isfinite(d2) & np.isfinite(dv) & (dv > 0)
                        row = {"pair": name, "radius_voxels": rv, "ms": {k: round(v, 4) for k, v in ms.items()}, "grid_build_ms": round(build, 4), "wall_ms": round(wall, 3),
                               "points_per_s": round(len(pts) / (ms["total"] * 1e-3)) if ms["total"] > 0 else None, "with_candidate": round(found, 4),
                               "vertex_nearest": {"query_ms": round(near_ms[0], 4), "build_ms": round(near_ms[1], 4), "wall_ms": round(1e3 * t_near, 3),
                                                  "found": round(float(np.isfinite(dv).mean()), 4),
                                                  "surface_over_vertex": round(float(np.sqrt(d2[both] / dv[both]).mean()), 4) if both.any() else None}}
                        res["rows"].append(row)
                        print(f"{n:>5} {name:>22} {rv:>6g} {ms['init']:8.4f} {ms['scatter']:9.4f} {ms['finish']:8.4f} {ms['total']:8.3f} {build:7.3f} {wall:8.2f} "
                              f"{len(pts) / max(ms['total'], 1e-9) / 1e3:8.1f} {found:6.3f}   vertices: {near_ms[0]:.3f} ms, found {row['vertex_nearest']['found']:.3f}, "
                              f"surface / vertex {row['vertex_nearest']['surface_over_vertex']}")
            if not args.trace:
                mid, low = float(np.float32(radii[len(radii) // 2] * voxel)), float(np.float32(min(radii) * voxel))
                with cloud.Cloud(scan, args.device) as c:
                    sweep, before = {}, os.environ.get("MPMVS_SURFACE_LARGE")
                    for large in [s.strip() for s in args.larges.split(",") if s.strip()]:
                        os.environ["MPMVS_SURFACE_LARGE"] = large
                        ms, wall, _, _ = timed_distance(h_simp, c, low, reps, warmup)
                        sweep[large] = round(ms["scatter"], 4)
                    os.environ.pop("MPMVS_SURFACE_LARGE", None)
                    if before is not None:
                        os.environ["MPMVS_SURFACE_LARGE"] = before
                    res["large_threshold_scatter_ms"] = sweep
                    print(f"{n:>5} scan -> simplified at {min(radii):g} voxels, scatter ms by large-triangle threshold (cells): {sweep}")
                    tol = [float(np.float32(rv * voxel)) for rv in radii]
                    t0 = time.perf_counter()
                    d_cascade = mesh.surface_distances(scan, h_simp, tol, device=args.device)
                    t1 = time.perf_counter()
                    with cloud.Cloud(scan, args.device) as c_one:   # a cloud of its own, as the cascade has to make one
                        d_single = np.sqrt(h_simp.distance(c_one, max(tol), want_tri=False))
                    t2 = time.perf_counter()
                    res["cascade"] = {"cascade_wall_ms": round(1e3 * (t1 - t0), 2), "single_call_wall_ms": round(1e3 * (t2 - t1), 2),
                                      "single_call_device_ms": round(h_simp.distance_ms()["total"], 4), "equal": bool(np.array_equal(d_cascade, d_single))}
                    print(f"{n:>5} surface_distances over {args.radii} voxels: cascade {1e3 * (t1 - t0):.1f} ms wall, a cloud and one call at the largest "
                          f"{1e3 * (t2 - t1):.1f} ms wall; equal: {res['cascade']['equal']}")
                if args.statement_points > 0:
                    import mesh_distance_common as md
                    sub = scan[:args.statement_points]
                    t0 = time.perf_counter()
                    want = md.distance_statement(simp["xyz"], simp["tri"], sub, mid, chunk=256)
                    t_host = time.perf_counter() - t0
                    with cloud.Cloud(sub, args.device) as c:
                        d2, tri = h_simp.distance(c, mid)
                    equal = bool(md.same_bits(d2, want[0]) and np.array_equal(tri, want[1]))
                    res["host"] = {"points": len(sub), "numpy_statement_s": round(t_host, 2), "equal": equal}
                    print(f"{n:>5} host: the numpy statement on {len(sub)} points x {len(simp['tri'])} triangles takes {t_host:.2f} s; the device result equals it: {equal}")
        out["sizes"][str(n)] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
