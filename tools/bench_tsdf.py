#!/usr/bin/env python3
"""The TSDF integration and the marching-tetrahedra mesh (mesh.Volume; csrc/pm_tsdf.hpp) on the synthetic
height field of mp-mvs_amd/synth.py.

Workload: --views cameras (default 8: the reference view and its neighbours of the 3 x 3 grid of synth.make_problem_scene) of --size
(default 1600x1200) with their analytic depth maps (the ray / height-field intersection synth renders its images with), integrated
into cubes of --sizes lattice points per axis (default 256,512) centred on the surface, truncation 4 voxels, then meshed at
min_weight 1.  --color: with the images as colours (24 instead of 8 bytes per voxel).

Reports per size the device ms per pass (integrate; mark + count, scan, vertices, triangles; HIP events), voxel-view pairs per second
through the integration, the bytes each pass must at least move and their share of the 8 TB/s HBM peak --
    integrate  the volume read and written once per launch of 8 views (8 + 8 bytes per voxel, 32 + 32 with colour) and the images once
    mark       sum and weight read (8), the mask cleared (4), the triangle count written (4) per voxel
    scan       mask and count read (8), both scans written (8) per voxel
    vertices   the mask read (4 per voxel), 12 (15 with colour) bytes written per vertex
    triangles  sum and weight read (8 per voxel), 12 bytes written per triangle
-- the wall time of both calls, and the numpy statement (tests/tsdf_common.py) beside it at --statement-size (default 64) lattice
points per axis, once, with a check that both agree bit for bit.  Medians of --reps repetitions after --warmup; every repetition
integrates into a fresh volume.  --trace: two repetitions and no statement, for
`rocprofv3 --kernel-trace --stats -- python tools/bench_tsdf.py --trace` (never together with counters).

--sparse: the brick-sparse volume (mesh.SparseVolume; csrc/pm_tsdf_sparse.hpp) beside the dense one on the same
workload: per size of --sizes a dense and a sparse volume alternate, repetition by repetition, in this process, and the sizes of
--sparse-sizes (default 1024) run sparse alone.  Per size: the device ms of allocate (marking; scan + commit), integrate and the four
mesh passes, the bricks and their share of the brick grid, the device bytes both volumes hold between calls and the mesh scratch
(12 bytes per dense voxel, per existing voxel), vertices and triangles beside the dense counts (the sparse mesh is a sub-mesh: the
share of dense triangles it misses is 1 - sparse / dense), and the ratios dense / sparse.  --coverage-size N (default 256, 0: skip):
once, the share of band voxels (a contribution with |s| <= trunc: exactly the voxels whose colour count a dense volume with colour
raises) that lie outside the allocated bricks at --pad.  --pad (default 1.0) is an untuned starting value.
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

import tsdf_common as tc  # noqa: E402

mesh = importlib.import_module("mp-mvs_amd.mesh")
synth = importlib.import_module("mp-mvs_amd.synth")

HBM_PEAK = 8.0e12   # bytes / s
PASSES = ("integrate", "mark", "scan", "vertices", "triangles")


def med(xs):
    return float(np.median(np.asarray(xs, np.float64)))


def box(n, side=5.6, centre=(0.0, 0.0, 5.0)):
    """(origin, voxel) of a cube of n lattice points per axis around the height field under the cameras"""
    voxel = side / (n - 1)
    return tuple(c - 0.5 * side for c in centre), voxel


def run(n, cams, depths, colors, reps, warmup, device):
    origin, voxel = box(n)
    ms = {k: [] for k in PASSES}
    wall = {"integrate": [], "mesh": []}
    for r in range(warmup + reps):
        with mesh.Volume(origin, voxel, (n, n, n), 4 * voxel, color=colors is not None, device=device) as v:
            t0 = time.perf_counter()   # the wall time of integrate() includes opening the device and clearing the volume
            v.integrate(cams, depths, colors)
            t1 = time.perf_counter()
            m = v.mesh(1)
            t2 = time.perf_counter()
            p = v.pass_ms()
        if r >= warmup:
            for k in PASSES:
                ms[k].append(p[k])
            wall["integrate"].append(t1 - t0)
            wall["mesh"].append(t2 - t1)
    return m, {k: med(v) for k, v in ms.items()}, {k: med(v) for k, v in wall.items()}


SPARSE_PASSES = ("allocate_mark", "allocate_commit") + PASSES


def run_pair(n, cams, depths, reps, warmup, device, pad, with_dense):
    """a dense and a sparse volume of n^3 alternating -> (dense mesh, dense ms, sparse mesh, sparse ms, sparse stats, wall seconds)"""
    origin, voxel = box(n)
    dms, sms = {k: [] for k in PASSES}, {k: [] for k in SPARSE_PASSES}
    wall = {"dense": [], "sparse": []}
    dm = sm = st = None
    for r in range(warmup + reps):
        if with_dense:
            t0 = time.perf_counter()
            with mesh.Volume(origin, voxel, (n, n, n), 4 * voxel, device=device) as v:
                v.integrate(cams, depths)
                dm = v.mesh(1)
                p = v.pass_ms()
            t1 = time.perf_counter()
            if r >= warmup:
                wall["dense"].append(t1 - t0)
                for k in PASSES:
                    dms[k].append(p[k])
        t0 = time.perf_counter()
        with mesh.SparseVolume(origin, voxel, (n, n, n), 4 * voxel, pad=pad, device=device) as v:
            v.allocate(cams, depths)
            v.integrate(cams, depths)
            sm = v.mesh(1)
            p = dict(v.pass_ms())
            st = v.stats()
        t1 = time.perf_counter()
        p.update({"allocate_mark": st["allocate_mark"], "allocate_commit": st["allocate_commit"]})
        if r >= warmup:
            wall["sparse"].append(t1 - t0)
            for k in SPARSE_PASSES:
                sms[k].append(p[k])
    return (dm, {k: med(v) for k, v in dms.items()} if with_dense else None, sm, {k: med(v) for k, v in sms.items()}, st,
            {k: med(v) for k, v in wall.items() if v})


def coverage(n, cams, depths, device, pad):
    """the share of band voxels outside the allocated bricks: the band from a dense volume with (grey, all-zero) colour, whose colour
    count rises exactly where a contribution has |s| <= trunc"""
    origin, voxel = box(n)
    grey = [np.zeros(d.shape, np.uint8) for d in depths]
    with mesh.Volume(origin, voxel, (n, n, n), 4 * voxel, color=True, device=device) as v:
        v.integrate(cams, depths, grey)
        band = v.get()["color"][..., 3] > 0
    with mesh.SparseVolume(origin, voxel, (n, n, n), 4 * voxel, pad=pad, device=device) as v:
        v.allocate(cams, depths)
        coords = v.bricks()
    b = (n + 7) // 8
    bricks = np.zeros((b, b, b), bool)
    bricks[coords[:, 2], coords[:, 1], coords[:, 0]] = True
    exists = np.repeat(np.repeat(np.repeat(bricks, 8, 0), 8, 1), 8, 2)[:n, :n, :n]
    return int(band.sum()), int((band & ~exists).sum())


def main_sparse(args, cams, depths, w, h, reps, warmup):
    sizes = [(int(s), True) for s in args.sizes.split(",") if s.strip()] + [(int(s), False) for s in args.sparse_sizes.split(",") if s.strip()]
    out = {"views": args.views, "size": [w, h], "sparse": True, "pad": args.pad, "reps": reps, "warmup": warmup, "sizes": {}}
    print(f"{args.views} views of {w} x {h}, no colour, truncation 4 voxels, min_weight 1, pad {args.pad} (untuned); dense and sparse alternating")
    print(f"{'n':>5} {'pass':>16} {'dense ms':>9} {'sparse ms':>9} {'ratio':>7}")
    for n, with_dense in sizes:
        dm, dms, sm, sms, st, wall = run_pair(n, cams, depths, reps, warmup, args.device, args.pad, with_dense)
        rec = {"bricks": st["bricks"], "grid_cells": st["grid_cells"], "brick_share": round(st["brick_share"], 5),
               "sparse_bytes_held": st["device_bytes"], "sparse_mesh_scratch": 12 * 512 * st["bricks"],
               "sparse_ms": {k: round(v, 4) for k, v in sms.items()}, "sparse_vertices": len(sm["xyz"]), "sparse_triangles": len(sm["tri"]),
               "wall_s": {k: round(v, 4) for k, v in wall.items()}}
        s_int = sms["allocate_mark"] + sms["allocate_commit"] + sms["integrate"]
        s_mesh = sum(sms[k] for k in PASSES[1:])
        rec["sparse_sum_ms"] = {"allocate+integrate": round(s_int, 4), "mesh": round(s_mesh, 4)}
        for k in SPARSE_PASSES:
            d = dms[k] if with_dense and k in PASSES else None
            ratio = f"{d / sms[k]:7.2f}" if d and sms[k] > 0 else f"{'':>7}"
            print(f"{n:>5} {k:>16} {d if d is not None else float('nan'):9.3f} {sms[k]:9.3f} {ratio}")
        if with_dense:
            d_mesh = sum(dms[k] for k in PASSES[1:])
            rec.update({"dense_ms": {k: round(v, 4) for k, v in dms.items()}, "dense_vertices": len(dm["xyz"]), "dense_triangles": len(dm["tri"]),
                        "dense_bytes_held": 8 * n ** 3, "dense_mesh_scratch": 12 * n ** 3,
                        "dense_sum_ms": {"integrate": round(dms["integrate"], 4), "mesh": round(d_mesh, 4)},
                        "ratio_dense_over_sparse": {"integrate_vs_allocate+integrate": round(dms["integrate"] / s_int, 3), "mesh": round(d_mesh / s_mesh, 3),
                                                    "bytes_held": round(8 * n ** 3 / st["device_bytes"], 3)},
                        "dense_triangles_missing_share": round(1.0 - len(sm["tri"]) / max(len(dm["tri"]), 1), 6)})
            print(f"{n:>5} sums: dense integrate {dms['integrate']:.3f} + mesh {d_mesh:.3f} ms; sparse allocate + integrate {s_int:.3f} + mesh {s_mesh:.3f} ms")
            print(f"{n:>5} triangles dense {len(dm['tri'])}, sparse {len(sm['tri'])}; vertices dense {len(dm['xyz'])}, sparse {len(sm['xyz'])}")
        else:
            print(f"{n:>5} sums: sparse allocate + integrate {s_int:.3f} + mesh {s_mesh:.3f} ms; {len(sm['xyz'])} vertices, {len(sm['tri'])} triangles")
        print(f"{n:>5} bricks {st['bricks']} of {st['grid_cells']} ({100 * st['brick_share']:.2f} %); held: sparse {st['device_bytes'] / 1e6:.1f} MB"
              + (f", dense {8 * n ** 3 / 1e6:.1f} MB" if with_dense else "") + f"; mesh scratch: sparse {12 * 512 * st['bricks'] / 1e6:.1f} MB"
              + (f", dense {12 * n ** 3 / 1e6:.1f} MB" if with_dense else ""))
        out["sizes"][str(n)] = rec
    if args.coverage_size > 0:
        band, outside = coverage(args.coverage_size, cams, depths, args.device, args.pad)
        out["coverage"] = {"n": args.coverage_size, "band_voxels": band, "outside_bricks": outside, "share_outside": round(outside / max(band, 1), 6)}
        print(f"coverage at {args.coverage_size}^3, pad {args.pad}: {outside} of {band} band voxels lie outside the allocated bricks")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--size", default="1600x1200")
    ap.add_argument("--color", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--statement-size", type=int, default=64)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--no-statement", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--sparse", action="store_true", help="the brick-sparse volume beside the dense one")
    ap.add_argument("--sparse-sizes", default="1024", help="--sparse: sizes that run sparse alone")
    ap.add_argument("--pad", type=float, default=1.0, help="--sparse: voxels around a ray sample whose bricks are allocated; 1.0 is an untuned starting value")
    ap.add_argument("--coverage-size", type=int, default=256, help="--sparse: the size at which the band voxels outside the bricks are counted (0: skip)")
    args = ap.parse_args()
    w, h = (int(v) for v in args.size.lower().split("x"))
    sizes = [int(s) for s in args.sizes.split(",") if s.strip()]
    reps, warmup = (2, 0) if args.trace else (args.reps, args.warmup)
    if not 1 <= args.views <= 9:
        raise SystemExit("--views must lie in 1..9")
    sc = synth.make_problem_scene(w, h, n_src=max(args.views - 1, 1), quantize=True)
    views = sc.views[:args.views]
    cams, depths = [v.cam for v in views], [v.gt_depth for v in views]
    colors = [v.image.astype(np.uint8) for v in views] if args.color else None
    if args.sparse:
        if args.color:
            raise SystemExit("--sparse measures without colour")
        return main_sparse(args, cams, depths, w, h, reps, warmup)
    pixels = args.views * w * h
    out = {"views": args.views, "size": [w, h], "color": bool(args.color), "reps": reps, "warmup": warmup, "sizes": {}}
    per_vox = 48 if args.color else 16
    print(f"{args.views} views of {w} x {h}, colour {bool(args.color)}, truncation 4 voxels, min_weight 1")
    print(f"{'n':>5} {'pass':>10} {'ms':>9} {'MB needed':>10} {'HBM share':>9}")
    for n in sizes:
        m, ms, wall = run(n, cams, depths, colors, reps, warmup, args.device)
        n_vox, nv, nt = n ** 3, len(m["xyz"]), len(m["tri"])
        launches = -(-args.views // 8)
        need = {"integrate": launches * per_vox * n_vox + pixels * (4 + (1 if args.color else 0)), "mark": 16 * n_vox, "scan": 16 * n_vox,
                "vertices": 4 * n_vox + (15 if args.color else 12) * nv, "triangles": 8 * n_vox + 12 * nt}
        share = {k: (round(need[k] / (ms[k] * 1e-3) / HBM_PEAK, 5) if ms[k] > 0 else None) for k in PASSES}
        pairs = n_vox * args.views / (ms["integrate"] * 1e-3) if ms["integrate"] > 0 else None
        out["sizes"][str(n)] = {"n_vox": n_vox, "vertices": nv, "triangles": nt, "ms": {k: round(v, 4) for k, v in ms.items()}, "bytes_needed": need,
                                "hbm_share": share, "voxel_view_pairs_per_s": round(pairs) if pairs else None,
                                "wall_s": {k: round(v, 4) for k, v in wall.items()}}
        for k in PASSES:
            print(f"{n:>5} {k:>10} {ms[k]:9.3f} {need[k] / 1e6:10.1f} {100 * (share[k] or 0):8.2f}%")
        print(f"{n:>5} {nv} vertices, {nt} triangles; {(pairs or 0) / 1e9:.2f} G voxel-view pairs / s; integrate() {wall['integrate'] * 1e3:.1f} ms wall, "
              f"mesh() {wall['mesh'] * 1e3:.1f} ms wall")

    if not args.trace and not args.no_statement:
        n = args.statement_size
        origin, voxel = box(n)
        with mesh.Volume(origin, voxel, (n, n, n), 4 * voxel, color=args.color, device=args.device) as v:
            t0 = time.perf_counter()
            v.integrate(cams, depths, colors)
            got_vol = v.get()
            got = v.mesh(1)
            t_gpu = time.perf_counter() - t0
        t0 = time.perf_counter()
        want_vol = tc.integrate_statement(origin, voxel, (n, n, n), 4 * voxel, cams, depths, colors)
        t1 = time.perf_counter()
        want = tc.mesh_statement(want_vol[0], want_vol[1], want_vol[2], (n, n, n), origin, voxel, 1)
        t2 = time.perf_counter()
        same = (np.array_equal(got_vol["sum"].view(np.uint32), want_vol[0].view(np.uint32)) and np.array_equal(got_vol["weight"], want_vol[1])
                and (not args.color or np.array_equal(got_vol["color"], want_vol[2]))
                and np.array_equal(got["xyz"].view(np.uint32), want["xyz"].view(np.uint32)) and np.array_equal(got["tri"], want["tri"])
                and (not args.color or np.array_equal(got["rgb"], want["rgb"])))
        out["statement"] = {"n": n, "integrate_wall_s": round(t1 - t0, 4), "mesh_wall_s": round(t2 - t1, 4), "gpu_wall_s": round(t_gpu, 4),
                            "triangles": int(len(want["tri"])), "equals_statement": bool(same)}
        print(f"numpy statement at {n}^3, one thread: integrate {(t1 - t0) * 1e3:.1f} ms, mesh {(t2 - t1) * 1e3:.1f} ms wall "
              f"(the device calls with their copies: {t_gpu * 1e3:.1f} ms); bit for bit equal: {same}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
