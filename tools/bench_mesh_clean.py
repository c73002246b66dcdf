#!/usr/bin/env python3
"""Device and wall times of cleaning and shading a mesh on the GPU (mp-mvs_amd/mesh.py: Mesh; csrc/pm_mesh.hpp; DESIGN.md section
24), on the mesh of tools/bench_tsdf.py's synthetic height field.

    python tools/bench_mesh_clean.py [--sizes 256,512] [--views 8] [--size 1600x1200] [--shells 4000] [--reps 5] [--warmup 1] [--trace]

Per size n the views are integrated into an n^3 volume and meshed (about 0.5 M triangles at 256, 2.0 M at 512); --shells small closed
tetrahedra (4 triangles each) are planted beside the surface, so that there is something to remove, and the vertex numbers of the
whole mesh stay as the mesher and the planting left them.  Then, --reps times after --warmup (medians): a Mesh handle of it, its
components, its normals and the select that keeps the components of at least 5 triangles.  Reported per pass: device ms (HIP events),
the bytes the pass has to move at the least and their share of the HBM peak at that time; for the normals pass the 64-bit integer
atomics per second (nine per triangle, counted whether or not a term is 0 and skipped); the wall ms of the three calls (each
includes its download, the first one the upload of the mesh).  Beside them, on the host: scipy.sparse.csgraph.connected_components over the triangles' edges and the normals statement in
numpy with np.add.at (one run each; skipped where scipy is missing), and whether the device results equal them.
--trace: two repetitions and no host statement, for `rocprofv3 --kernel-trace --stats -- python tools/bench_mesh_clean.py --trace`
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

import mesh_clean_common as mc  # noqa: E402

mesh = importlib.import_module("mp-mvs_amd.mesh")
synth = importlib.import_module("mp-mvs_amd.synth")

HBM_PEAK = 8.0e12   # bytes / s
PASSES = ("cc_hook", "cc_flatten", "cc_sizes", "normals_accumulate", "normals_finish", "select_flag", "select_scan", "select_emit")


def med(xs):
    return float(np.median(np.asarray(xs, np.float64)))


def surface(n, cams, depths, device, side=5.6, centre=(0.0, 0.0, 5.0)):
    voxel = side / (n - 1)
    with mesh.Volume(tuple(c - 0.5 * side for c in centre), voxel, (n, n, n), 4 * voxel, device=device) as v:
        v.integrate(cams, depths)
        return v.mesh(1), voxel


def plant(m, shells, voxel, seed=1):
    """`shells` closed tetrahedra of about a voxel, each a few voxels off a random vertex of the surface"""
    rng = np.random.default_rng(seed)
    at = m["xyz"][rng.integers(0, len(m["xyz"]), shells)].astype(np.float64) + rng.uniform(3, 6, (shells, 1)) * voxel * np.array([0.0, 0.0, -1.0])
    pos = (at[:, None] + mc.TET_XYZ[None] * voxel).reshape(-1, 3)
    tri = (mc.TET[None] + 4 * np.arange(shells)[:, None, None]).reshape(-1, 3) + len(m["xyz"])
    return {"xyz": np.concatenate([m["xyz"], pos.astype(np.float32)]), "tri": np.concatenate([m["tri"], tri.astype(np.int32)]), "rgb": None}


def host_statement(m):
    """-> (labels or None, seconds, normals, seconds): scipy's connected components and the numpy normals statement"""
    n, tri = len(m["xyz"]), m["tri"].astype(np.int64)
    label, t_cc = None, None
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        t0 = time.perf_counter()
        a = np.concatenate([tri[:, 0], tri[:, 0]])
        b = np.concatenate([tri[:, 1], tri[:, 2]])
        _, comp = connected_components(coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(n, n)), directed=False)
        first = np.full(comp.max() + 1, n, np.int64)
        np.minimum.at(first, comp, np.arange(n))   # the smallest vertex index of each component
        label = first[comp].astype(np.int32)
        t_cc = time.perf_counter() - t0
    except ImportError:
        pass
    t0 = time.perf_counter()
    nrm, _ = mc.normals_statement(m["xyz"], m["tri"])
    return label, t_cc, nrm, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--size", default="1600x1200")
    ap.add_argument("--shells", type=int, default=4000)
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
    out = {"views": args.views, "size": [w, h], "shells": args.shells, "reps": reps, "warmup": warmup, "sizes": {}}
    print(f"{'n':>5} {'pass':>19} {'ms':>9} {'MB needed':>10} {'HBM share':>9}")
    for n in (int(s) for s in args.sizes.split(",") if s.strip()):
        base, voxel = surface(n, cams, depths, args.device)
        m = plant(base, args.shells, voxel)
        nv, nt = len(m["xyz"]), len(m["tri"])
        ms = {k: [] for k in PASSES}
        wall = {"create": [], "components": [], "normals": [], "select": []}
        for r in range(warmup + reps):
            t0 = time.perf_counter()
            with mesh.Mesh(m["xyz"], m["tri"], device=args.device) as hd:
                t1 = time.perf_counter()
                label, _, tris, counts = hd.components(want_verts=False)   # includes the upload of the mesh
                t2 = time.perf_counter()
                nrm, nd = hd.normals()
                t3 = time.perf_counter()
                keep = mesh.rank_components(label, tris, 5)
                t4 = time.perf_counter()
                sel = hd.select(keep)
                t5 = time.perf_counter()
                p = hd.pass_ms()
            if r >= warmup:
                for k in PASSES:
                    ms[k].append(p[k])
                for k, v in (("create", t1 - t0), ("components", t2 - t1), ("normals", t3 - t2), ("select", t5 - t4)):
                    wall[k].append(v)
        ms = {k: med(v) for k, v in ms.items()}
        wall = {k: med(v) for k, v in wall.items()}
        kv, kt = len(sel["xyz"]), len(sel["tri"])
        # the least each pass has to move: every array it must read or write once
        need = {"cc_hook": 12 * nt + 8 * nv, "cc_flatten": 8 * nv, "cc_sizes": 4 * nt + 28 * nv, "normals_accumulate": 12 * nt + 12 * nv + 48 * nv,
                "normals_finish": 24 * nv + 12 * nv, "select_flag": 12 * nt + nv + 4 * nt + 4 * nv, "select_scan": 8 * (nv + nt),
                "select_emit": 8 * nv + 12 * nv + 16 * kv + 8 * nt + 12 * nt + 12 * kt}
        share = {k: (round(need[k] / (ms[k] * 1e-3) / HBM_PEAK, 5) if ms[k] > 0 else None) for k in PASSES}
        atomics = 9 * nt / (ms["normals_accumulate"] * 1e-3) if ms["normals_accumulate"] > 0 else None
        res = {"vertices": nv, "triangles": nt, "components": counts["components"], "largest_component": counts["largest_triangles"], "kept_vertices": kv,
               "kept_triangles": kt, "normals_defined": nd, "ms": {k: round(v, 4) for k, v in ms.items()}, "bytes_needed": need, "hbm_share": share,
               "normals_atomics_per_s": round(atomics) if atomics else None, "wall_ms": {k: round(1e3 * v, 3) for k, v in wall.items()}}
        for k in PASSES:
            print(f"{n:>5} {k:>19} {ms[k]:9.4f} {need[k] / 1e6:10.1f} {100 * (share[k] or 0):8.2f}%")
        print(f"{n:>5} {nv} vertices, {nt} triangles, {counts['components']} components; kept {kv} / {kt}; {(atomics or 0) / 1e9:.2f} G atomics / s; wall ms: "
              + ", ".join(f"{k} {1e3 * v:.1f}" for k, v in wall.items()))
        if not args.trace:
            hl, t_cc, hn, t_n = host_statement(m)
            res["host"] = {"scipy_components_ms": None if t_cc is None else round(1e3 * t_cc, 1), "numpy_normals_ms": round(1e3 * t_n, 1),
                           "labels_equal": None if hl is None else bool(np.array_equal(hl, label)),
                           "normals_equal": bool(np.array_equal(hn.view(np.uint32), nrm.view(np.uint32)))}
            print(f"{n:>5} host: scipy components {res['host']['scipy_components_ms']} ms, numpy normals {res['host']['numpy_normals_ms']} ms; labels equal "
                  f"{res['host']['labels_equal']}, normals equal {res['host']['normals_equal']}")
        out["sizes"][str(n)] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
