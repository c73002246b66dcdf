#!/usr/bin/env python3
"""Simplify any triangle mesh PLY on the GPU by vertex clustering with quadrics (mp-mvs_amd/mesh.py: Mesh.simplify, simplify;
csrc/pm_simplify.hpp).

    python tools/simplify_mesh.py --input A.ply --output B.ply --cell C [--placement mean|quadric] [--keep_unreferenced] [--normals]

Reads what mesh.write_ply_mesh writes (binary little-endian, float x y z, optional float nx ny nz and uchar red green blue, triangles
only).  Every occupied cell of a uniform grid of edge C (scene units) becomes one vertex: the mean of its members (mean) or the point
of the cell where the planes of the triangles around it meet best (quadric, the default; where that point leaves the cell, the mean).
Triangles that collapse and duplicates of a triangle already kept go; a cell far below the sampling distance only welds coincident
vertices.  Vertices that no kept triangle names are dropped unless --keep_unreferenced.  --normals writes area-weighted vertex
normals of the new mesh; normals of the input are not carried over.
Prints one JSON line: n, m (in), n_out, m_out, the counts non_finite / collapsed / duplicates, the clusters by placed (0 none, 1
quadric, 2 fell back), device ms per pass, wall seconds."""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--input", required=True)
    ap.add_argument("--output", required=True)
    ap.add_argument("--cell", type=float, required=True, help="edge of the clustering grid in scene units")
    ap.add_argument("--placement", choices=("mean", "quadric"), default="quadric")
    ap.add_argument("--keep_unreferenced", action="store_true", help="keep the clusters that no kept triangle names")
    ap.add_argument("--normals", action="store_true", help="write area-weighted vertex normals")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    if not (args.cell > 0.0 and args.cell < float("inf")):
        raise SystemExit("--cell must be finite and positive")
    return args


def load(args):
    """the input mesh and the head of the result line; no device is touched"""
    mesh = importlib.import_module("mp-mvs_amd.mesh")
    try:
        m = mesh.read_ply_mesh(args.input)
    except (ValueError, OSError) as e:
        raise SystemExit(str(e)) from None
    return m, {"input": args.input, "n": int(len(m["xyz"])), "m": int(len(m["tri"])), "cell": args.cell, "placement": args.placement}


def main(argv=None):
    args = parse_args(argv)
    import torch  # noqa: F401  (the HIP runtime torch bundles, before our library: engine.load)
    mesh = importlib.import_module("mp-mvs_amd.mesh")
    t0 = time.perf_counter()
    m, res = load(args)
    t1 = time.perf_counter()
    try:
        out = mesh.simplify(m, args.cell, args.placement, drop_unreferenced=not args.keep_unreferenced, normals=args.normals, device=args.device)
        t2 = time.perf_counter()
        mesh.write_ply_mesh(args.output, out["xyz"], out["tri"], out["rgb"], normals=out["normals"])
    except (ValueError, OSError, RuntimeError) as e:
        raise SystemExit(str(e)) from None
    t3 = time.perf_counter()
    res.update({"clusters": int(len(out["count"])), "n_out": int(len(out["xyz"])), "m_out": int(len(out["tri"]))})
    res.update(out["counts"])
    res.update({"placed": [int((out["placed"] == p).sum()) for p in range(3)]})
    if args.normals:
        res["normals_defined"] = out["normals_defined"]
    res.update({"device_ms": {k: round(v, 4) for k, v in out["device_ms"].items()},
                "seconds": {"read": round(t1 - t0, 4), "simplify": round(t2 - t1, 4), "write": round(t3 - t2, 4), "wall": round(t3 - t0, 4)}, "output": args.output})
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
