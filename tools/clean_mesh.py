#!/usr/bin/env python3
"""Clean and shade any triangle mesh PLY on the GPU: drop the small detached pieces, add vertex normals (mp-mvs_amd/mesh.py: Mesh,
remove_small_components; csrc/pm_mesh.hpp).

    python tools/clean_mesh.py --input A.ply --output B.ply [--min_component N] [--largest K] [--normals]

Reads what mesh.write_ply_mesh writes (binary little-endian, float x y z, optional float nx ny nz and uchar red green blue, triangles
only).  --min_component N drops the connected components with fewer than N triangles (0 = off, the default), --largest K all but the K
largest by triangle count (ties to the component with the smaller first vertex); vertices that no triangle names go with them.
Connectivity is by index: coincident vertices are not welded.  --normals writes area-weighted vertex normals; normals of the input
are not carried over.  The mesh is cleaned first, then shaded.  N has not been tuned on any real scene.
Prints one JSON line: vertices and triangles in and out, components, largest_component, removed_triangles, normals_defined, device ms
per pass, wall seconds."""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--input", required=True)
    ap.add_argument("--output", required=True)
    ap.add_argument("--min_component", type=int, default=0, help="drop connected components with fewer triangles; 0 = off; untuned on real scenes")
    ap.add_argument("--largest", type=int, help="keep only the K largest components by triangle count")
    ap.add_argument("--normals", action="store_true", help="write area-weighted vertex normals")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    if args.min_component < 0 or (args.largest is not None and args.largest < 1):
        raise SystemExit("--min_component must not be negative and --largest must be at least 1")

    import torch  # noqa: F401  (the HIP runtime torch bundles, before our library: engine.load)
    mesh = importlib.import_module("mp-mvs_amd.mesh")
    t0 = time.perf_counter()
    try:
        m = mesh.read_ply_mesh(args.input)
        res = {"input": args.input, "vertices_in": int(len(m["xyz"])), "triangles_in": int(len(m["tri"]))}
        t1 = time.perf_counter()
        info, normals = mesh.clean_and_shade(m, args.min_component, args.largest, args.normals, device=args.device)
        m = info.pop("mesh")
        t2 = time.perf_counter()
        mesh.write_ply_mesh(args.output, m["xyz"], m["tri"], m["rgb"], normals=normals)
    except (ValueError, OSError, RuntimeError) as e:
        raise SystemExit(str(e)) from None
    t3 = time.perf_counter()
    res.update({"vertices": int(len(m["xyz"])), "triangles": int(len(m["tri"])), "device_ms": {k: round(v, 4) for k, v in info.pop("device_ms").items()}})
    res.update(info)
    res.update({"seconds": {"read": round(t1 - t0, 4), "clean": round(t2 - t1, 4), "write": round(t3 - t2, 4), "wall": round(t3 - t0, 4)}, "output": args.output})
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
