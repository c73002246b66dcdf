#!/usr/bin/env python3
"""Estimates a surface normal per point of a PLY cloud on the GPU: the plane fitted to the k nearest neighbours within a radius
(mp-mvs_amd/cloud.py: Cloud.normals).

    python tools/normals_ply.py --input A.ply --output B.ply --radius R [--k 16] [--viewpoint X Y Z] [--drop_undefined] [--device 0]

The sign of a normal, which a plane fit cannot decide: with --viewpoint every normal looks at that point (a scanner position);
without it, a file that has normals of its own (the PatchMatch normals of a fused cloud) gives each estimated normal the side of its
stored one; otherwise the component of the largest magnitude is positive.  A point with fewer than two neighbours within the
radius, with all of them on one exact line, or with a non-finite coordinate has no normal: it is written with the normal 0 0 0, or
left out with --drop_undefined.  Writes the points in input order in the reference's 27-byte records (cloud.write_ply: x y z nx ny nz
red green blue), colours kept, zeros where the input has none.
The last line printed is one JSON line: n, defined, undefined, device ms, wall seconds per stage, and -- when the input had normals
-- the median and the 90th percentile of the angle in degrees between the stored and the estimated normals (sign ignored with
--viewpoint), over the points where both exist."""
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

cloud = importlib.import_module("mp-mvs_amd.cloud")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--input", required=True)
    ap.add_argument("--output", required=True)
    ap.add_argument("--radius", type=float, required=True, help="search radius of the neighbours, in the cloud's units")
    ap.add_argument("--k", type=int, default=16, help="neighbours per point (2 .. 32)")
    ap.add_argument("--viewpoint", type=float, nargs=3, metavar=("X", "Y", "Z"), help="every normal looks at this point")
    ap.add_argument("--drop_undefined", action="store_true", help="leave out the points without a normal")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if not (np.isfinite(args.radius) and args.radius > 0):
        raise SystemExit("--radius needs a finite positive length")
    t0 = time.perf_counter()
    src = cloud.read_ply(args.input)
    t1 = time.perf_counter()
    stored = src.get("normals")
    orientation = "viewpoint" if args.viewpoint is not None else ("stored" if stored is not None else "canonical")
    with cloud.Cloud(src["xyz"], args.device) as c:
        nrm, curv = c.normals(args.radius, args.k, viewpoint=args.viewpoint, reference=stored if orientation == "stored" else None)
        ms, build_ms = c.normals_ms()
    t2 = time.perf_counter()
    defined = np.isfinite(curv)
    keep = defined if args.drop_undefined else np.ones(len(defined), bool)
    sys.stdout.flush()
    cloud.write_ply(args.output, src["xyz"][keep], nrm[keep], src["colors"][keep] if "colors" in src else None)
    t3 = time.perf_counter()
    line = {"n": int(len(defined)), "defined": int(defined.sum()), "undefined": int((~defined).sum()), "written": int(keep.sum()), "radius": args.radius,
            "k": args.k, "orientation": orientation, "device_ms": round(ms, 4), "build_ms": round(build_ms, 4),
            "seconds": {"read": round(t1 - t0, 4), "normals": round(t2 - t1, 4), "write": round(t3 - t2, 4), "total": round(t3 - t0, 4)}}
    if stored is not None:
        s = stored.astype(np.float64)
        length = np.linalg.norm(s, axis=1)
        both = defined & np.isfinite(length) & (length > 0)
        med = p90 = None
        if both.any():
            a, b = nrm[both].astype(np.float64), s[both] / length[both, None]
            dot = (a * b).sum(1)
            ang = np.degrees(np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), np.abs(dot) if orientation == "viewpoint" else dot))
            med, p90 = float(np.median(ang)), float(np.percentile(ang, 90))
        line["stored_normals"] = {"compared": int(both.sum()), "angle_median_deg": med, "angle_p90_deg": p90}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
