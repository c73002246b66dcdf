#!/usr/bin/env python3
"""Thins a point cloud on a voxel grid on the GPU: one point per occupied voxel -- the mean position, the normalised sum of the
normals and the mean colour of its members (mp-mvs_amd/cloud.py: voxel_downsample).

    python tools/downsample_ply.py --input A.ply --output B.ply --voxel V [--device 0]

Reads positions, normals and colours of the `vertex` element (cloud.read_ply) and writes the reference's 27-byte records
(hostlib.write_ply: x y z nx ny nz red green blue); normals or colours the input lacks are written as zeros.  The output points
come in the order in which their voxels first appear in the input.
The last line printed is one JSON line: n, m, device ms of the kernels and wall seconds per stage."""
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
    ap.add_argument("--voxel", type=float, required=True, help="edge length of a voxel, in the cloud's units")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if not (np.isfinite(args.voxel) and args.voxel > 0):
        raise SystemExit("--voxel needs a finite positive edge length")
    t0 = time.perf_counter()
    src = cloud.read_ply(args.input)
    t1 = time.perf_counter()
    res = cloud.voxel_downsample(src["xyz"], args.voxel, normals=src.get("normals"), colors=src.get("colors"), device=args.device)
    t2 = time.perf_counter()
    m = len(res["xyz"])
    sys.stdout.flush()
    cloud.write_ply(args.output, res["xyz"], res.get("normals"), res.get("colors"))
    t3 = time.perf_counter()
    print(json.dumps({"n": int(len(src["xyz"])), "m": int(m), "voxel": args.voxel, "device_ms": round(cloud.last_voxel_ms(), 4),
                      "seconds": {"read": round(t1 - t0, 4), "downsample": round(t2 - t1, 4), "write": round(t3 - t2, 4), "total": round(t3 - t0, 4)}}),
          flush=True)


if __name__ == "__main__":
    main()
