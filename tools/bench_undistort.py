#!/usr/bin/env python3
"""The undistortion warp (mpmvs_undistort_u8, csrc/pm_undistort.hpp) on 1600 x 1200 and 6048 x 4032 images of 3 channels through
SIMPLE_RADIAL and OPENCV_FISHEYE cameras, to the output camera of mpmvs_undistort_camera (blank_pixels = 0).

Per shape and model: wall time of the call (host buffers in and out: stage copies, transfers, kernel), the kernel's own time
(HIP events, mpmvs_undistort_kernel_ms), the bytes the kernel has to move (3 W H source bytes + 3 W' H' output bytes) and their
share of the 8 TB/s HBM peak -- to be set beside the 41 % of k_ingest_quads, the project's yardstick for a byte-gather kernel
(profiles/EXPERIMENTS.md 57) -- and the time of the host statement mpmvs_host_undistort_u8 on the OpenMP team.  Medians,
quartiles and extremes of --reps repetitions after --warmup, the protocol of tools/bench_ingest.py.  --trace: three calls per
case only, for `rocprofv3 --kernel-trace --stats -- python tools/bench_undistort.py --trace`.  Prints a table and one JSON line."""
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

engine = importlib.import_module("mp-mvs_amd.engine")
hostlib = importlib.import_module("mp-mvs_amd.hostlib")
colmap = importlib.import_module("mp-mvs_amd.colmap")

HBM_PEAK = 8.0e12   # bytes / s


def stats(xs):
    a = np.sort(np.asarray(xs, np.float64))
    return {"median": round(float(np.median(a)), 3), "q1": round(float(np.percentile(a, 25)), 3), "q3": round(float(np.percentile(a, 75)), 3),
            "min": round(float(a[0]), 3), "max": round(float(a[-1]), 3), "n": int(a.size)}


def camera(name, w, h):
    f = 0.9 * w
    if name == "SIMPLE_RADIAL":
        return [f, w / 2 - 3.25, h / 2 + 1.5, -0.12]
    return [f, f, w / 2 - 3.25, h / 2 + 1.5, -0.03, 0.012, -0.004, 0.0007]   # OPENCV_FISHEYE


def run_case(name, w, h, reps, warmup, host_reps):
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    prm = camera(name, w, h)
    dst = engine.undistort_camera(name, prm, w, h)
    _, fns = engine.load()
    wall, kern = [], []
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        out = engine.undistort_u8(img, name, prm, dst)
        t1 = time.perf_counter()
        if r >= warmup:
            wall.append((t1 - t0) * 1e3)
            kern.append(fns["undistort_kernel_ms"]() * 1e3)   # microseconds
    host = []
    for r in range(host_reps + 1):
        t0 = time.perf_counter()
        ref = hostlib.undistort_u8(img, colmap.CAMERA_MODELS.index(name), prm, dst)
        if r >= 1:
            host.append((time.perf_counter() - t0) * 1e3)
    assert out.tobytes() == ref.tobytes(), "device and host statement differ"
    need = 3 * w * h + 3 * dst[1] * dst[2]
    res = {"out_size": [dst[1], dst[2]], "bytes_needed": need, "wall_ms": stats(wall), "kernel_us": stats(kern)}
    if host:
        res["host_ms"] = stats(host)
        res["host_threads"] = hostlib.undistort_threads()
    k = res["kernel_us"]["median"]
    res["hbm_share"] = round(need / (k * 1e-6) / HBM_PEAK, 4) if k > 0 else None
    print(f"{name:15s} {w} x {h} -> {dst[1]} x {dst[2]}: kernel {k:9.1f} us (quartiles {res['kernel_us']['q1']:.1f} .. {res['kernel_us']['q3']:.1f}), "
          f"{need} bytes = {100 * (res['hbm_share'] or 0):.1f} % of the HBM peak; call {res['wall_ms']['median']:.2f} ms wall"
          + (f"; host statement {res['host_ms']['median']:.1f} ms on {res['host_threads']} threads" if host else ""), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    reps, warmup, host_reps = (3, 0, 0) if args.trace else (args.reps, args.warmup, args.host_reps)
    out = {}
    for w, h in ((1600, 1200), (6048, 4032)):
        for name in ("SIMPLE_RADIAL", "OPENCV_FISHEYE"):
            out[f"{name}_{w}x{h}"] = run_case(name, w, h, reps, warmup, host_reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
