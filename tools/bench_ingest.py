#!/usr/bin/env python3
"""Image upload through the two entries of include/mpmvs.h: mpmvs_set_views (fp32 arrays; the host sweeps them to find out that
they are bytes) against mpmvs_set_views_u8 (the bytes themselves; oversized views are shrunk on the device, csrc/pm_ingest.hpp).

  A  cfg-1 shape: 9 integer views of 1600 x 1200, nothing resampled.
  B  oversized shape: 9 views of 6048 x 4032 -> 3200 x 2133.  The fp32 side is what a caller of the C ABI has to do today:
     hostlib.resize_linear of the nine (already widened) images, then set_views.

Per shape and entry: host time of the call(s), and time until the context's stream is idle (the span ends in mpmvs_wait, which
synchronises the stream).  The two entries alternate within one process; medians, quartiles and extremes of --reps repetitions
after --warmup.  --trace: a short run of shape B only, for `rocprofv3 --kernel-trace --stats -- python tools/bench_ingest.py --trace`:
the resampling kernels and k_pack_quads_f32 on the same output size in one trace; the bytes each has to move are printed for the
share-of-peak arithmetic.  Prints a table and one JSON line."""
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

pm = importlib.import_module("mp-mvs_amd")
engine = importlib.import_module("mp-mvs_amd.engine")
hostlib = importlib.import_module("mp-mvs_amd.hostlib")

N_VIEWS = 9
CENTERS = [(0.0, 0.0, 0.0)] + [(0.15 * dx, 0.15 * dy, 0.0) for dx, dy in pm.synth._RING]


def stats(xs):
    a = np.sort(np.asarray(xs, np.float64))
    return {"median": round(float(np.median(a)), 3), "q1": round(float(np.percentile(a, 25)), 3), "q3": round(float(np.percentile(a, 75)), 3),
            "min": round(float(a[0]), 3), "max": round(float(a[-1]), 3), "n": int(a.size)}


def timed(h, fn):
    """(host ms of fn, ms until the stream is idle)"""
    t0 = time.perf_counter()
    fn()
    t1 = time.perf_counter()
    h.wait()
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t0) * 1e3


def shape(src_w, src_h, w, h, seed):
    rng = np.random.default_rng(seed)
    cams = pm.synth.scene_cameras(w, h, CENTERS)
    bytes_ = [rng.integers(0, 256, (src_h, src_w), dtype=np.uint8) for _ in range(N_VIEWS)]
    return cams, bytes_


def run_shape(name, src_w, src_h, w, h, reps, warmup):
    cams, bytes_ = shape(src_w, src_h, w, h, 7)
    floats = [b.astype(np.float32) for b in bytes_]
    resample = (src_w, src_h) != (w, h)
    old, new = engine.create(0), engine.create(0)
    res = {k: [] for k in ("f32_host", "f32_idle", "u8_host", "u8_idle")}

    def old_entry():
        old.set_views(cams, [hostlib.resize_linear(f, w, h) for f in floats] if resample else floats)

    def new_entry():
        new.set_views_u8(cams, bytes_)

    for r in range(warmup + reps):
        a = timed(old, old_entry)
        b = timed(new, new_entry)
        if r >= warmup:
            res["f32_host"].append(a[0])
            res["f32_idle"].append(a[1])
            res["u8_host"].append(b[0])
            res["u8_idle"].append(b[1])
    assert old.texture_format() == new.texture_format() == ("f32" if resample else "u8")
    out = {k: stats(v) for k, v in res.items()}
    for k, s in out.items():
        print(f"{name} {k:9s} median {s['median']:9.3f} ms   quartiles {s['q1']:9.3f} .. {s['q3']:9.3f}   range {s['min']:9.3f} .. {s['max']:9.3f}   n {s['n']}", flush=True)
    return out


def trace_run(reps):
    """shape B through both entries, the host resize done once outside: the trace then holds k_ingest_quads<true>, k_ingest_pad and, on the
    same output size, k_pack_quads_f32 / k_pad"""
    src_w, src_h, w, h = 6048, 4032, 3200, 2133
    cams, bytes_ = shape(src_w, src_h, w, h, 7)
    small = [engine.resize_u8(b, w, h) for b in bytes_]     # (k_ingest_pad with apron 0)
    old, new = engine.create(0), engine.create(0)
    for _ in range(reps):
        old.set_views(cams, small)
        old.wait()
        new.set_views_u8(cams, bytes_)
        new.wait()
    need = {"k_ingest_quads<true> per view: read src bytes + write 16 B texels": src_w * src_h + 16 * w * h,
            "k_pack_quads_f32 per view: read 4 B pixels + write 16 B texels": 4 * w * h + 16 * w * h,
            "k_ingest_pad (reference image): read src bytes + write padded fp32": src_w * src_h + 4 * (w + 40) * (h + 40),
            "k_ingest_pad (probe, apron 0): read src bytes + write fp32": src_w * src_h + 4 * w * h}
    for k, v in need.items():
        print(f"{k}: {v} bytes")
    return {"bytes_needed": need, "reps": reps, "views": N_VIEWS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="A,B")
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    out = {}
    if args.trace:
        out["trace"] = trace_run(3)
    else:
        if "A" in args.shapes:
            out["A_1600x1200"] = run_shape("A", 1600, 1200, 1600, 1200, args.reps, args.warmup)
        if "B" in args.shapes:
            out["B_6048x4032_to_3200x2133"] = run_shape("B", 6048, 4032, 3200, 2133, args.reps, args.warmup)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
