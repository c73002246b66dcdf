#!/usr/bin/env python3
"""Timing of the COLMAP converter on a synthetic model: 2000 images, 1 M points with tracks of mean length ~6 plus a tail
of 300-long tracks.  Reports
  - mpmvs_view_select: device time of its kernels (HIP events) and wall time of the call,
  - read_model + convert wall times from a .bin model on disk (stage by stage),
  - the reference's cost: a pairwise literal statement of its score ([p for p in ids_i if p in ids_j], then the angles),
    timed on a sample of pairs and extrapolated to all N (N - 1) / 2 pairs (an extrapolation, not a run).

  python tools/bench_colmap.py [--images 2000] [--points 1000000] [--tail 2000] [--sample 20]"""
import argparse
import importlib
import json
import os
import struct
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synth_model(n, n_points, tail, tail_len=300, seed=5):
    """(centers, qvec, tvec, xyz, obs_off, obs_pt): point-major tracks of neighbouring images, scattered into per-image lists"""
    rng = np.random.default_rng(seed)
    a = np.linspace(0, 2 * np.pi, n, endpoint=False)
    C = np.stack([10 * np.cos(a), 10 * np.sin(a), -20 + rng.normal(0, 0.5, n)], 1)
    xyz = rng.normal(0, 2.0, (n_points, 3))
    L = 2 + rng.poisson(4, n_points)
    L[:tail] = tail_len
    pt = np.repeat(np.arange(n_points, dtype=np.int32), L)
    base = np.repeat(rng.integers(0, n, n_points), L)
    img = (base + rng.integers(-15, 16, len(pt))) % n
    tail_obs = pt < tail
    img[tail_obs] = rng.integers(0, n, int(tail_obs.sum()))
    order = np.lexsort((rng.random(len(pt)), img))
    obs_pt = pt[order]
    obs_off = np.concatenate([[0], np.cumsum(np.bincount(img, minlength=n))]).astype(np.int64)
    # cameras on a circle 20 in front of the points, all with the identity rotation
    q = np.tile([1.0, 0.0, 0.0, 0.0], (n, 1))
    t = -C
    return C, q, t, xyz, obs_off, obs_pt


def write_bin(d, q, t, xyz, obs_off, obs_pt, jpeg):
    sp, im = os.path.join(d, "sparse"), os.path.join(d, "images")
    os.makedirs(sp)
    os.makedirs(im)
    n = len(q)
    with open(os.path.join(sp, "cameras.bin"), "wb") as f:
        f.write(struct.pack("<QiiQQ4d", 1, 1, 1, 64, 48, 50.0, 50.0, 32.0, 24.0))
    with open(os.path.join(sp, "images.bin"), "wb") as f:
        f.write(struct.pack("<Q", n))
        for i in range(n):
            ids = obs_pt[obs_off[i]:obs_off[i + 1]]
            rec = np.zeros(len(ids), [("x", "<f8"), ("y", "<f8"), ("id", "<i8")])
            rec["id"] = ids.astype(np.int64) + 1
            f.write(struct.pack("<i4d3di", i + 1, *q[i], *t[i], 1) + b"im%05d.jpg\0" % i + struct.pack("<Q", len(ids)) + rec.tobytes())
    counts = np.bincount(obs_pt, minlength=len(xyz))
    with open(os.path.join(sp, "points3D.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(xyz)))
        for k in range(len(xyz)):   # tracks are written empty-valued (image 0, index 0): the converter does not read them
            f.write(struct.pack("<Q3d3BdQ", k + 1, *xyz[k], 0, 0, 0, 0.5, counts[k]) + bytes(8 * counts[k]))
    for i in range(n):
        with open(os.path.join(im, "im%05d.jpg" % i), "wb") as f:
            f.write(jpeg)


def literal_pair(ids_i, ids_j, ci, cj, xyz):
    common = [p for p in ids_i if p in ids_j]
    th = []
    for p in common:
        a, b = ci - xyz[p], cj - xyz[p]
        th.append((180 / np.pi) * np.arccos(np.dot(a, b) / np.linalg.norm(a) / np.linalg.norm(b)))
    return len(common), th


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=2000)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--tail", type=int, default=2000, help="points with 300-long tracks")
    ap.add_argument("--sample", type=int, default=20, help="pairs timed with the literal statement")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    colmap = importlib.import_module("mp-mvs_amd.colmap")
    engine = importlib.import_module("mp-mvs_amd.engine")
    _, fns = engine.load()
    C, q, t, xyz, off, pts = synth_model(a.images, a.points, a.tail)
    n = a.images
    L = np.bincount(pts, minlength=a.points)
    pair_events = int((L * (L - 1) // 2).sum())
    num_view = min(20, n - 1)
    colmap.view_select(C, xyz, off, pts, num_view, a.device)   # warm-up: code objects, pool buffers
    walls, kms = [], []
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        colmap.view_select(C, xyz, off, pts, num_view, a.device)
        walls.append(time.perf_counter() - t0)
        kms.append(fns["view_select_kernel_ms"]())
    from PIL import Image
    import io
    buf = io.BytesIO()
    Image.fromarray(np.full((48, 64), 128, np.uint8)).save(buf, "JPEG")
    res = {}
    with tempfile.TemporaryDirectory() as d:
        dense = os.path.join(d, "dense")
        write_bin(dense, q, t, xyz, off, pts, buf.getvalue())
        t0 = time.perf_counter()
        m = colmap.read_model(os.path.join(dense, "sparse"), ".bin")
        res["read_model_s"] = time.perf_counter() - t0
        assert m.n_images == n and len(m.obs_pt) == len(pts)
        t0 = time.perf_counter()
        stages = colmap.convert(dense, os.path.join(d, "out"), device=a.device)
        res["convert_s"] = time.perf_counter() - t0
        res["convert_stages_s"] = {k: round(v, 4) for k, v in stages.items()}
    rng = np.random.default_rng(1)
    lists = [pts[off[i]:off[i + 1]] + 1 for i in range(n)]
    xyz1 = np.concatenate([np.zeros((1, 3)), xyz])   # ids 1..P as in the model file
    t0 = time.perf_counter()
    for _ in range(a.sample):
        i, j = sorted(rng.choice(n, 2, replace=False))
        literal_pair(lists[i], lists[j], C[i], C[j], xyz1)
    per_pair = (time.perf_counter() - t0) / a.sample
    n_pairs = n * (n - 1) // 2
    out = dict(images=n, points=a.points, observations=int(len(pts)), mean_track=float(L.mean()), pair_events=pair_events,
               view_select_kernel_ms=round(float(np.median(kms)), 3), view_select_wall_ms=round(1000 * float(np.median(walls)), 3),
               read_model_s=round(res["read_model_s"], 3), convert_s=round(res["convert_s"], 3), convert_stages_s=res["convert_stages_s"],
               literal_per_pair_s=round(per_pair, 5), literal_extrapolated_core_hours=round(per_pair * n_pairs / 3600, 2))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
