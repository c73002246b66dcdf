#!/usr/bin/env python3
"""The sky-segmentation network on the GPU (mpmvs_skyseg_*, csrc/pm_skyseg.hpp): time per image.

  python tools/bench_skyseg.py [--model DIR] [--reps 30] [--warmup 5]
  rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_skyseg.py --trace      (per-kernel share, a run of its own)

Weights: --model DIR holds skysegsmall_sim-opt-fp16.{param,bin}; without it the same topology (tests/skyseg_common.u2net_small)
with seeded weights is written to a temporary folder -- the work per image is the same, 28.45 GMAC.

Printed, and repeated in one JSON line:
  network      device time of the kernels of one mpmvs_skyseg_run (HIP events around the launches, no copies), median / quartiles
               of --reps runs after --warmup; the launch count; the fraction of the fp32-matrix roofline
               (2 x MACs / 157.3 TFLOP/s = 0.36 ms for the real model)
  run_u8       the same with the preprocessing in front (1600 x 1200 B,G,R bytes: one pyrDown level, resize, normalise), and the
               host wall time of the whole call (upload and download included)
  full         wall time of one image of GenerateSkyRegionMask without the files: run_u8 + ResizeLinear of the mask (host) +
               mpmvs_sky_bilateral at 1600 x 1200
  shapes       the six convolution shapes that carry 86 % of the MACs, each timed alone (a one-layer net, device events) and
               multiplied by the number of such layers in the model: their share of the network time
  yardsticks   (not asserted anywhere) the same graph through torch: on the GPU (eager, MIOpen; in a child process with a time
               limit -- left out with a note if MIOpen cannot prepare its kernels) and on the CPU (16 threads, fp32)"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import skyseg_common as sc  # noqa: E402

ROOFLINE_TFLOPS = 157.3  # fp32 matrix peak of the MI355X
STEM = sc.MODEL_STEM
# (C_in, C_out, size): layers of that shape in U^2-Net-small; together 86 % of the MACs
BIG_SHAPES = [(128, 64, 384), (32, 64, 384), (64, 16, 384), (128, 64, 192), (64, 64, 192), (32, 64, 192)]


def stats(xs):
    a = np.sort(np.asarray(xs, np.float64))
    return {"median": round(float(np.median(a)), 4), "q1": round(float(np.percentile(a, 25)), 4), "q3": round(float(np.percentile(a, 75)), 4),
            "min": round(float(a[0]), 4), "max": round(float(a[-1]), 4), "n": int(a.size)}


def model_files(model_dir, tmp):
    if model_dir:
        return os.path.join(model_dir, STEM + ".param"), os.path.join(model_dir, STEM + ".bin"), "real weights"
    g, out = sc.u2net_small()
    pp, bp = sc.write_pair(tmp, g.emit(), seed=1, stem=STEM)
    return pp, bp, "seeded weights"


def torch_graph(pp, bp, device, dtype=torch.float32):
    """the graph as a function x -> output blob "1959", weights resident on `device`"""
    import torch.nn.functional as F
    _, _, layers = sc.read_param(pp)
    W = {k: (torch.from_numpy(w.copy()).to(device, dtype), torch.from_numpy(b.copy()).to(device, dtype) if b is not None else None)
         for k, (w, b) in sc.read_weights(layers, bp).items()}
    live = sc.live_blobs(layers, "1959")

    def run(x):
        blobs = {}
        for t, name, ins, outs, prm in layers:
            if not set(outs) & live:
                continue
            a = [blobs[i] for i in ins]
            if t == "Input":
                r = [x]
            elif t == "Convolution":
                w, b = W[name]
                cout, k = int(prm[0]), int(prm[1])
                y = F.conv2d(a[0], w.reshape(cout, a[0].shape[1], k, k), b, padding=int(prm.get(4, 0)), dilation=int(prm.get(2, 1)))
                act = int(prm.get(9, 0))
                r = [F.relu(y) if act == 1 else torch.sigmoid(y) if act == 4 else y]
            elif t == "Split":
                r = [a[0]] * len(outs)
            elif t == "Pooling":
                r = [F.max_pool2d(a[0], 2, 2, ceil_mode=True)]
            elif t == "Concat":
                r = [torch.cat(a, 1)]
            elif t == "Interp":
                r = [F.interpolate(a[0], size=(int(prm[3]), int(prm[4])), mode="bilinear", align_corners=False)]
            elif t == "BinaryOp":
                r = [a[0] + a[1]]
            else:
                r = [torch.sigmoid(a[0])]
            for o, v in zip(outs, r):
                blobs[o] = v
        return blobs["1959"]
    return run


def yardstick(pp, bp, device, reps, warmup):
    x = torch.from_numpy(sc.probe_sky_image())[None].to(device)
    run = torch_graph(pp, bp, device)
    ms = []
    with torch.no_grad():
        for r in range(warmup + reps):
            if device != "cpu":
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            y = run(x)
            if device != "cpu":
                torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
    return stats(ms[warmup:]), float(y.float().mean())


def shape_times(engine, tmp, reps, warmup):
    """each big shape alone: device ms of a one-convolution net"""
    out = {}
    for cin, cout, size in BIG_SHAPES:
        g = sc.Graph(cin, size, size)
        c = g.conv("in0", cout)
        pp, bp = sc.write_pair(tmp, g.emit(), seed=cin + cout, stem=f"shape_{cin}_{cout}_{size}")
        net = engine.SkySeg(pp, bp, size, size, c)
        x = sc.noise_image(cin, size, size, 1)
        ms = []
        for r in range(warmup + reps):
            net.run(x)
            ms.append(net.ms()[0])
        net.close()
        macs = cin * cout * 9 * size * size
        med = float(np.median(ms[warmup:]))
        out[f"{cin}x{cout}@{size}"] = {"ms": round(med, 4), "tflops": round(2 * macs / med / 1e9, 1)}
    return out


def count_shapes(pp):
    """number of convolution layers per (C_in, C_out, size) in the model, from the .param and the 384 x 384 input"""
    _, _, layers = sc.read_param(pp)
    shape = {}
    counts = {}
    for t, name, ins, outs, prm in layers:
        if t == "Input":
            shape[outs[0]] = (3, 384, 384)
        elif t == "Convolution":
            c, h, w = shape[ins[0]]
            shape[outs[0]] = (int(prm[0]), h, w)
            if int(prm[1]) == 3:
                counts[(c, int(prm[0]), h)] = counts.get((c, int(prm[0]), h), 0) + 1
        elif t == "Split":
            for o in outs:
                shape[o] = shape[ins[0]]
        elif t == "Pooling":
            c, h, w = shape[ins[0]]
            shape[outs[0]] = (c, (h + 1) // 2, (w + 1) // 2)
        elif t == "Interp":
            shape[outs[0]] = (shape[ins[0]][0], int(prm[3]), int(prm[4]))
        elif t == "Concat":
            shape[outs[0]] = (sum(shape[i][0] for i in ins),) + shape[ins[0]][1:]
        else:
            shape[outs[0]] = shape[ins[0]]
    return counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default=os.environ.get("MPMVS_SKY_MODEL"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace", action="store_true", help="a short run of the bare network and of run_u8 only, for rocprofv3")
    ap.add_argument("--yardstick", choices=["gpu", "cpu"], help="(internal) print the torch timing of the graph and exit")
    ap.add_argument("--no-yardsticks", action="store_true")
    ap.add_argument("--gpu-yardstick-timeout", type=int, default=240)
    a = ap.parse_args()
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    tmp = tempfile.mkdtemp(prefix="skyseg_bench_")
    pp, bp, what = model_files(a.model, tmp)
    if a.yardstick:
        st, mean = yardstick(pp, bp, "cuda" if a.yardstick == "gpu" else "cpu", a.reps if a.yardstick == "gpu" else 5, a.warmup if a.yardstick == "gpu" else 1)
        print(json.dumps({"ms": st, "mean_output": mean}))
        return
    engine = importlib.import_module("mp-mvs_amd.engine")
    hostlib = importlib.import_module("mp-mvs_amd.hostlib")
    fusion = importlib.import_module("mp-mvs_amd.fusion")
    info = engine.skyseg_inspect(pp, bp, 384, 384, "1959")
    net = engine.SkySeg(pp, bp, 384, 384, "1959")
    x = sc.probe_sky_image()
    rs = np.random.RandomState(0)
    yy, xx = np.mgrid[0:1200, 0:1600]
    photo = np.clip(np.stack([200 - yy // 8, 150 + 0 * xx, 90 + xx // 16], -1) + rs.randint(-10, 11, (1200, 1600, 3)), 0, 255).astype(np.uint8)
    if a.trace:
        for _ in range(3):
            net.run(x)
            net.run_u8(photo)
        print(json.dumps({"trace": True, "weights": what, "launches_per_run": net.launches}))
        return
    roof_ms = 2 * info["macs"] / (ROOFLINE_TFLOPS * 1e12) * 1e3
    res = {"weights": what, "macs": info["macs"], "launches": net.launches, "roofline_ms": round(roof_ms, 4)}
    net_ms, wall = [], []
    for r in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        p = net.run(x)
        wall.append((time.perf_counter() - t0) * 1e3)
        net_ms.append(net.ms()[0])
    res["network_ms"] = stats(net_ms[a.warmup:])
    res["network_wall_ms"] = stats(wall[a.warmup:])
    res["fraction_of_roofline"] = round(roof_ms / res["network_ms"]["median"], 4)
    res["sky_fraction"] = round(float((p > 0.5).mean()), 4)
    u8_dev, u8_wall, full_wall = [], [], []
    for r in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        prob = net.run_u8(photo)
        t1 = time.perf_counter()
        mask = hostlib.resize_linear(prob[0], 1600, 1200)
        fusion.sky_bilateral(photo, mask)
        t2 = time.perf_counter()
        u8_wall.append((t1 - t0) * 1e3)
        full_wall.append((t2 - t0) * 1e3)
        u8_dev.append(sum(net.ms()))
    res["run_u8_device_ms"] = stats(u8_dev[a.warmup:])
    res["run_u8_wall_ms"] = stats(u8_wall[a.warmup:])
    res["full_image_wall_ms"] = stats(full_wall[a.warmup:])
    net.close()
    # the six big shapes, each alone
    per_shape = shape_times(engine, tmp, a.reps, a.warmup)
    counts = count_shapes(pp)
    big_ms = 0.0
    for cin, cout, size in BIG_SHAPES:
        k = f"{cin}x{cout}@{size}"
        per_shape[k]["layers"] = counts.get((cin, cout, size), 0)
        big_ms += per_shape[k]["ms"] * per_shape[k]["layers"]
    res["big_shapes"] = per_shape
    res["big_shapes_ms"] = round(big_ms, 4)
    res["big_shapes_share_of_network"] = round(big_ms / res["network_ms"]["median"], 4)
    if not a.no_yardsticks:
        for dev, limit in (("gpu", a.gpu_yardstick_timeout), ("cpu", 600)):
            cmd = [sys.executable, os.path.abspath(__file__), "--yardstick", dev, "--reps", str(a.reps), "--warmup", str(a.warmup)] + (["--model", a.model] if a.model else [])
            try:
                out = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
                res[f"torch_{dev}"] = json.loads(out.stdout.strip().splitlines()[-1]) if out.returncode == 0 else {"left_out": out.stderr.strip().splitlines()[-1:]}
            except subprocess.TimeoutExpired:
                res[f"torch_{dev}"] = {"left_out": f"no result within {limit} s (MIOpen preparing its kernels)" if dev == "gpu" else f"no result within {limit} s"}
    for k, v in res.items():
        print(f"{k}: {v}", flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
