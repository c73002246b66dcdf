#!/usr/bin/env python3
"""bench.py -- Mpix/s of estimated depth+normal for the MP-MVS PatchMatch hot path.

Default workload (BASELINE.json configs[1]): one "step" = one PatchMatchCUDA::Run() (reference src/PatchMatch.cu:1188-1254)
over one reference-image Problem: 1 reference + 8 source views, 1600x1200, single scale (max_scale = 0), photometric only,
3 red/black iterations, synthetic seeded scene.  What is timed:

  value            inputs resident in HBM when the timed region starts; a step is the reference's Run() in full, i.e. its
                   launches AND the device-to-host copies that end it (ref .cu:1246-1251: planes + costs, 38 MB, into pinned
                   host buffers), one blocking call per step (mpmvs_run_get) as the reference's Run() is
  pipelined_value  the same steps through mpmvs_run_get_async (the maps of step i cross PCIe while step i + 1 computes); reported,
                   never `value`
  resident_value   the same without the D2H block (kernels only; round 1's headline number)
  with_h2d_value   SURVEY 8(d)'s wording of the metric: upload of the 9 images (mpmvs_set_views: host conversion, H2D,
                   texture packing) + Run() + D2H per step -- reported, never `value` (the bench contract keeps inputs resident)

`roofline` describes the dominant kernel (k_update) from HIP events on the context's stream; `secondary` carries the other
single-GPU configurations of BASELINE.json (cfg 2, cfg 3) and the two non-headline formats of cfg 1 (fp32 textures, 20 source
views), each with its own k_update average and roofline fraction; `cpu_baseline` is the oracle on the host cores.

A plain run (`python bench.py --gpus 1 --steps K --warmup W`) sets up, warms up, times the K steps and prints the line: `value`
and the figures read from those same steps (`roofline`, `kernel_ms_per_step`, `within_1pct_of_gt`).  Every other reading --
pipelined_value, resident_value, the with-upload readings (`value_survey_8d*`), `secondary`, `cpu_baseline`, and with N > 1 the
peer tables, the peer-copy check and configs[4] -- runs only with --full.  --dump-outputs DIR writes what the last timed step
returned as .npy files.

Multi-GPU (--gpus N): one process per GPU.  Under torch.distributed.run (RANK / WORLD_SIZE in the environment) this process is
one rank; started plainly (`python bench.py --gpus N`), it becomes a launcher that never touches the GPU: it starts N fresh child
processes with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set, forwards rank 0's JSON line and exits non-zero if any rank failed
(no exec of a process that has initialised HIP).  cfg 1 Problems are independent, one per rank per step, no data-path collective
(weak scaling); RCCL only provides the barrier and the max-reduce of the time.  With N > 1 the same invocation then runs
configs[4] once (`secondary.cfg4`, below) so that one driver command also exercises the exchange.

--workload cfg4 (BASELINE.json configs[4]): 64 reference-image Problems (8x8 camera grid, 8 nearest neighbours as sources)
sharded over the ranks, the shipped schedule (photometric 3 scales -> geometric + planar prior -> geometric), ONE
all_gather_into_tensor of the depth maps per pass over RCCL (mp-mvs_amd/schedule.py); strong scaling.
"""
import argparse
import ctypes
import importlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

W, H, V, ITERS = 1600, 1200, 8, 3
FLOP_PER_EVAL = 2144.0        # one (hypothesis, view) NCC evaluation = 36 taps
HYP_PER_UPDATE = 14           # 8 propagated + current + 5 refinement
PEAK_VALU_TFLOPS = 157.3      # MI355X_MICROARCH.md: peak FP32 vector
PEAK_HBM_GBPS = 8000.0        # MI355X_MICROARCH.md: HBM3E peak
PRIOR_SEED_OFFSET = 0x9E3779B97F4A7C15


# ---------------------------------------------------------------------------------------------------------------------
# scenes (seeded, cached on local disk: rendering 9 x 1600x1200 takes ~30 s of numpy)
# ---------------------------------------------------------------------------------------------------------------------
def _cache_dir():
    d = os.path.join(os.environ.get("TMPDIR", "/tmp"), "mpmvs_scene_cache")
    os.makedirs(d, exist_ok=True)
    return d


def _cam_bytes(cam):
    return np.frombuffer(ctypes.string_at(ctypes.addressof(cam), ctypes.sizeof(cam)), np.uint8).copy()


def _cam_from(pm, raw):
    cam = pm.Camera()
    b = raw.tobytes()
    ctypes.memmove(ctypes.addressof(cam), b, len(b))
    return cam


def load_views(pm, w, h, centers, tag, rank=0, world=1, barrier=None):
    """cameras, unrounded fp32 images and ground-truth depths of the views at `centers` (one .npz per view; with world > 1 the
    ranks share the rendering)"""
    sc_mod = pm.synth
    paths = [os.path.join(_cache_dir(), f"view_{tag}_{w}x{h}_{sc_mod.SCENE_SEED}_{i:03d}.npz") for i in range(len(centers))]
    missing = [i for i, p in enumerate(paths) if not os.path.exists(p)]
    if missing:
        mine = [i for i in missing if i % world == rank]
        if mine:
            sc = sc_mod.make_scene(w, h, centers, quantize=False, only=set(mine))   # every view keeps its rotation of the full scene
            for i in mine:
                v = sc.views[i]
                tmp = paths[i] + f".{os.getpid()}.tmp.npz"
                np.savez(tmp, img=v.image, gt=v.gt_depth, cam=_cam_bytes(v.cam))
                os.replace(tmp, paths[i])
    if barrier is not None:
        barrier()   # unconditional: a rank that finds the cache complete must still meet the ranks that are filling it
    cams, imgs, gts = [], [], []
    for p in paths:
        z = np.load(p)
        cams.append(_cam_from(pm, z["cam"]))
        imgs.append(z["img"])
        gts.append(z["gt"])
    return cams, imgs, gts


def problem_centers(pm, n_src, spacing=0.15):
    ring = list(pm.synth._RING)
    if n_src > 8:   # second ring of the 5x5 grid, nearest first
        far = sorted(((dx * dx + dy * dy, dx, dy) for dx in range(-2, 3) for dy in range(-2, 3) if max(abs(dx), abs(dy)) == 2))
        ring += [(dx, dy) for _, dx, dy in far]
    return [(0.0, 0.0, 0.0)] + [(spacing * dx, spacing * dy, 0.0) for dx, dy in ring[:n_src]]


def load_scene(pm, w, h, v, quantize):
    """(cams, images, gt depth of the reference view) of one Problem: reference + v sources"""
    cams, imgs, gts = load_views(pm, w, h, problem_centers(pm, v), f"p{v}")
    if quantize:
        imgs = [np.rint(im).astype(np.float32) for im in imgs]
    return cams, imgs, gts[0]


# ---------------------------------------------------------------------------------------------------------------------
def kernel_build_sha256():
    """identifies the kernel BUILD a profile belongs to: the hash of the HIP library that is loaded (the build is deterministic, and a
    comment-only edit of the sources gives the same binary); tools/summarize_prof.py writes the same hash into its summary"""
    import hashlib
    path = os.environ.get("MPMVS_HIP_LIB", os.path.join(ROOT, "mp-mvs_amd", "csrc", "libmpmvs_hip.so"))
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]


def profile_counters(upd_avg_ms):
    """PMC figures of k_update from the latest committed `profiles/*pmc_summary*` file (rocprofv3 --pmc passes of this same
    command, tools/profile_gpu.sh: PMC cannot be read in-process) -- but only if that profile describes THIS build and THIS
    run: its recorded hash of the HIP library must equal that of the library in use and its kernel-trace average of k_update must lie within 3 % of
    the average this run measured with HIP events.  Otherwise every figure is None and `reason` says why.
    FETCH_SIZE / WRITE_SIZE are KiB at the L2's memory side.  MI355X_MICROARCH.md: on gfx950 FETCH_SIZE tallies 128-byte
    requests at 64 bytes (exactly half for wide coalesced streaming reads), other access widths are uncalibrated: this kernel's
    reads are L2 misses of 8 / 16-byte gathers plus scratch refills, so the bytes lie between the raw sum (`traffic`) and the
    sum with FETCH_SIZE doubled (`traffic_if_fetch_doubled`)."""
    none = {"traffic": None, "traffic_if_fetch_doubled": None, "valu_busy": None, "source": None, "reason": None}
    pdir = os.path.join(ROOT, "profiles")
    names = sorted(n for n in os.listdir(pdir) if n.endswith(".txt") and "pmc_summary" in n) if os.path.isdir(pdir) else []
    if not names:
        return dict(none, reason="no profiles/*pmc_summary*.txt")
    name = names[-1]   # last in name order = latest round
    vals, kern, meta, trace_avg = {}, None, {}, None
    for line in open(os.path.join(pdir, name)):
        t = line.strip()
        if t.startswith("#") and ":" in t:
            k, v = t[1:].split(":", 1)
            meta[k.strip()] = v.strip()
        elif t.startswith("k_update") and " avg " in t and trace_avg is None:
            trace_avg = float(t.split(" avg ")[1].split()[0])
        elif t.startswith("k_"):
            kern = t.split()[0]
        elif kern == "k_update" and "avg=" in t:
            vals[t.split()[0]] = float(t.split("avg=")[1])
    src = f"profiles/{name}"
    # since round 5 one k_update dispatch chains the passes of a scale (6 in cfg 1): the profile's per-dispatch figures are
    # brought to ONE PASS, the unit `roofline` is quoted in (a pass = what rounds 1-4 launched as one kernel)
    passes = float(meta.get("k_update_passes_per_dispatch", "1"))
    if trace_avg is not None:
        trace_avg /= passes
    vals = {k: v / passes for k, v in vals.items()}
    if meta.get("kernel_build_sha256") != kernel_build_sha256():
        return dict(none, source=src, reason=f"{src} was collected on another kernel build (library hash {meta.get('kernel_build_sha256')} != {kernel_build_sha256()})")
    if trace_avg is None or abs(trace_avg - upd_avg_ms) > 0.03 * upd_avg_ms:
        return dict(none, source=src, reason=f"{src}: k_update averaged {trace_avg} ms there, {upd_avg_ms:.4f} ms in this run (more than 3 % apart)")
    out = dict(none, source=src + f" (git {meta.get('git_head', '?')}, k_update trace average {trace_avg:.4f} ms per pass, {passes:g} passes per dispatch; command: {meta.get('command', '?')})")
    if "FETCH_SIZE" in vals and "WRITE_SIZE" in vals:
        out["traffic"] = (vals["FETCH_SIZE"] + vals["WRITE_SIZE"]) * 1024.0
        out["traffic_if_fetch_doubled"] = (2.0 * vals["FETCH_SIZE"] + vals["WRITE_SIZE"]) * 1024.0
    if "SQ_ACTIVE_INST_VALU" in vals and "GRBM_GUI_ACTIVE" in vals:
        # executed-work utilisation: SQ_ACTIVE_INST_VALU x 4 / (1024 SIMDs x GRBM_GUI_ACTIVE / 8), per k_update launch
        out["valu_busy"] = round(vals["SQ_ACTIVE_INST_VALU"] * 4.0 / (1024.0 * vals["GRBM_GUI_ACTIVE"] / 8.0), 4)
    return out


def roofline_of(upd_avg_ms, w, h, v):
    """fraction of the fp32 vector peak at SURVEY 8d's NOMINAL work per launch (14 hypotheses x v views x 2144 flop per pixel
    of one colour); the kernel executes less than that (hoisted weights and homography, skipped zero-weight views)"""
    flops = (w * h / 2) * HYP_PER_UPDATE * v * FLOP_PER_EVAL
    tflops = flops / (upd_avg_ms * 1e-3) / 1e12
    return flops, tflops


def pinned(shape):
    import torch
    return torch.empty(shape, dtype=torch.float32, pin_memory=True).numpy()


DUMP_LIMIT_BYTES = 60 * 10 ** 6   # under 64 MB in all, .npy headers included


def dump_outputs(path, arrays):
    """--dump-outputs: every array as <path>/<name>.npy in float32 (inputs and seeds are fixed by the arguments, so two builds can
    be compared file for file)"""
    os.makedirs(path, exist_ok=True)
    arrays = {k: np.ascontiguousarray(v, np.float32) for k, v in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit(f"--dump-outputs: {total} bytes exceed the {DUMP_LIMIT_BYTES}-byte limit")
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), a)


def timed_runs(pm, ctx, prm, seed, steps, bufs=None):
    """K x Run() [+ D2H into bufs]; returns (wall seconds, k_update ms sum, k_update launches, all-kernel ms sum)"""
    upd_ms, upd_n, all_ms = 0.0, 0, 0.0
    t0 = time.perf_counter()
    for i in range(steps):
        if bufs is not None:
            ctx.run_into(prm, seed + i, *bufs)   # Run() incl. the D2H copies that end it (mpmvs_run_get)
        else:
            ctx.run(prm, seed + i)
        ms, cnt = ctx.kernel_times()
        upd_ms += ms[pm.KIND_BLACK] + ms[pm.KIND_RED]
        upd_n += cnt[pm.KIND_BLACK] + cnt[pm.KIND_RED]
        all_ms += sum(ms)
    return time.perf_counter() - t0, upd_ms, upd_n, all_ms


def timed_runs_pipelined(pm, ctx, prm, seed, steps, bufsets):
    """K x Run() incl. its D2H through mpmvs_run_get_async: the maps of step i cross PCIe while step i + 1 computes (alternating
    pinned buffer sets); returns when every map of every step is on the host.  Same tuple as timed_runs."""
    t0 = time.perf_counter()
    for i in range(steps):
        ctx.run_into_async(prm, seed + i, *bufsets[i % len(bufsets)])
    ctx.wait()
    dt = time.perf_counter() - t0
    ms, cnt = ctx.kernel_times()      # accumulated over the pipelined steps
    return dt, ms[pm.KIND_BLACK] + ms[pm.KIND_RED], cnt[pm.KIND_BLACK] + cnt[pm.KIND_RED], sum(ms)


def host_cpu_facts():
    """hardware threads this process may use, physical cores among them, and the container's CPU quota (cgroup v2 / v1)"""
    cpus = sorted(os.sched_getaffinity(0))
    cores = set()
    for c in cpus:
        try:
            with open(f"/sys/devices/system/cpu/cpu{c}/topology/thread_siblings_list") as f:
                cores.add(f.read().strip())
        except OSError:
            cores.add(str(c))
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            quota = float(q) / float(per)
    except (OSError, ValueError):
        try:
            q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                quota = q / per
        except (OSError, ValueError):
            pass
    return len(cpus), len(cores), quota


def cpu_baseline_child(out_path, seed, quantize=True):
    """runs in a child process of its own (see cpu_baseline): the oracle on the host cores, nothing else loaded"""
    pm = importlib.import_module("mp-mvs_amd")
    from oracle import binding as ob
    avail, physical, quota = host_cpu_facts()
    counts = sorted({min(16, avail), physical, avail})
    ws, hs = W // 2, H // 2
    cs, ims, _ = load_views(pm, ws, hs, problem_centers(pm, V), f"p{V}")
    ims = [np.rint(im).astype(np.float32) for im in ims]
    dmin, dmax = pm.synth.kernel_depth_range(cs[0])
    prm_s = pm.PatchMatchParams(num_images=V + 1, depth_min=float(dmin), depth_max=float(dmax), max_scale=0, max_iterations=ITERS)
    sample = {}
    for n in counts:
        ob.set_num_threads(n)
        o = ob.create()
        o.set_views(cs, ims)
        t0 = time.perf_counter()
        o.run(prm_s, seed)
        sample[n] = ws * hs / (time.perf_counter() - t0) / 1e6
    best = max(sample, key=sample.get)
    cams, imgs, _ = load_scene(pm, W, H, V, quantize)
    dmin, dmax = pm.synth.kernel_depth_range(cams[0])
    prm = pm.PatchMatchParams(num_images=V + 1, depth_min=float(dmin), depth_max=float(dmax), max_scale=0, max_iterations=ITERS)
    ob.set_num_threads(best)
    o = ob.create()
    o.set_views(cams, imgs)
    t0 = time.perf_counter()
    o.run(prm, seed)
    dt = time.perf_counter() - t0
    op, oc = o.get()
    np.savez(out_path, planes=op, costs=oc)
    print(json.dumps({"best": best, "dt": dt, "sample": {str(k): v for k, v in sample.items()}, "avail": avail, "physical": physical, "quota": quota,
                      "bind": os.environ.get("OMP_PROC_BIND"), "places": os.environ.get("OMP_PLACES")}), flush=True)


def cpu_baseline(pm, ctx, cams, imgs, prm, seed, quantize=True):
    """the oracle (our CPU port; the reference has no CPU path) on the host cores.  Three thread counts -- 16 (the
    share of one GPU on the pool's boxes), the physical cores and all hardware threads, OMP_PROC_BIND=close -- are timed on a
    bounded sample (the same Problem rendered at half the size in each direction: same views, schedule and seed; Mpix/s does
    not depend on the image size); the best of them then runs the WHOLE workload, which gives `value` and, since both results
    are at hand, a bit-for-bit comparison with the HIP path's.  It runs in a child process: the OpenMP binding variables make
    the runtime pin the process's first thread to one core, and every thread created afterwards would inherit that mask."""
    env = dict(os.environ, OMP_PROC_BIND="close", OMP_PLACES="cores")
    with tempfile.TemporaryDirectory() as tmp:
        out_path = os.path.join(tmp, "oracle_result.npz")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-baseline-child", out_path, "--child-seed", str(seed)] +
                           ([] if quantize else ["--float-images"]), env=env,
                           capture_output=True, text=True)
        if r.returncode != 0:
            return {"value": None, "unit": "Mpix/s", "cores": 0, "kind": "port", "sample": "the CPU baseline child failed: " + r.stderr[-400:]}
        info = json.loads(r.stdout.strip().splitlines()[-1])
        z = np.load(out_path)
        op, oc = z["planes"], z["costs"]
    ctx.run(prm, seed)             # untimed
    gp, gc = ctx.get()
    best, dt, sample, quota = info["best"], info["dt"], info["sample"], info["quota"]
    return {"value": round(W * H / dt / 1e6, 5), "unit": "Mpix/s", "cores": best, "kind": "port",
            "sample": f"thread count chosen on a bounded sample (the same Problem at {W // 2}x{H // 2}: {', '.join(f'{n} threads {v:.4f} Mpix/s' for n, v in sample.items())}); "
                      f"`value` = the whole workload (one {W}x{H} Problem, {V} src views, same inputs, seed and Run() schedule) on {best} threads, {dt:.1f} s; "
                      f"OpenMP oracle in a child process, OMP_PROC_BIND={info['bind']} OMP_PLACES={info['places']}; host: {info['avail']} hardware threads / "
                      f"{info['physical']} physical cores usable, container CPU quota {'none' if quota is None else f'{quota:g} CPUs'}",
            "threads_tried_Mpix_per_s": {k: round(v, 5) for k, v in sample.items()},
            "hip_result_bit_identical": bool(np.array_equal(op, gp) and np.array_equal(oc, gc))}


# ---------------------------------------------------------------------------------------------------------------------
# secondary configurations (N = 1 only)
# ---------------------------------------------------------------------------------------------------------------------
def run_schedule(pm, hostlib, ctx, cams, prm0, src_depths, geom_iters, geom_pp, max_scale, seed):
    """one Problem through the pass schedule of reference src/main.cpp:20-41 with fixed source depth maps (SURVEY 8d cfg 2/3);
    the planar prior is built on the device except for the Delaunay triangulation.  Returns wall seconds and a breakdown."""
    t = {"gpu_runs": 0.0, "prior_device": 0.0, "prior_delaunay_host": 0.0, "d2h": 0.0}
    kms, kn = 0.0, 0
    t0 = time.perf_counter()

    def run(p, s):
        nonlocal kms, kn
        a = time.perf_counter()
        ctx.run(p, s)
        t["gpu_runs"] += time.perf_counter() - a
        ms, cnt = ctx.kernel_times()
        kms += ms[pm.KIND_BLACK] + ms[pm.KIND_RED]
        kn += cnt[pm.KIND_BLACK] + cnt[pm.KIND_RED]

    p = pm.PatchMatchParams(num_images=prm0.num_images, depth_min=prm0.depth_min, depth_max=prm0.depth_max, max_scale=max_scale)
    run(p, seed)
    ntri = 0
    for g in range(geom_iters):
        planar = geom_pp and g != geom_iters - 1
        p.geom_consistency, p.planar_prior, p.max_iterations, p.geomPlanarPrior = True, False, 2, planar
        run(p, seed + 1 + g)
        if planar:
            a = time.perf_counter()
            verts = ctx.prior_vertices(True)
            t["prior_device"] += time.perf_counter() - a
            a = time.perf_counter()
            tris = hostlib.delaunay(ctx.W, ctx.H, verts)
            t["prior_delaunay_host"] += time.perf_counter() - a
            a = time.perf_counter()
            ctx.prior_from_triangles(p, tris)
            t["prior_device"] += time.perf_counter() - a
            ntri = len(tris)
            p.geom_consistency, p.planar_prior, p.max_iterations = False, True, 3
            run(p, seed + 1 + g + PRIOR_SEED_OFFSET)
    a = time.perf_counter()
    planes, costs = ctx.get()
    t["d2h"] += time.perf_counter() - a
    return time.perf_counter() - t0, t, kms / max(kn, 1), planes, costs, ntri


def secondary(pm, engine, dev_index, cams, imgs_f32, gts, prm, args):
    hostlib = importlib.import_module("mp-mvs_amd.hostlib")
    out = {}
    gt = gts[0]
    imgs_u8 = [np.rint(im).astype(np.float32) for im in imgs_f32]
    # -- cfg 2 / cfg 3 on the cfg-1 scene: source depth maps = ground truth + 0.5 % noise, held fixed
    rng = np.random.default_rng(7)
    src_depths = [gts[i] * (1.0 + 0.005 * rng.standard_normal((H, W))).astype(np.float32) for i in range(1, V + 1)]
    ctx = engine.create(dev_index)
    ctx.set_views(cams, imgs_u8)
    ctx.set_src_depths(src_depths)
    ctx.set_profiling(True)
    for name, geom_iters, geom_pp, evals in (("cfg2", 1, False, 156), ("cfg3", 2, True, 228)):
        best = None
        for rep in range(2):
            wall, t, upd_ms, planes, costs, ntri = run_schedule(pm, hostlib, ctx, cams, prm, src_depths, geom_iters, geom_pp, 2, 1 + rep)
            if best is None or wall < best[0]:
                best = (wall, t, upd_ms, planes, ntri)
        wall, t, upd_ms, planes, ntri = best
        rel = np.abs(planes[..., 3] - gt) / gt
        out[name] = {"workload": ("configs[2]: photometric 3 scales x 3 iterations, then one geometric Run (2 iterations)" if name == "cfg2" else
                                  "configs[3]: shipped config.yaml: photometric 3 scales -> geometric Run + planar prior + prior Run -> geometric Run"),
                     "wall_s": round(wall, 4), "Mpix_per_s": round(W * H / wall / 1e6, 2), "Mpix_per_s_gpu_runs_only": round(W * H / t["gpu_runs"] / 1e6, 2),
                     "seconds": {k: round(v, 4) for k, v in t.items()}, "k_update_avg_ms_all_modes": round(upd_ms, 4),
                     "hypothesis_evaluations_per_pixel": evals, "within_1pct_of_gt": round(float((rel < 0.01).mean()), 4)}
        if ntri:
            out[name]["prior_triangles"] = int(ntri)
    del ctx
    # configs[3] through the C++ mirror of the reference's interface (PatchMatchCUDA / ProcessProblem, mp-mvs_amd/host): what a
    # user of the reference's API gets, host arrays and per-pass hand-over included
    best = None
    for rep in range(2):
        t0 = time.perf_counter()
        hostlib.run_pipeline(dev_index, cams, imgs_u8, 2, 2, True, True, 5 + rep, src_depths)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    out["cfg3"]["via_process_problem_mirror_s"] = round(best, 4)
    # -- cfg 1 with non-integer images: the fp32 texture format (what every rescaled image takes)
    ctx = engine.create(dev_index)
    ctx.set_views(cams, imgs_f32)
    ctx.set_profiling(True)
    ctx.run(prm, 1)
    dt, upd_ms, upd_n, _ = timed_runs(pm, ctx, prm, 100, 5)
    _, tf = roofline_of(upd_ms / upd_n, W, H, V)
    out["cfg1_fp32_textures"] = {"workload": "configs[1] with non-integer images (fp32 quad-difference texels, 16 B)", "texture_format": ctx.texture_format(),
                                 "resident_Mpix_per_s": round(W * H * 5 / dt / 1e6, 3), "k_update_avg_ms": round(upd_ms / upd_n, 4),
                                 "roofline_frac": round(tf / PEAK_VALU_TFLOPS, 4)}
    del ctx
    # -- cfg 1 on the opt-in build with CUDA's 8-bit texture interpolation fractions (libmpmvs_hip_q8.so)
    try:
        ctx = engine.create_q8(dev_index)
        ctx.set_views(cams, imgs_u8)
        ctx.set_profiling(True)
        ctx.run(prm, 1)
        dt, upd_ms, upd_n, _ = timed_runs(pm, ctx, prm, 100, 5)
        _, tf = roofline_of(upd_ms / upd_n, W, H, V)
        planes, _ = ctx.get()
        rel = np.abs(planes[..., 3] - gt) / gt
        out["cfg1_8bit_texture_fractions"] = {"workload": "configs[1] on libmpmvs_hip_q8.so: bilinear fractions quantised to 8 bits like the reference's texture hardware (opt-in)",
                                              "resident_Mpix_per_s": round(W * H * 5 / dt / 1e6, 3), "k_update_avg_ms": round(upd_ms / upd_n, 4),
                                              "roofline_frac": round(tf / PEAK_VALU_TFLOPS, 4), "within_1pct_of_gt": round(float((rel < 0.01).mean()), 4)}
        del ctx
    except RuntimeError as e:
        out["cfg1_8bit_texture_fractions"] = {"error": str(e)}
    # -- cfg 1 with 20 source views (the shipped `Max source images num`, config/config.yaml:19) at 800x600
    w2, h2, v2 = 800, 600, 20
    cams20, imgs20, gts20 = load_views(pm, w2, h2, problem_centers(pm, v2), f"p{v2}")
    imgs20 = [np.rint(im).astype(np.float32) for im in imgs20]
    dmin, dmax = pm.synth.kernel_depth_range(cams20[0])
    prm20 = pm.PatchMatchParams(num_images=v2 + 1, depth_min=float(dmin), depth_max=float(dmax), max_scale=0, max_iterations=ITERS)
    ctx = engine.create(dev_index)
    ctx.set_views(cams20, imgs20)
    ctx.set_profiling(True)
    ctx.run(prm20, 1)
    dt, upd_ms, upd_n, _ = timed_runs(pm, ctx, prm20, 100, 5)
    _, tf = roofline_of(upd_ms / upd_n, w2, h2, v2)
    planes, _ = ctx.get()
    rel = np.abs(planes[..., 3] - gts20[0]) / gts20[0]
    out["cfg1_20_views"] = {"workload": f"configs[1] schedule with {v2} source views, {w2}x{h2}", "resident_Mpix_per_s": round(w2 * h2 * 5 / dt / 1e6, 3),
                            "k_update_avg_ms": round(upd_ms / upd_n, 4), "roofline_frac": round(tf / PEAK_VALU_TFLOPS, 4),
                            "ns_per_nominal_evaluation": round(upd_ms / upd_n * 1e6 / ((w2 * h2 / 2) * HYP_PER_UPDATE * v2), 5),
                            "within_1pct_of_gt": round(float((rel < 0.01).mean()), 4)}
    return out


# ---------------------------------------------------------------------------------------------------------------------
# cfg 4
# ---------------------------------------------------------------------------------------------------------------------
def run_cfg4(args, pm, engine, dist, rank, world, dev_index, barrier, steps=None, warmup=None, dump=None):
    """configs[4]; every rank calls it, rank 0 gets the result line (a dict), the others None.  dump: directory for the maps rank 0
    holds after the last step, a fixed, seeded sample of pixels (the same in every map)"""
    import torch
    steps = args.steps if steps is None else steps
    warmup = args.warmup if warmup is None else warmup
    sched = importlib.import_module("mp-mvs_amd.schedule")
    w4, h4 = (int(v) for v in args.cfg4_size.lower().split("x"))
    g = args.cfg4_grid
    centers = [((i - (g - 1) / 2.0) * 0.15, (j - (g - 1) / 2.0) * 0.15, 0.0) for j in range(g) for i in range(g)]
    cams, imgs, gts = load_views(pm, w4, h4, centers, f"grid{g}", rank, world, barrier)
    imgs = [np.rint(im).astype(np.float32) for im in imgs]
    neigh = []
    for j in range(g):
        for i in range(g):
            cand = sorted(((ii - i) ** 2 + (jj - j) ** 2, jj * g + ii) for jj in range(g) for ii in range(g) if (ii, jj) != (i, j))
            neigh.append([c[1] for c in cand[:8]])
    device_tensors = args.backend == "nccl" or world == 1
    s = sched.SceneScheduler(cams, imgs, neigh, lambda: engine.create(dev_index), rank=rank, world=world, dist=dist, device_tensors=device_tensors,
                             max_scale=2, workers=args.workers)
    s.fetch_results = not device_tensors
    s.timing = []
    barrier()
    for i in range(warmup):
        s.run(seed=999 + i)
    barrier()
    t0 = time.perf_counter()
    for i in range(steps):
        s.run(seed=12345 + i)
    barrier()
    dt = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([dt], device="cuda" if args.backend == "nccl" else "cpu", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    res = s.fetch()
    acc = [float((np.abs(r[0][..., 3] - gts[i]) / gts[i] < 0.01).mean()) for i, r in res.items()]
    if dump is not None and rank == 0:
        ids = sorted(res)
        k = min(w4 * h4, DUMP_LIMIT_BYTES // (6 * 4 * len(ids)))   # 6 floats per pixel: plane (4), cost, geometric cost
        pix = np.sort(np.random.default_rng(0).choice(w4 * h4, k, replace=False))
        dump_outputs(dump, {"planes": np.stack([res[i][0].reshape(-1, 4)[pix] for i in ids]),
                            "costs": np.stack([res[i][1].reshape(-1)[pix] for i in ids]),
                            "geom_costs": np.stack([res[i][2].reshape(-1)[pix] for i in ids])})
    if rank == 0:
        n = g * g
        passes = s.timing[-3:]
        out = {"metric": f"Mpix/s depth+normal (shipped schedule, {w4}x{h4}, 8 src views, {n} Problems sharded over the GPUs)",
               "value": round(n * w4 * h4 * steps / dt / 1e6, 3), "unit": "Mpix/s", "n_gpus": world, "steps": steps, "warmup": warmup,
               "ms_per_step": round(dt / steps * 1e3, 2), "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32",
               "data": "synthetic, seeded height-field scene, images rounded to 8 bits",
               "config": {"workload": f"configs[4]: {n} reference-image Problems ({g}x{g} camera grid, 8 nearest neighbours as sources) sharded round-robin "
                                      f"over {world} rank(s); photometric 3 scales -> geometric + planar prior -> geometric; Jacobi barrier = one "
                                      f"all-gather of the depth maps per pass ({'RCCL all_gather_into_tensor on device buffers' if device_tensors and world > 1 else 'device buffers, single rank' if device_tensors else 'gloo, host staging (rehearsal)'})",
                          "width": w4, "height": h4, "problems": n, "src_views": 8, "host_threads_per_rank": args.workers},
               "passes_last_step": passes, "within_1pct_of_gt_rank0_mean": round(float(np.mean(acc)), 4)}
        return out
    return None


# ---------------------------------------------------------------------------------------------------------------------
# self-launch: `python bench.py --gpus N` without torch.distributed.run
# ---------------------------------------------------------------------------------------------------------------------
def _free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_ranks(n, argv):
    """Parent of a self-launched multi-rank run.  Must not have touched the GPU (it has imported neither torch nor the HIP
    library): starts n fresh children of this script, one per rank, waits for them, forwards rank 0's stdout (the JSON line)
    and returns the exit code -- non-zero if any rank failed, in which case the others are terminated (by PID)."""
    port = os.environ.get("MASTER_PORT") or str(_free_port())
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: RCCL between processes needs it on this driver
        env.setdefault("OMP_NUM_THREADS", str(max(1, len(os.sched_getaffinity(0)) // n)))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env,
                                      stdout=subprocess.PIPE if r == 0 else sys.stderr, text=(r == 0) or None))
    import threading
    lines = []

    def pump():
        for line in procs[0].stdout:
            lines.append(line)
            # stdout carries the JSON line only; whatever else rank 0 or its libraries print there (gloo announces its connections
            # on stdout) goes to stderr
            out = sys.stdout if line.lstrip().startswith("{") else sys.stderr
            out.write(line)
            out.flush()

    th = threading.Thread(target=pump, daemon=True)
    th.start()
    rc = 0
    pending = set(range(n))
    while pending:
        for r in sorted(pending):
            code = procs[r].poll()
            if code is None:
                continue
            pending.discard(r)
            if code != 0 and rc == 0:
                rc = code if code > 0 else 1
                print(f"bench.py launcher: rank {r} exited with code {code}; stopping the other ranks", file=sys.stderr, flush=True)
                for q in pending:
                    procs[q].terminate()
        if pending:
            time.sleep(0.05)
    th.join(timeout=10)
    if rc == 0 and not any(l.lstrip().startswith("{") for l in lines):
        print("bench.py launcher: rank 0 printed no JSON line", file=sys.stderr, flush=True)
        rc = 1
    return rc


def launch_check(args):
    """--launch-check: the rank-side plumbing of a self-launched run without any GPU work (CPU test of the launcher): gloo
    rendezvous from the environment the launcher set, a max-reduce over the ranks, one JSON line from rank 0."""
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo")
    if args.launch_check_fail_rank == rank:
        time.sleep(0.5)
        raise SystemExit(3)
    t = torch.tensor([float(rank + 1)], dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dist.barrier()
    if rank == 0:
        print(json.dumps({"launch_check": True, "n_gpus": world, "max_rank_plus_1": float(t.item()), "local_rank": int(os.environ["LOCAL_RANK"]),
                          "master": os.environ["MASTER_ADDR"] + ":" + os.environ["MASTER_PORT"]}), flush=True)
    dist.destroy_process_group()


# ---------------------------------------------------------------------------------------------------------------------
# multi-GPU diagnostics: nothing here is timed
# ---------------------------------------------------------------------------------------------------------------------
class stage:
    """`with stage(rank, "call"):` -- a failure inside names the rank and the call on stderr and ends the rank with a non-zero code
    (the launcher then stops the others) instead of leaving a bare traceback, or a hang of the ranks that wait for this one"""

    def __init__(self, rank, what):
        self.rank, self.what = rank, what

    def __enter__(self):
        return self

    def __exit__(self, et, ev, tb):
        if et is None or et in (SystemExit, KeyboardInterrupt):
            return False
        import traceback
        print(f"bench.py: rank {self.rank}: {self.what} FAILED: {et.__name__}: {ev}", file=sys.stderr, flush=True)
        traceback.print_tb(tb, file=sys.stderr)
        sys.stderr.flush()
        os._exit(2)


class native_stdout_to_stderr:
    """inside the block file descriptor 1 is file descriptor 2: what native libraries print on stdout while a communicator comes up
    (gloo's connection banner, RCCL's library path) lands on stderr, and rank 0's stdout stays the one JSON line"""

    def __enter__(self):
        sys.stdout.flush()
        self.saved = os.dup(1)
        os.dup2(2, 1)
        return self

    def __exit__(self, *exc):
        sys.stdout.flush()
        os.dup2(self.saved, 1)
        os.close(self.saved)
        return False


PEER_CHECK_TIMEOUT_S = 60
_LINK = {4: "xGMI", 2: "PCIe", 0: "HyperTransport", 1: "QPI", 3: "InfiniBand", -1: "unknown"}


def peer_table(engine, dev_index):
    """how this rank's device reaches every other visible device: {peer: {"access": 0/1, "link": "xGMI", "hops": 1}}"""
    out = {}
    for peer in range(engine.device_count()):
        if peer == dev_index:
            continue
        can, link, hops = engine.peer_info(dev_index, peer)
        out[str(peer)] = {"access": can, "link": _LINK.get(link, str(link)), "hops": hops}
    return out


def peer_copy_check(pm, engine, ctx, cams, gts, prm, dev_index, allow_self=False):
    """ONE untimed execution of the GPU-to-GPU branch of mpmvs_set_src_depths_mixed (mpmvs_api.hip: hipMemcpyPeerAsync) per neighbour
    device, verified: the V source depth maps are placed on the neighbour, copied into this rank's context from there, and the
    geometric-cost probe (mpmvs_eval_geom) must then equal the one after a plain host upload of the same maps, bit for bit.  Returns
    {"peer": p, "ok": bool, ...}; on a one-device view there is no neighbour ("peer": None)."""
    import torch
    n_dev = engine.device_count()
    if n_dev < 2 and not allow_self:
        return {"peer": None, "ok": None, "note": "one visible device: the GPU-to-GPU branch has no neighbour to copy from"}
    _, fns = engine.load()
    peer = (dev_index + 1) % n_dev   # (allow_self on a one-GPU box: the device itself -- rehearses this check, not the peer copy)
    Vn = len(cams) - 1
    h, w = gts[0].shape
    maps = [np.ascontiguousarray(gts[i], np.float32) for i in range(1, Vn + 1)]
    planes = np.zeros((h, w, 4), np.float32)
    planes[..., 2] = -1.0
    planes[..., 3] = gts[0]
    ctx.set_src_depths(maps)
    want = ctx.eval_geom(prm, planes)
    ctx.set_src_depths([np.zeros_like(m) for m in maps])         # so that a copy that silently did nothing would show
    remote = [torch.from_numpy(m).to(f"cuda:{peer}") for m in maps]
    torch.cuda.synchronize(peer)
    torch.cuda.set_device(dev_index)
    FP = ctypes.POINTER(ctypes.c_float)
    t0 = time.perf_counter()
    rc = fns["set_src_depths_mixed"](ctx._ctx, Vn, (FP * Vn)(*[None] * Vn), (ctypes.c_void_p * Vn)(*[t.data_ptr() for t in remote]),
                                     (ctypes.c_int * Vn)(*[peer] * Vn), (ctypes.c_int * Vn)(*[w] * Vn), (ctypes.c_int * Vn)(*[h] * Vn))
    dt = time.perf_counter() - t0
    if rc != 0:
        return {"peer": peer, "ok": False, "note": f"mpmvs_set_src_depths_mixed returned {rc}: {fns['last_error'](ctx._ctx).decode()}"}
    got = ctx.eval_geom(prm, planes)
    del remote
    ok = bool(np.array_equal(got, want))
    return {"peer": peer, "ok": ok, "GBps": round(Vn * h * w * 4 / dt / 1e9, 1), "bytes": Vn * h * w * 4,
            "note": "geometric-cost probe after the GPU-to-GPU copies == after a host upload of the same maps" if ok else "the probe DIFFERS after the GPU-to-GPU copies"}


def other_readings(pm, engine, ctx, dev_index, cams, imgs, prm, seed, args, bufs, barrier, dist):
    """--full: the other readings of the metric after the timed region; every time is the max over the ranks.  Returns the
    seconds of the pipelined, kernel-only, with-upload and two-context steps and the host time per step of the last"""
    import torch
    bufs2 = (pinned((H, W, 4)), pinned((H, W)))
    # untimed by the driver: pipelined steps, kernels only, and with the image upload
    ctx.run_into_async(prm, seed + 999, *bufs2)
    ctx.wait()
    barrier()
    t0 = time.perf_counter()
    timed_runs_pipelined(pm, ctx, prm, seed, args.steps, (bufs, bufs2))   # the maps of step i travel while step i + 1 computes
    dt_pipelined = time.perf_counter() - t0
    dt_res, _, _, _ = timed_runs(pm, ctx, prm, seed, args.steps)
    # SURVEY 8(d)'s wording of the metric ("uploads/downloads included"): image upload + Run() + D2H per step, on the same
    # number of steps and between the same barriers as `value`
    barrier()
    t0 = time.perf_counter()
    for i in range(args.steps):
        ctx.set_views(cams, imgs)
        ctx.run_into(prm, seed + i, *bufs)
    barrier()
    dt_h2d = time.perf_counter() - t0
    # ... and the same as a pipeline over TWO contexts, the way a job with many Problems runs ("several Problems resident
    # per GPU"): Problem i + 1 is converted, uploaded and packed on its own context and stream while Problem i computes, and the
    # maps of Problem i travel back while Problem i + 1 computes.  Every upload and every map is complete inside the timed region.
    dt_h2d_pipe = float("nan")
    pipe_host_ms = None
    if not args.no_overlap_phase:
        ctx_b = engine.create(dev_index)
        ctx_b.set_views(cams, imgs)      # untimed: allocations of the second context ...
        ctx_b.run_into_async(prm, seed + 998, *bufs2)   # ... including the staging buffers and the copy stream of its pipelined Run()
        ctx_b.wait()
        pair = ((ctx, bufs), (ctx_b, bufs2))
        barrier()
        t_wait = t_set = t_run = t_wait_max = 0.0
        t0 = time.perf_counter()
        for i in range(args.steps):
            c_i, b_i = pair[i % 2]
            t1 = time.perf_counter()
            c_i.wait()                   # its previous Run() has delivered: textures and host buffers are free again
            t2 = time.perf_counter()
            c_i.set_views(cams, imgs)    # host conversion to 8 bit; the transfer and the texture packing are only enqueued
            t3 = time.perf_counter()
            c_i.run_into_async(prm, seed + i, *b_i)
            t4 = time.perf_counter()
            t_wait, t_set, t_run, t_wait_max = t_wait + (t2 - t1), t_set + (t3 - t2), t_run + (t4 - t3), max(t_wait_max, t2 - t1)
        ctx.wait()
        ctx_b.wait()
        barrier()
        dt_h2d_pipe = time.perf_counter() - t0
        # where the host thread that drives both contexts spent the step (it should sit in wait(): the GPU is the bottleneck then)
        pipe_host_ms = {"wait": round(t_wait / args.steps * 1e3, 3), "wait_max": round(t_wait_max * 1e3, 3), "set_views": round(t_set / args.steps * 1e3, 3),
                        "run_async": round(t_run / args.steps * 1e3, 3), "step": round(dt_h2d_pipe / args.steps * 1e3, 3)}
        del ctx_b
    if dist is not None:
        t = torch.tensor([dt_res, dt_h2d, dt_pipelined, dt_h2d_pipe], device="cuda" if args.backend == "nccl" else "cpu", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt_res, dt_h2d, dt_pipelined, dt_h2d_pipe = (float(v) for v in t.tolist())
    return dt_pipelined, dt_res, dt_h2d, dt_h2d_pipe, pipe_host_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--workload", default="cfg1", choices=["cfg1", "cfg4"])
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure everything beyond the headline: pipelined / resident / with-upload readings, the "
                         "secondary configurations, the CPU baseline, and with --gpus N > 1 the peer tables, the peer-copy check and configs[4]")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the last timed step returned to DIR/<name>.npy (float32; cfg4: a fixed, seeded sample of pixels)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-secondary", action="store_true", help="with --full: skip the secondary configurations (cfg 2, cfg 3, fp32 textures, 20 views)")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="torch.distributed backend for --gpus > 1 (nccl = RCCL; gloo only to rehearse the multi-rank path on one GPU)")
    ap.add_argument("--share-device", action="store_true", help="rehearsal: every rank uses GPU 0")
    ap.add_argument("--float-images", action="store_true",
                    help="keep the rendered images as non-integer fp32 (rescaled-image case) instead of 8-bit camera-like images")
    ap.add_argument("--cfg4-size", default="1600x1200")
    ap.add_argument("--cfg4-grid", type=int, default=8)
    ap.add_argument("--workers", type=int, default=6, help="cfg4: host threads per rank driving its Problems (measured on one MI355X, 64 Problems: 1 / 3 / 6 / 10 threads 14.6 / 10.7 / 9.4 / 9.7 s)")
    ap.add_argument("--size", default=None, help="WxH of the cfg-1 Problem instead of 1600x1200 (tests of the multi-rank plumbing; the line says so)")
    ap.add_argument("--cpu-baseline-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-seed", type=int, default=12345, help=argparse.SUPPRESS)
    ap.add_argument("--no-overlap-phase", action="store_true",
                    help="with --full: skip the untimed two-context pipeline (value_survey_8d_pipelined): its kernels overlap, which inflates the per-kernel "
                         "durations of a kernel trace of this command (tools/profile_gpu.sh, tools/trace_kernels.sh use it)")
    ap.add_argument("--peer-check-self", action="store_true", help=argparse.SUPPRESS)   # rehearsal of the peer-copy check on a one-GPU box (the device copies from itself)
    ap.add_argument("--launch-check", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--launch-check-fail-rank", type=int, default=-1, help=argparse.SUPPRESS)
    args = ap.parse_args()
    global W, H
    if args.size:
        W, H = (int(v) for v in args.size.lower().split("x"))
    if args.cpu_baseline_child:
        cpu_baseline_child(args.cpu_baseline_child, args.child_seed, not args.float_images)
        return
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # started plainly: become the launcher (nothing below this line runs in this process, which never touches the GPU)
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))
    if args.launch_check:
        launch_check(args)
        return
    if args.steps is None:
        args.steps = 5 if args.workload == "cfg1" else 1
    if args.warmup is None:
        args.warmup = 1 if (args.workload == "cfg1" or args.gpus > 1) else 0   # cfg4 with ranks: the first collective sets up the communicator
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    import torch
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: start it plainly (python bench.py --gpus N launches its own ranks) or with "
                         f"torch.distributed.run --nproc-per-node {args.gpus}")
    dist = None
    dev_index = 0 if args.share_device else local_rank
    torch.cuda.set_device(dev_index)
    if world > 1:
        import torch.distributed as dist
        with stage(rank, f"torch.distributed.init_process_group({args.backend!r}) on cuda:{dev_index}"), native_stdout_to_stderr():
            if args.backend == "nccl":
                dist.init_process_group("nccl", device_id=torch.device("cuda", dev_index))
            else:
                dist.init_process_group("gloo")
            dist.barrier()   # the communicator comes up here, whatever the workload does first (and says what it has to say on stderr)
    # a CPU-only side channel (gloo) for the diagnostics that must get through even if a GPU call of some rank never returns
    side = None
    if dist is not None and args.full:
        try:
            if args.backend == "nccl" and "GLOO_SOCKET_IFNAME" not in os.environ:
                import socket
                try:
                    socket.gethostbyname(socket.gethostname())
                except OSError:   # a container whose hostname does not resolve: gloo would not find its own address; one node, so loopback does
                    os.environ["GLOO_SOCKET_IFNAME"] = "lo"
            if args.backend == "nccl":
                with native_stdout_to_stderr():
                    side = dist.new_group(backend="gloo")
            else:
                side = dist.group.WORLD
        except Exception as e:   # noqa: BLE001 -- no side channel: the peer-copy check is skipped (it would have no safe way to report)
            print(f"bench.py: rank {rank}: no gloo side channel ({type(e).__name__}: {e}); the peer-copy check will be skipped", file=sys.stderr, flush=True)

    pm = importlib.import_module("mp-mvs_amd")
    engine = importlib.import_module("mp-mvs_amd.engine")

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    if args.workload == "cfg4":
        with stage(rank, "configs[4] (SceneScheduler.run: one all_gather_into_tensor of the depth maps per pass)"):
            out = run_cfg4(args, pm, engine, dist, rank, world, dev_index, barrier, dump=args.dump_outputs)
        if rank == 0:
            print(json.dumps(out), flush=True)
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return

    quantize = not args.float_images
    if rank == 0:
        cams, imgs_f32, gts = load_views(pm, W, H, problem_centers(pm, V), f"p{V}")   # renders once, the other ranks read the cache
    if dist is not None:
        dist.barrier()
    if rank != 0:
        cams, imgs_f32, gts = load_views(pm, W, H, problem_centers(pm, V), f"p{V}")
    imgs = [np.rint(im).astype(np.float32) for im in imgs_f32] if quantize else imgs_f32
    gt = gts[0]
    dmin, dmax = pm.synth.kernel_depth_range(cams[0])
    prm = pm.PatchMatchParams(num_images=V + 1, depth_min=float(dmin), depth_max=float(dmax), max_scale=0, max_iterations=ITERS)
    ctx = engine.create(dev_index)
    ctx.set_views(cams, imgs)   # inputs resident in HBM from here on
    ctx.set_profiling(True)
    seed = 12345 + rank
    bufs = (pinned((H, W, 4)), pinned((H, W)))

    devices = None
    peers = None
    if dist is not None:
        # every rank sees the whole job, on a device of its own (unless --share-device rehearses on one GPU)
        with stage(rank, "first collective (all_gather of rank / device ids: sets the communicator up)"), native_stdout_to_stderr():
            assert dist.get_world_size() == args.gpus, f"rank {rank}: the process group has {dist.get_world_size()} ranks, --gpus {args.gpus}"
            mine = torch.tensor([rank, torch.cuda.current_device()], dtype=torch.int64, device="cuda" if args.backend == "nccl" else "cpu")
            seen = [torch.empty_like(mine) for _ in range(world)]
            dist.all_gather(seen, mine)
            devices = {int(t[0]): int(t[1]) for t in seen}
            assert sorted(devices) == list(range(world)), f"ranks seen by the collective: {sorted(devices)}"
            if not args.share_device:
                assert len(set(devices.values())) == world, f"ranks share devices: {devices}"
    if dist is not None and args.full:
        # how this rank's GPU reaches the others (hipDeviceCanAccessPeer, link type, hops): printed per rank before anything is
        # measured, and gathered into the line
        with stage(rank, "mpmvs_peer_info"):
            mine_peers = peer_table(engine, dev_index)
            print(f"bench.py: rank {rank} on cuda:{dev_index} of {engine.device_count()} visible: peers {json.dumps(mine_peers)}", file=sys.stderr, flush=True)
            gathered = [None] * world
            dist.all_gather_object(gathered, {"rank": rank, "device": dev_index, "peers": mine_peers})
            peers = gathered

    # THE timed region (driver contract): W untimed steps, then exactly K steps between barriers.  A step is ONE blocking call,
    # mpmvs_run_get: the launches of Run() and the device-to-host copies that end it (ref .cu:1246-1251) -- the headline of
    # rounds 2 and 3.  (Round 4 pipelined the steps here; that figure is `pipelined_value`, measured after the timed region with --full.)
    with stage(rank, "the timed region (warm-up, barrier, K x mpmvs_run_get, barrier, max over the ranks)"):
        for i in range(args.warmup):
            ctx.run_into(prm, seed + 1000 * (i + 1), *bufs)
        barrier()
        t0 = time.perf_counter()
        _, upd_ms, upd_n, all_ms = timed_runs(pm, ctx, prm, seed, args.steps, bufs)
        barrier()
        dt = time.perf_counter() - t0
        if dist is not None:
            t = torch.tensor([dt], device="cuda" if args.backend == "nccl" else "cpu", dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())

    # sanity of the last result
    planes, costs = bufs[0].copy(), bufs[1].copy()
    rel = np.abs(planes[..., 3] - gt) / gt
    within = float((rel < 0.01).mean())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"planes": planes, "costs": costs})

    readings = other_readings(pm, engine, ctx, dev_index, cams, imgs, prm, seed, args, bufs, barrier, dist) if args.full else None

    # configs[4] in the same invocation when there is more than one rank: the only workload whose passes exchange depth maps
    # (one all-gather per pass), so that one driver command yields the weak-scaling line AND an execution of the collective.
    # One untimed warm-up step first: the communicator is set up by the first collective, and `passes_last_step` should show a
    # steady-state exchange, not that.
    cfg4_line = None
    if world > 1 and args.full and not args.no_secondary:
        del ctx
        with stage(rank, "configs[4] (SceneScheduler.run: one all_gather_into_tensor of the depth maps per pass)"):
            cfg4_line = run_cfg4(args, pm, engine, dist, rank, world, dev_index, barrier, steps=1, warmup=1)
        ctx = engine.create(dev_index)
        ctx.set_views(cams, imgs)
    # The GPU-to-GPU branch of the depth-map hand-over (mpmvs_set_src_depths_mixed: hipMemcpyPeerAsync), which the C++ pass schedule
    # takes when its Problems live on several devices of one process, executed ONCE per rank towards its neighbour device and
    # verified -- untimed, after every measurement of this run (the measured paths exchange through RCCL, not through this branch),
    # so that its first execution anywhere is neither inside a measurement nor unobserved.  A failure is reported (stderr and the
    # line) but does not void the measurements above.
    # It runs on a thread of its own under a watchdog, and its outcome travels over the CPU-only side channel: should the copy never
    # return on some node (it has not run between two GPUs anywhere yet), the line is still printed -- with "timed out" for that rank --
    # and every rank then leaves without the final GPU barrier.
    peer_checks, peer_check_hung = None, False
    if dist is not None and side is not None and (not args.share_device or args.peer_check_self):
        import threading
        barrier()   # every measurement of every rank is complete
        box = {}

        def run_check():
            try:
                box.update(peer_copy_check(pm, engine, ctx, cams, gts, prm, dev_index, allow_self=args.peer_check_self))
            except Exception as e:   # noqa: BLE001 -- reported, not fatal
                box.update({"ok": False, "note": f"{type(e).__name__}: {e}"})

        th = threading.Thread(target=run_check, daemon=True)
        th.start()
        th.join(PEER_CHECK_TIMEOUT_S)
        if th.is_alive():
            mine_check = {"rank": rank, "device": dev_index, "ok": False, "timed_out": True,
                          "note": f"the GPU-to-GPU copy did not return within {PEER_CHECK_TIMEOUT_S} s (abandoned; the measurements above were complete before it started)"}
        else:
            mine_check = dict(box, rank=rank, device=dev_index)
        if mine_check.get("ok") is False:
            print(f"bench.py: rank {rank}: peer-copy check towards device {mine_check.get('peer')} FAILED: {mine_check.get('note')}", file=sys.stderr, flush=True)
        gathered = [None] * world
        dist.all_gather_object(gathered, mine_check, group=side)
        peer_checks = gathered
        peer_check_hung = any(c.get("timed_out") for c in gathered)

    if rank == 0:
        mpix = world * W * H * args.steps / dt / 1e6
        upd_avg_ms = upd_ms / max(upd_n, 1)
        flops_per_launch, tflops = roofline_of(upd_avg_ms, W, H, V)
        hbm_bytes_per_launch = W * H * (4 * (V + 1) + 36)      # SURVEY.md 8d COMPULSORY_HBM_BYTES / L
        gbps = hbm_bytes_per_launch / (upd_avg_ms * 1e-3) / 1e9
        prof = profile_counters(upd_avg_ms)
        if readings is not None:
            dt_pipelined, dt_res, dt_h2d, dt_h2d_pipe, pipe_host_ms = readings
        out = {
            "metric": f"Mpix/s depth+normal (fixed iters, {W}x{H}, 8 src views)",
            "value": round(mpix, 3),
            "unit": "Mpix/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(dt / args.steps * 1e3, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic, seeded height-field scene; images " + ("rounded to 8 bits like the reference's imread input" if quantize else "non-integer fp32") + f"; resident texture format {ctx.texture_format()}",
            "config": {"workload": ("" if (W, H) == (1600, 1200) else "NOT the BASELINE size (--size): ") + f"configs[1]: 1 ref + 8 src views, {W}x{H}, single-scale, photometric only, 3 red/black iterations, one Problem per GPU per step; "
                                   "a step = ONE blocking Run() incl. its device-to-host copies of planes + costs (mpmvs_run_get, as the reference's Run() ends, "
                                   "ref .cu:1246-1251; every map of every step is in host memory when its call returns); "
                                   "the 9 images are resident in HBM when the timed region "
                                   "starts (bench contract), i.e. the image upload (H2D) is EXCLUDED from `value` -- SURVEY 8(d)'s wording of the metric, "
                                   "upload + Run() + D2H per step, is `value_survey_8d` in the line of a --full run",
                       "width": W, "height": H, "src_views": V, "max_scale": 0, "iterations": ITERS},
            "blocking_value": round(mpix, 3),
            **({} if readings is None else {
            "comparable_across_rounds": "`value` is Run() + D2H one blocking step at a time: the headline of rounds 2, 3 and 5 and round 4's `blocking_value`; round 4's `value` "
                                        "(steps pipelined through mpmvs_run_get_async) is `pipelined_value` here; `resident_value` (kernels only) was round 1's headline",
            "pipelined_value": round(world * W * H * args.steps / dt_pipelined / 1e6, 3),
            "pipelined_value_is": "the same steps through mpmvs_run_get_async on one context: the maps of step i cross PCIe while step i + 1 computes (every map of every step is in "
                                  "host memory when the region ends); a re-run of one resident Problem, which a real job -- set_views per Problem -- never does: reported, not the headline",
            "resident_value": round(world * W * H * args.steps / dt_res / 1e6, 3),
            "value_survey_8d": round(world * W * H * args.steps / dt_h2d / 1e6, 3),
            "value_survey_8d_is": "SURVEY 8(d)'s wording of the metric: image upload (host 8-bit conversion, H2D, texture packing) + Run() + D2H per step, "
                                  f"{args.steps} steps one after the other on one context, between the same barriers as `value`; `value` itself keeps the inputs resident (bench contract)",
            "value_survey_8d_pipelined": None if args.no_overlap_phase else round(world * W * H * args.steps / dt_h2d_pipe / 1e6, 3),
            "value_survey_8d_pipelined_is": "the same work -- every step uploads its 9 images, runs and returns its maps inside the timed region -- as a pipeline over two contexts "
                                            "(Problem i + 1 is uploaded and Problem i - 1 downloaded while Problem i computes): what a job with many Problems gets",
            "value_survey_8d_pipelined_host_ms_per_step": pipe_host_ms,
            }),
            "roofline": {
                "kernel": "k_update<photometric> (BlackPixelUpdate/RedPixelUpdate)",
                "bound": "valu_fp32",
                "frac_is": "algorithmic-equivalent rate (SURVEY 8d's nominal flop / measured time / peak), NOT executed-VALU utilisation: see `note` and "
                           "`valu_busy_from_profile`",
                "valu_busy_from_profile": prof["valu_busy"],
                "achieved": round(tflops, 3),
                "peak": PEAK_VALU_TFLOPS,
                "unit": "TFLOP/s",
                "frac": round(tflops / PEAK_VALU_TFLOPS, 4),
                "note": "achieved = SURVEY 8d's ALGORITHMIC flop per launch (14 hypotheses x 8 views x 2144 flop per pixel of one colour) / measured launch time; the "
                        "kernel executes roughly half of that (bilateral weights and reference moments once per pixel, homography as 9 fmas, one reciprocal per six taps, "
                        "zero-weight views skipped): it is an algorithmic-equivalent rate, not the VALU utilisation (that is in profiles/: SQ_ACTIVE_INST_VALU)",
                "traffic": prof["traffic"],
                "traffic_if_fetch_doubled": prof["traffic_if_fetch_doubled"],
                "traffic_source": prof["source"],
                "traffic_null_reason": prof["reason"],
                "avg_launch_ms": round(upd_avg_ms, 4),
                "launches_timed": upd_n,
                "k_update_passes_per_dispatch": (2 * ITERS if ctx.chain_status() == 1 else 1),
                "launch_is": "one PASS (BlackPixelUpdate or RedPixelUpdate over the image) -- what the reference launches as one kernel (ref .cu:1211-1236) and rounds 1-4 did too; since round 5 one "
                             "k_update dispatch chains the passes of a window scale (6 here), its blocks waiting for their neighbours of the pass before: avg_launch_ms = HIP-event time of "
                             "the dispatch / its passes, and every per-launch figure of this object (flop, bytes, traffic) is per pass",
                "algorithmic_flop_per_launch": flops_per_launch,
                "hbm": {"achieved": round(gbps, 2), "peak": PEAK_HBM_GBPS, "unit": "GB/s", "frac": round(gbps / PEAK_HBM_GBPS, 5),
                        "algorithmic_bytes_per_launch": hbm_bytes_per_launch},
                # SURVEY 8(d)'s third figure, a diagnostic at L1 / LDS level (reuse makes it exceed the HBM peak): 36 taps x 20 logical
                # bytes (1 reference + 4 source texels, fp32) per nominal (hypothesis, view) evaluation
                "tap_gather": {"achieved": round((W * H // 2) * 14 * V * 36 * 20 / (upd_avg_ms * 1e-3) / 1e12, 2), "unit": "TB/s (logical)"},
            },
            "kernel_ms_per_step": round(all_ms / args.steps, 3),
            "within_1pct_of_gt": round(within, 4),
        }
        if devices is not None:
            out["ranks"] = {"world_size_seen_by_the_collective": len(devices), "backend": args.backend,
                            "cuda_device_of_rank": {str(r): d for r, d in sorted(devices.items())},
                            "peer_access": peers, "peer_copy_check": peer_checks}
        if world == 1 and args.full and not args.no_secondary:
            del ctx
            out["secondary"] = secondary(pm, engine, dev_index, cams, imgs_f32, gts, prm, args)
            ctx = engine.create(dev_index)
            ctx.set_views(cams, imgs)
        if cfg4_line is not None:
            out.setdefault("secondary", {})["cfg4"] = cfg4_line
        if world == 1 and args.full and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(pm, ctx, cams, imgs, prm, seed, quantize)
        print(json.dumps(out), flush=True)
    if dist is not None:
        if peer_check_hung:   # some rank holds a GPU call that never returned: no further GPU collective, no teardown that could wait for it
            sys.stdout.flush()
            sys.stderr.flush()
            os._exit(0)
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
