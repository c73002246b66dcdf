"""GPU parity of the layers above Run(): the C++ ProcessProblem pass schedule
(reference src/main.cpp:20-41 + src/PatchMatch.cpp:506-638) with the host-built
planar prior, and the multi-Problem scheduler with device-resident depth-map
exchange -- each against the same schedule driven on the CPU oracle."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PRIOR_SEED_OFFSET = 0x9E3779B97F4A7C15


def oracle_pipeline(pm, oracle, hostlib, cams, imgs, src_depths, max_scale, geom_iterations, planar_prior, geom_pp, seed):
    """the schedule of mpmvs_host_run_pipeline on the oracle"""
    h = oracle.create()
    h.set_views(cams, imgs)
    dmin, dmax = pm.synth.kernel_depth_range(cams[0])
    state = {}

    def process(geom, planar, sd):
        p = pm.PatchMatchParams(num_images=len(cams), depth_min=float(dmin), depth_max=float(dmax), max_scale=max_scale)
        p.geom_consistency = geom
        p.max_iterations = 2 if geom else 3
        p.geomPlanarPrior = bool(geom and planar)
        if geom:
            h.set_src_depths(src_depths)
            h.set_state(state["planes"], state["costs"])
        h.run(p, sd)
        if planar:
            planes, costs, g = h.get(geom=True)
            gpp = bool(p.geomPlanarPrior)
            prior, mask, ntri = hostlib.build_prior(cams[0], planes, costs, g if gpp else None, gpp, p.depth_min, p.depth_max)
            assert ntri > 0
            h.set_prior(prior, mask)
            p.planar_prior = True
            p.geom_consistency = False
            p.max_iterations = 3
            h.run(p, (sd + PRIOR_SEED_OFFSET) & 0xFFFFFFFFFFFFFFFF)
        state["planes"], state["costs"] = h.get()

    process(False, (not geom_pp) and planar_prior, seed)
    for g in range(geom_iterations):
        process(True, geom_pp and g != geom_iterations - 1, seed + 1 + g)
    return state["planes"], state["costs"]


def test_oversized_images_are_shrunk_once_and_k_follows(pm, oracle, engine):
    """PatchMatchInit's "Adjust image scale" (reference src/PatchMatch.cpp:893-925): images above max_image_size are shrunk
    (INTER_LINEAR) and K is scaled; the Scene caches the shrunk image together with the scaled K, so the second Run() of the
    planar-prior schedule and later passes see a consistent pair.  HIP pipeline == oracle on the shrunk inputs."""
    import copy
    hostlib = importlib.import_module("mp-mvs_amd.hostlib")
    sc = pm.synth.make_problem_scene(160, 120, n_src=3, spacing=0.4, quantize=True)
    cams, imgs = sc.problem(0, [1, 2, 3])
    new_w, new_h = 100, 75                                   # factor min(100/160, 100/120) = 0.625
    # photometric Run() + planar-prior Run(): two Run()s on the cached, shrunk scene
    depth, normal, cost = hostlib.run_pipeline(0, cams, imgs, 1, 0, True, False, 99, None, max_image_size=100, out_size=(new_h, new_w))
    small_imgs = [hostlib.resize_linear(im, new_w, new_h) for im in imgs]
    sx, sy = np.float32(new_w) / np.float32(160), np.float32(new_h) / np.float32(120)
    small_cams = []
    for c in cams:
        k = copy.copy(c)
        K = np.array(list(c.K), np.float32)
        K[0], K[2], K[4], K[5] = K[0] * sx, K[2] * sx, K[4] * sy, K[5] * sy
        for j in range(9):
            k.K[j] = float(K[j])
        k.width, k.height = new_w, new_h
        small_cams.append(k)
    planes, costs = oracle_pipeline(pm, oracle, hostlib, small_cams, small_imgs, None, 1, 0, True, False, 99)
    assert depth.shape == (new_h, new_w)
    assert np.array_equal(depth, planes[..., 3]) and np.array_equal(normal, planes[..., :3]) and np.array_equal(cost, costs)


@pytest.mark.parametrize("geom_iterations,planar_prior,geom_pp,max_scale", [(1, False, False, 2),   # cfg 2
                                                                           (2, True, True, 2),      # cfg 3 (shipped config.yaml)
                                                                           (0, True, False, 0)])    # photometric + prior
def test_process_problem_pipeline_bit_exact(pm, oracle, engine, geom_iterations, planar_prior, geom_pp, max_scale):
    hostlib = importlib.import_module("mp-mvs_amd.hostlib")
    sc = pm.synth.make_problem_scene(128, 96, n_src=4, spacing=0.4, quantize=True)
    cams, imgs = sc.problem(0, [1, 2, 3, 4])
    rng = np.random.default_rng(3)
    src_depths = [sc.views[i].gt_depth * (1.0 + 0.005 * rng.standard_normal((96, 128))).astype(np.float32) for i in (1, 2, 3, 4)]
    depth, normal, cost = hostlib.run_pipeline(0, cams, imgs, max_scale, geom_iterations, planar_prior, geom_pp, 4242, src_depths)
    planes, costs = oracle_pipeline(pm, oracle, hostlib, cams, imgs, src_depths, max_scale, geom_iterations, planar_prior, geom_pp, 4242)
    assert np.array_equal(depth, planes[..., 3]) and np.array_equal(normal, planes[..., :3]) and np.array_equal(cost, costs)
    gt = sc.views[0].gt_depth
    assert (np.abs(depth - gt) / gt < 0.05).mean() > 0.85


def test_scheduler_device_exchange_bit_exact(pm, oracle, engine):
    """6 Problems on one GPU with depth maps exchanged in HBM (export -> gather
    buffer -> set_src_depths_device) == the same schedule on the oracle with host arrays"""
    sched = importlib.import_module("mp-mvs_amd.schedule")
    sc, neigh = pm.synth.make_grid_scene(64, 48, 3, 2, spacing=0.5, rot_deg=1.0, quantize=True)
    cams = [v.cam for v in sc.views]
    imgs = [v.image for v in sc.views]
    kw = dict(geom_iterations=2, planar_prior=True, geom_planar_prior=True, seed=99)
    gpu = sched.SceneScheduler(cams, imgs, neigh, lambda: engine.create(0), device_tensors=True, max_scale=1)
    cpu = sched.SceneScheduler(cams, imgs, neigh, oracle.create, device_tensors=False, max_scale=1)
    rg, rc = gpu.run(**kw), cpu.run(**kw)
    assert np.array_equal(gpu.depth_maps(), cpu.depth_maps())
    for i in range(6):
        assert np.array_equal(rg[i][0], rc[i][0]) and np.array_equal(rg[i][1], rc[i][1]), f"problem {i}"
    # worker threads overlap host and device work of different Problems; same bits
    gpu3 = sched.SceneScheduler(cams, imgs, neigh, lambda: engine.create(0), device_tensors=True, max_scale=1, workers=3)
    r3 = gpu3.run(**kw)
    for i in range(6):
        assert np.array_equal(r3[i][0], rc[i][0]) and np.array_equal(r3[i][1], rc[i][1]), f"problem {i} (3 workers)"


def test_scheduler_device_exchange_full_size_bit_exact(pm, engine):
    """The device-resident exchange at BASELINE size: 16 Problems of 1600x1200 (4x4 camera grid, 8 source views each), one
    photometric and one geometric pass of one iteration, worker threads on.  Depth maps exchanged in HBM (export -> gathered
    buffer -> device-to-device copies on the contexts' own streams; state resident) against the same schedule with every map
    staged through host arrays (get -> numpy -> set_src_depths / set_state), which no stream-ordering mistake can touch.
    At this size a map is 7.7 MB and the gathered buffer 123 MB: a copy or fill that is still in flight when the next stage
    reads or overwrites the buffer changes bits (tests at 64x48 cannot see that)."""
    from concurrent.futures import ThreadPoolExecutor
    sched = importlib.import_module("mp-mvs_amd.schedule")
    W, H, G = 1600, 1200, 4
    centers = [((i - (G - 1) / 2.0) * 0.15, (j - (G - 1) / 2.0) * 0.15, 0.0) for j in range(G) for i in range(G)]
    with ThreadPoolExecutor(8) as pool:       # numpy releases the GIL in the big array operations of the renderer
        views = list(pool.map(lambda i: pm.synth.make_scene(W, H, centers, quantize=True, only={i}).views[i], range(G * G)))
    cams, imgs = [v.cam for v in views], [v.image for v in views]
    neigh = []
    for j in range(G):
        for i in range(G):
            cand = sorted(((ii - i) ** 2 + (jj - j) ** 2, jj * G + ii) for jj in range(G) for ii in range(G) if (ii, jj) != (i, j))
            neigh.append([c[1] for c in cand[:8]])
    kw = dict(geom_iterations=1, planar_prior=False, geom_planar_prior=False, seed=4711)
    dev = sched.SceneScheduler(cams, imgs, neigh, lambda: engine.create(0), device_tensors=True, max_scale=0, workers=4, iterations=1)
    rd = dev.run(**kw)
    dd = dev.depth_maps()
    del dev
    host = sched.SceneScheduler(cams, imgs, neigh, lambda: engine.create(0), device_tensors=False, max_scale=0, workers=1, iterations=1)
    rh = host.run(**kw)
    assert np.array_equal(dd, host.depth_maps())
    for i in range(G * G):
        assert np.array_equal(rd[i][0], rh[i][0]) and np.array_equal(rd[i][1], rh[i][1]) and np.array_equal(rd[i][2], rh[i][2]), f"problem {i}"
    assert np.isfinite(dd).all() and dd.min() > 0


def test_folder_pipeline_matches_oracle(pm, oracle, engine, tmp_path):
    """the reference's file-based flow (src/main.cpp:20-41 over pair.txt / cams / images,
    results exchanged through depths/normals/costs.dmb, sequential and in place) on the HIP
    path == the same sequence driven on the oracle in memory"""
    hostlib = importlib.import_module("mp-mvs_amd.hostlib")
    sc, neigh = pm.synth.make_grid_scene(64, 48, 3, 2, spacing=0.5, rot_deg=1.0, quantize=True)
    cams = [v.cam for v in sc.views]
    imgs = [v.image for v in sc.views]
    hostlib.write_dataset(str(tmp_path), cams, imgs, neigh)
    SEED, GEOM_IT, MAX_SCALE = 31337, 2, 1
    hostlib.run_folder(tmp_path, device=0, geom_iterations=GEOM_IT, planar_prior=True, geom_planar_prior=True, max_scale=MAX_SCALE, seed=SEED)
    # the pipeline works from the files: ReadCamera recomputes C = -R^T t in fp32
    # (reference src/PatchMatch.cpp:134-136), so the replica must use the cameras as parsed
    file_cams = []
    for i in range(6):
        c = hostlib.read_camera(tmp_path / "cams" / f"{i:08d}_cam.txt")
        c.height, c.width = imgs[i].shape
        file_cams.append(c)
    cams = file_cams

    # oracle replica (Gauss-Seidel: Problem i+1 already sees Problem i's new depth map)
    state = {}
    handles = {}
    for i in range(6):
        h = oracle.create()
        ids = [i] + neigh[i]
        h.set_views([cams[j] for j in ids], [imgs[j] for j in ids])
        handles[i] = h

    def process(i, geom, planar, seed):
        h = handles[i]
        dmin, dmax = pm.synth.kernel_depth_range(cams[i])
        p = pm.PatchMatchParams(num_images=1 + len(neigh[i]), depth_min=float(dmin), depth_max=float(dmax), max_scale=MAX_SCALE)
        p.geom_consistency, p.max_iterations, p.geomPlanarPrior = geom, (2 if geom else 3), bool(geom and planar)
        if geom:
            h.set_src_depths([state[j][0][..., 3] for j in neigh[i]])
            h.set_state(state[i][0], state[i][1])
        h.run(p, seed)
        if planar:
            planes, costs, g = h.get(geom=True)
            gpp = bool(p.geomPlanarPrior)
            prior, mask, ntri = hostlib.build_prior(cams[i], planes, costs, g if gpp else None, gpp, p.depth_min, p.depth_max)
            h.set_prior(prior, mask)
            p.planar_prior, p.geom_consistency, p.max_iterations = True, False, 3
            h.run(p, (seed + PRIOR_SEED_OFFSET) & 0xFFFFFFFFFFFFFFFF)
        state[i] = h.get()

    for i in range(6):
        process(i, False, False, SEED + i)
    for g in range(GEOM_IT):
        for i in range(6):
            process(i, True, g != GEOM_IT - 1, SEED + 100003 * (g + 1) + i)
    for i in range(6):
        d = tmp_path / "MPMVS" / f"2333_{i:08d}"
        assert np.array_equal(hostlib.read_dmb(d / "depths.dmb"), state[i][0][..., 3]), f"depths of image {i}"
        assert np.array_equal(hostlib.read_dmb(d / "normals.dmb"), state[i][0][..., :3]), f"normals of image {i}"
        assert np.array_equal(hostlib.read_dmb(d / "costs.dmb"), state[i][1]), f"costs of image {i}"
    # reference main()'s last step: RunFusion over the written maps -> MPMVS_model.ply
    npts = hostlib.fuse_folder(tmp_path)
    fusion = importlib.import_module("mp-mvs_amd.fusion")
    cloud, _, _ = oracle.fuse(cams, [True] * 6, [state[i][0][..., 3] for i in range(6)], [np.ascontiguousarray(state[i][0][..., :3]) for i in range(6)], imgs, neigh)
    assert npts == len(cloud) and npts > 100
    body = open(tmp_path / "MPMVS" / "MPMVS_model.ply", "rb").read().split(b"end_header\n", 1)[1]
    xyz = np.frombuffer(body, np.uint8).reshape(npts, 27)[:, :12].copy().view(np.float32)
    assert np.array_equal(xyz, cloud[:, :3])


def test_end_to_end_scene_tool(pm, engine, tmp_path):
    """tools/run_scene.py: schedule -> fusion -> PLY on a small scene"""
    import json
    import subprocess
    import sys
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ply = tmp_path / "scene.ply"
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "run_scene.py"), "--size", "160x120", "--grid", "3x2", "--out", str(ply)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    assert rep["images"] == 6 and rep["fused_points"] > 2000 and rep["median_point_error"] < 0.05
    assert rep["depth_within_1pct_of_gt"] > 0.7
    raw = open(ply, "rb").read()
    assert raw.startswith(b"ply\n") and len(raw.split(b"end_header\n", 1)[1]) == rep["fused_points"] * 27


@pytest.mark.parametrize("jacobi_workers", [0, 2])
def test_config_driven_main_flow(pm, engine, tmp_path, jacobi_workers):
    """tools/mpmvs_main.py = the reference's main() (src/main.cpp:6-55) with its config.yaml keys: JPEG images in,
    depth-map passes, sky-mask refinement, fusion, PLY out"""
    import json
    import os
    import subprocess
    import sys
    hostlib = importlib.import_module("mp-mvs_amd.hostlib")
    sc, neigh = pm.synth.make_grid_scene(160, 120, 3, 2, spacing=0.4, rot_deg=1.0, quantize=True)
    cams = [v.cam for v in sc.views]
    cols = [np.stack([g, 255 - g, g // 2 + 20], -1).astype(np.uint8) for g in (np.asarray(v.image).astype(np.uint8) for v in sc.views)]
    hostlib.write_dataset(str(tmp_path), cams, cols, neigh, fmt="jpg", jpeg_options=dict(quality=97, subsampling=0))
    for i in range(6):
        d = tmp_path / "MPMVS" / f"2333_{i:08d}"
        d.mkdir(parents=True)
        m = np.zeros((120, 160), np.uint8)
        m[:12] = 255
        open(d / "skymask.pgm", "wb").write(b"P5\n160 120\n255\n" + m.tobytes())
    cfg = tmp_path / "config.yaml"
    cfg.write_text(f'%YAML:1.0\n---\nInput-folder: "{tmp_path}"\nOutput-folder: "{tmp_path}"\nGeometric consistency iterations: 1\nPlaner prior: 1\n'
                   'Geometric consistency planer prior: 0\nSky segment: 1\nUse dynamic_consistency to fuse: 1\nSave Dmb as JPG: 1\n'
                   'Max source images num: 20\nMax image size: 3200\n')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "mpmvs_main.py"), "--config", str(cfg), "--seed", "7", "--jacobi-workers", str(jacobi_workers)],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    assert rep["sky_masks"] == 6 and rep["fused_points"] > 1000
    body = open(rep["ply"], "rb").read().split(b"end_header\n", 1)[1]
    assert len(body) == rep["fused_points"] * 27
    xyz = np.frombuffer(body, np.uint8).reshape(-1, 27)[:, :12].copy().view(np.float32)
    err = np.abs(xyz[:, 2] - pm.synth.height_field(xyz[:, 0].astype(np.float64), xyz[:, 1].astype(np.float64)))
    assert np.median(err) < 0.05
    for i in range(6):
        assert (tmp_path / "MPMVS" / f"2333_{i:08d}" / "skymask_refine.pgm").exists() and (tmp_path / "MPMVS" / f"2333_{i:08d}" / "depths.dmb").exists()


def test_folder_jacobi_workers_equal_the_scheduler(pm, engine, tmp_path):
    """RunFolderJacobi (C++, worker threads over a dataset folder) == SceneScheduler (Python, one process per GPU) on the same
    scene, seeds and schedule: both implement the Jacobi order of DESIGN.md section 7; the result does not depend on the
    number of workers"""
    hostlib = importlib.import_module("mp-mvs_amd.hostlib")
    schedule = importlib.import_module("mp-mvs_amd.schedule")
    sc, neigh = pm.synth.make_grid_scene(96, 72, 3, 2, spacing=0.4, rot_deg=1.0, quantize=True)
    cams = [v.cam for v in sc.views]
    imgs = [v.image for v in sc.views]
    out = {}
    for workers in (3, 1):
        d = tmp_path / f"w{workers}"
        hostlib.write_dataset(str(d), cams, imgs, neigh)
        assert hostlib.run_folder_jacobi(d, devices=(0,), workers=workers, geom_iterations=2, planar_prior=True, geom_planar_prior=True, max_scale=1, seed=321) == 6
        out[workers] = [tuple(hostlib.read_dmb(d / "MPMVS" / f"2333_{i:08d}" / f"{k}.dmb") for k in ("depths", "normals", "costs")) for i in range(6)]
    for a, b in zip(out[3], out[1]):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # the depth maps change hands in HBM between the passes (round 5: Scene::device_depth, mpmvs_set_src_depths_mixed); staged through
    # host arrays as in rounds 1-4 (MPMVS_FOLDER_HOST_EXCHANGE=1) the files are the same, bit for bit
    import os
    d = tmp_path / "host_exchange"
    hostlib.write_dataset(str(d), cams, imgs, neigh)
    os.environ["MPMVS_FOLDER_HOST_EXCHANGE"] = "1"
    try:
        assert hostlib.run_folder_jacobi(d, devices=(0,), workers=3, geom_iterations=2, planar_prior=True, geom_planar_prior=True, max_scale=1, seed=321) == 6
    finally:
        del os.environ["MPMVS_FOLDER_HOST_EXCHANGE"]
    for i in range(6):
        for k, want in zip(("depths", "normals", "costs"), out[3][i]):
            assert np.array_equal(hostlib.read_dmb(d / "MPMVS" / f"2333_{i:08d}" / f"{k}.dmb"), want), (i, k)
    file_cams = []
    for i in range(6):
        c = hostlib.read_camera(tmp_path / "w1" / "cams" / f"{i:08d}_cam.txt")
        c.height, c.width = imgs[i].shape
        file_cams.append(c)
    sched = schedule.SceneScheduler(file_cams, imgs, neigh, lambda: engine.create(0), max_scale=1, workers=2)
    res = sched.run(geom_iterations=2, planar_prior=True, geom_planar_prior=True, seed=321)
    for i in range(6):
        planes, costs, _ = res[i]
        assert np.array_equal(out[3][i][0], planes[..., 3]) and np.array_equal(out[3][i][1], planes[..., :3]) and np.array_equal(out[3][i][2], costs), f"image {i}"


def test_folder_schedule_fused_from_resident_contexts(pm, engine, tmp_path):
    """The pass schedule with the reference's last step, RunFusion (src/main.cpp:49), taken straight out of the Problems' resident
    contexts (RunFolderJacobi + FuseAtEnd -> mpmvs_fuse_ply_ctx: the final depth / normal maps are not uploaded again, and with
    write_maps = 0 never touch the disk) writes the same MPMVS_model.ply, byte for byte, as the file flow: run_folder_jacobi, then
    fuse_folder over the depths.dmb / normals.dmb it wrote."""
    hostlib = importlib.import_module("mp-mvs_amd.hostlib")
    sc, neigh = pm.synth.make_grid_scene(96, 72, 3, 2, spacing=0.4, rot_deg=1.0, quantize=True)
    cams = [v.cam for v in sc.views]
    imgs = [v.image for v in sc.views]
    kw = dict(devices=(0,), workers=3, geom_iterations=2, planar_prior=True, geom_planar_prior=True, max_scale=1, seed=321)
    a, b, c = tmp_path / "files", tmp_path / "resident", tmp_path / "resident_no_maps"
    for d in (a, b, c):
        hostlib.write_dataset(str(d), cams, imgs, neigh)
    assert hostlib.run_folder_jacobi(a, **kw) == 6
    n_files = hostlib.fuse_folder(a)
    want = (a / "MPMVS" / "MPMVS_model.ply").read_bytes()
    assert n_files > 100
    assert hostlib.run_folder_jacobi_fused(b, **kw) == n_files
    assert (b / "MPMVS" / "MPMVS_model.ply").read_bytes() == want
    assert (b / "MPMVS" / "2333_00000000" / "depths.dmb").exists()
    assert hostlib.run_folder_jacobi_fused(c, write_maps=False, **kw) == n_files
    assert (c / "MPMVS" / "MPMVS_model.ply").read_bytes() == want
    assert not (c / "MPMVS" / "2333_00000000" / "depths.dmb").exists()


def test_bench_self_launched_two_ranks_share_the_gpu():
    """`python bench.py --gpus 2 --full` started plainly: the launcher (which never touches the GPU) starts two fresh ranks; here both
    use GPU 0 over gloo (a 1-GPU box cannot run RCCL between two ranks).  One JSON line: the cfg-1 weak-scaling figures and,
    in the same invocation, configs[4] with its per-pass exchange (`secondary.cfg4`)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--backend", "gloo", "--share-device", "--size", "320x240",
                        "--cfg4-size", "160x120", "--cfg4-grid", "3", "--steps", "2", "--warmup", "1", "--workers", "2", "--peer-check-self", "--full"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 2 and out["scaling"] == "weak" and out["value"] > 0
    assert out["config"]["width"] == 320 and "NOT the BASELINE size" in out["config"]["workload"]
    assert out["value_survey_8d"] > 0 and out["within_1pct_of_gt"] > 0.8
    c4 = out["secondary"]["cfg4"]
    assert c4["n_gpus"] == 2 and c4["scaling"] == "strong" and c4["config"]["problems"] == 9
    assert [p["pass"] for p in c4["passes_last_step"]] == ["photometric", "geometric + planar prior", "geometric"]
    assert all(p["exchange_ms"] >= 0 for p in c4["passes_last_step"]) and c4["within_1pct_of_gt_rank0_mean"] > 0.6   # 160x120 views: coarser than the cfg-1 check above
    # the multi-GPU diagnostics of the line (round 6): every rank's peer table (empty on a one-GPU box) and its verified copy of the
    # source depth maps from a device buffer through mpmvs_set_src_depths_mixed -- here from the device itself (--peer-check-self)
    ranks = out["ranks"]
    assert [p["rank"] for p in ranks["peer_access"]] == [0, 1] and all(isinstance(p["peers"], dict) for p in ranks["peer_access"])
    assert [c["rank"] for c in ranks["peer_copy_check"]] == [0, 1] and all(c["ok"] is True for c in ranks["peer_copy_check"]), ranks["peer_copy_check"]


def test_scheduler_exchange_through_rccl_single_rank(pm, engine):
    """The exchange's collective on the real device: torch.distributed with the nccl backend (= RCCL) and ONE rank -- all this pool's
    1-GPU boxes allow -- issues all_gather_into_tensor on the gathered device buffer between the passes (RCCL's stream against the
    contexts' own streams: the ordering of schedule.py:_exchange).  Same bits as the run without the collective."""
    import os
    import socket
    import torch
    import torch.distributed as dist
    sched = importlib.import_module("mp-mvs_amd.schedule")
    sc, neigh = pm.synth.make_grid_scene(96, 64, 3, 2, spacing=0.5, rot_deg=1.0, quantize=True)
    cams = [v.cam for v in sc.views]
    imgs = [v.image for v in sc.views]
    kw = dict(geom_iterations=2, planar_prior=True, geom_planar_prior=True, seed=99)
    plain = sched.SceneScheduler(cams, imgs, neigh, lambda: engine.create(0), device_tensors=True, max_scale=1)
    want = plain.run(**kw)
    want_depths = plain.depth_maps()
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    torch.cuda.set_device(0)
    try:
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    except Exception as e:  # noqa: BLE001 -- a box without a usable bootstrap interface: the collective cannot be exercised there
        pytest.skip(f"RCCL could not be initialised on this box: {e}")
    try:
        coll = sched.SceneScheduler(cams, imgs, neigh, lambda: engine.create(0), rank=0, world=1, dist=dist, device_tensors=True, max_scale=1, workers=2)
        coll.force_collective = True
        got = coll.run(**kw)
        assert np.array_equal(coll.depth_maps(), want_depths)
        for i in range(6):
            assert np.array_equal(got[i][0], want[i][0]) and np.array_equal(got[i][1], want[i][1]), f"problem {i}"
    finally:
        dist.destroy_process_group()
