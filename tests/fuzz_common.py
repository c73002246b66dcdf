"""The seeded random configurations of the parity sweeps (tests/test_fuzz_gpu.py for the default build, tests/test_q8_variants_gpu.py
for the build with 8-bit interpolation fractions): draw(case) makes every random draw of a case, in one fixed order, without
rendering or running anything; run_case runs the drawn case on a GPU handle and an oracle handle and compares them bit for bit.

The order of the draws is part of the cases: a draw added, dropped or moved gives every case other inputs."""
import importlib
from types import SimpleNamespace

import numpy as np

VIEW_COUNTS = [1, 2, 3, 4, 5, 7, 8, 9, 12, 16, 17, 20, 24, 25, 32]   # every bucket of the update kernel (8 / 16 / 24 / 32 views) and its edges


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def draw(case):
    """the configuration of `case`: sizes, view count, texel format, schedule, scene arguments, parameters, and the random arrays
    of the geometric (mode >= 1) and planar-prior (mode == 2) runs"""
    synth = importlib.import_module("mp-mvs_amd").synth
    rng = np.random.default_rng(1000 + case)
    c = SimpleNamespace(case=case)
    c.W = int(rng.integers(6, 90))
    c.H = int(rng.integers(6, 70))
    c.V = int(rng.choice(VIEW_COUNTS))
    c.quantize = bool(rng.integers(0, 2))
    c.max_scale = int(rng.integers(0, 3))
    c.iters = int(rng.integers(1, 4))
    c.spacing = float(rng.uniform(0.2, 0.8))
    c.harsh = case % 3 == 0   # every third case: strongly different cameras
    c.scene = dict(n_src=min(c.V, 8), spacing=c.spacing, rot_deg=float(rng.uniform(0, 15 if c.harsh else 4)), quantize=c.quantize,
                   seed=int(rng.integers(1, 10 ** 6)), focal_jitter=0.25 if c.harsh else 0.0)
    c.ids = [1 + (i % 8) for i in range(c.V)]
    c.textureless = bool(rng.integers(0, 3) == 0)   # a textureless patch (variance sentinel)
    # the depth range is the reference camera's, which the scene's seed decides without an image being rendered
    dmin, dmax = synth.kernel_depth_range(synth.scene_cameras(c.W, c.H, [(0.0, 0.0, 0.0)], seed=c.scene["seed"], rot_deg=c.scene["rot_deg"],
                                                              focal_jitter=c.scene["focal_jitter"])[0])
    if rng.integers(0, 4) == 0:            # a depth range that throws hypotheses out of view
        dmin = dmin * 0.2
    c.dmin, c.dmax = dmin, dmax
    c.params = dict(num_images=c.V + 1, depth_min=float(dmin), depth_max=float(dmax), max_scale=c.max_scale, max_iterations=c.iters,
                    top_k=int(rng.integers(1, 6)), sigma_spatial=float(rng.uniform(2, 8)), sigma_color=float(rng.uniform(1, 6)))
    c.mode = int(rng.integers(0, 3))
    if c.mode >= 1:                        # geometric consistency on top
        c.depth_noise = []
        for _ in c.ids:
            noise = (1.0 + 0.01 * rng.standard_normal((c.H, c.W))).astype(np.float32)
            c.depth_noise.append((noise, rng.uniform(size=noise.shape) < 0.05))
        c.geom_iters = int(rng.integers(1, 3))
    if c.mode == 2:                        # planar prior on top
        prior = np.zeros((c.H, c.W, 4), np.float32)
        n = rng.normal(size=(c.H, c.W, 3)) * 0.1
        n[..., 2] = -1.0
        n /= np.linalg.norm(n, axis=-1, keepdims=True)
        prior[..., :3] = n
        prior[..., 3] = rng.uniform(dmin, dmax, (c.H, c.W))
        c.prior = prior
        c.mask = (rng.uniform(size=(c.H, c.W)) < 0.5).astype(np.uint32) * 7
        c.prior_iters = int(rng.integers(1, 4))
    return c


def run_case(pm, make_gpu, make_cpu, case):
    """whole Run() schedules of the drawn case on make_gpu() and make_cpu(): photometric, then geometric and planar-prior on top
    as the case's mode says; planes, costs, selected views and geometric costs must agree bit for bit"""
    c = draw(case)
    W, H, V = c.W, c.H, c.V
    sc = pm.synth.make_problem_scene(W, H, **c.scene)
    cams, imgs = sc.problem(0, c.ids)
    imgs = [im.copy() for im in imgs]
    if c.textureless:
        imgs[0][: H // 2, : W // 3] = 128.0
    dmin, dmax = pm.synth.kernel_depth_range(cams[0])
    assert (c.dmin == dmin * 0.2 or c.dmin == dmin) and c.dmax == dmax, "draw() and the rendered scene disagree about the reference camera"
    p = pm.PatchMatchParams(**c.params)
    gpu, cpu = make_gpu(), make_cpu()
    for h in (gpu, cpu):
        h.set_views(cams, imgs)
        h.run(p, 77 + case)
    gp, gc = gpu.get()
    cp, cc = cpu.get()
    assert _same(gp, cp) and _same(gc, cc) and np.array_equal(gpu.get_selected_views(), cpu.get_selected_views()), f"photometric W={W} H={H} V={V}"
    if c.mode >= 1:
        depths = []
        for i, (noise, drop) in zip(c.ids, c.depth_noise):
            d = sc.views[i].gt_depth * noise
            d[drop] = 0.0
            depths.append(d)
        p.geom_consistency, p.max_iterations = True, c.geom_iters
        for h in (gpu, cpu):
            h.set_src_depths(depths)
            h.run(p, 78 + case)
        g3, c3 = gpu.get(geom=True), cpu.get(geom=True)
        assert all(_same(a, b) for a, b in zip(g3, c3)), f"geom W={W} H={H} V={V}"
    if c.mode == 2:
        p.geom_consistency, p.planar_prior, p.max_iterations = False, True, c.prior_iters
        for h in (gpu, cpu):
            h.set_prior(c.prior, c.mask)
            h.run(p, 79 + case)
        assert _same(gpu.get()[0], cpu.get()[0]) and _same(gpu.get()[1], cpu.get()[1]), f"prior W={W} H={H} V={V}"
