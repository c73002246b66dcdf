"""Seeded randomized parity sweep: random sizes / view counts / scales / iterations /
texture formats / modes, whole Run() schedules on the HIP path against the oracle, bit exact."""
import os

import numpy as np
import pytest

import fuzz_common

pytestmark = pytest.mark.gpu


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# 600 cases by default since round 5 (half a minute of the driver's GPU-test budget; rounds 1-4 ran 24 there and 400 / 1500 once by
# hand; 2000 passed on the round-5 and round-6 builds with the chained update launch, 87 s); MPMVS_FUZZ_CASES=N widens or narrows the sweep
@pytest.mark.parametrize("case", range(int(os.environ.get("MPMVS_FUZZ_CASES", "600"))))
def test_random_configuration_bit_exact(pm, oracle, engine, case):
    fuzz_common.run_case(pm, lambda: engine.create(0), oracle.create, case)


@pytest.mark.parametrize("V", [9, 13, 16, 17, 20, 24])
@pytest.mark.parametrize("quantize", [True, False])
def test_many_views_all_modes_bit_exact(pm, oracle, engine, V, quantize):
    """the shipped configuration allows 20 source views (reference config/config.yaml:19): photometric, geometric and
    planar-prior Run() at 9..24 views, both texture formats, against the oracle"""
    rng = np.random.default_rng(5000 + V)
    W, H = 57, 41
    sc = pm.synth.make_problem_scene(W, H, n_src=8, spacing=0.4, rot_deg=3.0, quantize=quantize, seed=V)
    ids = [1 + (i % 8) for i in range(V)]
    cams, imgs = sc.problem(0, ids)
    dmin, dmax = pm.synth.kernel_depth_range(cams[0])
    p = pm.PatchMatchParams(num_images=V + 1, depth_min=float(dmin), depth_max=float(dmax), max_scale=1, max_iterations=2)
    gpu, cpu = engine.create(0), oracle.create()
    for h in (gpu, cpu):
        h.set_views(cams, imgs)
        h.run(p, V)
    assert _same(gpu.get()[0], cpu.get()[0]) and _same(gpu.get()[1], cpu.get()[1])
    depths = [sc.views[i].gt_depth * (1.0 + 0.01 * rng.standard_normal((H, W))).astype(np.float32) for i in ids]
    p.geom_consistency, p.max_iterations = True, 2
    for h in (gpu, cpu):
        h.set_src_depths(depths)
        h.run(p, V + 1)
    assert all(_same(a, b) for a, b in zip(gpu.get(geom=True), cpu.get(geom=True)))
    prior = np.zeros((H, W, 4), np.float32)
    prior[..., 2] = -1.0
    prior[..., 3] = sc.views[0].gt_depth
    mask = (rng.uniform(size=(H, W)) < 0.5).astype(np.uint32)
    p.geom_consistency, p.planar_prior, p.max_iterations = False, True, 2
    for h in (gpu, cpu):
        h.set_prior(prior, mask)
        h.run(p, V + 2)
    assert _same(gpu.get()[0], cpu.get()[0]) and _same(gpu.get()[1], cpu.get()[1])
