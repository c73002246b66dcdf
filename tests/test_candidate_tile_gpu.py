"""The candidate-cost tile of the update kernel (csrc/pm_cand_tile.hpp; update_body, pm_kernels.hpp): a block stages the stored costs
its 88-neighbour searches can ask for once in LDS, with the search's start value at positions outside the image, and every pixel
searches the tile.  HIP and the CPU oracle must agree bit for bit on planes, costs and selected views (and geometric costs).

Sizes (photometric Run(), max_scale 0; 8-bit images run one-wave 16x8 blocks, non-integer images four-wave 16x32 blocks; chained
and one launch per pass):
  17x9   one pixel column and one row spill into a second block; nearly the whole tile lies outside the image
  47x24  the horizontal strip of the centre column ends exactly at columns 0 and W - 1, the vertical strip reaches row 0 from row 23
  62x54  exactly one bounding box of a one-wave block
  96x87  several block rows, odd height, a partial last block
and 96x87 with max_scale 2 (scales 1 and 2 run 256-thread blocks: at scale 1 their 36 x 52 reference tile is staged next to the cost
tile, at scale 2 the reference tile is too large and only the cost tile is staged), a geometric Run() and a
planar-prior step sequence at 47x24 (separate instantiations of the same search).

Ties and sentinels: states set with set_state in which all stored costs are equal, and in which single positions -- image corners,
border midpoints, positions 23 away from a border, both colours -- hold 2.0, +0.0, 3.402823466e+38 (the search's start value),
infinity and NaN; one step of each colour from each.  The oracle takes any state as it is (set_state copies; its search is the
reference's strict `best > cost` under the bounds test), so no value is left out: test_oracle_accepts_the_sentinel_states checks
that on the CPU.
"""
import os

import numpy as np
import pytest

SEED = 977
V = 8

SIZES = [(17, 9), (47, 24), (62, 54), (96, 87)]
SENTINELS = np.array([2.0, 0.0, 3.402823466e+38, np.inf, np.nan], np.float32)


def same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def state(h, geom=False):
    """planes, costs, (geometric costs,) selected views"""
    return tuple(h.get(geom=geom)) + (h.get_selected_views(),)


def assert_state(what, got, want):
    names = ("planes", "costs", "geom costs", "selected views") if len(want) == 4 else ("planes", "costs", "selected views")
    for n, g, w in zip(names, got, want):
        assert same(g, w), f"{what}: {n} differ on {int((np.asarray(g).view(np.uint32) != np.asarray(w).view(np.uint32)).sum())} values"


_scenes = {}


def problem(pm, W, H, quantize):
    key = (W, H, quantize)
    if key not in _scenes:
        sc = pm.synth.make_problem_scene(W, H, n_src=V, spacing=0.5, quantize=quantize)
        cams, imgs = sc.problem(0, list(range(1, V + 1)))
        dmin, dmax = pm.synth.kernel_depth_range(cams[0])
        _scenes[key] = (sc, cams, imgs, float(dmin), float(dmax))
    return _scenes[key]


def params(pm, W, H, quantize, max_scale=0):
    sc, cams, imgs, dmin, dmax = problem(pm, W, H, quantize)
    return pm.PatchMatchParams(num_images=V + 1, depth_min=dmin, depth_max=dmax, max_scale=max_scale)


def cpu_handle(pm, oracle, W, H, quantize):
    sc, cams, imgs, dmin, dmax = problem(pm, W, H, quantize)
    cpu = oracle.create()
    cpu.set_views(cams, imgs)
    return cpu


def gpu_handle(pm, engine, W, H, quantize, per_pass=False):
    sc, cams, imgs, dmin, dmax = problem(pm, W, H, quantize)
    if per_pass:
        os.environ["MPMVS_CHAIN"] = "0"
    try:
        gpu = engine.create(0)
    finally:
        os.environ.pop("MPMVS_CHAIN", None)
    gpu.set_views(cams, imgs)
    assert gpu.texture_format() == ("u8" if quantize else "f32")
    assert gpu.chain_status() == (0 if per_pass else 1)
    return gpu


_runs = {}


def oracle_run(pm, oracle, W, H, quantize, max_scale=0):
    """the oracle's photometric Run(), computed once per case and shared"""
    key = (W, H, quantize, max_scale)
    if key not in _runs:
        cpu = cpu_handle(pm, oracle, W, H, quantize)
        cpu.run(params(pm, W, H, quantize, max_scale), SEED)
        _runs[key] = tuple(np.array(a) for a in state(cpu))
    return _runs[key]


@pytest.mark.gpu
@pytest.mark.parametrize("per_pass", [False, True])
@pytest.mark.parametrize("quantize", [True, False])
@pytest.mark.parametrize("W,H", SIZES)
def test_photometric_run(pm, oracle, engine, W, H, quantize, per_pass):
    want = oracle_run(pm, oracle, W, H, quantize)
    gpu = gpu_handle(pm, engine, W, H, quantize, per_pass)
    gpu.run(params(pm, W, H, quantize), SEED)
    assert_state(f"{W}x{H}", state(gpu), want)


@pytest.mark.gpu
def test_run_over_three_scales(pm, oracle, engine):
    W, H = 96, 87
    want = oracle_run(pm, oracle, W, H, True, max_scale=2)
    gpu = gpu_handle(pm, engine, W, H, True)
    gpu.run(params(pm, W, H, True, max_scale=2), SEED)
    assert_state("max_scale 2", state(gpu), want)


@pytest.mark.gpu
def test_geometric_run(pm, oracle, engine):
    W, H = 47, 24
    p0, c0, s0 = oracle_run(pm, oracle, W, H, True)
    sc = problem(pm, W, H, True)[0]
    rng = np.random.default_rng(7)
    depths = [sc.views[1 + i].gt_depth * (1.0 + 0.005 * rng.standard_normal((H, W))).astype(np.float32) for i in range(V)]
    prm = params(pm, W, H, True)
    prm.geom_consistency, prm.max_iterations = True, 2
    out = []
    for h in (cpu_handle(pm, oracle, W, H, True), gpu_handle(pm, engine, W, H, True)):
        h.set_src_depths(depths)
        h.set_state(p0, c0)
        h.set_selected_views(s0)
        h.run(prm, SEED + 1)
        out.append(state(h, geom=True))
    assert_state("geometric", out[1], out[0])


@pytest.mark.gpu
def test_planar_prior_steps(pm, oracle, engine):
    """INIT with the prior, then two iterations of black / red passes, one step each, compared after every launch"""
    W, H = 47, 24
    p0, c0, s0 = oracle_run(pm, oracle, W, H, True)
    sc = problem(pm, W, H, True)[0]
    rng = np.random.default_rng(9)
    cam, gt = sc.views[0].cam, sc.views[0].gt_depth.astype(np.float64)
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    X = np.stack([gt * (u - cam.K[2]) / cam.K[0], gt * (v - cam.K[5]) / cam.K[4], gt], -1)
    n = np.zeros((H, W, 3))
    n[..., 2] = -1.0
    n[..., 0] = 0.05 * rng.standard_normal((H, W))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    prior = np.concatenate([n, -(n * X).sum(-1)[..., None]], -1).astype(np.float32)
    mask = (rng.uniform(size=(H, W)) < 0.6).astype(np.uint32) * np.arange(1, H * W + 1, dtype=np.uint32).reshape(H, W)
    prm = params(pm, W, H, True)
    prm.planar_prior = True
    seq = [(pm.KIND_INIT, 0, 0)] + [(k, it, 0) for it in range(2) for k in (pm.KIND_BLACK, pm.KIND_RED)]
    cpu, gpu = cpu_handle(pm, oracle, W, H, True), gpu_handle(pm, engine, W, H, True)
    for h in (cpu, gpu):
        h.set_state(p0, c0)
        h.set_selected_views(s0)
        h.set_prior(prior, mask)
    for launch, (kind, it, scale) in enumerate(seq):
        for h in (cpu, gpu):
            h.step(prm, SEED + 2, kind, it, scale, launch)
        assert_state(f"prior, launch {launch}", state(gpu), state(cpu))


def sentinel_states(W, H, base):
    """all costs equal; then, five times, the sentinels dealt to the marked positions, each time one place further: every position
    holds every value once"""
    yield "all equal", np.full((H, W), 0.25, np.float32)
    xs, ys = [0, 1, 23, 24, W // 2, W - 25, W - 24, W - 2, W - 1], [0, 1, 23, 24, H // 2, H - 25, H - 24, H - 2, H - 1]
    marks = [(x, y) for y in ys for x in xs]   # corners, border points, 23 and 24 away from each border (both colours), the centre
    for turn in range(len(SENTINELS)):
        c = base.copy()
        for k, (x, y) in enumerate(marks):
            c[y, x] = SENTINELS[(k + turn) % len(SENTINELS)]
        yield f"sentinels, turn {turn}", c


def step_each_colour(pm, handles, prm, W, H, p0, s0, costs):
    """from the same state, one black step and one red step on every handle; returns the states [handle][colour]"""
    out = [[] for _ in handles]
    for launch, kind in ((1, pm.KIND_BLACK), (2, pm.KIND_RED)):
        for k, h in enumerate(handles):
            h.set_state(p0, costs)
            h.set_selected_views(s0)
            h.step(prm, SEED + 3, kind, 0, 0, launch)
            out[k].append(state(h))
    return out


def test_oracle_accepts_the_sentinel_states(pm, oracle):
    """CPU only: the oracle steps from every sentinel state, keeps the costs of the colour it does not update as they were set
    (bit for bit, NaN included) and writes finite costs for the colour it updates"""
    W, H = 62, 54
    p0, c0, s0 = oracle_run(pm, oracle, W, H, True)
    cpu = cpu_handle(pm, oracle, W, H, True)
    prm = params(pm, W, H, True)
    yy, xx = np.mgrid[0:H, 0:W]
    for name, costs in sentinel_states(W, H, c0):
        (black, red), = step_each_colour(pm, [cpu], prm, W, H, p0, s0, costs)
        for colour, st in ((0, black), (1, red)):
            other = ((xx + yy) & 1) != colour
            assert same(st[1][other], costs[other]), f"{name}: colour {colour} touched the other colour's costs"
            assert np.isfinite(st[1][~other]).all(), f"{name}: colour {colour} left a non-finite cost"


@pytest.mark.gpu
@pytest.mark.parametrize("quantize", [True, False])
def test_ties_and_sentinels(pm, oracle, engine, quantize):
    W, H = 62, 54
    p0, c0, s0 = oracle_run(pm, oracle, W, H, quantize)
    cpu, gpu = cpu_handle(pm, oracle, W, H, quantize), gpu_handle(pm, engine, W, H, quantize)
    prm = params(pm, W, H, quantize)
    for name, costs in sentinel_states(W, H, c0):
        want, got = step_each_colour(pm, [cpu, gpu], prm, W, H, p0, s0, costs)
        for colour in (0, 1):
            assert_state(f"{name}, colour {colour}", got[colour], want[colour])
