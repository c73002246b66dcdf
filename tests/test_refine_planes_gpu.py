"""The five refinement candidates' planes of the update kernel (update_body, csrc/pm_kernels.hpp: cpl) live in registers in the
variants that have them (kPlanesInRegs) and in private memory in the others: the dealt rounds publish a live candidate's plane from
there and the final acceptance takes the survivor from there.  Placement only, so nothing may change a bit: planes, costs, selected
views and geometric costs are compared with the CPU oracle, bit for bit, every pixel (the uint32 comparison of
tests/test_update_bookkeeping_gpu.py, which covers up to 9 views; this file covers the buckets above and the states below).

Sizes: 16x8 (exactly one wave) and 33x17 (the last column and the last row hold one pixel: waves with n_here < 64).
View counts, at the edges of the buckets (1-8, 9-16, 17-24, 25-32 views) whose variants keep the planes in registers; the sources
repeat the views 1-8:
  photometric Run() with max_scale 2 (scales 2, 1, 0)   fp16 texels 8, 25, 32 (25-32: scales 0 and 2; scale 1 stays in memory and runs
                                                        in the same Run())                         fp32 texels 9, 16
  geometric Run()                                       fp16 texels 8, 9, 16, 17, 24               fp32 texels 9, 16
  planar-prior Run() with masked pixels                 fp16 texels 8
Left out because every variant of the bucket stayed in memory (their code is the parent's): photometric with fp16 texels and 9-24
views, fp32 texels with 1-8 and 17-32 views in every mode, the geometric variant with 25-32 views, the planar prior with fp32 texels
and with more than 8 views.
Launches: chained, and one launch per pass (MPMVS_CHAIN=0) at one size and one view count per mode (k_update receives one pass instead
of six, the body is the same code).
Three states at which the register form can go wrong, each at view counts of variants in registers:
  1. depth_min == depth_max on fronto-parallel planes at that depth: nearly every candidate is out of range, rounds are empty and
     the final acceptance has to skip all five;
  2. masked prior pixels with restricted_cost == 0: every pixel holds the prior's plane, so no neighbour beats the current plane
     (the same plane gives the same restricted cost, and the test is strict), restricted_cost stays 0, every in-range candidate with
     a valid prior term would be accepted in turn and only the last of them is evaluated: the final acceptance takes exactly that one;
  3. source views 2-7 (and their repetitions) blank: few views carry weight and a round publishes for few candidates.
The build with 8-bit interpolation fractions runs the flagship variant only here (photometric, 8 views, fp16 texels, scale 0); its
other variants and these states run in tests/test_q8_variants_gpu.py, on the helpers of tests/update_variants_common.py.
"""
import numpy as np
import pytest

from update_variants_common import assert_state, cpu_handle, gpu_handle, one_plane, params, prior_planes, problem, start, state, wanted

pytestmark = pytest.mark.gpu

SEED = 2407
SIZES = [(16, 8), (33, 17)]
# (view count, quantize): quantize = 8-bit images, fp16 texels; otherwise fp32 texels
PHOTO_VIEWS = [(V, True) for V in (8, 25, 32)] + [(9, False), (16, False)]
GEOM_VIEWS = [(V, True) for V in (8, 9, 16, 17, 24)] + [(9, False), (16, False)]
PRIOR_VIEWS = [(8, True)]


def cases(views, per_pass):
    return [(W, H, V, q, False) for (W, H) in SIZES for (V, q) in views] + [(33, 17) + per_pass + (True,)]


def photometric(pm, oracle, W, H, V, quantize):
    def compute():
        cpu = cpu_handle(pm, oracle, W, H, V, quantize)
        cpu.run(params(pm, W, H, V, quantize, max_scale=2), SEED)
        return state(cpu)
    return wanted(("photo", W, H, V, quantize), compute)


@pytest.mark.parametrize("W,H,V,quantize,per_pass", cases(PHOTO_VIEWS, (25, True)))
def test_photometric_scales_2_1_0(pm, oracle, engine, W, H, V, quantize, per_pass):
    want = photometric(pm, oracle, W, H, V, quantize)
    gpu = gpu_handle(pm, engine, W, H, V, quantize, per_pass)
    gpu.run(params(pm, W, H, V, quantize, max_scale=2), SEED)
    assert_state(f"{W}x{H}, {V} views", state(gpu), want)


@pytest.mark.parametrize("W,H,V,quantize,per_pass", cases(GEOM_VIEWS, (16, False)))
def test_geometric_run(pm, oracle, engine, W, H, V, quantize, per_pass):
    st = photometric(pm, oracle, W, H, V, quantize)
    sc = problem(pm, W, H, V, quantize)[0]
    rng = np.random.default_rng(7)
    depths = [sc.views[1 + (i % 8)].gt_depth * (1.0 + 0.005 * rng.standard_normal((H, W))).astype(np.float32) for i in range(V)]
    prm = params(pm, W, H, V, quantize, max_scale=0)
    prm.geom_consistency, prm.max_iterations = True, 2

    def run(h):
        h.set_src_depths(depths)
        start(h, st)
        h.run(prm, SEED + 1)
        return state(h, geom=True)

    want = wanted(("geom", W, H, V, quantize), lambda: run(cpu_handle(pm, oracle, W, H, V, quantize)))
    assert_state(f"geometric {W}x{H}, {V} views", run(gpu_handle(pm, engine, W, H, V, quantize, per_pass)), want)


@pytest.mark.parametrize("W,H,V,quantize,per_pass", cases(PRIOR_VIEWS, (8, True)))
def test_planar_prior_run(pm, oracle, engine, W, H, V, quantize, per_pass):
    st = photometric(pm, oracle, W, H, V, quantize)
    prior, mask = prior_planes(problem(pm, W, H, V, quantize)[0], W, H, np.random.default_rng(9))
    assert (mask > 0).any() and (mask == 0).any()
    prm = params(pm, W, H, V, quantize, max_scale=0)
    prm.planar_prior = True

    def run(h):
        start(h, st)
        h.set_prior(prior, mask)
        h.run(prm, SEED + 2)
        return state(h)

    want = wanted(("prior", W, H, V, quantize), lambda: run(cpu_handle(pm, oracle, W, H, V, quantize)))
    assert_state(f"prior {W}x{H}, {V} views", run(gpu_handle(pm, engine, W, H, V, quantize, per_pass)), want)


@pytest.mark.parametrize("V,quantize", [(8, True), (32, True), (16, False)])
def test_depth_range_of_one_value(pm, oracle, engine, V, quantize):
    """state 1: every pixel holds a fronto-parallel plane at depth d, and depth_min == depth_max == d; one black and one red pass,
    compared after each"""
    W, H = 33, 17
    sc, cams, imgs, dmin, dmax = problem(pm, W, H, V, quantize)
    st = photometric(pm, oracle, W, H, V, quantize)
    d = np.float32(0.5 * (dmin + dmax))
    prm = pm.PatchMatchParams(num_images=V + 1, depth_min=float(d), depth_max=float(d), max_scale=0)
    cpu, gpu = cpu_handle(pm, oracle, W, H, V, quantize), gpu_handle(pm, engine, W, H, V, quantize)
    for h in (cpu, gpu):
        start(h, (one_plane(W, H, d), st[1], st[2]))
    for launch, kind in ((1, pm.KIND_BLACK), (2, pm.KIND_RED)):
        for h in (cpu, gpu):
            h.step(prm, SEED + 4, kind, 0, 0, launch)
        assert_state(f"one depth, {V} views, launch {launch}", state(gpu), state(cpu))


@pytest.mark.parametrize("W,H", SIZES)
def test_masked_prior_with_restricted_cost_zero(pm, oracle, engine, W, H):
    """state 2: the prior is one fronto-parallel plane, every pixel holds that plane and every pixel is masked.  A neighbour's plane is
    the pixel's own, its restricted cost equals the current one and the strict test fails: restricted_cost stays 0 and each pass
    accepts the last in-range candidate with a valid prior term, whatever its cost.  A black and a red pass, each from that state."""
    V, quantize = 8, True
    sc, cams, imgs, dmin, dmax = problem(pm, W, H, V, quantize)
    st = photometric(pm, oracle, W, H, V, quantize)
    planes = one_plane(W, H, np.float32(0.5 * (dmin + dmax)))
    mask = np.arange(1, H * W + 1, dtype=np.uint32).reshape(H, W)
    prm = params(pm, W, H, V, quantize, max_scale=0)
    prm.planar_prior = True
    cpu, gpu = cpu_handle(pm, oracle, W, H, V, quantize), gpu_handle(pm, engine, W, H, V, quantize)
    yy, xx = np.mgrid[0:H, 0:W]
    for launch, kind, parity in ((1, pm.KIND_BLACK, 0), (2, pm.KIND_RED, 1)):
        for h in (cpu, gpu):
            start(h, (planes, st[1], st[2]))
            h.set_prior(planes, mask)
            h.step(prm, SEED + 5, kind, 0, 0, launch)
        want = state(cpu)
        moved = (want[0].view(np.uint32) != planes.view(np.uint32)).any(-1)
        updated = ((xx + yy) & 1) == parity
        assert not moved[~updated].any()
        # the state is the one meant: every pixel of the pass took its LAST candidate (the current normal at a depth perturbed by at
        # most 2 %, always in range here), which a positive restricted_cost or the cost test of an unmasked pixel would not let through
        got = want[0][updated]
        assert moved[updated].all() and (got[:, :3] == planes[0, 0, :3]).all() and (np.abs(got[:, 3] / planes[0, 0, 3] - 1.0) < 0.0201).all()
        assert_state(f"restricted cost 0, {W}x{H}, launch {launch}", state(gpu), want)


@pytest.mark.parametrize("V,quantize", [(8, True), (32, True), (16, False)])
def test_blank_source_views(pm, oracle, engine, V, quantize):
    """state 3: the source views 2-7 of 8, and every repetition of them, hold one grey value: no texture, cost 2.0 against every plane"""
    W, H = 33, 17
    sc, cams, imgs, dmin, dmax = problem(pm, W, H, V, quantize)
    textured = [k for k in range(V) if k % 8 < 2]
    blank = [im if k == 0 or (k - 1) in textured else np.full_like(im, 128.0) for k, im in enumerate(imgs)]   # imgs[0] is the reference, imgs[1 + k] source view k
    prm = params(pm, W, H, V, quantize, max_scale=0)
    cpu = cpu_handle(pm, oracle, W, H, V, quantize, blank)
    cpu.run(prm, SEED + 3)
    want = state(cpu)
    sel = want[2][: 2 * (H // 2)]   # the rows the checkerboard passes update
    chosen = np.array([int(((sel >> v) & 1).sum()) for v in range(V)])
    is_tex = np.array([v in textured for v in range(V)])
    assert 2 * chosen[~is_tex].max() < chosen[is_tex].min(), f"the blank views are meant to be left without weight mostly: {chosen.tolist()}"
    gpu = gpu_handle(pm, engine, W, H, V, quantize, imgs=blank)
    gpu.run(prm, SEED + 3)
    assert_state(f"blank views, {V} views", state(gpu), want)


@pytest.mark.parametrize("W,H", SIZES)
def test_q8_build_flagship_variant(pm, oracle, engine, W, H):
    """the build with 8-bit interpolation fractions: photometric, 8 views, fp16 texels, scale 0"""
    V, quantize = 8, True
    prm = params(pm, W, H, V, quantize, max_scale=0)
    cpu = cpu_handle(pm, oracle, W, H, V, quantize, q8=True)
    cpu.run(prm, SEED + 6)
    gpu = gpu_handle(pm, engine, W, H, V, quantize, q8=True)
    gpu.run(prm, SEED + 6)
    assert_state(f"8-bit fractions, {W}x{H}", state(gpu), state(cpu))
