"""The build with 8-bit interpolation fractions (libmpmvs_hip_q8.so: csrc/mpmvs_api.hip compiled with -DPM_TEX_Q8) carries its own
copy of every kernel that samples a source image -- 40 instantiations of k_update, 24 of k_init, the eval_ncc kernels -- each with
its own register allocation and, for the update, its own choice of where the candidate planes and costs live (kPlanesInRegs,
kCostsByCandidate in csrc/pm_kernels.hpp; one choice exists in this build only: photometric, 25-32 views, fp16 texels, scale 0).
Every comparison here is on uint32 bits against the oracle in the same arithmetic (orc_set_texture_q8).

a. Named matrix: 16x8 (one wave) and 33x17 (the last row and column hold one pixel), source views at both edges of every bucket
   (1, 8, 9, 16, 17, 24, 25, 32; the sources repeat the views 1-8), both texel formats; per context a photometric Run() through
   the scales 2, 1, 0, and from its state a geometric Run() and a planar-prior Run() with about 60 % of the pixels masked.
b. One launch per pass (MPMVS_CHAIN=0), the three Run()s, one context per bucket.
c. k_init at the scales 0, 1, 2 through step(KIND_INIT): Run() reaches it at max_scale only.
d. The states of tests/test_refine_planes_gpu.py (a depth range of one value, masked prior with restricted cost 0, blank source
   views) at the variant that only this build keeps in another form and at its neighbours.
e. Seeded sweep: the cases 0 .. Q8_FUZZ_CASES - 1 of tests/test_fuzz_gpu.py's draws (MPMVS_Q8_FUZZ_CASES widens it).
f. Tied fractions: a scene whose sample coordinates are exact, with fractions on, just below and just above (k + 0.5) / 256
   (q8_variants_common): rounding the tie to even instead of up differs only there.  Random scenes meet a tie now and then (a
   coordinate of 16 .. 32 has 19 bits of fraction, one tap in 2^11 sits on one: a build that rounds to even, tried once by hand,
   differed from the oracle in most cases of a-e, by a handful of values each); here every tap of whole views sits on one, at chosen k, and the
   views are compared among themselves as well.
tests/test_q8_variants_cpu.py counts the variants that a-e reach and checks the construction of f on the oracle."""
import os

import numpy as np
import pytest

import fuzz_common
import q8_variants_common as q8c
from q8_variants_common import SEED
from update_variants_common import (assert_state, cpu_handle, create_gpu, gpu_handle, one_plane, params, prior_planes, problem, same, start, state,
                                    wanted)

pytestmark = pytest.mark.gpu


def cpu_q8(pm, oracle, W, H, V, quantize, imgs=None):
    return cpu_handle(pm, oracle, W, H, V, quantize, imgs, q8=True)


def gpu_q8(pm, engine, W, H, V, quantize, per_pass=False, imgs=None):
    return gpu_handle(pm, engine, W, H, V, quantize, per_pass, imgs, q8=True)


def test_the_twin_is_the_build_under_test(engine):
    assert engine.load_variant(engine.LIB_Q8_PATH)[1]["texture_filter_bits"]() == 8


# --- a, b: the three Run()s of a context ------------------------------------------------------------------------------------------

def photometric(pm, oracle, W, H, V, quantize):
    def compute():
        cpu = cpu_q8(pm, oracle, W, H, V, quantize)
        cpu.run(params(pm, W, H, V, quantize, max_scale=2), SEED)
        return state(cpu)
    return wanted(("q8 photo", W, H, V, quantize), compute)


def check_photometric(pm, oracle, engine, W, H, V, quantize, per_pass=False):
    want = photometric(pm, oracle, W, H, V, quantize)
    gpu = gpu_q8(pm, engine, W, H, V, quantize, per_pass)
    gpu.run(params(pm, W, H, V, quantize, max_scale=2), SEED)
    assert_state(f"photometric {W}x{H}, {V} views", state(gpu), want)


def check_geometric(pm, oracle, engine, W, H, V, quantize, per_pass=False):
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

    want = wanted(("q8 geom", W, H, V, quantize), lambda: run(cpu_q8(pm, oracle, W, H, V, quantize)))
    assert (want[2] != 0).any()   # there are geometric costs to compare
    assert_state(f"geometric {W}x{H}, {V} views", run(gpu_q8(pm, engine, W, H, V, quantize, per_pass)), want)


def check_prior(pm, oracle, engine, W, H, V, quantize, per_pass=False):
    st = photometric(pm, oracle, W, H, V, quantize)
    prior, mask = prior_planes(problem(pm, W, H, V, quantize)[0], W, H, np.random.default_rng(9))
    assert 0.45 < (mask > 0).mean() < 0.75
    prm = params(pm, W, H, V, quantize, max_scale=0)
    prm.planar_prior = True

    def run(h):
        start(h, st)
        h.set_prior(prior, mask)
        h.run(prm, SEED + 2)
        return state(h)

    want = wanted(("q8 prior", W, H, V, quantize), lambda: run(cpu_q8(pm, oracle, W, H, V, quantize)))
    assert_state(f"prior {W}x{H}, {V} views", run(gpu_q8(pm, engine, W, H, V, quantize, per_pass)), want)


@pytest.mark.parametrize("W,H,V,quantize", q8c.MATRIX)
def test_photometric_scales_2_1_0(pm, oracle, engine, W, H, V, quantize):
    check_photometric(pm, oracle, engine, W, H, V, quantize)


@pytest.mark.parametrize("W,H,V,quantize", q8c.MATRIX)
def test_geometric_run(pm, oracle, engine, W, H, V, quantize):
    check_geometric(pm, oracle, engine, W, H, V, quantize)


@pytest.mark.parametrize("W,H,V,quantize", q8c.MATRIX)
def test_planar_prior_run(pm, oracle, engine, W, H, V, quantize):
    check_prior(pm, oracle, engine, W, H, V, quantize)


@pytest.mark.parametrize("V,quantize", q8c.PER_PASS)
def test_one_launch_per_pass(pm, oracle, engine, V, quantize):
    """MPMVS_CHAIN=0: k_update receives one pass instead of up to six; gpu_handle asserts chain_status() == 0"""
    for check in (check_photometric, check_geometric, check_prior):
        check(pm, oracle, engine, 33, 17, V, quantize, per_pass=True)


# --- c: k_init at every scale -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("V,quantize,scale", q8c.INIT)
def test_init_at_each_scale(pm, oracle, engine, V, quantize, scale):
    """InitializeScore with random planes (photometric mode) and the window of `scale`: planes, costs, selected views"""
    W, H = 33, 17
    prm = params(pm, W, H, V, quantize, max_scale=2)
    cpu, gpu = cpu_q8(pm, oracle, W, H, V, quantize), gpu_q8(pm, engine, W, H, V, quantize)
    for h in (cpu, gpu):
        h.step(prm, SEED + 7, pm.KIND_INIT, 0, scale, 0)
    want = state(cpu)
    assert (want[1] < 2.0).mean() > 0.25 and (want[2] != 0).any()   # real costs and real selections are compared
    assert_state(f"init, {V} views, scale {scale}", state(gpu), want)


# --- d: the states at which the register form of the update can go wrong -------------------------------------------------------------

@pytest.mark.parametrize("V,quantize", q8c.STATES)
def test_depth_range_of_one_value(pm, oracle, engine, V, quantize):
    """every pixel holds a fronto-parallel plane at depth d, and depth_min == depth_max == d: nearly every candidate is out of range;
    one black and one red pass, compared after each"""
    W, H = 33, 17
    sc, cams, imgs, dmin, dmax = problem(pm, W, H, V, quantize)
    st = photometric(pm, oracle, W, H, V, quantize)
    d = np.float32(0.5 * (dmin + dmax))
    prm = pm.PatchMatchParams(num_images=V + 1, depth_min=float(d), depth_max=float(d), max_scale=0)
    cpu, gpu = cpu_q8(pm, oracle, W, H, V, quantize), gpu_q8(pm, engine, W, H, V, quantize)
    for h in (cpu, gpu):
        start(h, (one_plane(W, H, d), st[1], st[2]))
    for launch, kind in ((1, pm.KIND_BLACK), (2, pm.KIND_RED)):
        for h in (cpu, gpu):
            h.step(prm, SEED + 4, kind, 0, 0, launch)
        assert_state(f"one depth, {V} views, launch {launch}", state(gpu), state(cpu))


@pytest.mark.parametrize("V,quantize", q8c.STATES_PRIOR)
def test_masked_prior_with_restricted_cost_zero(pm, oracle, engine, V, quantize):
    """the prior is one fronto-parallel plane, every pixel holds it and every pixel is masked: restricted_cost stays 0 and each pass
    accepts the last in-range candidate with a valid prior term, whatever its cost.  A black and a red pass, each from that state."""
    W, H = 33, 17
    sc, cams, imgs, dmin, dmax = problem(pm, W, H, V, quantize)
    st = photometric(pm, oracle, W, H, V, quantize)
    planes = one_plane(W, H, np.float32(0.5 * (dmin + dmax)))
    mask = np.arange(1, H * W + 1, dtype=np.uint32).reshape(H, W)
    prm = params(pm, W, H, V, quantize, max_scale=0)
    prm.planar_prior = True
    cpu, gpu = cpu_q8(pm, oracle, W, H, V, quantize), gpu_q8(pm, engine, W, H, V, quantize)
    yy, xx = np.mgrid[0:H, 0:W]
    for launch, kind, parity in ((1, pm.KIND_BLACK, 0), (2, pm.KIND_RED, 1)):
        for h in (cpu, gpu):
            start(h, (planes, st[1], st[2]))
            h.set_prior(planes, mask)
            h.step(prm, SEED + 5, kind, 0, 0, launch)
        want = state(cpu)
        moved = (want[0].view(np.uint32) != planes.view(np.uint32)).any(-1)
        updated = ((xx + yy) & 1) == parity
        got = want[0][updated]
        # the state is the one meant: every pixel of the pass took its last candidate (the current normal at a depth perturbed by at most 2 %)
        assert not moved[~updated].any() and moved[updated].all()
        assert (got[:, :3] == planes[0, 0, :3]).all() and (np.abs(got[:, 3] / planes[0, 0, 3] - 1.0) < 0.0201).all()
        assert_state(f"restricted cost 0, {V} views, launch {launch}", state(gpu), want)


@pytest.mark.parametrize("V,quantize", q8c.STATES)
def test_blank_source_views(pm, oracle, engine, V, quantize):
    """the source views 2-7 of 8, and every repetition of them, hold one grey value: no texture, cost 2.0 against every plane"""
    W, H = 33, 17
    sc, cams, imgs, dmin, dmax = problem(pm, W, H, V, quantize)
    textured = [k for k in range(V) if k % 8 < 2]
    blank = [im if k == 0 or (k - 1) in textured else np.full_like(im, 128.0) for k, im in enumerate(imgs)]   # imgs[0] is the reference
    prm = params(pm, W, H, V, quantize, max_scale=0)
    cpu = cpu_q8(pm, oracle, W, H, V, quantize, blank)
    cpu.run(prm, SEED + 3)
    want = state(cpu)
    sel = want[2][: 2 * (H // 2)]   # the rows the checkerboard passes update
    chosen = np.array([int(((sel >> v) & 1).sum()) for v in range(V)])
    is_tex = np.array([v in textured for v in range(V)])
    assert 2 * chosen[~is_tex].max() < chosen[is_tex].min(), f"the blank views are meant to be left without weight mostly: {chosen.tolist()}"
    gpu = gpu_q8(pm, engine, W, H, V, quantize, imgs=blank)
    gpu.run(prm, SEED + 3)
    assert_state(f"blank views, {V} views", state(gpu), want)


# --- e: seeded sweep -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", range(int(os.environ.get("MPMVS_Q8_FUZZ_CASES", str(q8c.Q8_FUZZ_CASES)))))
def test_random_configuration_bit_exact(pm, oracle, engine, case):
    def make_cpu():
        cpu = oracle.create()
        oracle.set_texture_q8(cpu, True)
        return cpu
    fuzz_common.run_case(pm, lambda: engine.create_q8(0), make_cpu, case)


# --- f: tied fractions ---------------------------------------------------------------------------------------------------------------

def tie_handles(pm, oracle, engine, V, quantize):
    cams, imgs, prm = q8c.tie_problem(pm, V, quantize)
    cpu, gpu = oracle.create(), create_gpu(engine, q8=True)
    oracle.set_texture_q8(cpu, True)
    for h in (cpu, gpu):
        h.set_views(cams, imgs)
        q8c.assert_tie_homographies(h, V)   # on both sides, before anything relies on it
    assert gpu.texture_format() == ("u8" if quantize else "f32")
    return cpu, gpu, prm


@pytest.mark.parametrize("quantize", q8c.FORMATS)
@pytest.mark.parametrize("V", q8c.TIE_CONTEXTS)
def test_tied_fractions_eval_ncc(pm, oracle, engine, V, quantize):
    cpu, gpu, prm = tie_handles(pm, oracle, engine, V, quantize)
    groups = 0
    for scale in (0, 1, 2):
        for d in (3.0, 4.5):
            planes = q8c.tie_planes(d)
            want, got = cpu.eval_ncc(prm, planes, scale), gpu.eval_ncc(prm, planes, scale)
            assert (want == 2.0).mean() < 0.5
            assert same(got, want), f"{V} views, scale {scale}, depth {d}: {int((q8c.bits(got) != q8c.bits(want)).sum())} costs differ"
            groups += q8c.assert_tie_relations(got, V, quantize)   # on the GPU's result itself
    assert groups == 6 * {8: 2, 16: 4, 24: 8, 32: 10 if quantize else 8}[V]


@pytest.mark.parametrize("quantize", q8c.FORMATS)
def test_tied_fractions_photometric_run(pm, oracle, engine, quantize):
    cpu, gpu, prm = tie_handles(pm, oracle, engine, 32, quantize)
    for h in (cpu, gpu):
        h.run(prm, SEED + 8)
    assert_state("tied fractions, Run()", state(gpu), state(cpu))
