"""The bookkeeping of the update kernel around its evaluations (update_body, csrc/pm_kernels.hpp): the cost matrix of phase A lies
[view][candidate] in private memory, the weighted candidate costs are formed view by view from one batch of loads per view (under a
per-lane select on the view's weight; the planar prior with 9-16 views keeps the candidate-by-candidate loop), the geometric variants
fetch a view's eight costs ahead of its depth gathers, and the dealt rounds of the refinement publish, evaluate and collect around them.
None of this may change a bit: planes, costs, selected views and geometric costs are compared with the CPU oracle, bit for bit, every
pixel.

Sizes: 48x40 (three block columns, several block rows, waves with 24 .. 64 pixels), 33x17 (a last column and a last row with one
pixel: waves whose lanes mostly have no pixel, n_here < 64; the reference's row limit 16 < H) and 16x8 (exactly one wave).
View counts: 1, 3 (the geometric term of the refinement reads view_w[candidate] beyond V), 8 (the MAXV = 8 kernels) and 9 (MAXV = 16).
Modes: a photometric Run() with max_scale 2 (its launches run the window scales 2, 1 and 0), a geometric Run() and a planar-prior
Run() with masked pixels, the last two from the photometric result.  Texel formats: 8-bit images (fp16 texels) and non-integer images
(fp32 texels).  Launches: chained, and one launch per pass (MPMVS_CHAIN=0).  Every size, view count and format meets every mode in
the chained launch; one launch per pass differs from it in the launch alone (k_update receives one pass instead of six, the body is
the same code), so it runs all photometric cases and, of the geometric and prior ones, both formats at the two sizes with partial
waves and at the view counts 3 and 9.
Two further states: source views 2-7 blank (their costs are 2.0, the views get weight 0, rounds publish for few candidates), and a
state of fronto-parallel planes at one depth with depth_min == depth_max == that depth (nearly every refinement candidate is out of
range: empty rounds, and views without a single item).
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 2207
SIZES = [(48, 40), (33, 17), (16, 8)]
VIEWS = [1, 3, 8, 9]
CASES = [(W, H, V, q) for (W, H) in SIZES for V in VIEWS for q in (True, False)]
# (W, H, V, quantize, per_pass) of the geometric and the prior runs
MODE_CASES = [c + (False,) for c in CASES] + [(48, 40, 3, True, True), (48, 40, 9, False, True), (33, 17, 9, True, True), (33, 17, 3, False, True)]


def same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def state(h, geom=False):
    """planes, costs, (geometric costs,) selected views"""
    return tuple(np.array(a) for a in h.get(geom=geom)) + (np.array(h.get_selected_views()),)


def assert_state(what, got, want):
    names = ("planes", "costs", "geom costs", "selected views") if len(want) == 4 else ("planes", "costs", "selected views")
    for n, g, w in zip(names, got, want):
        assert same(g, w), f"{what}: {n} differ on {int((np.asarray(g).view(np.uint32) != np.asarray(w).view(np.uint32)).sum())} values"


_scenes = {}


def problem(pm, W, H, V, quantize):
    key = (W, H, V, quantize)
    if key not in _scenes:
        sc = pm.synth.make_problem_scene(W, H, n_src=min(V, 8), spacing=0.5, quantize=quantize)
        cams, imgs = sc.problem(0, [1 + (i % 8) for i in range(V)])
        dmin, dmax = pm.synth.kernel_depth_range(cams[0])
        _scenes[key] = (sc, cams, imgs, float(dmin), float(dmax))
    return _scenes[key]


def params(pm, W, H, V, quantize, **kw):
    sc, cams, imgs, dmin, dmax = problem(pm, W, H, V, quantize)
    return pm.PatchMatchParams(num_images=V + 1, depth_min=dmin, depth_max=dmax, **kw)


def cpu_handle(pm, oracle, W, H, V, quantize, imgs=None):
    sc, cams, own, dmin, dmax = problem(pm, W, H, V, quantize)
    cpu = oracle.create()
    cpu.set_views(cams, own if imgs is None else imgs)
    return cpu


def gpu_handle(pm, engine, W, H, V, quantize, per_pass=False, imgs=None):
    sc, cams, own, dmin, dmax = problem(pm, W, H, V, quantize)
    if per_pass:
        os.environ["MPMVS_CHAIN"] = "0"
    try:
        gpu = engine.create(0)
    finally:
        os.environ.pop("MPMVS_CHAIN", None)
    gpu.set_views(cams, own if imgs is None else imgs)
    assert gpu.texture_format() == ("u8" if quantize else "f32")
    assert gpu.chain_status() == (0 if per_pass else 1)
    return gpu


_wanted = {}


def wanted(key, compute):
    """the oracle's result of a case: computed once, shared by the launch modes, never written to"""
    if key not in _wanted:
        _wanted[key] = compute()
        for a in _wanted[key]:
            a.setflags(write=False)
    return _wanted[key]


def photometric(pm, oracle, W, H, V, quantize):
    def compute():
        cpu = cpu_handle(pm, oracle, W, H, V, quantize)
        cpu.run(params(pm, W, H, V, quantize, max_scale=2), SEED)
        return state(cpu)
    return wanted(("photo", W, H, V, quantize), compute)


@pytest.mark.parametrize("per_pass", [False, True])
@pytest.mark.parametrize("W,H,V,quantize", CASES)
def test_photometric_scales_2_1_0(pm, oracle, engine, W, H, V, quantize, per_pass):
    want = photometric(pm, oracle, W, H, V, quantize)
    gpu = gpu_handle(pm, engine, W, H, V, quantize, per_pass)
    gpu.run(params(pm, W, H, V, quantize, max_scale=2), SEED)
    assert_state(f"{W}x{H}, {V} views", state(gpu), want)


def start(h, st):
    h.set_state(st[0], st[1])
    h.set_selected_views(st[2])


@pytest.mark.parametrize("W,H,V,quantize,per_pass", MODE_CASES)
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


def prior_planes(sc, W, H, rng):
    """planes close to the ground truth, and a mask that covers 60 % of the pixels"""
    cam, gt = sc.views[0].cam, sc.views[0].gt_depth.astype(np.float64)
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    X = np.stack([gt * (u - cam.K[2]) / cam.K[0], gt * (v - cam.K[5]) / cam.K[4], gt], -1)
    n = np.zeros((H, W, 3))
    n[..., 2] = -1.0
    n[..., 0] = 0.05 * rng.standard_normal((H, W))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    prior = np.concatenate([n, -(n * X).sum(-1)[..., None]], -1).astype(np.float32)
    mask = (rng.uniform(size=(H, W)) < 0.6).astype(np.uint32) * np.arange(1, H * W + 1, dtype=np.uint32).reshape(H, W)
    return prior, mask


@pytest.mark.parametrize("W,H,V,quantize,per_pass", MODE_CASES)
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


@pytest.mark.parametrize("quantize", [True, False])
def test_blank_source_views(pm, oracle, engine, quantize):
    """source views 2-7 of 8 hold one grey value: no texture, cost 2.0 against every plane"""
    W, H, V = 48, 40, 8
    sc, cams, imgs, dmin, dmax = problem(pm, W, H, V, quantize)
    blank = [im if k < 3 else np.full_like(im, 128.0) for k, im in enumerate(imgs)]   # imgs[0] is the reference, imgs[1 + k] source view k
    prm = params(pm, W, H, V, quantize, max_scale=0)
    cpu = cpu_handle(pm, oracle, W, H, V, quantize, blank)
    cpu.run(prm, SEED + 3)
    want = state(cpu)
    sel = want[2][: 2 * (H // 2)]   # the rows the checkerboard passes update
    chosen = [int(((sel >> v) & 1).sum()) for v in range(V)]
    assert 2 * max(chosen[2:]) < min(chosen[:2]), f"the blank views are meant to be left without weight mostly: {chosen}"
    gpu = gpu_handle(pm, engine, W, H, V, quantize, imgs=blank)
    gpu.run(prm, SEED + 3)
    assert_state("blank views 2-7", state(gpu), want)


@pytest.mark.parametrize("quantize", [True, False])
def test_depth_range_of_one_value(pm, oracle, engine, quantize):
    """every pixel holds a fronto-parallel plane at depth d, and depth_min == depth_max == d: a candidate survives the range test only
    where its depth comes back as exactly d; one black and one red pass, compared after each"""
    W, H, V = 48, 40, 8
    sc, cams, imgs, dmin, dmax = problem(pm, W, H, V, quantize)
    st = photometric(pm, oracle, W, H, V, quantize)
    d = np.float32(0.5 * (dmin + dmax))
    planes = np.zeros((H, W, 4), np.float32)
    planes[..., 2], planes[..., 3] = -1.0, d
    prm = pm.PatchMatchParams(num_images=V + 1, depth_min=float(d), depth_max=float(d), max_scale=0)
    cpu, gpu = cpu_handle(pm, oracle, W, H, V, quantize), gpu_handle(pm, engine, W, H, V, quantize)
    for h in (cpu, gpu):
        start(h, (planes, st[1], st[2]))
    for launch, kind in ((1, pm.KIND_BLACK), (2, pm.KIND_RED)):
        for h in (cpu, gpu):
            h.step(prm, SEED + 4, kind, 0, 0, launch)
        assert_state(f"one depth, launch {launch}", state(gpu), state(cpu))
