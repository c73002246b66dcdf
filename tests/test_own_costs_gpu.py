"""The per-view costs kept from InitializeScore (StateDev::own, mpmvs_dbg_own_costs): the first black and the first red update pass
after k_init read the photometric cost of the unchanged current plane back instead of evaluating it again.

Every comparison is bit for bit, three ways: the buffer in use, the buffer switched off (every pass recomputes) and the CPU oracle.
`passes_served` proves which path ran: 2 per Run() (or per INIT / BLACK / RED sequence at one window scale), 0 where the buffer is
switched off or no longer describes the planes.

Shapes: 72x33 (odd height: the reference's row limit 32 < H, the last row is initialised but never updated; 4.5 update blocks per
row), 40x56 (more block rows than columns, a partial last block in x and y) and 96x64 (whole 16x32 blocks, several 16x16 init blocks).
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 4321


def same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def state(h, geom=False):
    """planes, costs, (geometric costs,) selected views"""
    return tuple(h.get(geom=geom)) + (h.get_selected_views(),)


def assert_state(what, got, want):
    names = ("planes", "costs", "geom costs", "selected views") if len(want) == 4 else ("planes", "costs", "selected views")
    for n, g, w in zip(names, got, want):
        assert same(g, w), f"{what}: {n} differ on {int((np.asarray(g) != np.asarray(w)).sum())} values"


def make(pm, oracle, engine, W, H, V, quantize, per_pass=False):
    sc = pm.synth.make_problem_scene(W, H, n_src=min(V, 8), spacing=0.5, quantize=quantize)
    cams, imgs = sc.problem(0, [1 + (i % 8) for i in range(V)])
    if per_pass:
        os.environ["MPMVS_CHAIN"] = "0"
    try:
        gpu = engine.create(0)
    finally:
        os.environ.pop("MPMVS_CHAIN", None)
    cpu = oracle.create()
    for h in (gpu, cpu):
        h.set_views(cams, imgs)
    assert gpu.texture_format() == ("u8" if quantize else "f32")
    assert gpu.chain_status() == (0 if per_pass else 1)
    dmin, dmax = pm.synth.kernel_depth_range(cams[0])
    prm = pm.PatchMatchParams(num_images=V + 1, depth_min=float(dmin), depth_max=float(dmax), max_scale=0)
    return sc, gpu, cpu, prm


def run_on_and_off(gpu, prm, seed, before=None, geom=False):
    """Run() with the buffer in use and switched off, each from the state `before` sets up; returns both states and checks the counter"""
    out = []
    for enable, served in ((True, 2), (False, 0)):
        if before:
            before(gpu)
        n0 = gpu.dbg_own_costs(enable)
        gpu.run(prm, seed)
        assert gpu.dbg_own_costs() - n0 == served, f"passes served with enable={enable}"
        out.append(state(gpu, geom))
    gpu.dbg_own_costs(True)
    return out


# V = 3: the view_w[candidate] quirk below 5 views; V = 8: the full MAXV = 8 kernels; V = 9: the MAXV = 16 kernels.
# quantize: 8-bit images (fp16 texels) / non-integer images (fp32 texels).  max_scale 2: only the two first scale-2 passes are served.
@pytest.mark.parametrize("per_pass", [False, True])
@pytest.mark.parametrize("W,H,V,max_scale,quantize", [(72, 33, 3, 0, True), (40, 56, 8, 2, True), (96, 64, 9, 0, False), (96, 64, 8, 0, False),
                                                      (72, 33, 9, 2, True), (40, 56, 3, 2, False)])
def test_photometric_run(pm, oracle, engine, W, H, V, max_scale, quantize, per_pass):
    sc, gpu, cpu, prm = make(pm, oracle, engine, W, H, V, quantize, per_pass)
    prm.max_scale = max_scale
    cpu.run(prm, SEED)
    want = state(cpu)
    on, off = run_on_and_off(gpu, prm, SEED)
    assert_state("buffer on vs oracle", on, want)
    assert_state("buffer off vs oracle", off, want)


def src_depths(sc, V, W, H, rng):
    return [sc.views[1 + (i % 8)].gt_depth * (1.0 + 0.005 * rng.standard_normal((H, W))).astype(np.float32) for i in range(V)]


@pytest.mark.parametrize("W,H,V,quantize", [(96, 64, 3, True), (72, 33, 9, False)])
def test_geometric_run(pm, oracle, engine, W, H, V, quantize):
    sc, gpu, cpu, prm = make(pm, oracle, engine, W, H, V, quantize)
    cpu.run(prm, SEED)
    p0, c0 = cpu.get()
    s0 = cpu.get_selected_views()
    depths = src_depths(sc, V, W, H, np.random.default_rng(7))
    for h in (gpu, cpu):
        h.set_src_depths(depths)
    prm.geom_consistency, prm.max_iterations = True, 2

    def before(h):
        h.set_state(p0, c0)
        h.set_selected_views(s0)

    before(cpu)
    cpu.run(prm, SEED + 1)
    want = state(cpu, geom=True)
    on, off = run_on_and_off(gpu, prm, SEED + 1, before, geom=True)
    assert_state("geometric, buffer on vs oracle", on, want)
    assert_state("geometric, buffer off vs oracle", off, want)


@pytest.mark.parametrize("W,H,V,quantize", [(96, 64, 3, False), (40, 56, 9, True)])
def test_planar_prior_run(pm, oracle, engine, W, H, V, quantize):
    sc, gpu, cpu, prm = make(pm, oracle, engine, W, H, V, quantize)
    cpu.run(prm, SEED)
    p0, c0 = cpu.get()
    s0 = cpu.get_selected_views()
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
    prm.planar_prior = True

    def before(h):
        h.set_state(p0, c0)
        h.set_selected_views(s0)
        h.set_prior(prior, mask)

    before(cpu)
    cpu.run(prm, SEED + 2)
    want = state(cpu)
    on, off = run_on_and_off(gpu, prm, SEED + 2, before)
    assert_state("prior, buffer on vs oracle", on, want)
    assert_state("prior, buffer off vs oracle", off, want)


def steps(h, prm, seed, seq):
    """seq of (kind, iteration, scale): launch ids count up from 0"""
    for launch, (kind, it, scale) in enumerate(seq):
        h.step(prm, seed, kind, it, scale, launch)


@pytest.mark.parametrize("W,H,V,scale,quantize", [(72, 33, 3, 0, True), (96, 64, 8, 1, False), (40, 56, 9, 2, True)])
def test_run_schedule_through_step(pm, oracle, engine, W, H, V, scale, quantize):
    """INIT and two iterations of black / red passes, one mpmvs_step each, compared after every launch"""
    sc, gpu, cpu, prm = make(pm, oracle, engine, W, H, V, quantize)
    prm.max_scale = scale
    seq = [(pm.KIND_INIT, 0, scale)] + [(k, it, scale) for it in range(2) for k in (pm.KIND_BLACK, pm.KIND_RED)]
    want = []
    for launch, (kind, it, s) in enumerate(seq):
        cpu.step(prm, SEED, kind, it, s, launch)
        want.append(state(cpu))
    for enable, served in ((True, [0, 1, 2, 2, 2]), (False, [0] * 5)):
        n0 = gpu.dbg_own_costs(enable)
        for launch, (kind, it, s) in enumerate(seq):
            gpu.step(prm, SEED, kind, it, s, launch)
            assert gpu.dbg_own_costs() - n0 == served[launch], f"enable={enable}, launch {launch}"
            assert_state(f"enable={enable}, launch {launch}", state(gpu), want[launch])


def check_sequence(pm, gpu, cpu, prm, seq, served, mid=None):
    """the same launches on both sides (mid(h) between the first launch and the rest), the state compared at the end"""
    n0 = gpu.dbg_own_costs(True)
    for h in (gpu, cpu):
        h.step(prm, SEED, *seq[0], 0)
        if mid:
            mid(h)
        for launch, (kind, it, scale) in enumerate(seq[1:], 1):
            h.step(prm, SEED, kind, it, scale, launch)
    assert gpu.dbg_own_costs() - n0 == served
    assert_state("sequence", state(gpu), state(cpu))


@pytest.mark.parametrize("W,H,V,quantize", [(72, 33, 3, True), (96, 64, 8, False)])
def test_invalidation_by_scale_and_by_a_second_pass(pm, oracle, engine, W, H, V, quantize):
    sc, gpu, cpu, prm = make(pm, oracle, engine, W, H, V, quantize)
    prm.max_scale = 1
    # costs evaluated with the scale-1 window say nothing about the scale-0 window
    check_sequence(pm, gpu, cpu, prm, [(pm.KIND_INIT, 0, 1), (pm.KIND_BLACK, 0, 0)], served=0)
    # the second black pass finds planes the first one wrote: it recomputes
    check_sequence(pm, gpu, cpu, prm, [(pm.KIND_INIT, 0, 1), (pm.KIND_BLACK, 0, 1), (pm.KIND_BLACK, 0, 1)], served=1)
    # red after black is still served (the black pass wrote black pixels only), a second red pass is not
    check_sequence(pm, gpu, cpu, prm, [(pm.KIND_INIT, 0, 0), (pm.KIND_BLACK, 0, 0), (pm.KIND_RED, 0, 0), (pm.KIND_RED, 1, 0)], served=2)


@pytest.mark.parametrize("W,H,V,quantize", [(40, 56, 3, True), (96, 64, 9, False)])
def test_invalidation_by_set_state(pm, oracle, engine, W, H, V, quantize):
    """INIT, then other planes through set_state, then RED: the red pass must evaluate the planes it finds"""
    sc, gpu, cpu, prm = make(pm, oracle, engine, W, H, V, quantize)
    cpu.step(prm, SEED, pm.KIND_INIT, 0, 0, 0)
    p0, c0 = cpu.get()
    perturbed = np.ascontiguousarray(np.roll(p0, (3, 5), axis=(0, 1)))   # every pixel gets the plane of another one

    def mid(h):
        h.set_state(perturbed, c0)

    check_sequence(pm, gpu, cpu, prm, [(pm.KIND_INIT, 0, 0), (pm.KIND_RED, 0, 0)], served=0, mid=mid)


def test_back_to_back_runs(pm, oracle, engine):
    """two Run()s on one context with different seeds, blocking and pipelined: the second k_init rewrites the buffer behind the
    first chain, and each Run() is served its own two passes"""
    import torch
    W, H, V = 96, 64, 8
    sc, gpu, cpu, prm = make(pm, oracle, engine, W, H, V, True)
    prm.max_scale = 1
    want = []
    for seed in (SEED, SEED + 1):
        cpu.run(prm, seed)
        want.append(cpu.get())
    bufs = [tuple(torch.empty(shape, dtype=torch.float32, pin_memory=True).numpy() for shape in ((H, W, 4), (H, W))) for _ in range(4)]
    n0 = gpu.dbg_own_costs(True)
    for k, seed in enumerate((SEED, SEED + 1)):
        gpu.run_into(prm, seed, *bufs[k])
    assert gpu.dbg_own_costs() - n0 == 4
    for k, seed in enumerate((SEED, SEED + 1)):
        gpu.run_into_async(prm, seed, *bufs[2 + k])
    gpu.wait()
    assert gpu.dbg_own_costs() - n0 == 8
    for k in range(4):
        assert same(bufs[k][0], want[k % 2][0]) and same(bufs[k][1], want[k % 2][1]), f"run {k}"
