"""Scenes, handles and comparisons shared by the files that run the update kernel's variants against the CPU oracle bit for bit
(tests/test_refine_planes_gpu.py for the default build, tests/test_q8_variants_gpu.py for the build with 8-bit interpolation
fractions), and the map from a configuration to the kernel instantiation that serves it."""
import os

import numpy as np

BUCKETS = (8, 16, 24, 32)          # bounds on the number of source views the NCC kernels are instantiated for (mpmvs_api.hip, dispatch_variant)
MODES = ("photometric", "geometric", "prior")


def bucket_of(V):
    assert 1 <= V <= BUCKETS[-1]
    return next(b for b in BUCKETS if V <= b)


def variant_of(V, quantize, mode, scale):
    """(mode, bucket, u8, scale): the k_update instantiation that launch_update picks for V source views, the texel format (8-bit exact
    images take fp16 texels) and the window scale; the geometric and the planar-prior update exist at scale 0 only"""
    assert mode in MODES and scale in (0, 1, 2)
    if mode != "photometric" and scale != 0:
        raise ValueError(f"the {mode} update runs at scale 0 only")
    return (mode, bucket_of(V), bool(quantize), scale)


def init_variant_of(V, quantize, scale):
    """(bucket, u8, scale): the k_init instantiation"""
    assert scale in (0, 1, 2)
    return (bucket_of(V), bool(quantize), scale)


ALL_UPDATE_VARIANTS = frozenset(variant_of(b, u8, m, s) for b in BUCKETS for u8 in (True, False) for m in MODES
                                for s in ((0, 1, 2) if m == "photometric" else (0,)))
ALL_INIT_VARIANTS = frozenset(init_variant_of(b, u8, s) for b in BUCKETS for u8 in (True, False) for s in (0, 1, 2))


def run_variants(V, quantize, mode, max_scale):
    """(update variants, init variants) that one Run() launches: InitializeScore at max_scale in every mode, then the photometric
    passes at max_scale .. 0 or the geometric / prior passes at scale 0 (mpmvs_api.hip, enqueue_updates)"""
    scales = range(max_scale, -1, -1) if mode == "photometric" else (0,)
    return {variant_of(V, quantize, mode, s) for s in scales}, {init_variant_of(V, quantize, max_scale)}


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
        sc = pm.synth.make_problem_scene(W, H, n_src=8, spacing=0.5, quantize=quantize)
        cams, imgs = sc.problem(0, [1 + (i % 8) for i in range(V)])
        dmin, dmax = pm.synth.kernel_depth_range(cams[0])
        _scenes[key] = (sc, cams, imgs, float(dmin), float(dmax))
    return _scenes[key]


def params(pm, W, H, V, quantize, **kw):
    sc, cams, imgs, dmin, dmax = problem(pm, W, H, V, quantize)
    return pm.PatchMatchParams(num_images=V + 1, depth_min=dmin, depth_max=dmax, **kw)


def cpu_handle(pm, oracle, W, H, V, quantize, imgs=None, q8=False):
    sc, cams, own, dmin, dmax = problem(pm, W, H, V, quantize)
    cpu = oracle.create()
    if q8:
        oracle.set_texture_q8(cpu, True)
    cpu.set_views(cams, own if imgs is None else imgs)
    return cpu


def create_gpu(engine, per_pass=False, q8=False):
    """a context of the default build or of its twin; per_pass: one launch per update pass (MPMVS_CHAIN=0, read when the context is made)"""
    if per_pass:
        os.environ["MPMVS_CHAIN"] = "0"
    try:
        gpu = engine.create_q8(0) if q8 else engine.create(0)
    finally:
        os.environ.pop("MPMVS_CHAIN", None)
    assert gpu.chain_status() == (0 if per_pass else 1)
    return gpu


def gpu_handle(pm, engine, W, H, V, quantize, per_pass=False, imgs=None, q8=False):
    sc, cams, own, dmin, dmax = problem(pm, W, H, V, quantize)
    gpu = create_gpu(engine, per_pass, q8)
    gpu.set_views(cams, own if imgs is None else imgs)
    assert gpu.texture_format() == ("u8" if quantize else "f32")
    assert gpu.chain_status() == (0 if per_pass else 1)
    return gpu


_wanted = {}


def wanted(key, compute):
    """the oracle's result of a case: computed once, shared by the tests and launch modes that need it, never written to"""
    if key not in _wanted:
        _wanted[key] = compute()
        for a in _wanted[key]:
            a.setflags(write=False)
    return _wanted[key]


def start(h, st):
    h.set_state(st[0], st[1])
    h.set_selected_views(st[2])


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


def one_plane(W, H, d):
    planes = np.zeros((H, W, 4), np.float32)
    planes[..., 2], planes[..., 3] = -1.0, d
    return planes
