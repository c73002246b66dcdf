"""The banded end of Run() (mpmvs_api.hip, enqueue_band_tail): with page-locked output buffers mpmvs_run_get runs
GetDepthandNormal, the median filter and the device-to-host copies band by band while the last update pass still runs.
Every map must be the bits of the whole-image tail -- mpmvs_run + mpmvs_get on a context with the same history -- for odd
sizes, tiny images, every Run() mode, both texture formats, any subset of the outputs and two contexts back to back."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 777


class Pinned:
    """page-locked float32 arrays from the library's pinned pool (mpmvs_alloc_pinned)"""

    def __init__(self, engine):
        self._f = engine.load()[1]
        self._ptrs = []

    def array(self, shape):
        n = int(np.prod(shape))
        ptr = self._f["alloc_pinned"](n * 4)
        assert ptr, "mpmvs_alloc_pinned failed"
        self._ptrs.append(ptr)
        a = np.ctypeslib.as_array((C.c_float * n).from_address(ptr)).reshape(shape)
        a.fill(np.nan)
        return a

    def free(self):
        for p in self._ptrs:
            self._f["free_pinned"](p)
        self._ptrs = []


@pytest.fixture
def pinned(engine):
    p = Pinned(engine)
    yield p
    p.free()


def bits_equal(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def run_get(h, prm, seed, planes=None, costs=None, geom=None):
    """mpmvs_run_get with any subset of the outputs"""
    ptr = lambda a: a.ctypes.data if a is not None else None
    h._chk(h._f["run_get"](h._ctx, C.byref(prm), int(seed), ptr(planes), ptr(costs), ptr(geom)), "run_get")


def scene(pm, W, H, V, quantize=True):
    sc = pm.synth.make_problem_scene(W, H, n_src=V, spacing=0.5, quantize=quantize)
    cams, imgs = sc.problem(0, list(range(1, V + 1)))
    dmin, dmax = (float(v) for v in pm.synth.kernel_depth_range(cams[0]))
    return sc, cams, imgs, dmin, dmax


def pair(engine, cams, imgs, fp32=False):
    """two contexts with the same inputs: the banded one and the whole-image reference"""
    hs = [engine.create(0), engine.create(0)]
    for h in hs:
        if fp32:
            h.set_texture_format(True)
        h.set_views(cams, imgs)
    assert hs[0].chain_status() == 1, "the banded end needs the chained launch"
    return hs


def bands_of(H):
    """the steps (one GetDepthandNormal launch each) of enqueue_band_tail for an image of H rows: bands of a multiple of 32 rows
    (kTailBands = 12); the step whose wait covers every band counter takes the rest of the image"""
    bh = 32 * max(1, (H + 16 * 12) // (32 * 12))
    rows = min(H, 32 * ((H // 2 + 15) // 16))
    groups, gpb = (rows + 7) // 8, bh // 8
    for s in range(1, (H + bh - 1) // bh + 1):
        need = min(groups, (min(H, s * bh) + 22) // 8 + 1)
        if (need + gpb - 1) // gpb * gpb >= groups:
            return s
    return (H + bh - 1) // bh


def check_banded(pm, h, ref, prm, seed, pinned, outputs=("planes", "costs", "geom")):
    W, H = h.W, h.H
    out = {"planes": pinned.array((H, W, 4)) if "planes" in outputs else None,
           "costs": pinned.array((H, W)) if "costs" in outputs else None,
           "geom": pinned.array((H, W)) if "geom" in outputs else None}
    h.set_profiling(True)
    run_get(h, prm, seed, out["planes"], out["costs"], out["geom"])
    _, cnt = h.kernel_times()
    h.set_profiling(False)
    # one GetDepthandNormal launch per band: the maps came through the banded end, not the whole-image tail
    assert cnt[pm.KIND_DEPTH_NORMAL] == bands_of(H), cnt
    ref.run(prm, seed)
    want = dict(zip(("planes", "costs", "geom"), ref.get(geom=True)))
    for name in outputs:
        assert bits_equal(out[name], want[name]), f"{name}: {int((out[name] != want[name]).sum())} values differ"
    return want


@pytest.mark.parametrize("W,H", [(400, 301), (96, 20)])
def test_photometric_odd_and_tiny_sizes(pm, engine, pinned, W, H):
    """heights that are no multiple of the band (32 rows) nor of the block height; fewer block rows than bands"""
    _, cams, imgs, dmin, dmax = scene(pm, W, H, 4)
    prm = pm.PatchMatchParams(num_images=5, depth_min=dmin, depth_max=dmax, max_scale=1, max_iterations=3)
    a, b = pair(engine, cams, imgs)
    for k in range(3):   # the band counters only grow from Run() to Run()
        check_banded(pm, a, b, prm, SEED + k, pinned)


def test_banded_equals_oracle(pm, oracle, engine, pinned):
    W, H = 120, 77
    _, cams, imgs, dmin, dmax = scene(pm, W, H, 3)
    prm = pm.PatchMatchParams(num_images=4, depth_min=dmin, depth_max=dmax, max_scale=1)
    h = engine.create(0)
    h.set_views(cams, imgs)
    planes, costs = pinned.array((H, W, 4)), pinned.array((H, W))
    run_get(h, prm, SEED, planes, costs)
    cpu = oracle.create()
    cpu.set_views(cams, imgs)
    cpu.run(prm, SEED)
    cp, cc = cpu.get()
    assert np.array_equal(planes, cp, equal_nan=True) and np.array_equal(costs, cc, equal_nan=True)


@pytest.mark.parametrize("outputs", [("planes",), ("costs",), ("geom",), ("planes", "costs"), ("planes", "costs", "geom")])
def test_output_subsets(pm, engine, pinned, outputs):
    _, cams, imgs, dmin, dmax = scene(pm, 333, 250, 4)
    prm = pm.PatchMatchParams(num_images=5, depth_min=dmin, depth_max=dmax, max_scale=0)
    a, b = pair(engine, cams, imgs)
    check_banded(pm, a, b, prm, SEED, pinned, outputs)


def test_fp32_textures(pm, engine, pinned):
    _, cams, imgs, dmin, dmax = scene(pm, 320, 263, 4, quantize=False)
    prm = pm.PatchMatchParams(num_images=5, depth_min=dmin, depth_max=dmax, max_scale=1)
    a, b = pair(engine, cams, imgs, fp32=True)
    assert a.texture_format() == "f32"
    check_banded(pm, a, b, prm, SEED, pinned)


def test_geometric_and_planar_prior_runs(pm, engine, pinned):
    """the flow of ProcessProblem: photometric, geometric (source depth maps), then planar prior -- with the geom output"""
    W, H, V = 300, 233, 4
    sc, cams, imgs, dmin, dmax = scene(pm, W, H, V)
    a, b = pair(engine, cams, imgs)
    prm = pm.PatchMatchParams(num_images=V + 1, depth_min=dmin, depth_max=dmax, max_scale=1)
    want = check_banded(pm, a, b, prm, SEED, pinned)
    rng = np.random.default_rng(3)
    depths = [(sc.views[i].gt_depth * (1 + 0.01 * rng.standard_normal((H, W)))).astype(np.float32) for i in range(1, V + 1)]
    for h in (a, b):
        h.set_src_depths(depths)
    prm.geom_consistency, prm.max_iterations, prm.geomPlanarPrior = True, 2, True
    want = check_banded(pm, a, b, prm, SEED + 1, pinned)
    prior = want["planes"].copy()
    mask = (want["costs"] < 0.6).astype(np.uint32)
    for h in (a, b):
        h.set_prior(prior, mask)
    prm.geom_consistency, prm.planar_prior, prm.max_iterations = False, True, 3
    check_banded(pm, a, b, prm, SEED + 2, pinned)


def test_two_contexts_back_to_back(pm, engine, pinned):
    """two banded contexts of different sizes on one device, alternating: each waits only for its own counters"""
    sets = []
    for W, H in ((256, 200), (180, 131)):
        _, cams, imgs, dmin, dmax = scene(pm, W, H, 4)
        prm = pm.PatchMatchParams(num_images=5, depth_min=dmin, depth_max=dmax, max_scale=1)
        sets.append((pair(engine, cams, imgs), prm))
    for k in range(3):
        for (a, b), prm in sets:
            check_banded(pm, a, b, prm, SEED + 10 * k, pinned)
