"""ctypes view of the reference's own device code compiled for the host (oracle/ref_driver.cpp, `make -C oracle ref`):
oracle/_ref/libmpmvs_ref.so (IEEE operations as written) and libmpmvs_ref_fma.so (the same text with contracted multiply-adds).

The libraries are build products of __graft_entry__.build() on a machine that holds the reference tree; they travel with the
working tree to machines that do not.  A missing library is an error, never a skip.  Shared by tests/test_reference_cpu.py and
tests/test_reference_gpu.py, together with the scenes, plane sets and draw tables both use."""
import ctypes as C
import importlib
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
_abi = importlib.import_module("mp-mvs_amd._abi")
_P = C.c_void_p
_FPP = C.POINTER(C.POINTER(C.c_float))
_PRM = C.POINTER(_abi.PatchMatchParams)
DRAW_CAP = 96     # uniforms per pixel and launch handed to the reference's code (most ever consumed on the scenes here: 36)
_cache = {}


def lib(fma=False):
    name = "libmpmvs_ref_fma.so" if fma else "libmpmvs_ref.so"
    if name not in _cache:
        path = os.path.join(ORACLE_DIR, "_ref", name)
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: __graft_entry__.build() makes it where the reference tree is present (MPMVS_REFERENCE)")
        l = C.CDLL(path)
        l.ref_create.restype = _P
        l.ref_create.argtypes = [C.c_int, C.POINTER(_abi.Camera), _FPP, C.c_int]
        l.ref_destroy.argtypes = [_P]
        l.ref_set_src_depths.argtypes = [_P, _FPP, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]
        l.ref_set_prior.argtypes = [_P, _P, _P]
        l.ref_set_state.argtypes = [_P, _P, _P, _P]
        l.ref_get.argtypes = [_P, _P, _P, _P, _P]
        l.ref_homography.argtypes = [_P, _P, C.c_int, _P]
        l.ref_eval_ncc.argtypes = [_P, _PRM, _P, C.c_int, _P]
        l.ref_eval_geom.restype = C.c_int
        l.ref_eval_geom.argtypes = [_P, _PRM, _P, _P]
        l.ref_eval_initial.argtypes = [_P, _PRM, _P, C.c_int, _P, _P]
        l.ref_launch.restype = C.c_int
        l.ref_launch.argtypes = [_P, _PRM, C.c_int, C.c_int, C.c_int, _P, C.c_int]
        l.ref_sky_bilateral.argtypes = [_P, _P, _P, C.c_int, C.c_int]
        _cache[name] = l
    return _cache[name]


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


class Reference:
    """one problem (reference view + source views) on the compiled reference; q8 = CUDA's 8-bit interpolation fractions"""

    def __init__(self, cams, images, q8=False, fma=False):
        self._l = lib(fma)
        n = len(cams)
        imgs = [_f32(im) for im in images]
        for cam, im in zip(cams, imgs):
            assert im.shape == (cam.height, cam.width)
        ptrs = (C.POINTER(C.c_float) * n)(*[im.ctypes.data_as(C.POINTER(C.c_float)) for im in imgs])
        self._q8 = 1 if q8 else 0
        self._ctx = self._l.ref_create(n, (_abi.Camera * n)(*cams), ptrs, self._q8)
        self.n_img, (self.H, self.W) = n, imgs[0].shape

    def __del__(self):
        if getattr(self, "_ctx", None):
            self._l.ref_destroy(self._ctx)
            self._ctx = None

    def set_src_depths(self, depths):
        ds = [_f32(d) for d in depths]
        n = len(ds)
        assert n == self.n_img - 1
        ptrs = (C.POINTER(C.c_float) * n)(*[d.ctypes.data_as(C.POINTER(C.c_float)) for d in ds])
        self._l.ref_set_src_depths(self._ctx, ptrs, (C.c_int * n)(*[d.shape[1] for d in ds]), (C.c_int * n)(*[d.shape[0] for d in ds]), self._q8)

    def set_prior(self, prior, mask):
        p, m = _f32(prior), np.ascontiguousarray(mask, np.uint32)
        assert p.shape == (self.H, self.W, 4) and m.shape == (self.H, self.W)
        self._l.ref_set_prior(self._ctx, p.ctypes.data, m.ctypes.data)

    def set_state(self, planes=None, costs=None, sel=None):
        p = _f32(planes) if planes is not None else None
        c = _f32(costs) if costs is not None else None
        s = np.ascontiguousarray(sel, np.uint32) if sel is not None else None
        self._l.ref_set_state(self._ctx, *(a.ctypes.data if a is not None else None for a in (p, c, s)))

    def get(self):
        """(planes, costs, selected views, geometric costs)"""
        planes, costs = np.empty((self.H, self.W, 4), np.float32), np.empty((self.H, self.W), np.float32)
        sel, geom = np.empty((self.H, self.W), np.uint32), np.empty((self.H, self.W), np.float32)
        self._l.ref_get(self._ctx, planes.ctypes.data, costs.ctypes.data, sel.ctypes.data, geom.ctypes.data)
        return planes, costs, sel, geom

    def homography(self, plane, v):
        p, out = _f32(plane).reshape(4), np.empty(9, np.float32)
        self._l.ref_homography(self._ctx, p.ctypes.data, int(v), out.ctypes.data)
        return out.reshape(3, 3)

    def eval_ncc(self, prm, planes, scale):
        p = _f32(planes)
        assert p.shape == (self.H, self.W, 4)
        out = np.empty((prm.num_images - 1, self.H, self.W), np.float32)
        self._l.ref_eval_ncc(self._ctx, C.byref(prm), p.ctypes.data, int(scale), out.ctypes.data)
        return out

    def eval_geom(self, prm, planes):
        p = _f32(planes)
        out = np.empty((prm.num_images - 1, self.H, self.W), np.float32)
        if self._l.ref_eval_geom(self._ctx, C.byref(prm), p.ctypes.data, out.ctypes.data) != 0:
            raise RuntimeError("ref_eval_geom needs source depth maps")
        return out

    def eval_initial(self, prm, planes, scale):
        p = _f32(planes)
        costs, sel = np.empty((self.H, self.W), np.float32), np.empty((self.H, self.W), np.uint32)
        self._l.ref_eval_initial(self._ctx, C.byref(prm), p.ctypes.data, int(scale), costs.ctypes.data, sel.ctypes.data)
        return costs, sel

    def launch(self, prm, kind, it=0, scale=0, draws=None):
        """one kernel of Run() with the reference's block shape and grid size; returns the most draws one pixel consumed"""
        d = _f32(draws) if draws is not None else None
        if d is not None:
            assert d.shape == (self.H * self.W, DRAW_CAP)
        rc = self._l.ref_launch(self._ctx, C.byref(prm), int(kind), int(it), int(scale), d.ctypes.data if d is not None else None, DRAW_CAP if d is not None else 0)
        if rc == -1:
            raise RuntimeError(f"a pixel consumed more than the {DRAW_CAP if d is not None else 0} uniforms of its row")
        if rc < 0:
            raise RuntimeError(f"ref_launch refused its arguments ({rc})")
        return rc


def sky_bilateral(bgr, mask, fma=False):
    bgr, mask = np.ascontiguousarray(bgr, np.uint8), _f32(mask)
    assert bgr.shape == mask.shape + (3,)
    out = np.empty(mask.shape, np.float32)
    lib(fma).ref_sky_bilateral(bgr.ctypes.data, mask.ctypes.data, out.ctypes.data, mask.shape[0], mask.shape[1])
    return out


def draw_table(oracle, seed, launch, npix):
    """the project's own random stream as a table: row p = the first DRAW_CAP uniforms of stream (seed, pixel p, launch)"""
    return oracle.rng_table(seed, launch, npix, DRAW_CAP)


def ring_centres(n_src, spacing):
    """n_src distinct camera centres around the reference, nearest first"""
    cand = sorted((dx * dx + dy * dy, dx, dy) for dx in range(-3, 4) for dy in range(-3, 4) if (dx, dy) != (0, 0))
    return [(0.0, 0.0, 0.0)] + [(spacing * dx, spacing * dy, 0.0) for _, dx, dy in cand[:n_src]]


def planes_for(cam, depth, tilt, rng):
    """per-pixel camera-frame planes through the points at `depth` with normals tilted away from the optical axis by ~`tilt`"""
    h, w = depth.shape
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    n = np.zeros((h, w, 3))
    n[..., 2] = -1.0
    n[..., :2] = tilt * rng.normal(size=(h, w, 2))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    X = np.stack([depth * (u - cam.K[2]) / cam.K[0], depth * (v - cam.K[5]) / cam.K[4], depth], -1)
    return np.concatenate([n, -(n * X).sum(-1)[..., None]], -1).astype(np.float32)


def plane_sets(sc, dmin, dmax, rng):
    """true surface, 10 % depth noise with tilted normals, fully random"""
    gt = sc.views[0].gt_depth.astype(np.float64)
    cam = sc.views[0].cam
    return [("true surface", planes_for(cam, gt, 0.0, rng)), ("noisy, tilted", planes_for(cam, gt * rng.uniform(0.9, 1.1, gt.shape), 0.3, rng)),
            ("random", planes_for(cam, rng.uniform(dmin, dmax, gt.shape), 1.0, rng))]


def same_bits(a, b):
    """bitwise equality of two float32 / uint32 arrays (NaN equals NaN whatever its payload)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float32:
        nan = np.isnan(a)
        if not np.array_equal(nan, np.isnan(b)):
            return False
        return bool(np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]))
    return bool(np.array_equal(a, b))


def n_diff(a, b):
    """how many elements differ (NaN equals NaN), for messages"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float32:
        return int(((a != b) & ~(np.isnan(a) & np.isnan(b))).sum())
    return int((a != b).sum())


# ---------------------------------------------------------------------------------------------------------------------------------
# The canonical arithmetic against the compiled reference, directly.  `handle` is a context of the HIP library
# (tests/test_reference_gpu.py) or of the oracle in its canonical mode (tests/test_reference_cpu.py): the two are bit-identical
# (tests/test_parity_gpu.py), so the CPU run predicts the GPU run exactly and the inputs below were chosen on the CPU.
# ---------------------------------------------------------------------------------------------------------------------------------
DIRECT_W, DIRECT_H, DIRECT_V = 96, 64, 4
DIRECT_PLANE_SEED, DIRECT_STEP_SEED, DIRECT_STATE_SEED = 11, 11, 7


class Direct:
    """the 96x64, 4-source scene of the direct comparisons: problem, source depth maps, prior, and both builds of the reference"""

    def __init__(self, pm):
        w, h, nv = DIRECT_W, DIRECT_H, DIRECT_V
        self.sc = pm.synth.make_problem_scene(w, h, n_src=nv, quantize=True)
        ids = list(range(1, nv + 1))
        self.cams, self.imgs = self.sc.problem(0, ids)
        self.dmin, self.dmax = (float(v) for v in pm.synth.kernel_depth_range(self.cams[0]))
        rng = np.random.default_rng(5)
        self.src_depths = [self.sc.views[i].gt_depth * (1.0 + 0.005 * rng.standard_normal((h, w))).astype(np.float32) for i in ids]
        self.prior = np.zeros((h, w, 4), np.float32)
        self.prior[..., 2] = -1.0
        self.prior[..., 3] = self.sc.views[0].gt_depth
        self.mask = (rng.uniform(size=(h, w)) < 0.6).astype(np.uint32)
        self.planes = plane_sets(self.sc, self.dmin, self.dmax, np.random.default_rng(DIRECT_PLANE_SEED))

    def reference(self, q8=False, fma=False):
        r = Reference(self.cams, self.imgs, q8=q8, fma=fma)
        r.set_src_depths(self.src_depths)
        r.set_prior(self.prior, self.mask)
        return r

    def attach(self, handle):
        handle.set_views(self.cams, self.imgs)
        handle.set_src_depths(self.src_depths)
        handle.set_prior(self.prior, self.mask)
        return handle

    def params(self, pm, **kw):
        return pm.PatchMatchParams(num_images=DIRECT_V + 1, depth_min=self.dmin, depth_max=self.dmax, **kw)


def check_ncc_direct(pm, d, handle, bars):
    """T1 of tests/test_literal_gpu.py with the compiled reference in the place of the literal modes; returns the worst |d| per build"""
    prm = d.params(pm, max_scale=0)
    refs = {1: d.reference(q8=False), 2: d.reference(q8=True)}
    worst = {1: 0.0, 2: 0.0}
    for pname, planes in d.planes:
        for scale in (0, 1, 2):
            got = handle.eval_ncc(prm, planes, scale)
            for mode, ref in refs.items():
                want = ref.eval_ncc(prm, planes, scale)
                both = (got < 2.0) & (want < 2.0)
                dd = np.abs(got - want)[both]
                print(f"NCC vs compiled reference, planes '{pname}', scale {scale}, {'8-bit fractions' if mode == 2 else 'IEEE'}: valid {both.mean():.3f}, sentinel disagreement "
                      f"{((got == 2.0) != (want == 2.0)).mean():.2e}, max {dd.max():.2e}, median {np.median(dd):.2e}, above {bars.T1_BAR:g}: {int((dd > bars.T1_BAR).sum())} of {dd.size}")
                worst[mode] = max(worst[mode], float(dd.max()))
                assert both.mean() > bars.T1_BOTH_VALID
                assert ((got == 2.0) != (want == 2.0)).mean() < bars.T1_SENTINEL_DISAGREEMENT
                if mode == 1:
                    assert (dd > bars.T1_BAR).mean() <= bars.T1_SHARE_ABOVE_BAR, (pname, scale, float(dd.max()))
                    assert dd.max() < bars.T1_MAX
                    assert np.median(dd) < bars.T1_MEDIAN
                else:
                    assert (dd > bars.T1_BAR).mean() <= bars.T1_Q8_SHARE_ABOVE_BAR, (pname, scale, float(dd.max()))
                    assert dd.max() < bars.T1_Q8_MAX
    return worst


# the bars of the canonical geometric check against the literal chain (tests/test_oracle_cpu.py::test_geom_cost_canonical_vs_literal): the
# literal chain IS the reference's code bit for bit (tests/test_reference_cpu.py::test_geometric_cost), so they carry over unchanged
from test_oracle_cpu import GEOM_CAP_DISAGREEMENT, GEOM_MEDIAN, GEOM_P999, GEOM_TEXEL_FLIP, GEOM_TEXEL_FLIP_SHARE  # noqa: E402


def check_geom_direct(pm, d, handle):
    prm = d.params(pm, max_scale=0, geom_consistency=True)
    ref = d.reference()
    worst = 0.0
    for pname, planes in d.planes[:2]:      # planes near the surface: a random plane's point misses the source surface and every check ends at the cap
        got, want = handle.eval_geom(prm, planes), ref.eval_geom(prm, planes)
        both = (got < 3.0) & (want < 3.0)
        dd = np.abs(got - want)[both]
        print(f"geometric cost vs compiled reference, planes '{pname}': below the cap {both.mean():.3f}, cap disagreement {((got == 3.0) != (want == 3.0)).mean():.2e}, "
              f"median {np.median(dd):.2e}, 99.9 % {np.percentile(dd, 99.9):.2e}, texel flips {(dd > GEOM_TEXEL_FLIP).mean():.2e}, max {dd.max():.2e}")
        worst = max(worst, float(np.percentile(dd, 99.9)))
        assert both.mean() > 0.5
        assert ((got == 3.0) != (want == 3.0)).mean() < GEOM_CAP_DISAGREEMENT
        assert np.median(dd) < GEOM_MEDIAN and np.percentile(dd, 99.9) < GEOM_P999 and (dd > GEOM_TEXEL_FLIP).mean() < GEOM_TEXEL_FLIP_SHARE
    return worst


# Homography.  The canonical H comes from constants composed in double and two fp32 operations per element; the reference's chain
# forms each element from at most 16 rounded fp32 operations on terms no larger than (1 + cx / fx + cy / fy) max|H| < 2.2 max|H|
# (K^-1 is applied as `- H0 cx / fx - H1 cy / fy + H2`).  Worst case, every rounding in the same direction:
# 16 x 2^-24 x 2.2 max|H| < 2^-18 max|H|.
HOMOGRAPHY_BAR = 2.0 ** -18


def check_homography_direct(pm, d, handle):
    ref = d.reference()
    rng = np.random.default_rng(3)
    worst = 0.0
    for pname, planes in d.planes:
        for y, x in zip(rng.integers(0, DIRECT_H, 16), rng.integers(0, DIRECT_W, 16)):
            for v in range(DIRECT_V):
                got, want = handle.homography(planes[y, x], v).astype(np.float64), ref.homography(planes[y, x], v).astype(np.float64)
                rel = float(np.abs(got - want).max() / np.abs(want).max())
                worst = max(worst, rel)
                assert rel < HOMOGRAPHY_BAR, (pname, x, y, v, rel)
    print(f"homography vs compiled reference: worst |dH| / max|H| = {worst:.2e} (bar {HOMOGRAPHY_BAR:.2e})")
    return worst


def flips(a, b):
    """share of the pixels whose plane's fourth component differs by more than 1e-3 relative (T2 of tests/test_literal_gpu.py)"""
    rel = np.abs(a[..., 3] - b[..., 3]) / np.maximum(np.abs(b[..., 3]), 1e-6)
    return float((rel > 1e-3).mean())


def check_steps_direct(pm, oracle, d, handle, bars):
    """InitializeScore, then one BlackPixelUpdate from an identical state, in the three modes of Run(): `handle` against the
    reference's IEEE build, beside the control: the reference's IEEE build against its own contracted build"""
    H, W = DIRECT_H, DIRECT_W
    ref, ref_q8, ref_fma = d.reference(), d.reference(q8=True), d.reference(fma=True)
    handle.run(d.params(pm, max_scale=0), DIRECT_STATE_SEED)      # a converged photometric result: what the geometric and prior runs start from
    s_planes, s_costs = handle.get()
    rows = []
    for name, geom, planar in (("photometric", False, False), ("geometric", True, False), ("prior", False, True)):
        prm = d.params(pm, max_scale=0, geom_consistency=geom, planar_prior=planar)
        zeros = np.zeros((H, W), np.uint32)
        handle.set_state(s_planes, s_costs)
        handle.set_selected_views(zeros)
        handle.step(prm, DIRECT_STEP_SEED, pm.KIND_INIT, 0, 0, 0)
        ip, ic = handle.get()
        isel = handle.get_selected_views()
        ref.set_state(s_planes, s_costs, zeros)
        ref.launch(prm, pm.KIND_INIT, 0, 0, draw_table(oracle, DIRECT_STEP_SEED, 0, H * W))
        rp, rcost, rsel, _ = ref.get()
        f_init = flips(ip, rp)
        if name == "photometric":
            assert same_bits(ip, rp), f"InitializeScore: {n_diff(ip, rp)} plane components differ"      # drawn, not selected: the same bits
        # geometric / prior: stored planes re-encoded, priors perturbed through sin / cos: T2's bar (photometric: 0 follows from the bits)
        assert f_init <= (0.0 if name == "photometric" else bars.T2_INIT_FLIPS), (name, f_init)
        both = (ic < 2.0) & (rcost < 2.0)
        di = np.abs(ic - rcost)[both]
        assert both.mean() > bars.T1_BOTH_VALID and ((ic == 2.0) != (rcost == 2.0)).mean() < bars.T1_SENTINEL_DISAGREEMENT
        assert (di > bars.T1_BAR).mean() <= bars.T1_SHARE_ABOVE_BAR and di.max() < bars.T1_MAX and np.median(di) < bars.T1_MEDIAN, (name, float(di.max()))
        # one BlackPixelUpdate from the state InitializeScore left on `handle`, on every side
        draws = draw_table(oracle, DIRECT_STEP_SEED, 1, H * W)
        out = {}
        for key, r in (("ieee", ref), ("fma", ref_fma), ("q8", ref_q8)):
            r.set_state(ip, ic, isel)
            r.launch(prm, pm.KIND_BLACK, 0, 0, draws)
            out[key] = r.get()
        handle.step(prm, DIRECT_STEP_SEED, pm.KIND_BLACK, 0, 0, 1)
        up, uc = handle.get()
        assert (up != ip).any(-1).mean() > 0.3                                                              # the pass moved its pixels
        far = float((np.abs(uc - out["ieee"][1]) > bars.T2_COST_FAR).mean())
        mh, ml = float(uc.mean()), float(out["ieee"][1].mean())
        rows.append((name, f_init, float(di.max()), flips(up, out["ieee"][0]), flips(out["fma"][0], out["ieee"][0]), flips(out["q8"][0], out["ieee"][0]), far, mh, ml))
    print("one BlackPixelUpdate from an identical state, pixels whose plane differs by more than 1e-3 from the compiled reference (IEEE build):")
    for name, f_init, dmax, f_h, f_fma, f_q8, far, mh, ml in rows:
        print(f"  {name}: canonical / HIP {f_h:.2e}; control, the reference against itself: contracted build {f_fma:.2e}, 8-bit fractions {f_q8:.2e}; "
              f"ratio to the contracted build {f_h / f_fma if f_fma > 0 else float('inf'):.2f}; after InitializeScore {f_init:.1e}, worst cost |d| {dmax:.2e}; "
              f"costs: |d| > {bars.T2_COST_FAR:g} at {far:.1e} of the pixels, mean {mh:.5f} / {ml:.5f}")
    for name, f_init, dmax, f_h, f_fma, f_q8, far, mh, ml in rows:
        assert far <= bars.T2_COST_FAR_SHARE and abs(mh / ml - 1.0) <= bars.T2_MEAN_COST_REL, (name, far, mh, ml)
    return rows
