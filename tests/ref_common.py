"""ctypes view of the reference's own device code compiled for the host (oracle/ref_driver.cpp, `make -C oracle ref`):
oracle/_ref/libmpmvs_ref.so (IEEE operations as written) and libmpmvs_ref_fma.so (the same text with contracted multiply-adds);
and of its host code (oracle/ref_host_driver.cpp): libmpmvs_ref_host.so and libmpmvs_ref_host_rcp.so, RunFusion with its PLY
writer and GetTriangulateVertices, the two differing only in the stand-in for OpenCV's `Vec3f /= float` (ref_fuse, ref_vertices).

The libraries are build products of __graft_entry__.build() on a machine that holds the reference tree; they travel with the
working tree to machines that do not.  A missing library is an error, never a skip.  Shared by tests/test_reference_cpu.py and
tests/test_reference_gpu.py, together with the scenes, plane sets and draw tables both use."""
import ctypes as C
import importlib
import os
import tempfile

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


def host_lib(rcp=False):
    """the reference's host code: RunFusion + PLY writer and GetTriangulateVertices; rcp: the build whose Vec3f `/=` multiplies
    by the fp32 reciprocal instead of dividing"""
    name = "libmpmvs_ref_host_rcp.so" if rcp else "libmpmvs_ref_host.so"
    if name not in _cache:
        path = os.path.join(ORACLE_DIR, "_ref", name)
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: __graft_entry__.build() makes it where the reference tree is present (MPMVS_REFERENCE)")
        l = C.CDLL(path)
        pp_f, pp_u8 = C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.POINTER(C.c_ubyte))
        l.refh_fuse.restype = C.c_int
        l.refh_fuse.argtypes = [C.c_int, C.POINTER(_abi.Camera), pp_f, pp_f, pp_u8, pp_u8, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_char_p]
        l.refh_vertices.restype = C.c_int
        l.refh_vertices.argtypes = [_P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int]
        _cache[name] = l
    return _cache[name]


PLY_RECORD = 27      # 6 floats and 3 bytes per vertex


def ref_fuse(cams, depths, normals, colours_bgr, sky_or_none, sources, use_dynamic, rcp=False):
    """the reference's RunFusion and its own PLY writer over arrays: every image estimated, refID == index, image k's maps of the
    size cams[k] states.  colours_bgr[k]: [h][w][3] uint8; sky_or_none: None (sky_seg off) or per image a [h][w] uint8 mask or
    None (an all-zero mask on the reference's side); sources[k]: the source ids of image k without k itself.
    Returns (header bytes, records [M, 27] uint8) of the file the reference wrote."""
    n = len(cams)
    shapes = [(cams[k].height, cams[k].width) for k in range(n)]
    d = [np.ascontiguousarray(depths[k], np.float32) for k in range(n)]
    nm = [np.ascontiguousarray(normals[k], np.float32) for k in range(n)]
    g = [np.ascontiguousarray(colours_bgr[k], np.uint8) for k in range(n)]
    for k in range(n):
        assert d[k].shape == shapes[k] and nm[k].shape == shapes[k] + (3,) and g[k].shape == shapes[k] + (3,)
        assert np.isfinite(d[k]).all(), "the reference's int() of a NaN coordinate is undefined: keep non-finite depths out"
    sk = None
    if sky_or_none is not None:
        sk = [np.zeros(shapes[k], np.uint8) if m is None else np.ascontiguousarray(m, np.uint8) for k, m in enumerate(sky_or_none)]
        assert all(m.shape == sh for m, sh in zip(sk, shapes))
    ids, off = [], [0]
    for k in range(n):
        ids += [k] + [int(s) for s in sources[k]]
        off.append(len(ids))
    fp = lambda arrs: (C.POINTER(C.c_float) * n)(*[a.ctypes.data_as(C.POINTER(C.c_float)) for a in arrs])
    up = lambda arrs: (C.POINTER(C.c_ubyte) * n)(*[a.ctypes.data_as(C.POINTER(C.c_ubyte)) for a in arrs])
    with tempfile.TemporaryDirectory() as tmp:
        rc_ = host_lib(rcp).refh_fuse(n, (_abi.Camera * n)(*cams), fp(d), fp(nm), up(g), None if sk is None else up(sk), (C.c_int * (n + 1))(*off),
                                      (C.c_int * len(ids))(*ids), 1 if use_dynamic else 0, tmp.encode())
        if rc_ != 0:
            raise RuntimeError(f"refh_fuse failed ({rc_}): " + ("an image or mask would have been resampled" if rc_ == -1 else "unknown image number in a path"))
        raw = open(os.path.join(tmp, "MPMVS_model.ply"), "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    body = np.frombuffer(raw, np.uint8, offset=end)
    assert len(body) % PLY_RECORD == 0
    return raw[:end], body.reshape(-1, PLY_RECORD).copy()


def ref_vertices(costs, geom, geom_rule, rcp=False):
    """the reference's GetTriangulateVertices over one cost map (and geometric cost map): [n, 2] int32 of x, y"""
    c = _f32(costs)
    g = _f32(geom if geom is not None else np.zeros_like(c))
    assert c.ndim == 2 and g.shape == c.shape
    h, w = c.shape
    cap = 3 * ((w + 4) // 5) * ((h + 4) // 5)
    out = np.zeros((cap, 2), np.int32)
    n = host_lib(rcp).refh_vertices(c.ctypes.data, g.ctypes.data, w, h, 1 if geom_rule else 0, out.ctypes.data, cap)
    assert 0 <= n <= cap
    return out[:n].copy()


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


# ---------------------------------------------------------------------------------------------------------------------------------
# The cases of the fusion and vertex comparisons against the reference's compiled HOST code (tests/test_reference_host_cpu.py on
# the CPU, tests/test_reference_gpu.py on the GPU).  Built once per session; the arrays are shared and nobody writes to them.
# ---------------------------------------------------------------------------------------------------------------------------------
MAX_FUSE_SOURCES = 32      # mpmvs_fuse takes an image and up to MPMVS_MAX_SRC_VIEWS sources (include/mpmvs.h)


class FuseCase:
    """one fusion input.  ours: the colours as the project's entry points get them (1 channel for the grey case);
    bgr: the same as the 3-channel images the reference reads"""

    def __init__(self, name, cams, depths, normals, ours, bgr, sky, sources, dynamic):
        self.name, self.cams, self.depths, self.normals, self.ours, self.bgr, self.sky, self.sources, self.dynamic = name, cams, depths, normals, ours, bgr, sky, sources, dynamic
        self.n = len(cams)
        self._ref = {}

    def reference(self, rcp=False):
        """(header, records) of the file the reference writes for this case"""
        if rcp not in self._ref:
            self._ref[rcp] = ref_fuse(self.cams, self.depths, self.normals, self.bgr, self.sky, self.sources, self.dynamic, rcp=rcp)
        return self._ref[rcp]

    def oracle_records(self, oracle, fusion, mode):
        """PLY records of oracle mode 1 (literal) or 2 (reference order, canonical arithmetic) or 0 (snapshot)"""
        cloud, _, _ = oracle.fuse(self.cams, [True] * self.n, self.depths, self.normals, self.ours, self.sources, use_dynamic=self.dynamic,
                                  sequential_literal=(mode == 1), sky=self.sky, reference_order=(mode == 2))
        return fusion.ply_records(cloud)

    def truncated_pixels(self):
        """from a float64 projection of the inputs: how many (pixel, source slot) pairs land on a source coordinate with
        coordinate + 0.5 in (-1, 0), which `int()` truncates to pixel 0 (the last slot is left out: it may not be visited)"""
        count = 0
        for i in range(self.n):
            cam = self.cams[i]
            K, R, Cc = (np.array(v, np.float64) for v in (cam.K, cam.R, cam.C))
            h, w = cam.height, cam.width
            u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
            d = self.depths[i].astype(np.float64)
            X = np.stack([d * (u - K[2]) / K[0], d * (v - K[5]) / K[4], d], -1)
            P = X @ R.reshape(3, 3) + Cc                              # world = R^T X + C
            for s in self.sources[i][:-1]:
                sc = self.cams[s]
                Ks, Rs, ts = (np.array(a, np.float64) for a in (sc.K, sc.R, sc.t))
                Y = P @ Rs.reshape(3, 3).T + ts
                q = Y @ Ks.reshape(3, 3).T
                with np.errstate(all="ignore"):
                    x, y = q[..., 0] / q[..., 2] + 0.5, q[..., 1] / q[..., 2] + 0.5
                inside_x, inside_y = (x > -1) & (x < sc.width), (y > -1) & (y < sc.height)
                count += int(((d > 0) & inside_x & inside_y & (((x > -1) & (x < 0)) | ((y > -1) & (y < 0)))).sum())
        return count


_fuse_cases = {}


def fusion_cases(pm):
    """name -> FuseCase, over the scenes of tests/test_fusion_cpu.py (3 x 2 camera grid, five sources per image)"""
    if _fuse_cases:
        return _fuse_cases
    from test_fusion_cpu import _colours_and_sky, _scene

    def scene(size):
        sc, cams, depths, normals, grays, neigh = _scene(pm, size=size)
        cols, sky = _colours_and_sky(grays)
        return cams, depths, normals, grays, cols, sky, neigh

    def add(name, cams, depths, normals, ours, bgr, sky, neigh, dynamic=True):
        _fuse_cases[name] = FuseCase(name, cams, depths, normals, ours, bgr, sky, neigh, dynamic)

    cams, depths, normals, grays, cols, sky, neigh = scene((96, 72))
    add("96x72_dynamic", cams, depths, normals, cols, cols, None, neigh)
    add("96x72_static", cams, depths, normals, cols, cols, None, neigh, dynamic=False)
    g8 = [np.clip(np.rint(g), 0, 255).astype(np.uint8) for g in grays]
    add("96x72_grey", cams, depths, normals, g8, [np.repeat(g[..., None], 3, -1) for g in g8], None, neigh)
    add("96x72_colour_sky", cams, depths, normals, cols, cols, sky, neigh)
    # the longest list mpmvs_fuse accepts: the five sources repeated (the same source in two slots is legal in the reference)
    add("96x72_32_sources", cams, depths, normals, cols, cols, None, [[s[j % len(s)] for j in range(MAX_FUSE_SOURCES)] for s in neigh])
    holes = [d.copy() for d in depths]
    holes[0][30:50, 5:40] = 0.0
    holes[2][10:30, 20:60] = 0.0
    holes[3][40:60, 50:90] = -1.0
    holes[5][0:20, 0:30] = -3.5
    add("96x72_zero_and_negative_depth", cams, holes, normals, cols, cols, None, neigh)
    # two sizes in one scene: views 1 and 4 at 64x48 -- the same cameras with K scaled by 2/3 (make_scene ties K to the size)
    small = scene((64, 48))
    mix = lambda a, b: [b[k] if k in (1, 4) else a[k] for k in range(len(a))]
    add("96x72_and_64x48", mix(cams, small[0]), mix(depths, small[1]), mix(normals, small[2]), mix(cols, small[4]), mix(cols, small[4]), None, neigh)
    for size in ((131, 97), (257, 256)):        # 257 x 256: 257 chunks of 256 pixels, the second round of k_scan_totals<LastValid>
        cams, depths, normals, grays, cols, sky, neigh = scene(size)
        add(f"{size[0]}x{size[1]}", cams, depths, normals, cols, cols, None, neigh)
    return _fuse_cases


def record_rows(rec):
    """[M, 27] uint8 -> [M] of one 27-byte value each, for set operations"""
    return np.ascontiguousarray(rec).view(np.dtype((np.void, PLY_RECORD))).ravel()


def cloud_difference(got, want):
    """(relative difference of the point counts, share of the records -- as 27-byte rows -- that one cloud has and the other
    lacks, over the count of `want`)"""
    a, b = np.unique(record_rows(got)), np.unique(record_rows(want))
    only = len(np.setdiff1d(a, b, assume_unique=True)) + len(np.setdiff1d(b, a, assume_unique=True))
    return abs(len(got) - len(want)) / len(want), only / len(want)


VERTEX_SIZES = [(85, 75), (83, 71), (1285, 5), (7, 3)]      # 83x71: partial cells on both edges; 7x3: one partial row of cells
VERTEX_INPUTS = ["random", "ties", "exact", "invalid_cells_and_origin", "nan", "all_invalid"]
# 7x3 has two cells: the seed is the first for which every input leaves both rules a vertex count inside the bar of the tests
# (at least one vertex: the second cell must hold a reliable pixel, since two inputs take the first cell out)
VERTEX_SEEDS = {(7, 3): 9101}
_vertex_inputs = {}


def vertex_inputs(w, h, kind):
    """(costs, geometric costs) of one vertex case; the base is _random_costs of tests/test_prior_gpu.py"""
    key = (w, h, kind)
    if key in _vertex_inputs:
        return _vertex_inputs[key]
    from test_prior_gpu import _random_costs
    costs, geom = _random_costs(w, h, VERTEX_SEEDS.get((w, h), 9100 + w))
    rng = np.random.default_rng(77 + w + h)
    if kind == "ties":            # multiples of 1 / 64: cells hold ties for first, second and third place
        costs = (np.floor(costs * 64.0) / 64.0).astype(np.float32)
        geom = np.minimum(geom, np.float32(0.39))                   # every pixel a candidate of the geometric rule
    elif kind == "exact":         # the constants of both rules, exactly
        pick = rng.integers(0, 12, (h, w))
        for k, val in enumerate((0.1, 0.2, 1.0, 2.0)):
            costs[pick == k] = np.float32(val)
        geom[rng.integers(0, 4, (h, w)) == 0] = np.float32(0.4)
    elif kind == "invalid_cells_and_origin":
        for cy in range(0, h, 5):                                    # a fifth of the cells: every cost at or above 2
            for cx in range(0, w, 5):
                if rng.random() < 0.2:
                    costs[cy:cy + 5, cx:cx + 5] = rng.uniform(2.0, 2.6, costs[cy:cy + 5, cx:cx + 5].shape).astype(np.float32)
        # the first cell's threshold 0.85 * sum / (x_end * y_end) exceeds 2.0: the reference pushes its never-assigned (0, 0)
        costs[:5, :5] = np.float32(3.0)
    elif kind == "nan":
        costs[rng.random((h, w)) < 0.01] = np.nan
        costs[min(2, h - 1), min(3, w - 1)] = np.nan
    elif kind == "all_invalid":
        costs = rng.uniform(2.0, 2.6, (h, w)).astype(np.float32)
    _vertex_inputs[key] = (costs, geom)
    return costs, geom
