"""Seeded random inputs of the depth-map fusion, shared by tests/test_fusion_fuzz_cpu.py (what the sweep covers, on the oracle) and
tests/test_fusion_fuzz_gpu.py (the sweep on the MI355X), and the comparison rule both use.  case(pm, k) is a pure function of k.

What a case varies: 2..12 images (every tenth case 34 or 35, to reach the 33 slots of a view list), up to three image sizes with
widths and heights at the edges of k_fuse's 32 x 8 tile and down to one row or one pixel, view lists that are random permutations
of the other images (0..32 sources, never in ascending order by construction), estimate flags, a largest image that is only a
source, depths that are zero, negative, NaN, +-inf, denormal or huge, patches of NaN and of zero normals, grey or B,G,R colours,
sky masks, both consistency criteria.  One case in seven is CLEAN -- every image estimated, finite depths and normals, B,G,R
colours: what the reference's compiled RunFusion can be run on (its int(v + 0.5f) of a NaN is undefined behaviour)."""
import numpy as np

CASE_SEED = 7000
DEFAULT_CASES = 150                                         # what the sweep runs unless MPMVS_FUSE_FUZZ_CASES says otherwise; the coverage test is over these
SPECIAL_W, SPECIAL_H = (1, 31, 32, 33), (1, 7, 8, 9)       # k_fuse: 32 columns x 8 rows per block
MAX_PIXELS = 25000                                          # per case, over all images
MAX_SOURCES = 32                                            # MPMVS_MAX_SRC_VIEWS
BAD_DEPTHS = {"zero": 0.0, "negative": -1.0, "nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "denormal": 1e-40, "huge": 1e30}
FINITE_BAD = ("zero", "negative", "denormal", "huge")
_cache = {}


def analytic_normals(pm, v, eps=1e-3):
    """analytic world normal of the height field z = Z(x, y) at the pixels of view v: (Zx, Zy, -1) / |.|"""
    H, W = v.gt_depth.shape
    u, w = np.meshgrid(np.arange(W), np.arange(H))
    ray = np.stack([(u - v.K[0, 2]) / v.K[0, 0], (w - v.K[1, 2]) / v.K[1, 1], np.ones_like(u, float)], -1) @ v.R
    P = v.C + v.gt_depth[..., None] * ray
    Zx = (pm.synth.height_field(P[..., 0] + eps, P[..., 1]) - pm.synth.height_field(P[..., 0] - eps, P[..., 1])) / (2 * eps)
    Zy = (pm.synth.height_field(P[..., 0], P[..., 1] + eps) - pm.synth.height_field(P[..., 0], P[..., 1] - eps)) / (2 * eps)
    n = np.stack([Zx, Zy, -np.ones_like(Zx)], -1)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    return n.astype(np.float32)


def multi_size_views(pm, sizes, centers, **kw):
    """view i of make_scene(sizes[i], centers): one scene per distinct size over the same centres (K follows the size; the
    rotations are drawn per view in order, so they agree between the scenes)"""
    views = [None] * len(sizes)
    for size in sorted(set(sizes)):
        mine = [i for i, s in enumerate(sizes) if s == size]
        sc = pm.synth.make_scene(size[0], size[1], centers, only=set(mine), **kw)
        for i in mine:
            views[i] = sc.views[i]
    return views


class FuzzCase:
    """sources[k]: the source ids of image k without k itself (what fusion.fuse and oracle.fuse take)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self.n = len(self.cams)

    def args(self):
        return self.cams, self.est, self.depths, self.normals, self.cols, self.sources, self.dynamic

    def slots(self):
        """list lengths as the library counts them (own image included) of the estimated images"""
        return [1 + len(s) for s, e in zip(self.sources, self.est) if e]

    def pixels(self, k):
        return self.sizes[k][0] * self.sizes[k][1]

    def larger_unestimated_source(self):
        """an image that is not estimated, larger than every estimated one, and a source of an estimated one"""
        top = max((self.pixels(k) for k in range(self.n) if self.est[k]), default=0)
        used = {s for k in range(self.n) if self.est[k] for s in self.sources[k]}
        return any(not self.est[s] and self.pixels(s) > top for s in used)


def _draw_size(rng, thin_allowed):
    """thin (one column or one row) only where the case has another size to give points"""
    while True:
        w = int(rng.choice(SPECIAL_W)) if rng.random() < 0.4 else int(rng.integers(6, 65))
        h = int(rng.choice(SPECIAL_H)) if rng.random() < 0.4 else int(rng.integers(6, 49))
        if thin_allowed or (w > 1 and h > 1):
            return w, h


def _patch(rng, h, w):
    """a random rectangle of about a quarter of each side, at least one pixel"""
    ph, pw = max(1, h // 4), max(1, w // 4)
    y, x = int(rng.integers(0, h - ph + 1)), int(rng.integers(0, w - pw + 1))
    return slice(y, y + ph), slice(x, x + pw)


def case(pm, k):
    if k in _cache:
        return _cache[k]
    rng = np.random.default_rng(CASE_SEED + k)
    clean = k % 7 == 3
    wide = k % 10 == 7
    n = int(rng.integers(34, 36)) if wide else int(rng.integers(2, 13))
    if n < 4 and rng.random() < 0.85:       # two images cannot give a point (the last slot is skipped while nothing is consistent), three hardly
        n = int(rng.integers(4, 13))
    # sizes: up to three, dealt to the images at random; the one that contributes most is redrawn until the case fits
    kinds = [_draw_size(rng, j > 0) for j in range(int(rng.integers(1, 4)))]
    which = rng.integers(0, len(kinds), n)
    while True:
        load = [int((which == j).sum()) * kinds[j][0] * kinds[j][1] for j in range(len(kinds))]
        if sum(load) <= MAX_PIXELS:
            break
        j = int(np.argmax(load))
        kinds[j] = _draw_size(rng, j > 0)
    sizes = [kinds[j] for j in which]
    centers = np.stack([rng.uniform(-0.3, 0.3, n), rng.uniform(-0.2, 0.2, n), rng.uniform(-0.05, 0.05, n)], -1)
    with np.errstate(all="ignore"):       # a one-column image has fy = 0.9 and rays far off the axis: the ray caster may not converge there
        views = multi_size_views(pm, sizes, centers, seed=int(rng.integers(1, 10 ** 6)), rot_deg=float(rng.uniform(0.0, 3.0)), quantize=True)
    cams = [v.cam for v in views]
    # estimate flags; in some cases every image of the largest size is a source only
    est = [True] * n if clean else [bool(e) for e in rng.random(n) < 0.85]
    px = [w * h for w, h in sizes]
    only_source = not clean and len(set(px)) > 1 and rng.random() < 0.35
    if only_source:
        est = [e and p < max(px) for e, p in zip(est, px)]
    if not any(est):
        est[int(np.argmin(px))] = True
    # view lists: a random permutation of the other images, cut at a random length
    sources = []
    for i in range(n):
        others = rng.permutation([j for j in range(n) if j != i])
        longest = min(n - 1, MAX_SOURCES)
        # any length in the cases of 34 or 35 images (every slot count up to 33 turns up); else mostly the longer half
        length = int(rng.integers(0, longest + 1)) if wide or rng.random() < 0.2 else int(rng.integers((longest + 1) // 2, longest + 1))
        sources.append([int(s) for s in others[:length]])
    if only_source:
        big = int(np.argmax(px))
        host = int(rng.choice([i for i in range(n) if est[i]]))
        if big not in sources[host]:
            sources[host] = ([big] + sources[host])[: MAX_SOURCES]
    # maps
    names = FINITE_BAD if clean else tuple(BAD_DEPTHS)
    bad_used = set()
    depths, normals = [], []
    for v in views:
        gt = np.where(np.isfinite(v.gt_depth) & (v.gt_depth > 0) & (v.gt_depth < 1e3), v.gt_depth, np.float32(0.0))    # no surface found: a hole
        d = gt * (1.0 + 0.002 * rng.standard_normal(gt.shape)).astype(np.float32)
        at = rng.random(d.shape) < 0.03
        pick = rng.integers(0, len(names), d.shape)
        for j, name in enumerate(names):
            sel = at & (pick == j)
            if sel.any():
                d[sel] = np.float32(BAD_DEPTHS[name])
                bad_used.add(name)
        depths.append(d)
        with np.errstate(all="ignore"):
            nm = analytic_normals(pm, v)
        nm[~np.isfinite(nm).all(-1)] = (0.0, 0.0, -1.0)
        normals.append(nm)
    bad_normals = not clean and rng.random() < 1 / 3
    if bad_normals:
        for i in {int(rng.integers(0, n)), int(rng.integers(0, n))}:
            h, w = depths[i].shape
            normals[i][_patch(rng, h, w)] = np.nan
            normals[i][_patch(rng, h, w)] = 0.0
    # colours: grey or B,G,R; sky masks as tests/test_fusion_cpu.py::_colours_and_sky builds them (top rows and scattered pixels; any
    # value > 0 counts), the rows scaled to the height, one image without a mask
    g8 = [np.clip(np.rint(np.nan_to_num(v.image, nan=0.0, posinf=255.0, neginf=0.0)), 0, 255).astype(np.uint8) for v in views]
    colour = clean or rng.random() < 0.5
    cols = [np.stack([g, 255 - g, (g * 0.5 + 20)], -1).round().astype(np.uint8) for g in g8] if colour else g8
    sky = None
    if rng.random() < 1 / 3:
        sky = []
        for i, g in enumerate(g8):
            m = np.zeros(g.shape, np.uint8)
            m[: (g.shape[0] * (1 + i % 3)) // 8] = 255
            m[rng.random(g.shape) < 0.02] = 1
            sky.append(m)
        sky[int(rng.integers(0, n))] = None
    dynamic = bool(rng.random() < 0.65)
    for a in depths + normals + cols + [m for m in (sky or []) if m is not None]:
        a.setflags(write=False)
    c = FuzzCase(k=k, cams=cams, est=est, depths=depths, normals=normals, cols=cols, sky=sky, sources=sources, dynamic=dynamic, sizes=sizes,
                 clean=clean, colour=colour, bad_depths=bad_used, bad_normals=bad_normals)
    _cache[k] = c
    return c


def same_bits(a, b):
    """the comparison rule of the sweep: equal bits wherever `b` (the oracle) is not NaN, NaN wherever it is; payloads of NaNs are
    not compared (nobody has measured whether the GPU and x86 carry the same payload through `sp += T`)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.float32:
        return bool(np.array_equal(a, b))
    nan = np.isnan(b)
    return bool(np.isnan(a[nan]).all() and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]))


def same_records(a, b):
    """PLY records under the same rule: six floats, three colour bytes"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != np.uint8 or b.dtype != np.uint8:
        return False
    fa, fb = (np.ascontiguousarray(x[:, :24]).view(np.float32) for x in (a, b))
    return same_bits(fa, fb) and bool(np.array_equal(a[:, 24:], b[:, 24:]))


def same_result(got, want):
    """(cloud, valid, masks) of fusion.fuse against the oracle's"""
    return same_bits(got[0], want[0]) and all(np.array_equal(a, b) for a, b in zip(got[1], want[1])) and \
        all(np.array_equal(a, b) for a, b in zip(got[2], want[2]))


# The cap: 35 images, image 0 with the 32 sources a list may hold (33 slots: slot 32 is bit 31 of the track's slot word).  The
# seed is recorded like VERTEX_SEEDS of ref_common: what tests/test_fusion_fuzz_cpu.py asserts on the oracle -- pixels of image 0
# that are consistent with every one of the 32 sources -- holds for it (seed 5, the first tried: 8 such pixels).
CAP_SEED = 5
CAP_IMAGES, CAP_SIZES = 35, ((40, 30), (33, 25))


def cap_case(pm):
    """images alternate between two sizes over centres close enough that every source sees image 0's surface; noise-free depths"""
    if "cap" in _cache:
        return _cache["cap"]
    rng = np.random.default_rng(CAP_SEED)
    n = CAP_IMAGES
    sizes = [CAP_SIZES[i % 2] for i in range(n)]
    centers = np.stack([rng.uniform(-0.05, 0.05, n), rng.uniform(-0.035, 0.035, n), np.zeros(n)], -1)
    views = multi_size_views(pm, sizes, centers, seed=CAP_SEED, rot_deg=0.5, quantize=True)
    g8 = [np.clip(np.rint(v.image), 0, 255).astype(np.uint8) for v in views]
    sources = [list(range(1, MAX_SOURCES + 1))] + [[(i + d) % n for d in (1, 2, 3, 4)] for i in range(1, n)]
    c = FuzzCase(k="cap", cams=[v.cam for v in views], est=[True] * n, depths=[v.gt_depth.copy() for v in views],
                 normals=[analytic_normals(pm, v) for v in views], cols=[np.stack([g, 255 - g, g // 2 + 20], -1) for g in g8], sky=None,
                 sources=sources, dynamic=True, sizes=sizes, clean=True, colour=True, bad_depths=set(), bad_normals=False)
    _cache["cap"] = c
    return c
