"""What tests/test_q8_variants_gpu.py runs in the build with 8-bit interpolation fractions, kept apart from it so that
tests/test_q8_variants_cpu.py can count the kernel variants those lists reach and can check the construction of the tied fractions
on the oracle alone, without a GPU."""
import numpy as np

from update_variants_common import init_variant_of, run_variants, variant_of

SEED = 2611
SIZES = [(16, 8), (33, 17)]                      # one wave; last row and last column hold one pixel
EDGE_VIEWS = [1, 8, 9, 16, 17, 24, 25, 32]       # both edges of every bucket of views
FORMATS = [True, False]                          # quantize: 8-bit images -> fp16 texels; otherwise fp32 texels
# a. named matrix: photometric Run() at max_scale 2, geometric Run(), planar-prior Run(), each context
MATRIX = [(W, H, V, q) for (W, H) in SIZES for V in EDGE_VIEWS for q in FORMATS]
# b. one launch per pass, all three Run()s, 33x17
PER_PASS = [(8, True), (16, False), (24, True), (32, True)]
# c. k_init through step(KIND_INIT, scale), 33x17
INIT = [(V, q, s) for V in (8, 16, 24, 32) for q in FORMATS for s in (0, 1, 2)]
# d. the states of tests/test_refine_planes_gpu.py, 33x17; the prior state only where the prior variant keeps its planes in registers
STATES = [(32, True), (8, True), (16, False)]
STATES_PRIOR = [(32, True), (8, True)]
# e. seeded sweep: the cases 0 .. Q8_FUZZ_CASES - 1 of fuzz_common; the smallest multiple of 50 at which the census of
# tests/test_q8_variants_cpu.py holds
Q8_FUZZ_CASES = 150


def named_variants():
    """(update variants, init variants) that the lists above launch, by the part that launches them"""
    upd, ini = {}, {}

    def add(part, u, i):
        upd.setdefault(part, set()).update(u)
        ini.setdefault(part, set()).update(i)

    for part, contexts in (("a", [(V, q) for (_, _, V, q) in MATRIX]), ("b", PER_PASS)):
        for V, q in contexts:
            add(part, *run_variants(V, q, "photometric", 2))
            add(part, *run_variants(V, q, "geometric", 0))
            add(part, *run_variants(V, q, "prior", 0))
    for V, q, s in INIT:
        add("c", set(), {init_variant_of(V, q, s)})
    for V, q in STATES:
        add("d", {variant_of(V, q, "photometric", 0)}, set())          # depth range of one value: black and red steps
        add("d", *run_variants(V, q, "photometric", 0))                 # blank views: a Run() at max_scale 0
    for V, q in STATES_PRIOR:
        add("d", {variant_of(V, q, "prior", 0)}, set())
    return upd, ini


# ---------------------------------------------------------------------------
# f. tied fractions
# ---------------------------------------------------------------------------
# All cameras share one centre and one rotation and differ in the principal point only: the homography of source view v is the
# translation by (sx_v, sy_v) for every plane, and a sample coordinate is an integer plus that shift -- at most 6 + 12 bits, exact
# in fp32 -- so the interpolation fraction of every tap inside the image is the shift's fraction, exactly.
TIE_W, TIE_H = 33, 17
TIE_K = [[64.0, 0.0, 16.0], [0.0, 64.0, 8.0], [0.0, 0.0, 1.0]]
TIE_DEPTHS = (2.0, 6.0)
TIE_E = 2.0 ** -12
TIE_KS = (0, 127, 128, 255)        # fractions (k + 0.5) / 256: the ties of floor(a * 256 + 0.5), the first, the middle two and the last
TIE_OTHER = 0.25                   # the shift on the other axis
# (name, shift) along the axis under test; view 2 i shifts x by shift i, view 2 i + 1 shifts y by it
TIE_SHIFTS = ([((k, e), (k + 0.5) / 256.0 + e * TIE_E) for k in TIE_KS for e in (-1, 0, 1)]
              + [((k, 0), (k + 0.5) / 256.0) for k in (1, 254)] + [("zero", 0.0), ("one", 1.0)])
TIE_CONTEXTS = (8, 16, 24, 32)     # source views of a context: the first that many of the list
TIE_PLANES = ((0.0, 0.0, -1.0, 3.0), (0.6, 0.0, -0.8, 4.5))


def tie_view(name, axis):
    """index of the source view that shifts `axis` (0: x, 1: y) by the shift called `name`"""
    return 2 * [n for n, _ in TIE_SHIFTS].index(name) + axis


def tie_shift(v):
    s = TIE_SHIFTS[v // 2][1]
    return (s, TIE_OTHER) if v % 2 == 0 else (TIE_OTHER, s)


def tie_problem(pm, V, quantize):
    """(cams, images, params): reference + the first V source views; every view holds the same image, random bytes (fp16 texels) or
    the same bytes plus a random fraction (fp32 texels)"""
    assert len(TIE_SHIFTS) == 16 and V <= 32
    rng = np.random.default_rng(SEED)
    img = rng.integers(0, 256, (TIE_H, TIE_W)).astype(np.float32)
    frac = rng.uniform(0.0625, 0.9375, (TIE_H, TIE_W)).astype(np.float32)
    if not quantize:
        img = img + frac
        img[img > 255.0] = 255.0
    cams = []
    for v in range(-1, V):
        sx, sy = (0.0, 0.0) if v < 0 else tie_shift(v)
        K = [[TIE_K[0][0], 0.0, TIE_K[0][2] + sx], [0.0, TIE_K[1][1], TIE_K[1][2] + sy], [0.0, 0.0, 1.0]]
        cams.append(pm.make_camera(K, np.eye(3), np.zeros(3), TIE_H, TIE_W, *TIE_DEPTHS))
    prm = pm.PatchMatchParams(num_images=V + 1, depth_min=TIE_DEPTHS[0], depth_max=TIE_DEPTHS[1], max_scale=2)
    return cams, [img] * (V + 1), prm


def assert_tie_homographies(h, V):
    """the homography of every source view of handle h is the exact translation by the view's shift, for two different planes"""
    for v in range(V):
        sx, sy = tie_shift(v)
        want = np.array([[1.0, 0.0, sx], [0.0, 1.0, sy], [0.0, 0.0, 1.0]])
        assert np.float32(sx) == sx and np.float32(sy) == sy
        for plane in TIE_PLANES:
            got = h.homography(plane, v).astype(np.float64)
            assert np.array_equal(got, want), f"view {v}, plane {plane}: {got.tolist()}"


def tie_planes(d):
    planes = np.zeros((TIE_H, TIE_W, 4), np.float32)
    planes[..., 2], planes[..., 3] = -1.0, d
    return planes


def bits(a):
    return np.asarray(a).view(np.uint32)


def assert_tie_relations(costs, V, quantize, q8=True):
    """costs: eval_ncc's [V][H][W] of a tie context in 8-bit-fraction arithmetic.  Equal quantised fractions on equal images give
    equal bits, so per axis and k: the views at (k + 0.5) / 256 and at 2^-12 above it agree, the view 2^-12 below differs from
    them (the tie rounds up: floor(a * 256 + 0.5)), and on byte images the view at 255.5 / 256 -- fraction 1.0, the whole weight on
    the next texel -- agrees with the view shifted by one pixel wherever that view sees the pixel (its last column or row projects
    to x = W or y = H, out of view: the sentinel 2.0).
    q8=False: the exact-fraction arithmetic, where the three views of a k all differ (the inputs sit where the quantiser decides).
    Returns the number of (axis, k) groups checked."""
    checked = 0
    for axis in (0, 1):
        for k in TIE_KS:
            lo, mid, hi = (tie_view((k, e), axis) for e in (-1, 0, 1))
            if hi >= V:
                continue
            checked += 1
            what = f"axis {axis}, k {k}"
            if q8:
                assert np.array_equal(bits(costs[mid]), bits(costs[hi])), f"{what}: the tie and the fraction above it differ"
                assert not np.array_equal(bits(costs[lo]), bits(costs[mid])), f"{what}: the tie rounded down"
            else:
                for a, b in ((lo, mid), (mid, hi), (lo, hi)):
                    assert not np.array_equal(bits(costs[a]), bits(costs[b])), f"{what}: views {a} and {b} agree with exact fractions"
        one, last = tie_view("one", axis), tie_view((255, 0), axis)
        if q8 and quantize and one < V:
            seen = np.ones((TIE_H, TIE_W), bool)
            if axis == 0:
                seen[:, -1] = False
            else:
                seen[-1, :] = False
            assert (costs[one][~seen] == 2.0).all() and (costs[last] < 2.0).any()
            assert np.array_equal(bits(costs[last])[seen], bits(costs[one])[seen]), f"axis {axis}: fraction 1.0 is not the next texel"
            checked += 1
    return checked
