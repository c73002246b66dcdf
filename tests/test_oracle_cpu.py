"""CPU tests of the oracle (the checker itself): known answers for each function
of the path, the reference's quirks, and convergence to analytic ground truth.

The reference holds no tests or golden vectors for this path
and cannot be built here, so the oracle is "parity unpinned" against reference
outputs; these tests pin it to analytic facts and to the committed fixtures in
tests/golden/ (regression pins of the oracle's own outputs).
"""
import numpy as np
import pytest

SEED = 12345
# The bars of the canonical geometric check against the reference's literal chain (test_geom_cost_canonical_vs_literal), by name:
# tests/ref_common.py applies the same ones against the reference's own compiled code.
GEOM_CAP_DISAGREEMENT = 1e-4   # share of the checks whose cap / hole decision may differ
GEOM_MEDIAN = 5e-5             # px
GEOM_P999 = 5e-4               # px, 99.9th percentile
GEOM_TEXEL_FLIP = 5e-3         # px: beyond this the nearest-texel read landed on the neighbouring texel ...
GEOM_TEXEL_FLIP_SHARE = 1e-4   # ... at most this share of the checks


def _scene(pm, oracle, W=96, H=64, V=3, spacing=0.5, rot_deg=2.0):
    sc = pm.synth.make_problem_scene(W, H, n_src=V, spacing=spacing, rot_deg=rot_deg)
    cams, imgs = sc.problem(0, list(range(1, V + 1)))
    h = oracle.create()
    h.set_views(cams, imgs)
    dmin, dmax = pm.synth.kernel_depth_range(cams[0])
    prm = pm.PatchMatchParams(num_images=V + 1, depth_min=float(dmin), depth_max=float(dmax), max_scale=0)
    return sc, h, prm


# ---------------------------------------------------------------------------
# canonical math against libm (accuracy of the specification itself)
# ---------------------------------------------------------------------------
def _ulp_err(got, want64):
    want = want64.astype(np.float32)
    ulp = np.spacing(np.abs(want)).astype(np.float64)
    return np.abs(got.astype(np.float64) - want64) / np.maximum(ulp, 1e-45)


def test_det_math_accuracy(pm, oracle):
    f = oracle.fns()
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.uniform(-3000, 3000, 100000), rng.uniform(-2, 2, 100000)]).astype(np.float32)
    x = x[x != 0]
    assert _ulp_err(pm._abi.math_probe(f, 0, x), 1.0 / x.astype(np.float64)).max() <= 2.0
    x = rng.uniform(-79.0, 3.0, 200000).astype(np.float32)
    assert _ulp_err(pm._abi.math_probe(f, 1, x), np.exp(x.astype(np.float64))).max() <= 2.0
    x = rng.uniform(-0.78, 0.78, 200000).astype(np.float32)
    assert _ulp_err(pm._abi.math_probe(f, 2, x), np.sin(x.astype(np.float64))).max() <= 2.0
    assert _ulp_err(pm._abi.math_probe(f, 3, x), np.cos(x.astype(np.float64))).max() <= 2.0
    x = rng.uniform(-1.0, 1.0, 200000).astype(np.float32)
    err = np.abs(pm._abi.math_probe(f, 4, x).astype(np.float64) - np.arccos(x.astype(np.float64)))
    assert err.max() < 1e-6


def test_det_math_special_values(pm, oracle):
    f = oracle.fns()
    e = pm._abi.math_probe(f, 1, np.array([0.0, -80.5, -1e9, np.nan, 81.0], np.float32))
    assert e[0] == 1.0 and e[1] == 0.0 and e[2] == 0.0 and np.isnan(e[3]) and np.isinf(e[4])
    a = pm._abi.math_probe(f, 4, np.array([1.0000001, -1.0000001, np.nan, 1.0, -1.0, 0.0], np.float32))
    assert np.isnan(a[:3]).all()  # the reference relies on acos(>1) = NaN (ref .cu:704)
    assert a[3] == 0.0 and abs(a[4] - np.pi) < 1e-6 and abs(a[5] - np.pi / 2) < 1e-6


def test_rng_stream_properties(pm, oracle):
    f = oracle.fns()
    u = pm._abi.rng_probe(f, SEED, 77, 3, 4096)
    assert u.min() > 0.0 and u.max() <= 1.0          # curand_uniform's (0, 1] (ref .cu:200)
    assert abs(u.mean() - 0.5) < 0.02 and abs(u.var() - 1 / 12) < 0.005
    assert np.array_equal(u, pm._abi.rng_probe(f, SEED, 77, 3, 4096))
    assert not np.array_equal(u[:64], pm._abi.rng_probe(f, SEED, 78, 3, 64))
    assert not np.array_equal(u[:64], pm._abi.rng_probe(f, SEED, 77, 4, 64))
    assert not np.array_equal(u[:64], pm._abi.rng_probe(f, SEED + 1, 77, 3, 64))


def test_philox_known_answer(pm, oracle):
    """Philox4x32-10 known-answer vector from the Random123 distribution
    (counter = key = 0 -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8); the oracle's
    counter layout is (pix, launch, block, tag) so the KAT is checked on a
    Python restatement, and the oracle stream against that restatement."""
    def philox(c, k):
        c = list(c)
        k = list(k)
        for _ in range(10):
            p0 = 0xD2511F53 * c[0]
            p1 = 0xCD9E8D57 * c[2]
            c = [((p1 >> 32) ^ c[1] ^ k[0]) & 0xFFFFFFFF, p1 & 0xFFFFFFFF, ((p0 >> 32) ^ c[3] ^ k[1]) & 0xFFFFFFFF, p0 & 0xFFFFFFFF]
            k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
        return c
    assert philox([0, 0, 0, 0], [0, 0]) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert philox([0xffffffff] * 4, [0xffffffff] * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    seed, pix, launch = (0xABCDEF01 << 32) | 0x12345678, 4242, 9
    want = []
    for blk in range(3):
        for w in philox([pix, launch, blk, 0x4D504D56], [seed & 0xFFFFFFFF, seed >> 32]):
            want.append(np.float32(((w >> 8) + 1)) * np.float32(2.0 ** -24))
    got = pm._abi.rng_probe(oracle.fns(), seed, pix, launch, 12)
    assert np.array_equal(got, np.array(want, np.float32))


# ---------------------------------------------------------------------------
# geometry known answers
# ---------------------------------------------------------------------------
def test_homography_maps_plane_points(pm, oracle):
    """H(plane) must send a reference pixel to the projection, in the source
    view, of the 3-D point where its ray meets the plane (ref .cu:228-288)."""
    sc, h, prm = _scene(pm, oracle)
    v0 = sc.views[0]
    rng = np.random.default_rng(3)
    for v in range(3):
        vs = sc.views[v + 1]
        for _ in range(20):
            n = rng.normal(size=3)
            n[2] = -abs(n[2]) - 0.5
            n /= np.linalg.norm(n)
            u, w = rng.uniform(0, 95), rng.uniform(0, 63)
            depth = rng.uniform(3.5, 7.0)
            Xc = np.array([depth * (u - v0.K[0, 2]) / v0.K[0, 0], depth * (w - v0.K[1, 2]) / v0.K[1, 1], depth])
            d = -n @ Xc
            Hm = h.homography(np.array([*n, d], np.float32), v).astype(np.float64)
            q = Hm @ np.array([u, w, 1.0])
            Xw = v0.R.T @ Xc + v0.C
            Xs = vs.R @ (Xw - vs.C)
            want = vs.K @ Xs
            assert np.allclose(q[:2] / q[2], want[:2] / want[2], atol=2e-2), (q[:2] / q[2], want[:2] / want[2])


def test_ncc_identical_views_cost_zero(pm, oracle):
    """two identical cameras: any plane warps by the identity, so the bilateral
    NCC of a textured window is 0 and of a flat window the sentinel 2
    (variance < 1e-5, ref .cu:406-408)"""
    sc = pm.synth.make_problem_scene(64, 48, n_src=1, rot_deg=0.0)
    v0 = sc.views[0]
    img = v0.image.copy()
    img[:, 40:] = 100.0  # flat region
    cams, imgs = [v0.cam, v0.cam], [img, img]
    h = oracle.create()
    h.set_views(cams, imgs)
    prm = pm.PatchMatchParams(num_images=2, depth_min=2.0, depth_max=9.0)
    planes = np.zeros((48, 64, 4), np.float32)
    planes[..., 2] = -1.0
    planes[..., 3] = 5.0
    c = h.eval_ncc(prm, planes, 0)[0]
    assert np.abs(c[8:40, 8:30]).max() < 1e-4 and np.abs(c[8:40, 8:30]).mean() < 1e-5
    assert np.all(c[10:38, 50:60] == 2.0)


def test_ncc_out_of_view_sentinel(pm, oracle):
    sc, h, prm = _scene(pm, oracle)
    planes = np.zeros((64, 96, 4), np.float32)
    planes[..., 2] = -1.0
    planes[..., 3] = 0.05  # 5 cm in front of the camera: projects far outside every source
    c = h.eval_ncc(prm, planes, 0)
    assert np.all(c == 2.0)  # ref .cu:351-353


def test_geom_cost_zero_on_consistent_depth(pm, oracle):
    """forward/backward reprojection through the true source depth returns to
    the start pixel: cost ~ 0 (ref .cu:617-640); holes give the cap 3"""
    sc, h, prm = _scene(pm, oracle, W=160, H=120, V=2, spacing=0.3, rot_deg=1.0)
    depths = [sc.views[1].gt_depth.copy(), np.zeros_like(sc.views[2].gt_depth)]
    h.set_src_depths(depths)
    cam = sc.views[0].cam
    gt = sc.views[0].gt_depth.astype(np.float64)
    H, W = gt.shape
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    planes = np.zeros((H, W, 4), np.float32)
    planes[..., 2] = -1.0
    planes[..., 3] = gt  # fronto-parallel plane through the true point: n.X + d = 0 with n = (0,0,-1)
    g = h.eval_geom(prm, planes)
    assert np.median(g[0, 10:-10, 10:-10]) < 0.15  # nearest-texel depth lookup -> sub-pixel residual
    assert np.all(g[1] == 3.0)


def test_geom_cost_canonical_vs_literal(pm, oracle):
    """the canonical geometric check (two composed projective maps, no division: DESIGN.md 3.8) against the reference's literal
    chain through world coordinates (ref .cu:582-640), on planes from the true surface to fully random, rotated cameras with
    per-view intrinsics, noisy and partly missing source depth maps.  The term enters a cost with weight 0.2: north_star's 1e-3
    on costs allows 5e-3 px here; 99.9 % of the checks agree to 1e-4 px."""
    W, H, V = 200, 150, 4
    sc = pm.synth.make_problem_scene(W, H, n_src=V, spacing=0.3, rot_deg=3.0, focal_jitter=0.05)
    cams, imgs = sc.problem(0, list(range(1, V + 1)))
    import copy
    cams = [copy.copy(c) for c in cams]
    for i, c in enumerate(cams):
        # a full K: skew and a small off-diagonal term -- ProjectPoint uses all nine entries (ref .cu:612-614), BackProjectPoint2W
        # only fx, fy, cx, cy (:587-589); the composed maps must treat each camera the same two ways
        c.K[1] = 0.7 + 0.1 * i
        c.K[3] = 0.02 * (i + 1)
    h = oracle.create()
    h.set_views(cams, imgs)
    dmin, dmax = pm.synth.kernel_depth_range(cams[0])
    prm = pm.PatchMatchParams(num_images=V + 1, depth_min=float(dmin), depth_max=float(dmax))
    rng = np.random.default_rng(3)
    depths = [sc.views[i].gt_depth * (1 + 0.01 * rng.standard_normal((H, W))).astype(np.float32) for i in range(1, V + 1)]
    depths[1][rng.uniform(size=(H, W)) < 0.1] = 0.0
    h.set_src_depths(depths)
    gt = sc.views[0].gt_depth
    stats = []
    for noise in (0.0, 0.02, 0.5):
        planes = np.zeros((H, W, 4), np.float32)
        n = np.stack([0.3 * noise * rng.standard_normal((H, W)), 0.3 * noise * rng.standard_normal((H, W)), -np.ones((H, W))], -1)
        n /= np.linalg.norm(n, axis=-1, keepdims=True)
        d = gt * (1 + noise * rng.uniform(-1, 1, (H, W)))
        cam = cams[0]
        u, v = np.meshgrid(np.arange(W), np.arange(H))
        X = np.stack([d * (u - cam.K[2]) / cam.K[0], d * (v - cam.K[5]) / cam.K[4], d], -1)
        planes[..., :3] = n
        planes[..., 3] = -(n * X).sum(-1)
        can = h.eval_geom(prm, planes)
        lit = oracle.eval_geom_literal(h, prm, planes)
        assert np.mean((can == 3.0) != (lit == 3.0)) < GEOM_CAP_DISAGREEMENT   # the cap / hole decisions agree
        both = (can < 3.0) & (lit < 3.0)
        dd = np.abs(can - lit)[both]
        # the depth texel is the NEAREST one (truncation, ref .cu:626): a coordinate that differs in its last bits across an
        # integer boundary reads the neighbouring texel -- a discontinuity of the reference's own formula, which any second
        # arithmetic (the reference's --use_fast_math build included) trips at the same rate; everything else agrees to 1e-4 px
        stats.append((noise, float(np.median(dd)), float(np.percentile(dd, 99.9)), float((dd > GEOM_TEXEL_FLIP).mean()), float(dd.max())))
        assert np.median(dd) < GEOM_MEDIAN and np.percentile(dd, 99.9) < GEOM_P999 and (dd > GEOM_TEXEL_FLIP).mean() < GEOM_TEXEL_FLIP_SHARE
    print("\ngeometric check, canonical vs literal (px; x 0.2 in the cost): " +
          "; ".join(f"plane noise {a}: median {b:.1e}, 99.9 % {c:.1e}, texel flips {d:.1e} of the checks (max {e:.2f})" for a, b, c, d, e in stats))


# ---------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------
def test_init_random_planes_face_camera_in_range(pm, oracle):
    sc, h, prm = _scene(pm, oracle)
    h.step(prm, SEED, pm.KIND_INIT, 0, 0, 0)
    planes, costs = h.get()
    cam = sc.views[0].cam
    H, W = costs.shape
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    n = planes[..., :3].astype(np.float64)
    assert np.allclose(np.linalg.norm(n, axis=-1), 1.0, atol=1e-5)
    view = np.stack([(u - cam.K[2]) / cam.K[0], (v - cam.K[5]) / cam.K[4], np.ones_like(u, float)], -1)
    assert np.all((n * view).sum(-1) <= 1e-6)                      # ref .cu:210-216
    depth = -planes[..., 3] / (n * view).sum(-1)
    assert depth.min() >= prm.depth_min - 1e-3 and depth.max() <= prm.depth_max + 1e-3
    sel = h.get_selected_views()
    assert np.all(sel < 8) and np.all((costs >= 0) & (costs <= 2))
    assert np.all((sel == 0) == (costs == 2.0))                    # ref .cu:518-533


def test_checkerboard_touches_one_colour(pm, oracle):
    sc, h, prm = _scene(pm, oracle)
    h.step(prm, SEED, pm.KIND_INIT, 0, 0, 0)
    p0, c0 = h.get()
    h.step(prm, SEED, pm.KIND_BLACK, 0, 0, 1)
    p1, c1 = h.get()
    yy, xx = np.mgrid[0:64, 0:96]
    red = (xx + yy) % 2 == 1
    assert np.array_equal(p0[red], p1[red]) and np.array_equal(c0[red], c1[red])
    assert (p0[~red] != p1[~red]).any()


def test_uncovered_last_row_quirk(pm, oracle):
    """H = 33: H/2 = 16 is a multiple of 16, the reference grid stops at row 31
    (ref .cu:1196, SURVEY a-9 ii)"""
    sc, h, prm = _scene(pm, oracle, W=64, H=33, V=2)
    h.step(prm, SEED, pm.KIND_INIT, 0, 0, 0)
    p0, c0 = h.get()
    h.step(prm, SEED, pm.KIND_BLACK, 0, 0, 1)
    h.step(prm, SEED, pm.KIND_RED, 0, 0, 2)
    p1, c1 = h.get()
    assert np.array_equal(p0[32], p1[32]) and np.array_equal(c0[32], c1[32])
    assert not np.array_equal(p0[31], p1[31])


def test_border_pixels_do_not_propagate(pm, oracle):
    """unflagged regions carry cost 0 (the `= {2.0f}` initialiser, ref .cu:795)
    so within 5 px of the border no neighbour can win: the plane changes only
    through refinement, which keeps the depth within 2 % or draws uniformly"""
    sc, h, prm = _scene(pm, oracle)
    h.step(prm, SEED, pm.KIND_INIT, 0, 0, 0)
    h.step(prm, SEED, pm.KIND_BLACK, 0, 0, 1)
    p1, c1 = h.get()
    assert np.isfinite(p1).all()


def test_median_filter_known_answer(pm, oracle):
    sc, h, prm = _scene(pm, oracle, W=32, H=32, V=1)
    rng = np.random.default_rng(4)
    planes = np.zeros((32, 32, 4), np.float32)
    planes[..., 3] = rng.uniform(1, 9, (32, 32))
    costs = np.full((32, 32), 0.5, np.float32)
    costs[10, 10] = 0.0  # skipped: cost < 0.001 (ref .cu:1067)
    h.set_state(planes, costs)
    h.step(prm, SEED, pm.KIND_FILTER_BLACK, 0, 0, 0)
    out, _ = h.get()
    d = planes[..., 3]
    offs = [(0, 0), (-1, 0), (-3, 0), (-5, 0), (1, 0), (3, 0), (5, 0), (0, -1), (0, -3), (0, -5), (0, 1), (0, 3), (0, 5),
            (-1, 2), (1, 2), (-1, -2), (1, -2), (-2, -1), (-2, 1), (2, -1), (2, 1)]  # (dy, dx), interior pixel
    for (y, x) in [(16, 16), (12, 20)]:
        vals = sorted(d[y + dy, x + dx] for dy, dx in offs)
        assert out[y, x, 3] == vals[10]
    assert out[10, 10, 3] == d[10, 10]
    assert np.array_equal(out[..., 3][1::2, 0::2], d[1::2, 0::2])  # red pixels untouched
    # corner pixel (0,0): centre + 3 down + 3 right + (1,2) + (2,1) = 9 taps
    vals = sorted([d[0, 0], d[1, 0], d[3, 0], d[5, 0], d[0, 1], d[0, 3], d[0, 5], d[1, 2], d[2, 1]])
    assert out[0, 0, 3] == vals[4]


def test_depth_normal_conversion(pm, oracle):
    sc, h, prm = _scene(pm, oracle)
    h.step(prm, SEED, pm.KIND_INIT, 0, 0, 0)
    p0, _ = h.get()
    h.step(prm, SEED, pm.KIND_DEPTH_NORMAL, 0, 0, 1)
    p1, _ = h.get()
    v0 = sc.views[0]
    nw = p0[..., :3].astype(np.float64) @ v0.R  # R^T n, row-vector form
    assert np.allclose(p1[..., :3], nw, atol=1e-6)
    assert p1[..., 3].min() >= prm.depth_min - 1e-3 and p1[..., 3].max() <= prm.depth_max + 1e-3


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------
def test_run_converges_to_ground_truth(pm, oracle):
    sc, h, prm = _scene(pm, oracle, W=160, H=120, V=4, spacing=0.4, rot_deg=1.0)
    h.run(prm, SEED)
    planes, costs = h.get()
    gt = sc.views[0].gt_depth
    rel = np.abs(planes[..., 3] - gt) / gt
    assert (rel < 0.02).mean() > 0.85
    assert costs.mean() < 0.2
    # determinism: same seed, same bits; another seed, another result
    h2 = oracle.create()
    cams, imgs = sc.problem(0, [1, 2, 3, 4])
    h2.set_views(cams, imgs)
    h2.run(prm, SEED)
    assert np.array_equal(h2.get()[0], planes)
    h2.run(prm, SEED + 1)
    assert not np.array_equal(h2.get()[0], planes)


def test_thread_count_does_not_change_results(pm, oracle):
    sc, h, prm = _scene(pm, oracle, W=64, H=48, V=2)
    n = oracle.num_threads()
    h.run(prm, SEED)
    a = h.get()[0].copy()
    oracle.set_num_threads(1)
    try:
        h.run(prm, SEED)
        b = h.get()[0]
    finally:
        oracle.set_num_threads(n)
    assert np.array_equal(a, b)  # red/black split is race free


def test_geom_and_prior_modes_run(pm, oracle):
    sc, h, prm = _scene(pm, oracle, W=96, H=64, V=3)
    h.run(prm, SEED)
    planes, costs = h.get()
    gt0 = sc.views[0].gt_depth
    err0 = np.abs(planes[..., 3] - gt0) / gt0
    h.set_src_depths([sc.views[i].gt_depth for i in (1, 2, 3)])
    prm.geom_consistency = True
    prm.max_iterations = 2
    h.run(prm, SEED + 1)
    p2, c2, g2 = h.get(geom=True)
    err2 = np.abs(p2[..., 3] - gt0) / gt0
    assert (err2 < 0.05).mean() >= (err0 < 0.05).mean() - 0.02
    assert g2.min() >= 0 and g2.max() <= 0.6 + 1e-6  # 0.2 * min(3, .) (ref .cu:687)
    with pytest.raises(RuntimeError, match="prior"):
        prm.planar_prior = True
        h.run(prm, SEED)


def test_canonical_vs_literal_arithmetic(pm, oracle):
    """the canonical arithmetic (hoisted homography, one reciprocal per
    window column, own exp, explicit fma) must stay within north_star's 1e-3 of a LITERAL
    transcription of the reference's formulas (per-evaluation homography with its
    divisions, per-tap division, libm expf).  Costs live in [0, 2], so 1e-3 absolute.
    CUDA's 8-bit texture fractions are a property of the hardware sampler the
    reference uses, not of its formulas: their effect is reported, not bounded."""
    sc, h, prm = _scene(pm, oracle, W=160, H=120, V=4, spacing=0.3, rot_deg=2.0)
    cam = sc.views[0].cam
    rng = np.random.default_rng(11)
    H, W = 120, 160
    gt = sc.views[0].gt_depth.astype(np.float64)
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    for trial, (depth, tilt) in enumerate([(gt, 0.0), (gt * rng.uniform(0.9, 1.1, gt.shape), 0.3), (rng.uniform(prm.depth_min, prm.depth_max, gt.shape), 1.0)]):
        n = np.zeros((H, W, 3))
        n[..., 2] = -1.0
        n[..., :2] = tilt * rng.normal(size=(H, W, 2))
        n /= np.linalg.norm(n, axis=-1, keepdims=True)
        X = np.stack([depth * (u - cam.K[2]) / cam.K[0], depth * (v - cam.K[5]) / cam.K[4], depth], -1)
        planes = np.concatenate([n, -(n * X).sum(-1)[..., None]], -1).astype(np.float32)
        for scale in (0, 2):
            can = h.eval_ncc(prm, planes, scale)
            lit = oracle.eval_ncc_literal(h, prm, planes, scale)
            both = (can < 2.0) & (lit < 2.0)
            assert both.mean() > 0.3
            assert ((can == 2.0) != (lit == 2.0)).mean() < 2e-3      # window centre on the image border / variance threshold
            diff = np.abs(can - lit)[both]
            assert diff.max() < 1e-3, (trial, scale, diff.max())
            assert np.median(diff) < 5e-5    # fma vs separate rounding in E[x^2] - E[x]^2
    # CUDA texture fraction quantisation (for the record)
    q = oracle.eval_ncc_literal(h, prm, planes, 0, quantize_fraction=True)
    lit = oracle.eval_ncc_literal(h, prm, planes, 0)
    both = (q < 2.0) & (lit < 2.0)
    assert np.median(np.abs(q - lit)[both]) < 5e-3


def test_end_to_end_statistics_canonical_vs_literal(pm, oracle):
    """SURVEY 8c tier T3: the whole Run() schedule (random init, 2 window scales x 3 red/black iterations, view selection,
    refinement, filter) with EVERY NCC evaluation in (a) the canonical arithmetic the HIP kernels implement, (b) the
    reference's literal operation order with libm, (c) literal + CUDA's 8-bit texture fractions.  Individual decisions
    differ (ties flip, then the random walks diverge), the statistics must not: accuracy against the analytic ground truth
    within +-2 percentage points (seed-to-seed scatter is +-1), mean matching cost within 2 %."""
    ob = oracle
    sc = pm.synth.make_problem_scene(160, 120, 4, quantize=True)
    cams, imgs = sc.problem(0, [1, 2, 3, 4])
    gt = sc.views[0].gt_depth
    dmin, dmax = pm.synth.kernel_depth_range(cams[0])
    stats = {}
    for mode in (0, 1, 2):
        acc1, acc3, cost = [], [], []
        for seed in (1, 2):
            h = ob.create()
            h.set_views(cams, imgs)
            ob.set_literal_mode(h, mode)
            h.run(pm.PatchMatchParams(num_images=5, depth_min=float(dmin), depth_max=float(dmax), max_scale=1), seed)
            planes, costs = h.get()
            rel = np.abs(planes[..., 3] - gt) / gt
            acc1.append((rel < 0.01).mean())
            acc3.append((rel < 0.03).mean())
            cost.append(costs.mean())
        stats[mode] = (np.mean(acc1), np.mean(acc3), np.mean(cost))
    assert stats[0][1] > 0.8                                           # the schedule converges on this scene
    for mode in (1, 2):
        assert abs(stats[mode][0] - stats[0][0]) < 0.02 and abs(stats[mode][1] - stats[0][1]) < 0.02, stats
        assert abs(stats[mode][2] / stats[0][2] - 1.0) < 0.02, stats


def test_refinement_rejection_rules_hold_in_fp32(pm, oracle):
    """The arithmetic facts behind the exact early rejection of refinement candidates in k_update (pm_kernels.hpp; DESIGN.md
    section 5), checked on random data in the very fp32 operations the kernel and the oracle use.

    (1) Non-masked pixels: terms w * c are >= 0 and summed in sequence; T = fl(cost * norm) + 1 ulp.  Whenever a partial sum has
        reached T, the final quotient fl(sum / norm) is >= cost, i.e. the reference's `tc < cost_now` is false.
    (2) Masked prior pixels with a raised restricted cost rc: whenever fl(pr * 1.000001) <= rc, the reference's
        `exp(-tc^2 / beta) * pr > rc` is false for every tc in [0, 2.6] (the canonical exp is within 2 ulp and <= 1 + 2 ulp there)."""
    rng = np.random.default_rng(42)
    f32 = np.float32
    n, V = 200000, 8
    w = rng.integers(0, 5, size=(n, V)).astype(f32)
    w[:, 0] = np.maximum(w[:, 0], 1)
    c = (rng.uniform(0.0, 2.0, size=(n, V)) ** rng.choice([1.0, 3.0], size=(n, 1))).astype(f32)
    norm = w.sum(1, dtype=f32)
    cost = rng.uniform(0.0, 1.2, n).astype(f32)
    T = (cost * norm).view(np.uint32) + np.uint32(1)
    T = T.view(f32)
    s = np.zeros(n, f32)
    reached = np.zeros(n, bool)
    for v in range(V):
        s = (s + w[:, v] * c[:, v]).astype(f32)
        reached |= s >= T
    tc = (s / norm).astype(f32)
    assert reached.any() and (~reached).any()
    assert not (tc[reached] < cost[reached]).any()
    # (2)
    beta = f32(0.18)
    pr = rng.uniform(0.5, 1.5, n).astype(f32)
    rc = (pr * rng.uniform(0.98, 1.02, n)).astype(f32)                    # right around the prior term: the interesting zone
    tcs = np.concatenate([np.zeros(n // 2, f32), rng.uniform(0.0, 2.6, n - n // 2).astype(f32)])
    x = (-(tcs * tcs) / beta).astype(f32)
    e = pm._abi.math_probe(oracle.fns(), 1, x)
    rtc = (e * pr).astype(f32)
    dead = ~((pr * f32(1.000001)).astype(f32) > rc)
    assert dead.any() and (~dead).any()
    assert not (rtc[dead] > rc[dead]).any()
    assert e.max() <= np.nextafter(np.nextafter(f32(1.0), f32(2.0)), f32(2.0))


def test_T2_flip_rates_against_the_references_own_noise_floor(pm, oracle):
    """SURVEY 8c tier T2 with its control, on the CPU (tests/test_literal_gpu.py runs the same with the HIP path in the role of
    mode 0): one BlackPixelUpdate from an identical state in the canonical arithmetic (mode 0 = what the kernels compute, bit for
    bit) and in the measurement modes of the WHOLE path -- 1 the reference's formulas with IEEE operations and libm, 4 the same
    formulas as a --use_fast_math build computes them (approximate exp / reciprocal / sin / cos, contracted multiply-adds),
    2 with the texture hardware's 8-bit fractions.  The pixels whose depth then differs by more than 1e-3 are decision flips
    (threshold counts, sampled views, acceptance tests on costs that differ by 1e-4).  The canonical arithmetic must not flip
    more than 1.5 x what the reference's formulas flip against themselves under fast-math arithmetic alone."""
    W, H, V = 320, 240, 6
    sc = pm.synth.make_problem_scene(W, H, n_src=V, quantize=True)
    cams, imgs = sc.problem(0, list(range(1, V + 1)))
    dmin, dmax = (float(v) for v in pm.synth.kernel_depth_range(cams[0]))
    h = oracle.create()
    h.set_views(cams, imgs)
    rng = np.random.default_rng(5)
    h.set_src_depths([sc.views[i].gt_depth * (1.0 + 0.005 * rng.standard_normal((H, W))).astype(np.float32) for i in range(1, V + 1)])
    prior = np.zeros((H, W, 4), np.float32)
    prior[..., 2] = -1.0
    prior[..., 3] = sc.views[0].gt_depth
    h.set_prior(prior, (rng.uniform(size=(H, W)) < 0.6).astype(np.uint32))

    def flips(a, b):
        return float((np.abs(a[..., 3] - b[..., 3]) / np.maximum(np.abs(b[..., 3]), 1e-6) > 1e-3).mean())

    report = []
    for name, geom, planar in (("photometric", False, False), ("geometric", True, False), ("prior", False, True)):
        prm = pm.PatchMatchParams(num_images=V + 1, depth_min=dmin, depth_max=dmax, max_scale=0, geom_consistency=geom, planar_prior=planar)
        h.run(pm.PatchMatchParams(num_images=V + 1, depth_min=dmin, depth_max=dmax, max_scale=0), 7)
        s_planes, s_costs = h.get()
        after = {}
        for mode in (0, 1, 2, 4):
            oracle.set_literal_mode(h, mode)
            try:
                h.set_state(s_planes, s_costs)
                h.step(prm, 11, pm.KIND_INIT, 0, 0, 0)
                h.step(prm, 11, pm.KIND_BLACK, 0, 0, 1)
                after[mode] = h.get()[0]
            finally:
                oracle.set_literal_mode(h, 0)
        canonical, fastmath, tex8 = flips(after[0], after[1]), flips(after[4], after[1]), flips(after[2], after[1])
        report.append(f"{name}: canonical vs literal {canonical:.2e}, literal vs fast-math arithmetic {fastmath:.2e}, literal vs 8-bit fractions {tex8:.2e}")
        assert fastmath > 0 and canonical <= 1.5 * fastmath, report[-1]
        assert canonical <= tex8, report[-1]
    print("\nT2 flip rates after one BlackPixelUpdate: " + "; ".join(report))
