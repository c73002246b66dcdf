"""A THIRD statement of the reference's cost formulas, independent of both implementations under test: ComputeHomography,
ComputeCorrespondingPoint, ComputeBilateralWeight and ComputeBilateralNCC (reference src/PatchMatch.cu:228-414) and the texture fetch
they sample through (tex2D with linear filtering about texel centres, clamp addressing; src/PatchMatch.cpp:1003-1020) written out in
float64 numpy straight from the formulas -- no hoisting, no shared reciprocals, no canonical fp32 rules, nothing taken from
oracle/pm_oracle.cpp or the HIP kernels.  The oracle (canonical mode, and its literal fp32 transcription, mode 1) must agree with it to
fp32 accuracy on random evaluations of every kind the kernels meet: planes from the true surface to random, three window scales,
windows that hang over the source border, out-of-view centres, flat windows.

This pins the oracle to the reference's published FORMULAS by a second, differently written evaluation of them; the reference's own
device code, compiled for the host, pins the literal modes bit for bit (tests/test_reference_cpu.py).  It states the formulas and not the
sampler's coordinate rounding: `u` goes straight into the bilinear fetch, whereas the reference's call rounds `u + 0.5f` to fp32 before
the texture unit subtracts the 0.5 again (the literal modes reproduce that since the pinning; the canonical mode omits it by design).  The
tolerances below are unchanged by that."""
import numpy as np
import pytest


def _cam(c):
    return (np.array(c.K, np.float64).reshape(3, 3), np.array(c.R, np.float64).reshape(3, 3), np.array(c.t, np.float64), np.array(c.C, np.float64))


def _tex2d(img, x, y):
    """tex2D<float>(t, x + 0.5, y + 0.5) of an unnormalised, linearly filtered, clamp-addressed texture: bilinear about texel centres at
    the integers, indices clamped to the image"""
    h, w = img.shape
    x0, y0 = np.floor(x), np.floor(y)
    ax, ay = x - x0, y - y0
    xi0, xi1 = int(np.clip(x0, 0, w - 1)), int(np.clip(x0 + 1, 0, w - 1))
    yi0, yi1 = int(np.clip(y0, 0, h - 1)), int(np.clip(y0 + 1, 0, h - 1))
    return (img[yi0, xi0] * (1 - ax) + img[yi0, xi1] * ax) * (1 - ay) + (img[yi1, xi0] * (1 - ax) + img[yi1, xi1] * ax) * ay


def ncc_reference_formulas(cams, imgs, view, plane, px, py, scale, sigma_spatial=5.0, sigma_color=3.0):
    """cost of one (reference pixel, camera-frame plane (n, d), source view) evaluation, float64"""
    Kr, Rr, tr, Cr = _cam(cams[0])
    Ks, Rs, ts, Cs = _cam(cams[view + 1])
    ref, src = np.asarray(imgs[0], np.float64), np.asarray(imgs[view + 1], np.float64)
    n, d = np.asarray(plane[:3], np.float64), float(plane[3])
    # ComputeHomography (:228-279): H = K_s (R_rel - t_rel n^T / d) K_r^-1, K_r^-1 without skew
    R_rel = Rs @ Rr.T
    t_rel = Rs @ (Cr - Cs)
    fx, fy, cx, cy = Kr[0, 0], Kr[1, 1], Kr[0, 2], Kr[1, 2]
    Kr_inv = np.array([[1 / fx, 0, -cx / fx], [0, 1 / fy, -cy / fy], [0, 0, 1.0]])
    Ks_used = np.array([[Ks[0, 0], 0, Ks[0, 2]], [0, Ks[1, 1], Ks[1, 2]], [0, 0, Ks[2, 2]]])   # the entries the reference multiplies (:276-278)
    Hm = Ks_used @ (R_rel - np.outer(t_rel, n) / d) @ Kr_inv

    def warp(x, y):   # ComputeCorrespondingPoint (:281-288)
        q = Hm @ np.array([x, y, 1.0])
        with np.errstate(divide="ignore", invalid="ignore"):
            return q[0] / q[2], q[1] / q[2]

    sh, sw = src.shape
    ctr = warp(px, py)
    if not (0.0 <= ctr[0] < sw and 0.0 <= ctr[1] < sh):   # (:351-353); NaN fails the comparison as in the reference
        return 2.0
    step = 2 << scale            # nSizeStep doubles per scale (:342-346)
    radius = 5 * step // 2
    rc = ref[py, px]
    rh, rw_ = ref.shape
    sw_ = swr = swrr = sws = swss = swrs = 0.0
    for i in range(-radius, radius + 1, step):        # outer loop: x offset (:365)
        for j in range(-radius, radius + 1, step):    # inner loop: y offset (:373)
            r = ref[int(np.clip(py + j, 0, rh - 1)), int(np.clip(px + i, 0, rw_ - 1))]       # exact texel (clamped)
            sx, sy = warp(px + i, py + j)
            if not (np.isfinite(sx) and np.isfinite(sy)):
                return 2.0   # no usable warp: both implementations answer with the sentinel
            s = _tex2d(src, sx, sy)
            wgt = np.exp(-np.sqrt(float(i * i + j * j)) / (2 * sigma_spatial * sigma_spatial) - abs(r - rc) / (2 * sigma_color * sigma_color))   # (:318-323)
            sw_ += wgt
            swr += wgt * r
            swrr += wgt * r * r
            sws += wgt * s
            swss += wgt * s * s
            swrs += wgt * r * s
    inv = 1.0 / sw_
    mr, ms = swr * inv, sws * inv
    var_r, var_s = swrr * inv - mr * mr, swss * inv - ms * ms
    if var_r < 1e-5 or var_s < 1e-5:     # (:406-408)
        return 2.0
    cov = swrs * inv - mr * ms
    return float(min(2.0, max(0.0, 1.0 - cov / np.sqrt(var_r * var_s))))   # (:410-413)


@pytest.mark.parametrize("case", ["frontal", "rotated_cameras", "float_images"])
def test_oracle_ncc_equals_an_independent_float64_statement_of_the_formulas(pm, oracle, case):
    W, H, V = 160, 120, 4
    kw = dict(frontal=dict(rot_deg=2.0, quantize=True), rotated_cameras=dict(rot_deg=10.0, quantize=True, spacing=0.4), float_images=dict(rot_deg=2.0, quantize=False))[case]
    sc = pm.synth.make_problem_scene(W, H, n_src=V, **kw)
    cams, imgs = sc.problem(0, list(range(1, V + 1)))
    dmin, dmax = (float(v) for v in pm.synth.kernel_depth_range(cams[0]))
    h = oracle.create()
    h.set_views(cams, imgs)
    prm = pm.PatchMatchParams(num_images=V + 1, depth_min=dmin, depth_max=dmax, max_scale=0)
    rng = np.random.default_rng(101)
    cam = sc.views[0].cam
    gt = sc.views[0].gt_depth.astype(np.float64)
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    checked = sentinels = 0
    worst = {"canonical": 0.0, "literal": 0.0}
    diffs = {"canonical": [], "literal": []}
    for depth, tilt in ((gt, 0.0), (gt * rng.uniform(0.9, 1.1, gt.shape), 0.4), (rng.uniform(dmin, dmax, gt.shape), 1.0)):
        nrm = np.zeros((H, W, 3))
        nrm[..., 2] = -1.0
        nrm[..., :2] = tilt * rng.normal(size=(H, W, 2))
        nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
        X = np.stack([depth * (u - cam.K[2]) / cam.K[0], depth * (v - cam.K[5]) / cam.K[4], depth], -1)
        planes = np.concatenate([nrm, -(nrm * X).sum(-1)[..., None]], -1).astype(np.float32)
        for scale in (0, 1, 2):
            got = {"canonical": h.eval_ncc(prm, planes, scale), "literal": oracle.eval_ncc_literal(h, prm, planes, scale, mode=1)}
            # random pixels, the image border included (windows that hang over the edges: clamped reference taps, clamped source texels)
            for _ in range(60):
                x, y, view = int(rng.integers(0, W)), int(rng.integers(0, H)), int(rng.integers(0, V))
                want = ncc_reference_formulas(cams, imgs, view, planes[y, x].astype(np.float64), x, y, scale)
                for name in got:
                    g = float(got[name][view, y, x])
                    if (g == 2.0) != (want == 2.0):
                        # the sentinel is decided by a threshold (centre on the border of the source, variance at 1e-5): a disagreement is only
                        # legitimate right AT the threshold -- count it, bound it below
                        sentinels += 1
                        continue
                    diffs[name].append(abs(g - want))
                checked += 1
    assert checked == 3 * 3 * 60
    assert sentinels <= 4, sentinels     # of 1080 comparisons
    for name, d in diffs.items():
        d = np.array(d)
        print(f"{case}: oracle {name} mode vs the float64 formulas over {d.size} evaluations: median {np.median(d):.2e}, 99 % {np.percentile(d, 99):.2e}, max {d.max():.2e}; "
              f"sentinel disagreements {sentinels}")
        # fp32 implementations against float64 formulas: medians at the 1e-6 level, the tail set by ill-conditioned (low-variance, half-clamped) windows
        assert np.median(d) < 2e-5, (name, float(np.median(d)))               # measured 1.5e-6 .. 3.7e-6
        assert np.percentile(d, 99) < 3e-4, (name, float(np.percentile(d, 99)))   # measured <= 5.7e-5
        assert d.max() < 2e-3, (name, float(d.max()))                             # measured <= 1.6e-4
    # the flat-window and out-of-view sentinels, exactly
    flat = [np.full((H, W), 77.0, np.float32) for _ in imgs]
    assert ncc_reference_formulas(cams, flat, 0, planes[60, 80].astype(np.float64), 80, 60, 0) == 2.0
    near = np.array([0.0, 0.0, -1.0, 0.05])   # a plane 5 cm in front of the camera: every source sees it far outside its image
    assert ncc_reference_formulas(cams, imgs, 0, near, 80, 60, 0) == 2.0


def geom_cost_reference_formulas(cams, depth_maps, view, plane, px, py):
    """ComputeGeomConsistencyCost (ref .cu:617-640) with BackProjectPoint2W (:582-603), ProjectPoint (:605-615) and
    ComputeDepthfromPlaneHypothesis (:84-87), float64: forward-project the pixel at the hypothesis' depth, read the source depth at the
    truncated source pixel (clamped fetch), back-project, re-project into the reference view, distance capped at 3"""
    Kr, Rr, tr, Cr = _cam(cams[0])
    Ks, Rs, ts, Cs = _cam(cams[view + 1])
    n, d = np.asarray(plane[:3], np.float64), float(plane[3])

    def backproject(K, R, C, x, y, depth):     # uses fx, fy, cx, cy only; R^T and C
        X = np.array([depth * (x - K[0, 2]) / K[0, 0], depth * (y - K[1, 2]) / K[1, 1], depth])
        return R.T @ X + C

    def project(K, R, t, Pw):                  # the full K
        q = K @ (R @ Pw + t)
        return q[0] / q[2], q[1] / q[2]

    depth = -d * Kr[0, 0] / ((px - Kr[0, 2]) * n[0] + (Kr[0, 0] / Kr[1, 1]) * (py - Kr[1, 2]) * n[1] + Kr[0, 0] * n[2])
    su, sv = project(Ks, Rs, ts, backproject(Kr, Rr, Cr, px, py, depth))
    dm = np.asarray(depth_maps[view], np.float64)
    h, w = dm.shape
    if not (np.isfinite(su) and np.isfinite(sv)):
        return None    # the reference reads an arbitrary texel here: not compared
    xi, yi = int(np.clip(np.trunc(su), 0, w - 1)), int(np.clip(np.trunc(sv), 0, h - 1))   # tex2D(t, (int)x + 0.5, (int)y + 0.5): nearest, clamped
    sd = dm[yi, xi]
    if sd == 0.0:
        return 3.0
    ru, rv = project(Kr, Rr, tr, backproject(Ks, Rs, Cs, su, sv, sd))
    return float(min(3.0, np.hypot(px - ru, py - rv)))


def test_oracle_geometric_cost_equals_an_independent_float64_statement(pm, oracle):
    W, H, V = 160, 120, 3
    sc = pm.synth.make_problem_scene(W, H, n_src=V, spacing=0.3, rot_deg=4.0, focal_jitter=0.05)
    cams, imgs = sc.problem(0, list(range(1, V + 1)))
    h = oracle.create()
    h.set_views(cams, imgs)
    dmin, dmax = (float(v) for v in pm.synth.kernel_depth_range(cams[0]))
    prm = pm.PatchMatchParams(num_images=V + 1, depth_min=dmin, depth_max=dmax)
    rng = np.random.default_rng(7)
    depths = [sc.views[i].gt_depth * (1 + 0.01 * rng.standard_normal((H, W))).astype(np.float32) for i in range(1, V + 1)]
    depths[1][rng.uniform(size=(H, W)) < 0.1] = 0.0
    h.set_src_depths(depths)
    gt = sc.views[0].gt_depth.astype(np.float64)
    cam = sc.views[0].cam
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    diffs, flips, holes = {"canonical": [], "literal": []}, 0, 0
    for noise in (0.0, 0.05, 0.5):
        nrm = np.stack([0.3 * noise * rng.standard_normal((H, W)), 0.3 * noise * rng.standard_normal((H, W)), -np.ones((H, W))], -1)
        nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
        dd = gt * (1 + noise * rng.uniform(-1, 1, (H, W)))
        X = np.stack([dd * (u - cam.K[2]) / cam.K[0], dd * (v - cam.K[5]) / cam.K[4], dd], -1)
        planes = np.concatenate([nrm, -(nrm * X).sum(-1)[..., None]], -1).astype(np.float32)
        got = {"canonical": h.eval_geom(prm, planes), "literal": oracle.eval_geom_literal(h, prm, planes)}
        for _ in range(300):
            x, y, view = int(rng.integers(0, W)), int(rng.integers(0, H)), int(rng.integers(0, V))
            want = geom_cost_reference_formulas(cams, depths, view, planes[y, x].astype(np.float64), x, y)
            if want is None:
                continue
            holes += want == 3.0
            for name in got:
                g = float(got[name][view, y, x])
                if abs(g - want) > 0.05:
                    flips += 1      # the nearest-texel read lands on the neighbouring texel: a discontinuity of the formula itself
                else:
                    diffs[name].append(abs(g - want))
    assert holes > 20                     # caps and holes were among the samples
    assert flips <= 6, flips              # of 1800 comparisons: coordinates within fp32 rounding of an integer
    for name, d in diffs.items():
        d = np.array(d)
        print(f"geometric cost, oracle {name} vs the float64 formulas over {d.size} checks: median {np.median(d):.2e} px, 99 % {np.percentile(d, 99):.2e}, max {d.max():.2e}")
        assert np.median(d) < 5e-5 and np.percentile(d, 99) < 2e-3, (name, float(np.median(d)), float(np.percentile(d, 99)))


def test_initial_cost_and_selected_views_from_the_cost_vector(pm, oracle):
    """ComputeMultiViewInitialCostandSelectedViews (ref .cu:497-534) restated on the oracle's own per-view costs: sort the V costs,
    top_k = min(number of costs below 2, 4), cost = mean of the top_k smallest (fp32, summed in ascending order), mask = views whose
    cost is <= the k-th smallest; 2.0 and an empty mask if no view is valid.  InitializeScore's output (costs, selected views) must
    equal that exactly, at the window scale Run() initialises with."""
    W, H, V = 120, 90, 6
    sc = pm.synth.make_problem_scene(W, H, n_src=V, spacing=0.4, rot_deg=3.0, quantize=True)
    cams, imgs = sc.problem(0, list(range(1, V + 1)))
    h = oracle.create()
    h.set_views(cams, imgs)
    dmin, dmax = (float(v) for v in pm.synth.kernel_depth_range(cams[0]))
    for scale in (0, 2):
        prm = pm.PatchMatchParams(num_images=V + 1, depth_min=dmin, depth_max=dmax, max_scale=scale)
        h.step(prm, 5, pm.KIND_INIT, 0, scale, 0)             # random planes (photometric mode)
        planes, costs = h.get()                                 # raw state: camera-frame planes
        sel = h.get_selected_views()
        cv = h.eval_ncc(prm, planes, scale)                     # [V][H][W]
        srt = np.sort(cv, axis=0)
        n_valid = (cv < 2.0).sum(0)
        k = np.minimum(n_valid, 4)
        want_cost = np.full((H, W), 2.0, np.float32)
        want_sel = np.zeros((H, W), np.uint32)
        for kk in range(1, 5):
            m = k == kk
            acc = np.zeros((H, W), np.float32)
            for i in range(kk):
                acc = (acc + srt[i]).astype(np.float32)
            want_cost[m] = (acc / np.float32(kk))[m]
            thr = srt[kk - 1]
            bits = np.zeros((H, W), np.uint32)
            for v in range(V):
                bits |= (cv[v] <= thr).astype(np.uint32) << np.uint32(v)
            want_sel[m] = bits[m]
        assert (k == 0).sum() < 0.2 * W * H and (k == 4).sum() > 0.3 * W * H
        assert np.array_equal(costs, want_cost), f"scale {scale}: {int((costs != want_cost).sum())} costs differ"
        assert np.array_equal(sel, want_sel), f"scale {scale}: {int((sel != want_sel).sum())} masks differ"
