"""north_star's tolerance tested ON THE GPU against the closest thing to the reference's own formulas that can run here: the
oracle's LITERAL transcription of ComputeBilateralNCC (reference src/PatchMatch.cu:228-414: homography assembled per
evaluation with its divisions, one perspective division per tap, libm expf/sqrtf, row-by-row sums, nothing hoisted), mode 1,
and the same with CUDA's 8-bit texture interpolation fractions, mode 2 (`orc_set_literal_mode`).  The canonical arithmetic the
HIP kernels implement is bit-exact against the oracle's canonical mode (tests/test_parity_gpu.py); these
tests bound its distance to the literal formulas.

T1  NCC costs (range [0, 2]) on a 400x300 cfg-1 scene, 8 views, window scales 0..2, planes from the true surface to fully
    random.  Against the literal formulas (mode 1) the bar is north_star's 1e-3: at most 1e-5 of the evaluations may exceed it
    (measured on the MI355X since literal_tex rounds `x + 0.5f` as the reference's call does, profiles/r06_literal_modes.txt: none of 7.9 M, maximum 9.95e-4), none 2e-3.  CUDA's
    8-bit fractions (mode 2) are a property of the sampler hardware, not of the formulas: they alone move costs by up to
    2e-3, so that bar is 99.9 % within 1e-3 and none beyond 3e-3.
T2  one kernel step from an identical state (SURVEY 8c tier T2): InitializeScore and one BlackPixelUpdate in each of the three
    modes, HIP path against the oracle computing the WHOLE step literally (round 4: every libm call, division and the geometric
    chain, not only the NCC).  Costs differ at the 1e-4 level, so a threshold count, a sampled view, an arg-min or an acceptance
    test can flip at a pixel, and that pixel then carries a different -- equally good -- plane.  How many pixels that is, is
    measured against a CONTROL: the reference's formulas in IEEE arithmetic against the same formulas as the reference's own
    build computes them (mode 4: a model of nvcc --use_fast_math arithmetic; mode 2: its texture hardware; mode 3: both).
    Asserted: HIP vs literal flips <= 1.5 x the rate of the strictest control (fast-math arithmetic alone); cost disagreement (> 1e-2) <= 1e-3 of the pixels, mean cost
    within 0.1 %; InitializeScore leaves identical planes.
T3  the whole Run() schedule: individual decisions differ (ties flip, then the random walks diverge), the statistics must
    not: pixels within 1 % of the analytic ground-truth depth +-0.5 pp, mean matching cost +-2 %.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, V = 400, 300, 8

# The bars of T1 and T2, by name: tests/test_reference_gpu.py applies the same ones against the reference's own compiled code.
T1_BAR = 1e-3                  # north_star's tolerance on a cost in [0, 2]
T1_SHARE_ABOVE_BAR = 1e-5      # share of the evaluations that may exceed it against the IEEE formulas ...
T1_MAX = 2e-3                  # ... none beyond this
T1_MEDIAN = 5e-5
T1_Q8_SHARE_ABOVE_BAR = 1e-3   # against the 8-bit texture fractions (a property of the sampler hardware, not of the formulas)
T1_Q8_MAX = 3e-3
T1_BOTH_VALID = 0.5            # share of the evaluations that must be real costs on both sides
T1_SENTINEL_DISAGREEMENT = 1e-3
T2_INIT_FLIPS = 1e-4           # InitializeScore, geometric / prior modes: depths re-derived through one division (photometric: no flip at all)
T2_COST_FAR = 1e-2             # one step from an identical state: costs further apart than this ...
T2_COST_FAR_SHARE = 1e-3       # ... on at most this share of the pixels
T2_MEAN_COST_REL = 1e-3        # and the mean cost within 0.1 %


@pytest.fixture(scope="module")
def scene(pm, oracle, engine):
    sc = pm.synth.make_problem_scene(W, H, n_src=V, quantize=True)
    cams, imgs = sc.problem(0, list(range(1, V + 1)))
    dmin, dmax = pm.synth.kernel_depth_range(cams[0])
    gpu = engine.create(0)
    gpu.set_views(cams, imgs)
    cpu = oracle.create()
    cpu.set_views(cams, imgs)
    return sc, cams, imgs, gpu, cpu, float(dmin), float(dmax)


def test_T1_ncc_costs_vs_literal_formulas(pm, oracle, scene):
    sc, cams, imgs, gpu, cpu, dmin, dmax = scene
    prm = pm.PatchMatchParams(num_images=V + 1, depth_min=dmin, depth_max=dmax, max_scale=0)
    cam = sc.views[0].cam
    rng = np.random.default_rng(11)
    gt = sc.views[0].gt_depth.astype(np.float64)
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    worst = {1: 0.0, 2: 0.0, 3: 0.0}
    for depth, tilt in [(gt, 0.0), (gt * rng.uniform(0.9, 1.1, gt.shape), 0.3), (rng.uniform(dmin, dmax, gt.shape), 1.0)]:
        n = np.zeros((H, W, 3))
        n[..., 2] = -1.0
        n[..., :2] = tilt * rng.normal(size=(H, W, 2))
        n /= np.linalg.norm(n, axis=-1, keepdims=True)
        X = np.stack([depth * (u - cam.K[2]) / cam.K[0], depth * (v - cam.K[5]) / cam.K[4], depth], -1)
        planes = np.concatenate([n, -(n * X).sum(-1)[..., None]], -1).astype(np.float32)
        for scale in (0, 1, 2):
            hip = gpu.eval_ncc(prm, planes, scale)
            for mode in (1, 2, 3):
                lit = oracle.eval_ncc_literal(cpu, prm, planes, scale, mode=mode)
                both = (hip < 2.0) & (lit < 2.0)
                assert both.mean() > T1_BOTH_VALID
                assert ((hip == 2.0) != (lit == 2.0)).mean() < T1_SENTINEL_DISAGREEMENT     # window centre on the image border / variance threshold
                d = np.abs(hip - lit)[both]
                worst[mode] = max(worst[mode], float(d.max()))
                if mode == 1:
                    assert (d > T1_BAR).mean() <= T1_SHARE_ABOVE_BAR, (scale, tilt, float(d.max()))
                    assert d.max() < T1_MAX
                    assert np.median(d) < T1_MEDIAN
                else:
                    assert (d > T1_BAR).mean() <= T1_Q8_SHARE_ABOVE_BAR, (scale, tilt, float(d.max()))
                    assert d.max() < T1_Q8_MAX
    print(f"max |HIP - literal| = {worst[1]:.2e}, max |HIP - literal with 8-bit fractions| = {worst[2]:.2e}, max |HIP - fast-math model| = {worst[3]:.2e}")


def _planes_for(cam, depth, tilt, rng):
    """per-pixel planes through the points at `depth` with normals tilted away from the optical axis by ~`tilt`"""
    h, w = depth.shape
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    n = np.zeros((h, w, 3))
    n[..., 2] = -1.0
    n[..., :2] = tilt * rng.normal(size=(h, w, 2))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    X = np.stack([depth * (u - cam.K[2]) / cam.K[0], depth * (v - cam.K[5]) / cam.K[4], depth], -1)
    return np.concatenate([n, -(n * X).sum(-1)[..., None]], -1).astype(np.float32)


def _window_stats(cams, imgs, view, plane, x, y, scale):
    """float64 restatement of the window of ComputeBilateralNCC (ref .cu:325-414) for ONE evaluation -- reference pixel (x, y), camera-frame
    plane (n, d), source `view` (0-based) -- returning (weighted source variance, weighted reference variance, taps clamped to the
    source border): what makes an evaluation ill-conditioned.  Diagnostic only; no assertion depends on it."""
    def cam(c):
        return (np.array(c.K, np.float64).reshape(3, 3), np.array(c.R, np.float64).reshape(3, 3), np.array(c.C, np.float64))
    Kr, Rr, Cr = cam(cams[0])
    Ks, Rs, Cs = cam(cams[view + 1])
    n, d = np.asarray(plane[:3], np.float64), float(plane[3])
    Rrel, trel = Rs @ Rr.T, Rs @ (Cr - Cs)
    Hm = Ks @ (Rrel - np.outer(trel, n) / d) @ np.linalg.inv(Kr)
    ref, src = np.asarray(imgs[0], np.float64), np.asarray(imgs[view + 1], np.float64)
    hh, ww = src.shape
    step = 2 << scale
    radius = 5 * step // 2
    rc = ref[y, x]
    sw = swr = swrr = sws = swss = 0.0
    clamped = 0
    for i in range(-radius, radius + 1, step):
        for j in range(-radius, radius + 1, step):
            px, py = min(max(x + i, 0), ref.shape[1] - 1), min(max(y + j, 0), ref.shape[0] - 1)
            r = ref[py, px]
            q = Hm @ np.array([x + i, y + j, 1.0])
            sx, sy = q[0] / q[2], q[1] / q[2]
            if not (0.0 <= sx <= ww - 1 and 0.0 <= sy <= hh - 1):
                clamped += 1
            cx, cy = min(max(sx, 0.0), ww - 1.0), min(max(sy, 0.0), hh - 1.0)
            x0, y0 = int(np.floor(cx)), int(np.floor(cy))
            x1, y1 = min(x0 + 1, ww - 1), min(y0 + 1, hh - 1)
            ax, ay = cx - x0, cy - y0
            sv = (src[y0, x0] * (1 - ax) + src[y0, x1] * ax) * (1 - ay) + (src[y1, x0] * (1 - ax) + src[y1, x1] * ax) * ay
            wgt = np.exp(-np.sqrt(float(i * i + j * j)) / 50.0 - abs(r - rc) / 18.0)
            sw += wgt
            swr += wgt * r
            swrr += wgt * r * r
            sws += wgt * sv
            swss += wgt * sv * sv
    var_s, var_r = swss / sw - (sws / sw) ** 2, swrr / sw - (swr / sw) ** 2
    return var_s, var_r, clamped, (swss / sw) / max(var_s, 1e-30)   # E[s^2] / var_s: how much the fp32 subtraction E[s^2] - E[s]^2 amplifies rounding


def _ring_centres(n_src, spacing):
    """n_src distinct camera centres around the reference, nearest first (a 7 x 7 grid holds 48)"""
    cand = sorted((dx * dx + dy * dy, dx, dy) for dx in range(-3, 4) for dy in range(-3, 4) if (dx, dy) != (0, 0))
    return [(0.0, 0.0, 0.0)] + [(spacing * dx, spacing * dy, 0.0) for _, dx, dy in cand[:n_src]]


# Round 5: the bridge above stands on ONE near-frontal 400x300 scene and meets north_star's 1e-3 with 0.5 % of
# margin.  The same comparison -- HIP path against the oracle's literal transcription of the reference's formulas (mode 1) -- on the
# geometries the fuzz test uses but the bridge never saw: strongly rotated cameras with per-view intrinsics, 16 and 32 source views,
# non-integer fp32 images (the fp32 texture format), and the BASELINE size.  The bar stays where T1 has it (at most 1e-5 of the
# evaluations above 1e-3, none above 2e-3); the distribution of every case is printed and, with MPMVS_REPORT_DIR set, written to
# literal_modes_widened.txt (profiles/r05_literal_modes.txt is a copy).
WIDENED = [
    # name, width, height, views, spacing, rot_deg, focal_jitter, quantize, scales
    ("frontal_8_views_400x300 (the scene of T1)", 400, 300, 8, 0.15, 2.0, 0.0, True, (0, 1, 2)),
    ("harsh_cameras_12deg_focal25pct", 400, 300, 8, 0.4, 12.0, 0.25, True, (0, 1, 2)),
    ("harsh_cameras_15deg_focal25pct_fp32_images", 400, 300, 8, 0.5, 15.0, 0.25, False, (0, 1, 2)),
    ("16_views", 400, 300, 16, 0.12, 3.0, 0.0, True, (0, 1, 2)),
    ("32_views_5deg", 320, 240, 32, 0.1, 5.0, 0.1, True, (0, 2)),
    ("fp32_images_frontal", 400, 300, 8, 0.15, 2.0, 0.0, False, (0, 1, 2)),
    ("baseline_size_1600x1200", 1600, 1200, 8, 0.15, 2.0, 0.0, True, (0,)),
]


def test_T1_widened_geometries_vs_literal_formulas(pm, oracle, engine):
    import os
    rows, outliers, above_1e3 = [], [], []
    for name, w, h, nv, spacing, rot, fj, quant, scales in WIDENED:
        sc = pm.synth.make_scene(w, h, _ring_centres(nv, spacing), rot_deg=rot, focal_jitter=fj, quantize=quant, seed=pm.synth.SCENE_SEED + nv + int(rot))
        cams, imgs = sc.problem(0, list(range(1, nv + 1)))
        dmin, dmax = (float(v) for v in pm.synth.kernel_depth_range(cams[0]))
        gpu, cpu = engine.create(0), oracle.create()
        for hd in (gpu, cpu):
            hd.set_views(cams, imgs)
        prm = pm.PatchMatchParams(num_images=nv + 1, depth_min=dmin, depth_max=dmax, max_scale=0)
        rng = np.random.default_rng(17)
        gt = sc.views[0].gt_depth.astype(np.float64)
        plane_sets = [("true surface", gt, 0.0), ("10 % depth noise, tilted", gt * rng.uniform(0.9, 1.1, gt.shape), 0.3)]
        if w * h <= 400 * 300:
            plane_sets.append(("random", rng.uniform(dmin, dmax, gt.shape), 1.0))
        diffs, sentinel = [], 0.0
        for pname, depth, tilt in plane_sets:
            planes = _planes_for(sc.views[0].cam, depth, tilt, rng)
            for scale in scales:
                hip = gpu.eval_ncc(prm, planes, scale)
                lit = oracle.eval_ncc_literal(cpu, prm, planes, scale, mode=1)
                both = (hip < 2.0) & (lit < 2.0)
                sentinel = max(sentinel, float(((hip == 2.0) != (lit == 2.0)).mean()))
                dd = np.where(both, np.abs(hip - lit), 0.0)
                diffs.append(dd[both])
                if dd.max() > 2e-3:
                    # the evaluations beyond 2e-3, one by one, next to what the reference's OWN arithmetic variants make of them: the
                    # model of its binary (mode 3: fast-math + 8-bit texture fractions) against its formulas (mode 1) at the same spot
                    lit3 = oracle.eval_ncc_literal(cpu, prm, planes, scale, mode=3)
                    for v_, y_, x_ in zip(*np.nonzero(dd > 2e-3)):
                        outliers.append(f"    {name}: planes '{pname}', scale {scale}, view {v_}, pixel ({x_}, {y_}): HIP {hip[v_, y_, x_]:.6f}, literal {lit[v_, y_, x_]:.6f} "
                                        f"(|d| {dd[v_, y_, x_]:.2e}); the reference against itself there: model of its binary {lit3[v_, y_, x_]:.6f} "
                                        f"(|d| {abs(float(lit3[v_, y_, x_]) - float(lit[v_, y_, x_])):.2e})")
                if name.startswith("baseline") and (dd > 1e-3).any():
                    # every BASELINE-size evaluation above north_star's 1e-3, with what makes it ill-conditioned: the weighted source
                    # variance of its window (the NCC denominator; the cost is declared invalid below 1e-5, ref .cu:406-408) and the
                    # share of its 36 taps that were clamped to the border of the source image
                    for v_, y_, x_ in zip(*np.nonzero(dd > 1e-3)):
                        var_s, var_r, clamped, amp = _window_stats(cams, imgs, int(v_), planes[y_, x_], int(x_), int(y_), scale)
                        above_1e3.append(f"    {name}: planes '{pname}', view {v_}, pixel ({x_}, {y_}), plane n = ({planes[y_, x_, 0]:+.3f}, {planes[y_, x_, 1]:+.3f}, {planes[y_, x_, 2]:+.3f}) d = {planes[y_, x_, 3]:.3f}: "
                                         f"HIP {hip[v_, y_, x_]:.6f}, literal {lit[v_, y_, x_]:.6f} (|d| {dd[v_, y_, x_]:.2e}); var_s {var_s:.3e}, var_r {var_r:.3e} (grey levels^2), E[s^2] / var_s = {amp:.0f}, taps clamped {clamped}/36")
        d = np.concatenate(diffs)
        rows.append((name, gpu.texture_format(), d.size, float(d.max()), float(np.percentile(d, 99.99)), float(np.percentile(d, 99.9)), float(np.median(d)),
                     float((d > 1e-3).mean()), int((d > 1e-3).sum()), sentinel))
        del gpu, cpu
    lines = ["T1 widened: |HIP cost - literal formulas (mode 1)| over all valid evaluations of a case (costs in [0, 2]; north_star: 1e-3)",
             f"{'case':48s} {'texels':6s} {'evaluations':>11s} {'max':>9s} {'99.99 %':>9s} {'99.9 %':>9s} {'median':>9s} {'> 1e-3':>9s} {'count':>6s} {'sentinel disagreement':>22s}"]
    for r in rows:
        lines.append(f"{r[0]:48s} {r[1]:6s} {r[2]:11d} {r[3]:9.2e} {r[4]:9.2e} {r[5]:9.2e} {r[6]:9.2e} {r[7]:9.2e} {r[8]:6d} {r[9]:22.2e}")
    lines.append(f"evaluations beyond 2e-3 ({len(outliers)}):")
    lines += outliers
    lines.append(f"BASELINE-size evaluations above 1e-3, one by one ({len(above_1e3)}): a cost is 1 - cov / sqrt(var_r var_s) with var = E[x^2] - E[x]^2 formed in fp32 (ref .cu:398-404); "
                 "on a low-contrast window (standard deviation ~3 grey levels around a mean of ~130) that subtraction cancels 3 of fp32's 7 digits -- E[s^2] / var_s below -- "
                 "and ANY reordering of the sums moves the cost at the 1e-3 level, the reference's own fast-math build included")
    lines += above_1e3
    text = "\n".join(lines)
    print(text)
    rep = os.environ.get("MPMVS_REPORT_DIR")
    if rep:
        os.makedirs(rep, exist_ok=True)
        with open(os.path.join(rep, "literal_modes_widened.txt"), "w") as f:
            f.write(text + "\n")
    for r in rows:
        assert r[9] < 1e-3, r                       # window centre on the image border / variance threshold
        assert r[7] <= 1e-5, r                      # the bar of T1 on every geometry: at most 1e-5 of the evaluations above north_star's 1e-3
        assert r[4] < 1e-3 and r[6] < 5e-5, r       # 99.99 % of the evaluations inside 1e-3 (measured: <= 4.5e-4), median < 5e-5
    # Maxima: none beyond 2e-3 on the near-frontal geometries (the bar of T1).  The harsh geometries (>= 12 degrees of rotation, 25 %
    # focal jitter: windows warped half out of the source image, where clamped taps repeat and the source variance in the NCC
    # denominator collapses) keep the distribution but not the maximum: a handful of ill-conditioned evaluations in millions reach
    # 1e-2 -- listed above with what the model of the reference's own binary makes of the same evaluation.  Reported, not absorbed
    # into a wider bar: they must stay a handful.
    for r in rows:
        if r[0].startswith("harsh"):
            assert r[8] <= 10, r
        elif r[0].startswith("16_views") or r[0].startswith("baseline"):
            assert r[3] < 4e-3, r
        else:
            assert r[3] < 2e-3, r


# SURVEY 8(c) budgeted <= 0.5 % of the pixels for this tier.  That budget cannot hold against ANY second implementation of these
# formulas: a cost difference of 1e-4 flips a threshold count, a sampled view, an arg-min or an acceptance test, and the pixel
# then carries a different, equally good plane.  Since round 4 that statement is MEASURED instead of asserted: the oracle's
# measurement modes cover the whole path (libm expf / sinf / cosf / acosf, rsqrt, the double `0.8 *` of ref .cu:832, every
# division, the literal geometric chain), and mode 3 models the reference BINARY (nvcc --use_fast_math, ref CMakeLists.txt:18:
# approximate exp / sin / cos / reciprocal, contracted multiply-adds, 8-bit texture fractions).  The control is the reference
# against itself -- its formulas in IEEE arithmetic (mode 1) against the same formulas as its own build computes them (mode 3)
# (mode 3), against its texture hardware alone (mode 2) and against its build's arithmetic alone (mode 4 = mode 3 without the 8-bit
# fractions).  The HIP path may flip at most 1.5 x as many pixels against mode 1 as the reference's formulas flip against
# themselves under fast-math ARITHMETIC alone -- the strictest of the three controls.  Measured (400x300, MI355X, with literal_tex pinned to the
# reference's code; profiles/r06_literal_modes.txt): HIP vs literal 1.29 % / 4.71 % / 1.49 % (photometric / geometric / prior); literal vs
# fast-math arithmetic 1.20 % / 4.51 % / 1.39 %; literal vs 8-bit fractions 3.16 % / 9.30 % / 2.93 %.
SURVEY_T2_BUDGET = 0.005
CONTROL_FACTOR = 1.5
# ... and absolute caps beside the relative bound: a defect in code that the canonical mode and the control share would
# inflate both flip rates together; the caps are round 3's fixed limits, about twice what is measured
ABSOLUTE_CAP = {"photometric": 0.03, "geometric": 0.08, "prior": 0.03}


def test_T2_single_steps_vs_literal_formulas(pm, oracle, scene):
    sc, cams, imgs, gpu, cpu, dmin, dmax = scene
    rng = np.random.default_rng(5)
    ids = list(range(1, V + 1))
    depths = [sc.views[i].gt_depth * (1.0 + 0.005 * rng.standard_normal((H, W))).astype(np.float32) for i in ids]
    prior = np.zeros((H, W, 4), np.float32)
    prior[..., 2] = -1.0
    prior[..., 3] = sc.views[0].gt_depth
    mask = (rng.uniform(size=(H, W)) < 0.6).astype(np.uint32)
    for h in (gpu, cpu):
        h.set_src_depths(depths)
        h.set_prior(prior, mask)

    def flips(a, b):
        rel = np.abs(a[0][..., 3] - b[0][..., 3]) / np.maximum(np.abs(b[0][..., 3]), 1e-6)
        return float((rel > 1e-3).mean())

    rows = []
    for mode_name, geom, planar in (("photometric", False, False), ("geometric", True, False), ("prior", False, True)):
        prm = pm.PatchMatchParams(num_images=V + 1, depth_min=dmin, depth_max=dmax, max_scale=0, geom_consistency=geom, planar_prior=planar)
        # identical start state on every side: a converged photometric result (canonical arithmetic: bit-identical on both)
        p0 = pm.PatchMatchParams(num_images=V + 1, depth_min=dmin, depth_max=dmax, max_scale=0)
        for h in (gpu, cpu):
            h.run(p0, 7)
        s_planes, s_costs = cpu.get()
        assert np.array_equal(s_planes, gpu.get()[0])

        def two_steps(h, literal_mode):
            """InitializeScore, then one BlackPixelUpdate, from the saved state: (planes, costs) after each"""
            if literal_mode:
                oracle.set_literal_mode(h, literal_mode)
            try:
                h.set_state(s_planes, s_costs)
                h.step(prm, 11, pm.KIND_INIT, 0, 0, 0)
                after_init = h.get()
                h.step(prm, 11, pm.KIND_BLACK, 0, 0, 1)
                return after_init, h.get()
            finally:
                if literal_mode:
                    oracle.set_literal_mode(h, 0)

        hip_i, hip_u = two_steps(gpu, 0)
        lit = {m: two_steps(cpu, m) for m in (1, 2, 3, 4)}
        # InitializeScore: the planes are drawn / re-encoded, not selected: no flips at all against the IEEE formulas
        f_init = flips(hip_i, lit[1][0])
        f_hip = flips(hip_u, lit[1][1])
        control = {"fast-math arithmetic": flips(lit[4][1], lit[1][1]), "8-bit fractions": flips(lit[2][1], lit[1][1]),
                   "fast-math build (both)": flips(lit[3][1], lit[1][1])}
        dc = np.abs(hip_u[1] - lit[1][1][1])
        rows.append((mode_name, f_init, f_hip, control, float((dc > T2_COST_FAR).mean()), float(hip_u[1].mean()), float(lit[1][1][1].mean()), flips(hip_u, lit[3][1])))
    print("T2, pixels whose depth differs by more than 1e-3 after one BlackPixelUpdate (SURVEY budget %.1e):" % SURVEY_T2_BUDGET)
    for name, f_init, f_hip, control, far, mh, ml, f_hip3 in rows:
        print(f"  {name}: HIP vs literal {f_hip:.2e}; the reference against itself: literal vs " +
              ", vs ".join(f"{k} {v:.2e}" for k, v in control.items()) + f"; HIP vs fast-math model {f_hip3:.2e}; after InitializeScore {f_init:.1e}; "
              f"costs: |d| > 1e-2 at {far:.1e} of the pixels, mean {mh:.5f} / {ml:.5f}")
    for name, f_init, f_hip, control, far, mh, ml, f_hip3 in rows:
        assert f_init <= (0.0 if name == "photometric" else T2_INIT_FLIPS), (name, f_init)   # geometric / prior: depths re-derived through one division
        floor = control["fast-math arithmetic"]   # the strictest control: arithmetic alone, the texture hardware flips 2-3 x more
        assert floor > 0.0
        assert f_hip <= CONTROL_FACTOR * floor, f"{name}: HIP flips {f_hip:.3e} of the pixels against the literal formulas, the reference's own variants {floor:.3e}"
        assert f_hip <= ABSOLUTE_CAP[name] and floor <= ABSOLUTE_CAP[name], (name, f_hip, floor)
        assert far <= T2_COST_FAR_SHARE and abs(mh / ml - 1.0) <= T2_MEAN_COST_REL, (name, far, mh, ml)


def test_T3_schedule_statistics_vs_literal_formulas(pm, oracle, scene):
    sc, cams, imgs, gpu, cpu, dmin, dmax = scene
    gt = sc.views[0].gt_depth
    prm = pm.PatchMatchParams(num_images=V + 1, depth_min=dmin, depth_max=dmax, max_scale=2)
    stats = {}
    for mode in (0, 1, 2, 3):
        acc, cost = [], []
        for seed in (1, 2):
            if mode == 0:
                gpu.run(prm, seed)
                planes, costs = gpu.get()
            else:
                oracle.set_literal_mode(cpu, mode)
                cpu.run(prm, seed)
                planes, costs = cpu.get()
                oracle.set_literal_mode(cpu, 0)
            rel = np.abs(planes[..., 3] - gt) / gt
            acc.append(float((rel < 0.01).mean()))
            cost.append(float(costs.mean()))
        stats[mode] = (np.mean(acc), np.mean(cost))
    print("within 1 %% of GT / mean cost: HIP %.4f %.5f, literal %.4f %.5f, literal + 8-bit %.4f %.5f, fast-math model %.4f %.5f" % (stats[0] + stats[1] + stats[2] + stats[3]))
    assert stats[0][0] > 0.9                                              # the schedule converges on this scene
    for mode in (1, 2, 3):
        assert abs(stats[mode][0] - stats[0][0]) < 0.005, stats
        assert abs(stats[mode][1] / stats[0][1] - 1.0) < 0.02, stats


# ---------------------------------------------------------------------------------------------------------------------------------
# Round 6: T2 and T3 widened the way round 5 widened T1.  T2 above stands on one near-frontal scene, one
# BlackPixelUpdate, iteration 0.  Here the same comparison -- one kernel step from an identical state, HIP path against the oracle
# computing the WHOLE step with the reference's literal formulas (mode 1), flip rate against the CONTROL (the reference's formulas
# against their own fast-math arithmetic, mode 4; the model of its binary, mode 3, printed beside it) -- on the harsh-camera scene, 16
# views, fp32 images; for the black AND the red pass; at iteration 0 (photometric: straight from random planes) and at the last
# iteration (from the state the passes before it left); at window scale 2 for the photometric mode.  Identical states mid-schedule are
# made by driving the passes before the one under test on the HIP path (bit-identical to the canonical oracle: tests/test_parity_gpu.py)
# and handing its raw state (camera-frame planes, costs, selected views) to every variant.  Flips are counted over the pixels of the
# pass's colour (the other colour is not touched by the pass): a pixel flips when the depth of its plane differs by more than 1e-3
# relative.  The table goes to stdout and, with MPMVS_REPORT_DIR set, to literal_modes_t2_widened.txt (profiles/r06_literal_modes.txt).
# ---------------------------------------------------------------------------------------------------------------------------------
T2_SCENES = [
    # name, width, height, views, spacing, rot_deg, focal_jitter, quantize, step sets
    ("frontal_8_views", 400, 300, 8, 0.15, 2.0, 0.0, True, ("photo0", "photo2", "geom", "prior")),
    ("harsh_cameras_12deg_focal25pct", 400, 300, 8, 0.4, 12.0, 0.25, True, ("photo0", "photo2", "geom", "prior")),
    ("16_views", 400, 300, 16, 0.12, 3.0, 0.0, True, ("photo0", "geom")),
    ("fp32_images_frontal", 400, 300, 8, 0.15, 2.0, 0.0, False, ("photo0", "geom", "prior")),
]
# (pass, iteration, launch id) of the steps under test per set; the passes between them run canonically.  Launch ids as Run() numbers them.
T2_STEPS = {
    "photo0": [("black", 0, 1), ("red", 0, 2), ("black", 2, 5), ("red", 2, 6)],     # window scale 0: from random planes, then the last iteration
    "photo2": [("black", 0, 1), ("red", 0, 2)],                                      # window scale 2 (radius 20)
    "geom": [("black", 0, 1), ("red", 0, 2), ("black", 1, 3), ("red", 1, 4)],        # 2 iterations, from a converged photometric state
    "prior": [("black", 0, 1), ("red", 0, 2), ("black", 2, 5), ("red", 2, 6)],
}
T2_WIDENED_CAP = {"photo0": 0.12, "photo2": 0.12, "geom": 0.16, "prior": 0.06}   # absolute caps on flips among the pass's pixels (the caps of T2 above, per colour; random-plane passes: measured x 2)


def _depth_of_planes(cam, planes_cam):
    """ComputeDepthfromPlaneHypothesis (ref .cu:84-87) of camera-frame planes (n, d) at their own pixels, in float64"""
    h, w = planes_cam.shape[:2]
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    p = planes_cam.astype(np.float64)
    fx, fy, cx, cy = float(cam.K[0]), float(cam.K[4]), float(cam.K[2]), float(cam.K[5])
    den = (u - cx) * p[..., 0] + (fx / fy) * (v - cy) * p[..., 1] + fx * p[..., 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        return -p[..., 3] * fx / den


def test_T2_widened_scenes_passes_iterations_vs_literal_formulas(pm, oracle, engine):
    import os
    rows = []
    for name, w, h, nv, spacing, rot, fj, quant, sets in T2_SCENES:
        sc = pm.synth.make_scene(w, h, _ring_centres(nv, spacing), rot_deg=rot, focal_jitter=fj, quantize=quant, seed=pm.synth.SCENE_SEED + nv + int(rot))
        ids = list(range(1, nv + 1))
        cams, imgs = sc.problem(0, ids)
        dmin, dmax = (float(v) for v in pm.synth.kernel_depth_range(cams[0]))
        gpu, cpu = engine.create(0), oracle.create()
        rng = np.random.default_rng(5)
        depths = [sc.views[i].gt_depth * (1.0 + 0.005 * rng.standard_normal((h, w))).astype(np.float32) for i in ids]
        prior = np.zeros((h, w, 4), np.float32)
        prior[..., 2] = -1.0
        prior[..., 3] = sc.views[0].gt_depth
        mask = (rng.uniform(size=(h, w)) < 0.6).astype(np.uint32)
        for hd in (gpu, cpu):
            hd.set_views(cams, imgs)
            hd.set_src_depths(depths)
            hd.set_prior(prior, mask)
        yy, xx = np.mgrid[0:h, 0:w]
        colour = {"black": (xx + yy) % 2 == 0, "red": (xx + yy) % 2 == 1}
        kind_of = {"black": pm.KIND_BLACK, "red": pm.KIND_RED}
        # the converged photometric state the geometric and prior passes start from (world normals + depth, as Run() leaves it)
        p0 = pm.PatchMatchParams(num_images=nv + 1, depth_min=dmin, depth_max=dmax, max_scale=0)
        gpu.run(p0, 7)
        conv_planes, conv_costs = gpu.get()
        for st in sets:
            scale = 2 if st == "photo2" else 0
            prm = pm.PatchMatchParams(num_images=nv + 1, depth_min=dmin, depth_max=dmax, max_scale=scale,
                                      geom_consistency=(st == "geom"), planar_prior=(st == "prior"), max_iterations=2 if st == "geom" else 3)
            # canonical chain on the HIP path: InitializeScore (launch 0), then black / red in Run()'s order up to each step under test
            gpu.set_state(conv_planes, conv_costs)
            gpu.step(prm, 11, pm.KIND_INIT, 0, scale, 0)
            launch, it, todo = 1, 0, list(T2_STEPS[st])
            while todo:
                for pas in ("black", "red"):
                    pre = gpu.get() + (gpu.get_selected_views(),)
                    if todo and todo[0] == (pas, it, launch):
                        todo.pop(0)
                        res = {}
                        for variant in (0, 1, 4, 3):   # 0 = the HIP path; oracle modes: 1 literal IEEE formulas, 4 fast-math arithmetic, 3 model of the binary
                            hd = gpu if variant == 0 else cpu
                            if variant:
                                oracle.set_literal_mode(cpu, variant)
                            try:
                                hd.set_state(pre[0], pre[1])
                                hd.set_selected_views(pre[2])
                                hd.step(prm, 11, kind_of[pas], it, scale, launch)
                                res[variant] = hd.get()
                            finally:
                                if variant:
                                    oracle.set_literal_mode(cpu, 0)
                        m = colour[pas]
                        ref_depth = _depth_of_planes(cams[0], res[1][0])

                        def flips(planes):
                            d = _depth_of_planes(cams[0], planes)
                            rel = np.abs(d - ref_depth) / np.maximum(np.abs(ref_depth), 1e-6)
                            return float(((rel > 1e-3) | ~np.isfinite(rel))[m].mean())
                        dc = np.abs(res[0][1] - res[1][1])[m]
                        rows.append((name, st, pas, it, flips(res[0][0]), flips(res[4][0]), flips(res[3][0]), float((dc > 1e-2).mean()),
                                     float(res[0][1][m].mean()), float(res[1][1][m].mean())))
                        # the HIP path has just recomputed the canonical step: the chain goes on from its result
                    else:
                        gpu.step(prm, 11, kind_of[pas], it, scale, launch)
                    launch += 1
                it += 1
        del gpu, cpu
    lines = ["T2 widened: pixels of the pass's colour whose depth differs by more than 1e-3 (relative) from the literal IEEE formulas (oracle mode 1) after ONE pass from an identical state",
             f"{'scene':34s} {'mode':7s} {'pass':6s} {'iter':>4s} {'HIP':>9s} {'control: fast-math arithmetic':>30s} {'model of the binary':>20s} {'ratio':>6s} {'cost |d| > 1e-2':>16s} {'mean cost HIP / literal':>24s}"]
    over = []
    for (name, st, pas, it, f_hip, f_ctl, f_bin, far, mh, ml) in rows:
        ratio = f_hip / f_ctl if f_ctl > 0 else float("inf")
        lines.append(f"{name:34s} {st:7s} {pas:6s} {it:4d} {f_hip:9.2e} {f_ctl:30.2e} {f_bin:20.2e} {ratio:6.2f} {far:16.1e} {mh:12.5f} /{ml:10.5f}")
        if not (f_hip <= CONTROL_FACTOR * f_ctl) or f_hip > T2_WIDENED_CAP[st]:
            over.append(f"    {name} {st} {pas} iteration {it}: HIP {f_hip:.3e} vs {CONTROL_FACTOR} x control {f_ctl:.3e} = {CONTROL_FACTOR * f_ctl:.3e} (cap {T2_WIDENED_CAP[st]})")
    lines.append(f"cases beyond {CONTROL_FACTOR} x the control or beyond the absolute cap ({len(over)}):")
    lines += over
    lines.append("pooled over all cases: HIP flips / control flips = %.3f" % (sum(r[4] * (w_ * h_ // 2) for r in rows for (nm, w_, h_, *_) in T2_SCENES if nm == r[0]) /
                                                                         sum(r[5] * (w_ * h_ // 2) for r in rows for (nm, w_, h_, *_) in T2_SCENES if nm == r[0])))
    text = "\n".join(lines)
    print(text)
    rep = os.environ.get("MPMVS_REPORT_DIR")
    if rep:
        os.makedirs(rep, exist_ok=True)
        with open(os.path.join(rep, "literal_modes_t2_widened.txt"), "w") as f:
            f.write(text + "\n")
    # The bound of T2 (1.5 x the control) on every case -- except that a case whose control counts fewer than 100 pixels (of the 60 000
    # of a colour) is a ratio of two small Poisson counts: those may reach 2 x, are listed above as exceeding, and must stay a handful.
    # Pooled over all cases the ratio has no such noise and must stay well inside the bound.
    n_colour = {name: w * h // 2 for name, w, h, *_ in T2_SCENES}
    noisy = 0
    for (name, st, pas, it, f_hip, f_ctl, f_bin, far, mh, ml) in rows:
        assert f_ctl > 0.0, (name, st, pas, it)
        if f_hip > CONTROL_FACTOR * f_ctl:
            assert f_ctl * n_colour[name] < 100 and f_hip <= 2.0 * f_ctl, (f"{name} {st} {pas} iteration {it}: HIP flips {f_hip:.3e} of the pass's pixels against the literal "
                                                                            f"formulas, the reference's own fast-math arithmetic {f_ctl:.3e}")
            noisy += 1
        assert f_hip <= T2_WIDENED_CAP[st] and f_ctl <= T2_WIDENED_CAP[st], (name, st, pas, it, f_hip, f_ctl)
        assert far <= 2e-3 and abs(mh / ml - 1.0) <= 2e-3, (name, st, pas, it, far, mh, ml)
    assert noisy <= 3, over
    pooled = sum(r[4] * n_colour[r[0]] for r in rows) / sum(r[5] * n_colour[r[0]] for r in rows)
    print(f"pooled over the {len(rows)} cases: HIP flips / control flips = {pooled:.3f}")
    assert pooled <= 1.25, pooled


def test_T3_shipped_schedule_statistics_vs_literal_formulas(pm, oracle, engine):
    """T3 on the cfg-3 schedule (reference config/config.yaml: photometric 3 scales -> geometric Run + planar prior + prior Run ->
    geometric Run) at 400x300: the HIP path through the C++ ProcessProblem mirror against the same schedule on the oracle with the
    reference's literal formulas (mode 1) and with the model of its binary (mode 3).  Individual pixels diverge (ties flip, random
    walks separate); the statistics must not: pixels within 1 % of the analytic ground truth +-0.5 pp, mean cost +-2 %."""
    import importlib
    import os
    from test_pipeline_gpu import PRIOR_SEED_OFFSET
    hostlib = importlib.import_module("mp-mvs_amd.hostlib")
    sc = pm.synth.make_problem_scene(W, H, n_src=V, quantize=True)
    cams, imgs = sc.problem(0, list(range(1, V + 1)))
    dmin, dmax = (float(v) for v in pm.synth.kernel_depth_range(cams[0]))
    gt = sc.views[0].gt_depth
    rng = np.random.default_rng(3)
    src_depths = [sc.views[i].gt_depth * (1.0 + 0.005 * rng.standard_normal((H, W))).astype(np.float32) for i in range(1, V + 1)]

    def literal_schedule(mode, seed):
        hd = oracle.create()
        hd.set_views(cams, imgs)
        oracle.set_literal_mode(hd, mode)
        state = {}

        def process(geom, planar, sd):
            p = pm.PatchMatchParams(num_images=V + 1, depth_min=dmin, depth_max=dmax, max_scale=2)
            p.geom_consistency, p.max_iterations, p.geomPlanarPrior = geom, (2 if geom else 3), bool(geom and planar)
            if geom:
                hd.set_src_depths(src_depths)
                hd.set_state(state["planes"], state["costs"])
            hd.run(p, sd)
            if planar:
                planes, costs, g = hd.get(geom=True)
                prior, mask, ntri = hostlib.build_prior(cams[0], planes, costs, g, True, p.depth_min, p.depth_max)
                assert ntri > 0
                hd.set_prior(prior, mask)
                p.planar_prior, p.geom_consistency, p.max_iterations = True, False, 3
                hd.run(p, (sd + PRIOR_SEED_OFFSET) & 0xFFFFFFFFFFFFFFFF)
            state["planes"], state["costs"] = hd.get()

        process(False, False, seed)
        process(True, True, seed + 1)
        process(True, False, seed + 2)
        return state["planes"][..., 3], state["costs"]

    stats = {}
    for which in ("HIP", 1, 3):
        acc, cost = [], []
        for seed in (4242,):
            if which == "HIP":
                depth, _, costs = hostlib.run_pipeline(0, cams, imgs, 2, 2, True, True, seed, src_depths)
            else:
                depth, costs = literal_schedule(which, seed)
            acc.append(float((np.abs(depth - gt) / gt < 0.01).mean()))
            cost.append(float(costs.mean()))
        stats[which] = (float(np.mean(acc)), float(np.mean(cost)))
    text = ("T3 on the shipped schedule (cfg 3, 400x300, 8 views): pixels within 1 %% of the ground truth / mean cost: HIP %.4f %.5f, literal formulas %.4f %.5f, "
            "model of the reference's binary %.4f %.5f" % (stats["HIP"] + stats[1] + stats[3]))
    print(text)
    rep = os.environ.get("MPMVS_REPORT_DIR")
    if rep:
        os.makedirs(rep, exist_ok=True)
        with open(os.path.join(rep, "literal_modes_t3_cfg3.txt"), "w") as f:
            f.write(text + "\n")
    assert stats["HIP"][0] > 0.95
    for mode in (1, 3):
        assert abs(stats[mode][0] - stats["HIP"][0]) < 0.005, stats
        assert abs(stats[mode][1] / stats["HIP"][1] - 1.0) < 0.02, stats
