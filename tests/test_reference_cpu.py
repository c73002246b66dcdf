"""The oracle's LITERAL modes (1: the reference's formulas with IEEE operations and libm; 2: the same with CUDA's 8-bit texture
fractions) against the reference's OWN device code compiled for the host (oracle/ref_driver.cpp over oracle/ref_shim/, see
tests/ref_common.py): bit for bit, per function and per launch of Run() in its three modes.

This pins the hand transcription in oracle/pm_oracle.cpp (literal_ncc, literal_tex, geom_cost_literal and the literal paths
of init_pixel / update_pixel) to the text it transcribes; tests/test_literal_gpu.py then measures the canonical arithmetic
-- what the HIP kernels compute, bit for bit -- against those modes.

Both sides consume the same uniforms: the reference's curand_uniform reads a table filled from the project's stream
(seed, pixel, launch).  Each side continues from its OWN state and is compared after every launch, so a divergence is
reported at the launch where it starts.  Shapes are small because the reference side runs one thread at a time: 70x50 and
64x48, and 40x33, whose odd height with H / 2 a multiple of 16 makes the checkerboard grid miss the last row."""
import numpy as np
import pytest

import ref_common as rc

# name, width, height, source views, quantised images
SCENES = [("70x50_3src_u8", 70, 50, 3, True), ("64x48_9src_fp32", 64, 48, 9, False), ("40x33_3src_u8", 40, 33, 3, True)]


class Case:
    def __init__(self, pm, oracle, name, w, h, nv, quant):
        self.name, self.W, self.H, self.V = name, w, h, nv
        self.sc = pm.synth.make_scene(w, h, rc.ring_centres(nv, 0.15), rot_deg=3.0, focal_jitter=0.05, quantize=quant, seed=pm.synth.SCENE_SEED + nv + h)
        self.ids = list(range(1, nv + 1))
        self.cams, self.imgs = self.sc.problem(0, self.ids)
        self.dmin, self.dmax = (float(v) for v in pm.synth.kernel_depth_range(self.cams[0]))
        self._oracle = oracle
        rng = np.random.default_rng(5)
        # source depth maps with noise and holes (a hole is depth 0: the geometric cost's sentinel)
        self.src_depths = []
        for i in self.ids:
            d = self.sc.views[i].gt_depth * (1.0 + 0.01 * rng.standard_normal((h, w))).astype(np.float32)
            d[rng.uniform(size=(h, w)) < 0.1] = 0.0
            self.src_depths.append(d.astype(np.float32))
        self.cpu, self.ref = self.fresh()
        self.planes = rc.plane_sets(self.sc, self.dmin, self.dmax, np.random.default_rng(11))

    def fresh(self):
        """a new oracle context and a new pair of reference contexts (without / with 8-bit fractions): zeroed state on both sides"""
        cpu = self._oracle.create()
        cpu.set_views(self.cams, self.imgs)
        cpu.set_src_depths(self.src_depths)
        ref = {q8: rc.Reference(self.cams, self.imgs, q8=q8) for q8 in (False, True)}
        for r in ref.values():
            r.set_src_depths(self.src_depths)
        return cpu, ref

    def params(self, pm, **kw):
        return pm.PatchMatchParams(num_images=self.V + 1, depth_min=self.dmin, depth_max=self.dmax, **kw)


@pytest.fixture(scope="module", params=SCENES, ids=[s[0] for s in SCENES])
def case(request, pm, oracle):
    return Case(pm, oracle, *request.param)


@pytest.fixture(autouse=True)
def _canonical_afterwards(request, oracle):
    if "case" not in request.fixturenames:
        yield
        return
    case = request.getfixturevalue("case")
    yield
    oracle.set_literal_mode(case.cpu, 0)


# ---- per function ---------------------------------------------------------------------------------------------------------------
def test_homography(case, oracle):
    rng = np.random.default_rng(3)
    n = 0
    for _, planes in case.planes:
        for y, x in zip(rng.integers(0, case.H, 40), rng.integers(0, case.W, 40)):
            for v in range(case.V):
                a, b = oracle.homography_literal(case.cpu, planes[y, x], v), case.ref[False].homography(planes[y, x], v)
                assert rc.same_bits(a, b), (case.name, v, planes[y, x], a, b)
                n += 1
    assert n == 3 * 40 * case.V


@pytest.mark.parametrize("mode", [1, 2])
def test_ncc(case, oracle, pm, mode):
    """scales 0-2 (windows of radius 5, 10, 20: far over the border of these images), planes from the true surface to random (random
    planes project outside the source: the out-of-view sentinel)"""
    prm = case.params(pm, max_scale=0)
    sentinel, total = 0, 0
    for pname, planes in case.planes:
        for scale in (0, 1, 2):
            lit = oracle.eval_ncc_literal(case.cpu, prm, planes, scale, mode=mode)
            ref = case.ref[mode == 2].eval_ncc(prm, planes, scale)
            assert rc.same_bits(lit, ref), f"{case.name} planes '{pname}' scale {scale} mode {mode}: {rc.n_diff(lit, ref)} of {lit.size} evaluations differ, max |d| {np.nanmax(np.abs(lit - ref)):.2e}"
            sentinel += int((ref == 2.0).sum())
            total += ref.size
            if pname == "true surface":
                assert (ref < 2.0).mean() > 0.7 and np.median(ref[ref < 2.0]) < 0.2     # a real matching cost, not noise
    assert sentinel / total < 0.5 and sentinel > 0                                       # both the sentinel and real costs are compared


def test_geometric_cost(case, oracle, pm):
    prm = case.params(pm, max_scale=0, geom_consistency=True)
    capped = {}
    for pname, planes in case.planes:
        lit = oracle.eval_geom_literal(case.cpu, prm, planes)
        ref = case.ref[False].eval_geom(prm, planes)
        assert rc.same_bits(lit, ref), f"{case.name} planes '{pname}': {rc.n_diff(lit, ref)} of {lit.size} checks differ"
        capped[pname] = float((ref == 3.0).mean())
        if pname == "true surface":
            assert 0.02 < capped[pname] < 0.5 and np.median(ref) < 1.0                  # holes give the sentinel, the rest is consistent
    # random planes: points that leave the source image (clamped fetch) or miss its surface: more checks end at the cap, not all
    assert capped["true surface"] < capped["random"] < 1.0, capped


@pytest.mark.parametrize("mode", [1, 2])
def test_initial_cost_and_selected_views(case, oracle, pm, mode):
    """top_k = 4 of 3 views (every valid view is selected) and of 9 (the threshold acts); `cost_vector[32] = {2.0f}` leaves zeros behind
    the first element, which the sort never reaches"""
    prm = case.params(pm, max_scale=0)
    oracle.set_literal_mode(case.cpu, mode)
    for pname, planes in case.planes:
        for scale in (0, 2):
            lc, ls = oracle.eval_initial(case.cpu, prm, planes, scale)
            rcost, rsel = case.ref[mode == 2].eval_initial(prm, planes, scale)
            assert rc.same_bits(lc, rcost) and rc.same_bits(ls, rsel), f"{case.name} planes '{pname}' scale {scale} mode {mode}: {rc.n_diff(lc, rcost)} costs, {rc.n_diff(ls, rsel)} view sets differ"
            if pname == "true surface":
                nsel = np.array([bin(int(s)).count("1") for s in rsel.reshape(-1)])
                assert nsel.max() == min(4, case.V) and (rcost < 2.0).mean() > 0.7
                if case.V > 4:
                    assert (nsel == 4).mean() > 0.5                                     # the top_k threshold drops views


# ---- per launch -----------------------------------------------------------------------------------------------------------------
def _schedule(prm):
    """(kind, iteration, window scale) of Run()'s launches, in order (reference Run(); kinds as in include/mpmvs.h)"""
    out = [(0, 0, prm.max_scale)]
    scales = [0] if (prm.geom_consistency or prm.planar_prior) else list(range(prm.max_scale, -1, -1))
    for s in scales:
        for i in range(prm.max_iterations):
            out += [(1, i, s), (2, i, s)]
    return out + [(3, 0, 0), (4, 0, 0), (5, 0, 0)]


KIND_NAME = ["InitializeScore", "BlackPixelUpdate", "RedPixelUpdate", "GetDepthandNormal", "BlackPixelFilter", "RedPixelFilter"]


def _run_and_compare(case, oracle, prm, mode, seed, state=None, prior=None):
    """every launch of Run() on both sides, each from its own state; returns per update launch the share of its colour's pixels whose
    plane changed, and the largest number of draws one pixel consumed"""
    cpu, refs = case.fresh()
    ref = refs[mode == 2]
    H, W = case.H, case.W
    if prior is not None:
        cpu.set_prior(*prior)
        ref.set_prior(*prior)
    zeros = (np.zeros((H, W, 4), np.float32), np.zeros((H, W), np.float32))
    planes0, costs0 = state if state is not None else zeros
    cpu.set_state(planes0, costs0)
    cpu.set_selected_views(np.zeros((H, W), np.uint32))
    ref.set_state(planes0, costs0, np.zeros((H, W), np.uint32))
    oracle.set_literal_mode(cpu, mode)
    yy, xx = np.mgrid[0:H, 0:W]
    changed, most, rows_updated = [], 0, np.zeros(H, bool)
    for launch, (kind, it, scale) in enumerate(_schedule(prm)):
        before = ref.get()[0]
        cpu.step(prm, seed, kind, it, scale, launch)
        most = max(most, ref.launch(prm, kind, it, scale, rc.draw_table(oracle, seed, launch, H * W) if kind <= 2 else None))
        lp, lc, lg = cpu.get(geom=True)
        ls = cpu.get_selected_views()
        rp, rcost, rs, rg = ref.get()
        where = f"{case.name} mode {mode} launch {launch} ({KIND_NAME[kind]}, iteration {it}, scale {scale})"
        assert rc.same_bits(lp, rp), f"{where}: planes differ at {rc.n_diff(lp, rp)} components"
        assert rc.same_bits(lc, rcost), f"{where}: costs differ at {rc.n_diff(lc, rcost)} pixels"
        assert rc.same_bits(ls, rs), f"{where}: selected views differ at {rc.n_diff(ls, rs)} pixels"
        assert rc.same_bits(lg, rg), f"{where}: geometric costs differ at {rc.n_diff(lg, rg)} pixels"
        if kind in (1, 2):
            colour = (xx + yy) % 2 == (0 if kind == 1 else 1)
            changed.append(float((rp != before).any(-1)[colour].mean()))
            assert not (rp != before).any(-1)[~colour].any(), where              # a pass leaves the other colour alone
            assert (rcost == 2.0).mean() < 0.5, where
            rows_updated |= (rp != before).any((1, 2))
    return changed, most, rows_updated, ref.get()


def _guard(changed, most, floor):
    """equality must never be the equality of untouched arrays: a healthy share of every update launch's pixels took a new plane"""
    assert min(changed) > floor, changed
    assert 3 < most <= rc.DRAW_CAP


@pytest.mark.parametrize("mode,max_scale", [(1, 0), (1, 2), (2, 0)])
def test_run_photometric(case, oracle, pm, mode, max_scale):
    prm = case.params(pm, max_scale=max_scale, max_iterations=2)
    changed, most, rows_updated, _ = _run_and_compare(case, oracle, prm, mode, seed=12345)
    print(f"{case.name} photometric max_scale {max_scale} mode {mode}: changed per update launch {['%.2f' % c for c in changed]}, most draws {most}")
    _guard(changed, most, 0.5)
    if case.H % 2 == 1 and (case.H // 2) % 16 == 0:
        # the checkerboard grid stops one row short where H is odd and H / 2 a multiple of 16: no update launch touches the last row
        assert rows_updated[-5:-1].all() and not rows_updated[-1]


@pytest.fixture(scope="module")
def converged(case, oracle, pm):
    """a photometric result in the canonical arithmetic (world normals + depth, as Run() leaves it): the start of the geometric and prior runs"""
    oracle.set_literal_mode(case.cpu, 0)
    case.cpu.run(case.params(pm, max_scale=1), 7)
    planes, costs = case.cpu.get()
    return planes.copy(), costs.copy()


@pytest.mark.parametrize("mode", [1, 2])
def test_run_geometric(case, oracle, pm, converged, mode):
    prm = case.params(pm, max_scale=0, max_iterations=2, geom_consistency=True)
    changed, most, _, final = _run_and_compare(case, oracle, prm, mode, seed=4242, state=converged)
    print(f"{case.name} geometric mode {mode}: changed per update launch {['%.2f' % c for c in changed]}, most draws {most}")
    _guard(changed, most, 0.5)
    assert (final[3] > 0).mean() > 0.2                                         # geometric costs were written


@pytest.mark.parametrize("mode", [1, 2])
def test_run_planar_prior(case, oracle, pm, converged, mode):
    """masks that cover part of the image; priors on the surface, tilted priors, and priors whose depth leaves [depth_min, depth_max];
    stored costs on both sides of InitializeScore's 0.1 (which decides between the perturbed prior and the stored plane)"""
    H, W = case.H, case.W
    rng = np.random.default_rng(9)
    gt = case.sc.views[0].gt_depth
    prior = rc.planes_for(case.sc.views[0].cam, gt.astype(np.float64), 0.0, rng)
    tilted = rc.planes_for(case.sc.views[0].cam, gt.astype(np.float64) * 1.03, 0.2, rng)
    prior[:, W // 2:] = tilted[:, W // 2:]
    far = rc.planes_for(case.sc.views[0].cam, np.full((H, W), case.dmax * 1.3), 0.0, rng)
    near = rc.planes_for(case.sc.views[0].cam, np.full((H, W), case.dmin * 0.5), 0.0, rng)
    prior[: H // 5] = far[: H // 5]
    prior[-(H // 6):] = near[-(H // 6):]
    mask = (rng.uniform(size=(H, W)) < 0.6).astype(np.uint32)
    mask[:, : W // 6] = 0
    planes, costs = converged
    costs = np.where(rng.uniform(size=(H, W)) < 0.5, costs, np.float32(0.5)).astype(np.float32)
    assert 0.2 < ((costs >= 0.1) & (mask > 0)).mean() < 0.8
    prm = case.params(pm, max_scale=0, max_iterations=2, planar_prior=True)
    changed, most, _, _ = _run_and_compare(case, oracle, prm, mode, seed=777, state=(planes, costs), prior=(prior, mask))
    print(f"{case.name} planar prior mode {mode}: changed per update launch {['%.2f' % c for c in changed]}, most draws {most}")
    _guard(changed, most, 0.5)


# ---- sky filter -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(96, 72), (33, 17), (5, 3), (130, 49)])
def test_sky_filter(oracle, size):
    """both oracle modes against both builds, on the sizes of tests/test_sky_gpu.py"""
    from test_sky_cpu import sky_scene
    img, coarse, _ = sky_scene(*size, seed=size[0])
    rng = np.random.default_rng(0)
    for bgr, mask in ((img, coarse), (rng.integers(0, 256, img.shape, dtype=np.uint8), rng.random(coarse.shape).astype(np.float32))):
        outs = {(literal, fma): (oracle.sky_bilateral(bgr, mask, literal=literal), rc.sky_bilateral(bgr, mask, fma=fma)) for literal in (False, True) for fma in (False, True)}
        for (literal, fma), (a, b) in outs.items():
            assert np.array_equal(a, b), (size, literal, fma, int((a != b).sum()))
        if size[0] > 5:
            assert set(np.unique(outs[(True, False)][1])) == {0.0, 255.0}               # both outcomes are compared


# ---- the prediction of tests/test_reference_gpu.py ------------------------------------------------------------------------------
# The oracle's canonical mode is what the HIP kernels compute, bit for bit (tests/test_parity_gpu.py), so the checks of
# test_reference_gpu.py run here first, on the same scene with the same seeds and the same bars.
@pytest.fixture(scope="module")
def direct(pm):
    return rc.Direct(pm)


@pytest.fixture(scope="module")
def canonical(direct, oracle):
    return direct.attach(oracle.create())


def test_canonical_ncc_vs_compiled_reference(pm, direct, canonical):
    import test_literal_gpu as bars
    rc.check_ncc_direct(pm, direct, canonical, bars)


def test_canonical_geom_and_homography_vs_compiled_reference(pm, direct, canonical):
    rc.check_geom_direct(pm, direct, canonical)
    rc.check_homography_direct(pm, direct, canonical)


def test_canonical_init_and_one_black_update_vs_compiled_reference(pm, oracle, direct, canonical):
    import test_literal_gpu as bars
    rc.check_steps_direct(pm, oracle, direct, canonical, bars)
