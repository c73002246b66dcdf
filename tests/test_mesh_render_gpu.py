"""mpmvs_surface_render_depth on the GPU against the plain statement (tests/mesh_render_common.py): array_equal on the depth bits, on
the triangle maps and on counts[0:2], no tolerance anywhere; the hand scenes of test_mesh_render_cpu.py on the device, both paths
forced through MPMVS_RASTER_LARGE, and the render end to end on the synthetic scene."""
import copy
import ctypes as C
import importlib

import numpy as np
import pytest

import mesh_render_common as mr
import render_common as rc

pytestmark = pytest.mark.gpu
F = np.float32
D = np.float64
ALL, NONE_ = "0", "1073741824"   # MPMVS_RASTER_LARGE: every pair down the large path, none


@pytest.fixture(scope="module")
def mesh(engine):
    return importlib.import_module("mp-mvs_amd.mesh")


def same(got_d, got_t, want_d, want_t):
    assert len(got_d) == len(want_d)
    for v, (g, w) in enumerate(zip(got_d, want_d)):
        assert mr.same_bits(g, w), f"view {v}: {(g.view(np.uint32) != w.view(np.uint32)).sum()} depths differ"
    if got_t is not None:
        for v, (g, w) in enumerate(zip(got_t, want_t)):
            assert g.dtype == np.int32 and np.array_equal(g, w), f"view {v}: {(g != w).sum()} triangle ids differ"


def check(mesh, m, cams, want=None, h=None):
    """render on the device and compare with the statement; -> (depths, tris, counts of the device)"""
    want = want if want is not None else mr.statement(m["xyz"], m["tri"], cams)
    own = h is None
    h = h if h is not None else mesh.Mesh(m["xyz"], m["tri"])
    try:
        depths, tris = h.render_depth(cams, want_tri=True)
        counts = h.last_render_counts
        work = h.render_work()
    finally:
        if own:
            h.close()
    same(depths, tris, want[0], want[1])
    assert [counts["pairs"], counts["covered"]] == want[2].tolist()
    # every covered pixel lies in a box and took at least one atomic minimum; no pixel of a box takes more than one per pair
    assert counts["covered"] <= work["atomics"] <= work["box_pixels"]
    for d, t in zip(depths, tris):
        assert np.array_equal(t == -1, d == 0)
    return depths, tris, counts


def both_paths(mesh, m, cams, monkeypatch, default, want=None):
    """at the default threshold, with every pair listed and with none: the same bits; default: which of the taking-part pairs the
    default threshold lists: "all", "some" or "none" of them"""
    want = want if want is not None else mr.statement(m["xyz"], m["tri"], cams)
    out = {}
    for large in (None, ALL, NONE_):
        if large is None:
            monkeypatch.delenv("MPMVS_RASTER_LARGE", raising=False)
        else:
            monkeypatch.setenv("MPMVS_RASTER_LARGE", large)
        out[large] = check(mesh, m, cams, want)[2]
        listed, pairs = out[large]["large_pairs"], out[large]["pairs"]
        if large is None:
            assert {"all": listed == pairs > 0, "some": 0 < listed < pairs, "none": listed == 0 < pairs}[default], (listed, pairs)
        else:
            assert listed == (pairs if large == ALL else 0)
    monkeypatch.delenv("MPMVS_RASTER_LARGE", raising=False)
    return out


# ---- the hand scenes of the CPU tests -------------------------------------------------------------------------------------------------------
def test_fronto_parallel_triangle(mesh, monkeypatch):
    px = [(2, 1), (12, 1), (2, 9)]
    m = mr.mesh(mr.at_pixels(px, 2.0), [[0, 1, 2]])
    for large in (None, ALL, NONE_):
        if large is not None:
            monkeypatch.setenv("MPMVS_RASTER_LARGE", large)
        d, t, counts = check(mesh, m, [mr.hand_camera()])
        assert counts["covered"] == 51 and counts["pairs"] == 1 and mr.same_bits(d[0][d[0] != 0], np.full(51, 2.0, F))
        assert np.array_equal(d[0] != 0, mr.closed_triangle_pixels(*px, mr.HAND_W, mr.HAND_H))
        assert d[0][5, 7] == 2 and d[0][1, 12] == 2 and d[0][9, 2] == 2 and d[0][5, 8] == 0


@pytest.mark.parametrize("second", ([1, 3, 2], [1, 2, 3], [3, 2, 1], [2, 1, 3]))
def test_shared_diagonal(mesh, monkeypatch, second):
    m = mr.mesh(mr.at_pixels([(2, 1), (12, 1), (2, 9), (12, 9)], 2.0), [[0, 1, 2], second])
    for large in (None, ALL):
        if large is not None:
            monkeypatch.setenv("MPMVS_RASTER_LARGE", large)
        d, t, counts = check(mesh, m, [mr.hand_camera()])
        assert counts["covered"] == 99 and (d[0][1:10, 2:13] == 2).all() and [t[0][y, x] for x, y in ((12, 1), (7, 5), (2, 9))] == [0, 0, 0]


def test_ties_and_depth_order(mesh, monkeypatch):
    px = [(2, 1), (12, 1), (2, 9)]
    near, far = mr.at_pixels(px, 2.0), mr.at_pixels(px, 3.0)
    cam = [mr.hand_camera()]
    for large in (None, ALL):
        if large is not None:
            monkeypatch.setenv("MPMVS_RASTER_LARGE", large)
        d, t, _ = check(mesh, mr.mesh(near, [[0, 1, 2], [0, 1, 2], [2, 0, 1]]), cam)
        assert (t[0][d[0] != 0] == 0).all()
        for tri, winner in (([[0, 1, 2], [3, 4, 5]], 0), ([[3, 4, 5], [0, 1, 2]], 1)):
            d, t, counts = check(mesh, mr.mesh(np.concatenate([near, far]), tri), cam)
            assert counts["covered"] == 51 and (t[0][d[0] != 0] == winner).all() and (d[0][d[0] != 0] == 2).all()


def test_degenerate_and_non_finite_triangles(mesh):
    cam = [mr.hand_camera()]
    xyz = np.concatenate([mr.at_pixels([(2, 1), (7, 5), (12, 9), (12, 1)], 2.0), [[np.nan, 0, 2], [0, np.inf, 2], [0, 0, -np.inf]]]).astype(F)
    for tri, pairs in (([[0, 0, 0]], 1), ([[0, 0, 3]], 1), ([[3, 0, 0]], 1), ([[0, 1, 2]], 1), ([[0, 3, 4], [5, 0, 3], [0, 3, 6], [0, 0, 0]], 1)):
        d, t, counts = check(mesh, mr.mesh(xyz, tri), cam)
        assert counts["pairs"] == pairs and counts["covered"] == 0 and (d[0] == 0).all()
    d, t, counts = check(mesh, mr.mesh(xyz, [[0, 0, 0], [4, 0, 3], [0, 3, 2], [0, 0, 3]]), cam)
    assert counts["pairs"] == 3 and counts["covered"] > 0 and (t[0][d[0] != 0] == 2).all()


def test_the_camera_plane(mesh, monkeypatch):
    cam = [mr.pinhole(80.0, 47.5, 31.5, 96, 64)]
    for xyz in ([[-1, -1, -2], [1, -1, -3], [0, 1, -4]], [[-1, 0, 0], [1, 0, 0], [0, 1, 0]]):
        d, t, counts = check(mesh, mr.mesh(xyz, [[0, 1, 2]]), cam)
        assert counts["pairs"] == 0 and counts["covered"] == 0
    out = both_paths(mesh, mr.mesh([[-1, -1, 5], [1, -1, 5], [0, 2, -5]], [[0, 1, 2]]), cam, monkeypatch, "all")
    assert out[None]["covered"] == 3616 and out[None]["large_pairs"] == 1   # a crossing triangle's box is the whole image
    d = check(mesh, mr.mesh([[-1, -1, 5], [1, -1, 5], [0, 2, -5]], [[0, 1, 2]]), cam)[0][0]
    assert (d[d != 0] > 0).all() and d.max() <= 5.0 and abs(float(d[d != 0].min()) - 0.720721) <= 1e-6


# ---- the watertight height field and the cube, both paths ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("rev", (0, 3))
def test_watertight_height_field_on_both_paths(mesh, monkeypatch, rev):
    hf = mr.height_field(24, rev)
    near = mr.height_field_cameras()
    cams = near + [mr.look_at((0.1, 0.0, 8.0), (0, 0, 0), 80.0, 96, 64, up=(0, 1, 0)),     # from afar the triangles are small,
                   mr.look_at((0.0, 0.0, 0.22), (0.02, 0.01, 0.0), 80.0, 96, 64, up=(0, 1, 0))]   # from very near above the default threshold
    want = mr.cached(("height field far", rev), lambda: mr.statement(hf["xyz"], hf["tri"], cams))
    assert all(mr.fills_image(c) for c in near) and all((d != 0).all() for d in want[0][:4]) and (want[0][4] == 0).any()
    out = both_paths(mesh, hf, cams, monkeypatch, "some", want)
    assert 0 < out[None]["large_pairs"] < out[None]["pairs"] == 6 * len(hf["tri"])


def test_cube_on_both_paths(mesh, monkeypatch):
    cb = mr.cube()
    cams = mr.cube_cameras() + [mr.look_at((40.0, 3.0, 5.0), (0, 0, 0), 55.0, 64, 48)]
    want = mr.cached("cube far", lambda: mr.statement(cb["xyz"], cb["tri"], cams))
    out = both_paths(mesh, cb, cams, monkeypatch, "some", want)
    assert 0 < out[None]["large_pairs"] < out[None]["pairs"] == 13 * 12
    worst = 0.0
    for c, d in zip(cams[:12], want[0]):
        hit, miss, z = mr.ray_box(c, mr.CUBE_HALF)
        assert not (hit & (d == 0)).any() and not (miss & (d != 0)).any()
        worst = max(worst, float((np.abs(d[hit].astype(D) - z[hit]) / z[hit]).max()))
    assert worst <= 4 * 5.85e-8   # as test_mesh_render_cpu.py


def test_image_filling_triangles_and_a_mesh_outside_the_frustum(mesh, monkeypatch):
    cam = [mr.pinhole(120.0, 79.5, 59.5, 160, 120)]
    full = mr.mesh([[-100, -100, 4], [100, -100, 4], [0, 200, 4]], [[0, 1, 2]])
    crossing = mr.mesh([[-50, -60, 2], [50, -60, 2], [0, 90, -1]], [[0, 1, 2]])
    for m in (full, crossing):
        out = both_paths(mesh, m, cam, monkeypatch, "all")
        assert out[None]["covered"] == 160 * 120 and out[None]["large_pairs"] == 1   # served by the large path at the default threshold
    away = mr.height_field(8)
    away["xyz"] = (away["xyz"] + np.array([500.0, -300.0, 5.0], F)).astype(F)   # in front of the camera and far to the side
    out = both_paths(mesh, away, cam, monkeypatch, "none")
    assert out[None]["covered"] == 0 and out[None]["pairs"] == len(away["tri"])


# ---- seeded soups ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(mr.SOUP_CASES))
def test_soup(mesh, monkeypatch, seed):
    m, cams = mr.soup(seed)
    if seed % 3 == 1:
        monkeypatch.setenv("MPMVS_RASTER_LARGE", ALL)
    elif seed % 3 == 2:
        monkeypatch.setenv("MPMVS_RASTER_LARGE", NONE_)
    d, t, counts = check(mesh, m, cams)
    assert counts["pairs"] > 0 and (d[2] == 0).all()   # the camera that looks away sees nothing
    assert all(np.isfinite(x).all() and (x >= 0).all() for x in d)


# ---- views: a chunk plus one, optional triangle maps, nothing to do ------------------------------------------------------------------------------------
def raw_render(engine, handle, cams, depths, tris, counts=None, n_views=None, null_cams=False, null_depths=False):
    _abi = mr.abi()
    f = engine.load()[1]
    n = len(cams) if n_views is None else n_views
    arr = (_abi.Camera * max(len(cams), 1))(*cams)
    dp = (C.c_void_p * max(len(depths), 1))(*[None if d is None else d.ctypes.data for d in depths])
    tp = None if tris is None else (C.c_void_p * max(len(tris), 1))(*[None if t is None else t.ctypes.data for t in tris])
    rc_ = f["surface_render_depth"](handle, n, None if null_cams else arr, None if null_depths else dp, tp, counts)
    return rc_, (f["last_error"](None) or b"").decode()


def test_nine_views_of_nine_sizes_and_optional_triangle_maps(engine, mesh):
    hf = mr.height_field(12)
    cams = [mr.look_at((0.2 * k - 0.8, 0.1 * k - 0.3, 1.2 + 0.2 * k), (0.0, 0.05 * k, 0.0), 30.0 + 3 * k, 40 + 7 * k, 50 - 3 * k, up=(0, 1, 0)) for k in range(9)]
    want = mr.statement(hf["xyz"], hf["tri"], cams)
    with mesh.Mesh(hf["xyz"], hf["tri"]) as h:
        check(mesh, hf, cams, want, h)
        total, passes = h.render_ms()
        assert total > 0 and all(passes[k] > 0 for k in ("init", "small", "large", "resolve"))
        assert same(h.render_depth(cams), None, want[0], None) is None   # out_tri NULL
        shapes = [(int(c.height), int(c.width)) for c in cams]
        d = [np.full(s, 7.0, F) for s in shapes]
        t = [np.full(s, 7, np.int32) if k % 2 else None for k, s in enumerate(shapes)]   # NULL entries
        counts = (C.c_longlong * 3)()
        assert raw_render(engine, h._h, cams, d, t, counts)[0] == 0
        same(d, None, want[0], None)
        assert all(np.array_equal(t[k], want[1][k]) for k in range(1, 9, 2)) and list(counts)[:2] == want[2].tolist()
        assert raw_render(engine, h._h, cams, d, [None] * 9, None)[0] == 0
        # no view: outputs untouched
        d0, t0 = [np.full(shapes[0], 7.0, F)], [np.full(shapes[0], 7, np.int32)]
        assert raw_render(engine, h._h, cams[:1], d0, t0, n_views=0)[0] == 0 and (d0[0] == 7).all() and (t0[0] == 7).all()
        assert h.render_depth([]) == [] and h.render_depth([], want_tri=True) == ([], [])
    for m in (mr.mesh(np.zeros((0, 3), F), np.zeros((0, 3), np.int32)), mr.mesh(np.array([[np.nan, 0, 2], [0, np.inf, 2], [1, 2, -np.inf]], F), [[0, 1, 2]])):
        d, t, counts = check(mesh, m, cams[:2])
        assert counts == {"pairs": 0, "covered": 0, "large_pairs": 0}


def test_order_independence(mesh):
    m, cams = mr.soup(2)
    base_d, base_t, _ = check(mesh, m, cams)
    perm = np.random.default_rng(4).permutation(len(m["tri"]))
    mp = mr.mesh(m["xyz"], m["tri"][perm])
    d, t, _ = check(mesh, mp, cams)   # a fresh handle; the triangle maps equal the statement of the permuted mesh
    for a, b in zip(d, base_d):
        assert mr.same_bits(a, b)


def test_seventy_thousand_copies_of_one_triangle(mesh, monkeypatch):
    xyz = mr.at_pixels([(2, 1), (12, 1), (2, 9)], 2.0)
    m = mr.mesh(xyz, np.tile(np.array([[0, 1, 2]], np.int32), (70001, 1)))
    one = mr.statement(xyz, [[0, 1, 2]], [mr.hand_camera()])
    want = (one[0], one[1], np.array([70001, 51]))   # every copy takes part; the statement's minimum is index 0 wherever it covers
    for large in (None, ALL):
        if large is not None:
            monkeypatch.setenv("MPMVS_RASTER_LARGE", large)
        d, t, counts = check(mesh, m, [mr.hand_camera()], want)
        assert (t[0][d[0] != 0] == 0).all() and counts["covered"] == 51


def test_every_error_code_on_a_live_handle(engine, mesh):
    hf = mr.height_field(6)
    cams = mr.height_field_cameras(24, 16)[:2]
    with mesh.Mesh(hf["xyz"], hf["tri"]) as h:
        want = mr.statement(hf["xyz"], hf["tri"], cams)
        check(mesh, hf, cams, want, h)   # the handle is live: its mesh is on the device
        d = [np.full((16, 24), 7.0, F), np.full((16, 24), 7.0, F)]

        def sized(w, hh):
            c = copy.copy(cams[0])
            c.width, c.height = w, hh
            return c
        cases = [(-2, dict(handle=None)), (-2, dict(null_cams=True)), (-2, dict(null_depths=True)), (-2, dict(depths=[d[0], None])), (-2, dict(n_views=-1)),
                 (-2, dict(cams=[cams[0], sized(0, 16)])), (-2, dict(cams=[cams[0], sized(24, -1)])),
                 (-3, dict(cams=[cams[0], sized((1 << 24) + 1, 1)])), (-3, dict(cams=[cams[0], sized(1, (1 << 24) + 1)])),
                 (-3, dict(cams=[cams[0], sized(1 << 16, 1 << 15)])), (-3, dict(cams=[cams[0], sized(1 << 16, 1 << 16)]))]
        for code, kw in cases:
            args = dict(handle=h._h, cams=cams, depths=d, tris=None)
            args.update(kw)
            got, text = raw_render(engine, args.pop("handle"), args.pop("cams"), args.pop("depths"), args.pop("tris"), **args)
            assert got == code and text.startswith("surface render:"), (kw, got, text)
            assert (d[0] == 7).all() and (d[1] == 7).all()   # found before anything is written
        # (-100, a HIP failure, is not provoked)
        with pytest.raises(ValueError, match="surface_render_depth"):
            h.render_depth([sized(0, 16)])
        check(mesh, hf, cams, want, h)   # the handle still works


def test_other_calls_on_the_handle_are_unchanged_by_a_render(engine, mesh):
    cloud = importlib.import_module("mp-mvs_amd.cloud")
    m, cams = mr.soup(5)
    pts = (m["xyz"][np.isfinite(m["xyz"]).all(1)][::3] + F(0.01)).astype(F)
    with mesh.Mesh(m["xyz"], m["tri"]) as h, cloud.Cloud(pts) as c:
        comp0 = h.components()
        dist0 = h.distance(c, 0.2)
        want = mr.statement(m["xyz"], m["tri"], cams)
        check(mesh, m, cams, want, h)
        comp1 = h.components()
        dist1 = h.distance(c, 0.2)
        check(mesh, m, cams, want, h)
    assert all(np.array_equal(a, b) for a, b in zip(comp0[:3], comp1[:3])) and comp0[3] == comp1[3]
    assert mr.same_bits(dist0[0], dist1[0]) and np.array_equal(dist0[1], dist1[1])


# ---- end to end on the synthetic scene -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(pm):
    """smoke()'s scene at 96 x 64 and the mesh of view 1's analytic depth grid: its pixels back-projected, two triangles per pixel quad"""
    sc = pm.synth.make_problem_scene(96, 64, n_src=3, spacing=0.5)
    H, W = 64, 96
    xyz = rc.backproject(sc.views[1])
    idx = np.arange(H * W).reshape(H, W)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    tri = np.concatenate([np.stack([a, b, d], 1), np.stack([a, d, c], 1)]).astype(np.int32)
    assert len(tri) == 2 * 95 * 63
    return sc, mr.mesh(xyz, tri)


COVERED_SHARE = 0.859375          # measured with the statement: see test_synthetic_scene_end_to_end (views 0 and 1 overlap in part)
LARGEST_DEVIATION = 7.182719e-05


def test_synthetic_scene_end_to_end(mesh, scene):
    """the mesh of view 1's depth grid rendered into view 0 against view 0's analytic depth.  Measured with the statement: the share
    of view 0 that the mesh covers and the largest relative deviation over the covered pixels; asserted at the
    measured share less 0.005 and at twice the measured deviation.  The margin is for the piecewise-linear surface between the
    samples; it is not tuned."""
    sc, m = scene
    cam = [sc.views[0].cam]
    want = mr.cached("synthetic", lambda: mr.statement(m["xyz"], m["tri"], cam))
    d, t, counts = check(mesh, m, cam, want)
    gt = sc.views[0].gt_depth
    covered = d[0] != 0
    rel = np.abs(d[0].astype(D) - gt)[covered] / gt[covered]
    print(f"view 0: covered share {covered.mean():.6f}, largest relative deviation {rel.max():.6e}, large pairs {counts['large_pairs']} of {counts['pairs']}")
    assert covered.mean() >= COVERED_SHARE - 0.005
    assert rel.max() <= 2 * LARGEST_DEVIATION


def test_patchmatch_scored_against_the_rendered_mesh(pm, engine, mesh, scene):
    """smoke()'s Problem through PatchMatch, scored against the rendered mesh and against the analytic map over the covered pixels.
    |est - rendered| differs from |est - analytic| by at most delta = max |rendered - analytic|, so the count within t of the rendered
    map lies between the analytic counts at t - delta and t + delta (as test_render_gpu.py brackets the point render)."""
    depthmap = importlib.import_module("mp-mvs_amd.depthmap")
    sc, m = scene
    pcams, imgs = sc.problem(0, [1, 2, 3])
    dmin, dmax = pm.synth.kernel_depth_range(pcams[0])
    prm = pm.PatchMatchParams(num_images=4, depth_min=float(dmin), depth_max=float(dmax), max_scale=1)
    gpu = engine.create(0)
    gpu.set_views(pcams, imgs)
    gpu.run(prm, 12345)
    est = np.ascontiguousarray(gpu.get()[0][..., 3])
    cam = [sc.views[0].cam]
    want = mr.cached("synthetic", lambda: mr.statement(m["xyz"], m["tri"], cam))
    rendered = check(mesh, m, cam, want)[0][0]
    covered = rendered != 0
    analytic = np.where(covered, sc.views[0].gt_depth, F(0)).astype(F)
    delta = float(np.abs(rendered.astype(D) - analytic)[covered].max())
    tol = [0.05, 0.2]
    s_r = depthmap.score(est, rendered, tol)
    lo = depthmap.score(est, analytic, [t - delta for t in tol])
    hi = depthmap.score(est, analytic, [t + delta for t in tol])
    print(f"delta {delta:.3e}; within rendered {[r['within'] for r in s_r['tolerances']]}, analytic at t - delta {[r['within'] for r in lo['tolerances']]}, "
          f"at t + delta {[r['within'] for r in hi['tolerances']]}; n_gt {s_r['n_gt']}")
    assert 0 < delta < 0.05 and s_r["n_gt"] == lo["n_gt"] == int(covered.sum()) and s_r["n_est"] == lo["n_est"]
    for k in range(2):
        assert lo["tolerances"][k]["within"] <= s_r["tolerances"][k]["within"] <= hi["tolerances"][k]["within"]
    assert s_r["tolerances"][1]["within"] > 0.5 * s_r["n_gt"]
