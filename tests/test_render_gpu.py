"""mpmvs_cloud_render_depth on the GPU against the plain statement (tests/render_common.py): array_equal on the depth bits and
on idx, no tolerance anywhere; plus the known-answer cases of tests/test_depthmap_cpu.py on the device."""
import ctypes as C
import importlib

import numpy as np
import pytest

import render_common as rc
from cloud_common import assert_same as assert_same_nn
from render_common import check_borders, check_threshold, check_two_layers

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def cloud(engine):
    return importlib.import_module("mp-mvs_amd.cloud")


@pytest.fixture(scope="module")
def scene(pm):
    """smoke()'s scene, the points of views 1-3 (18 432), and six cameras: the scene's four, a 50 x 37 one and a 1 x 1 one"""
    sc = pm.synth.make_problem_scene(96, 64, n_src=3, spacing=0.5)
    xyz = np.concatenate([rc.backproject(sc.views[i]) for i in (1, 2, 3)])
    assert xyz.shape == (18432, 3) and xyz.dtype == f32
    cams = [v.cam for v in sc.views]
    cams.append(pm.synth.scene_cameras(50, 37, [(0.1, -0.2, 0.3)], rot_deg=6.0)[0])
    cams.append(pm.synth.scene_cameras(1, 1, [(0.0, 0.0, 0.0)], rot_deg=0.0)[0])
    return sc, xyz, cams


@pytest.fixture(scope="module")
def scene_cloud(cloud, scene):
    with cloud.Cloud(scene[1]) as c:
        yield c


def check(c, xyz, cams, splat, occl_rel, want_idx=True):
    got = c.render_depth(cams, splat, occl_rel, want_idx=want_idx)
    wd, wi = rc.render_statement(xyz, cams, splat, occl_rel)
    if want_idx:
        rc.assert_same(got[0], got[1], wd, wi)
        for d, i in zip(*got):
            assert np.array_equal(i == -1, d == 0)
    else:
        rc.assert_same(got, None, wd, wi)
    return got


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("want_idx", [True, False])
@pytest.mark.parametrize("occl_rel", [0.0, 0.02])
@pytest.mark.parametrize("splat", [0, 1, 2])
def test_synthetic_scene(scene, scene_cloud, splat, occl_rel, want_idx):
    sc, xyz, cams = scene
    got = check(scene_cloud, xyz, cams, splat, occl_rel, want_idx)
    depths = got[0] if want_idx else got
    assert [d.shape for d in depths] == [(64, 96)] * 4 + [(37, 50), (1, 1)]
    if (splat, occl_rel) == (1, 0.02):
        gt = sc.views[0].gt_depth
        covered = depths[0] != 0
        rel = np.abs(depths[0].astype(np.float64) - gt)[covered] / gt[covered]
        print(f"view 0: covered share {covered.mean():.4f}, largest relative error {rel.max():.3e}")
        assert covered.mean() >= 0.99 and rel.max() <= 5e-3


# 2 ---------------------------------------------------------------------------------------------------------------------------
def test_junk(cloud, scene):
    rng = np.random.default_rng(21)
    n = 150000
    xyz = np.stack([rng.uniform(-4, 4, n), rng.uniform(-4, 4, n), rng.uniform(-2, 8, n)], 1).astype(f32)   # z < 0: behind the cameras
    bad = rng.choice(n, n // 100, replace=False)
    xyz[bad, rng.integers(0, 3, len(bad))] = rng.choice(np.array([np.nan, np.inf, -np.inf], f32), len(bad))
    far = rng.choice(n, 12, replace=False)
    xyz[far[:4], 2] = 1e30
    xyz[far[4:8]] = f32(3e38)          # the sums of the projection overflow
    xyz[far[8:], 0] = -1e30
    cams = scene[2][:2] + scene[2][4:5]
    with cloud.Cloud(xyz) as c:
        for splat, occl_rel in ((1, 0.02), (2, 0.0)):
            depths, idxs = check(c, xyz, cams, splat, occl_rel)
    assert all(np.isfinite(d).all() and (d >= 0).all() for d in depths) and 0 < (depths[0] != 0).sum()
    assert not np.isin(np.concatenate([i.ravel() for i in idxs]), bad).any()


# 3, 4, 5: the known answers of the CPU tests, now from the device --------------------------------------------------------------
def test_borders(cloud):
    cam, xyz, xs, ys = rc.borders_case()
    with cloud.Cloud(xyz) as c:
        for splat in (0, 1):
            d, i = check(c, xyz, [cam], splat, 0.02)
            check_borders(d[0], i[0])


@pytest.mark.parametrize("occl_rel", [0.02, 0.0])
def test_visibility_threshold(cloud, occl_rel):
    cam, xyz, zb, zb2 = rc.threshold_case(occl_rel)

    def render(pts, splat):
        with cloud.Cloud(pts) as c:
            return check(c, pts, [cam], splat, occl_rel)[0][0]
    check_threshold(render, occl_rel)


def test_two_layers(cloud):
    sc, cam, xyz, n_back, _ = rc.two_layer_case()
    with cloud.Cloud(xyz) as c:
        def render(pts, splat, occl_rel):
            d, i = check(c, pts, [cam], splat, occl_rel)
            return d[0], i[0]
        through = check_two_layers(render)
    assert through == 4004   # what the statement gives (test_depthmap_cpu.test_statement_two_layers)


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_ties_and_order(cloud, scene, scene_cloud):
    sc, xyz, cams = scene
    n = len(xyz)
    base_d, base_i = scene_cloud.render_depth(cams, 1, 0.02, want_idx=True)
    x3 = np.concatenate([xyz, xyz, xyz])
    with cloud.Cloud(x3) as c:
        d3, i3 = check(c, x3, cams, 1, 0.02)
    for d, i, bd, bi in zip(d3, i3, base_d, base_i):
        assert np.array_equal(rc.bits(d), rc.bits(bd)) and np.array_equal(i, bi) and i.max() < n   # always the first copy
    perm = np.random.default_rng(4).permutation(n)
    xp = xyz[perm]
    with cloud.Cloud(xp) as c:
        dp, ip = check(c, xp, cams, 1, 0.02)
    for d, i, bd, bi in zip(dp, ip, base_d, base_i):
        assert np.array_equal(rc.bits(d), rc.bits(bd))
        seen = bi >= 0
        assert np.array_equal(seen, i >= 0) and np.array_equal(rc.bits(xp[i[seen]]), rc.bits(xyz[bi[seen]]))


# 7 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splat", [8, 0])
def test_window_against_image(pm, scene, scene_cloud, splat):
    small = pm.synth.scene_cameras(5, 4, [(0.0, 0.0, 0.0), (0.3, 0.1, 0.0)])
    d, i = check(scene_cloud, scene[1], small, splat, 0.02)
    assert (d[0] != 0).any()
    if splat == 8:   # the window is the whole image: what stays is within the factor of the view's nearest point
        for m in d:
            assert (m[m != 0] <= m[m != 0].min() * (f32(1) + f32(0.02))).all()


# 8 ---------------------------------------------------------------------------------------------------------------------------
def test_size(pm, cloud):
    sc = pm.synth.make_problem_scene(160, 120, n_src=5, spacing=0.4)
    rng = np.random.default_rng(8)
    pts = np.concatenate([rc.backproject(v) for v in sc.views])          # 115 200 surface points
    pts = np.concatenate([pts, pts + rng.normal(0, 0.01, pts.shape).astype(f32),
                          np.stack([rng.uniform(-4, 4, 69600), rng.uniform(-4, 4, 69600), rng.uniform(1, 7, 69600)], 1).astype(f32)])
    assert len(pts) == 300000
    cams = [v.cam for v in sc.views]
    assert len(cams) == 6
    with cloud.Cloud(pts) as c:
        d, i = check(c, pts, cams, 1, 0.02)
        total, passes = c.render_ms()
    assert total > 0 and passes["zmin"] > 0 and passes["index"] > 0 and passes["resolve"] > 0
    assert all((m != 0).any() for m in d)


def test_more_views_than_a_chunk(pm, scene, scene_cloud):
    # the point passes take 8 views per launch (kRenderChunk of csrc/pm_render.hpp): 9 views of different sizes are two launches
    cams = [pm.synth.scene_cameras(40 + 7 * k, 50 - 3 * k, [(0.1 * k - 0.4, 0.05 * k, 0.0)], seed=k)[0] for k in range(9)]
    check(scene_cloud, scene[1], cams, 1, 0.02)
    check(scene_cloud, scene[1], cams, 2, 0.02, want_idx=False)
    total, passes = scene_cloud.render_ms()
    assert passes["index"] == 0 and total > 0


# 9, 10: the C interface itself --------------------------------------------------------------------------------------------------
def raw_render(engine, handle, cams, splat, occl_rel, depths, idxs, n_views=None, null_cams=False, null_depths=False):
    """mpmvs_cloud_render_depth with explicit buffers; depths / idxs: lists of arrays or None entries, idxs may be None"""
    _abi = importlib.import_module("mp-mvs_amd._abi")
    f = engine.load()[1]
    n = len(cams) if n_views is None else n_views
    arr = (_abi.Camera * max(len(cams), 1))(*cams)
    dp = (C.c_void_p * max(len(depths), 1))(*[None if d is None else d.ctypes.data for d in depths])
    ip = None if idxs is None else (C.c_void_p * max(len(idxs), 1))(*[None if i is None else i.ctypes.data for i in idxs])
    rc_ = f["cloud_render_depth"](handle, n, None if null_cams else arr, splat, occl_rel, None if null_depths else dp, ip)
    return rc_, (f["last_error"](None) or b"").decode()


def test_degenerate(engine, cloud, scene, scene_cloud):
    sc, xyz, cams = scene
    for pts in (np.zeros((0, 3), f32), np.array([[np.nan, 0, 0], [0, np.inf, 0], [1, 2, -np.inf]], f32)):
        with cloud.Cloud(pts) as c:
            d, i = check(c, pts, cams[3:], 1, 0.02)
            assert all((m == 0).all() for m in d) and all((m == -1).all() for m in i)
            assert c.render_ms()[0] == 0
    assert scene_cloud.render_depth([], 1, 0.02) == [] and scene_cloud.render_depth([], want_idx=True) == ([], [])
    # n_views == 0 leaves the outputs untouched
    d = [np.full((64, 96), 7.0, f32)]
    i = [np.full((64, 96), 7, np.int32)]
    assert raw_render(engine, scene_cloud._h, cams[:1], 1, 0.02, d, i, n_views=0)[0] == 0
    assert (d[0] == 7).all() and (i[0] == 7).all()
    # out_idx NULL, and with NULL entries
    wd, wi = rc.render_statement(xyz, cams[:3], 1, 0.02)
    d = [np.full((64, 96), 7.0, f32) for _ in range(3)]
    assert raw_render(engine, scene_cloud._h, cams[:3], 1, 0.02, d, None)[0] == 0
    rc.assert_same(d, None, wd, wi)
    d = [np.full((64, 96), 7.0, f32) for _ in range(3)]
    i = [None, np.full((64, 96), 7, np.int32), None]
    assert raw_render(engine, scene_cloud._h, cams[:3], 1, 0.02, d, i)[0] == 0
    rc.assert_same(d, i, wd, wi)
    i = [None, None, None]
    assert raw_render(engine, scene_cloud._h, cams[:3], 2, 0.0, d, i)[0] == 0
    rc.assert_same(d, None, *rc.render_statement(xyz, cams[:3], 2, 0.0))


def test_errors(engine, cloud, scene, scene_cloud):
    import copy
    sc, xyz, cams = scene
    h = scene_cloud._h
    d = [np.full((64, 96), 7.0, f32), np.full((64, 96), 7.0, f32)]
    two = cams[:2]

    def sized(w, hh):
        c = copy.copy(cams[0])
        c.width, c.height = w, hh
        return c
    cases = [
        (-2, dict(handle=None)), (-2, dict(null_cams=True)), (-2, dict(null_depths=True)), (-2, dict(depths=[d[0], None])),
        (-2, dict(n_views=-1)),
        (-2, dict(cams=[cams[0], sized(0, 64)])), (-2, dict(cams=[cams[0], sized(96, -1)])),
        (-2, dict(splat=-1)), (-2, dict(splat=9)),
        (-2, dict(occl_rel=float("nan"))), (-2, dict(occl_rel=float("inf"))), (-2, dict(occl_rel=-0.01)),
        (-3, dict(cams=[cams[0], sized((1 << 24) + 1, 1)])), (-3, dict(cams=[cams[0], sized(1, (1 << 24) + 1)])),
        (-3, dict(cams=[cams[0], sized(1 << 16, 1 << 15)])), (-3, dict(cams=[cams[0], sized(1 << 16, 1 << 16)])),
    ]
    for code, kw in cases:
        args = dict(handle=h, cams=two, splat=1, occl_rel=0.02, depths=d, idxs=None)
        args.update(kw)
        got, text = raw_render(engine, args.pop("handle"), args.pop("cams"), args.pop("splat"), args.pop("occl_rel"), args.pop("depths"), args.pop("idxs"), **args)
        assert got == code and text.startswith("cloud render:"), (kw, got, text)
        assert (d[0] == 7).all() and (d[1] == 7).all()   # found before anything is written
    # splat and occl_rel are also checked when there is no view
    assert raw_render(engine, h, two, 9, 0.02, d, None, n_views=0)[0] == -2
    # (-100, a HIP failure, is not provoked)
    with pytest.raises(ValueError, match="splat"):
        scene_cloud.render_depth(two, splat=9)
    # the handle still works
    check(scene_cloud, xyz, two, 1, 0.02)


# 11 --------------------------------------------------------------------------------------------------------------------------
def test_interleaving(cloud, scene):
    sc, xyz, cams = scene
    q = (xyz[::7] + f32(0.003)).astype(f32)
    with cloud.Cloud(xyz) as c:
        a = c.nearest(q, 0.05)
        assert c.kernel_ms()[1] > 0
        check(c, xyz, cams, 1, 0.02)
        b = c.nearest(q, 0.05)
        assert c.kernel_ms()[1] == 0          # the grid of the first search is still there
        st = c.stats()
    assert_same_nn(b, a)
    assert st["finite"] == len(xyz)


# 12 --------------------------------------------------------------------------------------------------------------------------
def test_end_to_end(pm, engine, scene, scene_cloud):
    """smoke()'s Problem through PatchMatch, scored against the rendered ground truth and against the analytic one over the
    covered pixels.  |est - rendered| differs from |est - analytic| by at most delta = max |rendered - analytic|, so the count
    within t of the rendered map lies between the analytic counts at t - delta and t + delta."""
    depthmap = importlib.import_module("mp-mvs_amd.depthmap")
    sc, xyz, cams = scene
    pcams, imgs = sc.problem(0, [1, 2, 3])
    dmin, dmax = pm.synth.kernel_depth_range(pcams[0])
    prm = pm.PatchMatchParams(num_images=4, depth_min=float(dmin), depth_max=float(dmax), max_scale=1)
    gpu = engine.create(0)
    gpu.set_views(pcams, imgs)
    gpu.run(prm, 12345)
    est = np.ascontiguousarray(gpu.get()[0][..., 3])
    rendered = scene_cloud.render_depth(cams[:1], 1, 0.02)[0]
    stated = rc.render_one(cams[0], xyz, 1, 0.02)[0]
    assert np.array_equal(rc.bits(rendered), rc.bits(stated))
    covered = stated != 0
    analytic = np.where(covered, sc.views[0].gt_depth, f32(0)).astype(f32)
    delta = float(np.abs(stated.astype(np.float64) - analytic)[covered].max())
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


# the CLI's rendered path ----------------------------------------------------------------------------------------------------
def test_eval_depth_rendered(pm, hostlib, scene, tmp_path, capsys):
    """tools/eval_depth.py --ground_truth in process: a folder of smoke's scene with half-size depth maps, the scan as a PLY
    moved by a transform that --transform undoes; each view's score is that against the statement's render at the map's size"""
    import importlib.util
    import os
    depthmap = importlib.import_module("mp-mvs_amd.depthmap")
    spec = importlib.util.spec_from_file_location("eval_depth_tool", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "eval_depth.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    sc, xyz, cams = scene
    dense = tmp_path / "dense"
    hostlib.write_dataset(str(dense), cams[:4], [np.rint(v.image) for v in sc.views], [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]])
    est = {}
    for i in (0, 2):
        est[i] = np.ascontiguousarray(sc.views[i].gt_depth[::2, ::2]) + f32(0.01)
        os.makedirs(dense / "MPMVS" / f"2333_{i:08d}")
        hostlib.write_dmb(str(dense / "MPMVS" / f"2333_{i:08d}" / "depths.dmb"), est[i])
    moved = (xyz.astype(np.float64) * 2.0 + np.array([1.0, -2.0, 0.5])).astype(f32)
    rec = np.zeros((len(moved), 9), f32)
    rec[:, :3] = moved
    hostlib.write_ply(str(tmp_path / "scan.ply"), rec)
    T = np.eye(4)
    T[:3, :3] *= 0.5
    T[:3, 3] = [-0.5, 1.0, -0.25]
    np.savetxt(tmp_path / "T.txt", T)
    res = tool.main(["--dense_folder", str(dense), "--ground_truth", str(tmp_path / "scan.ply"), "--transform", str(tmp_path / "T.txt"),
                     "--tolerances", "0.02,0.1", "--splat", "1", "--occl", "0.05"])
    capsys.readouterr()
    back = tool.apply_transform(moved, T)
    assert sorted(res["views"]) == ["00000000", "00000002"] and res["ground_truth"] == "rendered" and res["render_device_ms"] > 0
    for i in (0, 2):
        cam = depthmap.camera_at_size(hostlib.read_camera(str(dense / "cams" / f"{i:08d}_cam.txt")), 96, 64, 48, 32)
        want = depthmap.score(est[i], rc.render_one(cam, back, 1, 0.05)[0], [0.02, 0.1])
        assert res["views"][f"{i:08d}"] == want and want["n_gt"] > 0.9 * 48 * 32
        assert want["tolerances"][1]["within"] > 0.9 * want["n_gt"]
