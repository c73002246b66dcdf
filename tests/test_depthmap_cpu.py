"""mp-mvs_amd/depthmap.py, tools/eval_depth.py without a scan, and the numpy statement of the render (tests/render_common.py)
on its known-answer cases: what the GPU tests compare against is pinned here without a GPU."""
import importlib
import importlib.util
import json
import os

import numpy as np
import pytest

import render_common as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def depthmap(pm):
    return importlib.import_module("mp-mvs_amd.depthmap")


@pytest.fixture(scope="module")
def eval_depth(pm):
    spec = importlib.util.spec_from_file_location("eval_depth_tool", os.path.join(ROOT, "tools", "eval_depth.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the statement -----------------------------------------------------------------------------------------------------
def test_statement_borders(pm):
    cam, xyz, xs, ys = rc.borders_case()
    assert xs[1] == f32(-0.5) and xs[3] == np.nextafter(f32(6.5), f32(0)) and ys[3] == np.nextafter(f32(4.5), f32(0))
    ok, px, py, z = rc.project(cam, xyz)
    # per axis and layer: -0.5 and its upper neighbour land, and the float below the far edge; the other three do not
    assert ok.tolist() == [False, True, True, True, False, False] * 4
    assert px[:6][ok[:6]].tolist() == [0, 0, 6] and py[6:12][ok[6:12]].tolist() == [0, 0, 4]
    for splat in (0, 1):
        rc.check_borders(*rc.render_one(cam, xyz, splat, 0.02))


@pytest.mark.parametrize("occl_rel", [0.02, 0.0])
def test_statement_threshold(pm, occl_rel):
    cam = rc.threshold_case(occl_rel)[0]
    rc.check_threshold(lambda xyz, splat: rc.render_one(cam, xyz, splat, occl_rel)[0], occl_rel)


def test_statement_two_layers(pm):
    through = rc.check_two_layers(lambda xyz, splat, occl: rc.render_one(rc.two_layer_case()[1], xyz, splat, occl))
    assert through == 4004   # 58 x 78 hull pixels less the 20 x 26 samples inside it (column 118 lies outside): every gap shows the back


def test_statement_window_min():
    a = np.arange(20, dtype=f32).reshape(4, 5)[::-1].copy()
    assert np.array_equal(rc.window_min(a, 0), a)
    assert (rc.window_min(a, 8) == 0).all()
    w1 = rc.window_min(a, 1)
    assert w1[0, 0] == a[1, 0] and w1[3, 4] == a[3, 3] and w1[1, 2] == a[2, 1]


# ---- score ---------------------------------------------------------------------------------------------------------------
def test_score_by_hand(depthmap):
    inf, nan = np.inf, np.nan
    gt = np.array([[1.0, 2.0, 4.0], [0.0, inf, -1.0], [8.0, 10.0, nan]], f32)
    est = np.array([[1.1, 2.5, 0.0], [3.0, 3.0, 3.0], [inf, 9.0, 1.0]], f32)
    # G: (0,0) (0,1) (0,2) (2,0) (2,1); E: (0,0) (0,1) (2,1); err: fl(1.1) - 1, 0.5, 1
    e00 = float(f32(1.1) - f32(1.0))
    s = depthmap.score(est, gt, [e00, 0.5, 0.99, 1.0])
    assert (s["n_gt"], s["n_est"]) == (5, 3)
    assert [r["within"] for r in s["tolerances"]] == [1, 2, 2, 3]          # the bound is inclusive
    assert s["tolerances"][1]["completeness"] == 2 / 5 and s["tolerances"][1]["accuracy"] == 2 / 3
    assert s["median_error"] == 0.5
    assert depthmap.score(est, gt, [np.nextafter(f32(e00), f32(0))])["tolerances"][0]["within"] == 0
    r = depthmap.score(est, gt, [0.1, 0.25, float(np.nextafter(f32(0.25), f32(0)))], relative=True)
    # bounds t * gt: (0,0) fl(0.1) * 1 against fl(1.1) - 1 = 0.10000002; (0,1) 0.5 against 0.5; (2,1) 2.5 against 1
    assert [x["within"] for x in r["tolerances"]] == [int(f32(e00) <= f32(0.1)) + 1, 3, 2]
    assert f32(e00) > f32(0.1)
    empty = depthmap.score(np.zeros((2, 2), f32), np.zeros((2, 2), f32), [0.1])
    assert empty["n_gt"] == 0 and empty["median_error"] is None and empty["tolerances"][0] == {"tolerance": 0.1, "within": 0, "completeness": 0.0, "accuracy": 0.0}
    no_est = depthmap.score(np.zeros((2, 2), f32), np.ones((2, 2), f32), [0.1])
    assert no_est["n_gt"] == 4 and no_est["n_est"] == 0 and no_est["tolerances"][0]["accuracy"] == 0.0 and no_est["median_error"] is None
    p = depthmap.pool([s, s, depthmap.score(np.ones((2, 2), f32), np.ones((2, 2), f32), [e00, 0.5, 0.99, 1.0])])
    assert (p["n_gt"], p["n_est"]) == (14, 10) and [x["within"] for x in p["tolerances"]] == [6, 8, 8, 10]
    assert p["tolerances"][0]["completeness"] == 6 / 14 and p["tolerances"][0]["accuracy"] == 6 / 10
    assert depthmap.pool([])["n_gt"] == 0
    with pytest.raises(ValueError):
        depthmap.pool([s, empty])
    with pytest.raises(ValueError):
        depthmap.score(est, gt[:2], [0.1])


# ---- readers ---------------------------------------------------------------------------------------------------------------
def test_read_eth3d_depth(depthmap, tmp_path):
    a = np.random.default_rng(1).uniform(0.5, 9.0, (5, 7)).astype(f32)
    raw = a.copy()
    raw[0, 0], raw[1, 2], raw[2, 3], raw[4, 6] = np.inf, np.nan, -2.0, 0.0
    p = tmp_path / "gt"
    p.write_bytes(raw.astype("<f4").tobytes())
    got = depthmap.read_eth3d_depth(p, 7, 5)
    want = a.copy()
    want[0, 0] = want[1, 2] = want[2, 3] = want[4, 6] = 0.0
    assert got.dtype == f32 and np.array_equal(got, want)
    for w, h in ((5, 7 + 1), (7, 4), (0, 0)):
        with pytest.raises(ValueError):
            depthmap.read_eth3d_depth(p, w, h)
    p.write_bytes(raw.tobytes()[:-1])
    with pytest.raises(ValueError):
        depthmap.read_eth3d_depth(p, 7, 5)


def test_read_colmap_map(depthmap, tmp_path):
    rng = np.random.default_rng(2)
    d = rng.uniform(0.0, 9.0, (4, 6)).astype(f32)
    n = rng.normal(size=(4, 6, 3)).astype(f32)
    depthmap.write_colmap_map(tmp_path / "d.bin", d)
    depthmap.write_colmap_map(tmp_path / "n.bin", n)
    assert (tmp_path / "d.bin").read_bytes().startswith(b"6&4&1&")
    got_d, got_n = depthmap.read_colmap_map(tmp_path / "d.bin"), depthmap.read_colmap_map(tmp_path / "n.bin")
    assert got_d.shape == (4, 6) and np.array_equal(got_d, d) and got_n.shape == (4, 6, 3) and np.array_equal(got_n, n)
    body = d.tobytes()
    for bad in (b"6&4&1&" + body[:-4], b"6&4&1&" + body + b"\0", b"6&4&1" + body, b"6 4 1&" + body, b"-6&4&1&" + body, b"0&4&1&", b"6&4&&" + body, b""):
        (tmp_path / "bad.bin").write_bytes(bad)
        with pytest.raises(ValueError):
            depthmap.read_colmap_map(tmp_path / "bad.bin")


def test_camera_at_size(pm, depthmap):
    cam = pm.synth.scene_cameras(160, 120, [(0.1, 0.2, 0.0)], focal_jitter=0.1)[0]
    out = depthmap.camera_at_size(cam, 160, 120, 53, 41)
    sx, sy = f32(53) / f32(160), f32(41) / f32(120)
    K = np.array(list(cam.K), f32)
    want = K.copy()
    want[0], want[2], want[4], want[5] = K[0] * sx, K[2] * sx, K[4] * sy, K[5] * sy
    assert np.array_equal(np.array(list(out.K), f32), want) and want[0] != K[0]
    assert (out.width, out.height) == (53, 41) and (cam.width, cam.height) == (160, 120) and list(cam.K) == K.tolist()
    assert list(out.R) == list(cam.R) and list(out.t) == list(cam.t) and list(out.C) == list(cam.C)
    same = depthmap.camera_at_size(cam, 160, 120, 160, 120)
    assert list(same.K) == list(cam.K) and (same.width, same.height) == (160, 120)


# ---- tools/eval_depth.py without a scan ------------------------------------------------------------------------------------
def test_eval_depth_dmb_folders(pm, hostlib, depthmap, eval_depth, tmp_path, capsys):
    W, H = 12, 9
    cams = pm.synth.scene_cameras(W, H, [(0, 0, 0), (0.2, 0, 0), (0, 0.2, 0)])
    rng = np.random.default_rng(3)
    imgs = [np.rint(rng.uniform(0, 255, (H, W))).astype(f32) for _ in cams]
    dense = tmp_path / "dense"
    hostlib.write_dataset(str(dense), cams, imgs, [[1, 2], [0, 2], [0, 1]])
    gt = [rng.uniform(3.0, 8.0, (H, W)).astype(f32) for _ in cams]
    est = [g + rng.normal(0, 0.05, (H, W)).astype(f32) for g in gt]
    est[0][0, :4] = 0.0
    gt[1][2, :] = 0.0
    a_root, b_root = dense / "MPMVS", tmp_path / "other"
    for i in (0, 1):           # view 2 has no result folder: not scored
        for root, maps in ((a_root, est), (b_root, gt)):
            os.makedirs(root / f"2333_{i:08d}")
            hostlib.write_dmb(str(root / f"2333_{i:08d}" / "depths.dmb"), maps[i])
    os.makedirs(a_root / "2333_00000002")   # a result folder without the map
    argv = ["--dense_folder", str(dense), "--gt_depth_dir", str(b_root), "--gt_format", "dmb", "--tolerances", "0.02,0.1"]
    res = eval_depth.main(argv)
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == res
    assert sorted(res["views"]) == ["00000000", "00000001"] and res["render_device_ms"] is None and res["ground_truth"] == "dmb"
    want = [depthmap.score(est[i], gt[i], [0.02, 0.1]) for i in (0, 1)]
    assert res["views"]["00000000"] == want[0] and res["views"]["00000001"] == want[1] and res["pooled"] == depthmap.pool(want)
    assert want[0]["n_est"] == H * W - 4 and want[1]["n_gt"] == H * W - W and 0 < want[0]["tolerances"][0]["within"] < want[0]["tolerances"][1]["within"]
    assert set(res["seconds"]) == {"read", "ground_truth", "score"}
    # --result_folder, --relative, and the other two formats through --gt_pattern
    gdir = tmp_path / "gtfiles"
    os.makedirs(gdir)
    for i in (0, 1):
        (gdir / f"{i:08d}.raw").write_bytes(gt[i].astype("<f4").tobytes())
        depthmap.write_colmap_map(gdir / f"{i}.geometric.bin", gt[i])
    rel = eval_depth.main(["--dense_folder", str(dense), "--result_folder", str(a_root), "--gt_depth_dir", str(gdir), "--gt_format", "eth3d",
                           "--gt_pattern", "{id:08d}.raw", "--tolerances", "0.01", "--relative"])
    assert rel["views"]["00000001"] == depthmap.score(est[1], gt[1], [0.01], relative=True)
    col = eval_depth.main(["--dense_folder", str(dense), "--gt_depth_dir", str(gdir), "--gt_format", "colmap", "--gt_pattern", "{id}.geometric.bin",
                           "--tolerances", "0.02,0.1"])
    assert col["views"] == res["views"]
    # a ground-truth map of another size is refused, naming both sizes
    hostlib.write_dmb(str(b_root / "2333_00000001" / "depths.dmb"), gt[1][:, :-1])
    with pytest.raises(SystemExit) as e:
        eval_depth.main(argv)
    assert f"{W - 1} x {H}" in str(e.value) and f"{W} x {H}" in str(e.value)
    for bad in (["--dense_folder", str(dense)], argv + ["--ground_truth", "scan.ply"], argv[:-4] + ["--tolerances", "0.1"], argv + ["--tolerances", "0,1"],
                ["--dense_folder", str(tmp_path)] + argv[2:], argv + ["--map", "nothing.dmb"]):
        with pytest.raises(SystemExit):
            eval_depth.main(bad)
