"""mpmvs_align_* on the GPU against the numpy statement (tests/align_common.py): array_equal on all 18 sums and on the frame;
mpmvs_align_icp against the loop over the two public calls and against the loop over the statement, bit for bit."""
import ctypes as C
import importlib
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import align_common as ac

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I4 = np.eye(4)


@pytest.fixture(scope="module")
def cloud(engine):
    return importlib.import_module("mp-mvs_amd.cloud")


def check(cloud, t, s, M, radius):
    with cloud.Cloud(t) as c, cloud.Aligner(c, s) as al:
        sums, frame = al.sums(radius, M)
    want, wframe = ac.brute_sums(t, s, M, radius)
    assert np.array_equal(frame, wframe), (frame, wframe)
    assert np.array_equal(sums, want), (sums - want)
    return sums, frame


def moved():
    return ac.similarity(np.random.default_rng(2), 0.05, 1.03, 0.02)


@pytest.fixture(scope="module")
def random_clouds():
    rng = np.random.default_rng(11)
    return rng.random((1500, 3), dtype=np.float32), rng.random((1000, 3), dtype=np.float32)


@pytest.mark.parametrize("transform", ["identity", "similarity"])
@pytest.mark.parametrize("radius", [0.02, 0.2, 4.0])
def test_random(cloud, random_clouds, radius, transform):
    t, s = random_clouds
    sums, frame = check(cloud, t, s, I4 if transform == "identity" else moved(), radius)
    if radius == 0.02:
        assert 0 < sums[0] < len(s)
    if radius == 4.0:
        assert sums[0] == len(s) and frame[3] == 16.0


@pytest.mark.parametrize("n_s", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_wave_and_block_borders(cloud, random_clouds, n_s):
    t, s = random_clouds
    sums, _ = check(cloud, t, s[:n_s], I4, 0.2)
    assert sums[0] == n_s


@pytest.mark.parametrize("kind", ["negative", "mixed"])
@pytest.mark.parametrize("n_s", [64, 600])
def test_carry_and_sign(cloud, kind, n_s):
    """targets at the corners +-(1 - 2^-5) with radius 2^-6: half the extent plus two radii is exactly 1 = u, so a and b are
    ~ +-0.97 and every fixed value ~ +-2^30; 64 of them pass 2^32 within one wave, 600 pass 2^38 across blocks"""
    rng = np.random.default_rng(n_s)
    corners = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float32) * np.float32(0.96875)
    pick = np.zeros(n_s, int) if kind == "negative" else rng.integers(0, 8, n_s)
    s = (corners[pick] * (1 - rng.random((n_s, 1)) * 2.0 ** -12)).astype(np.float32)
    sums, frame = check(cloud, corners, s, I4, 2.0 ** -6)
    assert frame[3] == 1.0 and sums[0] == n_s
    if kind == "negative":
        assert (sums[1:7] < -0.96 * n_s * 2 ** 30).all() and sums[1] < -(2 ** 32 if n_s == 64 else 2 ** 38)
        assert (sums[7:17] > 0.9 * n_s * 2 ** 30).all()
    else:
        assert (sums[7:17:4] > 0.9 * n_s * 2 ** 30).all()   # the products on the diagonal add up whatever the signs
        assert np.abs(sums[1:7]).max() < 0.5 * n_s * 2 ** 30


def test_ties_and_duplicates(cloud):
    rng = np.random.default_rng(5)
    base = rng.random((300, 3), dtype=np.float32)
    t = np.concatenate([base, base[rng.choice(300, 100, replace=False)]])
    t = t[rng.permutation(400)]
    check(cloud, t, np.concatenate([t, base + np.float32(0.001)]), I4, 0.6)
    # equidistant from two distinct targets: the smaller index enters the sums, so swapping the two changes them
    t2 = np.array([[0, 0, 0], [1, 0, 0], [0.5, 1, 0]], np.float32)
    s2 = np.array([[0.5, 0, 0]], np.float32)
    a, _ = check(cloud, t2, s2, I4, 0.75)
    b, _ = check(cloud, t2[[1, 0, 2]], s2, I4, 0.75)
    assert a[0] == b[0] == 1 and a[4] < 0 < b[4]


def test_nonfinite_and_empty(cloud):
    rng = np.random.default_rng(9)
    t = rng.random((700, 3), dtype=np.float32)
    s = rng.random((500, 3), dtype=np.float32)
    t[[3, 77], [0, 2]] = [np.nan, np.inf]
    s[[0, 64, 499], [1, 0, 2]] = [np.nan, -np.inf, np.inf]
    s[5] = 1e30
    sums, _ = check(cloud, t, s, I4, 0.2)
    assert 0 < sums[0] <= 496
    big = I4.copy()
    big[0, 0] = 1e300   # finite, but every image overflows fp32
    assert not check(cloud, t, s, big, 0.2)[0].any()
    assert not check(cloud, t, s + np.float32(10), I4, 0.2)[0].any()   # nothing within the radius
    sums, frame = check(cloud, t, np.zeros((0, 3), np.float32), I4, 0.2)
    assert not sums.any() and frame[3] == 1.0
    sums, frame = check(cloud, np.full((4, 3), np.nan, np.float32), s, I4, 0.2)
    assert not sums.any() and not frame.any()
    sums, frame = check(cloud, np.zeros((0, 3), np.float32), s, I4, 0.2)
    assert not sums.any() and not frame.any()


def test_icp_is_the_loop_of_the_public_calls(cloud):
    target, src, T_true, T0 = ac.icp_scene()
    eps = 2.0 ** -20
    with cloud.Cloud(target) as c, cloud.Aligner(c, src) as al:
        got = al.icp(0.05, T0, True, 30, eps)
        loop = cloud.icp_loop(al.sums, 0.05, T0, True, 30, eps)
        one = al.icp(0.05, T0, True, 1, eps)
        rigid = al.icp(0.05, T0, False, 30, eps)
        rigid_loop = cloud.icp_loop(al.sums, 0.05, T0, False, 30, eps)
    stated = cloud.icp_loop(lambda r, M: ac.brute_sums(target, src, M, r), 0.05, T0, True, 30, eps)
    for other in (loop, stated):
        assert np.array_equal(got[0], other[0]) and got[1:] == other[1:], (got, other)
    assert np.array_equal(rigid[0], rigid_loop[0]) and rigid[1:] == rigid_loop[1:]
    assert 1 < got[1] < 30 and got[2] == 1200
    assert one[1] == 1 and not np.array_equal(one[0], ac.m34(T0))
    assert np.abs(got[0] - T_true[:3]).max() < 1e-6


def test_two_aligners_and_grid_reuse(cloud, random_clouds):
    t, s = random_clouds
    with cloud.Cloud(t) as c:
        c.nearest(s[:10], 0.2)
        assert c.kernel_ms()[1] > 0
        with cloud.Aligner(c, s) as a1, cloud.Aligner(c, s[:300]) as a2:
            s1, _ = a1.sums(0.2, I4)
            assert c.kernel_ms()[1] == 0   # the grid of the nearest() call served the pass
            assert a1.ms() > 0
            s2, _ = a2.sums(0.2, moved())
            s1b, _ = a1.sums(0.2, I4)
        c.nearest(s[:10], 0.2)
        assert c.kernel_ms()[1] == 0
    assert np.array_equal(s1, ac.brute_sums(t, s, I4, 0.2)[0]) and np.array_equal(s1, s1b)
    assert np.array_equal(s2, ac.brute_sums(t, s[:300], moved(), 0.2)[0])


def test_frame_on_the_host_and_close_order(cloud, random_clouds):
    t, s = random_clouds
    c = cloud.Cloud(t)
    al = cloud.Aligner(c, s)
    for r in (0.02, 0.2, 4.0):
        assert np.array_equal(c.frame(r), al.sums(r, I4)[1])
    c.close()   # closes its aligner first
    assert al._h is None and c._h is None
    al.close()
    with cloud.Cloud(np.full((2, 3), np.nan, np.float32)) as e:
        assert not e.frame(0.2).any()


UNBINNED = """
import importlib, sys
import numpy as np
sys.path[:0] = [{root!r}, {tests!r}]
import align_common as ac
cloud = importlib.import_module("mp-mvs_amd.cloud")
rng = np.random.default_rng(11)
t, s = rng.random((1500, 3), dtype=np.float32), rng.random((1000, 3), dtype=np.float32)
M = ac.similarity(np.random.default_rng(2), 0.05, 1.03, 0.02)
with cloud.Cloud(t) as c, cloud.Aligner(c, s) as al:
    for r in (0.02, 0.2):
        got, want = al.sums(r, M), ac.brute_sums(t, s, M, r)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), r
print("unbinned equal")
"""


def test_caller_order_pass(cloud):
    """MPMVS_CLOUD_BIN=0 is read once per process, so the unbinned pass runs in a child"""
    env = dict(os.environ, MPMVS_CLOUD_BIN="0")
    out = subprocess.run([sys.executable, "-c", UNBINNED.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "unbinned equal" in out.stdout, out.stderr[-2000:]


def test_error_codes(cloud, engine, random_clouds):
    t, s = random_clouds
    _, f = engine.load()
    PD, PL = C.POINTER(C.c_double), C.POINTER(C.c_longlong)
    m = np.ascontiguousarray(I4[:3]).reshape(12)
    sums, frame = np.zeros(18, np.int64), np.zeros(4)
    mp, sp, fp = m.ctypes.data_as(PD), sums.ctypes.data_as(PL), frame.ctypes.data_as(PD)
    h = C.c_void_p(None)
    with cloud.Cloud(t) as c:
        assert f["align_create"](None, 3, s.ctypes.data, C.byref(h)) == -2
        assert f["align_create"](c._h, -1, s.ctypes.data, C.byref(h)) == -2
        assert f["align_create"](c._h, 3, None, C.byref(h)) == -2
        assert f["align_create"](c._h, 3, s.ctypes.data, None) == -2
        assert f["align_create"](c._h, 2 ** 31, s.ctypes.data, C.byref(h)) == -3 and not h.value
        with cloud.Aligner(c, s) as al:
            assert f["align_sums"](None, 0.2, mp, sp, fp) == -2
            assert f["align_sums"](al._h, 0.2, None, sp, fp) == -2
            assert f["align_sums"](al._h, 0.2, mp, None, fp) == -2
            assert f["align_sums"](al._h, 0.2, mp, sp, None) == -2
            for r in (0.0, -1.0, np.inf, np.nan):
                assert f["align_sums"](al._h, r, mp, sp, fp) == -2
                assert f["align_icp"](al._h, r, 1, 5, 0.0, mp, None, None, None) == -2
            assert f["align_sums"](al._h, 1e-8, mp, sp, fp) == -3   # the unit cube spans more than 2^21 cells
            bad = m.copy()
            bad[7] = np.nan
            assert f["align_sums"](al._h, 0.2, bad.ctypes.data_as(PD), sp, fp) == -2
            assert f["align_icp"](al._h, 0.2, 1, 5, 0.0, bad.ctypes.data_as(PD), None, None, None) == -2
            assert f["align_icp"](al._h, 0.2, 1, 0, 0.0, mp, None, None, None) == -2
            assert f["align_icp"](al._h, 0.2, 1, 5, -1.0, mp, None, None, None) == -2
            assert f["align_icp"](al._h, 0.2, 1, 5, np.nan, mp, None, None, None) == -2
            assert f["align_icp"](None, 0.2, 1, 5, 0.0, mp, None, None, None) == -2
            assert f["align_icp"](al._h, 0.2, 1, 5, 0.0, None, None, None, None) == -2
            with pytest.raises(ValueError):
                al.sums(-1.0, I4)
            assert np.array_equal(al.sums(0.2, I4)[0], ac.brute_sums(t, s, I4, 0.2)[0])   # the handle stays usable
    assert f["align_solve"](None, fp, 1, mp, mp, None) == -2
    assert f["align_ms"](None) == 0.0
    f["align_destroy"](None)


def write_ply(path, xyz):
    with open(path, "wb") as fh:
        fh.write(f"ply\nformat binary_little_endian 1.0\nelement vertex {len(xyz)}\nproperty float x\nproperty float y\nproperty float z\nend_header\n".encode())
        fh.write(np.ascontiguousarray(xyz, "<f4").tobytes())


def run_tool(capsys, monkeypatch, argv):
    spec = importlib.util.spec_from_file_location("eval_ply_tool", os.path.join(ROOT, "tools", "eval_ply.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(sys, "argv", ["eval_ply.py"] + [str(a) for a in argv])
    capsys.readouterr()
    mod.main()
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def test_eval_ply_round_trip(cloud, tmp_path, capsys, monkeypatch):
    """a scan with repeated points and a transformed copy thinned to its distinct points: F1 = 1.0 at a tolerance of 1e-4
    only with refinement (the given transform is off by ~1e-2)"""
    rng = np.random.default_rng(8)
    base = rng.random((1200, 3), dtype=np.float32)
    scan = np.concatenate([base, base[rng.choice(1200, 800, replace=False)]])[rng.permutation(2000)]
    T_true = ac.similarity(rng, 0.5, 1.25, 0.7)
    rec = ((base.astype(np.float64) - T_true[:3, 3]) @ np.linalg.inv(T_true[:3, :3]).T).astype(np.float32)
    P = ac.similarity(rng, np.deg2rad(0.4), 1.004, 0.01)
    P[:3, 3] += 0.5 - P[:3, :3] @ np.full(3, 0.5)
    T0 = P @ T_true
    with cloud.Cloud(scan) as c:
        T, report = cloud.align(rec, c, T0, radii=(0.02, 0.05), with_scale=True)
    assert [r["radius"] for r in report] == [0.05, 0.02] and all(r["inliers"] == 1200 and r["passes"] < 30 for r in report)
    assert np.abs(T - T_true).max() < 1e-6 and np.array_equal(T[3], [0, 0, 0, 1])
    write_ply(tmp_path / "scan.ply", scan)
    write_ply(tmp_path / "rec.ply", rec)
    np.savetxt(tmp_path / "T0.txt", T0)
    base_args = ["--reconstruction", tmp_path / "rec.ply", "--ground_truth", tmp_path / "scan.ply", "--tolerances", "0.0001,0.00625", "--transform", tmp_path / "T0.txt"]
    plain = run_tool(capsys, monkeypatch, base_args)
    fine = run_tool(capsys, monkeypatch, base_args + ["--refine", "--save_transform", tmp_path / "T.txt"])
    assert "refine" not in plain and plain["tolerances"][0]["f1"] < 0.05
    assert fine["tolerances"][0]["f1"] == 1.0 and fine["tolerances"][0]["n_accurate"] == 1200 and fine["tolerances"][0]["n_complete"] == 2000
    assert [r["radius"] for r in fine["refine"]["rounds"]] == [0.05, 0.025, 0.0125]
    assert np.abs(np.loadtxt(tmp_path / "T.txt") - T_true).max() < 1e-6
    assert np.abs(np.array(fine["refine"]["matrix"]) - T_true).max() < 1e-6
    # --save_transform feeds --transform: the saved matrix alone gives the refined score
    again = run_tool(capsys, monkeypatch, base_args[:6] + ["--transform", tmp_path / "T.txt"])
    assert again["tolerances"] == fine["tolerances"]
