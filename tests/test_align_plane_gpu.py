"""mpmvs_align_plane_* on the GPU against the numpy statement (tests/align_plane_common.py): array_equal on all 38 sums and on
the frame; mpmvs_align_plane_icp against the loop over the two public calls and against the loop over the statement, bit for
bit; both kinds of pass mixed on one handle; tools/eval_ply.py --refine --refine_method plane end to end."""
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
import align_plane_common as pc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I4 = np.eye(4)


@pytest.fixture(scope="module")
def cloud(engine):
    return importlib.import_module("mp-mvs_amd.cloud")


def check(cloud, t, nrm, s, M, radius):
    with cloud.Cloud(t) as c, cloud.Aligner(c, s) as al:
        al.set_normals(nrm)
        sums, frame = al.plane_sums(radius, M)
    want, wframe = pc.plane_sums(t, nrm, s, M, radius)
    assert sums.shape == (38,) and frame.shape == (4,)
    assert np.array_equal(frame, wframe), (frame, wframe)
    assert np.array_equal(sums, want), (sums - want)
    return sums, frame


def moved():
    return ac.similarity(np.random.default_rng(2), 0.05, 1.03, 0.02)


def random_normals(rng, n):
    """random directions of lengths 2^-20 .. 2^20, with every kind of unusable normal and the smallest usable ones among them"""
    nrm = (rng.normal(size=(n, 3)) * np.exp2(rng.uniform(-20, 20, (n, 1)))).astype(np.float32)
    nrm[5] = 0.0
    nrm[6] = [-0.0, 0.0, -0.0]
    nrm[7, 0] = np.nan
    nrm[8, 1] = np.inf
    nrm[9] = [-np.inf, np.nan, 1.0]
    nrm[10] = np.array([3, -4, 12], np.float32) * np.float32(1e-42)   # subnormal length: usable, its square is no fp32 number
    nrm[11] = [0.0, 1e-45, 0.0]                                       # the smallest fp32 there is
    nrm[12] = np.float32(3e38)                                        # finite, its square is far above fp32
    return nrm


@pytest.fixture(scope="module")
def random_clouds():
    rng = np.random.default_rng(11)
    t, s = rng.random((1500, 3), dtype=np.float32), rng.random((1000, 3), dtype=np.float32)   # the clouds of test_align_gpu.py
    return t, s, random_normals(np.random.default_rng(12), len(t))


@pytest.mark.parametrize("transform", ["identity", "similarity"])
@pytest.mark.parametrize("radius", [0.02, 0.2, 4.0])
def test_random(cloud, random_clouds, radius, transform):
    t, s, nrm = random_clouds
    sums, frame = check(cloud, t, nrm, s, I4 if transform == "identity" else moved(), radius)
    n_point = int(ac.brute_sums(t, s, I4 if transform == "identity" else moved(), radius)[0][0])
    assert 0 < sums[0] <= n_point   # the pairs of the point-to-point pass, less those whose target has no usable normal
    if radius == 0.02:
        assert sums[0] < len(s)
    if radius == 4.0:
        assert frame[3] == 16.0 and n_point == len(s)


def test_unusable_normals_drop_their_pairs(cloud, random_clouds):
    t, s, nrm = random_clouds
    near = np.concatenate([t[5:13] + np.float32(1e-3), t[100:108] + np.float32(1e-3)])   # one source next to each special target
    sums, _ = check(cloud, t, nrm, near, I4, 0.01)
    assert sums[0] == 16 - 5   # targets 5..9 are unusable, 10..12 are not
    sums, _ = check(cloud, t, nrm, near[:5], I4, 0.01)
    assert not sums.any()
    for bad in (np.zeros_like(nrm), np.full_like(nrm, np.nan), np.full_like(nrm, np.inf)):
        assert not check(cloud, t, bad, s, I4, 0.2)[0].any()


@pytest.mark.parametrize("n_s", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_wave_and_block_borders(cloud, random_clouds, n_s):
    t, s, nrm = random_clouds
    usable = np.abs(np.nan_to_num(nrm, nan=1.0, posinf=1.0, neginf=1.0)) + np.float32(1e-3)   # every target counts
    sums, _ = check(cloud, t, usable, s[:n_s], I4, 0.2)
    assert sums[0] == n_s


@pytest.mark.parametrize("kind", ["negative", "mixed"])
@pytest.mark.parametrize("n_s", [64, 600])
def test_carry_and_sign(cloud, kind, n_s):
    """targets at the corners +-(1 - 2^-5) with diagonal normals, radius 2^-6: u = 1, |a_k| ~ 0.97 and nh_k = +-1 / sqrt 3, so
    g ~ +-1.68 and g * g ~ 2.8 * 2^30 per pair, the largest term there is; 64 pairs pass 2^32 within one wave, 600 pass 2^38
    across blocks.  With all sources at the corner - - - the sums of nh_i * g are negative."""
    rng = np.random.default_rng(n_s)
    corners = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float32) * np.float32(0.96875)
    nrm = -np.sign(corners) * np.float32(2.0)   # inward: at the corner - - - the normal is + + +, g < 0
    pick = np.zeros(n_s, int) if kind == "negative" else rng.integers(0, 8, n_s)
    s = (corners[pick] * (1 - rng.random((n_s, 1)) * 2.0 ** -12)).astype(np.float32)
    sums, frame = check(cloud, corners, nrm, s, I4, 2.0 ** -6)
    assert frame[3] == 1.0 and sums[0] == n_s
    big = 2 ** 32 if n_s == 64 else 2 ** 38
    assert sums[28] > 2.7 * n_s * 2 ** 30 and sums[28] > big   # g * g
    assert (sums[[19, 23, 26]] > 0.33 * n_s * 2 ** 30).all()   # nh_k^2 = 1 / 3
    assert sums[36] > 0 and (sums[29:36] != 0).any()           # the sources sit a little inside their corners: r > 0
    n_g, n_n = sums[[22, 25, 27]], sums[[20, 21, 24]]          # nh_k g = sign(corner_k) 0.97;  nh_i nh_j = sign_i sign_j / 3, i != j
    if kind == "negative":
        assert (n_g < -0.96 * n_s * 2 ** 30).all() and (n_g < -big).all()
        assert (n_n > 0.33 * n_s * 2 ** 30).all()
    else:
        assert np.abs(n_g).max() < 0.5 * n_s * 2 ** 30 and np.abs(n_n).max() < 0.2 * n_s * 2 ** 30   # both signs meet


def test_ties_between_targets_with_different_normals(cloud):
    """equidistant from two targets: the smaller index wins, and with it its normal, so swapping the two changes the sums"""
    t = np.array([[0, 0, 0], [1, 0, 0], [0.5, 1, 0]], np.float32)
    nrm = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    s = np.array([[0.5, 0.125, 0]], np.float32)
    a, _ = check(cloud, t, nrm, s, I4, 0.75)
    b, _ = check(cloud, t[[1, 0, 2]], nrm, s, I4, 0.75)      # the points swapped, the normals not: target 0 is (1 0 0) with nh = x
    c, _ = check(cloud, t[[1, 0, 2]], nrm[[1, 0, 2]], s, I4, 0.75)   # both swapped: target 0 is (1 0 0) with nh = y
    assert a[0] == b[0] == c[0] == 1
    assert a[19] == b[19] == 2 ** 30 and c[19] == 0 and c[23] == 2 ** 30   # nh_0^2, nh_1^2
    assert a[32] > 0 > b[32] and not np.array_equal(a, c)    # nh_0 r: the source is right of target (0 0 0), left of (1 0 0)
    rng = np.random.default_rng(5)
    base = rng.random((300, 3), dtype=np.float32)
    t2 = np.concatenate([base, base[rng.choice(300, 100, replace=False)]])[rng.permutation(400)]   # duplicates with their own normals
    check(cloud, t2, rng.normal(size=(400, 3)).astype(np.float32), np.concatenate([t2, base + np.float32(0.001)]), I4, 0.6)


def test_nonfinite_and_empty(cloud):
    rng = np.random.default_rng(9)
    t = rng.random((700, 3), dtype=np.float32)
    s = rng.random((500, 3), dtype=np.float32)
    nrm = rng.normal(size=(700, 3)).astype(np.float32)
    t[[3, 77], [0, 2]] = [np.nan, np.inf]
    s[[0, 64, 499], [1, 0, 2]] = [np.nan, -np.inf, np.inf]
    s[5] = 1e30
    sums, _ = check(cloud, t, nrm, s, I4, 0.2)
    assert 0 < sums[0] <= 496
    big = I4.copy()
    big[0, 0] = 1e300   # finite, but every image overflows fp32
    assert not check(cloud, t, nrm, s, big, 0.2)[0].any()
    assert not check(cloud, t, nrm, s + np.float32(10), I4, 0.2)[0].any()   # nothing within the radius
    sums, frame = check(cloud, t, nrm, np.zeros((0, 3), np.float32), I4, 0.2)
    assert not sums.any() and frame[3] == 1.0
    sums, frame = check(cloud, np.full((4, 3), np.nan, np.float32), nrm[:4], s, I4, 0.2)
    assert not sums.any() and not frame.any()
    sums, frame = check(cloud, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), s, I4, 0.2)
    assert not sums.any() and not frame.any()


@pytest.mark.parametrize("with_scale", [False, True])
def test_icp_is_the_loop_of_the_public_calls(cloud, with_scale):
    target, normals, src, T_true, T0 = pc.plane_scene(with_scale)
    eps = 2.0 ** -20
    with cloud.Cloud(target) as c, cloud.Aligner(c, src) as al:
        al.set_normals(normals)
        got = al.plane_icp(pc.RADIUS, T0, with_scale, 30, eps)
        loop = cloud.plane_icp_loop(al.plane_sums, pc.RADIUS, T0, with_scale, 30, eps)
        one = al.plane_icp(pc.RADIUS, T0, with_scale, 1, eps)
        al.set_normals(-normals)
        flipped = al.plane_icp(pc.RADIUS, T0, with_scale, 30, eps)
    stated = cloud.plane_icp_loop(lambda r, M: pc.plane_sums(target, normals, src, M, r), pc.RADIUS, T0, with_scale, 30, eps)
    for other in (loop, stated, flipped):
        assert np.array_equal(got[0], other[0]) and got[1:] == other[1:], (got, other)
    assert 1 < got[1] < 30 and got[2] > 1100 and got[3] <= got[4]
    assert one[1] == 1 and not np.array_equal(one[0], ac.m34(T0))
    assert np.abs(got[0] - T_true[:3]).max() < 1e-6


def test_point_and_plane_passes_share_a_handle(cloud, random_clouds):
    t, s, nrm = random_clouds
    want_point, want_plane = ac.brute_sums(t, s, moved(), 0.2)[0], pc.plane_sums(t, nrm, s, moved(), 0.2)[0]
    with cloud.Cloud(t) as c:
        c.nearest(s[:10], 0.2)
        assert c.kernel_ms()[1] > 0
        with cloud.Aligner(c, s) as al:
            al.set_normals(nrm)
            p0, _ = al.sums(0.2, moved())
            assert c.kernel_ms()[1] == 0 and al.ms() > 0   # the grid of the nearest() call served the point pass
            q0, _ = al.plane_sums(0.2, moved())
            assert c.kernel_ms()[1] == 0 and al.ms() > 0   # ... and the plane pass
            p1, _ = al.sums(0.2, moved())
            q1, _ = al.plane_sums(0.2, moved())
            assert np.array_equal(p0, want_point) and np.array_equal(p1, want_point)
            assert np.array_equal(q0, want_plane) and np.array_equal(q1, want_plane)
            al.set_normals(None)
            with pytest.raises(ValueError):
                al.plane_sums(0.2, moved())
            with pytest.raises(ValueError):
                al.plane_icp(0.2, moved())
            assert np.array_equal(al.sums(0.2, moved())[0], want_point)   # the handle stays usable
            al.set_normals(nrm)
            assert np.array_equal(al.plane_sums(0.2, moved())[0], want_plane)
        c.nearest(s[:10], 0.2)
        assert c.kernel_ms()[1] == 0


def test_two_aligners_with_different_normals(cloud, random_clouds):
    t, s, nrm = random_clouds
    other = np.roll(nrm, 1, axis=1).copy()
    with cloud.Cloud(t) as c, cloud.Aligner(c, s) as a1, cloud.Aligner(c, s[:300]) as a2:
        a1.set_normals(nrm)
        a2.set_normals(other)
        s1, _ = a1.plane_sums(0.2, I4)
        s2, _ = a2.plane_sums(0.2, moved())
        s1b, _ = a1.plane_sums(0.2, I4)
    assert np.array_equal(s1, pc.plane_sums(t, nrm, s, I4, 0.2)[0]) and np.array_equal(s1, s1b)
    assert np.array_equal(s2, pc.plane_sums(t, other, s[:300], moved(), 0.2)[0])
    assert not np.array_equal(s2, pc.plane_sums(t, nrm, s[:300], moved(), 0.2)[0])


UNBINNED = """
import importlib, sys
import numpy as np
sys.path[:0] = [{root!r}, {tests!r}]
import align_common as ac
import align_plane_common as pc
cloud = importlib.import_module("mp-mvs_amd.cloud")
rng = np.random.default_rng(11)
t, s = rng.random((1500, 3), dtype=np.float32), rng.random((1000, 3), dtype=np.float32)
nrm = rng.normal(size=(1500, 3)).astype(np.float32)
nrm[::7] = 0
M = ac.similarity(np.random.default_rng(2), 0.05, 1.03, 0.02)
with cloud.Cloud(t) as c, cloud.Aligner(c, s) as al:
    al.set_normals(nrm)
    for r in (0.02, 0.2):
        got, want = al.plane_sums(r, M), pc.plane_sums(t, nrm, s, M, r)
        assert want[0][0] > 0 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), r
print("unbinned equal")
"""


def test_caller_order_pass(cloud):
    """MPMVS_CLOUD_BIN=0 is read once per process, so the unbinned pass runs in a child"""
    env = dict(os.environ, MPMVS_CLOUD_BIN="0")
    out = subprocess.run([sys.executable, "-c", UNBINNED.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "unbinned equal" in out.stdout, out.stderr[-2000:]


def test_error_codes(cloud, engine, random_clouds):
    t, s, nrm = random_clouds
    _, f = engine.load()
    PD, PL = C.POINTER(C.c_double), C.POINTER(C.c_longlong)
    m = np.ascontiguousarray(I4[:3]).reshape(12)
    sums, frame = np.zeros(38, np.int64), np.zeros(4)
    mp, sp, fp = m.ctypes.data_as(PD), sums.ctypes.data_as(PL), frame.ctypes.data_as(PD)
    with cloud.Cloud(t) as c, cloud.Aligner(c, s) as al:
        # no normals yet: -2 from the pass and from the loop, whatever else is right
        assert f["align_plane_sums"](al._h, 0.2, mp, sp, fp) == -2
        assert f["align_plane_icp"](al._h, 0.2, 1, 5, 0.0, mp, None, None, None, None) == -2
        assert f["align_set_normals"](None, nrm.ctypes.data) == -2
        assert f["align_set_normals"](al._h, nrm.ctypes.data) == 0
        assert f["align_plane_sums"](None, 0.2, mp, sp, fp) == -2
        assert f["align_plane_sums"](al._h, 0.2, None, sp, fp) == -2
        assert f["align_plane_sums"](al._h, 0.2, mp, None, fp) == -2
        assert f["align_plane_sums"](al._h, 0.2, mp, sp, None) == -2
        for r in (0.0, -1.0, np.inf, np.nan):
            assert f["align_plane_sums"](al._h, r, mp, sp, fp) == -2
            assert f["align_plane_icp"](al._h, r, 1, 5, 0.0, mp, None, None, None, None) == -2
        assert f["align_plane_sums"](al._h, 1e-8, mp, sp, fp) == -3   # the unit cube spans more than 2^21 cells
        assert f["align_plane_icp"](al._h, 1e-8, 1, 5, 0.0, mp, None, None, None, None) == -3
        bad = m.copy()
        bad[7] = np.nan
        assert f["align_plane_sums"](al._h, 0.2, bad.ctypes.data_as(PD), sp, fp) == -2
        assert f["align_plane_icp"](al._h, 0.2, 1, 5, 0.0, bad.ctypes.data_as(PD), None, None, None, None) == -2
        assert f["align_plane_icp"](al._h, 0.2, 1, 0, 0.0, mp, None, None, None, None) == -2
        assert f["align_plane_icp"](al._h, 0.2, 1, 5, -1.0, mp, None, None, None, None) == -2
        assert f["align_plane_icp"](al._h, 0.2, 1, 5, np.nan, mp, None, None, None, None) == -2
        assert f["align_plane_icp"](None, 0.2, 1, 5, 0.0, mp, None, None, None, None) == -2
        assert f["align_plane_icp"](al._h, 0.2, 1, 5, 0.0, None, None, None, None, None) == -2
        assert f["align_plane_icp"](al._h, 0.2, 1, 5, 0.0, mp, None, None, None, None) == 0   # every output may be NULL
        with pytest.raises(ValueError):
            al.plane_sums(-1.0, I4)
        with pytest.raises(ValueError):
            al.set_normals(nrm[:-1])
        assert np.array_equal(al.plane_sums(0.2, I4)[0], pc.plane_sums(t, nrm, s, I4, 0.2)[0])   # the handle stays usable
        with pytest.raises(ValueError):
            cloud.align(s, c, radii=(0.2,), method="plane")   # neither normals nor a radius to estimate them with
        with pytest.raises(ValueError):
            cloud.align(s, c, radii=(0.2,), method="planes")
    assert f["align_plane_solve"](None, fp, 1, mp, mp, None, None) == -2


def write_ply(path, xyz, normals=None):
    cols = "xyz" if normals is None else ("x", "y", "z", "nx", "ny", "nz")
    data = xyz if normals is None else np.concatenate([xyz, normals], 1)
    with open(path, "wb") as fh:
        fh.write((f"ply\nformat binary_little_endian 1.0\nelement vertex {len(xyz)}\n" + "".join(f"property float {c}\n" for c in cols) + "end_header\n").encode())
        fh.write(np.ascontiguousarray(data, "<f4").tobytes())


def run_tool(capsys, monkeypatch, argv):
    spec = importlib.util.spec_from_file_location("eval_ply_tool", os.path.join(ROOT, "tools", "eval_ply.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(sys, "argv", ["eval_ply.py"] + [str(a) for a in argv])
    capsys.readouterr()
    mod.main()
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def test_align_and_eval_ply_end_to_end(cloud, tmp_path, capsys, monkeypatch):
    """plane_scene() as PLY files: --refine_method plane reaches the known transform to 1e-6 with the scan's own normals and
    with normals estimated at --refine_normal_radius 0.1 (an inset face point has neighbours on its own face only);
    --refine_method point on the same files does not come within 1e-3"""
    target, normals, src, T_true, T0 = pc.plane_scene(True)
    with cloud.Cloud(target) as c:
        T, report = cloud.align(src, c, T0, radii=(pc.RADIUS,), method="plane", target_normals=normals)
        Te, report_e = cloud.align(src, c, T0, radii=(pc.RADIUS,), method="plane", normal_radius=0.1)
        Tp, report_p = cloud.align(src, c, T0, radii=(pc.RADIUS,))
    assert set(report[0]) == {"radius", "passes", "inliers", "rmse", "rmse_plane"} and set(report_p[0]) == {"radius", "passes", "inliers", "rmse"}
    assert report[0]["passes"] < 30 and report[0]["rmse_plane"] < report[0]["rmse"]
    assert np.abs(T - T_true).max() < 1e-6 and np.abs(Te - T_true).max() < 1e-6 and np.array_equal(T[3], [0, 0, 0, 1])
    assert np.abs(Tp - T_true).max() > 1e-3
    write_ply(tmp_path / "scan_n.ply", target, normals)
    write_ply(tmp_path / "scan.ply", target)
    write_ply(tmp_path / "rec.ply", src)
    np.savetxt(tmp_path / "T0.txt", T0)
    args = ["--reconstruction", tmp_path / "rec.ply", "--tolerances", "0.025", "--transform", tmp_path / "T0.txt", "--refine", "--refine_radii", pc.RADIUS]
    own = run_tool(capsys, monkeypatch, args + ["--ground_truth", tmp_path / "scan_n.ply", "--refine_method", "plane"])
    est = run_tool(capsys, monkeypatch, args + ["--ground_truth", tmp_path / "scan.ply", "--refine_method", "plane", "--refine_normal_radius", 0.1])
    point = run_tool(capsys, monkeypatch, args + ["--ground_truth", tmp_path / "scan_n.ply", "--refine_method", "point"])
    default = run_tool(capsys, monkeypatch, args + ["--ground_truth", tmp_path / "scan_n.ply"])
    for res in (own, est):
        assert res["refine"]["method"] == "plane" and "rmse_plane" in res["refine"]["rounds"][0]
        assert np.abs(np.array(res["refine"]["matrix"]) - T_true).max() < 1e-6
    assert own["refine"]["normals"] == "ground truth file" and est["refine"]["normals"] == "estimated"
    assert np.array_equal(np.array(own["refine"]["matrix"]), T)
    assert point["refine"]["method"] == "point" and np.abs(np.array(point["refine"]["matrix"]) - T_true).max() > 1e-3
    assert default["refine"] == {**point["refine"], "seconds": default["refine"]["seconds"]}   # the default stays point-to-point
