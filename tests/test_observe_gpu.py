"""mpmvs_observer_* on the GPU against the plain statement (tests/observe_common.py): array_equal on the map bits and on both
counts, no tolerance anywhere; the room scene end to end through Observer, evaluate(scanners=...) and tools/eval_ply.py."""
import importlib
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

import observe_common as oc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
MARGINS = ((0.0, 0.0), (0.02, 0.0), (0.05, 0.01))
CHUNK = 8   # kObserveChunk of csrc/pm_observe.hpp: scanners per launch of the scan passes


@pytest.fixture(scope="module")
def cloud(engine):
    return importlib.import_module("mp-mvs_amd.cloud")


@pytest.fixture(scope="module")
def data():
    """64 scanners (number 2 so far out that differences overflow), a scan of 200 000 points and 100 000 queries, both with
    1 % junk and with points on the scanners"""
    rng = np.random.default_rng(21)
    scanners = rng.uniform(-1.0, 1.0, (64, 3)).astype(f32)
    scanners[2] = (-3e38, 0.25, 0.0)
    return scanners, oc.junk_cloud(rng, 200_000, scanners), oc.junk_cloud(rng, 100_000, scanners)


@pytest.fixture(scope="module")
def scan_cloud(cloud, data):
    with cloud.Cloud(data[1]) as c:
        yield c


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check(cloud, c, scan, scanners, R, w, q, owner=None, margins=MARGINS):
    """an Observer on the Cloud c of `scan` against the statement: every map, the pixel count and both counts per margin"""
    Zc, Zn = oc.maps(scan, scanners, R, w, owner)
    with cloud.Observer(c, scanners, owner, R, w) as obs:
        for j in range(len(scanners)):
            assert same_bits(obs.near_map(j), Zn[j]), (R, w, j)
        assert obs.stats() == {"covered_pixels": int(np.isfinite(Zn).sum()), "pixels": Zn.size}
        placed = [oc.locate(q, S, R) for S in scanners]
        for rel, ab in margins:
            free, cov = obs.classify(q, rel, ab)
            wf, wc = oc.classify(q, scanners, Zn, rel, ab, placed)
            assert free.dtype == np.int32 and cov.dtype == np.int32 and np.array_equal(free, wf) and np.array_equal(cov, wc), (R, w, rel, ab)
            free2, none = obs.classify(q, rel, ab, want_covered=False)   # out_covered == NULL
            assert none is None and np.array_equal(free2, wf)
    return Zc, Zn


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,w,n_sc", [(1, 0, 1), (1, 8, 2), (2, 1, 3), (3, 8, 3), (3, 2, CHUNK + 1), (8, 1, 64), (8, 0, 2), (64, 2, 3), (64, 8, 1), (64, 1, 2),
                                      (64, 0, CHUNK + 1)])
def test_random_scans(cloud, data, scan_cloud, R, w, n_sc):
    scanners, scan, q = data
    Zc, Zn = check(cloud, scan_cloud, scan, scanners[:n_sc], R, w, q)
    if w == 0:
        assert same_bits(Zc, Zn)
    if n_sc >= 3:
        assert (Zn[2] > 1e38).any() and np.isfinite(Zn[2]).any()   # the far scanner: differences near the largest float, and past it


# 2 ---------------------------------------------------------------------------------------------------------------------------
def lattice(S):
    pts = [S + f32(s) * np.array([a, b, c], f32) for s in (0.5, 1.0, 3.0, 1e-3) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)]
    for m in range(3):
        for sm in (-1.0, 1.0):
            for sb in (-1.0, 1.0):
                for e in (np.nextafter(f32(1), f32(0)), np.nextafter(f32(1), f32(2))):
                    d = np.full(3, 0.125, f32)
                    d[m], d[(m + 1) % 3] = sm, sb * e
                    pts.append(S + d)
                    d[(m + 1) % 3], d[(m + 2) % 3] = 0.125, sb * e
                    pts.append(S + d)
    return np.array(pts, f32)


def test_direction_lattice(cloud):
    """ties between the axes, the clamp at x == R and all six faces, as scan points and as queries"""
    S = np.array([[0.25, -0.5, 1.0]], f32)
    pts = lattice(S[0])
    q = np.concatenate([pts, (S[0] + (pts - S[0]) * f32(0.5)).astype(f32), (S[0] + (pts - S[0]) * f32(2.0)).astype(f32)])
    part, f, px, py, z = oc.locate(pts, S[0], 8)
    assert set(f[part].tolist()) == set(range(6)) and (px[part] == 7).any() and (px[part] == 0).any() and (~part).sum() == 4   # d = 0 four times
    with cloud.Cloud(pts) as c:
        for R in (1, 2, 3, 8, 64):
            for w in (0, 1):
                check(cloud, c, pts, S, R, w, q, margins=((0.0, 0.0), (0.02, 0.0)))


# 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rel,ab", MARGINS)
def test_threshold_to_the_last_bit(cloud, rel, ab):
    """per scan range Z: the largest z the statement still calls free, and the next float above it"""
    S = np.zeros((1, 3), f32)
    for Z in (f32(2.5), f32(1e-3), f32(1000.0), f32(0.7)):
        scan = np.array([[0, Z, 0]], f32)
        Zn = oc.maps(scan, S, 1, 0)[1]

        def is_free(z):
            return bool(oc.classify(np.array([[0, z, 0]], f32), S, Zn, rel, ab)[0][0])

        lo, hi = 0, int(Z.view(np.uint32))   # bits order as the positive values; free is monotone in z
        assert not is_free(Z)
        if not is_free(np.nextafter(f32(0), f32(1))):   # abs_margin alone reaches the range: nothing is free
            q = np.array([[0, np.nextafter(f32(0), f32(1)), 0], [0, Z / 2, 0]], f32)
        else:
            while hi - lo > 1:
                mid = (lo + hi) // 2
                if is_free(np.uint32(mid).view(f32)):
                    lo = mid
                else:
                    hi = mid
            z_last = np.uint32(lo).view(f32)
            assert is_free(z_last) and not is_free(np.nextafter(z_last, f32(np.inf))) and z_last < Z
            q = np.array([[0, z_last, 0], [0, np.nextafter(z_last, f32(np.inf)), 0], [0, np.nextafter(z_last, f32(0)), 0]], f32)
        with cloud.Cloud(scan) as c:
            check(cloud, c, scan, S, 1, 0, q, margins=((rel, ab),))
            with cloud.Observer(c, S, None, 1, 0) as obs:
                assert obs.classify(q, rel, ab)[0].tolist() == ([1, 0, 1] if len(q) == 3 else [0, 0])


# 4 ---------------------------------------------------------------------------------------------------------------------------
def test_owner(cloud, data, scan_cloud):
    scanners, scan, q = data
    rng = np.random.default_rng(5)
    q = q[:20_000]
    # no owner, and every point owned by the one scanner: the same bits
    a = check(cloud, scan_cloud, scan, scanners[:1], 8, 1, q)
    b = check(cloud, scan_cloud, scan, scanners[:1], 8, 1, q, owner=np.zeros(len(scan), np.int32))
    assert same_bits(a[1], b[1])
    split = rng.integers(0, 3, len(scan)).astype(np.int32)
    check(cloud, scan_cloud, scan, scanners[:3], 8, 1, q, owner=split)
    split[rng.choice(len(scan), len(scan) // 3, replace=False)] = -1
    check(cloud, scan_cloud, scan, scanners[:3], 64, 2, q, owner=split)
    over = rng.integers(-1, CHUNK + 3, len(scan)).astype(np.int32)   # owners on both sides of a chunk border
    check(cloud, scan_cloud, scan, scanners[:CHUNK + 3], 3, 1, q, owner=over)
    none = np.full(len(scan), -1, np.int32)
    Zn = check(cloud, scan_cloud, scan, scanners[:2], 4, 1, q, owner=none)[1]
    assert np.isinf(Zn).all()
    for bad in (3, -2, 64):   # a value of n_scanners, or below -1, is refused before the device is touched
        split[-1] = bad
        with pytest.raises(ValueError, match="owner"):
            cloud.Observer(scan_cloud, scanners[:3], split, 8, 1)
    with pytest.raises(ValueError, match="owner"):
        cloud.Observer(scan_cloud, scanners[:3], split[:-1], 8, 1)


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_order_independence(cloud, data):
    scanners, scan, q = data
    scan = scan[:50_000]
    rng = np.random.default_rng(6)
    want = oc.maps(scan, scanners[:3], 16, 1)[1]
    for pts in (scan, scan[rng.permutation(len(scan))], np.concatenate([scan, scan[::-1], scan])):
        with cloud.Cloud(pts) as c, cloud.Observer(c, scanners[:3], None, 16, 1) as obs:
            for j in range(3):
                assert same_bits(obs.near_map(j), want[j])


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_contention(cloud):
    """70 001 scan points on one ray: one pixel takes every atomic"""
    t = (f32(1.0) + (np.arange(70001) * 7919 % 70001).astype(f32) * f32(1e-4)).astype(f32)
    scan = (t[:, None] * np.array([0.3, 1.0, -0.2], f32)).astype(f32)
    S = np.zeros((1, 3), f32)
    q = (np.linspace(0.9, 1.3, 257, dtype=f32)[:, None] * np.array([0.3, 1.0, -0.2], f32)).astype(f32)
    with cloud.Cloud(scan) as c:
        Zc, Zn = check(cloud, c, scan, S, 2, 0, q)
    assert np.isfinite(Zc).sum() == 1 and Zc.min() == scan[:, 1].min() == f32(1.0)


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_degenerate_inputs_and_error_codes(cloud, data, scan_cloud):
    scanners, scan, q = data
    q = q[:5000]
    for pts in (np.zeros((0, 3), f32), np.full((7, 3), np.nan, f32), np.array([[np.inf, 0, 0], [0, -np.inf, 1], [1, 2, np.nan]], f32)):
        with cloud.Cloud(pts) as c:
            Zn = check(cloud, c, pts, scanners[:3], 4, 1, q)[1]
            assert np.isinf(Zn).all()
    with cloud.Observer(scan_cloud, scanners[:2], None, 4, 1) as obs:
        free, cov = obs.classify(np.zeros((0, 3), f32))   # n_q == 0
        assert free.shape == (0,) and cov.shape == (0,) and obs.ms()[0] == 0.0
        obs.classify(q)
        ms, build = obs.ms()
        assert ms > 0 and build["zmin"] > 0 and build["near"] > 0
        for kw in ({"rel": -0.1}, {"rel": 1.0}, {"rel": np.nan}, {"abs_margin": -1.0}, {"abs_margin": np.inf}):
            with pytest.raises(ValueError):
                obs.classify(q, **kw)
        for j in (-1, 2):
            with pytest.raises(ValueError, match="scanner"):
                obs.near_map(j)
        with pytest.raises(ValueError):
            obs.classify(np.zeros((3, 2), f32))
    for kw in ({"face_size": 0}, {"face_size": 4097}, {"window": -1}, {"window": 9}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            cloud.Observer(scan_cloud, scanners[:2], None, **{"face_size": 4, "window": 1, **kw})
    bad = scanners[:2].copy()
    bad[1, 2] = np.inf
    for s in (bad, np.zeros((0, 3), f32), np.zeros((65, 3), f32)):
        with pytest.raises(ValueError):
            cloud.Observer(scan_cloud, s, None, 4, 1)
    with pytest.raises(ValueError, match="2\\^31"):   # -3
        cloud.Observer(scan_cloud, scanners, None, 4096, 1)
    closed = cloud.Cloud(scan[:10])
    closed.close()
    with pytest.raises(ValueError, match="no scan"):
        cloud.Observer(closed, scanners[:2], None, 4, 1)


# 8 ---------------------------------------------------------------------------------------------------------------------------
def test_lifetime_and_grid_cache(cloud, data):
    """the observer does not touch the cloud's grids, and outlives the cloud"""
    scanners, scan, q = data
    q = q[:20_000]
    with np.errstate(invalid="ignore"):
        scan = scan[np.abs(scan).max(1) <= 2.0]   # a search grid of 0.05 cannot span the far-away values
    c = cloud.Cloud(scan)
    d2a, ia = c.nearest(q, 0.05)
    assert c.kernel_ms()[1] > 0
    stats = c.stats()
    obs = cloud.Observer(c, scanners[:3], None, 32, 1)
    assert c.stats() == stats
    d2b, ib = c.nearest(q, 0.05)
    assert c.kernel_ms()[1] == 0.0 and c.stats() == stats   # the grid of 0.05 is still there
    assert same_bits(d2a, d2b) and np.array_equal(ia, ib)
    free, cov = obs.classify(q)
    maps = [obs.near_map(j) for j in range(3)]
    c.close()
    free2, cov2 = obs.classify(q)
    assert np.array_equal(free, free2) and np.array_equal(cov, cov2) and all(same_bits(obs.near_map(j), maps[j]) for j in range(3))
    Zn = oc.maps(scan, scanners[:3], 32, 1)[1]
    wf, wc = oc.classify(q, scanners[:3], Zn, 0.02, 0.0)
    assert np.array_equal(free, wf) and np.array_equal(cov, wc) and all(same_bits(maps[j], Zn[j]) for j in range(3))
    obs.close()
    obs.close()


# 9 ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def room():
    return oc.room()


@pytest.fixture(scope="module")
def room_cloud(cloud, room):
    with cloud.Cloud(room[0]) as c:
        yield c


@pytest.mark.parametrize("w", [0, 1])
@pytest.mark.parametrize("R", [16, 32, 64])
def test_room(cloud, room, room_cloud, R, w):
    scan, S, floaters, outside, through = room
    with cloud.Observer(room_cloud, S[None], None, R, w) as obs:
        got = {name: obs.classify(q, 0.05, 0.0) for name, q in (("walls", scan), ("floaters", floaters), ("outside", outside), ("through", through))}
    Zn = oc.maps(scan, S[None], R, w)[1]
    for name, q in (("walls", scan), ("floaters", floaters), ("outside", outside), ("through", through)):
        wf, wc = oc.classify(q, S[None], Zn, 0.05, 0.0)
        assert np.array_equal(got[name][0], wf) and np.array_equal(got[name][1], wc), name
    print(f"R {R} w {w}: " + ", ".join(f"{k} free {int(v[0].sum())} covered {int(v[1].sum())} of {len(v[0])}" for k, v in got.items()))
    assert got["walls"][0].sum() == 0 and got["outside"][0].sum() == 0          # nothing on or behind the walls is free
    assert got["through"][1].sum() == 0                                         # the opening returned nothing
    free, cov = got["floaters"]
    assert np.array_equal(free, cov) and cov.sum() >= 490                       # the rest look at the opening


def test_room_evaluate(cloud, room):
    scan, S, floaters, outside, through = room
    rec = np.concatenate([scan, floaters, outside, through])
    t = 0.05
    plain = cloud.evaluate(rec, scan, [t])
    res = cloud.evaluate(rec, scan, [t], scanners=S[None], face_size=64, window=1, free_rel=0.05)
    with cloud.Cloud(scan) as c, cloud.Observer(c, S[None], None, 64, 1) as obs:
        n_free = int(obs.classify(floaters, 0.05, 0.0)[0].sum())
        stats = obs.stats()
    row, old = res["tolerances"][0], plain["tolerances"][0]
    assert {k: row[k] for k in old} == old and {k: res[k] for k in plain if k != "tolerances"} == {k: plain[k] for k in plain if k != "tolerances"}
    assert set(res) == set(plain) | {"observed"} and set(row) == set(old) | {"n_free_inaccurate", "n_unobserved", "accuracy_observed", "f1_observed"}
    assert row["n_accurate"] == len(scan) and n_free >= 490
    assert row["n_free_inaccurate"] == n_free and row["n_unobserved"] == 1200 - n_free
    assert row["accuracy_observed"] == len(scan) / (len(scan) + n_free) and row["accuracy"] == len(scan) / len(rec)
    acc, com = row["accuracy_observed"], row["completeness"]
    assert com == 1.0 and row["f1_observed"] == 2 * acc * com / (acc + com)
    assert res["observed"] == {"scanners": 1, "face_size": 64, "window": 1, "free_rel": 0.05, "free_abs": 0.0, **stats}
    # owner, filtered with the non-finite points, and the resampling after the maps
    gt = np.concatenate([scan[:5], np.full((2, 3), np.nan, f32), scan[5:]])
    owner = np.concatenate([np.zeros(5, np.int32), np.array([7, -9], np.int32), np.zeros(len(scan) - 5, np.int32)])
    own = cloud.evaluate(rec, gt, [t], scanners=S[None], owner=owner, face_size=64, window=1, free_rel=0.05)
    assert own["tolerances"] == res["tolerances"] and own["observed"] == res["observed"] and own["dropped_ground_truth"] == 2
    vox = cloud.evaluate(rec, scan, [t], voxel=0.04, scanners=S[None], face_size=64, window=1, free_rel=0.05)
    assert vox["observed"] == res["observed"] and vox["n_ground_truth"] < len(scan) and vox["tolerances"][0]["n_free_inaccurate"] > 0
    with pytest.raises(ValueError, match="owner"):
        cloud.evaluate(rec, gt, [t], scanners=S[None], owner=owner[:-1])


def run_tool(capsys, monkeypatch, argv):
    spec = importlib.util.spec_from_file_location("eval_ply_tool", os.path.join(ROOT, "tools", "eval_ply.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(sys, "argv", ["eval_ply.py"] + [str(a) for a in argv])
    capsys.readouterr()
    mod.main()
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def test_room_eval_ply(cloud, room, tmp_path, capsys, monkeypatch):
    """--scanners against evaluate(scanners=...), and --scan_alignment: the scan as two files in frames of their own"""
    scan, S, floaters, outside, through = room
    rec = np.concatenate([scan, floaters, outside, through])
    cloud.write_ply(str(tmp_path / "rec.ply"), rec)
    cloud.write_ply(str(tmp_path / "scan.ply"), scan)
    (tmp_path / "scanners.txt").write_text("# the one scanner\n0.2 -0.1 0.3\n")
    args = ["--reconstruction", tmp_path / "rec.ply", "--tolerances", "0.05"]
    opts = ["--face_size", 64, "--free_rel", 0.05]
    plain = run_tool(capsys, monkeypatch, args + ["--ground_truth", tmp_path / "scan.ply"])
    seen = run_tool(capsys, monkeypatch, args + ["--ground_truth", tmp_path / "scan.ply", "--scanners", tmp_path / "scanners.txt"] + opts)
    want = cloud.evaluate(rec, scan, [0.05], scanners=S[None], face_size=64, window=1, free_rel=0.05)
    assert "observed" not in plain and "accuracy_observed" not in plain["tolerances"][0] and set(plain["seconds"]) == {"read", "upload_build", "query"}
    assert seen["tolerances"] == want["tolerances"] and seen["observed"] == want["observed"] and "observe" in seen["seconds"]
    assert {k: seen[k] for k in plain if k not in ("seconds", "tolerances")} == {k: plain[k] for k in plain if k not in ("seconds", "tolerances")}
    vox = run_tool(capsys, monkeypatch, args + ["--ground_truth", tmp_path / "scan.ply", "--scanners", tmp_path / "scanners.txt", "--voxel", 0.04] + opts)
    want_v = cloud.evaluate(rec, scan, [0.05], voxel=0.04, scanners=S[None], face_size=64, window=1, free_rel=0.05)
    assert vox["tolerances"] == want_v["tolerances"] and vox["observed"] == want["observed"] and vox["n_ground_truth"] == want_v["n_ground_truth"]
    # two scans: the walls with x < 0 seen from the room's scanner, the others from a second one; each file in its scanner's frame
    S2 = np.array([-0.3, 0.2, -0.1], f32)
    left = scan[:, 0] < 0
    cloud.write_ply(str(tmp_path / "a.ply"), scan[~left] - S)
    cloud.write_ply(str(tmp_path / "b.ply"), scan[left] - S2)
    rows = lambda s: "".join(f"{r[0]} {r[1]} {r[2]} {float(v)!r}\n" for r, v in zip(np.eye(3, dtype=int), s)) + "0 0 0 1\n"
    (tmp_path / "scans.mlp").write_text("<!DOCTYPE MeshLabDocument>\n<MeshLabProject>\n <MeshGroup>\n" + "".join(
        f'  <MLMesh label="{n}" filename="{n}">\n   <MLMatrix44>\n{rows(s)}</MLMatrix44>\n  </MLMesh>\n' for n, s in (("a.ply", S), ("b.ply", S2))) +
        " </MeshGroup>\n</MeshLabProject>\n")
    two = run_tool(capsys, monkeypatch, args + ["--scan_alignment", tmp_path / "scans.mlp"] + opts)
    gt = np.concatenate([(scan[~left] - S).astype(np.float64) + S.astype(np.float64), (scan[left] - S2).astype(np.float64) + S2.astype(np.float64)]).astype(f32)
    owner = np.concatenate([np.zeros((~left).sum(), np.int32), np.ones(left.sum(), np.int32)])
    want2 = cloud.evaluate(rec, gt, [0.05], scanners=np.stack([S, S2]), owner=owner, face_size=64, window=1, free_rel=0.05)
    assert two["tolerances"] == want2["tolerances"] and two["observed"] == want2["observed"] and two["observed"]["scanners"] == 2
    for bad in (["--ground_truth", tmp_path / "scan.ply", "--scan_alignment", tmp_path / "scans.mlp"], [], ["--ground_truth", tmp_path / "scan.ply", "--window", 2],
                ["--scan_alignment", tmp_path / "scans.mlp", "--scanners", tmp_path / "scanners.txt"]):
        with pytest.raises(SystemExit):
            run_tool(capsys, monkeypatch, args + bad)
