"""mpmvs_cloud_voxel_downsample on the GPU against the numpy statement of voxel_common.py, bit for bit (include/mpmvs.h, DESIGN.md
section 16), its place in evaluate(), and the two tools end to end."""
import importlib
import importlib.util
import json
import os
import sys
import threading

import numpy as np
import pytest

from voxel_common import assert_same, statement

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cloud(engine):
    return importlib.import_module("mp-mvs_amd.cloud")


def check(cloud, x, voxel, normals=None, colors=None, what=""):
    got = cloud.voxel_downsample(x, voxel, normals=normals, colors=colors, want_map=True)
    want = statement(x, voxel, normals, colors)
    assert_same(got, want, what)
    return got


def lattice(shift):
    """on each axis in turn: the borders mn + (k + 1/2) voxel, k = 0 .. 5 (exact in fp32) with their fp32 neighbours below and
    above, and mn itself"""
    voxel = np.float32(0.25)
    mn = np.float32(2.0) + np.float32(shift)
    b = (mn + (np.arange(6, dtype=np.float32) + np.float32(0.5)) * voxel).astype(np.float32)
    assert np.array_equal(b.astype(np.float64), float(mn) + (np.arange(6) + 0.5) * 0.25)
    line = np.concatenate([b, np.nextafter(b, np.float32(-np.inf)), np.nextafter(b, np.float32(np.inf))])
    pts = [np.full((1, 3), mn, np.float32)]
    for axis in range(3):
        p = np.full((len(line), 3), mn, np.float32)
        p[:, axis] = line
        pts.append(p)
    return np.concatenate(pts), voxel


@pytest.mark.parametrize("shift", [0.0, 1000.25])
def test_border_lattice(cloud, shift):
    x, voxel = lattice(shift)
    got = check(cloud, x, voxel, what=f"lattice + {shift}")
    # the property itself, not only the agreement: a border belongs to the upper cell, its neighbour below to the lower one
    v = got["voxel_of"]
    for axis in range(3):
        at, below, above = (v[1 + 18 * axis + 6 * j:1 + 18 * axis + 6 * j + 6] for j in range(3))
        assert np.array_equal(at, above) and len(set(at)) == 6
        assert below[0] == v[0] and np.array_equal(below[1:], at[:-1])
    assert len(got["xyz"]) == 19


@pytest.fixture(scope="module")
def random_cloud():
    rng = np.random.default_rng(5)
    n = 5000
    x = (10.0 + 3.0 * rng.random((n, 3))).astype(np.float32)
    x[1000:1300] = x[0:300]                                     # exact duplicates
    x[17, 0], x[18, 1], x[19, 2], x[4999] = np.nan, np.inf, -np.inf, np.nan
    x[20] = 900.0                                               # far away
    x[23] = -700.0
    nr = rng.normal(size=(n, 3)).astype(np.float32)
    nr /= np.linalg.norm(nr, axis=1, keepdims=True)
    nr[5, 1], nr[1005, 0] = np.nan, np.inf                      # a member whose normal adds nothing
    nr[40] *= 3                                                 # clamped components
    col = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    x[21] = x[22] = 500.0                                       # a pair alone in a voxel:
    nr[22] = -nr[21]                                            # n, -n -> the zero normal
    col[21], col[22] = 0, 1                                     # bytes {0, 1} -> 1, round half up
    return x, nr, col


def test_random_cloud(cloud, random_cloud):
    x, nr, col = random_cloud
    voxel = 0.2
    full = check(cloud, x, voxel, nr, col, "random")
    v = full["voxel_of"][21]
    assert v == full["voxel_of"][22] and full["count"][v] == 2
    assert np.array_equal(full["normals"][v], np.zeros(3, np.float32)) and np.array_equal(full["colors"][v], [1, 1, 1])
    assert (full["voxel_of"][[17, 18, 19, 4999]] == -1).all() and 1000 < len(full["xyz"]) < 4000
    for normals, colors in ((None, None), (nr, None), (None, col)):
        part = check(cloud, x, voxel, normals, colors, "random, optional arrays")
        for k in part:
            assert np.array_equal(part[k].view(np.uint8), full[k].view(np.uint8))
    bare = cloud.voxel_downsample(x, voxel, normals=nr, colors=col)   # out_voxel_of NULL
    assert "voxel_of" not in bare
    for k in bare:
        assert np.array_equal(bare[k].view(np.uint8), full[k].view(np.uint8))
    check(cloud, x, 0.003, nr, col, "random, fine")
    assert len(check(cloud, x, 4000.0, nr, col, "random, one voxel")["xyz"]) == 1


def test_70001_points_in_one_voxel_and_in_70001(cloud):
    """beyond one round of k_scan_totals (256 x 256 points), and the heaviest contention on one accumulator"""
    rng = np.random.default_rng(6)
    n = 70001
    x = (5.0 + 0.01 * rng.random((n, 3))).astype(np.float32)
    nr = np.full((n, 3), 0.577, np.float32)
    col = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    got = check(cloud, x, 1.0, nr, col, "one voxel")
    assert len(got["xyz"]) == 1 and got["count"][0] == n and got["first"][0] == 0
    i = np.arange(n)
    x = np.stack([1.0 + (i % 300) / 256.0, 1.0 + (i // 300) / 256.0, np.full(n, 1.5)], 1).astype(np.float32)
    got = check(cloud, x, 1.0 / 512.0, nr, col, "one-point voxels")
    assert np.array_equal(got["xyz"].view(np.uint32), x.view(np.uint32))
    assert np.array_equal(got["first"], i) and np.array_equal(got["voxel_of"], i) and (got["count"] == 1).all()
    assert np.array_equal(got["colors"], col)


@pytest.mark.parametrize("n", [1, 257])
def test_small_counts(cloud, n):
    rng = np.random.default_rng(n)
    x = (rng.random((n, 3)) * 0.1 - 3.0).astype(np.float32)
    got = check(cloud, x, 1.0 / 64.0, x[::-1].copy(), rng.integers(0, 256, (n, 3), dtype=np.uint8), f"n = {n}")
    assert 1 <= len(got["xyz"]) <= n


def test_pass_times(cloud):
    """the six pass times of a call with normals and colours are device times, the total is their sum as the library forms it, and a
    call that is answered on the host clears all seven"""
    rng = np.random.default_rng(11)
    n = 300
    x = (2.0 + rng.random((n, 3))).astype(np.float32)
    nr = rng.normal(size=(n, 3)).astype(np.float32)
    col = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    check(cloud, x, 0.125, nr, col, "pass times")
    total, passes = cloud.last_voxel_ms(passes=True)
    names = ("insert", "first", "scan", "number", "accumulate", "finish")
    assert tuple(passes) == names
    p = [np.float32(passes[k]) for k in names]
    print("voxel pass ms:", [float(v) for v in p], "total", total)
    assert all(v > 0.0 for v in p), passes
    assert np.float32(total) == ((p[0] + p[1]) + (p[2] + p[3])) + (p[4] + p[5])
    got = cloud.voxel_downsample(np.full((5, 3), np.nan, np.float32), 0.125, want_map=True)
    assert len(got["xyz"]) == 0 and (got["voxel_of"] == -1).all()
    total, passes = cloud.last_voxel_ms(passes=True)
    assert total == 0.0 and all(passes[k] == 0.0 for k in names), (total, passes)


def by_cell(res):
    """the output records as a sorted table (position, normal and colour bits, count): order-free"""
    cols = [res["xyz"].view(np.uint32), res["normals"].view(np.uint32), res["colors"].astype(np.uint32), res["count"].astype(np.uint32)[:, None]]
    tab = np.concatenate(cols, 1)
    return tab[np.lexsort(tab.T[::-1])]


def test_order_does_not_show(cloud, random_cloud):
    x, nr, col = random_cloud
    a = cloud.voxel_downsample(x, 0.2, normals=nr, colors=col, want_map=True)
    b = cloud.voxel_downsample(x, 0.2, normals=nr, colors=col, want_map=True)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k                      # twice on the same input: identical bytes
    perm = np.random.default_rng(7).permutation(len(x))
    p = cloud.voxel_downsample(x[perm], 0.2, normals=nr[perm], colors=col[perm], want_map=True)
    assert np.array_equal(by_cell(a), by_cell(p))                       # the same multiset of records
    # the maps are related by the permutation: input point perm[j] is point j of the permuted run
    ok = a["voxel_of"][perm] >= 0
    assert np.array_equal(ok, p["voxel_of"] >= 0)
    va, vp = a["voxel_of"][perm][ok], p["voxel_of"][ok]
    assert np.array_equal(a["xyz"][va].view(np.uint32), p["xyz"][vp].view(np.uint32))
    pair = np.unique(np.stack([va, vp], 1), axis=0)
    assert len(pair) == len(a["xyz"]) == len(p["xyz"])                  # one voxel there per voxel here
    # first = the smallest member index, in each run's own numbering
    inv = np.empty(len(perm), np.int64)
    inv[perm] = np.arange(len(perm))
    for v_a, v_p in pair[:200]:
        members = np.flatnonzero(a["voxel_of"] == v_a)
        assert a["first"][v_a] == members.min() and p["first"][v_p] == inv[members].min()


def test_map_reproduces_every_output(cloud, random_cloud):
    x, nr, col = random_cloud
    got = cloud.voxel_downsample(x, 0.2, normals=nr, colors=col, want_map=True)
    v = got["voxel_of"]
    m = len(got["xyz"])
    part = v >= 0
    assert np.array_equal(part, np.isfinite(x).all(1)) and set(v[part]) == set(range(m))
    assert np.array_equal(got["count"], np.bincount(v[part], minlength=m))
    first = np.full(m, len(x), np.int64)
    np.minimum.at(first, v[part], np.flatnonzero(part))
    assert np.array_equal(got["first"], first) and (np.diff(first) > 0).all()   # numbered by first appearance
    # the statement's arithmetic over the groups the map names
    e = float(np.float32(0.2))
    o = x[part].min(0).astype(np.float64) - 0.5 * e
    t = (x[part].astype(np.float64) - o) / e
    c = np.floor(t)
    S = np.zeros((m, 3), np.int64)
    np.add.at(S, v[part], np.rint((t - c) * 2.0 ** 30).astype(np.int64))
    cv = np.zeros((m, 3))
    cv[v[part]] = c
    assert np.array_equal(cv[v[part]], c)                                        # one cell per voxel
    xyz = (o + (cv + S.astype(np.float64) / (got["count"].astype(np.float64)[:, None] * 2.0 ** 30)) * e).astype(np.float32)
    assert np.array_equal(xyz.view(np.uint32), got["xyz"].view(np.uint32))
    good = part & np.isfinite(nr).all(1)
    N = np.zeros((m, 3), np.int64)
    np.add.at(N, v[good], np.rint(np.clip(nr[good].astype(np.float64), -1, 1) * 2.0 ** 30).astype(np.int64))
    Nd = N.astype(np.float64)
    L = np.sqrt((Nd[:, 0] * Nd[:, 0] + Nd[:, 1] * Nd[:, 1]) + Nd[:, 2] * Nd[:, 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        nrm = np.where(L[:, None] == 0, 0.0, Nd / L[:, None]).astype(np.float32)
    assert np.array_equal(nrm.view(np.uint32), got["normals"].view(np.uint32))
    Cs = np.zeros((m, 3), np.int64)
    np.add.at(Cs, v[part], col[part].astype(np.int64))
    cnt = got["count"].astype(np.int64)[:, None]
    assert np.array_equal(((2 * Cs + cnt) // (2 * cnt)).astype(np.uint8), got["colors"])


def test_two_host_threads(cloud, random_cloud):
    x, nr, col = random_cloud
    jobs = [(x, 0.2), (x[::-1].copy(), 0.05)]
    single = [cloud.voxel_downsample(p, v, want_map=True) for p, v in jobs]
    got, errors = [[], []], []

    def work(t):
        try:
            for _ in range(4):
                got[t].append(cloud.voxel_downsample(*jobs[t], want_map=True))
                assert cloud.last_voxel_ms() > 0.0
        except Exception as e:   # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors
    for t in range(2):
        assert len(got[t]) == 4
        for r in got[t]:
            for k in single[t]:
                assert r[k].tobytes() == single[t][k].tobytes(), (t, k)


@pytest.fixture(scope="module")
def score_case():
    """a ground-truth plane patch; a reconstruction of an over-dense accurate part (20 points per voxel) and a sparse part
    displaced by 3 tolerances"""
    rng = np.random.default_rng(9)
    tol, V = 0.02, 0.01
    g = np.arange(0, 100) * 0.004
    gt = np.stack([*np.meshgrid(g, g, indexing="ij"), np.zeros((100, 100))], -1).reshape(-1, 3).astype(np.float32)
    cells = np.stack(np.meshgrid(np.arange(20), np.arange(20), indexing="ij"), -1).reshape(-1, 2)
    dense = np.concatenate([(np.repeat(cells, 20, 0) + 0.1 + 0.8 * rng.random((8000, 2))) * V, 0.001 * rng.random((8000, 1))], 1)
    sparse = np.concatenate([0.2 + (cells + 0.5) * V * 1.05, np.full((400, 1), 3 * tol)], 1)
    rec = np.concatenate([dense, sparse]).astype(np.float32)
    return rec[rng.permutation(len(rec))], gt, tol, V


def test_score_with_voxel(cloud, score_case):
    rec, gt, tol, V = score_case
    tols = [tol, 2 * tol]
    plain = cloud.evaluate(rec, gt, tols)
    vox = cloud.evaluate(rec, gt, tols, voxel=V)
    s_rec, s_gt = statement(rec, V), statement(gt, V)
    ref = cloud.evaluate(s_rec["xyz"], s_gt["xyz"], tols)
    for k in ref:
        assert vox[k] == ref[k], k                                       # every field they share
    assert vox["voxel"] == V and vox["n_reconstruction_in"] == len(rec) and vox["n_ground_truth_in"] == len(gt)
    assert vox["n_reconstruction"] == len(s_rec["xyz"]) and vox["n_ground_truth"] == len(s_gt["xyz"])
    assert not {"voxel", "n_reconstruction_in", "n_ground_truth_in"} & set(plain)
    # the dense accurate part no longer outweighs the displaced one: a property of the input, so of the statement too
    assert ref["tolerances"][0]["accuracy"] < plain["tolerances"][0]["accuracy"]
    assert vox["tolerances"][0]["accuracy"] < plain["tolerances"][0]["accuracy"]
    assert plain["tolerances"][0]["accuracy"] > 0.9 and vox["tolerances"][0]["accuracy"] < 0.6


def write_ply(path, xyz, normals=None, colors=None):
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    head = "property float x\nproperty float y\nproperty float z\n"
    if normals is not None:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        head += "property float nx\nproperty float ny\nproperty float nz\n"
    if colors is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        head += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    rec = np.zeros(len(xyz), np.dtype(fields))
    for k, name in enumerate("xyz"):
        rec[name] = xyz[:, k]
    if normals is not None:
        for k, name in enumerate(("nx", "ny", "nz")):
            rec[name] = normals[:, k]
    if colors is not None:
        for k, name in enumerate(("red", "green", "blue")):
            rec[name] = colors[:, k]
    with open(path, "wb") as fh:
        fh.write(f"ply\nformat binary_little_endian 1.0\nelement vertex {len(xyz)}\n{head}end_header\n".encode())
        fh.write(rec.tobytes())


def run_tool(tool, capsys, monkeypatch, argv):
    spec = importlib.util.spec_from_file_location(tool + "_tool", os.path.join(ROOT, "tools", tool + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(sys, "argv", [tool + ".py"] + [str(a) for a in argv])
    capsys.readouterr()
    mod.main()
    return capsys.readouterr().out


def test_eval_ply_voxel(cloud, score_case, tmp_path, capsys, monkeypatch):
    rec, gt, tol, V = score_case
    write_ply(tmp_path / "rec.ply", rec)
    write_ply(tmp_path / "gt.ply", gt)
    args = ["--reconstruction", tmp_path / "rec.ply", "--ground_truth", tmp_path / "gt.ply", "--tolerances", f"{tol},{2 * tol}"]
    plain_out = run_tool("eval_ply", capsys, monkeypatch, args)
    plain = json.loads(plain_out.strip().splitlines()[-1])
    vox = json.loads(run_tool("eval_ply", capsys, monkeypatch, args + ["--voxel", V]).strip().splitlines()[-1])
    s_rec, s_gt = statement(rec, V), statement(gt, V)
    assert (vox["voxel"], vox["n_reconstruction_in"], vox["n_ground_truth_in"]) == (V, len(rec), len(gt))
    assert (vox["n_reconstruction"], vox["n_ground_truth"]) == (len(s_rec["xyz"]), len(s_gt["xyz"]))
    want = cloud.evaluate(rec, gt, [tol, 2 * tol], voxel=V)
    assert vox["tolerances"] == want["tolerances"]
    # without the flag: the output of before
    base = cloud.evaluate(rec, gt, [tol, 2 * tol])
    assert set(plain) == set(base) | {"seconds"} and set(plain["seconds"]) == {"read", "upload_build", "query"}
    assert all(plain[k] == base[k] for k in base)
    # the resampled clouds are registered: --refine runs on them
    fine = json.loads(run_tool("eval_ply", capsys, monkeypatch, args + ["--voxel", V, "--refine", "--refine_no_scale"]).strip().splitlines()[-1])
    assert fine["n_reconstruction"] == len(s_rec["xyz"]) and all(r["inliers"] <= len(s_rec["xyz"]) for r in fine["refine"]["rounds"])
    with pytest.raises(SystemExit):
        run_tool("eval_ply", capsys, monkeypatch, ["--help"])
    assert "Tanks and Temples uses half its tolerance" in " ".join(capsys.readouterr().out.split())


def test_downsample_ply(cloud, random_cloud, tmp_path, capsys, monkeypatch):
    x, nr, col = random_cloud
    ok = np.isfinite(x).all(1) & np.isfinite(nr).all(1)
    x, nr, col = x[ok], nr[ok], col[ok]
    write_ply(tmp_path / "a.ply", x, nr, col)
    out = run_tool("downsample_ply", capsys, monkeypatch, ["--input", tmp_path / "a.ply", "--output", tmp_path / "b.ply", "--voxel", 0.2])
    line = json.loads(out.strip().splitlines()[-1])
    want = statement(x, 0.2, nr, col)
    assert line["n"] == len(x) and line["m"] == len(want["xyz"]) and line["device_ms"] > 0
    back = cloud.read_ply(tmp_path / "b.ply")
    for k in ("xyz", "normals", "colors"):
        assert np.array_equal(back[k].view(np.uint8), want[k].view(np.uint8)), k
    data = open(tmp_path / "b.ply", "rb").read()
    body = data.index(b"\n", data.index(b"end_header")) + 1
    assert len(data) - body == 27 * line["m"] and len(back["xyz"]) == line["m"]   # the reference's 27-byte records
    # positions only: normals and colours are written as zeros
    write_ply(tmp_path / "c.ply", x)
    out = run_tool("downsample_ply", capsys, monkeypatch, ["--input", tmp_path / "c.ply", "--output", tmp_path / "d.ply", "--voxel", 0.2])
    back = cloud.read_ply(tmp_path / "d.ply")
    assert np.array_equal(back["xyz"].view(np.uint32), want["xyz"].view(np.uint32))
    assert not back["normals"].any() and not back["colors"].any()
