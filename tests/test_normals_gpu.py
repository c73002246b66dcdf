"""mpmvs_cloud_normals on the GPU against the numpy statement of normals_common.py, bit for bit (include/mpmvs.h, DESIGN.md section
18), and tools/normals_ply.py end to end."""
import ctypes as C
import importlib
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from knn_common import assert_knn_same, bits, brute_knn, first_k, property_scene
from normals_common import angle_to, assert_normals_same, sphere_scene, statement_normals
from test_knn_gpu import random_cloud, run_tool, write_ply  # noqa: F401  (random_cloud is a fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (2, 3, 4, 5, 8, 9, 16, 17, 31, 32)
VIEW = (11.5, 11.25, 40.0)


@pytest.fixture(scope="module")
def cloud(engine):
    return importlib.import_module("mp-mvs_amd.cloud")


@pytest.fixture(scope="module")
def ref_normals():
    """reference normals for the 5 000 points of random_cloud: random, some NaN, inf and zero"""
    ref = np.random.default_rng(44).normal(size=(5000, 3)).astype(np.float32)
    ref[40], ref[41, 2], ref[42] = np.nan, np.inf, 0.0
    return ref


def want(x, radius, k, full=None, **kw):
    """the statement at k, from the brute-force answer for k = 32 when there is one"""
    return statement_normals(x, radius, k, knn=first_k(full, k) if full is not None else None, **kw)


@pytest.mark.parametrize("radius", [0.05, 0.3, 4000.0])
def test_random_cloud(cloud, random_cloud, ref_normals, radius):
    x, _ = random_cloud
    full = brute_knn(x, None, radius, 32)
    defined = 0
    with cloud.Cloud(x) as c:
        for k in KS:
            assert_normals_same(c.normals(radius, k, want_within=True), want(x, radius, k, full), f"canonical, radius {radius}, k {k}")
            assert_normals_same(c.normals(radius, k, viewpoint=VIEW, want_within=True), want(x, radius, k, full, viewpoint=VIEW),
                                f"viewpoint, radius {radius}, k {k}")
            got = c.normals(radius, k, reference=ref_normals, want_within=True)
            assert_normals_same(got, want(x, radius, k, full, reference=ref_normals), f"reference, radius {radius}, k {k}")
            defined = int(np.isfinite(got[1]).sum())
            ms, _ = c.normals_ms()
            assert ms > 0
        nrm, none = c.normals(radius, 5, want_curvature=False)           # out_curvature and out_within NULL
        assert none is None and np.array_equal(bits(nrm), bits(want(x, radius, 5, full)[0]))
        nrm, none, within = c.normals(radius, 5, want_curvature=False, want_within=True)
        assert none is None and np.array_equal(within, full[2]) and np.array_equal(bits(nrm), bits(want(x, radius, 5, full)[0]))
    if radius == 0.05:
        assert 5 < defined < 1000            # mostly undefined: empty rows, single twins
    if radius == 0.3:
        assert 4900 < defined <= 4994        # the two far points have no neighbour
    if radius == 4000.0:
        assert defined == 4996               # every finite point


def test_candidate_counts_0_to_3_and_around_k(cloud):
    """clusters of m + 1 points far apart: every member has exactly m candidates"""
    rng = np.random.default_rng(12)
    sizes = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33)
    x = np.concatenate([np.array([100.0 * m, 0, 0]) + 0.01 * rng.random((m + 1, 3)) for m in sizes]).astype(np.float32)
    member = np.concatenate([np.full(m + 1, m) for m in sizes])
    with cloud.Cloud(x) as c:
        for k in (2, 4, 8, 16, 32):
            got = c.normals(0.05, k, want_within=True)
            assert_normals_same(got, statement_normals(x, 0.05, k), f"clusters, k {k}")
            assert np.array_equal(got[2], member) and np.array_equal(np.isfinite(got[1]), member >= 2)
            for m in (k - 1, k, k + 1):
                assert m in sizes


def test_duplicates_only_and_collinear(cloud):
    x = np.array([[1, 2, 3]] * 6 + [[50 + 0.25 * j, 7, -2] for j in range(7)] + [[90 + 0.25 * j, 0.25 * j, 3] for j in range(5)]
                 + [[200, 0, 0], [200.5, 0, 0], [200, 0.5, 0]], np.float32)
    with cloud.Cloud(x) as c:
        for k in (2, 4, 6):
            got = c.normals(2.0, k, want_within=True)
            assert_normals_same(got, statement_normals(x, 2.0, k), f"degenerate, k {k}")
            assert not bits(got[0][:18]).any() and np.isposinf(got[1][:18]).all() and (got[2][:18] >= 4).all()   # undefined: +0 0 0 and inf
            assert (np.abs(got[0][18:, 2]) == 1.0).all() and not got[1][18:].any()                               # two neighbours off a line


@pytest.mark.parametrize("shift", [0.0, 1000.25, -3.125])
def test_lattice_cell_borders(cloud, shift):
    """the cell-border lattice of test_knn_gpu.py as a cloud of its own: neighbours at exactly the radius, one ulp beyond and a little
    inside along x, and the ties of a cubic lattice in the pick"""
    r = np.float32(0.25)
    g = np.arange(-4, 5, dtype=np.float32) * r
    t = (np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + np.float32(shift)).astype(np.float32)
    parts = [t]
    for s in (r, np.nextafter(r, np.float32(1)), r - np.float32(2.0 ** -20)):
        for sign in (-1.0, 1.0):
            parts.append(t + np.array([sign * s, 0, 0], np.float32))
    x = np.concatenate(parts).astype(np.float32)
    x[len(t):] += np.array([0, 0.0625, 0.03125], np.float32)         # off the lattice in y and z
    full = brute_knn(x, None, float(r), 32)
    with cloud.Cloud(x) as c:
        for k in (5, 8, 32):
            assert_normals_same(c.normals(float(r), k, want_within=True), want(x, float(r), k, full), f"lattice + {shift}, k {k}")
        assert_normals_same(c.normals(float(r), 32, viewpoint=(shift, shift, shift), want_within=True),
                            want(x, float(r), 32, full, viewpoint=(shift, shift, shift)), f"lattice + {shift}, viewpoint")


def test_exact_lattice(cloud):
    g = np.arange(3, dtype=np.float32)
    x = np.stack([*np.meshgrid(g, g, indexing="ij"), np.zeros((3, 3), np.float32)], -1).reshape(-1, 3) + np.float32(4.0)
    up = np.tile(np.array([0, 0, 1], np.float32), (9, 1))
    with cloud.Cloud(x) as c:
        nrm, curv = c.normals(1.5, 8)
        assert np.array_equal(bits(nrm), bits(up)) and not bits(curv).any()
        assert np.array_equal(c.normals(1.5, 8, viewpoint=(5, 5, -9))[0], -up)
        assert np.array_equal(bits(c.normals(1.5, 8, viewpoint=(100, -3, 4))[0]), bits(up))     # in the plane: dot == 0
        ref = -up.copy()
        ref[3] = np.nan
        assert np.array_equal(c.normals(1.5, 8, reference=ref)[0][:, 2], np.where(np.arange(9) == 3, 1.0, -1.0))


@pytest.mark.parametrize("scale", [-40, 40])
def test_scaled_cloud(cloud, random_cloud, scale):
    """tiny and huge magnitudes through the fp64 path of the device"""
    x = np.ldexp(random_cloud[0][:1500], scale).astype(np.float32)
    radius = float(np.ldexp(np.float32(0.3), scale))
    view = tuple(float(v) for v in np.ldexp(np.array(VIEW), scale))
    full = brute_knn(x, None, radius, 32)
    with cloud.Cloud(x) as c:
        for k in (3, 8, 16, 32):
            got = c.normals(radius, k, viewpoint=view, want_within=True)
            assert_normals_same(got, want(x, radius, k, full, viewpoint=view), f"x 2^{scale}, k {k}")
        assert np.isfinite(got[1]).sum() > 1000


@pytest.mark.parametrize("n", [1, 257])
def test_small_counts(cloud, n):
    rng = np.random.default_rng(n)
    x = (rng.random((n, 3)) * 0.1 - 3.0).astype(np.float32)
    with cloud.Cloud(x) as c:
        for k in (2, 9, 32):
            assert_normals_same(c.normals(1.0 / 64.0, k, want_within=True), statement_normals(x, 1.0 / 64.0, k), f"n {n}, k {k}")
            assert_normals_same(c.normals(0.05, k, viewpoint=(0, 0, 0), want_within=True), statement_normals(x, 0.05, k, viewpoint=(0, 0, 0)), f"n {n}, k {k}, wide")
    r = cloud.estimate_normals(x, 0.05, 9)
    assert_normals_same((r["normals"], r["curvature"], r["within"]), statement_normals(x, 0.05, 9), f"n {n}, estimate_normals")


def test_70001_points_in_one_cell(cloud):
    rng = np.random.default_rng(6)
    n = 70001
    x = (5.0 + 0.01 * rng.random((n, 3))).astype(np.float32)
    rows = np.sort(rng.choice(n, 500, replace=False))
    rows[0], rows[-1] = 0, n - 1
    ref = rng.normal(size=(n, 3)).astype(np.float32)
    with cloud.Cloud(x) as c:
        nrm, curv, within = c.normals(1.0, 32, reference=ref, want_within=True)
        assert c.stats()["fullest"] == n and c.stats()["cells"] == 1
    assert (within == n - 1).all()
    assert_normals_same((nrm[rows], curv[rows], within[rows]), statement_normals(x, 1.0, 32, reference=ref[rows], self_rows=rows,
                                                                               knn=brute_knn(x, None, 1.0, 32, chunk=128, self_rows=rows)), "one cell")


def test_argument_errors(cloud, engine):
    _, fns = engine.load()
    t = np.random.default_rng(1).random((50, 3)).astype(np.float32)
    out = np.full((50, 3), 7.0, np.float32)
    view = (C.c_double * 3)(0.0, 0.0, 1.0)
    h = C.c_void_p(None)
    assert fns["cloud_create"](0, 50, t.ctypes.data, C.byref(h)) == 0

    def call(radius=0.1, k=4, orient=0, v=None, ref=None, o=out):
        return fns["cloud_normals"](h, radius, k, orient, v, ref, o.ctypes.data if o is not None else None, None, None)

    try:
        for k in (1, 0, 33, -1):
            assert call(k=k) == -2, k
            assert "k must lie in [2, 32]" in fns["last_error"](None).decode()
        assert call(o=None) == -2                                         # NULL out_normals
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert call(radius=bad) == -2, bad
        for orient in (-1, 3):
            assert call(orient=orient, v=view, ref=t.ctypes.data) == -2
        assert call(orient=1) == -2                                       # NULL view
        for j in range(3):
            for bad in (float("nan"), float("inf")):
                v = (C.c_double * 3)(0.0, 0.0, 1.0)
                v[j] = bad
                assert call(orient=1, v=v) == -2 and "viewpoint" in fns["last_error"](None).decode()
        assert call(orient=2) == -2                                       # NULL ref_normals
        assert (out == 7.0).all()                                         # a refusal writes nothing
        assert call(radius=1e-8) == -3 and "2^21" in fns["last_error"](None).decode()
        assert (out == 7.0).all()
        assert call(k=32, orient=1, v=view) == 0                          # still usable
        assert np.array_equal(bits(out), bits(statement_normals(t, 0.1, 32, viewpoint=(0, 0, 1))[0]))
    finally:
        fns["cloud_destroy"](h)
    with cloud.Cloud(t) as c:
        for k in (1, 33):
            with pytest.raises(ValueError):
                c.normals(0.1, k)
        with pytest.raises(ValueError):
            c.normals(-1.0)
        with pytest.raises(ValueError):
            c.normals(0.1, viewpoint=(0, 0, 1), reference=t)              # mutually exclusive
        with pytest.raises(ValueError):
            c.normals(0.1, viewpoint=(0, 0, float("nan")))
        with pytest.raises(ValueError):
            c.normals(0.1, reference=t[:10])
    # a cloud without a finite point, and an empty one: answered without a launch
    for empty in (np.full((4, 3), np.nan, np.float32), np.zeros((0, 3), np.float32)):
        with cloud.Cloud(empty) as c:
            nrm, curv, within = c.normals(0.5, 3, want_within=True)
            assert nrm.shape == (len(empty), 3) and not bits(nrm).any() and np.isposinf(curv).all() and not within.any()
            assert c.normals_ms() == (0.0, 0.0)


def test_handle_reuse_and_grid_cache(cloud, random_cloud):
    x, q = random_cloud
    with cloud.Cloud(x) as c:
        res, build = [], []
        for step, r in enumerate((0.05, 0.3, 0.05, 0.3)):
            if step == 1:
                near = c.nearest(q, r)                       # this call builds the grid of 0.3 ...
                assert c.kernel_ms()[1] > 0
            if step == 2:
                knn = c.knn_self(r, 8, want_within=True)     # a knn call in between
            res.append(c.normals(r, 8, viewpoint=VIEW, want_within=True))
            ms, b = c.normals_ms()
            assert ms > 0
            build.append(b)
        assert build[0] > 0 and build[1] == 0 and build[2] == 0 and build[3] == 0   # ... so no normals call builds it again
        c.knn_self(0.05, 4)
        assert c.knn_ms()[1] == 0                            # and knn reuses the grid a normals call built
        c.nearest(q, 0.05)
        assert c.kernel_ms()[1] == 0
    for a, b in ((0, 2), (1, 3)):
        for u, v in zip(res[a], res[b]):
            assert u.tobytes() == v.tobytes()                # two runs: identical bytes
    full = {r: brute_knn(x, None, r, 8) for r in (0.05, 0.3)}
    assert_knn_same(knn, full[0.05], "knn in between")
    assert_knn_same((near[0][:, None], near[1][:, None]), first_k(brute_knn(x, q, 0.3, 1), 1)[:2] + (None,), "nearest in between")
    assert_normals_same(res[0], want(x, 0.05, 8, full[0.05], viewpoint=VIEW), "reused handle, 0.05")
    assert_normals_same(res[1], want(x, 0.3, 8, full[0.3], viewpoint=VIEW), "reused handle, 0.3")


def test_two_host_threads(cloud, random_cloud, ref_normals):
    x, _ = random_cloud
    jobs = [(x, 0.3, 16, {"viewpoint": VIEW}), (x[::-1].copy(), 0.05, 4, {"reference": ref_normals})]
    single = []
    for xx, r, k, kw in jobs:
        with cloud.Cloud(xx) as c:
            single.append(c.normals(r, k, want_within=True, **kw))
    got, errors = [[], []], []

    def work(t):
        try:
            xx, r, k, kw = jobs[t]
            with cloud.Cloud(xx) as c:                       # a handle of the thread's own
                for _ in range(4):
                    got[t].append(c.normals(r, k, want_within=True, **kw))
                    assert c.normals_ms()[0] > 0.0
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
            for u, v in zip(r, single[t]):
                assert u.tobytes() == v.tobytes(), t
    assert_normals_same(single[0], statement_normals(x, 0.3, 16, viewpoint=VIEW), "thread 0's job")


CALLER_ORDER_CHILD = """
import importlib, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
cloud = importlib.import_module("mp-mvs_amd.cloud")
z = np.load(sys.argv[2])
x, ref = z["x"], z["ref"]
out = {}
with cloud.Cloud(x) as c:
    for k in (2, 5, 16, 32):
        out[f"cn{k}"], out[f"cc{k}"], out[f"cw{k}"] = c.normals(0.3, k, want_within=True)
        out[f"vn{k}"], out[f"vc{k}"], out[f"vw{k}"] = c.normals(0.3, k, viewpoint=(11.5, 11.25, 40.0), want_within=True)
        out[f"rn{k}"], out[f"rc{k}"], out[f"rw{k}"] = c.normals(0.3, k, reference=ref, want_within=True)
np.savez(sys.argv[3], **out)
"""


def test_caller_order_in_a_child_process(random_cloud, ref_normals, tmp_path):
    """MPMVS_CLOUD_BIN=0 is read once per process: a child with the variable set serves the points in caller order (no binning,
    order == NULL in the kernel) and must give the same bits"""
    x = random_cloud[0][:1500].copy()
    ref = ref_normals[:1500].copy()
    np.savez(tmp_path / "in.npz", x=x, ref=ref)
    env = dict(os.environ, MPMVS_CLOUD_BIN="0")
    done = subprocess.run([sys.executable, "-c", CALLER_ORDER_CHILD, ROOT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], env=env,
                          capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    got = np.load(tmp_path / "out.npz")
    full = brute_knn(x, None, 0.3, 32)
    for k in (2, 5, 16, 32):
        assert_normals_same((got[f"cn{k}"], got[f"cc{k}"], got[f"cw{k}"]), want(x, 0.3, k, full), f"caller order, canonical, k {k}")
        assert_normals_same((got[f"vn{k}"], got[f"vc{k}"], got[f"vw{k}"]), want(x, 0.3, k, full, viewpoint=VIEW), f"caller order, viewpoint, k {k}")
        assert_normals_same((got[f"rn{k}"], got[f"rc{k}"], got[f"rw{k}"]), want(x, 0.3, k, full, reference=ref), f"caller order, reference, k {k}")


# ---- the property scenes -----------------------------------------------------------------------------------------------------
def test_plane_scene(cloud):
    x, plane = property_scene()
    with cloud.Cloud(x) as c:
        got = c.normals(0.05, 16, want_within=True)
    assert_normals_same(got, statement_normals(x, 0.05, 16), "plane scene")
    ang = angle_to(got[0][plane], [0.0, 0.0, 1.0])
    print(f"plane scene on the device: max {ang.max():.2f} deg, median {np.median(ang):.2f} deg")
    assert plane.sum() == 1600 and np.isfinite(got[1][plane]).all() and ang.max() < 15.0


def test_sphere_scene(cloud):
    x, centre = sphere_scene()
    with cloud.Cloud(x) as c:
        got = c.normals(0.2, 16, viewpoint=centre, want_within=True)
    assert_normals_same(got, statement_normals(x, 0.2, 16, viewpoint=centre), "sphere scene")
    radial = centre - x.astype(np.float64)
    ang = angle_to(got[0], radial)
    print(f"sphere scene on the device: max {ang.max():.2f} deg")
    assert np.isfinite(got[1]).all() and ang.max() < 15.0 and ((got[0] * radial).sum(1) > 0).all()


# ---- the tool -------------------------------------------------------------------------------------------------------------------
def read_records(path, n):
    data = open(path, "rb").read()
    body = data.index(b"\n", data.index(b"end_header")) + 1
    assert len(data) - body == 27 * n                                    # the reference's 27-byte records
    return np.frombuffer(data, np.dtype([("p", "<f4", 3), ("n", "<f4", 3), ("c", "u1", 3)]), n, body)


def test_normals_ply(cloud, tmp_path, capsys, monkeypatch):
    x, plane = property_scene()
    rng = np.random.default_rng(3)
    stored = np.tile(np.array([0.1, -0.1, -1.0], np.float32), (len(x), 1)) + 0.05 * rng.normal(size=x.shape).astype(np.float32)
    col = rng.integers(0, 256, x.shape, dtype=np.uint8)
    # a file with normals: they decide the sign, and the angle to them is reported
    write_ply(tmp_path / "a.ply", x, stored, col)
    out = run_tool("normals_ply", capsys, monkeypatch, ["--input", tmp_path / "a.ply", "--output", tmp_path / "b.ply", "--radius", 0.05, "--k", 16])
    line = json.loads(out.strip().splitlines()[-1])
    nrm, curv, _ = statement_normals(x, 0.05, 16, reference=stored)
    defined = np.isfinite(curv)
    assert (line["n"], line["defined"], line["undefined"], line["written"]) == (len(x), int(defined.sum()), int((~defined).sum()), len(x))
    assert line["orientation"] == "stored" and line["device_ms"] > 0 and 0 < line["undefined"] <= 61
    s = line["stored_normals"]
    assert s["compared"] == line["defined"] and 0 < s["angle_median_deg"] < 15 and s["angle_median_deg"] <= s["angle_p90_deg"] < 180
    rec = read_records(tmp_path / "b.ply", len(x))
    assert np.array_equal(bits(rec["p"]), bits(x)) and np.array_equal(bits(rec["n"]), bits(nrm)) and np.array_equal(rec["c"], col)
    assert (rec["n"][plane][:, 2] < 0).all() and not rec["n"][~defined].any()
    # positions only, a viewpoint above, the undefined points dropped
    write_ply(tmp_path / "c.ply", x)
    out = run_tool("normals_ply", capsys, monkeypatch, ["--input", tmp_path / "c.ply", "--output", tmp_path / "d.ply", "--radius", 0.05, "--viewpoint", 0.2, 0.2,
                                                       3.0, "--drop_undefined"])
    line = json.loads(out.strip().splitlines()[-1])
    nrm, curv, _ = statement_normals(x, 0.05, 16, viewpoint=(0.2, 0.2, 3.0))
    defined = np.isfinite(curv)
    assert line["orientation"] == "viewpoint" and line["written"] == int(defined.sum()) == line["defined"] and "stored_normals" not in line
    rec = read_records(tmp_path / "d.ply", int(defined.sum()))
    assert np.array_equal(bits(rec["p"]), bits(x[defined])) and np.array_equal(bits(rec["n"]), bits(nrm[defined])) and not rec["c"].any()
    assert (rec["n"][plane[defined]][:, 2] > 0).all()
    # neither: canonical
    out = run_tool("normals_ply", capsys, monkeypatch, ["--input", tmp_path / "c.ply", "--output", tmp_path / "e.ply", "--radius", 0.05, "--k", 8])
    assert json.loads(out.strip().splitlines()[-1])["orientation"] == "canonical"
    assert np.array_equal(bits(read_records(tmp_path / "e.ply", len(x))["n"]), bits(statement_normals(x, 0.05, 8)[0]))
