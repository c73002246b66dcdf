"""mpmvs_cloud_knn and mpmvs_cloud_outliers on the GPU against the numpy statements of knn_common.py, bit for bit (include/mpmvs.h,
DESIGN.md section 17), and tools/clean_ply.py end to end."""
import ctypes as C
import importlib
import importlib.util
import json
import os
import sys
import threading

import numpy as np
import pytest

from cloud_common import brute_nearest
from knn_common import assert_knn_same, assert_outliers_same, bits, brute_knn, first_k, property_scene, statement_outliers

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1, 2, 5, 8, 9, 16, 32)


@pytest.fixture(scope="module")
def cloud(engine):
    return importlib.import_module("mp-mvs_amd.cloud")


@pytest.fixture(scope="module")
def random_cloud():
    """5 000 points with 300 exact duplicates, NaN / +-inf points and two far points (test_voxel_gpu.py::random_cloud), and 1 000
    queries of their own, some not finite and some on a target"""
    rng = np.random.default_rng(5)
    n = 5000
    x = (10.0 + 3.0 * rng.random((n, 3))).astype(np.float32)
    x[1000:1300] = x[0:300]                                     # exact duplicates
    x[17, 0], x[18, 1], x[19, 2], x[4999] = np.nan, np.inf, -np.inf, np.nan
    x[20] = 900.0                                               # far away
    x[23] = -700.0
    q = (10.0 + 3.0 * rng.random((1000, 3))).astype(np.float32)
    q[5, 2], q[6, 0], q[7, 1] = np.nan, np.inf, -np.inf
    q[8:40] = x[100:132]                                        # on a target, each of which has a twin: (0, 100 + j), then (0, 1100 + j)
    return x, q


_REF = {}


def reference(x, q, radius):
    """the statement for k = 32, computed once per radius and kind of query and left unchanged"""
    key = (radius, q is None)
    if key not in _REF:
        _REF[key] = brute_knn(x, q, radius, 32)
        for a in _REF[key]:
            a.setflags(write=False)
    return _REF[key]


@pytest.mark.parametrize("radius", [0.05, 0.3, 4000.0])
def test_random_cloud(cloud, random_cloud, radius):
    x, q = random_cloud
    with cloud.Cloud(x) as c:
        for k in KS:
            assert_knn_same(c.knn_self(radius, k, want_within=True), first_k(reference(x, None, radius), k), f"self, radius {radius}, k {k}")
            assert_knn_same(c.knn(q, radius, k, want_within=True), first_k(reference(x, q, radius), k), f"queries, radius {radius}, k {k}")
        d2, none = c.knn_self(radius, 5, want_idx=False)      # out_idx and out_within NULL
        assert none is None and np.array_equal(bits(d2), bits(reference(x, None, radius)[0][:, :5]))
    d2, idx, within = reference(x, None, radius)
    assert np.array_equal(idx == -1, np.isinf(d2)) and (within[[17, 18, 19, 4999]] == 0).all()
    if radius == 0.05:
        assert 600 <= (within > 0).sum() < 2000                            # mostly empty rows; the twins have each other
    if radius == 4000.0:
        assert (within[np.isfinite(x).all(1)] == 4995).all()               # every finite point but itself


def test_k_1_equals_nearest(cloud, random_cloud):
    x, q = random_cloud
    with cloud.Cloud(x) as c:
        for radius in (0.05, 0.3):
            d2n, idxn = c.nearest(q, radius)
            d2, idx = c.knn(q, radius, 1)
            assert np.array_equal(bits(d2[:, 0]), bits(d2n)) and np.array_equal(idx[:, 0], idxn)


def test_self_exclusion_is_by_index(cloud, random_cloud):
    x, _ = random_cloud
    radius = 0.3
    with cloud.Cloud(x) as c:
        d2q, idxq = c.knn(x, radius, 4)                      # the cloud's own array as explicit queries: every point finds itself
        d2s, idxs = c.knn_self(radius, 4)
    fin = np.isfinite(x).all(1)
    twin = np.flatnonzero((x[1000:1300] == x[0:300]).all(1))  # the pairs j, 1000 + j still equal after the special points went in
    assert len(twin) == 295
    first = np.arange(len(x))
    first[1000 + twin] = twin                                # the smallest index at a duplicated position
    assert not d2q[fin, 0].any() and np.array_equal(idxq[fin, 0], first[fin])
    assert (idxs != np.arange(len(x))[:, None]).all()        # never itself
    # a duplicated point: its twin at d2 = +0 comes first
    assert not bits(d2s[twin, 0]).any() and np.array_equal(idxs[twin, 0], 1000 + twin)
    assert not bits(d2s[1000 + twin, 0]).any() and np.array_equal(idxs[1000 + twin, 0], twin)
    single = fin.copy()
    single[twin] = single[1000 + twin] = False
    assert (d2s[single, 0] > 0).all()
    # the self answer is the explicit answer with the own index struck out
    own = idxq == np.arange(len(x))[:, None]
    assert (own[fin].sum(1) == 1).all()
    for i in (0, 150, 1000, 2500, 4998):
        keep = ~own[i]
        assert np.array_equal(idxs[i, :3], idxq[i][keep][:3]) and np.array_equal(bits(d2s[i, :3]), bits(d2q[i][keep][:3]))


@pytest.mark.parametrize("shift", [0.0, 1000.25])
def test_lattice_cell_borders(cloud, shift):
    """the cell-border lattice of test_cloud_gpu.py: queries displaced from lattice points by the radius, by one ulp more and by a
    little less, along the axes and the face diagonals"""
    r = np.float32(0.25)
    g = np.arange(-4, 5, dtype=np.float32) * r
    t = (np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + np.float32(shift)).astype(np.float32)
    steps = [r, np.nextafter(r, np.float32(1)), r - np.float32(2.0 ** -20)]
    qs = [t]
    for s in steps:
        for sign in (-1.0, 1.0):
            for ax in range(3):
                d = np.zeros(3, np.float32)
                d[ax] = sign * s
                qs.append(t + d)
            for a, b in ((0, 1), (1, 2), (0, 2)):
                d = np.zeros(3, np.float32)
                d[a], d[b] = sign * s, -sign * s
                qs.append(t + d)
    q = np.concatenate(qs).astype(np.float32)
    want = brute_knn(t, q, float(r), 32)
    with cloud.Cloud(t) as c:
        got = c.knn(q, float(r), 32, want_within=True)
        assert_knn_same(got, want, f"lattice + {shift}")
        assert_knn_same(c.knn(q, float(r), 5, want_within=True), first_k(want, 5), f"lattice + {shift}, k 5")
        assert_knn_same(c.knn_self(float(r), 8, want_within=True), brute_knn(t, None, float(r), 8), f"lattice + {shift}, self")
    d2, idx, within = got
    n = len(t)
    if shift == 0.0:
        # the boundary is inclusive: the lattice point a query was displaced from by exactly the radius along +-x (an exact sum
        # here) is a candidate at d2 == r2
        origin = np.arange(n)
        r2_bits = bits(r * r)[0]
        for block in (1, 7):                                  # steps[0], sign -1 and +1, axis 0
            rows = slice(block * n, (block + 1) * n)
            hit = idx[rows] == origin[:, None]
            assert hit.any(1).all() and (bits(d2[rows])[hit] == r2_bits).all()
        assert within[:n].max() == 7 and within[:n].min() == 4   # a lattice point as a query: itself and its 6 (a corner: 3) neighbours at the radius


def test_boundary_is_inclusive(cloud):
    """d2 == r2 is a candidate, one ulp beyond is not: every operand below is exact in fp32"""
    r = np.float32(0.25)
    up = np.nextafter(r, np.float32(1))
    t = np.array([[0, 0, 0], [r, 0, 0], [up, 0, 0], [0, -r, 0], [0, 0, -up], [0, r, 0]], np.float32)
    want = brute_knn(t, None, float(r), 4)
    assert want[1][0].tolist() == [1, 3, 5, -1] and want[2].tolist() == [3, 2, 1, 1, 0, 1] and (bits(want[0][0, :3]) == bits(r * r)[0]).all()
    with cloud.Cloud(t) as c:
        assert_knn_same(c.knn_self(float(r), 4, want_within=True), want, "boundary")
        q = np.array([[0, 0, 0]], np.float32)
        assert_knn_same(c.knn(q, float(r), 8, want_within=True), brute_knn(t, q, float(r), 8), "boundary, query")


def test_candidate_count_around_k(cloud):
    """clusters of m + 1 points far apart: every member has exactly m candidates"""
    rng = np.random.default_rng(12)
    sizes = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33)
    x = np.concatenate([np.array([100.0 * m, 0, 0]) + 0.01 * rng.random((m + 1, 3)) for m in sizes]).astype(np.float32)
    member = np.concatenate([np.full(m + 1, m) for m in sizes])
    with cloud.Cloud(x) as c:
        for k in (1, 4, 8, 16, 32):
            got = c.knn_self(0.05, k, want_within=True)
            assert_knn_same(got, brute_knn(x, None, 0.05, k), f"clusters, k {k}")
            assert np.array_equal(got[2], member)
            filled = np.isfinite(got[0]).sum(1)
            assert np.array_equal(filled, np.minimum(member, k))
            for m in (k - 1, k, k + 1):
                assert m in sizes                              # exactly k - 1, k and k + 1 candidates are among the cases


@pytest.mark.parametrize("n", [1, 257])
def test_small_counts(cloud, n):
    rng = np.random.default_rng(n)
    x = (rng.random((n, 3)) * 0.1 - 3.0).astype(np.float32)
    with cloud.Cloud(x) as c:
        for k in (1, 9, 32):
            assert_knn_same(c.knn_self(1.0 / 64.0, k, want_within=True), brute_knn(x, None, 1.0 / 64.0, k), f"n {n}, k {k}")
            assert_knn_same(c.knn(x[::-1].copy(), 0.05, k, want_within=True), brute_knn(x, x[::-1].copy(), 0.05, k), f"n {n}, k {k}, queries")


def test_70001_points_in_one_cell(cloud):
    rng = np.random.default_rng(6)
    n = 70001
    x = (5.0 + 0.01 * rng.random((n, 3))).astype(np.float32)
    rows = np.sort(rng.choice(n, 500, replace=False))
    rows[0], rows[-1] = 0, n - 1
    with cloud.Cloud(x) as c:
        d2, idx, within = c.knn_self(1.0, 32, want_within=True)
        assert c.stats()["fullest"] == n and c.stats()["cells"] == 1
    assert (within == n - 1).all()
    assert_knn_same((d2[rows], idx[rows], within[rows]), brute_knn(x, None, 1.0, 32, chunk=128, self_rows=rows), "one cell")


def test_more_queries_than_one_chunk(cloud):
    """the queries are served 2^23 / k at a time, 2^18 at k = 32: rows on both sides of the border, and the self-exclusion beyond
    it; at k = 2 the same queries fit one launch"""
    rng = np.random.default_rng(18)
    n = (1 << 18) + 300
    x = rng.random((n, 3)).astype(np.float32)
    x[(1 << 18) + 5] = x[3]                                  # twins across the border
    radius = 0.03                                            # about 30 candidates: full and padded rows
    rows = np.unique(np.concatenate([rng.choice(n, 300, replace=False), np.arange((1 << 18) - 20, (1 << 18) + 20), [3, n - 1]]))
    q = x[::-1].copy()
    want = brute_knn(x, None, radius, 32, chunk=64, self_rows=rows)
    wantq = brute_knn(x, q[rows], radius, 32, chunk=64)
    assert (want[2] < 32).any() and (want[2] > 32).any()
    with cloud.Cloud(x) as c:
        got = c.knn_self(radius, 32, want_within=True)
        assert_knn_same(tuple(a[rows] for a in got), want, "self across chunks")
        gotq = c.knn(q, radius, 32, want_within=True)
        assert_knn_same(tuple(a[rows] for a in gotq), wantq, "queries across chunks")
        assert_knn_same(tuple(a[rows] for a in c.knn_self(radius, 2, want_within=True)), first_k(want, 2), "self in one launch")
    assert got[1][3, 0] == (1 << 18) + 5 and got[1][(1 << 18) + 5, 0] == 3 and not got[0][[3, (1 << 18) + 5], 0].any()
    assert np.array_equal(gotq[1][:, 0], np.where(np.arange(n) == n - 1 - ((1 << 18) + 5), 3, np.arange(n)[::-1]))   # every point finds itself, the twin its elder


def test_argument_errors(cloud, engine):
    _, fns = engine.load()
    t = np.random.default_rng(1).random((50, 3)).astype(np.float32)
    d2 = np.full((50, 32), 7.0, np.float32)
    h = C.c_void_p(None)
    assert fns["cloud_create"](0, 50, t.ctypes.data, C.byref(h)) == 0
    try:
        for k in (0, 33, -1):
            assert fns["cloud_knn"](h, 0.1, k, 50, None, d2.ctypes.data, None, None) == -2, k
            assert "k must lie in [1, 32]" in fns["last_error"](None).decode()
        assert fns["cloud_knn"](h, 0.1, 4, 49, None, d2.ctypes.data, None, None) == -2        # NULL q_xyz with n_q != n
        assert fns["cloud_knn"](h, 0.1, 4, 0, None, d2.ctypes.data, None, None) == -2
        assert fns["cloud_knn"](h, 0.1, 4, -1, t.ctypes.data, d2.ctypes.data, None, None) == -2
        assert fns["cloud_knn"](h, 0.1, 4, 50, t.ctypes.data, None, None, None) == -2
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert fns["cloud_knn"](h, bad, 4, 50, None, d2.ctypes.data, None, None) == -2, bad
        assert fns["cloud_knn"](h, 0.1, 4, 2 ** 31, t.ctypes.data, d2.ctypes.data, None, None) == -3
        assert fns["cloud_knn"](h, 1e-8, 4, 50, None, d2.ctypes.data, None, None) == -3
        assert "2^21" in fns["last_error"](None).decode()
        assert fns["cloud_knn"](h, 0.1, 4, 0, t.ctypes.data, d2.ctypes.data, None, None) == 0   # n_q == 0 writes nothing
        assert (d2 == 7.0).all()
        assert fns["cloud_knn"](h, 0.1, 32, 50, None, d2.ctypes.data, None, None) == 0          # still usable
        assert np.array_equal(bits(d2), bits(brute_knn(t, None, 0.1, 32)[0]))
    finally:
        fns["cloud_destroy"](h)
    with cloud.Cloud(t) as c:
        for k in (0, 33):
            with pytest.raises(ValueError):
                c.knn_self(0.1, k)
        with pytest.raises(ValueError):
            c.knn(t, -1.0, 4)
    # a cloud without a finite point, and an empty one
    for empty in (np.full((4, 3), np.nan, np.float32), np.zeros((0, 3), np.float32)):
        with cloud.Cloud(empty) as c:
            d2e, idxe, we = c.knn(t, 0.5, 3, want_within=True)
            assert np.isposinf(d2e).all() and (idxe == -1).all() and not we.any() and d2e.shape == (50, 3)
            d2e, idxe, we = c.knn_self(0.5, 3, want_within=True)
            assert d2e.shape == (len(empty), 3) and np.isposinf(d2e).all() and (idxe == -1).all() and not we.any()


def test_handle_reuse_and_grid_cache(cloud, random_cloud):
    x, q = random_cloud
    with cloud.Cloud(x) as c:
        res, build = [], []
        for step, r in enumerate((0.05, 0.3, 0.05, 0.3)):
            if step == 1:
                near = c.nearest(q, r)                       # this call builds the grid of 0.3 ...
                assert c.kernel_ms()[1] > 0
            res.append(c.knn_self(r, 8, want_within=True))
            ms, b = c.knn_ms()
            assert ms > 0
            build.append(b)
        assert build[0] > 0 and build[1] == 0 and build[2] == 0 and build[3] == 0   # ... so no knn call builds it again
        c.nearest(q, 0.05)
        assert c.kernel_ms()[1] == 0                         # and nearest reuses the grid a knn call built
        assert_knn_same((near[0][:, None], near[1][:, None]), first_k(reference(x, q, 0.3), 1)[:2] + (None,), "nearest in between")
    for a, b in ((0, 2), (1, 3)):
        for u, v in zip(res[a], res[b]):
            assert u.tobytes() == v.tobytes()                # two runs: identical bytes
    assert_knn_same(res[0], first_k(reference(x, None, 0.05), 8), "reused handle, 0.05")
    assert_knn_same(res[1], first_k(reference(x, None, 0.3), 8), "reused handle, 0.3")


CALLER_ORDER_CHILD = """
import importlib, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
cloud = importlib.import_module("mp-mvs_amd.cloud")
z = np.load(sys.argv[2])
x, q = z["x"], z["q"]
out = {}
with cloud.Cloud(x) as c:
    for k in (1, 5, 16, 32):
        out[f"sd{k}"], out[f"si{k}"], out[f"sw{k}"] = c.knn_self(0.3, k, want_within=True)
        out[f"qd{k}"], out[f"qi{k}"], out[f"qw{k}"] = c.knn(q, 0.3, k, want_within=True)
for k in (4, 16):
    r = cloud.remove_outliers(x, 0.3, k, 2.0, 3)
    out.update({f"o{k}_{name}": r[name] for name in r})
np.savez(sys.argv[3], **out)
"""


def test_caller_order_in_a_child_process(random_cloud, tmp_path):
    """MPMVS_CLOUD_BIN=0 is read once per process: a child with the variable set serves the queries in caller order (no binning,
    order == NULL in both kernels) and must give the same bits"""
    import subprocess
    x, q = random_cloud
    x, q = x[:1500].copy(), q[:300].copy()
    np.savez(tmp_path / "in.npz", x=x, q=q)
    env = dict(os.environ, MPMVS_CLOUD_BIN="0")
    done = subprocess.run([sys.executable, "-c", CALLER_ORDER_CHILD, ROOT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], env=env,
                          capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    got = np.load(tmp_path / "out.npz")
    full_s, full_q = brute_knn(x, None, 0.3, 32), brute_knn(x, q, 0.3, 32)
    for k in (1, 5, 16, 32):
        assert_knn_same((got[f"sd{k}"], got[f"si{k}"], got[f"sw{k}"]), first_k(full_s, k), f"caller order, self, k {k}")
        assert_knn_same((got[f"qd{k}"], got[f"qi{k}"], got[f"qw{k}"]), first_k(full_q, k), f"caller order, queries, k {k}")
    for k in (4, 16):
        want = statement_outliers(x, 0.3, k, 2.0, 3)
        assert_outliers_same({name: got[f"o{k}_{name}"] for name in want}, want, f"caller order, filter, k {k}")


# ---- the filter --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius,k,std_ratio,min_within", [(0.3, 16, 2.0, 0), (0.3, 8, float("inf"), 30), (0.05, 1, 1.0, 2), (0.3, 32, 0.0, 0),
                                                            (0.001, 2, 2.0, 0)])
def test_remove_outliers_against_the_statement(cloud, random_cloud, radius, k, std_ratio, min_within):
    x, _ = random_cloud
    got = cloud.remove_outliers(x, radius, k, std_ratio, min_within)
    want = statement_outliers(x, radius, k, std_ratio, min_within)
    print(f"radius {radius} k {k}: counts {got['counts'].tolist()} stats {got['stats'].tolist()} device ms {cloud.last_outliers_ms():.3f}")
    assert_outliers_same(got, want, f"radius {radius}, k {k}")
    assert cloud.last_outliers_ms() > 0
    finite, dense, kept = want["counts"]
    assert finite == 4996
    if radius == 0.001:
        assert dense == 0 and kept == 0 and not want["stats"].any()       # c == 0: every point is isolated (a twin is one neighbour, k is 2)
        assert want["within"][24:300].all() and not want["within"][2000:].any()
    elif np.isinf(std_ratio):
        assert np.isposinf(want["stats"][2]) and 0 < kept < dense         # only the radius rule removes
        assert np.array_equal(want["keep"], np.isfinite(want["mean_dist"]) & (want["within"] >= min_within))
    else:
        assert 0 < kept < dense <= finite


def test_property_scene(cloud):
    x, plane = property_scene()
    want = statement_outliers(x, 0.05, 8, 2.0)
    got = cloud.remove_outliers(x, 0.05, k=8, std_ratio=2.0)
    for name, r in (("statement", want), ("device", got)):
        print(name, "plane kept", r["keep"][plane].mean(), "others kept", int(r["keep"][~plane].sum()))
        assert r["keep"][plane].mean() > 0.95 and r["keep"][~plane].sum() == 0
    assert_outliers_same(got, want, "property scene")


def test_two_host_threads(cloud, random_cloud):
    x, _ = random_cloud
    jobs = [(x, 0.3, 16, 2.0, 0), (x[::-1].copy(), 0.05, 4, 1.0, 3)]
    single = [cloud.remove_outliers(*j) for j in jobs]
    got, errors = [[], []], []

    def work(t):
        try:
            for _ in range(4):
                got[t].append(cloud.remove_outliers(*jobs[t]))
                assert cloud.last_outliers_ms() > 0.0
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
            for key in single[t]:
                assert r[key].tobytes() == single[t][key].tobytes(), (t, key)


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
    for j, name in enumerate("xyz"):
        rec[name] = xyz[:, j]
    if normals is not None:
        for j, name in enumerate(("nx", "ny", "nz")):
            rec[name] = normals[:, j]
    if colors is not None:
        for j, name in enumerate(("red", "green", "blue")):
            rec[name] = colors[:, j]
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


def test_clean_ply(cloud, tmp_path, capsys, monkeypatch):
    x, plane = property_scene()
    rng = np.random.default_rng(3)
    nr = rng.normal(size=x.shape).astype(np.float32)
    col = rng.integers(0, 256, x.shape, dtype=np.uint8)
    write_ply(tmp_path / "a.ply", x, nr, col)
    out = run_tool("clean_ply", capsys, monkeypatch, ["--input", tmp_path / "a.ply", "--output", tmp_path / "b.ply", "--radius", 0.05, "--k", 8])
    line = json.loads(out.strip().splitlines()[-1])
    want = statement_outliers(x, 0.05, 8, 2.0)
    keep = want["keep"]
    finite, dense, kept = (int(v) for v in want["counts"])
    assert (line["n"], line["kept"], line["isolated"], line["nonfinite"]) == (len(x), kept, finite - dense, 0) and line["device_ms"] > 0
    assert [line["mean"], line["sigma"], line["threshold"]] == want["stats"].tolist()
    data = open(tmp_path / "b.ply", "rb").read()
    body = data.index(b"\n", data.index(b"end_header")) + 1
    rec = np.zeros(kept, np.dtype([("p", "<f4", 3), ("n", "<f4", 3), ("c", "u1", 3)]))   # the reference's 27-byte records
    rec["p"], rec["n"], rec["c"] = x[keep], nr[keep], col[keep]
    assert rec.dtype.itemsize == 27 and data[body:] == rec.tobytes()
    back = cloud.read_ply(tmp_path / "b.ply")
    assert np.array_equal(bits(back["xyz"]), bits(x[keep])) and not (back["xyz"][:, 2] > 0.02).any()
    # positions only, the statistical test off and the radius rule on
    write_ply(tmp_path / "c.ply", x)
    out = run_tool("clean_ply", capsys, monkeypatch, ["--input", tmp_path / "c.ply", "--output", tmp_path / "d.ply", "--radius", 0.05, "--k", 4,
                                                     "--std_ratio", "inf", "--min_within", 20])
    line = json.loads(out.strip().splitlines()[-1])
    want = statement_outliers(x, 0.05, 4, float("inf"), 20)
    assert line["kept"] == int(want["counts"][2]) and line["threshold"] is None and 0 < line["kept"] < len(x)
    back = cloud.read_ply(tmp_path / "d.ply")
    assert np.array_equal(bits(back["xyz"]), bits(x[want["keep"]])) and not back["normals"].any() and not back["colors"].any()
