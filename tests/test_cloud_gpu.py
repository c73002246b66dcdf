"""mpmvs_cloud_* on the GPU against the brute-force statement (tests/cloud_common.py): array_equal on the d2 bits and on idx."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

from cloud_common import assert_same, bits, brute_nearest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cloud_nn_golden_v1.npz")


@pytest.fixture(scope="module")
def cloud(engine):
    return importlib.import_module("mp-mvs_amd.cloud")


def check(cloud, t, q, radius):
    with cloud.Cloud(t) as c:
        got = c.nearest(q, radius)
        st = c.stats()
    want = brute_nearest(t, q, radius)
    assert_same(got, want)
    assert np.array_equal(got[1] == -1, np.isinf(got[0]))
    return got, st


@pytest.mark.parametrize("radius", [0.02, 0.2, 4.0])
def test_random(cloud, radius):
    rng = np.random.default_rng(11)
    t = rng.random((1500, 3), dtype=np.float32)
    q = rng.random((1000, 3), dtype=np.float32)
    (d2, idx), st = check(cloud, t, q, radius)
    assert st["finite"] == 1500 and st["slots"] == 4096
    if radius == 4.0:
        assert st["cells"] <= 8 and np.isfinite(d2).all()
    if radius == 0.02:
        assert 0 < np.isinf(d2).sum() < len(q)


@pytest.mark.parametrize("n_q", [1, 256, 257, 513])
def test_query_counts_around_the_bin_floor(cloud, n_q):
    """the queries are binned into max(2^8, the power of two >= n_q) bins: one query, the floor itself, one above it (2^9 bins) and
    one power further (2^10); some queries without a cell, which go to bin 0"""
    rng = np.random.default_rng(100 + n_q)
    t = rng.random((300, 3), dtype=np.float32)
    q = rng.random((n_q, 3), dtype=np.float32)
    bad = [np.nan, np.inf, -np.inf]
    for j, i in enumerate(range(3, n_q, 50)):
        q[i, j % 3] = bad[j % 3]
    for radius in (0.05, 0.3):
        (d2, idx), st = check(cloud, t, q, radius)
        assert st["finite"] == 300
        assert np.isinf(d2[3::50]).all() and (idx[3::50] == -1).all()
    assert np.isfinite(d2).sum() == n_q - len(range(3, n_q, 50))   # at 0.3 every finite query has a candidate among 300 in the unit cube


@pytest.mark.parametrize("shift", [0.0, 1000.25])
def test_lattice_cell_borders(cloud, shift):
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
    (d2, idx), _ = check(cloud, t, q, float(r))
    n = len(t)
    assert np.array_equal(idx[:n], np.arange(n)) and not d2[:n].any()
    if shift == 0.0:
        # a query displaced by exactly the radius along one axis finds its origin (d2 == r2) unless a lattice neighbour is nearer
        assert (d2[n:2 * n] <= r * r).all()


def test_ties_and_duplicates(cloud):
    rng = np.random.default_rng(5)
    base = rng.random((300, 3), dtype=np.float32)
    t = np.concatenate([base, base[rng.choice(300, 100, replace=False)]])
    t = t[rng.permutation(400)]
    mid = ((t[:200] + t[200:]) * np.float32(0.5)).astype(np.float32)
    q = np.concatenate([t, mid])
    radius = 0.6
    (d2, idx), _ = check(cloud, t, q, radius)
    assert not d2[:400].any()
    # the duplicated positions answer with the smaller of the two indices
    first = np.array([np.flatnonzero((t == p).all(1))[0] for p in t])
    assert np.array_equal(idx[:400], first) and (first < np.arange(400)).sum() == 100
    perm = rng.permutation(400)
    t2 = t[perm]                       # t2[k] = t[perm[k]]
    with cloud.Cloud(t2) as c:
        d2b, idxb = c.nearest(q, radius)
    assert np.array_equal(bits(d2b), bits(d2))
    assert_same((d2b, idxb), brute_nearest(t2, q, radius))
    # at the duplicated positions either order answers with the same point, at the smallest index it has in that order
    assert np.array_equal(bits(t2[idxb[:400]]), bits(t[idx[:400]]))
    first2 = np.array([np.flatnonzero((t2 == p).all(1))[0] for p in t])
    assert np.array_equal(idxb[:400], first2)


def test_many_cells(cloud):
    rng = np.random.default_rng(3)
    radius = 0.01
    side = 42                                   # 42^3 = 74088 >= 70000 lattice sites
    sites = rng.permutation(side ** 3)[:70000]
    ijk = np.stack(np.unravel_index(sites, (side, side, side)), 1).astype(np.float64)
    # spacing 3 cell edges, jitter below a tenth of a radius: wherever the grid's origin falls, no two points share a cell
    t = ((ijk * 3 + 0.5) * radius * (1 + 2.0 ** -10) + rng.uniform(-0.1, 0.1, ijk.shape) * radius).astype(np.float32)
    q = (t[rng.integers(0, len(t), 2000)] + rng.normal(0, 0.6 * radius, (2000, 3))).astype(np.float32)
    (d2, idx), st = check(cloud, t, q, radius)
    assert st["cells"] == 70000 and st["fullest"] == 1 and st["slots"] == 1 << 18
    assert 100 < np.isfinite(d2).sum() < 2000


def test_one_full_cell(cloud):
    rng = np.random.default_rng(8)
    radius = 0.5
    v = rng.normal(size=(5000, 3))
    v *= (0.45 * radius * rng.random(5000) ** (1 / 3) / np.linalg.norm(v, axis=1))[:, None]
    far = rng.uniform(-3, 3, (50, 3))
    far[0] = -3                                                   # the grid's origin: the minimum of the bounding box
    centre = -3 + 6.5 * radius * (1 + 2.0 ** -10) * np.ones(3)    # the middle of cell (6, 6, 6); the ball's radius is 0.45 of the edge
    t = np.concatenate([centre + v, far]).astype(np.float32)
    q = np.concatenate([centre + rng.normal(0, 0.3 * radius, (200, 3)), centre + rng.normal(0, 1.5 * radius, (100, 3))]).astype(np.float32)
    _, st = check(cloud, t, q, radius)
    assert st["fullest"] >= 5000


def test_nonfinite_and_empty(cloud, engine):
    rng = np.random.default_rng(2)
    t = rng.random((200, 3), dtype=np.float32)
    t[3, 0] = np.nan
    t[10, 1] = np.inf
    t[11, 2] = -np.inf
    t[50] = np.nan
    q = rng.random((100, 3), dtype=np.float32)
    q[5, 2] = np.nan
    q[6, 0] = np.inf
    q[7, 1] = -np.inf
    (d2, idx), st = check(cloud, t, q, 0.5)
    assert st["finite"] == 196
    assert not np.isin(idx, [3, 10, 11, 50]).any()
    assert np.isinf(d2[5:8]).all() and (idx[5:8] == -1).all() and np.isfinite(np.delete(d2, [5, 6, 7])).all()
    # out_idx == NULL
    with cloud.Cloud(t) as c:
        d2n, none = c.nearest(q, 0.5, want_idx=False)
    assert none is None and np.array_equal(bits(d2n), bits(d2))
    # n == 0, and a cloud without a finite point
    for empty in (np.zeros((0, 3), np.float32), np.full((4, 3), np.nan, np.float32)):
        with cloud.Cloud(empty) as c:
            d2e, idxe = c.nearest(q, 0.5)
            assert np.isinf(d2e).all() and (idxe == -1).all() and c.stats()["finite"] == 0
    # n_q == 0 returns 0 and touches no output
    _, fns = engine.load()
    h = C.c_void_p(None)
    assert fns["cloud_create"](0, len(t), t.ctypes.data, C.byref(h)) == 0
    try:
        d2s = np.full(4, 7.0, np.float32)
        idxs = np.full(4, 7, np.int32)
        assert fns["cloud_nearest"](h, 0.5, 0, None, d2s.ctypes.data, idxs.ctypes.data) == 0
        assert (d2s == 7.0).all() and (idxs == 7).all()
    finally:
        fns["cloud_destroy"](h)


def test_errors(cloud, engine):
    _, fns = engine.load()
    t = np.array([[0, 0, 0], [0, 1e6, 0]], np.float32)
    q = np.array([[0, 0.05, 0], [0, 1e6, 0.01], [5, 5, 5]], np.float32)
    d2 = np.empty(3, np.float32)
    idx = np.empty(3, np.int32)
    h = C.c_void_p(None)
    assert fns["cloud_create"](0, 2, t.ctypes.data, C.byref(h)) == 0
    try:
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert fns["cloud_nearest"](h, bad, 3, q.ctypes.data, d2.ctypes.data, idx.ctypes.data) == -2, bad
        assert fns["cloud_nearest"](h, 0.1, 3, q.ctypes.data, None, idx.ctypes.data) == -2
        assert fns["cloud_nearest"](h, 0.1, -1, q.ctypes.data, d2.ctypes.data, idx.ctypes.data) == -2
        assert fns["cloud_nearest"](h, 0.1, 3, None, d2.ctypes.data, idx.ctypes.data) == -2
        assert fns["cloud_nearest"](None, 0.1, 3, q.ctypes.data, d2.ctypes.data, idx.ctypes.data) == -2
        assert fns["cloud_nearest"](h, 0.1, 2 ** 31, q.ctypes.data, d2.ctypes.data, idx.ctypes.data) == -3
        assert fns["cloud_nearest"](h, 0.1, 3, q.ctypes.data, d2.ctypes.data, idx.ctypes.data) == -3
        msg = fns["last_error"](None).decode()
        assert "along y" in msg and "2^21" in msg, msg
        # still usable
        assert fns["cloud_nearest"](h, 1000.0, 3, q.ctypes.data, d2.ctypes.data, idx.ctypes.data) == 0
        assert_same((d2, idx), brute_nearest(t, q, 1000.0))
        assert idx.tolist() == [0, 1, 0]
    finally:
        fns["cloud_destroy"](h)
    h = C.c_void_p(12345)
    assert fns["cloud_create"](0, 2, None, C.byref(h)) == -2 and not h.value
    assert fns["cloud_create"](0, -1, t.ctypes.data, C.byref(h)) == -2
    assert fns["cloud_create"](0, 2 ** 31, t.ctypes.data, C.byref(h)) == -3
    h = C.c_void_p(12345)
    assert fns["cloud_create"](4096, 2, t.ctypes.data, C.byref(h)) == -100 and not h.value
    with pytest.raises(ValueError):
        with cloud.Cloud(t) as c:
            c.nearest(q, 0.1)
    # the calls after a refused device still work
    with cloud.Cloud(t) as c:
        assert c.nearest(q, 1000.0)[1].tolist() == [0, 1, 0]


def test_handle_reuse(cloud):
    rng = np.random.default_rng(21)
    t = rng.random((3000, 3), dtype=np.float32)
    q = rng.random((800, 3), dtype=np.float32)
    with cloud.Cloud(t) as c:
        res, build = [], []
        for r in (0.1, 0.3, 0.1):
            res.append(c.nearest(q, r))
            build.append(c.kernel_ms()[1])
    assert build[0] > 0 and build[1] > 0 and build[2] == 0
    for r, got in zip((0.1, 0.3, 0.1), res):
        with cloud.Cloud(t) as fresh:
            assert_same(got, fresh.nearest(q, r))
    assert_same(res[0], brute_nearest(t, q, 0.1))
    assert_same(res[1], brute_nearest(t, q, 0.3))


def test_cascade_and_metrics(cloud):
    g = np.arange(60, dtype=np.float64) * 0.01
    gt = np.stack(list(np.meshgrid(g, g, indexing="ij")) + [np.zeros((60, 60))], -1).reshape(-1, 3).astype(np.float32)
    rng = np.random.default_rng(4)
    out = (rng.uniform(5, 9, (72, 3)) * rng.choice([-1, 1], (72, 3))).astype(np.float32)
    rec = np.concatenate([gt + np.array([0, 0, 0.004], np.float32), out]).astype(np.float32)
    tol = [0.002, 0.005, 0.02]
    res = cloud.evaluate(rec, gt, tol)
    acc = [r["accuracy"] for r in res["tolerances"]]
    com = [r["completeness"] for r in res["tolerances"]]
    assert acc == [0, 3600 / 3672, 3600 / 3672] and com == [0, 1, 1]
    assert res["tolerances"][0]["f1"] == 0 and res["n_reconstruction"] == 3672 and res["n_ground_truth"] == 3600
    a, c = 3600 / 3672, 1.0
    assert res["tolerances"][1]["f1"] == 2 * a * c / (a + c)
    assert res["reconstruction_to_ground_truth"]["resolved"] == 3600
    assert abs(res["ground_truth_to_reconstruction"]["median"] - 0.004) < 1e-6
    # distances == brute force capped at the largest tolerance, both ways (unordered tolerances: the cascade sorts them)
    for qs, ts in ((rec, gt), (gt, rec)):
        with cloud.Cloud(ts) as c_t:
            d = cloud.distances(qs, c_t, [0.02, 0.002, 0.005])
        bd2, bidx = brute_nearest(ts, qs, 0.02)
        assert np.array_equal(bits(d), bits(np.sqrt(bd2)))
    # nearest partners are unique here: point k of the lattice pairs with point k of the displaced lattice
    with cloud.Cloud(gt) as c_t:
        assert np.array_equal(c_t.nearest(rec[:3600], 0.005)[1], np.arange(3600))


def test_independent_fixture(cloud):
    z = np.load(GOLDEN)
    t, q, dist = z["targets"], z["queries"], z["distance"]
    assert t.dtype == np.float32 and q.dtype == np.float32 and dist.dtype == np.float64
    big = float(max(np.abs(t).max(), np.abs(q).max()))
    for radius in z["radii"]:
        radius = float(radius)
        with cloud.Cloud(t) as c:
            d2, idx = c.nearest(q, radius)
        inside = dist < radius * (1 - 1e-5)
        outside = dist > radius * (1 + 1e-5)
        assert (inside | outside).all()          # the generator checked that the band is empty: no case is left out
        assert inside.any() and outside.any()
        err = np.abs(np.sqrt(d2[inside].astype(np.float64)) - dist[inside])
        print(f"radius {radius}: max error {err.max():.3e}, bound {4e-6 * (big + radius):.3e}")
        assert (err <= 4e-6 * (big + radius)).all()
        assert np.isinf(d2[outside]).all() and (idx[outside] == -1).all()
        # the index is that of a point at the returned distance
        dd = np.linalg.norm(q[inside].astype(np.float64) - t[idx[inside]].astype(np.float64), axis=1)
        assert (np.abs(dd - dist[inside]) <= 4e-6 * (big + radius)).all()
