"""mpmvs_cloud_components on the GPU against the numpy statement of components_common.py (include/mpmvs.h),
cloud.remove_small_clusters against its statement, and tools/clean_ply.py with the cluster flags end to end.  Every comparison is
array_equal: the result is a pure function of the point set."""
import ctypes as C
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from components_common import assert_components_same, cluster_scene, statement_components, statement_small_clusters
from knn_common import bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADII = (0.04, 0.055, 0.065, 0.09)


@pytest.fixture(scope="module")
def cloud(engine):
    return importlib.import_module("mp-mvs_amd.cloud")


def random_cloud(kind="plain"):
    """3 000 points in a unit cube at 100: below percolation at 0.04 and 0.055, above it at 0.065 and 0.09.  "nonfinite": 5 % of the
    rows NaN / +-inf; "duplicates": 300 rows copied onto 300 others"""
    x = (np.random.default_rng(17).random((3000, 3)) + 100).astype(np.float32)
    rng = np.random.default_rng(29)
    if kind == "nonfinite":
        rows = np.concatenate([[0], 1 + rng.choice(2999, 149, replace=False)])   # the smallest index takes no part
        x[rows, rng.integers(0, 3, 150)] = np.array([np.nan, np.inf, -np.inf], np.float32)[rng.integers(0, 3, 150)]
    elif kind == "duplicates":
        rows = rng.choice(3000, 600, replace=False)
        x[rows[:300]] = x[rows[300:]]
    elif kind == "permuted":
        x = x[rng.permutation(3000)]
    return x


_REF = {}


def reference(kind, radius):
    """the statement, computed once per cloud and radius and left unchanged"""
    key = (kind, radius)
    if key not in _REF:
        _REF[key] = statement_components(random_cloud(kind), radius)
        for a in _REF[key]:
            a.setflags(write=False)
    return _REF[key]


def component_sizes(ref):
    label, size, _ = ref
    return size[np.flatnonzero(label == np.arange(len(label)))]


# ---- the chain: the deepest trees and the longest hooking sequences ------------------------------------------------------------
@pytest.mark.parametrize("shift", [0.0, 1000.25])
@pytest.mark.parametrize("order", ["ascending", "descending", "scrambled"])
def test_chain(cloud, order, shift):
    n, step = 4096, np.float32(257.0 / 1024.0)
    pos = np.float32(shift) + np.arange(n, dtype=np.float32) * step
    assert np.array_equal(pos.astype(np.float64), shift + np.arange(n) * (257.0 / 1024.0))          # exact in fp32
    assert (np.diff(pos) == step).all()
    at = {"ascending": np.arange(n), "descending": np.arange(n)[::-1], "scrambled": np.random.default_rng(3).permutation(n)}[order]
    x = np.zeros((n, 3), np.float32)
    x[:, 0] = pos[at]
    with cloud.Cloud(x) as c:
        label, size, counts = c.components(float(step))            # neighbours at exactly the radius: one component
        assert np.array_equal(label, np.zeros(n, np.int32)) and np.array_equal(size, np.full(n, n, np.int32)) and counts.tolist() == [n, 1, n, 0]
        label, size, counts = c.components(0.25)                    # just below the spacing: nobody has a neighbour
        assert np.array_equal(label, np.arange(n, dtype=np.int32)) and np.array_equal(size, np.ones(n, np.int32)) and counts.tolist() == [n, n, 1, 0]
    if order == "scrambled" and shift:
        assert_components_same((label, size, counts), statement_components(x, 0.25), "chain, singletons")
        assert statement_components(x, float(step))[2].tolist() == [n, 1, n, 0]


# ---- the bridge: one pair across two blobs, at exactly the radius and one ulp beyond ------------------------------------------------
@pytest.mark.parametrize("apart", [False, True])
def test_bridge(cloud, apart):
    rng = np.random.default_rng(11)
    r = np.float32(0.25)
    gap = np.nextafter(r, np.float32(1)) if apart else r
    left = np.array([-0.1, 0, 0]) - rng.random((199, 3)) * [0.3, 0.3, 0.3]          # all x <= -0.1: more than the radius from the pair's right end
    right = np.array([float(gap) + 0.1, 0, 0]) + rng.random((199, 3)) * [0.3, 0.3, 0.3]
    x = np.concatenate([left, [[0, 0, 0]], right, [[gap, 0, 0]]]).astype(np.float32)   # 200 points each; gap - 0 is exact
    x = x[rng.permutation(len(x))]
    want = statement_components(x, 0.25)
    assert want[2].tolist()[:3] == ([400, 2, 200] if apart else [400, 1, 400])      # checked on the CPU: the pair alone joins the blobs
    with cloud.Cloud(x) as c:
        assert_components_same(c.components(0.25), want, "bridge")


# ---- a random cloud on both sides of percolation ---------------------------------------------------------------------------------
def test_the_random_cloud_is_what_it_should_be():
    """the scene cannot quietly degenerate: counts found on the CPU (a k-d tree in fp64 agrees)"""
    sizes = component_sizes(reference("plain", 0.04))
    assert (int((sizes == 1).sum()), int((sizes >= 2).sum()), int(sizes.max())) == (1383, 566, 12)
    sizes = component_sizes(reference("plain", 0.055))
    assert (sizes >= 2).sum() >= 100 and (sizes >= 50).sum() >= 1
    assert (int((sizes >= 2).sum()), int(sizes.max())) == (419, 100)
    assert component_sizes(reference("plain", 0.065)).max() == 2257 and component_sizes(reference("plain", 0.09)).max() == 2994


@pytest.mark.parametrize("kind", ["plain", "nonfinite", "duplicates"])
def test_random_cloud(cloud, kind):
    x = random_cloud(kind)
    with cloud.Cloud(x) as c:
        for radius in RADII:
            got = c.components(radius)
            assert_components_same(got, reference(kind, radius), f"{kind} cloud at {radius}")
            assert c.components_ms()[0] > 0
    if kind == "nonfinite":
        bad = ~np.isfinite(x).all(1)
        assert bad.sum() == 150 and (got[0][bad] == -1).all() and (got[1][bad] == 0).all() and got[2][0] == 2850 and (got[0][~bad] > 0).all()
    if kind == "duplicates":
        assert component_sizes(reference(kind, 0.04)).min() == 1 and (reference(kind, 0.04)[1] >= 2).sum() > (reference("plain", 0.04)[1] >= 2).sum()


def test_scheduling_independence(cloud):
    x = random_cloud("permuted")
    with cloud.Cloud(x) as c:
        for radius in (0.055, 0.065):
            a = c.components(radius)
            b = c.components(radius)
            assert all(u.tobytes() == v.tobytes() for u, v in zip(a, b))                # two runs: identical bytes
            assert_components_same(a, reference("permuted", radius), f"permuted cloud at {radius}")
    # the same point set in another order: the same partition, named by the new indices
    sizes_a, sizes_b = component_sizes(reference("permuted", 0.055)), component_sizes(reference("plain", 0.055))
    assert np.array_equal(np.sort(sizes_a), np.sort(sizes_b))


def test_contention_8193_duplicates_in_one_cell(cloud):
    n = 8193
    x = np.tile(np.array([[5.0, -6.5, 7.25]], np.float32), (n, 1))
    with cloud.Cloud(x) as c:
        label, size, counts = c.components(0.5)
        assert c.stats()["cells"] == 1 and c.stats()["fullest"] == n
    assert not label.any() and (size == n).all() and counts.tolist() == [n, 1, n, 0]


def test_grid_cache_and_null_outputs(cloud, engine):
    x = random_cloud("plain")
    _, fns = engine.load()
    with cloud.Cloud(x) as c:
        c.knn_self(0.055, 1)                                        # builds the grid of 0.055 ...
        assert c.knn_ms()[1] > 0
        got = c.components(0.055)
        ms, build, passes = c.components_ms(passes=True)
        assert build == 0 and ms > 0 and passes["hook"] > 0 and passes["flatten"] > 0 and passes["size"] > 0   # ... and components reuses it
        assert_components_same(got, reference("plain", 0.055), "after knn_self")
        c.components(0.065)
        assert c.components_ms()[1] > 0                             # another radius builds its own
        c.nearest(x[:10], 0.065)
        assert c.kernel_ms()[1] == 0                                # and nearest reuses the grid a components call built
        # out_size = NULL and counts = NULL are legal
        label = np.full(len(x), 7, np.int32)
        assert fns["cloud_components"](c._h, 0.055, label.ctypes.data, None, None) == 0
        assert np.array_equal(label, reference("plain", 0.055)[0]) and c.components_ms(passes=True)[2]["size"] == 0
        label2, none, counts = c.components(0.055, want_size=False)
        assert none is None and np.array_equal(label2, label) and np.array_equal(counts, reference("plain", 0.055)[2])


def test_argument_errors_and_empty_results(cloud, engine):
    x = random_cloud("plain")
    _, fns = engine.load()
    label, size = np.full(len(x), 7, np.int32), np.full(len(x), 7, np.int32)
    counts = (C.c_longlong * 4)(7, 7, 7, 7)

    def untouched():
        return (label == 7).all() and (size == 7).all() and list(counts) == [7, 7, 7, 7]

    with cloud.Cloud(x) as c:
        for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
            assert fns["cloud_components"](c._h, bad, label.ctypes.data, size.ctypes.data, counts) == -2, bad
            assert "radius" in fns["last_error"](None).decode()
        assert fns["cloud_components"](c._h, 0.1, None, size.ctypes.data, counts) == -2     # NULL out_label with n > 0
        assert fns["cloud_components"](c._h, 1e-8, label.ctypes.data, size.ctypes.data, counts) == -3
        text = fns["last_error"](None).decode()
        assert "along " in text and "2^21" in text and "extent / radius = " in text, text
        assert untouched()                                           # a refused call writes nothing
        with pytest.raises(ValueError):
            c.components(-1.0)
        with pytest.raises(ValueError):
            c.components(1e-8)
        assert_components_same(c.components(0.09), reference("plain", 0.09), "still usable")
    # no point takes part: answered on the host
    for pts in (np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]], np.float32), np.zeros((0, 3), np.float32)):
        with cloud.Cloud(pts) as c:
            lab, siz, cnt = c.components(0.1)
            assert (lab == -1).all() and not siz.any() and lab.shape == (len(pts),) and cnt.tolist() == [0, 0, 0, -1]
            assert c.components_ms(passes=True) == (0.0, 0.0, {"hook": 0.0, "flatten": 0.0, "size": 0.0})
            assert fns["cloud_components"](c._h, 0.0, lab.ctypes.data, None, None) == -2
    with cloud.Cloud(np.zeros((0, 3), np.float32)) as c:
        assert fns["cloud_components"](c._h, 0.1, None, None, None) == 0                    # n == 0: nothing to write into


# ---- the filter on top -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_size,largest", [(1, None), (2, None), (5, None), (101, None), (1, 1), (2, 3), (1, 400), (1, 5000), (50, 2)])
def test_remove_small_clusters_against_the_statement(cloud, min_size, largest):
    x = random_cloud("plain")
    want = statement_small_clusters(x, 0.055, min_size, largest)
    got = cloud.remove_small_clusters(x, 0.055, min_size, largest)
    assert set(got) == set(want) and got["keep"].dtype == bool
    for key in want:
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key
    assert cloud.last_clusters_ms() > 0
    if (min_size, largest) == (101, None):
        assert not got["keep"].any()
    if (min_size, largest) == (1, 1):
        assert got["keep"].sum() == 100


def test_property_scene(cloud):
    x, plane, blob = cluster_scene()
    got = cloud.remove_small_clusters(x, 0.02, min_size=100)
    want = statement_small_clusters(x, 0.02, 100)
    assert all(np.array_equal(got[k], want[k]) for k in want)
    assert got["keep"][plane].mean() > 0.95 and got["keep"][blob].sum() == 0


# ---- tools/clean_ply.py as a fresh child process --------------------------------------------------------------------------------------
def write_ply(path, xyz):
    rec = np.zeros(len(xyz), np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")]))
    for j, name in enumerate("xyz"):
        rec[name] = xyz[:, j]
    with open(path, "wb") as fh:
        fh.write(f"ply\nformat binary_little_endian 1.0\nelement vertex {len(xyz)}\nproperty float x\nproperty float y\nproperty float z\nend_header\n".encode())
        fh.write(rec.tobytes())


def run_clean_ply(*args):
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "clean_ply.py")] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    return json.loads(done.stdout.strip().splitlines()[-1])


def test_clean_ply_with_and_without_the_cluster_flags(cloud, tmp_path):
    x, plane, blob = cluster_scene()
    write_ply(tmp_path / "a.ply", x)
    outliers = cloud.remove_outliers(x, 0.05, k=8)
    first = outliers["keep"]
    assert first[blob].sum() > 60                                   # the outlier filter keeps most of the blobs ...
    # without the flags: what the outlier filter alone gives, byte for byte, and the JSON keys of before
    line = run_clean_ply("--input", tmp_path / "a.ply", "--output", tmp_path / "plain.ply", "--radius", 0.05, "--k", 8)
    cloud.write_ply(tmp_path / "want_plain.ply", x[first])
    assert open(tmp_path / "plain.ply", "rb").read() == open(tmp_path / "want_plain.ply", "rb").read()
    assert set(line) == {"n", "kept", "isolated", "nonfinite", "mean", "sigma", "threshold", "radius", "k", "std_ratio", "min_within", "device_ms", "seconds"}
    assert line["kept"] == int(first.sum())
    # with them: the cluster filter after the outlier filter, on the points that filter kept; the blobs of 40 pass --min_cluster 30 and fall to --largest 1
    line = run_clean_ply("--input", tmp_path / "a.ply", "--output", tmp_path / "b.ply", "--radius", 0.05, "--k", 8, "--cluster_radius", 0.02,
                         "--min_cluster", 30, "--largest", 1)
    at = np.flatnonzero(first)
    want = statement_small_clusters(x[at], 0.02, 30, 1)
    assert statement_small_clusters(x[at], 0.02, 30)["keep"][blob[at]].sum() > 60
    keep = first.copy()
    keep[at] = want["keep"]
    back = cloud.read_ply(tmp_path / "b.ply")
    assert np.array_equal(bits(back["xyz"]), bits(x[keep])) and not keep[blob].any() and keep[plane].mean() > 0.95   # ... and the cluster filter drops them
    assert line["kept"] == int(keep.sum()) == line["largest_cluster"] and line["clusters"] == int(want["counts"][1])
    assert line["removed_by_cluster"] == int(first.sum() - keep.sum()) > 0 and line["cluster_device_ms"] > 0
