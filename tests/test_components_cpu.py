"""mpmvs_cloud_components without a GPU: the symbols, the refusals that need no handle, the empty results of the Python wrapper, its
ValueErrors, and the numpy statement of components_common.py against expectations written out by hand.  A handle cannot be made
without a device (mpmvs_cloud_create opens its stream first), so the refusals of a live handle -- the radius, the cell span -- and
its empty results are in test_components_gpu.py; here the NULL handle stands for them, as in test_knn_cpu.py."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

from components_common import adjacent_pairs, cluster_scene, statement_components, statement_small_clusters
from knn_common import statement_outliers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mpmvs_cloud_components", "mpmvs_cloud_components_ms")
BAD_DEVICE = 12345


@pytest.fixture(scope="module")
def eng(pm):
    return importlib.import_module("mp-mvs_amd.engine")


@pytest.fixture(scope="module")
def cloud(pm):
    return importlib.import_module("mp-mvs_amd.cloud")


def test_symbols_declared_exported_and_bound(eng):
    header = open(os.path.join(ROOT, "include", "mpmvs.h")).read()
    declared = set(re.findall(r"\b(mpmvs_[a-z0-9_]+)\s*\(", header))
    lib, fns = eng.load()
    lib_q8, fns_q8 = eng.load_variant(eng.LIB_Q8_PATH)
    for name in NEW + ("mpmvs_cloud_components_pass_ms",):
        assert name in declared and name in eng.ALL_SYMBOLS
        assert hasattr(lib, name) and hasattr(lib_q8, name)
        assert name[len("mpmvs_"):] in fns and name[len("mpmvs_"):] in fns_q8
    f = fns["cloud_components"]
    assert f.restype is C.c_int and f.argtypes == [C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.POINTER(C.c_longlong)]
    f = fns["cloud_components_ms"]
    assert f.restype is C.c_float and f.argtypes == [C.c_void_p, C.POINTER(C.c_float)]
    f = fns["cloud_components_pass_ms"]
    assert f.restype is C.c_int and f.argtypes == [C.c_void_p, C.POINTER(C.c_float)]
    # the library follows the header: the cloud unit includes it, and the objects depend on what they include (generated dependencies)
    csrc = os.path.join(ROOT, "mp-mvs_amd", "csrc")
    assert '#include "pm_components.hpp"' in open(os.path.join(csrc, "mpmvs_cloud.hip")).read()
    makefile = open(os.path.join(csrc, "Makefile")).read()
    assert "mpmvs_cloud" in makefile and "-MMD" in makefile and "-include $(OBJS:.o=.d)" in makefile
    assert os.path.exists(os.path.join(ROOT, "mp-mvs_amd", "csrc", "pm_components.hpp"))


def test_null_cloud_is_minus_2_and_writes_nothing(eng):
    _, fns = eng.load()
    label, size = np.full(4, 7, np.int32), np.full(4, 7, np.int32)
    counts = (C.c_longlong * 4)(7, 7, 7, 7)
    for radius in (0.1, 0.0, float("nan")):
        assert fns["cloud_components"](None, radius, label.ctypes.data, size.ctypes.data, counts) == -2
        assert "components" in fns["last_error"](None).decode()
    assert (label == 7).all() and (size == 7).all() and list(counts) == [7, 7, 7, 7]
    assert fns["cloud_components_ms"](None, None) == 0.0
    ms = (C.c_float * 3)(7.0, 7.0, 7.0)
    assert fns["cloud_components_pass_ms"](None, ms) == -2 and list(ms) == [7.0, 7.0, 7.0]


def test_empty_results_need_no_device(cloud):
    r = cloud.remove_small_clusters(np.zeros((0, 3), np.float32), 0.1, device=BAD_DEVICE)
    assert r["keep"].shape == (0,) and r["keep"].dtype == bool and r["label"].shape == (0,) and r["size"].shape == (0,)
    assert r["counts"].tolist() == [0, 0, 0, -1] and r["counts"].dtype == np.int64
    x = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan] * 3], np.float32)
    r = cloud.remove_small_clusters(x, 0.1, min_size=1, device=BAD_DEVICE)
    want = statement_small_clusters(x, 0.1, 1)
    assert set(r) == {"keep", "label", "size", "counts"}
    for key in want:
        assert r[key].dtype == want[key].dtype and np.array_equal(r[key], want[key]), key
    assert not r["keep"].any() and (r["label"] == -1).all() and not r["size"].any() and r["counts"].tolist() == [0, 0, 0, -1]
    assert cloud.last_clusters_ms() == 0.0
    with pytest.raises(RuntimeError):   # a finite point: only now is the device looked for
        cloud.remove_small_clusters(np.zeros((2, 3), np.float32), 0.1, device=BAD_DEVICE)


def test_wrapper_value_errors(cloud):
    x = np.zeros((2, 3), np.float32)
    for bad in ({"radius": -1.0}, {"radius": 0.0}, {"radius": float("nan")}, {"radius": float("inf")}, {"radius": 0.1, "min_size": 0},
                {"radius": 0.1, "min_size": -3}, {"radius": 0.1, "min_size": 2.5}, {"radius": 0.1, "largest": 0}, {"radius": 0.1, "largest": -1},
                {"radius": 0.1, "largest": 1.5}):
        with pytest.raises(ValueError):
            cloud.remove_small_clusters(x, device=BAD_DEVICE, **bad)
    with pytest.raises(ValueError):
        cloud.remove_small_clusters(np.zeros((2, 4), np.float32), 0.1, device=BAD_DEVICE)


def twelve():
    """two triangles, a duplicate pair, one NaN, and one bridge at exactly the radius 0.25 (all distances below are exact in fp32)"""
    return np.array([[10.0, 0.0, 0.0],      # 0  triangle A
                     [20.0, 0.0, 0.0],      # 1  triangle B
                     [10.125, 0.0, 0.0],    # 2  A
                     [np.nan, 0.0, 0.0],    # 3  takes no part
                     [20.0, 0.125, 0.0],    # 4  B
                     [10.0, 0.125, 0.0],    # 5  A
                     [30.0, 1.0, 1.0],      # 6  duplicate pair
                     [20.0, 0.0, 0.125],    # 7  B
                     [30.0, 1.0, 1.0],      # 8  duplicate of 6, adjacent at d2 = +0
                     [10.375, 0.0, 0.0],    # 9  the bridge: exactly 0.25 from 2, and 0.375 from 0
                     [40.0, 0.0, 0.0],      # 10 alone
                     [10.375, 0.2501, 0.0]  # 11 just beyond the radius from 9: alone
                     ], np.float32)


def test_statement_on_twelve_points_by_hand():
    x = twelve()
    i, j = adjacent_pairs(x, 0.25)
    assert sorted(zip(i.tolist(), j.tolist())) == [(2, 0), (4, 1), (5, 0), (5, 2), (7, 1), (7, 4), (8, 6), (9, 2)]
    label, size, counts = statement_components(x, 0.25)
    assert label.tolist() == [0, 1, 0, -1, 1, 0, 6, 1, 6, 0, 10, 11] and label.dtype == np.int32
    assert size.tolist() == [4, 3, 4, 0, 3, 4, 2, 3, 2, 4, 1, 1] and size.dtype == np.int32
    assert counts.tolist() == [11, 5, 4, 0] and counts.dtype == np.int64
    # one ulp below the bridge's distance: the bridge is a component of its own, and the triangles tie at 3 -- the smaller label wins
    label, size, counts = statement_components(x, np.nextafter(np.float32(0.25), np.float32(0)))
    assert label.tolist() == [0, 1, 0, -1, 1, 0, 6, 1, 6, 9, 10, 11] and counts.tolist() == [11, 6, 3, 0]
    # the keep rule
    r = statement_small_clusters(x, 0.25, min_size=2)
    assert r["keep"].tolist() == [True, True, True, False, True, True, True, True, True, True, False, False]
    r = statement_small_clusters(x, 0.25, min_size=1, largest=2)
    assert r["keep"].tolist() == [True, True, True, False, True, True, False, True, False, True, False, False]
    r = statement_small_clusters(x, 0.25, min_size=4, largest=3)
    assert np.flatnonzero(r["keep"]).tolist() == [0, 2, 5, 9]
    r = statement_small_clusters(x, 0.25, min_size=1, largest=4)       # the singletons 10 and 11 tie at size 1: 10 comes first
    assert np.flatnonzero(~r["keep"]).tolist() == [3, 11]


def test_wrapper_keep_rule_equals_the_statement(cloud):
    x = twelve()
    for radius in (0.25, 0.2, 50.0):
        label, size, _ = statement_components(x, radius)
        for min_size, largest in ((1, None), (2, None), (3, 1), (1, 2), (1, 4), (4, 3), (1, 100)):
            want = statement_small_clusters(x, radius, min_size, largest)["keep"]
            assert np.array_equal(cloud.cluster_keep(label, size, min_size, largest), want), (radius, min_size, largest)


def test_property_scene_shows_why():
    """the cluster filter removes the detached blobs and keeps the surface; the outlier rules at the tool's defaults keep the blobs"""
    x, plane, blob = cluster_scene()
    got = statement_small_clusters(x, 0.02, min_size=100)
    print("clusters: plane kept", got["keep"][plane].mean(), "blob points kept", int(got["keep"][blob].sum()), "components", got["counts"].tolist())
    assert got["keep"][plane].mean() > 0.95 and got["keep"][blob].sum() == 0
    out = statement_outliers(x, 0.05, 16, 2.0, 0)
    print("outliers: plane kept", out["keep"][plane].mean(), "blob points kept", int(out["keep"][blob].sum()), "of", int(blob.sum()))
    assert out["keep"][blob].mean() > 0.5
