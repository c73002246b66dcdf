"""The host half of the cloud score (mp-mvs_amd/cloud.py): PLY reading, the metric arithmetic and the tests' own brute force.
No GPU."""
import importlib

import numpy as np
import pytest

from cloud_common import brute_nearest


@pytest.fixture(scope="module")
def cloud(pm):
    return importlib.import_module("mp-mvs_amd.cloud")


def test_read_ply_round_trip(cloud, hostlib, tmp_path):
    rng = np.random.default_rng(1)
    pts = np.empty((1000, 9), np.float32)
    pts[:, :3] = rng.normal(0, 50, (1000, 3))
    n = rng.normal(size=(1000, 3))
    pts[:, 3:6] = n / np.linalg.norm(n, axis=1, keepdims=True)
    pts[:, 6:] = rng.integers(0, 256, (1000, 3))
    path = tmp_path / "model.ply"
    hostlib.write_ply(path, pts)
    assert path.stat().st_size - path.read_bytes().index(b"end_header\n") - len(b"end_header\n") == 27 * 1000
    got = cloud.read_ply(path)
    assert got["xyz"].dtype == np.float32 and got["normals"].dtype == np.float32 and got["colors"].dtype == np.uint8
    assert got["xyz"].tobytes() == pts[:, :3].tobytes()
    assert got["normals"].tobytes() == pts[:, 3:6].tobytes()
    # points9 carries the colour as B, G, R (the reference's cv::Vec3b); the file's properties are red, green, blue
    assert np.array_equal(got["colors"], pts[:, [8, 7, 6]].astype(np.uint8))


ASCII_PLY = """ply
format ascii 1.0
comment written by hand
element vertex 3
property float x
property float y
property double quality
property float z
property uchar red
property uchar green
property uchar blue
element face 2
property list uchar int vertex_indices
element edge 1
property int a
property int b
end_header
0 0.5 9.25 1 255 0 7
-1.5 2 8 3e2 1 2 3
4 5 7 6 10 20 30
3 0 1 2
4 0 1 2 0
0 1
"""


def test_read_ply_ascii_with_extras(cloud, tmp_path):
    path = tmp_path / "a.ply"
    path.write_text(ASCII_PLY)
    got = cloud.read_ply(path)
    assert np.array_equal(got["xyz"], np.array([[0, 0.5, 1], [-1.5, 2, 300], [4, 5, 6]], np.float32))
    assert np.array_equal(got["colors"], np.array([[255, 0, 7], [1, 2, 3], [10, 20, 30]], np.uint8))
    assert "normals" not in got


def _binary_ply(header_extra_elem_first, body):
    return b"ply\nformat binary_little_endian 1.0\n" + header_extra_elem_first + b"end_header\n" + body


def test_read_ply_binary_skips_other_elements(cloud, tmp_path):
    # a list element BEFORE the vertices has to be walked entry by entry; an extra vertex property is skipped by its size
    head = (b"element tag 2\nproperty list uchar short v\nproperty uchar k\n"
            b"element vertex 2\nproperty float x\nproperty ushort extra\nproperty float y\nproperty float z\n")
    tags = bytes([2]) + np.array([5, 6], "<i2").tobytes() + bytes([9]) + bytes([0]) + bytes([8])
    rec = np.zeros(2, np.dtype([("x", "<f4"), ("e", "<u2"), ("y", "<f4"), ("z", "<f4")]))
    rec["x"], rec["y"], rec["z"], rec["e"] = [1.5, -2], [3, 4], [5, 6.25], [77, 78]
    path = tmp_path / "b.ply"
    path.write_bytes(_binary_ply(head, tags + rec.tobytes()))
    got = cloud.read_ply(path)
    assert np.array_equal(got["xyz"], np.array([[1.5, 3, 5], [-2, 4, 6.25]], np.float32)) and set(got) == {"xyz"}


def test_read_ply_refusals(cloud, hostlib, tmp_path):
    path = tmp_path / "big.ply"
    path.write_bytes(b"ply\nformat binary_big_endian 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\nend_header\n" + bytes(12))
    with pytest.raises(ValueError, match="big-endian"):
        cloud.read_ply(path)
    full = tmp_path / "full.ply"
    hostlib.write_ply(full, np.ones((10, 9), np.float32))
    cut = tmp_path / "cut.ply"
    cut.write_bytes(full.read_bytes()[:-5])
    with pytest.raises(ValueError, match="truncated"):
        cloud.read_ply(cut)
    lst = tmp_path / "list.ply"
    lst.write_bytes(_binary_ply(b"element vertex 1\nproperty float x\nproperty float y\nproperty float z\nproperty list uchar int n\n", bytes(13)))
    with pytest.raises(ValueError, match="list"):
        cloud.read_ply(lst)
    asc = tmp_path / "asc_cut.ply"
    asc.write_text(ASCII_PLY.split("4 5 7")[0])
    with pytest.raises(ValueError, match="truncated"):
        cloud.read_ply(asc)
    junk = tmp_path / "junk.ply"
    junk.write_bytes(b"not a ply")
    with pytest.raises(ValueError):
        cloud.read_ply(junk)


def test_score_arithmetic(cloud):
    inf = np.inf
    # thresholds are inclusive, in fp32
    d_rec = np.array([0.0, 0.1, np.float32(0.2), 0.3, inf], np.float32)
    d_gt = np.array([np.float32(0.1), 0.25, inf, inf], np.float32)
    res = cloud.score(d_rec, d_gt, [0.1, 0.2, 0.05])
    by = {r["tolerance"]: r for r in res["tolerances"]}
    assert [r["tolerance"] for r in res["tolerances"]] == [0.1, 0.2, 0.05]     # the caller's order
    assert (by[0.1]["n_accurate"], by[0.1]["n_complete"]) == (2, 1)
    assert (by[0.2]["n_accurate"], by[0.2]["n_complete"]) == (3, 1)
    assert (by[0.05]["n_accurate"], by[0.05]["n_complete"]) == (1, 0)
    assert by[0.1]["accuracy"] == 2 / 5 and by[0.1]["completeness"] == 1 / 4
    assert by[0.1]["f1"] == 2 * (2 / 5) * (1 / 4) / (2 / 5 + 1 / 4)
    assert by[0.05]["f1"] == 0.0      # completeness 0
    assert res["n_reconstruction"] == 5 and res["n_ground_truth"] == 4
    assert res["reconstruction_to_ground_truth"]["resolved"] == 4
    assert res["reconstruction_to_ground_truth"]["mean"] == pytest.approx(0.15, abs=1e-7)
    assert res["ground_truth_to_reconstruction"]["median"] == pytest.approx(0.175, abs=1e-7)
    # F1 is 0 at 0 / 0, and empty clouds divide nothing
    res = cloud.score(np.array([inf, inf]), np.array([inf]), [0.1])
    assert res["tolerances"][0]["accuracy"] == 0 and res["tolerances"][0]["completeness"] == 0 and res["tolerances"][0]["f1"] == 0
    assert res["reconstruction_to_ground_truth"] == {"resolved": 0, "mean": None, "median": None}
    res = cloud.score(np.zeros(0), np.zeros(0), [0.1])
    assert res["tolerances"][0]["f1"] == 0 and res["n_reconstruction"] == 0


def test_nonfinite_points_are_dropped_and_counted(cloud):
    a = np.arange(15, dtype=np.float32).reshape(5, 3)
    a[1, 2] = np.nan
    a[3, 0] = -np.inf
    kept, dropped = cloud.drop_nonfinite(a)
    assert dropped == 2 and np.array_equal(kept, a[[0, 2, 4]])
    res = cloud.score(np.zeros(3), np.zeros(4), [1.0], dropped=(dropped, 0))
    assert res["dropped_reconstruction"] == 2 and res["dropped_ground_truth"] == 0 and res["tolerances"][0]["f1"] == 1.0
    with pytest.raises(ValueError):
        cloud.drop_nonfinite(np.zeros((4, 2)))


def test_brute_force_by_hand():
    t = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [np.nan, 0, 0], [1, 0, 0]], np.float32)
    q = np.array([[0.5, 0, 0],        # ties between 0 and 1 (and 4): the smallest index
                  [1, 0.5, 0],        # nearest 1 (and its copy 4) at d2 0.25
                  [0, 1, 0],          # 0 and 2 at d2 1: outside radius 0.75
                  [0, 2.75, 0],       # 2 at exactly d2 = 0.5625 = r2: inside
                  [np.inf, 0, 0]], np.float32)
    d2, idx = brute_nearest(t, q, 0.75)
    assert idx.tolist() == [0, 1, -1, 2, -1]
    assert d2.tolist() == [0.25, 0.25, np.inf, 0.5625, np.inf]
    d2, idx = brute_nearest(t, q[:3], 1.0)
    assert idx.tolist() == [0, 1, 0] and d2.tolist() == [0.25, 0.25, 1.0]
    d2, idx = brute_nearest(np.zeros((0, 3), np.float32), q, 1.0)
    assert np.isinf(d2).all() and (idx == -1).all()
