"""Shared helpers of the COLMAP converter tests: the recorded fixture, a literal numpy statement of the pair score, and the
comparison of cams/ with the recorded ones."""
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "colmap_v1")


def parse_pairs(path):
    """pair.txt -> (ids, scores), each (N, num_view) int arrays"""
    tok = open(path).read().split()
    n, k = int(tok[0]), 1
    ids, scores = [], []
    for i in range(n):
        assert int(tok[k]) == i
        m = int(tok[k + 1])
        v = np.array([int(t) for t in tok[k + 2:k + 2 + 2 * m]], np.int64).reshape(m, 2)
        ids.append(v[:, 0])
        scores.append(v[:, 1])
        k += 2 + 2 * m
    return np.array(ids), np.array(scores)


def angle(ci, cj, p):
    """triangulation angle in degrees, float64, in the order of the contract"""
    a, b = ci - p, cj - p
    dot = lambda x, y: (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        return (180 / np.pi) * np.arccos(dot(a, b) / np.sqrt(dot(a, a)) / np.sqrt(dot(b, b)))


def literal_score(ids_i, ids_j, centers_i, centers_j, xyz):
    """the score of one pair, written pairwise: every entry of i's list whose point j also observes counts (duplicates
    in i's list each time), zeroed when the 75th-percentile angle (sorted, index int(0.75 n)) is below 1 degree"""
    sj = set(int(p) for p in ids_j if p >= 0)
    common = [int(p) for p in ids_i if p >= 0 and int(p) in sj]
    if not common:
        return 0
    th = angle(centers_i, centers_j, xyz[common])
    if np.sort(th)[int(len(th) * 0.75)] < 1:
        return 0
    return len(common)


def expected_order(score_row, num_view):
    """score descending, then index descending"""
    k = np.arange(len(score_row), dtype=np.int64)
    key = (np.asarray(score_row, np.int64) << 32) | k
    return np.argsort(-key, kind="stable")[:num_view]


def check_cams(got_dir, exp_dir, n):
    assert sorted(os.listdir(got_dir)) == sorted(os.listdir(exp_dir)) == ["%08d_cam.txt" % i for i in range(n)]
    for i in range(n):
        got = open(os.path.join(got_dir, "%08d_cam.txt" % i)).read()
        exp = open(os.path.join(exp_dir, "%08d_cam.txt" % i)).read()
        g, e = got.rstrip("\n").split("\n"), exp.rstrip("\n").split("\n")
        assert g[:-1] == e[:-1], i   # extrinsic and intrinsic blocks byte for byte
        assert np.allclose([float(v) for v in g[-1].split()], [float(v) for v in e[-1].split()], rtol=0, atol=1.0000001e-6), (i, g[-1], e[-1])
