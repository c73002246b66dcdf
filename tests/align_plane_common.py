"""The plain-loop statement of the point-to-plane pass (mpmvs_align_plane_sums; include/mpmvs.h) in numpy,
built on cloud_common.brute_nearest and align_common.frame_of / transform; the Gauss-Newton step through np.linalg.solve and
Rodrigues' formula, written independently of the C++ solver; and the scene of the tests.  numpy does not fuse, and every
operation of plane_sums is one fp64 operation in the order the contract states."""
import numpy as np

from align_common import FIX, frame_of, m34, similarity, transform
from cloud_common import brute_nearest

TRIU = [(i, j) for i in range(7) for j in range(i, 7)]   # the upper triangle row by row: sums[1..28]


def plane_sums(target, normals, source, M, radius):
    """(sums int64 [38], frame float64 [4]) of the statement"""
    t = np.ascontiguousarray(target, np.float32).reshape(-1, 3)
    nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    assert len(nrm) == len(t)
    frame = frame_of(t, radius)
    sums = np.zeros(38, np.int64)
    y = transform(source, M)
    if frame[3] == 0.0 or len(y) == 0:
        return sums, frame
    d2, idx = brute_nearest(t, y, radius)
    hit = idx >= 0
    if not hit.any():
        return sums, frame
    n = nrm[idx[hit]].astype(np.float64)
    with np.errstate(all="ignore"):
        q = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
    ok = np.isfinite(q) & (q != 0.0)
    if not ok.any():
        return sums, frame
    o, iu = frame[:3], 1.0 / frame[3]
    a = ((y[hit].astype(np.float64) - o) * iu)[ok]
    b = ((t[idx[hit]].astype(np.float64) - o) * iu)[ok]
    assert (np.abs(a) <= 1.0).all() and (np.abs(b) <= 1.0).all()
    nh = n[ok] / np.sqrt(q[ok])[:, None]
    e = a - b
    r = (e[:, 0] * nh[:, 0] + e[:, 1] * nh[:, 1]) + e[:, 2] * nh[:, 2]
    c0 = a[:, 1] * nh[:, 2] - a[:, 2] * nh[:, 1]
    c1 = a[:, 2] * nh[:, 0] - a[:, 0] * nh[:, 2]
    c2 = a[:, 0] * nh[:, 1] - a[:, 1] * nh[:, 0]
    g = (a[:, 0] * nh[:, 0] + a[:, 1] * nh[:, 1]) + a[:, 2] * nh[:, 2]
    J = [c0, c1, c2, nh[:, 0], nh[:, 1], nh[:, 2], g]
    assert (np.abs(nh) <= 1.0).all() and np.abs(r).max() < 0.87 and max(np.abs(v).max() for v in J) < 2.0

    def fix(x):
        return np.rint(x * FIX).astype(np.int64).sum()

    sums[0] = int(ok.sum())
    for k, (i, j) in enumerate(TRIU):
        sums[1 + k] = fix(J[i] * J[j])
    for i in range(7):
        sums[29 + i] = fix(J[i] * r)
    sums[36] = fix(r * r)
    sums[37] = fix(d2[hit][ok].astype(np.float64) * (iu * iu))
    return sums, frame


def normal_equations(sums):
    """(H float64 [7, 7], gvec float64 [7]) of the sums"""
    s = np.asarray(sums, np.float64) / FIX
    H = np.zeros((7, 7))
    for k, (i, j) in enumerate(TRIU):
        H[i, j] = H[j, i] = s[1 + k]
    return H, s[29:36]


def gauss_newton(sums, frame, M, with_scale):
    """(M_out [3, 4], rmse_plane, rmse_point): the step of the contract for sums it accepts, through np.linalg.solve, with the
    rotation of the unit quaternion (1, omega / 2) / |.| written as Rodrigues' formula about omega by the angle 2 atan(|omega| / 2)"""
    M = m34(M).copy()
    n = int(sums[0])
    m = 7 if with_scale else 6
    H, gvec = normal_equations(sums)
    o, u = np.asarray(frame[:3], np.float64), float(frame[3])
    x = np.linalg.solve(H[:m, :m], -gvec[:m])
    w, t, c = x[:3], x[3:6], (1.0 + x[6] if with_scale else 1.0)
    R = np.eye(3)
    nw = float(np.linalg.norm(w))
    if nw > 0:
        ax, th = w / nw, 2.0 * np.arctan(0.5 * nw)
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    D = np.eye(4)
    D[:3, :3] = c * R
    D[:3, 3] = o - c * R @ o + u * t
    M4 = np.eye(4)
    M4[:3] = M
    s = np.asarray(sums, np.float64) / FIX
    return (D @ M4)[:3], float(np.sqrt(s[36] / n) * u), float(np.sqrt(s[37] / n) * u)


FACES = ((0, 0.0), (1, 0.0), (2, 0.0), (0, 1.0))   # (axis, offset): x = 0, y = 0, z = 0, x = 1


def faces(rng, per_face, which=FACES):
    """(points float32, normals float32): `per_face` uniform samples of [0.1, 0.9]^2 on each face of `which`"""
    pts, nrm = [], []
    for axis, off in which:
        p = (0.1 + 0.8 * rng.random((per_face, 3))).astype(np.float32)
        p[:, axis] = off
        n = np.zeros((per_face, 3), np.float32)
        n[:, axis] = 1.0
        pts.append(p)
        nrm.append(n)
    return np.concatenate(pts), np.concatenate(nrm)


def plane_scene(with_scale=True, seed=4, which=FACES):
    """Four faces of the unit cube (x = 0, y = 0, z = 0, x = 1) sampled on [0.1, 0.9]^2: the target has 500 points per face, and
    the source 300 per face drawn INDEPENDENTLY -- no source is a target sample -- under the inverse of a known transform T_true
    (a similarity of scale 1.25, rigid with with_scale=False).  The start T0 is T_true perturbed by 0.4 degrees and 0.01 (and
    0.4 % in scale) about the cube's centre; the radius of the tests is RADIUS.  The two parallel faces fix the scale.
    Returns (target, target normals, source, T_true, T0)."""
    rng = np.random.default_rng(seed)
    target, normals = faces(rng, 500, which)
    on_faces, _ = faces(rng, 300, which)
    T_true = similarity(rng, 0.5, 1.25 if with_scale else 1.0, 0.7)
    src = ((on_faces.astype(np.float64) - T_true[:3, 3]) @ np.linalg.inv(T_true[:3, :3]).T).astype(np.float32)
    P = similarity(rng, np.deg2rad(0.4), 1.004 if with_scale else 1.0, 0.01)
    c = np.full(3, 0.5)
    P[:3, 3] += c - P[:3, :3] @ c
    return target, normals, src, T_true, P @ T_true


RADIUS = 0.05
CORNER = FACES[:3]   # three faces that meet in one point: the scale about that point moves no source off its plane
