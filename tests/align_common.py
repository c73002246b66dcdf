"""The plain-loop statement of the ICP pass (mpmvs_align_sums; include/mpmvs.h) in numpy, built on
cloud_common.brute_nearest, and Umeyama's closed form through numpy's SVD, written independently of the C++ solver.  numpy
does not fuse, and every operation below is one fp64 (or fp32) operation in the order the contract states."""
import numpy as np

from cloud_common import brute_nearest

FIX = 2.0 ** 30


def m34(M):
    a = np.asarray(M, np.float64)
    return a[:3] if a.shape == (4, 4) else a.reshape(3, 4)


def frame_of(targets, radius):
    """frame float64 [4] = (o, u); all zero for a target without a finite point"""
    t = np.ascontiguousarray(targets, np.float32).reshape(-1, 3)
    t = t[np.isfinite(t).all(1)]
    if len(t) == 0:
        return np.zeros(4)
    mn, mx = t.min(0).astype(np.float64), t.max(0).astype(np.float64)
    h = 0.5 * float((mx - mn).max()) + 2.0 * float(np.float32(radius))
    u = 1.0
    while u < h:
        u *= 2.0
    while u * 0.5 >= h:
        u *= 0.5
    return np.array([*(0.5 * (mn + mx)), u])


def transform(source, M):
    """y float32 [n, 3] of the statement; rows of non-finite sources are NaN"""
    s = np.ascontiguousarray(source, np.float32).reshape(-1, 3).astype(np.float64)
    M = m34(M)
    with np.errstate(all="ignore"):
        y = np.stack([((M[k, 0] * s[:, 0] + M[k, 1] * s[:, 1]) + M[k, 2] * s[:, 2]) + M[k, 3] for k in range(3)], 1).astype(np.float32)
    y[~np.isfinite(s).all(1)] = np.nan
    return y


def brute_sums(target, source, M, radius):
    """(sums int64 [18], frame float64 [4]) of the statement"""
    t = np.ascontiguousarray(target, np.float32).reshape(-1, 3)
    frame = frame_of(t, radius)
    sums = np.zeros(18, np.int64)
    y = transform(source, M)
    if frame[3] == 0.0 or len(y) == 0:
        return sums, frame
    d2, idx = brute_nearest(t, y, radius)
    hit = idx >= 0
    if not hit.any():
        return sums, frame
    o, iu = frame[:3], 1.0 / frame[3]
    a = (y[hit].astype(np.float64) - o) * iu
    b = (t[idx[hit]].astype(np.float64) - o) * iu
    assert (np.abs(a) <= 1.0).all() and (np.abs(b) <= 1.0).all()

    def fix(x):
        return np.rint(x * FIX).astype(np.int64).sum()

    sums[0] = int(hit.sum())
    for k in range(3):
        sums[1 + k] = fix(a[:, k])
        sums[4 + k] = fix(b[:, k])
        for j in range(3):
            sums[7 + 3 * k + j] = fix(a[:, k] * b[:, j])
    sums[16] = fix((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])
    sums[17] = fix(d2[hit].astype(np.float64) * (iu * iu))
    return sums, frame


def sigma_of(sums):
    """the cross-covariance of the matched pairs in the normalised frame (target rows, source columns)"""
    s = np.asarray(sums, np.float64) / FIX
    n = float(sums[0])
    return (s[7:16].reshape(3, 3) / n).T - np.outer(s[4:7] / n, s[1:4] / n)


def umeyama(sums, frame, M, with_scale):
    """(status, M_out [3, 4], rmse): Umeyama 1991 on the moments the sums hold, with numpy's SVD"""
    M = m34(M).copy()
    n = int(sums[0])
    s = np.asarray(sums, np.float64) / FIX
    o, u = np.asarray(frame[:3], np.float64), float(frame[3])
    rmse = float(np.sqrt(s[17] / n) * u) if n > 0 else 0.0
    if n < 3:
        return 1, M, rmse
    mu_a, mu_b = s[1:4] / n, s[4:7] / n
    sigma = (s[7:16].reshape(3, 3) / n).T - np.outer(mu_b, mu_a)   # target rows, source columns
    var_a = s[16] / n - mu_a @ mu_a
    if not var_a > 0:
        return 1, M, rmse
    U, d, Vt = np.linalg.svd(sigma)
    if not d[0] > 0:
        return 1, M, rmse
    S = np.diag([1.0, 1.0, -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0])
    R = U @ S @ Vt
    c = float((d * np.diag(S)).sum() / var_a) if with_scale else 1.0
    t = mu_b - c * R @ mu_a
    D = np.eye(4)
    D[:3, :3] = c * R
    D[:3, 3] = o - c * R @ o + u * t
    M4 = np.eye(4)
    M4[:3] = M
    return 0, (D @ M4)[:3], rmse


def similarity(rng, angle, scale, shift):
    """4 x 4: a rotation by `angle` about a random axis, times `scale`, plus a translation of length `shift`"""
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K
    t = rng.normal(size=3)
    T = np.eye(4)
    T[:3, :3] = scale * R
    T[:3, 3] = t / np.linalg.norm(t) * shift
    return T


def icp_scene(seed=3):
    """the scene of the statement-loop tests: a volumetric random target of 2 000 points in the unit cube (typical spacing
    ~0.08), the source an exact subset of 1 200 of them under the inverse of a known similarity T_true, and a start T0 that is
    T_true perturbed by less than half the spacing anywhere in the cube (0.4 degrees, scale 1.004, shift 0.01)."""
    rng = np.random.default_rng(seed)
    target = rng.random((2000, 3), dtype=np.float32)
    T_true = similarity(rng, 0.5, 1.25, 0.7)
    pick = rng.choice(2000, 1200, replace=False)
    src = ((target[pick].astype(np.float64) - T_true[:3, 3]) @ np.linalg.inv(T_true[:3, :3]).T).astype(np.float32)
    P = similarity(rng, np.deg2rad(0.4), 1.004, 0.01)
    c = np.full(3, 0.5)
    P[:3, 3] += c - P[:3, :3] @ c   # the perturbation turns and scales about the cube's centre
    return target, src, T_true, P @ T_true
