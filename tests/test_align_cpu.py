"""mpmvs_align_solve (host code of the HIP library; no GPU) against numpy's Umeyama on sums of the numpy statement, and the ICP
loop of the statement (align_common.brute_sums + mpmvs_align_solve) on a scene with a known answer."""
import importlib

import numpy as np
import pytest

import align_common as ac
from cloud_common import brute_nearest

# Largest element difference |M_out - numpy's| measured on the solver cases below (CPU, numpy with OpenBLAS' LAPACK): 1.11e-15
# (matrices with elements of magnitude ~1).  Asserted: 16 x that, the margin for another LAPACK build.
SOLVE_MEASURED = 1.11e-15
SOLVE_BOUND = 16 * SOLVE_MEASURED
# Largest element difference between the matrix the statement loop ends with and the known similarity, measured on icp_scene():
# 1.55e-9 (the sources are fp32 roundings of the exact pre-images, ~3e-8 each, averaged over 1 200 pairs).  Asserted: 16 x that.
ICP_MEASURED = 1.55e-9
ICP_BOUND = 16 * ICP_MEASURED


@pytest.fixture(scope="module")
def cloud(pm):
    return importlib.import_module("mp-mvs_amd.cloud")


def solver_cases():
    rng = np.random.default_rng(21)
    t = rng.random((1500, 3), dtype=np.float32)
    cases = {}
    T = ac.similarity(rng, 0.3, 1.1, 0.2)
    s = ((t[:800].astype(np.float64) - T[:3, 3]) @ np.linalg.inv(T[:3, :3]).T).astype(np.float32)
    s = s + rng.normal(size=s.shape).astype(np.float32) * np.float32(0.01)
    cases["random similarity"] = (t, s, ac.similarity(rng, 0.02, 1.01, 0.01) @ T, 0.1)
    cases["identity"] = (t, t[:700].copy(), np.eye(4), 0.1)
    # a thin slab on a jittered lattice of spacing 1/16, and its mirror image in the slab's mid-plane: a source is at most
    # 0.02 from its own mirror partner and more than 0.04 from any other target, so nearest = index, the pairs are the mirror
    # pairs and the best orthogonal map is the reflection: det(Sigma) < 0
    g = (np.arange(16, dtype=np.float32) + np.float32(0.5)) / np.float32(16)
    slab = np.stack([*np.meshgrid(g, g, indexing="ij"), np.zeros((16, 16), np.float32)], -1).reshape(-1, 3)
    rng_slab = np.random.default_rng(22)   # its own stream: the other cases keep their points
    slab[:, :2] += (rng_slab.random((256, 2), dtype=np.float32) - np.float32(0.5)) * np.float32(0.01)
    slab[:, 2] = np.float32(0.5) + (rng_slab.random(256, dtype=np.float32) - np.float32(0.5)) * np.float32(0.02)
    mirrored = slab.copy()
    mirrored[:, 2] = 1 - mirrored[:, 2]
    cases["reflection fix"] = (slab, mirrored, np.eye(4), 0.03)
    tp = t.copy()
    tp[:, 2] = 0.25
    sp = tp[:500] + np.float32(0.01) * rng.normal(size=(500, 3)).astype(np.float32)
    sp[:, 2] = 0.25
    cases["planar"] = (tp, sp, np.eye(4), 0.1)
    return cases


CASES = solver_cases()


@pytest.mark.parametrize("with_scale", [True, False])
@pytest.mark.parametrize("name", list(CASES))
def test_solver_matches_numpy_umeyama(cloud, name, with_scale):
    """measured 1.11e-15, asserted 1.78e-14 (SOLVE_BOUND)"""
    t, s, M, radius = CASES[name]
    sums, frame = ac.brute_sums(t, s, M, radius)
    assert sums[0] >= 256
    rc, got, rmse = cloud.solve(sums, frame, M, with_scale)
    rc_np, want, rmse_np = ac.umeyama(sums, frame, M, with_scale)
    diff = float(np.abs(got - want).max())
    print(f"{name} with_scale={with_scale}: n {int(sums[0])} max |diff| {diff:.3e} rmse {rmse:.6g}")
    assert rc == 0 and rc_np == 0
    assert diff <= SOLVE_BOUND
    assert abs(rmse - rmse_np) <= 4 * np.finfo(np.float64).eps * rmse_np
    R = got[:, :3] @ np.linalg.inv(ac.m34(M)[:, :3])   # the update's linear part: a rotation times a positive scale
    assert np.linalg.det(R) > 0
    if name == "reflection fix":
        # the matches are the mirror pairs, the covariance has a negative determinant, and the fix is what keeps R proper
        assert np.array_equal(brute_nearest(t, ac.transform(s, M), radius)[1], np.arange(len(t)))
        U, _, Vt = np.linalg.svd(ac.sigma_of(sums))
        assert np.linalg.det(U) * np.linalg.det(Vt) < 0
        assert np.abs(U @ Vt - R / np.cbrt(np.linalg.det(R))).max() > 0.5   # the unfixed answer is an improper map, far away
    if not with_scale:
        assert np.abs(R.T @ R - np.eye(3)).max() < 1e-12


def test_solver_returns_1(cloud):
    """fewer than 3 pairs, no source variance, no covariance: status 1 and M_out = M_in, in numpy's Umeyama alike"""
    M = ac.similarity(np.random.default_rng(1), 0.1, 1.0, 0.0)
    M[:3, 3] = 0
    I = np.eye(4)
    corners = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)
    few = (corners, corners[:2].copy(), I, 0.25)
    # o = 0.5, u = 1: a = 0.125 exactly in every pair, so the variance cancels exactly
    t_var = np.concatenate([corners, np.full((1, 3), 0.625, np.float32)])
    no_var = (t_var, np.full((5, 3), 0.625, np.float32), I, 0.25)
    # one target position (b = 0 exactly), three distinct sources
    no_cov = (np.full((4, 3), 0.5, np.float32), np.array([[0.5, 0.5, 0.6], [0.4, 0.5, 0.5], [0.5, 0.6, 0.5]], np.float32), I, 0.25)
    for name, (t, s, M0, radius), n in (("few", few, 2), ("no variance", no_var, 5), ("no covariance", no_cov, 3)):
        sums, frame = ac.brute_sums(t, s, M0, radius)
        assert sums[0] == n, name
        rc, got, _ = cloud.solve(sums, frame, M, True)
        assert rc == 1 and np.array_equal(got, M[:3]), name
        assert ac.umeyama(sums, frame, M, True)[0] == 1, name
    rc, got, rmse = cloud.solve(np.zeros(18, np.int64), np.zeros(4), M, True)
    assert rc == 1 and np.array_equal(got, M[:3]) and rmse == 0.0


@pytest.fixture(scope="module")
def statement_loop(cloud):
    target, src, T_true, T0 = ac.icp_scene()
    eps = 2.0 ** -20
    return cloud.icp_loop(lambda r, M: ac.brute_sums(target, src, M, r), 0.05, T0, True, 30, eps), T_true, T0


def test_statement_loop_recovers_known_similarity(statement_loop):
    """measured 1.55e-9, asserted 2.48e-8 (ICP_BOUND); the start is 9.67e-3 away"""
    (M, passes, inliers, rmse), T_true, T0 = statement_loop
    err = float(np.abs(M - T_true[:3]).max())
    print(f"passes {passes} inliers {inliers} rmse {rmse:.3e} max |M - T_true| {err:.3e}, start {np.abs(T0 - T_true).max():.3e}")
    assert passes < 30   # it ended by the eps rule
    assert inliers == 1200
    assert np.abs(T0 - T_true).max() > 1e-3
    assert err <= ICP_BOUND


def test_update_move_is_zero_for_identity(cloud):
    assert cloud.update_move(np.eye(4)[:3], [0.5, 0.5, 0.5, 1.0]) == 0.0
    D = np.eye(4)[:3].copy()
    D[0, 3] = 0.25
    assert cloud.update_move(D, [0.5, 0.5, 0.5, 1.0]) == 0.25
