"""mpmvs_align_plane_solve (host code of the HIP library; no GPU) against np.linalg.solve on sums of the numpy statement
(tests/align_plane_common.py), its refusals, and the point-to-plane loop of the statement on a scene whose source shares no
sample with its target: it reaches the known transform where the point-to-point loop stays where it started."""
import ctypes as C
import importlib

import numpy as np
import pytest

import align_common as ac
import align_plane_common as pc

# Largest element difference |M_out - numpy's| measured on the two solver cases below (CPU, numpy with OpenBLAS' LAPACK):
# 2.22e-16 (matrices with elements of magnitude ~1: one unit in the last place).  Asserted: 16 x that, the margin for another LAPACK build.
SOLVE_MEASURED = 2.22e-16
SOLVE_BOUND = 16 * SOLVE_MEASURED
# Largest element difference between the matrix the point-to-plane statement loop ends with and the known transform on
# plane_scene(): 5.83e-9 rigid and 4.49e-9 with scale, after 3 passes each (the sources are fp32 roundings of exact pre-images on the faces, ~3e-8 each).  Asserted:
# 16 x the measured value, and in any case below 1e-6.
ICP_MEASURED = {False: 5.83e-9, True: 4.49e-9}
ICP_BOUND = {k: min(16 * v, 1e-6) for k, v in ICP_MEASURED.items()}

NEW = ["mpmvs_align_set_normals", "mpmvs_align_plane_sums", "mpmvs_align_plane_solve", "mpmvs_align_plane_icp"]


@pytest.fixture(scope="module")
def cloud(pm):
    return importlib.import_module("mp-mvs_amd.cloud")


def test_symbols_in_both_libraries(pm):
    engine = importlib.import_module("mp-mvs_amd.engine")
    assert set(NEW) <= set(engine.ALL_SYMBOLS)
    for path in (engine.LIB_PATH, engine.LIB_Q8_PATH):
        lib = C.CDLL(path)
        for name in NEW:
            assert hasattr(lib, name), (path, name)


def test_null_arguments(pm):
    """found before the device is touched: this runs without one"""
    engine = importlib.import_module("mp-mvs_amd.engine")
    _, f = engine.load()
    PD, PL = C.POINTER(C.c_double), C.POINTER(C.c_longlong)
    m, sums, frame = np.ascontiguousarray(np.eye(4)[:3]).reshape(12), np.zeros(38, np.int64), np.zeros(4)
    mp, sp, fp = m.ctypes.data_as(PD), sums.ctypes.data_as(PL), frame.ctypes.data_as(PD)
    nrm = np.zeros((4, 3), np.float32)
    assert f["align_set_normals"](None, nrm.ctypes.data) == -2
    assert f["align_set_normals"](None, None) == -2
    assert f["align_plane_sums"](None, 0.2, mp, sp, fp) == -2
    assert f["align_plane_icp"](None, 0.2, 1, 5, 0.0, mp, None, None, None, None) == -2
    assert f["align_plane_solve"](None, fp, 1, mp, mp, None, None) == -2
    assert f["align_plane_solve"](sp, None, 1, mp, mp, None, None) == -2
    assert f["align_plane_solve"](sp, fp, 1, None, mp, None, None) == -2
    assert f["align_plane_solve"](sp, fp, 1, mp, None, None, None) == -2
    assert f["align_plane_solve"](sp, fp, 1, mp, mp, None, None) == 1   # no pairs; both rmse pointers may be NULL


@pytest.fixture(scope="module")
def scenes():
    return {ws: pc.plane_scene(ws) for ws in (False, True)}


@pytest.mark.parametrize("with_scale", [False, True])
def test_solver_matches_numpy_solve(cloud, scenes, with_scale):
    """measured 2.22e-16, asserted 3.55e-15 (SOLVE_BOUND)"""
    target, normals, src, T_true, T0 = scenes[with_scale]
    sums, frame = pc.plane_sums(target, normals, src, T0, pc.RADIUS)
    assert sums[0] >= 1000
    rc, got, rmse_plane, rmse_point = cloud.plane_solve(sums, frame, T0, with_scale)
    want, rp_np, rq_np = pc.gauss_newton(sums, frame, T0, with_scale)
    diff = float(np.abs(got - want).max())
    print(f"with_scale={with_scale}: n {int(sums[0])} max |diff| {diff:.3e} rmse_plane {rmse_plane:.6g} rmse_point {rmse_point:.6g}")
    assert rc == 0
    assert diff <= SOLVE_BOUND
    assert abs(rmse_plane - rp_np) <= 4 * np.finfo(np.float64).eps * rp_np and abs(rmse_point - rq_np) <= 4 * np.finfo(np.float64).eps * rq_np
    assert rmse_plane < rmse_point   # a distance along a unit normal is at most the distance
    L = got[:, :3] @ np.linalg.inv(ac.m34(T0)[:, :3])   # the update's linear part: a rotation times a positive scale
    s = np.cbrt(np.linalg.det(L))
    assert s > 0 and np.abs(L.T @ L / (s * s) - np.eye(3)).max() < 1e-12
    if not with_scale:
        assert abs(s - 1.0) < 1e-12
    # status 1 leaves M alone and still reports both rmse
    rc, same, rp1, rq1 = cloud.plane_solve(np.concatenate([[5], sums[1:]]), frame, T0, with_scale)
    assert rc == 1 and np.array_equal(same, ac.m34(T0)) and rp1 > 0 and rq1 > 0


def test_exact_planes_are_refused(cloud):
    """one exact plane, and two parallel ones: the in-plane translations and the rotation about the normal do not move a source
    off its plane, their columns of J are exactly 0, and so is a pivot"""
    rng = np.random.default_rng(31)
    for which in ((pc.FACES[2],), (pc.FACES[0], pc.FACES[3])):
        t, n = pc.faces(rng, 300, which)
        s, _ = pc.faces(rng, 200, which)
        s = s + np.float32(0.01) * np.eye(3, dtype=np.float32)[which[0][0]]   # off the plane along the normal: r != 0
        sums, frame = pc.plane_sums(t, n, s, np.eye(4), pc.RADIUS)
        assert sums[0] >= 100
        H, _ = pc.normal_equations(sums)
        assert (np.diag(H) == 0).any()
        for ws in (False, True):
            rc, M, rmse_plane, _ = cloud.plane_solve(sums, frame, np.eye(4), ws)
            assert rc == 1 and np.array_equal(M, np.eye(4)[:3]) and abs(rmse_plane - 0.01) < 1e-6


def test_corner_fixes_a_rigid_motion_but_no_scale(cloud):
    """three faces that meet in one point: with the sources on their planes (at T_true, up to their fp32 rounding) a scale
    change about that point keeps them there, so with scale the last pivot is rounding only (status 1); the rigid step of the
    same sums, and the one from the perturbed start, are well determined (status 0)"""
    target, normals, src, T_true, T0 = pc.plane_scene(False, which=pc.CORNER)
    sums, frame = pc.plane_sums(target, normals, src, T_true, pc.RADIUS)
    assert sums[0] >= 700
    rc, M, _, _ = cloud.plane_solve(sums, frame, T_true, True)
    assert rc == 1 and np.array_equal(M, T_true[:3])
    rc, M, _, _ = cloud.plane_solve(sums, frame, T_true, False)
    assert rc == 0 and np.abs(M - T_true[:3]).max() < 1e-7
    sums, frame = pc.plane_sums(target, normals, src, T0, pc.RADIUS)
    rc, M, _, _ = cloud.plane_solve(sums, frame, T0, False)
    assert rc == 0 and np.abs(M - T_true[:3]).max() < 0.1 * np.abs(ac.m34(T0) - T_true[:3]).max()
    # 0.4 degrees off, the free direction turns with the source to first order: the last pivot is 6.8e-11 of its diagonal
    rc, M, _, _ = cloud.plane_solve(sums, frame, T0, True)
    assert rc == 1 and np.array_equal(M, ac.m34(T0))


def test_few_pairs_and_bad_scale(cloud):
    target, normals, src, T_true, T0 = pc.plane_scene(True)
    sums, frame = pc.plane_sums(target, normals, src, T0, pc.RADIUS)
    few = sums.copy()
    few[0] = 6
    assert cloud.plane_solve(few, frame, T0, True)[0] == 1 and cloud.plane_solve(few, frame, T0, False)[0] == 0
    few[0] = 5
    assert cloud.plane_solve(few, frame, T0, False)[0] == 1
    # a residual that asks for sigma <= -1: gvec = 1.5 H e_6, so x = -1.5 e_6 up to rounding and the scale would be -0.5
    H, _ = pc.normal_equations(sums)
    bad = sums.copy()
    bad[29:36] = np.rint(1.5 * H[:, 6] * ac.FIX).astype(np.int64)
    rc, M, _, _ = cloud.plane_solve(bad, frame, T0, True)
    assert rc == 1 and np.array_equal(M, ac.m34(T0))
    assert cloud.plane_solve(bad, frame, T0, False)[0] == 0


@pytest.mark.parametrize("with_scale", [False, True])
def test_statement_loop_reaches_the_transform_where_point_to_point_does_not(cloud, scenes, with_scale):
    """measured 5.83e-9 rigid and 4.49e-9 with scale, asserted 9.33e-8 and 7.18e-8 (ICP_BOUND); the point-to-point loop from the
    same start ends 7.78e-3 (rigid, 30 passes) and 1.25e-2 (with scale, 19 passes) away, no nearer than the start (1.25e-2, 1.54e-2)"""
    target, normals, src, T_true, T0 = scenes[with_scale]
    eps = 2.0 ** -20
    M, passes, inliers, rmse_plane, rmse_point = cloud.plane_icp_loop(lambda r, X: pc.plane_sums(target, normals, src, X, r), pc.RADIUS, T0, with_scale, 30, eps)
    err = float(np.abs(M - T_true[:3]).max())
    Mp, passes_p, _, _ = cloud.icp_loop(lambda r, X: ac.brute_sums(target, src, X, r), pc.RADIUS, T0, with_scale, 30, eps)
    err_p = float(np.abs(Mp - T_true[:3]).max())
    print(f"with_scale={with_scale}: plane passes {passes} inliers {inliers} rmse_plane {rmse_plane:.3e} rmse_point {rmse_point:.3e} "
          f"max |M - T_true| {err:.3e}; point passes {passes_p} max |M - T_true| {err_p:.3e}; start {np.abs(T0 - T_true).max():.3e}")
    assert passes < 30   # it ended by the eps rule
    assert inliers > 1100
    assert err <= ICP_BOUND[with_scale] and err < 1e-6
    assert err_p > 1e-3


def test_flipped_normals_give_the_same_bits(scenes):
    target, normals, src, T_true, T0 = scenes[True]
    rng = np.random.default_rng(6)
    scaled = normals * rng.uniform(0.1, 10.0, (len(normals), 1)).astype(np.float32) + rng.normal(size=normals.shape).astype(np.float32) * np.float32(0.05)
    want, _ = pc.plane_sums(target, scaled, src, T0, pc.RADIUS)
    assert want[0] > 1000 and want[29:36].any()
    assert np.array_equal(pc.plane_sums(target, -scaled, src, T0, pc.RADIUS)[0], want)
    some = scaled * np.where(rng.random((len(normals), 1)) < 0.5, np.float32(-1), np.float32(1))
    assert np.array_equal(pc.plane_sums(target, some, src, T0, pc.RADIUS)[0], want)
