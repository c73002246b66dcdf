"""mpmvs_surface_distance and mpmvs_surface_sample on the device, bit for bit against the numpy statements of mesh_distance_common.py:
the hand-worked scenes, a sphere and a cube with points all around them, one triangle spanning the whole cloud (the large-triangle
path, also with the threshold forced low and high), a mesh reaching far outside the cloud, the seeded sweep; the refusals of a live
pair of handles and what is answered on the host; the sampler with colours and normals and its two refusals found on the device; and
evaluate_mesh and compare on top of them."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import mesh_clean_common as mc
import mesh_distance_common as md
import mesh_simplify_common as msc

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def mesh(engine):
    return importlib.import_module("mp-mvs_amd.mesh")


@pytest.fixture(scope="module")
def cloud(engine):
    return importlib.import_module("mp-mvs_amd.cloud")


def _check(mesh, cloud, m, pts, radius, want=None):
    want = want or md.distance_statement(m["xyz"], m["tri"], pts, radius)
    with mesh.Mesh(m["xyz"], m["tri"]) as h, cloud.Cloud(pts) as c:
        d2, tri = h.distance(c, radius)
        assert md.same_bits(d2, want[0]) and np.array_equal(tri, want[1]) and tri.dtype == np.int32
        assert h.last_counts == {"with_candidate": int(want[2][0]), "taking_part": int(want[2][1])}
        only = h.distance(c, radius, want_tri=False)   # the grid is cached now; without the triangles
        assert md.same_bits(only, want[0])
        ms = h.distance_ms()
    return ms


@functools.lru_cache(maxsize=None)
def _sphere_want(radius):
    m, pts = md.sphere_shell()
    return md.distance_statement(m["xyz"], m["tri"], pts, radius)


def test_hand_worked_scenes(mesh, cloud):
    m = md.hand_mesh()
    on = np.array([[3, 4, 0], [0, 0, 0], [0, 4, 0], [1.5, 2, 0], [1.5, 4, 0], [0, 2, 0], [1, 3, 0]], F)
    just = np.array([[1, 3, 2], [1, 3, np.nextafter(F(2), F(3))], [1, 3, -2], [1, 3, np.nextafter(F(-2), F(-3))]], F)
    pts = np.concatenate([md.HAND_POINTS, on, just, [[np.nan, 1, 1]]]).astype(F)
    for radius in (2.0, 3.0, 10.0, 1e-3):
        _check(mesh, cloud, m, pts, radius)
    with mesh.Mesh(m["xyz"], m["tri"]) as h, cloud.Cloud(md.HAND_POINTS) as c:
        d2, tri = h.distance(c, 10.0)
        assert d2.tolist() == [6, 2, 25, 2, 4, 4, 4] and tri.tolist() == [0] * 7
    # ties: reversed, repeated and rotated copies; degenerate triangles
    tri = np.array([[2, 1, 0], [0, 1, 2], [0, 1, 2], [1, 2, 0]], np.int32)
    _check(mesh, cloud, mc._mesh(md.HAND_TRI, tri), pts, 10.0)
    deg = mc._mesh(np.array([[0, 0, 0], [0, 0, 0], [2, 0, 0]], F), [[0, 0, 0], [0, 1, 2], [0, 2, 2]])
    _check(mesh, cloud, deg, np.array([[-1, 1, 0], [0, 3, 0], [1, 1, 0], [3, 0, 0], [1, 0, 0]], F), 10.0)
    # scaled by 2^+-40 with the radius
    for p in (-40, 40):
        s = F(2.0) ** p
        _check(mesh, cloud, mc._mesh(md.HAND_TRI * s, tri), (pts * s).astype(F), float(F(3.0) * s))


@pytest.mark.parametrize("radius", md.SPHERE_RADII)
def test_sphere_with_a_shell_of_points(mesh, cloud, radius):
    m, pts = md.sphere_shell()
    want = _sphere_want(radius)
    if radius == md.SPHERE_RADII[1]:
        assert 0 < want[2][0] < want[2][1]   # some of the shell has no candidate
    ms = _check(mesh, cloud, m, pts, radius, want)
    assert ms["total"] > 0 and ms["scatter"] > 0


def test_cube_faces_edges_and_vertices(mesh, cloud):
    m, pts = md.cube_voronoi()
    for radius in (0.2, 0.6):
        _check(mesh, cloud, m, pts, radius)


@pytest.mark.parametrize("large", (None, "0", "1073741824"))
def test_one_triangle_spanning_the_cloud(mesh, cloud, monkeypatch, large):
    """the cell range of the triangle has tens of thousands of cells at this radius: by default a block walks them, as with the threshold
    forced low; forced high, one lane walks a range (at a larger radius) that it finishes in a blink"""
    m, pts, radius = md.spanning_triangle(n=4000 if large != "1073741824" else 300)
    if large is None:
        monkeypatch.delenv("MPMVS_SURFACE_LARGE", raising=False)
    else:
        monkeypatch.setenv("MPMVS_SURFACE_LARGE", large)
    radius = radius if large != "1073741824" else 0.25
    want = md.distance_statement(m["xyz"], m["tri"], pts, radius)
    assert 0 < want[2][0] < want[2][1]
    _check(mesh, cloud, m, pts, radius, want)


def test_mesh_reaching_far_outside_the_cloud(mesh, cloud):
    m, pts, radius = md.far_outside()
    want = md.distance_statement(m["xyz"], m["tri"], pts, radius)
    assert want[2][0] > 0
    _check(mesh, cloud, m, pts, radius, want)
    # and a cloud far larger than the mesh
    big = (np.random.default_rng(2).uniform(-40, 40, (3000, 3))).astype(F)
    _check(mesh, cloud, md.hand_mesh(), big, 6.0)


def test_seeded_sweep(mesh, cloud):
    for k in range(md.SWEEP_CASES):
        m, pts, radius = md.sweep_case(k)
        _check(mesh, cloud, m, pts, radius, md.sweep_want(k)[:3])


def test_refusals_of_a_live_pair_and_host_answers(mesh, cloud, engine):
    _, fns = engine.load()
    err = lambda: fns["last_error"](None).decode()   # noqa: E731
    m = md.hand_mesh()
    with mesh.Mesh(m["xyz"], m["tri"]) as h, cloud.Cloud(md.HAND_POINTS) as c:
        d2, tri, counts = np.full(7, 7, F), np.full(7, 7, np.int32), (C.c_longlong * 2)(7, 7)
        untouched = lambda: bool((d2 == 7).all() and (tri == 7).all()) and list(counts) == [7, 7]   # noqa: E731
        call = lambda mh, ch, r, out=d2.ctypes.data: fns["surface_distance"](mh, ch, r, out, tri.ctypes.data, counts)   # noqa: E731
        assert call(None, c._h, 1.0) == -2 and call(h._h, None, 1.0) == -2 and untouched()
        for r in (0.0, -1.0, float("nan"), float("inf")):
            assert call(h._h, c._h, r) == -2 and "radius" in err() and untouched(), r
        assert call(h._h, c._h, 1.0, None) == -2 and untouched()
        assert call(h._h, c._h, 1e-7) == -3 and "2^21" in err() and "surface distance" in err() and untouched()
        assert c.stats()["cells"] == 0   # no refusal built a grid
        with pytest.raises(ValueError):
            h.distance(c, -1.0)
    # answered on the host: no point, no triangle, no finite triangle, no finite point
    nan_mesh = mc._mesh(np.array([[0, 0, 0], [1, np.nan, 0], [0, 1, 0]], F), [[0, 1, 2]])
    no_tri = mc._mesh(m["xyz"], np.zeros((0, 3), np.int32))
    nan_pts = np.array([[np.nan, 0, 0], [0, np.inf, 0]], F)
    for mm, pts, part in ((m, np.zeros((0, 3), F), 0), (no_tri, md.HAND_POINTS, 7), (nan_mesh, md.HAND_POINTS, 7), (m, nan_pts, 0)):
        with mesh.Mesh(mm["xyz"], mm["tri"]) as h, cloud.Cloud(pts) as c:
            d2, tri = h.distance(c, 1.0)
            assert len(d2) == len(pts) and np.isinf(d2).all() and (tri == -1).all()
            assert h.last_counts == {"with_candidate": 0, "taking_part": part} and h.distance_ms()["total"] == 0.0


def test_the_cloud_keeps_serving_its_own_calls(mesh, cloud):
    """the distance call uses the cloud's grid cache as every operation does: nearest() before and after is the same, and the grid a
    distance call built is found by the nearest() call at that radius"""
    m, pts = md.sphere_shell()
    q = pts[:500] + F(0.01)
    with mesh.Mesh(m["xyz"], m["tri"]) as h, cloud.Cloud(pts) as c:
        before = c.nearest(q, 0.3)
        assert c.kernel_ms()[1] > 0
        h.distance(c, 0.3)
        h.distance(c, 0.7)
        after = c.nearest(q, 0.7)
        assert c.kernel_ms()[1] == 0   # built by the distance call
        again = c.nearest(q, 0.3)
        assert md.same_bits(again[0], before[0]) and np.array_equal(again[1], before[1])
        assert np.isfinite(after[0]).sum() >= np.isfinite(before[0]).sum()


# ---- the sampler ----------------------------------------------------------------------------------------------------------------------------
def _same_samples(got, want):
    return (md.same_bits(got["xyz"], want["xyz"]) and np.array_equal(got["tri_of"], want["tri_of"]) and got["tri_of"].dtype == np.int32
            and ((want["rgb"] is None and got["rgb"] is None) or np.array_equal(got["rgb"], want["rgb"]))
            and ((want["normals"] is None and got["normals"] is None) or md.same_bits(got["normals"], want["normals"])))


def test_samples_of_the_hand_triangle(mesh):
    rgb = np.array([[10, 200, 7], [20, 100, 8], [30, 50, 9]], np.uint8)
    with mesh.Mesh(md.HAND_TRI, [[0, 1, 2]], rgb) as h:
        for spacing in (5.0, 2.5, np.nextafter(F(2.5), F(0)), np.nextafter(F(2.5), F(9)), 5.0 / 3, 5.0 / 7, 0.013):
            for nrm in (False, True):
                assert _same_samples(h.sample(spacing, nrm), md.sample_statement(md.HAND_TRI, [[0, 1, 2]], spacing, rgb, nrm)), spacing
        assert h.sample_ms()["total"] > 0


def test_samples_of_meshes(mesh):
    rng = np.random.default_rng(4)
    m = mc.anchor()
    rgb = rng.integers(0, 256, (len(m["xyz"]), 3)).astype(np.uint8)
    with mesh.Mesh(m["xyz"], m["tri"], rgb) as h:
        for spacing in (0.5, 0.11):
            assert _same_samples(h.sample(spacing, True), md.sample_statement(m["xyz"], m["tri"], spacing, rgb, True))
    # a fan of one huge and many tiny triangles, a zero-size one and non-finite vertices; more than one block of samples and of triangles
    xyz = rng.uniform(-1, 1, (900, 3)).astype(F) * F(0.01)
    xyz[:3] = [[-3, -2, 1], [4, -1, 0], [0, 5, -1]]
    xyz[10] = np.nan
    tri = np.concatenate([[[0, 1, 2], [5, 5, 5], [10, 11, 12]], rng.integers(3, 900, (700, 3))]).astype(np.int32)
    with mesh.Mesh(xyz, tri) as h:
        for spacing in (0.05, 0.004):
            assert _same_samples(h.sample(spacing, True), md.sample_statement(xyz, tri, spacing, None, True))


def test_sample_refusals_found_on_the_device(mesh):
    xyz = np.array([[0.3, -7.25, 1e-3], [3, 4, 0], [0, 0, 0], [0, 4, 0]], F)
    with mesh.Mesh(xyz, [[0, 0, 0], [1, 2, 3]]) as h:
        assert len(h.sample(5.0 / 64)["xyz"]) == 1 + 64 * 64
        assert len(h.sample(F(5.0) / F(4096))["xyz"]) == 1 + 4096 * 4096   # the ratio is 4096 exactly: the last that passes
        with pytest.raises(ValueError, match=r"\(-3\).*triangle 1 .*4096"):
            h.sample(np.nextafter(F(5.0) / F(4096), F(0)))
        assert len(h.sample(2.5)["xyz"]) == 1 + 4   # the handle is as it was
    big = np.tile(np.arange(1, 4, dtype=np.int32), (80, 1))
    s = int(md.subdivisions(xyz, [[1, 2, 3]], 5.0 / 4000)[0][0])   # 4000 or 4001, as 5 / 4000 rounds to fp32
    with mesh.Mesh(xyz, big) as h:   # 80 x s^2 = 1.28e9 samples
        with pytest.raises(ValueError, match=rf"\(-3\).* {80 * s * s} samples.*2\^30"):
            h.sample(5.0 / 4000)


# ---- on top of the two calls ----------------------------------------------------------------------------------------------------------------
def test_compare_and_evaluate_mesh(mesh):
    m = msc.cube(4)
    same = mesh.compare(m, m, 0.2, 0.5)
    assert same["hausdorff"] <= 1e-7 and same["a_to_b"]["beyond"] == 0 and same["a_to_b"]["n"] == len(md.sample_statement(m["xyz"], m["tri"], 0.2)["xyz"])
    delta = 0.125
    out = mesh.compare(m, dict(m, xyz=(m["xyz"] + np.array([delta, 0, 0], F)).astype(F)), 0.2, 0.5)
    assert abs(out["hausdorff"] - delta) <= 1e-6 and out["a_to_b"]["beyond"] == out["b_to_a"]["beyond"] == 0
    gt = np.concatenate([md.sample_statement(m["xyz"], m["tri"], 0.1)["xyz"], [[np.nan, 0, 0]], [[0.5, 0.5, 1.3]]]).astype(F)
    timings = {}
    res = mesh.evaluate_mesh(m, gt, [0.05, 0.2, 0.4], timings=timings)
    assert [r["n_complete"] for r in res["tolerances"]] == [len(gt) - 2, len(gt) - 2, len(gt) - 1]
    assert res["tolerances"][-1]["accuracy"] == 1.0 and res["dropped_ground_truth"] == 1 and timings["device_ms"]["distance"] > 0
    vox = mesh.evaluate_mesh(m, gt, [0.05, 0.2], voxel=0.1)
    assert vox["voxel"] == 0.1 and vox["n_reconstruction"] < vox["n_samples"]
    # the cascade resolves every point at the level a single call at that radius does
    with mesh.Mesh(m["xyz"], m["tri"]) as h:
        d = mesh.surface_distances(gt, h, [0.4, 0.05])
        want = md.distance_statement(m["xyz"], m["tri"], gt, 0.4)[0]
        assert md.same_bits(d, np.sqrt(want))
