"""mpmvs_tsdf_integrate and mpmvs_tsdf_mesh on the GPU against the numpy statements of tsdf_common.py, bit for bit (include/mpmvs.h,
DESIGN.md section 22): the integration on an input built to sit on every branch of the statement, the mesh through mpmvs_tsdf_set
on lattices that cross a wave, a block and a scan tile, and both end to end."""
import importlib

import numpy as np
import pytest

import tsdf_common as tc

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def mesh(pm, engine):
    return importlib.import_module("mp-mvs_amd.mesh")


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- integrate ------------------------------------------------------------------------------------------------------------------
DIMS, ORIGIN, VOXEL, TRUNC = (13, 7, 5), (-1.5, -0.75, 1.5), 0.25, 0.5


def _integrate_input(pm):
    """Volume 13 x 7 x 5 with P = (-1.5 + i/4, -0.75 + j/4, 1.5 + k/4).  Camera A (32 x 24) sits at the origin and looks along +z with
    f = 32 and the principal point (15.5, 11.5): in layer k = 2 (Pz = 2) fu = 16 Px + 16, so i = 2 lands on fu = 0 exactly and i = 10 on
    fu = W = 32 exactly.  Its depth map is the plane d = 10 (s > trunc: clamped to 1, no colour) with planted pixels.  Camera B (24 x 32)
    looks from the side at a sphere.  Camera C (20 x 16) sits inside the volume at z = 2.1: the layers k <= 2 are behind it."""
    KA = np.array([[32.0, 0, 15.5], [0, 32.0, 11.5], [0, 0, 1]])
    camA = pm.make_camera(KA, np.eye(3), np.zeros(3), 24, 32, 0.5, 20.0)
    dA = np.full((24, 32), 10.0, F)
    # the voxel (6, 3, 2) = (0, 0, 2) lands on pixel (16, 12); d = z - trunc gives s == -trunc exactly: kept, adds -1
    dA[12, 16] = F(1.5)
    # its neighbour (7, 3, 2) = (.25, 0, 2) lands on (20, 12); one ulp less depth gives s < -trunc: skipped
    dA[12, 20] = np.nextafter(F(1.5), F(0))
    # (5, 3, 2) -> (12, 12): inside the band, negative; (6, 2, 2) -> (16, 8): inside the band, positive, with colour
    dA[12, 12] = F(1.75)
    dA[8, 16] = F(2.25)
    # depth 0, negative, NaN and inf under voxels of layer k = 2 (fv = 16 Py + 12: j = 4 -> row 16, j = 5 -> row 20)
    dA[16, 16], dA[16, 20], dA[20, 16], dA[20, 20] = 0.0, -3.0, np.nan, np.inf
    ang = np.deg2rad(35.0)
    RB = np.array([[np.cos(ang), 0, -np.sin(ang)], [0, 1, 0], [np.sin(ang), 0, np.cos(ang)]])
    CB = np.array([2.0, 0.1, -0.6])
    KB = np.array([[21.0, 0, 12.3], [0, 19.0, 15.7], [0, 0, 1]])
    camB = pm.make_camera(KB, RB, -RB @ CB, 32, 24, 0.5, 20.0)
    dB = _sphere_depth(camB, np.array([0.1, 0.0, 2.0]), 0.55, background=0.0)
    KC = np.array([[9.0, 0, 9.5], [0, 9.0, 7.5], [0, 0, 1]])
    CC = np.array([0.05, -0.02, 2.1])
    camC = pm.make_camera(KC, np.eye(3), -CC, 16, 20, 0.05, 20.0)
    v, u = np.meshgrid(np.arange(16, dtype=np.float64), np.arange(20, dtype=np.float64), indexing="ij")
    dC = (0.3 + 0.01 * u + 0.005 * v).astype(F)   # a slanted plane close to the camera
    rng = np.random.default_rng(5)
    cols = [rng.integers(0, 256, d.shape + (3,), dtype=np.uint8) for d in (dA, dB, dC)]
    return [camA, camB, camC], [dA, dB, dC], cols


def _sphere_depth(cam, centre, radius, background):
    """depth along the camera's z axis of the sphere's near side per pixel centre, fp64 -> fp32; `background` elsewhere"""
    K, R, t = np.array(cam.K, np.float64).reshape(3, 3), np.array(cam.R, np.float64).reshape(3, 3), np.array(cam.t, np.float64)
    W, H = int(cam.width), int(cam.height)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ray = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], -1)   # camera frame, z = 1
    c = R @ centre + t
    a, b, cc = (ray * ray).sum(-1), -2.0 * (ray @ c), float(c @ c) - radius * radius
    disc = b * b - 4 * a * cc
    with np.errstate(invalid="ignore"):
        lam = (-b - np.sqrt(disc)) / (2 * a)
    return np.where((disc > 0) & (lam > 0), lam, background).astype(F)


@pytest.fixture(scope="module")
def integrate_input(pm):
    return _integrate_input(pm)


def test_integrate_input_sits_on_every_branch(integrate_input):
    """the input has what the contract's branches need (checked on the statement, once, without the device)"""
    cams, depths, cols = integrate_input
    px, py, pz = tc.positions(ORIGIN, VOXEL, DIMS)
    Pz, Py, Px = np.meshgrid(pz, py, px, indexing="ij")
    z, fu, fv = tc.project(cams[0], Px, Py, Pz)
    assert fu[2, 3, 2] == 0.0 and fu[2, 3, 10] == 32.0 and (fu[2] < 0).any()          # the borders fu = 0 and fu = W, and beyond
    zc = tc.project(cams[2], Px, Py, Pz)[0]
    assert (zc < 0).any() and (zc > 0).any()                                           # voxels behind camera C
    s, w, c = tc.integrate_statement(ORIGIN, VOXEL, DIMS, TRUNC, cams[:1], depths[:1], cols[:1])
    assert w[2, 3, 2] == 1 and w[2, 3, 10] == 0 and w[2, 3, 1] == 0
    assert w[2, 3, 6] == 1 and s[2, 3, 6] == -1.0 and c[2, 3, 6, 3] == 1               # s == -trunc: kept, and within the colour band
    assert F(depths[0][12, 20]) - F(2.0) < -F(TRUNC) and w[2, 3, 7] == 0               # one ulp below: skipped
    assert s[2, 3, 5] == -0.5 and s[2, 2, 6] == 0.5 and c[2, 2, 6, 3] == 1 and c[2, 2, 6, :3].tolist() == cols[0][8, 16].tolist()
    assert w[2, 4, 6] == 0 and w[2, 4, 7] == 0 and w[2, 5, 6] == 0 and w[2, 5, 7] == 0  # depth 0, negative, NaN, inf
    assert s[2, 0, 6] == 1.0 and w[2, 0, 6] == 1 and c[2, 0, 6, 3] == 0               # s > trunc: clamped to 1, no colour
    full = tc.integrate_statement(ORIGIN, VOXEL, DIMS, TRUNC, cams, depths, cols)
    assert full[1].max() >= 2 and ((full[0] < 0) & (full[1] > 0)).any() and (full[1] == 0).any()


@pytest.mark.parametrize("color", ["none", "bgr", "grey"])
def test_integrate_equals_the_statement(mesh, integrate_input, color):
    cams, depths, cols = integrate_input
    images = None if color == "none" else cols if color == "bgr" else [c[..., 1].copy() for c in cols]
    want = tc.integrate_statement(ORIGIN, VOXEL, DIMS, TRUNC, cams, depths, images)
    print("observations", int(want[1].sum()), "voxels seen", int((want[1] > 0).sum()), "of", want[1].size)
    for split in (None, 1, 2):   # one call, and two calls with the list split
        with mesh.Volume(ORIGIN, VOXEL, DIMS, TRUNC, color=images is not None) as v:
            fresh = v.get()
            assert not fresh["sum"].any() and not fresh["weight"].any() and (images is None or not fresh["color"].any())
            if split is None:
                v.integrate(cams, depths, images)
            else:
                v.integrate(cams[:split], depths[:split], None if images is None else images[:split])
                v.integrate(cams[split:], depths[split:], None if images is None else images[split:])
            got = v.get()
            assert v.pass_ms()["integrate"] > 0.0
        assert np.array_equal(bits(got["sum"]), bits(want[0])), split
        assert np.array_equal(got["weight"], want[1]), split
        if images is not None:
            assert np.array_equal(got["color"], want[2]), split


def test_integrate_wide_volume_and_many_views(mesh, pm):
    """70 x 9 x 3: more than one tile along x and y; 11 views: more than one chunk, a different camera each"""
    dims, origin, voxel, trunc = (70, 9, 3), (-2.0, -0.5, 2.0), 0.0625, 0.2
    cams, depths, cols = [], [], []
    rng = np.random.default_rng(9)
    for q in range(11):
        ang = np.deg2rad(-25.0 + 5.0 * q)
        R = np.array([[np.cos(ang), 0, -np.sin(ang)], [0, 1, 0], [np.sin(ang), 0, np.cos(ang)]])
        C = np.array([0.4 * q - 2.0, 0.05 * q, 2.05 if q == 5 else -0.3])   # view 5 sits inside the volume
        K = np.array([[14.0 + q, 0, 11.0], [0, 15.0, 8.0], [0, 0, 1]])
        cam = pm.make_camera(K, R, -R @ C, 16 + q % 3, 22 + q % 2, 0.1, 20.0)
        cams.append(cam)
        depths.append(_sphere_depth(cam, np.array([0.2, 0.0, 2.1]), 0.45, background=2.4))
        cols.append(rng.integers(0, 256, depths[-1].shape, dtype=np.uint8))
    want = tc.integrate_statement(origin, voxel, dims, trunc, cams, depths, cols)
    with mesh.Volume(origin, voxel, dims, trunc, color=True) as v:
        v.integrate(cams, depths, cols)
        got = v.get()
    assert want[1].max() >= 4 and (want[1] == 0).any()
    assert np.array_equal(bits(got["sum"]), bits(want[0])) and np.array_equal(got["weight"], want[1]) and np.array_equal(got["color"], want[2])


# ---- mesh through set -------------------------------------------------------------------------------------------------------------
def _colors(dims, seed, empty_block=None):
    """random colour sums with counts 0..3 (a quarter of the voxels has no colour), and a block without any"""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    cnt = rng.integers(0, 4, (nz, ny, nx)).astype(np.uint32)
    c4 = np.empty((nz, ny, nx, 4), np.uint32)
    for c in range(3):
        c4[..., c] = rng.integers(0, 256, (nz, ny, nx)).astype(np.uint32) * cnt
    c4[..., 3] = cnt
    if empty_block is not None:
        c4[empty_block] = 0
    return c4


def _mesh_cases():
    cases = {}
    f, w = tc.sphere_volume((10, 9, 8), (4.3, 3.9, 3.4), 2.7)
    cases["anchor"] = ((10, 9, 8), f, w, None, 1)
    # one-corner and no-corner colour: a block of voxels without colour across the surface
    cases["anchor_colour"] = ((10, 9, 8), f, w, _colors((10, 9, 8), 1, (slice(2, 6), slice(2, 6), slice(4, 9))), 1)
    f0, w0 = tc.sphere_volume((7, 7, 7), (3, 3, 3), 2.0)
    cases["exact_zeros"] = ((7, 7, 7), f0, w0, _colors((7, 7, 7), 2), 1)
    wh = w.copy()
    wh[2:5, 3:6, 5:9] = 0
    wh[0, 0, 0] = -3
    cases["holes"] = ((10, 9, 8), f, wh, _colors((10, 9, 8), 3), 1)
    rng = np.random.default_rng(4)
    wm = rng.integers(1, 4, w.shape).astype(np.int32)
    for mw in (1, 2, 3):
        cases[f"min_weight_{mw}"] = ((10, 9, 8), (f * wm.astype(F)).astype(F), wm, None, mw)
    cases["nz_1"] = ((10, 9, 1), f[:1].copy(), w[:1].copy(), None, 1)
    cases["constant_sign"] = ((10, 9, 8), np.abs(f) + F(0.5), w, None, 1)
    cases["nothing_valid"] = ((10, 9, 8), f, np.zeros_like(w), None, 1)
    fw, ww = tc.sphere_volume((70, 3, 3), (34.5, 1.2, 0.9), 30.3)
    cases["70x3x3"] = ((70, 3, 3), fw, ww, _colors((70, 3, 3), 5), 1)
    fs, ws = tc.sphere_volume((130, 129, 2), (64.5, 63.2, 0.4), 50.3)
    cases["130x129x2"] = ((130, 129, 2), fs, ws, None, 1)
    # 298 scan tiles: the scan of the tile totals takes a second round with a carry
    fc, wc = tc.sphere_volume((70, 33, 33), (34.5, 16.2, 15.9), 12.3)
    cases["70x33x33"] = ((70, 33, 33), fc, wc, None, 1)
    fo, wo = tc.sphere_volume((13, 7, 5), (6.2, 3.1, 2.1), 1.6)
    cases["13x7x5"] = ((13, 7, 5), fo, wo, _colors((13, 7, 5), 6), 1)
    return cases


MESH_CASES = _mesh_cases()
MESH_ORIGIN, MESH_VOXEL = (0.25, -1.5, 3.0), 0.375


@pytest.mark.parametrize("name", list(MESH_CASES))
def test_mesh_equals_the_statement(mesh, name):
    dims, total, weight, color4, min_weight = MESH_CASES[name]
    want = tc.mesh_statement(total, weight, color4, dims, MESH_ORIGIN, MESH_VOXEL, min_weight)
    with mesh.Volume(MESH_ORIGIN, MESH_VOXEL, dims, 1.0, color=color4 is not None) as v:
        v.set(total, weight, color4)
        back = v.get()
        assert back["sum"].tobytes() == np.ascontiguousarray(total, F).tobytes() and back["weight"].tobytes() == np.ascontiguousarray(weight, np.int32).tobytes()
        assert color4 is None or back["color"].tobytes() == color4.tobytes()
        got = v.mesh(min_weight)
        again = v.mesh(min_weight)
        ms = v.pass_ms()
    print(name, "vertices", len(want["xyz"]), "triangles", len(want["tri"]), ms)
    assert got["xyz"].shape == want["xyz"].shape and np.array_equal(bits(got["xyz"]), bits(want["xyz"]))   # vertex order and positions
    assert got["tri"].shape == want["tri"].shape and np.array_equal(got["tri"], want["tri"])               # order, rotation, winding
    if color4 is None:
        assert got["rgb"] is None
    else:
        assert np.array_equal(got["rgb"], want["rgb"])
    for key in ("xyz", "tri"):
        assert np.array_equal(again[key], got[key])
    if name in ("nz_1", "constant_sign", "nothing_valid"):
        assert len(got["xyz"]) == 0 and len(got["tri"]) == 0
        assert ms["vertices"] == 0.0 and ms["triangles"] == 0.0 and (name != "nz_1" or ms["mark"] == 0.0)
    else:
        assert len(got["tri"]) > 0 and ms["mark"] > 0.0 and ms["triangles"] > 0.0
    if name == "anchor":
        topo = tc.topology(got["tri"])
        assert (topo["V"], topo["E"], topo["F"]) == (410, 1224, 816) and topo["closed"] and topo["euler"] == 2
    if name == "anchor_colour":   # all three colour rules occur
        assert (want["rgb"] == 128).all(1).any() and len(np.unique(want["rgb"])) > 50
    if name in ("exact_zeros", "13x7x5", "70x33x33"):
        topo = tc.topology(got["tri"])
        assert topo["closed"] and topo["euler"] == 2 and tc.signed_volume(got["xyz"], got["tri"]) > 0


def test_colour_of_a_volume_set_without_colours_is_grey(mesh):
    dims, total, weight, _, _ = MESH_CASES["anchor"]
    with mesh.Volume(MESH_ORIGIN, MESH_VOXEL, dims, 1.0, color=True) as v:
        v.set(total, weight, _colors(dims, 8))
        v.set(total, weight, None)   # clears the colour sums
        got = v.mesh()
    assert len(got["rgb"]) == 410 and (got["rgb"] == 128).all()


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def test_sphere_from_four_cameras_end_to_end(mesh, pm):
    dims, origin, voxel, trunc = (24, 24, 24), (-0.6, -0.6, 1.4), 0.05, 0.15
    centre, radius = np.array([0.0, 0.0, 2.0]), 0.4
    cams, depths, cols = [], [], []
    for q, (cx, cy) in enumerate(((-0.9, 0.0), (0.9, 0.1), (0.0, -0.9), (0.1, 0.9))):
        C = np.array([cx, cy, 0.2])
        zax = (centre - C) / np.linalg.norm(centre - C)
        xax = np.cross([0.0, 1.0, 0.0] if abs(zax[1]) < 0.5 else [1.0, 0.0, 0.0], zax)
        xax /= np.linalg.norm(xax)
        R = np.stack([xax, np.cross(zax, xax), zax])
        K = np.array([[70.0, 0, 39.5], [0, 70.0, 29.5], [0, 0, 1]])
        cam = pm.make_camera(K, R, -R @ C, 60, 80, 0.5, 20.0)
        cams.append(cam)
        depths.append(_sphere_depth(cam, centre, radius, background=0.0))
        cols.append(np.full(depths[-1].shape + (3,), (40 * q, 255 - 60 * q, 90), np.uint8))
    want_vol = tc.integrate_statement(origin, voxel, dims, trunc, cams, depths, cols)
    want = tc.mesh_statement(want_vol[0], want_vol[1], want_vol[2], dims, origin, voxel, 1)
    with mesh.Volume(origin, voxel, dims, trunc, color=True) as v:
        v.integrate(cams[:2], depths[:2], cols[:2])
        v.integrate(cams[2:], depths[2:], cols[2:])
        vol = v.get()
        got = v.mesh(1)
    assert np.array_equal(bits(vol["sum"]), bits(want_vol[0])) and np.array_equal(vol["weight"], want_vol[1]) and np.array_equal(vol["color"], want_vol[2])
    assert np.array_equal(bits(got["xyz"]), bits(want["xyz"])) and np.array_equal(got["tri"], want["tri"]) and np.array_equal(got["rgb"], want["rgb"])
    topo = tc.topology(got["tri"])
    print("end to end:", topo, "weights", np.bincount(want_vol[1].reshape(-1)).tolist())
    assert (want_vol[1] == 0).any() and topo["F"] > 500
    assert topo["manifold_with_boundary"]   # no directed half-edge repeats, so every half-edge has at most one opposite
    # the surface lies on the sphere to within a voxel
    r = np.linalg.norm(got["xyz"].astype(np.float64) - centre, axis=1)
    assert np.abs(r - radius).max() < voxel
