"""The brick-sparse TSDF volume on the GPU against the numpy statements of tsdf_sparse_common.py and tsdf_common.py, bit for bit
(include/mpmvs.h, statements A and B): the allocation on lattices whose bricks are cut off by dims, on cameras
of three sizes, over two chunks of views and with the camera inside the volume; the refusal at max_bricks; the integration against
the masked dense statement and the masked dense Volume; the mesh through mpmvs_tsdf_set_bricks; and all three end to end."""
import importlib

import numpy as np
import pytest

import tsdf_common as tc
import tsdf_sparse_common as sc
from test_tsdf_gpu import _colors, _integrate_input, _sphere_depth

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def mesh(pm, engine):
    return importlib.import_module("mp-mvs_amd.mesh")


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- allocate ---------------------------------------------------------------------------------------------------------------------
def _eleven_views(pm):
    """the views of test_tsdf_gpu.py's wide volume: 11 cameras (two chunks), three image sizes, view 5 inside the volume"""
    cams, depths = [], []
    for q in range(11):
        ang = np.deg2rad(-25.0 + 5.0 * q)
        R = np.array([[np.cos(ang), 0, -np.sin(ang)], [0, 1, 0], [np.sin(ang), 0, np.cos(ang)]])
        C = np.array([0.4 * q - 2.0, 0.05 * q, 2.05 if q == 5 else -0.3])
        K = np.array([[14.0 + q, 0, 11.0], [0, 15.0, 8.0], [0, 0, 1]])
        cam = pm.make_camera(K, R, -R @ C, 16 + q % 3, 22 + q % 2, 0.1, 20.0)
        cams.append(cam)
        depths.append(_sphere_depth(cam, np.array([0.2, 0.0, 2.1]), 0.45, background=2.4))
    return cams, depths


@pytest.fixture(scope="module")
def scenes(pm):
    """name -> (dims, origin, voxel, trunc, cams, depths, colours or None).  The three cameras of test_tsdf_gpu.py (32 x 24, 24 x 32 and
    20 x 16; camera C sits inside the volume; camera A's map holds depth 0, negative, NaN and inf) see 13 x 7 x 5 (2 x 1 x 1 bricks, all
    cut off) and 17 x 17 x 9 (3 x 3 x 2 bricks, the last of each axis one voxel thick); the eleven views see 70 x 9 x 3."""
    cams, depths, cols = _integrate_input(pm)
    many, many_depths = _eleven_views(pm)
    return {"13x7x5": ((13, 7, 5), (-1.5, -0.75, 1.5), 0.25, 0.5, cams, depths, cols),
            "17x17x9": ((17, 17, 9), (-1.7, -1.7, 1.2), 0.2, 0.3, cams, depths, cols),
            "70x9x3": ((70, 9, 3), (-2.0, -0.5, 2.0), 0.0625, 0.2, many, many_depths, None)}


@pytest.mark.parametrize("pad", [0.0, 1.0, 8.0])
@pytest.mark.parametrize("name", ["13x7x5", "17x17x9", "70x9x3"])
def test_allocate_equals_the_statement(mesh, scenes, name, pad):
    dims, origin, voxel, trunc, cams, depths, _ = scenes[name]
    want = sc.allocate_statement(origin, voxel, dims, trunc, pad, cams, depths)
    first = sc.allocate_statement(origin, voxel, dims, trunc, pad, cams[:1], depths[:1])
    print(name, "pad", pad, "bricks", int(want.sum()), "of", want.size, "after the first view", int(first.sum()))
    assert want.any()
    with mesh.SparseVolume(origin, voxel, dims, trunc, pad=pad) as v:
        assert v.bricks().shape == (0, 3)
        v.allocate(cams, depths)
        assert np.array_equal(v.bricks(), sc.brick_coords(want))
        st = v.stats()
        assert st["bricks"] == int(want.sum()) and st["grid_cells"] == want.size and st["allocate_mark"] > 0.0 and st["allocate_commit"] > 0.0
        assert st["device_bytes"] == 4 * want.size + int(want.sum()) * (4 + 512 * 8)
        fresh = v.get_bricks()
        assert not fresh["sum"].any() and not fresh["weight"].any()
        v.allocate(cams, depths)   # the same views again: no change
        assert np.array_equal(v.bricks(), sc.brick_coords(want))
    with mesh.SparseVolume(origin, voxel, dims, trunc, pad=pad) as v:   # two calls against one
        v.allocate(cams[:1], depths[:1])
        assert np.array_equal(v.bricks(), sc.brick_coords(first))
        v.allocate(cams[1:], depths[1:])
        assert np.array_equal(v.bricks(), sc.brick_coords(want))


def test_allocate_refuses_above_max_bricks_and_changes_nothing(mesh, scenes):
    dims, origin, voxel, trunc, cams, depths, _ = scenes["17x17x9"]
    first = sc.allocate_statement(origin, voxel, dims, trunc, 1.0, cams[:1], depths[:1])
    want = sc.allocate_statement(origin, voxel, dims, trunc, 1.0, cams, depths)
    need = int(want.sum())
    assert 0 < first.sum() < need
    with mesh.SparseVolume(origin, voxel, dims, trunc, pad=1.0, max_bricks=need - 1) as v:
        v.allocate(cams[:1], depths[:1])
        v.integrate(cams[:1], depths[:1])
        before = v.get_bricks()
        assert before["weight"].any()
        with pytest.raises(ValueError, match="max_bricks"):
            v.allocate(cams, depths)
        after = v.get_bricks()
        assert np.array_equal(after["coords"], sc.brick_coords(first)) and np.array_equal(bits(after["sum"]), bits(before["sum"]))
        assert np.array_equal(after["weight"], before["weight"]) and v.n_bricks() == int(first.sum())
    with mesh.SparseVolume(origin, voxel, dims, trunc, pad=1.0, max_bricks=need) as v:   # exact: accepted
        v.allocate(cams, depths)
        assert v.n_bricks() == need


# ---- integrate ------------------------------------------------------------------------------------------------------------------
def _check_bricks(got, dims, bricks, want, colour):
    assert np.array_equal(got["coords"], sc.brick_coords(bricks))
    assert np.array_equal(bits(got["sum"]), bits(sc.to_bricks(dims, bricks, want[0])))
    assert np.array_equal(got["weight"], sc.to_bricks(dims, bricks, want[1]))
    if colour:
        assert np.array_equal(got["color"], sc.to_bricks(dims, bricks, want[2]))


@pytest.mark.parametrize("color", ["none", "bgr", "grey"])
@pytest.mark.parametrize("name", ["13x7x5", "17x17x9"])
def test_integrate_equals_the_masked_statement_and_the_masked_dense_volume(mesh, scenes, name, color):
    dims, origin, voxel, trunc, cams, depths, cols = scenes[name]
    images = None if color == "none" else cols if color == "bgr" else [c[..., 1].copy() for c in cols]
    bricks = sc.allocate_statement(origin, voxel, dims, trunc, 1.0, cams[:2], depths[:2])   # not every brick: views 0 and 1 only
    assert bricks.any() and (name == "13x7x5" or not bricks.all())
    dense = tc.integrate_statement(origin, voxel, dims, trunc, cams, depths, images)
    want = sc.mask_dense(dims, bricks, *dense)
    assert (want[1] > 0).any() and (name == "13x7x5" or (dense[1] != want[1]).any())   # the mask cuts observations away
    with mesh.Volume(origin, voxel, dims, trunc, color=images is not None) as d:
        d.integrate(cams, depths, images)
        on_gpu = d.get()
    gpu_masked = sc.mask_dense(dims, bricks, on_gpu["sum"], on_gpu["weight"], on_gpu.get("color"))
    for split in (None, 1, 2):
        with mesh.SparseVolume(origin, voxel, dims, trunc, color=images is not None, pad=1.0) as v:
            v.allocate(cams[:2], depths[:2])
            if split is None:
                v.integrate(cams, depths, images)
            else:
                v.integrate(cams[:split], depths[:split], None if images is None else images[:split])
                v.integrate(cams[split:], depths[split:], None if images is None else images[split:])
            got = v.get_bricks()
            back = v.to_dense()
            assert v.pass_ms()["integrate"] > 0.0
        _check_bricks(got, dims, bricks, want, images is not None)
        _check_bricks(got, dims, bricks, gpu_masked, images is not None)
        assert np.array_equal(bits(back["sum"]), bits(want[0])) and np.array_equal(back["weight"], want[1])


def test_integrate_many_views_into_a_wide_volume(mesh, scenes):
    dims, origin, voxel, trunc, cams, depths, _ = scenes["70x9x3"]
    bricks = sc.allocate_statement(origin, voxel, dims, trunc, 0.0, cams[:3], depths[:3])
    want = sc.mask_dense(dims, bricks, *tc.integrate_statement(origin, voxel, dims, trunc, cams, depths))
    assert bricks.any() and not bricks.all() and want[1].max() >= 4
    with mesh.SparseVolume(origin, voxel, dims, trunc, pad=0.0) as v:
        v.allocate(cams[:3], depths[:3])
        v.integrate(cams, depths)
        _check_bricks(v.get_bricks(), dims, bricks, want, False)


def test_allocate_after_integrate_keeps_old_bricks_and_zeroes_new_ones(mesh, scenes):
    dims, origin, voxel, trunc, cams, depths, cols = scenes["17x17x9"]
    b1 = sc.allocate_statement(origin, voxel, dims, trunc, 0.0, cams[:1], depths[:1])
    b2 = sc.allocate_statement(origin, voxel, dims, trunc, 0.0, cams, depths, bricks=b1)
    coords1, coords2 = sc.brick_coords(b1).tolist(), sc.brick_coords(b2).tolist()
    assert 0 < b1.sum() < b2.sum() and coords2[:len(coords1)] != coords1   # a new brick sorts before an old one: the old ones move
    s1 = sc.mask_dense(dims, b1, *tc.integrate_statement(origin, voxel, dims, trunc, cams[:2], depths[:2], cols[:2]))
    want = sc.mask_dense(dims, b2, *tc.integrate_statement(origin, voxel, dims, trunc, cams[2:], depths[2:], cols[2:], state=s1))
    with mesh.SparseVolume(origin, voxel, dims, trunc, color=True, pad=0.0) as v:
        v.allocate(cams[:1], depths[:1])
        v.integrate(cams[:2], depths[:2], cols[:2])
        _check_bricks(v.get_bricks(), dims, b1, s1, True)
        v.allocate(cams, depths)
        mid = v.get_bricks()
        _check_bricks(mid, dims, b2, s1, True)   # old bricks carried over, new ones zero
        v.integrate(cams[2:], depths[2:], cols[2:])
        _check_bricks(v.get_bricks(), dims, b2, want, True)


# ---- mesh through set_bricks ------------------------------------------------------------------------------------------------------
def _all(dims):
    bx, by, bz = sc.brick_grid(dims)
    return np.ones((bz, by, bx), bool)


def _without(dims, *coords):
    b = _all(dims)
    for I, J, K in coords:
        b[K, J, I] = False
    return b


def _only(dims, *coords):
    return ~_without(dims, *coords)


def _mesh_cases():
    cases = {}
    A = (10, 9, 8)
    f, w = tc.sphere_volume(A, (4.3, 3.9, 3.4), 2.7)
    cases["anchor"] = (A, f, w, None, 1, _all(A))
    cases["anchor_colour"] = (A, f, w, _colors(A, 1, (slice(2, 6), slice(2, 6), slice(4, 9))), 1, _all(A))
    cases["anchor_one_brick_removed"] = (A, f, w, None, 1, _without(A, (1, 1, 0)))
    S, centre, radius = sc.SHIFTED
    fs, ws = tc.sphere_volume(S, centre, radius)
    cases["shifted"] = (S, fs, ws, _colors(S, 7), 1, _all(S))
    cases["shifted_one_brick_removed"] = (S, fs, ws, _colors(S, 7), 1, _without(S, (1, 1, 0)))
    cases["shifted_upper_layer_removed"] = (S, fs, ws, None, 1, _without(S, *[(I, J, 1) for I in range(3) for J in range(3)]))
    f0, w0 = tc.sphere_volume((7, 7, 7), (3, 3, 3), 2.0)
    cases["exact_zeros"] = ((7, 7, 7), f0, w0, _colors((7, 7, 7), 2), 1, _all((7, 7, 7)))
    wh = ws.copy()
    wh[2:5, 6:10, 7:12] = 0
    wh[0, 0, 0] = -3
    wh[3, 8, 8] = -1
    cases["holes_and_negative_weights"] = (S, fs, wh, _colors(S, 3), 1, _all(S))
    rng = np.random.default_rng(4)
    wm = rng.integers(1, 4, ws.shape).astype(np.int32)
    for mw in (1, 2, 3):
        cases[f"min_weight_{mw}"] = (S, (fs * wm.astype(F)).astype(F), wm, None, mw, _without(S, (0, 1, 0)))
    B = (20, 20, 20)
    fb, wb = tc.sphere_volume(B, (4.2, 4.1, 3.9), 3.5)   # reaches i = 7.7: cells whose far corners lie in bricks that do not exist
    cases["single_brick_empty_neighbours"] = (B, fb, wb, None, 1, _only(B, (0, 0, 0)))
    cases["single_inner_brick"] = (B, tc.sphere_volume(B, (11.5, 11.5, 11.5), 3.0)[0], wb, None, 1, _only(B, (1, 1, 1)))
    cases["nz_1"] = ((10, 9, 1), f[:1].copy(), w[:1].copy(), None, 1, _all((10, 9, 1)))
    cases["nothing_valid"] = (S, fs, np.zeros_like(ws), None, 1, _all(S))
    fw, ww = tc.sphere_volume((130, 129, 2), (64.5, 63.2, 0.4), 50.3)
    cases["130x129x2"] = ((130, 129, 2), fw, ww, None, 1, _all((130, 129, 2)))   # 17 x 17 x 1 bricks, 578 scan tiles: the scan carries
    cases["zero_bricks"] = (S, fs, ws, None, 1, ~_all(S))
    return cases


MESH_CASES = _mesh_cases()
MESH_ORIGIN, MESH_VOXEL = (0.25, -1.5, 3.0), 0.375
EMPTY = ("nz_1", "nothing_valid", "zero_bricks")


def _brick_arrays(dims, bricks, total, weight, color4, garbage):
    """what set_bricks takes; with `garbage` the entries of cut-off voxels are filled with values that would change the mesh"""
    masked = sc.mask_dense(dims, bricks, total, weight, color4)
    s, w = sc.to_bricks(dims, bricks, masked[0]), sc.to_bricks(dims, bricks, masked[1])
    c = None if color4 is None else sc.to_bricks(dims, bricks, masked[2])
    if garbage:
        cut = ~sc.to_bricks(dims, bricks, np.ones(dims[::-1], bool))
        s, w = np.where(cut, F(-1.5), s).astype(F), np.where(cut, 5, w).astype(np.int32)
        if c is not None:
            c = np.where(cut[..., None], 9, c).astype(np.uint32)
    return masked, s, w, c


@pytest.mark.parametrize("name", list(MESH_CASES))
def test_mesh_equals_the_masked_statement(mesh, name):
    dims, total, weight, color4, min_weight, bricks = MESH_CASES[name]
    masked, s, w, c = _brick_arrays(dims, bricks, total, weight, color4, garbage=True)
    want = sc.sparse_mesh_statement(total, weight, color4, dims, MESH_ORIGIN, MESH_VOXEL, bricks, min_weight)
    dense = tc.mesh_statement(total, weight, color4, dims, MESH_ORIGIN, MESH_VOXEL, min_weight)
    with mesh.SparseVolume(MESH_ORIGIN, MESH_VOXEL, dims, 1.0, color=color4 is not None) as v:
        v.set_bricks(sc.brick_coords(bricks), s, w, c)
        _check_bricks(v.get_bricks(), dims, bricks, masked, color4 is not None)   # cut-off entries were stored as 0
        got = v.mesh(min_weight)
        again = v.mesh(min_weight)
        ms = v.pass_ms()
    print(name, "bricks", int(bricks.sum()), "vertices", len(want["xyz"]), "triangles", len(want["tri"]), "dense", len(dense["tri"]), ms)
    assert got["xyz"].shape == want["xyz"].shape and np.array_equal(bits(got["xyz"]), bits(want["xyz"]))
    assert got["tri"].shape == want["tri"].shape and np.array_equal(got["tri"], want["tri"])
    if color4 is None:
        assert got["rgb"] is None
    else:
        assert np.array_equal(got["rgb"], want["rgb"])
    for key in ("xyz", "tri"):
        assert np.array_equal(again[key], got[key])
    assert sc.triangle_set(got) <= sc.triangle_set(dense)   # a sub-mesh of the dense mesh: never a different triangle
    if name in EMPTY:
        assert len(got["xyz"]) == 0 and len(got["tri"]) == 0 and ms["vertices"] == 0.0 and ms["triangles"] == 0.0
        assert name == "nothing_valid" or ms["mark"] == 0.0
    else:
        assert len(got["tri"]) > 0 and ms["mark"] > 0.0 and ms["triangles"] > 0.0
    topo = tc.topology(got["tri"])
    if name in ("anchor", "anchor_colour", "anchor_one_brick_removed"):   # every owner of the anchor lies in brick (0, 0, 0)
        assert (topo["V"], topo["E"], topo["F"]) == (410, 1224, 816) and topo["closed"] and topo["euler"] == 2
    if name == "130x129x2":   # open at the top layer, like the dense case
        assert len(got["tri"]) == len(dense["tri"]) == 2744 and topo["manifold_with_boundary"]
    if name in ("shifted", "exact_zeros", "single_inner_brick"):
        assert topo["closed"] and topo["euler"] == 2 and len(got["tri"]) == len(dense["tri"]) and tc.signed_volume(got["xyz"], got["tri"]) > 0
    if name in ("shifted_one_brick_removed", "shifted_upper_layer_removed", "single_brick_empty_neighbours"):
        assert topo["manifold_with_boundary"] and not topo["closed"] and 0 < len(got["tri"]) < len(dense["tri"])
        assert sc.triangle_set(got) < sc.triangle_set(dense)


def test_set_bricks_replaces_the_volume_and_clears_colour(mesh):
    dims, total, weight, color4, _, bricks = MESH_CASES["shifted"]
    _, s, w, c = _brick_arrays(dims, bricks, total, weight, color4, garbage=False)
    with mesh.SparseVolume(MESH_ORIGIN, MESH_VOXEL, dims, 1.0, color=True) as v:
        v.set_bricks(sc.brick_coords(bricks), s, w, c)
        v.set_bricks(sc.brick_coords(bricks), s, w, None)   # clears the colour sums
        got = v.mesh()
        assert len(got["rgb"]) > 0 and (got["rgb"] == 128).all()
        few = _only(dims, (0, 0, 0), (1, 1, 0))
        _, s2, w2, _ = _brick_arrays(dims, few, total, weight, None, garbage=False)
        v.set_bricks(sc.brick_coords(few), s2, w2)
        assert v.n_bricks() == 2 and np.array_equal(v.get_bricks()["weight"], w2)
        v.set_bricks(np.zeros((0, 3), np.int32), np.zeros(0, F), np.zeros(0, np.int32))
        assert v.n_bricks() == 0 and len(v.mesh()["tri"]) == 0


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def test_sphere_from_four_cameras_end_to_end(mesh, pm):
    dims, origin, voxel, trunc, cams, depths, cols = sc.sphere_scene(pm)
    bricks = sc.allocate_statement(origin, voxel, dims, trunc, 1.0, cams, depths)
    dense_vol = tc.integrate_statement(origin, voxel, dims, trunc, cams, depths, cols)
    want_vol = sc.mask_dense(dims, bricks, *dense_vol)
    want = sc.sparse_mesh_statement(*dense_vol, dims, origin, voxel, bricks, 1)
    band = sc.band_voxels(origin, voxel, dims, trunc, cams, depths)
    with mesh.SparseVolume(origin, voxel, dims, trunc, color=True, pad=1.0) as v:
        v.allocate(cams, depths)
        v.integrate(cams[:2], depths[:2], cols[:2])
        v.integrate(cams[2:], depths[2:], cols[2:])
        vol = v.get_bricks()
        got = v.mesh(1)
        st = v.stats()
    with mesh.Volume(origin, voxel, dims, trunc, color=True) as d:
        d.integrate(cams, depths, cols)
        dense = d.mesh(1)
    _check_bricks(vol, dims, bricks, want_vol, True)
    assert np.array_equal(bits(got["xyz"]), bits(want["xyz"])) and np.array_equal(got["tri"], want["tri"]) and np.array_equal(got["rgb"], want["rgb"])
    print("end to end:", st, "triangles", len(got["tri"]), "dense", len(dense["tri"]), "band voxels", int(band.sum()))
    assert sc.triangle_set(got) <= sc.triangle_set(dense) and len(got["tri"]) > 500
    assert tc.topology(got["tri"])["manifold_with_boundary"]
    # the cap on the scene: every band voxel lies in an allocated brick
    assert band.any() and not (band & ~sc.voxel_exists(dims, sc.bricks_from_coords(dims, vol["coords"]))).any()
