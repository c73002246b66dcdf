"""mpmvs_tsdf_* without a GPU: the symbols, the refusals that need no device (mpmvs_tsdf_create touches none, so a live handle can be
refused here too), the numpy statement of tsdf_common.py against expectations written out by hand, and the PLY round trip."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import tsdf_common as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mpmvs_tsdf_create", "mpmvs_tsdf_integrate", "mpmvs_tsdf_get", "mpmvs_tsdf_set", "mpmvs_tsdf_mesh", "mpmvs_tsdf_pass_ms", "mpmvs_tsdf_destroy")
_P = C.c_void_p


@pytest.fixture(scope="module")
def eng(pm):
    return importlib.import_module("mp-mvs_amd.engine")


@pytest.fixture(scope="module")
def mesh(pm):
    return importlib.import_module("mp-mvs_amd.mesh")


def test_symbols_declared_exported_and_bound(eng):
    header = open(os.path.join(ROOT, "include", "mpmvs.h")).read()
    declared = set(re.findall(r"\b(mpmvs_[a-z0-9_]+)\s*\(", header))
    lib, fns = eng.load()
    lib_q8, fns_q8 = eng.load_variant(eng.LIB_Q8_PATH)
    for name in NEW:
        assert name in declared and name in eng.ALL_SYMBOLS
        assert hasattr(lib, name) and hasattr(lib_q8, name)
        assert name[len("mpmvs_"):] in fns and name[len("mpmvs_"):] in fns_q8
    f = fns["tsdf_create"]
    assert f.restype is C.c_int and f.argtypes == [C.c_int, C.POINTER(C.c_float), C.c_float, C.POINTER(C.c_int), C.c_float, C.c_int, C.POINTER(_P)]
    f = fns["tsdf_integrate"]
    assert f.restype is C.c_int and f.argtypes == [_P, C.c_int, _P, _P, _P, C.c_int]
    for name in ("tsdf_get", "tsdf_set"):
        assert fns[name].restype is C.c_int and fns[name].argtypes == [_P, _P, _P, _P]
    f = fns["tsdf_mesh"]
    assert f.restype is C.c_longlong and f.argtypes == [_P, C.c_int, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_longlong)]
    f = fns["tsdf_pass_ms"]
    assert f.restype is C.c_int and f.argtypes == [_P, C.POINTER(C.c_float)]
    assert fns["tsdf_destroy"].restype is None and fns["tsdf_destroy"].argtypes == [_P]
    csrc = os.path.join(ROOT, "mp-mvs_amd", "csrc")
    assert '#include "pm_tsdf.hpp"' in open(os.path.join(csrc, "mpmvs_mesh.hip")).read()
    assert re.search(r"^TUS\s*=.*\bmpmvs_mesh\b", open(os.path.join(csrc, "Makefile")).read(), re.M)


def _create(fns, dims=(4, 3, 2), voxel=0.5, trunc=1.0, color=0, origin=(0.0, 0.0, 0.0)):
    h = _P(0x1234)   # a marker: a refused create must leave it
    rc = fns["tsdf_create"](0, (C.c_float * 3)(*origin), voxel, (C.c_int * 3)(*dims), trunc, color, C.byref(h))
    return rc, h


def test_create_refusals_need_no_device(eng):
    _, fns = eng.load()
    bad = [dict(dims=(0, 3, 2)), dict(dims=(4, -1, 2)), dict(dims=(4, 3, 0)), dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=float("nan")),
           dict(voxel=float("inf")), dict(trunc=0.0), dict(trunc=-2.0), dict(trunc=float("nan")), dict(trunc=float("inf")),
           dict(origin=(0.0, float("nan"), 0.0)), dict(origin=(3e38, 0.0, 0.0), dims=(1000, 2, 2), voxel=1e36)]
    for kw in bad:
        rc, h = _create(fns, **kw)
        assert rc == -2 and h.value == 0x1234, kw
        assert "tsdf create" in fns["last_error"](None).decode()
    for dims in ((1025, 1024, 1024), (1 << 16, 1 << 16, 1), (1 << 30, 2, 1), (2147483647, 2147483647, 2147483647)):
        rc, h = _create(fns, dims=dims)
        assert rc == -3 and h.value == 0x1234, dims
        assert "2^30" in fns["last_error"](None).decode()
    assert fns["tsdf_create"](0, (C.c_float * 3)(), 0.5, (C.c_int * 3)(2, 2, 2), 1.0, 0, None) == -2
    rc, h = _create(fns, dims=(1 << 10, 1 << 10, 1 << 10))   # exactly 2^30 voxels: a handle, and still no device
    assert rc == 0 and h.value not in (None, 0x1234)
    fns["tsdf_destroy"](h)
    fns["tsdf_destroy"](None)


def test_null_handle_is_minus_2_and_writes_nothing(eng):
    _, fns = eng.load()
    s, w = np.full(4, 7, np.float32), np.full(4, 7, np.int32)
    assert fns["tsdf_integrate"](None, 0, None, None, None, 0) == -2 and "tsdf integrate" in fns["last_error"](None).decode()
    assert fns["tsdf_get"](None, s.ctypes.data, w.ctypes.data, None) == -2 and "tsdf get" in fns["last_error"](None).decode()
    assert fns["tsdf_set"](None, s.ctypes.data, w.ctypes.data, None) == -2
    px, pt, nt = _P(0x55), _P(0x66), C.c_longlong(77)
    assert fns["tsdf_mesh"](None, 1, C.byref(px), None, C.byref(pt), C.byref(nt)) == -2 and "tsdf mesh" in fns["last_error"](None).decode()
    assert (px.value, pt.value, nt.value) == (0x55, 0x66, 77) and (s == 7).all() and (w == 7).all()
    ms = (C.c_float * 5)(*([7.0] * 5))
    assert fns["tsdf_pass_ms"](None, ms) == -2 and list(ms) == [7.0] * 5


def test_live_handle_refusals_need_no_device(eng, pm):
    _, fns = eng.load()
    cam = pm.make_camera(np.array([[20.0, 0, 8], [0, 20.0, 6], [0, 0, 1]]), np.eye(3), np.zeros(3), 12, 16, 1.0, 9.0)
    cams = (pm.Camera * 1)(cam)
    depth, grey = np.ones((12, 16), np.float32), np.zeros((12, 16), np.uint8)
    dp, cp = (_P * 1)(depth.ctypes.data), (_P * 1)(grey.ctypes.data)
    for color in (0, 1):
        rc, h = _create(fns, color=color)
        assert rc == 0
        px, pc, pt, nt = _P(0x55), _P(0x44), _P(0x66), C.c_longlong(77)
        rgb_arg = C.byref(pc) if color else None
        for mw in (0, -1, -2147483648):
            assert fns["tsdf_mesh"](h, mw, C.byref(px), rgb_arg, C.byref(pt), C.byref(nt)) == -2
            assert "min_weight" in fns["last_error"](None).decode()
        # out_rgb is NULL iff the volume has no colour
        assert fns["tsdf_mesh"](h, 1, C.byref(px), None if color else C.byref(pc), C.byref(pt), C.byref(nt)) == -2
        assert fns["tsdf_mesh"](h, 1, None, rgb_arg, C.byref(pt), C.byref(nt)) == -2
        assert fns["tsdf_mesh"](h, 1, C.byref(px), rgb_arg, None, C.byref(nt)) == -2
        assert fns["tsdf_mesh"](h, 1, C.byref(px), rgb_arg, C.byref(pt), None) == -2
        assert (px.value, pc.value, pt.value, nt.value) == (0x55, 0x44, 0x66, 77)
        # colours given to a colourless volume, and the reverse
        if color:
            assert fns["tsdf_integrate"](h, 1, cams, dp, None, 0) == -2 and "needs colours" in fns["last_error"](None).decode()
            for channels in (0, 2, 4):
                assert fns["tsdf_integrate"](h, 1, cams, dp, cp, channels) == -2 and "color_channels" in fns["last_error"](None).decode()
            assert fns["tsdf_integrate"](h, 1, cams, dp, (_P * 1)(None), 1) == -2
        else:
            assert fns["tsdf_integrate"](h, 1, cams, dp, cp, 1) == -2 and "without colour" in fns["last_error"](None).decode()
            assert fns["tsdf_integrate"](h, 0, None, None, cp, 1) == -2   # checked for an empty list too
            c4 = np.zeros(4 * 24, np.uint32)
            s, w = np.zeros(24, np.float32), np.zeros(24, np.int32)
            assert fns["tsdf_get"](h, s.ctypes.data, w.ctypes.data, c4.ctypes.data) == -2
            assert fns["tsdf_set"](h, s.ctypes.data, w.ctypes.data, c4.ctypes.data) == -2
        colors = cp if color else None
        channels = 1 if color else 0
        assert fns["tsdf_integrate"](h, -1, cams, dp, colors, channels) == -2
        assert fns["tsdf_integrate"](h, 1, None, dp, colors, channels) == -2
        assert fns["tsdf_integrate"](h, 1, cams, None, colors, channels) == -2
        assert fns["tsdf_integrate"](h, 1, cams, (_P * 1)(None), colors, channels) == -2
        flat = (pm.Camera * 1)(pm.make_camera(np.eye(3), np.eye(3), np.zeros(3), 0, 16, 1.0, 9.0))
        assert fns["tsdf_integrate"](h, 1, flat, dp, colors, channels) == -2
        wide = (pm.Camera * 1)(pm.make_camera(np.eye(3), np.eye(3), np.zeros(3), 1, (1 << 24) + 1, 1.0, 9.0))
        assert fns["tsdf_integrate"](h, 1, wide, dp, colors, channels) == -3
        big = (pm.Camera * 1)(pm.make_camera(np.eye(3), np.eye(3), np.zeros(3), 1 << 16, 1 << 16, 1.0, 9.0))
        assert fns["tsdf_integrate"](h, 1, big, dp, colors, channels) == -3
        assert fns["tsdf_integrate"](h, 0, None, None, None, 0) == 0    # nothing to do: no device needed
        assert fns["tsdf_get"](h, None, None, None) == -2 and fns["tsdf_set"](h, None, None, None) == -2
        ms = (C.c_float * 5)(*([7.0] * 5))
        assert fns["tsdf_pass_ms"](h, ms) == 0 and list(ms) == [0.0] * 5
        assert fns["tsdf_pass_ms"](h, None) == -2
        fns["tsdf_destroy"](h)


def test_a_volume_without_a_cell_meshes_empty_without_a_device(mesh):
    for dims in ((5, 4, 1), (1, 4, 3), (5, 1, 3), (1, 1, 1)):
        with mesh.Volume((0, 0, 0), 1.0, dims, 1.0, color=True, device=0) as v:
            m = v.mesh()
            assert m["xyz"].shape == (0, 3) and m["tri"].shape == (0, 3) and m["rgb"].shape == (0, 3)
            assert m["xyz"].dtype == np.float32 and m["tri"].dtype == np.int32 and m["rgb"].dtype == np.uint8
            assert v.pass_ms() == {"integrate": 0.0, "mark": 0.0, "scan": 0.0, "vertices": 0.0, "triangles": 0.0}
    with pytest.raises(ValueError):
        mesh.Volume((0, 0, 0), 0.0, (2, 2, 2), 1.0)
    with pytest.raises(ValueError):
        mesh.Volume((0, 0, 0), 1.0, (2, 2), 1.0)
    with mesh.Volume((0, 0, 0), 1.0, (2, 2, 2), 1.0) as v:
        with pytest.raises(ValueError):
            v.mesh(min_weight=0)


# ---- the statement against expectations written out by hand -----------------------------------------------------------------
def _cell(values, weights=None):
    """one cell: values[z][y][x]"""
    f = np.array(values, np.float32).reshape(2, 2, 2)
    w = np.ones((2, 2, 2), np.int32) if weights is None else np.array(weights, np.int32).reshape(2, 2, 2)
    return tc.mesh_statement(f, w, None, (2, 2, 2), (0, 0, 0), 1.0)


def test_orientation_table_by_hand():
    """tetrahedron 0 (xyz): v0 = 000, v1 = 100, v2 = 110, v3 = 111.  One inside corner v0: the triangle (e01, e02, e03) at the midpoints
    (.5,0,0), (.5,.5,0), (.5,.5,.5) has the normal (.25, -.25, 0) . (outside mean - inside mean = (1, 2/3, 1/3)) > 0: kept.  The
    complementary case has the same triangle and the opposite direction: swapped."""
    assert tc.tet_vertices(0) == [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1)]
    assert [tc.tet_vertices(t)[1:3] for t in range(6)] == [[(1, 0, 0), (1, 1, 0)], [(1, 0, 0), (1, 0, 1)], [(0, 1, 0), (1, 1, 0)],
                                                           [(0, 1, 0), (0, 1, 1)], [(0, 0, 1), (1, 0, 1)], [(0, 0, 1), (0, 1, 1)]]
    assert tc.FLIP[0][0b0001] == [False] and tc.FLIP[0][0b1110] == [True]
    for t in range(6):
        for m in (1, 2, 4, 8):   # one inside corner and its complement list the same triangle and face opposite ways
            assert [not x for x in tc.FLIP[t][m]] == tc.FLIP[t][15 - m], (t, m)
        for m in (3, 5, 6, 9, 10, 12):   # the two triangles of a quadrilateral share the diagonal e(a,c) - e(b,d): one winding for both
            assert len(tc.FLIP[t][m]) == 2 and tc.FLIP[t][m][0] == tc.FLIP[t][m][1], (t, m)
        assert tc.FLIP[t][0] == [] and tc.FLIP[t][15] == []
    assert tc.case_triangles([True, False, False, False]) == [[(0, 1), (0, 2), (0, 3)]]
    assert tc.case_triangles([True, True, False, True]) == [[(0, 2), (1, 2), (3, 2)]]
    assert tc.case_triangles([False, True, True, False]) == [[(1, 0), (1, 3), (2, 3)], [(1, 0), (2, 3), (2, 0)]]


def test_single_cell_one_inside_corner_by_hand():
    """corner 000 inside at f = -1, all others at +1: all six tetrahedra have the one inside corner v0, so each emits (e01, e02, e03);
    the seven edges that leave 000 carry the vertices 0..6 in slot order, each at t = 1/2"""
    m = _cell([[[-1, 1], [1, 1]], [[1, 1], [1, 1]]])
    want_xyz = 0.5 * np.array(tc.SLOTS, np.float32)
    assert np.array_equal(m["xyz"], want_xyz)
    slot = {off: s for s, off in enumerate(tc.SLOTS)}
    want = []
    for t in range(6):
        v = tc.tet_vertices(t)
        ids = [slot[v[1]], slot[v[2]], slot[v[3]]]
        p = want_xyz[ids].astype(np.float64)
        if np.dot(np.cross(p[1] - p[0], p[2] - p[0]), [1.0, 1.0, 1.0]) < 0:   # must face away from the inside corner
            ids = [ids[0], ids[2], ids[1]]
        want.append(ids)
    assert m["tri"].tolist() == want
    assert m["tri"].tolist()[0] == [0, 3, 6] and m["tri"].tolist()[1] == [0, 6, 4]   # xyz keeps its winding, xzy swaps
    topo = tc.topology(m["tri"])
    assert (topo["V"], topo["E"], topo["F"]) == (7, 12, 6) and topo["manifold_with_boundary"] and not topo["closed"]


def test_single_cell_case_classes_by_hand():
    # three inside corners of tetrahedron 0 (000, 100, 110 inside; 111 and the rest outside)
    f = np.ones((2, 2, 2), np.float32)
    f[0, 0, 0] = f[0, 0, 1] = f[0, 1, 1] = -1.0   # [z, y, x]
    m = tc.mesh_statement(f, np.ones((2, 2, 2), np.int32), None, (2, 2, 2), (0, 0, 0), 1.0)
    topo = tc.topology(m["tri"])
    # xyz has three inside corners (1 triangle), xzy and yxz two (2 each), yzx, zxy, zyx only 000 (1 each)
    assert topo["manifold_with_boundary"] and m["tri"].shape[0] == 1 + 2 + 2 + 1 + 1 + 1
    # the vertices by (owner, slot): 000 owns slots 1 2 4 5 6 (its edges to 100 and 110 do not cross) = 0..4, 100 owns 001 and 011
    # = 5, 6, 010 owns 100 = 7, 110 owns 001 = 8
    assert len(m["xyz"]) == 9
    # tetrahedron 0, inside mask 0b0111: (e(0,3), e(1,3), e(2,3)) = 000-111, 100-111, 110-111.  At the midpoints (.5,.5,.5), (1,.5,.5),
    # (1,1,.5) the normal is (0, 0, .25), and 111 - mean(000, 100, 110) = (1/3, 2/3, 1) lies on its side: not swapped
    assert m["tri"][0].tolist() == [4, 6, 8]
    assert np.array_equal(m["xyz"][[4, 6, 8]], np.array([[.5, .5, .5], [1, .5, .5], [1, 1, .5]], np.float32))
    # two inside corners: the x = 0 face inside, the x = 1 face outside: the plane x = 1/2 through every tetrahedron
    f = np.ones((2, 2, 2), np.float32)
    f[:, :, 0] = -1.0
    m = tc.mesh_statement(f, np.ones((2, 2, 2), np.int32), None, (2, 2, 2), (0, 0, 0), 1.0)
    assert (m["xyz"][:, 0] == 0.5).all() and len(m["xyz"]) == 4 + 4 + 1   # 4 axis edges, 4 face diagonals, the body diagonal
    p = m["xyz"][m["tri"]].astype(np.float64)
    normals = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    assert (normals[:, 0] > 0).all() and np.isclose(np.linalg.norm(normals, axis=1).sum() / 2, 1.0)   # faces +x, covers the unit square
    assert len(m["tri"]) == 1 + 1 + 2 + 1 + 2 + 1   # inside corners per tetrahedron: 1, 1, 2, 3, 2, 3
    # an invalid corner silences exactly the tetrahedra that touch it: 100 belongs to xyz and xzy only
    w = np.ones((2, 2, 2), np.int32)
    w[0, 0, 1] = 0
    m2 = tc.mesh_statement(f, w, None, (2, 2, 2), (0, 0, 0), 1.0)
    assert 0 < len(m2["tri"]) < len(m["tri"])
    # exact zero is outside: nothing is inside, nothing is emitted
    m3 = _cell(np.zeros((2, 2, 2)))
    assert len(m3["tri"]) == 0 and len(m3["xyz"]) == 0


def test_anchor_counts_and_topology():
    f, w = tc.sphere_volume((10, 9, 8), (4.3, 3.9, 3.4), 2.7)
    m = tc.mesh_statement(f, w, None, (10, 9, 8), (0, 0, 0), 1.0)
    topo = tc.topology(m["tri"])
    assert (topo["V"], topo["E"], topo["F"]) == (410, 1224, 816) and len(m["xyz"]) == 410
    assert topo["closed"] and topo["euler"] == 2
    vol = tc.signed_volume(m["xyz"], m["tri"])
    assert 0.85 * 4 / 3 * np.pi * 2.7 ** 3 < vol < 4 / 3 * np.pi * 2.7 ** 3   # positive: counter-clockwise from outside; inscribed
    # vertices ascend by (owner, slot): positions along an owner's edges never precede the owner's corner
    assert (np.diff(m["tri"].reshape(-1)) != 0).any() and m["tri"].min() == 0 and m["tri"].max() == 409


def test_exact_zeros_two_spheres_and_holes_stay_manifold():
    f, w = tc.sphere_volume((7, 7, 7), (3, 3, 3), 2.0)
    assert int((f == 0).sum()) == 6
    topo = tc.topology(tc.mesh_statement(f, w, None, (7, 7, 7), (0, 0, 0), 1.0)["tri"])
    assert topo["closed"] and topo["euler"] == 2
    fa, _ = tc.sphere_volume((12, 7, 7), (3.2, 3, 3), 2.1)
    fb, w = tc.sphere_volume((12, 7, 7), (7.9, 3, 3), 2.1)
    m = tc.mesh_statement(np.minimum(fa, fb), w, None, (12, 7, 7), (0, 0, 0), 1.0)
    topo = tc.topology(m["tri"])
    assert topo["closed"] and topo["euler"] in (2, 4) and tc.signed_volume(m["xyz"], m["tri"]) > 0
    f, w = tc.sphere_volume((10, 9, 8), (4.3, 3.9, 3.4), 2.7)
    w[2:5, 3:6, 5:9] = 0
    topo = tc.topology(tc.mesh_statement(f, w, None, (10, 9, 8), (0, 0, 0), 1.0)["tri"])
    assert topo["manifold_with_boundary"] and not topo["closed"] and 0 < topo["F"] < 816


def test_integrate_statement_by_hand(pm):
    """one camera at the origin looking along +z, f = 10, principal point (8, 6), 16 x 12; a wall at depth 5, trunc 1: the voxels on
    the axis at z = 3.5, 4.5, 5.25, 6, 6.5 get min(1, (5 - z) / 1) = 1, .5, -.25, -1 and nothing (s < -trunc)"""
    cam = pm.make_camera(np.array([[10.0, 0, 8], [0, 10.0, 6], [0, 0, 1]]), np.eye(3), np.zeros(3), 12, 16, 1.0, 9.0)
    depth = np.full((12, 16), 5.0, np.float32)
    col = np.full((12, 16, 3), (10, 20, 30), np.uint8)
    for z, want_sum, want_w, want_c in ((3.5, 1.0, 1, 0), (4.5, 0.5, 1, 1), (5.25, -0.25, 1, 1), (6.0, -1.0, 1, 1), (6.5, 0.0, 0, 0), (-1.0, 0.0, 0, 0)):
        s, w, c = tc.integrate_statement((0.0, 0.0, z), 1.0, (1, 1, 1), 1.0, [cam, cam], [depth, depth], [col, col])
        assert s.reshape(-1)[0] == np.float32(2 * want_sum) and w.reshape(-1)[0] == 2 * want_w, z
        assert c.reshape(-1).tolist() == [20 * want_c, 40 * want_c, 60 * want_c, 2 * want_c], z
    # the pixel: x = 0.76 at z = 4 projects to fu = 1.9 + 8 + .5 = 10.4 -> column 10; y = 0.4 to fv = 1 + 6 + .5 = 7.5 -> row 7
    depth = np.zeros((12, 16), np.float32)
    depth[7, 10] = 4.0
    s, w, _ = tc.integrate_statement((0.76, 0.4, 4.0), 1.0, (1, 1, 1), 1.0, [cam], [depth])
    assert w.reshape(-1)[0] == 1 and s.reshape(-1)[0] == 0.0
    # the borders: fu = 0 is inside, fu = W is outside (x = -3.4 -> fu = 0; x = +3.0 -> fu = 16)
    depth = np.full((12, 16), 4.0, np.float32)
    _, w, _ = tc.integrate_statement((-3.4, 0.0, 4.0), 6.4, (2, 1, 1), 1.0, [cam], [depth])
    assert w.reshape(-1).tolist() == [1, 0]
    # depth 0, negative, NaN, inf: no observation
    for bad in (0.0, -4.0, np.nan, np.inf):
        _, w, _ = tc.integrate_statement((0.0, 0.0, 4.0), 1.0, (1, 1, 1), 1.0, [cam], [np.full((12, 16), bad, np.float32)])
        assert w.reshape(-1)[0] == 0, bad


def test_ply_mesh_round_trip(mesh, tmp_path):
    f, w = tc.sphere_volume((10, 9, 8), (4.3, 3.9, 3.4), 2.7)
    m = tc.mesh_statement(f, w, None, (10, 9, 8), (0, 0, 0), 1.0)
    rgb = (np.arange(3 * len(m["xyz"])) % 251).astype(np.uint8).reshape(-1, 3)
    for colours in (None, rgb):
        path = str(tmp_path / "mesh.ply")
        mesh.write_ply_mesh(path, m["xyz"], m["tri"], colours)
        head = open(path, "rb").read(400)
        assert head.startswith(b"ply\nformat binary_little_endian 1.0\n") and b"element face 816\nproperty list uchar int vertex_indices\nend_header\n" in head
        back = mesh.read_ply_mesh(path)
        assert np.array_equal(back["xyz"].view(np.uint32), m["xyz"].view(np.uint32)) and np.array_equal(back["tri"], m["tri"])
        assert back["tri"].dtype == np.int32 and back["xyz"].dtype == np.float32
        assert (back["rgb"] is None) if colours is None else np.array_equal(back["rgb"], rgb)
        assert os.path.getsize(path) == head.index(b"end_header\n") + 11 + 410 * (12 if colours is None else 15) + 816 * 13
    path = str(tmp_path / "empty.ply")
    mesh.write_ply_mesh(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    back = mesh.read_ply_mesh(path)
    assert back["xyz"].shape == (0, 3) and back["tri"].shape == (0, 3)
    with pytest.raises(ValueError):
        mesh.write_ply_mesh(path, np.zeros((2, 3), np.float32), np.array([[0, 1, 2]], np.int32))
    with open(path, "wb") as fh:
        fh.write(b"ply\nformat ascii 1.0\nelement vertex 0\nend_header\n")
    with pytest.raises(ValueError):
        mesh.read_ply_mesh(path)
