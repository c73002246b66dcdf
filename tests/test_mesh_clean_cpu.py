"""mpmvs_mesh_* without a GPU: the symbols, the refusals (mpmvs_mesh_create touches no device, so a live handle can be refused here
too), what is answered on the host, the numpy statements of mesh_clean_common.py against numbers written out by hand, the seeded
sweep's census and the PLY round trip in its four layouts."""
import ctypes as C
import importlib
import math
import os
import re

import numpy as np
import pytest

import mesh_clean_common as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mpmvs_mesh_create", "mpmvs_mesh_components", "mpmvs_mesh_normals", "mpmvs_mesh_select", "mpmvs_mesh_pass_ms", "mpmvs_mesh_destroy")
_P = C.c_void_p
F = np.float32


@pytest.fixture(scope="module")
def eng(pm):
    return importlib.import_module("mp-mvs_amd.engine")


@pytest.fixture(scope="module")
def mesh(pm):
    return importlib.import_module("mp-mvs_amd.mesh")


def test_symbols_declared_exported_and_bound(eng):
    header = open(os.path.join(ROOT, "include", "mpmvs.h")).read()
    declared = set(re.findall(r"\b(mpmvs_[a-z0-9_]+)\s*\(", header))
    assert sorted(n for n in declared if n.startswith("mpmvs_mesh_")) == sorted(NEW)
    lib, fns = eng.load()
    lib_q8, fns_q8 = eng.load_variant(eng.LIB_Q8_PATH)
    for name in NEW:
        assert name in declared and name in eng.ALL_SYMBOLS
        assert hasattr(lib, name) and hasattr(lib_q8, name)
        assert name[len("mpmvs_"):] in fns and name[len("mpmvs_"):] in fns_q8
    f = fns["mesh_create"]
    assert f.restype is C.c_int and f.argtypes == [C.c_int, C.c_longlong, _P, _P, C.c_longlong, _P, C.POINTER(_P)]
    f = fns["mesh_components"]
    assert f.restype is C.c_int and f.argtypes == [_P, _P, _P, _P, C.POINTER(C.c_longlong)]
    f = fns["mesh_normals"]
    assert f.restype is C.c_int and f.argtypes == [_P, _P, C.POINTER(C.c_longlong)]
    f = fns["mesh_select"]
    assert f.restype is C.c_longlong and f.argtypes == [_P, _P, C.c_int, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_longlong)]
    f = fns["mesh_pass_ms"]
    assert f.restype is C.c_int and f.argtypes == [_P, C.POINTER(C.c_float)]
    assert fns["mesh_destroy"].restype is None and fns["mesh_destroy"].argtypes == [_P]
    csrc = os.path.join(ROOT, "mp-mvs_amd", "csrc")
    assert '#include "pm_mesh.hpp"' in open(os.path.join(csrc, "mpmvs_mesh.hip")).read()
    # the union-find is shared, not copied: one definition, included by both users
    assert "inline int cc_link(" in open(os.path.join(csrc, "pm_unionfind.hpp")).read()
    for user in ("pm_components.hpp", "pm_mesh.hpp"):
        text = open(os.path.join(csrc, user)).read()
        assert '#include "pm_unionfind.hpp"' in text and "inline int cc_link(" not in text and "inline int cc_find(" not in text


def _create(fns, xyz, tri, rgb=None, n=None, m=None, device=0):
    xyz = None if xyz is None else np.ascontiguousarray(xyz, F)
    tri = None if tri is None else np.ascontiguousarray(tri, np.int32)
    h = _P(0x1234)   # a marker: a refused create must leave it
    n = (0 if xyz is None else xyz.size // 3) if n is None else n
    m = (0 if tri is None else tri.size // 3) if m is None else m
    rc = fns["mesh_create"](device, n, None if xyz is None else xyz.ctypes.data, None if rgb is None else rgb.ctypes.data, m,
                            None if tri is None else tri.ctypes.data, C.byref(h))
    return rc, h


TRI_XYZ = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F)


def test_create_refusals_need_no_device(eng):
    _, fns = eng.load()
    one = np.array([[0, 1, 2]], np.int32)
    for kw in (dict(xyz=TRI_XYZ, tri=one, n=-1), dict(xyz=TRI_XYZ, tri=one, m=-1), dict(xyz=None, tri=None, n=3), dict(xyz=TRI_XYZ, tri=None, m=1),
               dict(xyz=TRI_XYZ, tri=one, device=-1)):
        rc, h = _create(fns, **kw)
        assert rc == -2 and h.value == 0x1234, kw
        assert "mesh create" in fns["last_error"](None).decode()
    for bad, where in ((3, 1), (-1, 1), (3, 0), (2147483647, 2), (-2147483648, 0)):
        tri = np.array([[0, 1, 2], [2, 1, 0], [1, 1, 1]], np.int32)
        tri[where, 1] = bad
        rc, h = _create(fns, TRI_XYZ, tri)
        text = fns["last_error"](None).decode()
        assert rc == -2 and h.value == 0x1234 and f"triangle {where} " in text and f"vertex {bad}," in text, text
    # the first bad triangle is the one that is named
    rc, h = _create(fns, TRI_XYZ, np.array([[0, 1, 2], [0, 5, 2], [0, -7, 2]], np.int32))
    assert rc == -2 and "triangle 1 " in fns["last_error"](None).decode()
    # a triangle of a mesh without vertices has no legal index
    rc, h = _create(fns, None, np.zeros((1, 3), np.int32))
    assert rc == -2 and h.value == 0x1234
    for kw in (dict(n=(1 << 30) + 1), dict(m=(1 << 30) + 1), dict(n=1 << 62, m=1 << 62)):
        rc, h = _create(fns, TRI_XYZ, one, **kw)   # refused before an array is read
        assert rc == -3 and h.value == 0x1234 and "2^30" in fns["last_error"](None).decode(), kw
    assert fns["mesh_create"](0, 0, None, None, 0, None, None) == -2
    rc, h = _create(fns, None, None)   # n == 0 and m == 0 are legal
    assert rc == 0 and h.value not in (None, 0x1234)
    fns["mesh_destroy"](h)
    fns["mesh_destroy"](None)


def test_null_handle_is_minus_2_and_writes_nothing(eng):
    _, fns = eng.load()
    lab, nrm = np.full(4, 7, np.int32), np.full(12, 7, F)
    counts, nd = (C.c_longlong * 4)(7, 7, 7, 7), C.c_longlong(7)
    assert fns["mesh_components"](None, lab.ctypes.data, lab.ctypes.data, lab.ctypes.data, counts) == -2 and "mesh components" in fns["last_error"](None).decode()
    assert fns["mesh_normals"](None, nrm.ctypes.data, C.byref(nd)) == -2 and "mesh normals" in fns["last_error"](None).decode()
    keep = np.ones(4, np.uint8)
    px, pc, pt, ps, mo = _P(0x55), _P(0x44), _P(0x66), _P(0x33), C.c_longlong(77)
    assert fns["mesh_select"](None, keep.ctypes.data, 1, C.byref(px), None, C.byref(pt), C.byref(ps), C.byref(mo)) == -2
    assert "mesh select" in fns["last_error"](None).decode()
    ms = (C.c_float * 8)(*([7.0] * 8))
    assert fns["mesh_pass_ms"](None, ms) == -2 and list(ms) == [7.0] * 8
    assert (lab == 7).all() and (nrm == 7).all() and list(counts) == [7] * 4 and nd.value == 7
    assert (px.value, pc.value, pt.value, ps.value, mo.value) == (0x55, 0x44, 0x66, 0x33, 77)


def test_live_handle_refusals_write_nothing_and_need_no_device(eng):
    _, fns = eng.load()
    rgb = np.zeros((3, 3), np.uint8)
    for color in (None, rgb):
        rc, h = _create(fns, TRI_XYZ, np.array([[0, 1, 2]], np.int32), color)
        assert rc == 0
        counts, nd = (C.c_longlong * 4)(7, 7, 7, 7), C.c_longlong(7)
        assert fns["mesh_components"](h, None, None, None, counts) == -2 and list(counts) == [7] * 4
        assert fns["mesh_normals"](h, None, C.byref(nd)) == -2 and nd.value == 7
        keep = np.ones(3, np.uint8)
        px, pc, pt, ps, mo = _P(0x55), _P(0x44), _P(0x66), _P(0x33), C.c_longlong(77)
        rgb_arg, wrong = (C.byref(pc), None) if color is not None else (None, C.byref(pc))
        assert fns["mesh_select"](h, None, 1, C.byref(px), rgb_arg, C.byref(pt), C.byref(ps), C.byref(mo)) == -2
        assert fns["mesh_select"](h, keep.ctypes.data, 1, None, rgb_arg, C.byref(pt), C.byref(ps), C.byref(mo)) == -2
        assert fns["mesh_select"](h, keep.ctypes.data, 1, C.byref(px), rgb_arg, None, C.byref(ps), C.byref(mo)) == -2
        assert fns["mesh_select"](h, keep.ctypes.data, 1, C.byref(px), rgb_arg, C.byref(pt), C.byref(ps), None) == -2
        assert fns["mesh_select"](h, keep.ctypes.data, 1, C.byref(px), wrong, C.byref(pt), C.byref(ps), C.byref(mo)) == -2
        assert "colour" in fns["last_error"](None).decode()
        assert (px.value, pc.value, pt.value, ps.value, mo.value) == (0x55, 0x44, 0x66, 0x33, 77)
        assert fns["mesh_pass_ms"](h, None) == -2
        ms = (C.c_float * 8)(*([7.0] * 8))
        assert fns["mesh_pass_ms"](h, ms) == 0 and list(ms) == [0.0] * 8   # nothing has run
        fns["mesh_destroy"](h)


def test_nothing_to_do_is_answered_on_the_host(mesh):
    """m == 0 and n == 0: no device is opened (this test runs without one)"""
    xyz = np.array([[0, 0, 0], [1, 2, 3], [np.nan, 0, 0], [4, 4, 4]], F)
    for rgb in (None, np.arange(12, dtype=np.uint8).reshape(4, 3)):
        with mesh.Mesh(xyz, np.zeros((0, 3), np.int32), rgb) as h:
            label, verts, tris, counts = h.components()
            assert label.tolist() == [0, 1, 2, 3] and verts.tolist() == [1] * 4 and tris.tolist() == [0] * 4
            assert counts == {"components": 0, "unnamed": 4, "largest_triangles": 0, "largest_label": -1}
            assert h.components(False, False)[1:3] == (None, None)
            nrm, nd = h.normals()
            assert nd == 0 and nrm.shape == (4, 3) and not nrm.view(np.uint32).any()
            out = h.select(np.ones(4, np.uint8), drop_unreferenced=True)   # no triangle: no vertex is referenced
            assert out["xyz"].shape == (0, 3) and out["tri"].shape == (0, 3) and out["src"].shape == (0,) and (out["rgb"] is None) == (rgb is None)
            assert all(v == 0.0 for v in h.pass_ms().values())
        with mesh.Mesh(np.zeros((0, 3), F), np.zeros((0, 3), np.int32), None if rgb is None else np.zeros((0, 3), np.uint8)) as h:
            label, verts, tris, counts = h.components()
            assert len(label) == 0 and counts == {"components": 0, "unnamed": 0, "largest_triangles": 0, "largest_label": -1}
            assert h.normals()[1] == 0
            for drop in (False, True):
                out = h.select(np.zeros(0, np.uint8), drop)
                assert out["xyz"].shape == (0, 3) and out["tri"].shape == (0, 3)
    # a mesh whose finite vertices coincide has no extent: its normals are zero, answered on the host as well
    with mesh.Mesh(np.ones((3, 3), F), np.array([[0, 1, 2]], np.int32)) as h:
        nrm, nd = h.normals()
        assert nd == 0 and not nrm.view(np.uint32).any()
    with pytest.raises(ValueError, match="triangle 0 names vertex 3"):
        mesh.Mesh(TRI_XYZ, np.array([[0, 1, 3]], np.int32))


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def test_normals_statement_by_hand():
    # one triangle in the plane z = 0, counter-clockwise seen from +z: ext = 1, B = 2 = 0.5 * 2^2 so e = 2; m = 1 so b = 0;
    # scale = 2^59; C = (0, 0, 1), F = (0, 0, 2^59) on all three vertices; len = 2^59; normal exactly (0, 0, 1)
    assert mc.normal_scale(TRI_XYZ, 1) == (2.0 ** 59, 2, 0, 1.0)
    nrm, nd, S = mc.normals_statement(TRI_XYZ, [[0, 1, 2]], sums=True)
    assert S.tolist() == [[0, 0, 1 << 59]] * 3 and nd == 3
    assert np.array_equal(_bits(nrm), _bits([[0, 0, 1]] * 3))
    # e, b and scale for one more case: extents (3, 0.5, 0) -> ext = 3, B = 18 = 0.5625 * 2^5: e = 5; m = 5 <= 2^3: b = 3; 61 - 3 - 5 = 53
    xyz = np.array([[1, 1, 7], [4, 1.5, 7], [2, 1.25, 7]], F)
    assert mc.normal_scale(xyz, 5) == (2.0 ** 53, 5, 3, 3.0)
    assert mc.normal_scale(xyz, 8)[2] == 3 and mc.normal_scale(xyz, 9)[2] == 4 and mc.normal_scale(xyz, 1)[2] == 0
    # two coincident triangles of opposite winding: F and -F cancel exactly in the integers
    nrm, nd, S = mc.normals_statement(TRI_XYZ, [[0, 1, 2], [0, 2, 1]], sums=True)
    assert nd == 0 and not S.any() and not _bits(nrm).any()
    # a triangle against the two halves it is cut into, wound the other way: at the apex (vertex 1) the doubled areas 1, -f and
    # -(1 - f), f = (float)0.1, are integers after the scaling and cancel exactly
    xyz = np.array([[0, 0, 0], [0, 1, 0], [0.1, 0, 0], [1, 0, 0]], F)
    nrm, nd = mc.normals_statement(xyz, [[0, 3, 1], [0, 1, 2], [2, 1, 3]])
    assert not _bits(nrm[1]).any() and nd == 3
    # a closed tetrahedron with corners 0, ex, ey, ez: the face normals are -ez, -ey, (1, 1, 1), -ex with doubled areas 1, 1, sqrt(3), 1.
    # C per face: (0, 0, -1), (0, -1, 0), (1, 1, 1), (-1, 0, 0); ext = 1, e = 2, m = 4 so b = 2, scale = 2^57.
    # vertex 0 misses the slanted face: S = 2^57 * (-1, -1, -1); vertex 1 (ex) misses -ex: S = 2^57 * (1, 0, 0); likewise ey, ez
    nrm, nd, S = mc.normals_statement(mc.TET_XYZ, mc.TET, sums=True)
    assert (S // (1 << 57)).tolist() == [[-1, -1, -1], [1, 0, 0], [0, 1, 0], [0, 0, 1]] and nd == 4
    r = F(-1.0 / math.sqrt(3.0))
    assert np.array_equal(_bits(nrm), _bits([[r, r, r], [1, 0, 0], [0, 1, 0], [0, 0, 1]]))
    # a 3 x 3 planar grid, 8 triangles: every normal (0, 0, 1); the sums count the incident triangles (each C = (0, 0, 1)):
    # corners 0 and 8 have 2, corners 2 and 6 have 1, edge midpoints 3, the centre 6.  ext = 2, B = 8 = 0.5 * 2^4, e = 4, b = 3, scale = 2^54
    g = mc.grid(3, 3)
    nrm, nd, S = mc.normals_statement(g["xyz"], g["tri"], sums=True)
    assert (S[:, 2] >> 54).tolist() == [2, 3, 1, 3, 6, 3, 1, 3, 2] and not S[:, :2].any() and nd == 9
    assert np.array_equal(_bits(nrm), _bits([[0, 0, 1]] * 9))
    # a vertex that only a triangle with a NaN vertex names: zero; the NaN vertex too; the others shaded by the finite triangle alone
    xyz = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0], [5, 5, 5]], F)
    nrm, nd = mc.normals_statement(xyz, [[0, 1, 2], [4, 3, 0]])
    assert nd == 3 and not _bits(nrm[3:]).any() and np.array_equal(_bits(nrm[:3]), _bits([[0, 0, 1]] * 3))
    # a triangle with a repeated index adds nothing
    nrm2, _ = mc.normals_statement(xyz, [[0, 1, 2], [4, 3, 0], [0, 0, 1], [2, 4, 4], [4, 4, 4]])
    assert np.array_equal(_bits(nrm2), _bits(nrm))


def test_normals_do_not_see_a_power_of_two():
    for m in (mc.anchor(), mc.tetrahedra(20, 3), mc.fan(100)):
        base, nd = mc.normals_statement(m["xyz"], m["tri"])
        assert nd > 0
        for p in (-40, 40):
            scaled = (m["xyz"].astype(np.float64) * 2.0 ** p).astype(F)
            assert np.array_equal(scaled.astype(np.float64), m["xyz"].astype(np.float64) * 2.0 ** p)   # the scaling is exact in fp32
            got, nd2 = mc.normals_statement(scaled, m["tri"])
            assert nd2 == nd and np.array_equal(_bits(got), _bits(base)), p
        assert mc.normal_scale((m["xyz"].astype(np.float64) * 2.0 ** 40).astype(F), len(m["tri"]))[1] == mc.normal_scale(m["xyz"], len(m["tri"]))[1] + 80


def test_components_statement_by_hand():
    # two tetrahedra sharing vertex 3: one component of 7 vertices and 8 triangles
    shared = np.concatenate([mc.TET, np.array([3, 4, 5, 6])[mc.TET]])
    label, verts, tris, counts = mc.components_statement(7, shared)
    assert label.tolist() == [0] * 7 and verts.tolist() == [7] * 7 and tris.tolist() == [8] * 7 and counts == [1, 0, 8, 0]
    # sharing a position only: vertices 3 and 4 coincide in space, which no triangle knows: two components
    apart = np.concatenate([mc.TET, mc.TET + 4])
    label, verts, tris, counts = mc.components_statement(8, apart)
    assert label.tolist() == [0] * 4 + [4] * 4 and verts.tolist() == [4] * 8 and tris.tolist() == [4] * 8
    assert counts == [2, 0, 4, 0]   # a tie at 4 triangles: the smaller label wins
    # an unnamed vertex in the middle, and a larger second component: vertex 2 is alone with 0 triangles
    tri = [[0, 1, 3], [4, 5, 6], [6, 5, 7], [7, 4, 4]]
    label, verts, tris, counts = mc.components_statement(8, tri)
    assert label.tolist() == [0, 0, 2, 0, 4, 4, 4, 4] and verts.tolist() == [3, 3, 1, 3, 4, 4, 4, 4] and tris.tolist() == [1, 1, 0, 1, 3, 3, 3, 3]
    assert counts == [2, 1, 3, 4]
    # a triangle belongs to the component of its first index, which is the component of all three
    label, _, tris, counts = mc.components_statement(11, mc.repeated()["tri"])
    assert label.tolist() == [0, 0, 0, 0, 0, 0, 0, 7, 7, 9, 10] and tris.tolist() == [5] * 7 + [1, 1, 1, 0] and counts == [3, 1, 5, 0]
    # the keep rule: at least 2 triangles; the 2 largest; ties to the smaller label
    assert mc.keep_statement(label, tris, 2).tolist() == [True] * 7 + [False] * 4
    assert mc.keep_statement(label, tris, 1, 2).tolist() == [True] * 7 + [True, True, False, False]
    assert mc.keep_statement(label, tris, 1).tolist() == [True] * 10 + [False]
    assert not mc.keep_statement(label, tris, 10 ** 6).any() and not mc.keep_statement(label, tris, 1, 0).any()


def test_rank_components_is_the_keep_statement(mesh):
    for name in ("tetrahedra", "repeated", "anchor"):
        w = mc.want(name)
        for mt, largest in ((1, None), (5, None), (10 ** 6, None), (1, 1), (2, 3), (1, 10 ** 4), (0, None)):
            assert np.array_equal(mesh.rank_components(w["label"], w["tris"], mt, largest), mc.keep_statement(w["label"], w["tris"], mt, largest)), (name, mt, largest)


def test_select_statement_by_hand():
    m = mc._mesh(np.arange(18).reshape(6, 3), [[0, 1, 2], [2, 3, 4], [4, 4, 5]], np.arange(18).reshape(6, 3) + 100)
    keep = np.array([1, 1, 1, 0, 9, 1], np.uint8)   # vertex 3 goes and takes triangle 1 with it
    out = mc.select_statement(m, keep, drop_unreferenced=False)
    assert out["src"].tolist() == [0, 1, 2, 4, 5] and out["tri"].tolist() == [[0, 1, 2], [3, 3, 4]]
    assert np.array_equal(out["xyz"], m["xyz"][[0, 1, 2, 4, 5]]) and np.array_equal(out["rgb"], m["rgb"][[0, 1, 2, 4, 5]])
    keep[5] = 0   # now triangle 2 goes as well and vertex 4 is kept but unreferenced
    out = mc.select_statement(m, keep, drop_unreferenced=False)
    assert out["src"].tolist() == [0, 1, 2, 4] and out["tri"].tolist() == [[0, 1, 2]]
    out = mc.select_statement(m, keep, drop_unreferenced=True)
    assert out["src"].tolist() == [0, 1, 2] and out["tri"].tolist() == [[0, 1, 2]]
    out = mc.select_statement(m, np.zeros(6), True)
    assert out["xyz"].shape == (0, 3) and out["tri"].shape == (0, 3) and out["rgb"].shape == (0, 3)


def test_anchor_is_one_component_shaded_outwards():
    a, w = mc.anchor(), mc.want("anchor")
    assert len(a["xyz"]) == 410 and len(a["tri"]) == 816
    assert (w["label"] == 0).all() and (w["verts"] == 410).all() and (w["tris"] == 816).all() and w["counts"] == [1, 0, 816, 0]
    assert w["n_defined"] == 410
    out = (w["normals"].astype(np.float64) * (a["xyz"].astype(np.float64) - np.array(mc.ANCHOR[1]))).sum(1)
    assert (out > 0).all()
    assert np.abs(np.linalg.norm(w["normals"].astype(np.float64), axis=1) - 1.0).max() < 1e-6
    clean = mc.clean_statement(mc.join(a, mc.tetrahedra(5, 2)), min_triangles=5)
    assert len(clean["xyz"]) == 410 and np.array_equal(clean["tri"], a["tri"]) and clean["counts"] == [6, 2, 816, 0]


def test_sweep_census():
    """conditions on the statement alone, so that the sweep cannot quietly degenerate"""
    c = mc.sweep_census()
    print(c)
    assert c["one_component"] >= 5 and c["over_100_components"] >= 5 and c["unnamed_vertices"] >= 5
    assert c["zero_normal_on_named"] >= 3 and c["drop_changes"] >= 3
    assert c["repeated"] >= 4 and c["non_finite"] >= 4 and 5 <= c["coloured"] <= 35


def _expected_ply(xyz, tri, rgb, normals):
    head = "ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" % len(xyz)
    if normals is not None:
        head += "property float nx\nproperty float ny\nproperty float nz\n"
    if rgb is not None:
        head += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    head += "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % len(tri)
    body = b""
    for v in range(len(xyz)):
        body += np.asarray(xyz[v], "<f4").tobytes()
        if normals is not None:
            body += np.asarray(normals[v], "<f4").tobytes()
        if rgb is not None:
            body += bytes(int(c) for c in rgb[v])
    for t in tri:
        body += b"\x03" + np.asarray(t, "<i4").tobytes()
    return head.encode("ascii") + body


def test_ply_round_trip_in_four_layouts(mesh, tmp_path):
    m = mc.tetrahedra(6, 2, color=True)
    nrm, _ = mc.normals_statement(m["xyz"], m["tri"])
    path = str(tmp_path / "mesh.ply")
    for rgb in (None, m["rgb"]):
        for normals in (None, nrm):
            if normals is None:
                mesh.write_ply_mesh(path, m["xyz"], m["tri"], rgb)   # the call of today
            else:
                mesh.write_ply_mesh(path, m["xyz"], m["tri"], rgb, normals=normals)
            assert open(path, "rb").read() == _expected_ply(m["xyz"], m["tri"], rgb, normals)
            back = mesh.read_ply_mesh(path)
            assert np.array_equal(_bits(back["xyz"]), _bits(m["xyz"])) and np.array_equal(back["tri"], m["tri"])
            assert (back["rgb"] is None) if rgb is None else np.array_equal(back["rgb"], rgb)
            assert (back["normals"] is None) if normals is None else (np.array_equal(_bits(back["normals"]), _bits(nrm)) and back["normals"].dtype == F)
    mesh.write_ply_mesh(path, m["xyz"], m["tri"], None, None)
    assert open(path, "rb").read() == _expected_ply(m["xyz"], m["tri"], None, None)
    with pytest.raises(ValueError):
        mesh.write_ply_mesh(path, m["xyz"], m["tri"], normals=nrm[:-1])
    with open(path, "wb") as fh:   # normals after the colours: not a layout of write_ply_mesh
        fh.write(b"ply\nformat binary_little_endian 1.0\nelement vertex 0\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\n"
                 b"property uchar green\nproperty uchar blue\nproperty float nx\nproperty float ny\nproperty float nz\nelement face 0\n"
                 b"property list uchar int vertex_indices\nend_header\n")
    with pytest.raises(ValueError):
        mesh.read_ply_mesh(path)
