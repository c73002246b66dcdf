"""The brick-sparse TSDF volume without a GPU (include/mpmvs.h, statements A and B): the new symbols, the
refusals that need no device (mpmvs_tsdf_create_sparse touches none), the numpy statement of A against samples worked out by hand,
the brick-major renumbering on the anchor, and the end-to-end scene's coverage as the statement alone gives it."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import tsdf_common as tc
import tsdf_sparse_common as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mpmvs_tsdf_create_sparse", "mpmvs_tsdf_allocate", "mpmvs_tsdf_bricks", "mpmvs_tsdf_get_bricks", "mpmvs_tsdf_set_bricks", "mpmvs_tsdf_sparse_stats")
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
    lib, fns = eng.load()
    lib_q8, fns_q8 = eng.load_variant(eng.LIB_Q8_PATH)
    for name in NEW:
        assert name in declared and name in eng.ALL_SYMBOLS
        assert hasattr(lib, name) and hasattr(lib_q8, name)
        assert name[len("mpmvs_"):] in fns and name[len("mpmvs_"):] in fns_q8
    f = fns["tsdf_create_sparse"]
    assert f.restype is C.c_int
    assert f.argtypes == [C.c_int, C.POINTER(C.c_float), C.c_float, C.POINTER(C.c_int), C.c_float, C.c_int, C.c_float, C.c_longlong, C.POINTER(_P)]
    assert fns["tsdf_allocate"].restype is C.c_int and fns["tsdf_allocate"].argtypes == [_P, C.c_int, _P, _P]
    assert fns["tsdf_bricks"].restype is C.c_longlong and fns["tsdf_bricks"].argtypes == [_P, C.POINTER(_P)]
    assert fns["tsdf_get_bricks"].restype is C.c_int and fns["tsdf_get_bricks"].argtypes == [_P, _P, _P, _P]
    assert fns["tsdf_set_bricks"].restype is C.c_int and fns["tsdf_set_bricks"].argtypes == [_P, C.c_longlong, _P, _P, _P, _P]
    assert fns["tsdf_sparse_stats"].restype is C.c_int and fns["tsdf_sparse_stats"].argtypes == [_P, C.POINTER(C.c_longlong), C.POINTER(C.c_float)]
    csrc = os.path.join(ROOT, "mp-mvs_amd", "csrc")
    assert '#include "pm_tsdf_sparse.hpp"' in open(os.path.join(csrc, "mpmvs_mesh.hip")).read()
    assert "A. ALLOCATE" in header and "B. MASKED-DENSE EQUIVALENCE" in header


def _create(fns, dims=(20, 12, 9), voxel=0.5, trunc=1.0, color=0, origin=(0.0, 0.0, 0.0), pad=1.0, max_bricks=64):
    h = _P(0x1234)   # a marker: a refused create must leave it
    rc = fns["tsdf_create_sparse"](0, (C.c_float * 3)(*origin), voxel, (C.c_int * 3)(*dims), trunc, color, pad, max_bricks, C.byref(h))
    return rc, h


def _create_dense(fns, dims=(4, 3, 2)):
    h = _P()
    assert fns["tsdf_create"](0, (C.c_float * 3)(), 0.5, (C.c_int * 3)(*dims), 1.0, 0, C.byref(h)) == 0
    return h


def test_create_sparse_refusals_need_no_device(eng):
    _, fns = eng.load()
    bad = [dict(pad=-1.0), dict(pad=8.5), dict(pad=float("nan")), dict(pad=float("inf")), dict(max_bricks=0), dict(max_bricks=-5),
           # the dense refusals
           dict(dims=(0, 3, 2)), dict(dims=(4, -1, 2)), dict(dims=(4, 3, 0)), dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=float("nan")),
           dict(voxel=float("inf")), dict(trunc=0.0), dict(trunc=-2.0), dict(trunc=float("nan")), dict(trunc=float("inf")),
           dict(origin=(0.0, float("nan"), 0.0)), dict(origin=(3e38, 0.0, 0.0), dims=(1000, 2, 2), voxel=1e36)]
    for kw in bad:
        rc, h = _create(fns, **kw)
        assert rc == -2 and h.value == 0x1234, kw
        assert "tsdf create_sparse" in fns["last_error"](None).decode()
    too_big = [dict(max_bricks=(1 << 21) + 1),
               dict(dims=(2049 * 8, 2049 * 8, 2049 * 8)),          # a 2049^3 brick grid: more than 2^24 cells
               dict(dims=(2147483647, 2147483647, 2147483647)),
               dict(trunc=1.0, voxel=1.0 / 16385.0),               # 4 * trunc / voxel = 65540 samples: more than 2^16
               dict(trunc=1e30, voxel=1e-30)]
    for kw in too_big:
        rc, h = _create(fns, **kw)
        assert rc == -3 and h.value == 0x1234, kw
    assert fns["tsdf_create_sparse"](0, (C.c_float * 3)(), 0.5, (C.c_int * 3)(2, 2, 2), 1.0, 0, 1.0, 8, None) == -2
    # the limits themselves: pad 0 and 8, max_bricks 2^21, a 256^3 brick grid (2^24 cells), n_s = 2^16 exactly; still no device
    for kw in (dict(pad=0.0), dict(pad=8.0), dict(max_bricks=1 << 21), dict(dims=(2048, 2048, 2048)), dict(trunc=1.0, voxel=1.0 / 16384.0)):
        rc, h = _create(fns, **kw)
        assert rc == 0 and h.value not in (None, 0x1234), kw
        info, ms = (C.c_longlong * 4)(), (C.c_float * 2)()
        assert fns["tsdf_sparse_stats"](h, info, ms) == 0 and info[0] == 0 and info[3] == 0 and list(ms) == [0.0, 0.0]
        fns["tsdf_destroy"](h)


def test_dense_and_sparse_handles_refuse_each_others_calls(eng, pm):
    _, fns = eng.load()
    cam = pm.make_camera(np.array([[20.0, 0, 8], [0, 20.0, 6], [0, 0, 1]]), np.eye(3), np.zeros(3), 12, 16, 1.0, 9.0)
    cams = (pm.Camera * 1)(cam)
    depth = np.ones((12, 16), np.float32)
    dp = (_P * 1)(depth.ctypes.data)
    s, w = np.full(512, 7, np.float32), np.full(512, 7, np.int32)
    coords = np.zeros(3, np.int32)
    info, ms = (C.c_longlong * 4)(*([7] * 4)), (C.c_float * 2)(7.0, 7.0)
    d = _create_dense(fns)
    assert fns["tsdf_allocate"](d, 1, cams, dp) == -2 and "dense" in fns["last_error"](None).decode()
    assert fns["tsdf_allocate"](d, 0, None, None) == -2
    p = _P(0x77)
    assert fns["tsdf_bricks"](d, C.byref(p)) == -2 and p.value == 0x77
    assert fns["tsdf_get_bricks"](d, s.ctypes.data, w.ctypes.data, None) == -2 and (s == 7).all() and (w == 7).all()
    assert fns["tsdf_set_bricks"](d, 1, coords.ctypes.data, s.ctypes.data, w.ctypes.data, None) == -2
    assert fns["tsdf_sparse_stats"](d, info, ms) == -2 and list(info) == [7] * 4 and list(ms) == [7.0, 7.0]
    fns["tsdf_destroy"](d)
    rc, h = _create(fns)
    assert rc == 0
    assert fns["tsdf_get"](h, s.ctypes.data, w.ctypes.data, None) == -2 and "mpmvs_tsdf_get_bricks" in fns["last_error"](None).decode()
    assert fns["tsdf_set"](h, s.ctypes.data, w.ctypes.data, None) == -2 and "mpmvs_tsdf_set_bricks" in fns["last_error"](None).decode()
    assert (s == 7).all() and (w == 7).all()
    # allocate has the argument checks and codes of integrate
    assert fns["tsdf_allocate"](None, 0, None, None) == -2
    assert fns["tsdf_allocate"](h, -1, cams, dp) == -2 and fns["tsdf_allocate"](h, 1, None, dp) == -2 and fns["tsdf_allocate"](h, 1, cams, None) == -2
    assert fns["tsdf_allocate"](h, 1, cams, (_P * 1)(None)) == -2
    flat = (pm.Camera * 1)(pm.make_camera(np.eye(3), np.eye(3), np.zeros(3), 0, 16, 1.0, 9.0))
    assert fns["tsdf_allocate"](h, 1, flat, dp) == -2
    wide = (pm.Camera * 1)(pm.make_camera(np.eye(3), np.eye(3), np.zeros(3), 1, (1 << 24) + 1, 1.0, 9.0))
    assert fns["tsdf_allocate"](h, 1, wide, dp) == -3
    big = (pm.Camera * 1)(pm.make_camera(np.eye(3), np.eye(3), np.zeros(3), 1 << 16, 1 << 16, 1.0, 9.0))
    assert fns["tsdf_allocate"](h, 1, big, dp) == -3
    assert fns["tsdf_allocate"](h, 0, None, None) == 0       # nothing to do: no device needed
    assert fns["tsdf_integrate"](h, 0, None, None, None, 0) == 0
    assert fns["tsdf_bricks"](h, None) == 0
    p = _P(0x77)
    assert fns["tsdf_bricks"](h, C.byref(p)) == 0 and p.value is None   # NULL when the count is 0
    assert fns["tsdf_bricks"](None, None) == -2 and fns["tsdf_get_bricks"](None, s.ctypes.data, w.ctypes.data, None) == -2
    assert fns["tsdf_get_bricks"](h, None, None, None) == -2
    assert fns["tsdf_get_bricks"](h, s.ctypes.data, w.ctypes.data, s.ctypes.data) == -2   # colours of a volume without colour
    assert fns["tsdf_sparse_stats"](None, info, ms) == -2 and fns["tsdf_sparse_stats"](h, None, ms) == -2
    assert fns["tsdf_sparse_stats"](h, info, ms) == 0 and list(info) == [0, 64, 3 * 2 * 2, 0]
    fns["tsdf_destroy"](h)


def test_set_bricks_refusals_need_no_device(eng):
    _, fns = eng.load()
    rc, h = _create(fns, dims=(20, 12, 9), max_bricks=3)   # a 3 x 2 x 2 brick grid
    assert rc == 0
    s, w = np.zeros(4 * 512, np.float32), np.zeros(4 * 512, np.int32)

    def call(coords, n=None):
        c = np.array(coords, np.int32).reshape(-1, 3)
        return fns["tsdf_set_bricks"](h, len(c) if n is None else n, c.ctypes.data, s.ctypes.data, w.ctypes.data, None)

    assert call([(1, 0, 0), (0, 0, 0)]) == -2 and "ascend" in fns["last_error"](None).decode()        # unsorted
    assert call([(0, 1, 0), (2, 0, 0)]) == -2                                                          # unsorted: linear 3, then 2
    assert call([(1, 1, 0), (1, 1, 0)]) == -2                                                          # a duplicate
    for outside in ((3, 0, 0), (0, 2, 0), (0, 0, 2), (-1, 0, 0)):
        assert call([outside]) == -2 and "outside" in fns["last_error"](None).decode(), outside
    assert call([(0, 0, 0), (1, 0, 0), (2, 0, 0), (0, 1, 0)]) == -3                                    # n above max_bricks
    assert call([(0, 0, 0)], n=-1) == -2
    assert fns["tsdf_set_bricks"](h, 1, None, s.ctypes.data, w.ctypes.data, None) == -2
    assert fns["tsdf_set_bricks"](h, 1, np.zeros(3, np.int32).ctypes.data, s.ctypes.data, w.ctypes.data, s.ctypes.data) == -2   # no colour
    assert fns["tsdf_set_bricks"](None, 0, None, None, None, None) == -2
    info, ms = (C.c_longlong * 4)(), (C.c_float * 2)()
    assert fns["tsdf_bricks"](h, None) == 0 and fns["tsdf_sparse_stats"](h, info, ms) == 0 and info[0] == 0 and info[3] == 0   # untouched
    fns["tsdf_destroy"](h)


def test_sparse_volume_without_a_brick_or_a_cell_needs_no_device(mesh):
    with mesh.SparseVolume((0, 0, 0), 1.0, (20, 12, 9), 1.0, color=True) as v:
        assert v.grid == (3, 2, 2) and v.max_bricks == 12 and v.pad == 1.0
        m = v.mesh()
        assert m["xyz"].shape == (0, 3) and m["tri"].shape == (0, 3) and m["rgb"].shape == (0, 3)
        b = v.get_bricks()
        assert b["coords"].shape == (0, 3) and b["sum"].shape == (0, 8, 8, 8) and b["color"].shape == (0, 8, 8, 8, 4)
        assert v.n_bricks() == 0 and v.stats()["bricks"] == 0 and v.stats()["brick_share"] == 0.0
        assert not v.to_dense()["weight"].any()
        with pytest.raises(ValueError):
            v.get()
        with pytest.raises(ValueError):
            v.mesh(min_weight=0)
    with pytest.raises(ValueError):
        mesh.SparseVolume((0, 0, 0), 1.0, (20, 12, 9), 1.0, pad=9.0)
    with pytest.raises(ValueError):
        mesh.SparseVolume((0, 0, 0), 1.0, (20, 12, 9), 1.0, max_bricks=0)
    with mesh.SparseVolume((0, 0, 0), 1.0, (2048, 2048, 2048), 1.0) as v:
        with pytest.raises(ValueError):
            v.to_dense()


# ---- statement A against samples worked out by hand ----------------------------------------------------------------------------
def _axis_cam(pm):
    """at the origin, looking along +z, f = 10, principal point (8, 6), 16 x 12: pixel (8, 6) is the optical axis"""
    return pm.make_camera(np.array([[10.0, 0, 8], [0, 10.0, 6], [0, 0, 1]]), np.eye(3), np.zeros(3), 12, 16, 1.0, 50.0)


def _one_pixel(ix, iy, d):
    depth = np.zeros((12, 16), F)
    depth[iy, ix] = d
    return depth


def _set(bricks):
    return {tuple(int(v) for v in c) for c in sc.brick_coords(bricks)}


def test_allocate_statement_by_hand(pm):
    cam = _axis_cam(pm)
    # 4 * 0.15f / 0.05f is a little above 12 in fp64 (the fp32 values are 0.150000006 and 0.0499999993): the ceiling is 13
    assert sc.n_samples(1.0, 1.0) == 4 and sc.n_samples(0.15, 0.05) == 13 and sc.n_samples(0.1, 1.0) == 1 and sc.n_samples(0.75, 0.25) == 12
    # trunc = voxel = 1: n_s = 4, the samples of d are z = d - 1, d - .5, d, d + .5, d + 1.  The axis pixel has xc = yc = 0, so with the
    # origin (-4, -4, 0) every sample sits at g = (4, 4, z).  d = 8, pad = 0: z = 7, 7.5, 8, 8.5, 9 -> voxels k = 7, 7, 8, 8, 9:
    # bricks (0, 0, 0) and (0, 0, 1).  z = 8 is exactly on the brick border: floorf(8 - 0) = 8 belongs to brick 1.
    one = sc.allocate_statement((-4, -4, 0), 1.0, (24, 24, 24), 1.0, 0.0, [cam], [_one_pixel(8, 6, 8.0)])
    assert _set(one) == {(0, 0, 0), (0, 0, 1)}
    # trunc = 0.1 gives n_s = 1 and two samples, z = 8.0 and 8.2 for d = 8.1; at pad = 0.25 both have lo = 7, hi = 8: both bricks
    border = sc.allocate_statement((-4, -4, 0), 1.0, (24, 24, 24), 0.1, 0.25, [cam], [_one_pixel(8, 6, 8.1)])
    assert _set(border) == {(0, 0, 0), (0, 0, 1)}
    # d = 9.5: z = 8.5 .. 10.5, all in brick K = 1 at pad 0; pad = 1 reaches down to floorf(8.5 - 1) = 7: brick 0 too, and no further
    assert _set(sc.allocate_statement((-4, -4, 0), 1.0, (24, 24, 24), 1.0, 0.0, [cam], [_one_pixel(8, 6, 9.5)])) == {(0, 0, 1)}
    assert _set(sc.allocate_statement((-4, -4, 0), 1.0, (24, 24, 24), 1.0, 1.0, [cam], [_one_pixel(8, 6, 9.5)])) == {(0, 0, 0), (0, 0, 1)}
    # pad = 8 reaches 27 bricks: origin (-8.5, -8.5, 0), d = 8.5: g = (8.5, 8.5, 7.5 .. 9.5); x and y: floorf(.5) = 0 .. floorf(16.5) = 16:
    # bricks 0..2; z: floorf(-.5) = -1 clamped to 0 .. floorf(17.5) = 17: bricks 0..2: the whole 3 x 3 x 3 grid
    all27 = sc.allocate_statement((-8.5, -8.5, 0), 1.0, (24, 24, 24), 1.0, 8.0, [cam], [_one_pixel(8, 6, 8.5)])
    assert all27.all() and all27.size == 27
    # z <= 0: d = 0.5 gives z = -.5, 0, .5, 1, 1.5; with the origin z = -7.75 those would be g_z = 7.25, 7.75 (brick 0, skipped) and
    # 8.25, 8.75, 9.25 (brick 1)
    assert _set(sc.allocate_statement((-4, -4, -7.75), 1.0, (24, 24, 24), 1.0, 0.0, [cam], [_one_pixel(8, 6, 0.5)])) == {(0, 0, 1)}
    # a ray leaving the box: pixel (15, 6) has xc = 0.7 z; dims (8, 24, 24), origin (-4, -4, -2): d = 5.5 gives z = 4.5, 5, 5.5, 6, 6.5,
    # g_x = 7.15, 7.5, 7.85 | 8.2, 8.55 (outside: lo = 8 > n_x - 1 = 7, skipped), g_z = 6.5, 7, 7.5 | 8, 8.5: only brick K = 0
    assert _set(sc.allocate_statement((-4, -4, -2), 1.0, (8, 24, 24), 1.0, 0.0, [cam], [_one_pixel(15, 6, 5.5)])) == {(0, 0, 0)}
    # ... but with pad = 1 the sample at g_x = 8.2 reaches back to lo = 7: inside, and it marks K = 1 (g_z = 8)
    assert _set(sc.allocate_statement((-4, -4, -2), 1.0, (8, 24, 24), 1.0, 1.0, [cam], [_one_pixel(15, 6, 5.5)])) == {(0, 0, 0), (0, 0, 1)}
    # depth 0, negative, NaN and inf take no part
    for bad in (0.0, -4.0, np.nan, np.inf):
        assert not sc.allocate_statement((-4, -4, 0), 1.0, (24, 24, 24), 1.0, 8.0, [cam], [np.full((12, 16), bad, F)]).any(), bad
    # allocated bricks stay, and the order of the views does not matter
    more = sc.allocate_statement((-4, -4, 0), 1.0, (24, 24, 24), 1.0, 0.0, [cam], [_one_pixel(8, 6, 20.0)], bricks=one)
    assert _set(more) == {(0, 0, 0), (0, 0, 1), (0, 0, 2)}


def test_mask_and_brick_major_index_by_hand():
    dims = (10, 9, 8)                       # 2 x 2 x 1 bricks
    bricks = np.array([[[True, False], [True, True]]])   # (0,0,0), (0,1,0), (1,1,0): ranks 0, 1, 2
    assert sc.brick_coords(bricks).tolist() == [[0, 0, 0], [0, 1, 0], [1, 1, 0]]
    lin = lambda i, j, k: (k * 9 + j) * 10 + i   # noqa: E731
    got = sc.brick_major_index(dims, bricks, [lin(0, 0, 0), lin(7, 7, 7), lin(8, 0, 0), lin(0, 8, 0), lin(9, 8, 3), lin(3, 8, 7)])
    assert got.tolist() == [0, 511, -1, 512, 2 * 512 + (3 * 8 + 0) * 8 + 1, 512 + (7 * 8 + 0) * 8 + 3]
    ex = sc.voxel_exists(dims, bricks)
    assert ex.shape == (8, 9, 10) and ex[:, :8, :8].all() and not ex[:, :8, 8:].any() and ex[:, 8:, :].all()
    f, w = tc.sphere_volume(dims, (4.3, 3.9, 3.4), 2.7)
    mf, mw, _ = sc.mask_dense(dims, bricks, f, w)
    assert (mw == ex).all() and (mf[~ex] == 0).all() and np.array_equal(mf[ex], f[ex])
    packed = sc.to_bricks(dims, bricks, mw)
    assert packed.shape == (3, 8, 8, 8) and packed[0].all() and packed[1, :, 0].all() and not packed[1, :, 1:].any()   # brick (0,1,0): j = 8 only
    assert packed[2, :, 0, :2].all() and not packed[2, :, :, 2:].any()


def test_renumbering_on_the_anchor():
    dims = (10, 9, 8)
    f, w = tc.sphere_volume(dims, (4.3, 3.9, 3.4), 2.7)
    dense = tc.mesh_statement(f, w, None, dims, (0, 0, 0), 1.0)
    keys, cells = sc.mesh_structure(f, w, dims)
    assert len(keys) == 410 and len(cells) == 816 and (np.diff(cells) >= 0).all()
    full = np.ones((1, 2, 2), bool)
    m = sc.sparse_mesh_statement(f, w, None, dims, (0, 0, 0), 1.0, full)
    topo = tc.topology(m["tri"])
    assert (topo["V"], topo["E"], topo["F"]) == (410, 1224, 816) and len(m["xyz"]) == 410 and topo["closed"] and topo["euler"] == 2
    assert sc.triangle_set(m) == sc.triangle_set(dense) and len(sc.triangle_set(m)) == 816
    # every owner of the anchor lies in brick (0, 0, 0) (the sphere spans i = 1.6 .. 7.0, j = 1.2 .. 6.6): brick-major order is the
    # dense order here, and only that brick matters.  The sphere of SHIFTED crosses the corner where eight bricks meet.
    assert np.array_equal(m["tri"], dense["tri"]) and np.array_equal(m["xyz"], dense["xyz"])
    lone = np.zeros((1, 2, 2), bool)
    lone[0, 0, 0] = True
    p = sc.sparse_mesh_statement(f, w, None, dims, (0, 0, 0), 1.0, lone)
    # no cell with a corner at i = 8 or j = 8 emits (nothing there is inside): without the other three bricks the mesh is the same,
    # so the anchor cannot show a boundary by losing one of them, and without brick (0, 0, 0) it is empty
    assert np.array_equal(p["tri"], dense["tri"]) and np.array_equal(p["xyz"], dense["xyz"])
    assert len(sc.sparse_mesh_statement(f, w, None, dims, (0, 0, 0), 1.0, ~lone)["tri"]) == 0
    dims, centre, radius = sc.SHIFTED
    f, w = tc.sphere_volume(dims, centre, radius)
    dense = tc.mesh_statement(f, w, None, dims, (0, 0, 0), 1.0)
    full = np.ones((2, 3, 3), bool)
    m = sc.sparse_mesh_statement(f, w, None, dims, (0, 0, 0), 1.0, full)
    topo = tc.topology(m["tri"])
    assert topo["closed"] and topo["euler"] == 2 and topo["F"] == len(dense["tri"]) and len(m["xyz"]) == len(dense["xyz"])
    assert sc.triangle_set(m) == sc.triangle_set(dense) and len(sc.triangle_set(m)) == len(dense["tri"])
    assert not np.array_equal(m["tri"], dense["tri"])                         # the order did change ...
    assert sorted(map(bytes, m["xyz"])) == sorted(map(bytes, dense["xyz"]))   # ... and nothing else
    keys, cells = sc.mesh_structure(f, w, dims)
    owner = sc.brick_major_index(dims, full, keys // 7)
    assert len(np.unique(owner // 512)) >= 4                                  # owners in several bricks
    # vertex r of the renumbered mesh is the one with the r-th smallest (brick-major owner, slot): its position is its owner's edge
    order = np.argsort(owner * 7 + keys % 7)
    assert np.array_equal(m["xyz"], dense["xyz"][order])
    # one brick removed: a boundary, no repeated half-edge, a subset of the full triangles
    part = full.copy()
    part[0, 1, 1] = False
    p = sc.sparse_mesh_statement(f, w, None, dims, (0, 0, 0), 1.0, part)
    topo = tc.topology(p["tri"])
    assert topo["manifold_with_boundary"] and not topo["closed"] and 0 < topo["F"] < len(dense["tri"])
    assert sc.triangle_set(p) < sc.triangle_set(dense)


def test_end_to_end_scene_is_covered_by_the_statement(pm):
    """the cap on the scene: every band voxel (a contribution with |s| <= trunc) of the four-camera sphere lies in a brick that
    statement A allocates at pad = 1"""
    dims, origin, voxel, trunc, cams, depths, _ = sc.sphere_scene(pm)
    bricks = sc.allocate_statement(origin, voxel, dims, trunc, 1.0, cams, depths)
    band = sc.band_voxels(origin, voxel, dims, trunc, cams, depths)
    assert band.any() and 0 < bricks.sum() <= 27
    assert not (band & ~sc.voxel_exists(dims, bricks)).any()
