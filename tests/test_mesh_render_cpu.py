"""mpmvs_surface_render_depth without a GPU: the symbols, every refusal that needs no device and what is answered on the host, the numpy
statement of mesh_render_common.py pinned on cases worked out by hand (the closed triangle, shared edges in both orientations, ties,
degenerate triangles, the camera plane), on a watertight height field and on a cube against the analytic ray-box depth;
mesh.triangle_coverage, tools/eval_depth.py --ground_truth_mesh through a stubbed renderer, and the host check program under the
sanitizers."""
import ctypes as C
import importlib
import importlib.util
import json
import os
import re
import subprocess

import numpy as np
import pytest

import mesh_render_common as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mpmvs_surface_render_depth", "mpmvs_surface_render_ms", "mpmvs_surface_render_work")
_P = C.c_void_p
F = np.float32
D = np.float64


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
    f = fns["surface_render_depth"]
    assert f.restype is C.c_int and f.argtypes == [_P, C.c_int, _P, _P, _P, C.POINTER(C.c_longlong)]
    f = fns["surface_render_ms"]
    assert f.restype is C.c_float and f.argtypes == [_P, C.POINTER(C.c_float)]
    f = fns["surface_render_work"]
    assert f.restype is C.c_int and f.argtypes == [_P, C.POINTER(C.c_longlong)]
    assert len(set(re.findall(r"\b(mpmvs_mesh_[a-z0-9_]+)\s*\(", header))) == 6   # the mesh section's own prefix keeps its six names


def test_kernels_live_in_a_header_of_their_own():
    text = open(os.path.join(ROOT, "mp-mvs_amd", "csrc", "pm_raster.hpp")).read()
    assert len(re.findall(r"^inline __global__", text, re.M)) == 4 and not re.findall(r"^__global__", text, re.M)
    assert "void k_scan_" not in text   # no second copy of a scan
    for k in ("k_raster_init", "k_raster_small", "k_raster_large", "k_raster_resolve"):
        assert f"void {k}(" in text
    assert "pm_raster.hpp" in open(os.path.join(ROOT, "mp-mvs_amd", "csrc", "mpmvs_mesh.hip")).read()
    assert "k_raster" not in open(os.path.join(ROOT, "mp-mvs_amd", "csrc", "pm_surface.hpp")).read()


def _handle(fns, m):
    xyz, tri = m["xyz"], m["tri"]
    h = _P()
    assert fns["mesh_create"](0, len(xyz), xyz.ctypes.data if len(xyz) else None, None, len(tri), tri.ctypes.data if len(tri) else None, C.byref(h)) == 0
    return h


def _hand_mesh():
    return mr.mesh(mr.at_pixels([(2, 1), (12, 1), (2, 9)], 2.0), [[0, 1, 2]])


def test_every_refusal_without_a_device_leaves_the_outputs_untouched(eng):
    _, fns = eng.load()
    abi = mr.abi()
    err = lambda: fns["last_error"](None).decode()   # noqa: E731
    render = fns["surface_render_depth"]
    h = _handle(fns, _hand_mesh())
    cam = mr.hand_camera()
    npix = mr.HAND_W * mr.HAND_H
    depth, tri = np.full((2, npix), 7, F), np.full((2, npix), 7, np.int32)
    counts = (C.c_longlong * 3)(7, 7, 7)
    untouched = lambda: bool((depth == 7).all() and (tri == 7).all()) and list(counts) == [7, 7, 7]   # noqa: E731
    cams = (abi.Camera * 2)(cam, cam)
    dp = (_P * 2)(depth[0].ctypes.data, depth[1].ctypes.data)
    tp = (_P * 2)(tri[0].ctypes.data, tri[1].ctypes.data)
    # the handle and the number of views first, also for n_views == 0
    assert render(None, 2, cams, dp, tp, counts) == -2 and "surface render" in err() and untouched()
    assert render(None, 0, cams, dp, tp, counts) == -2 and untouched()
    assert render(h, -1, cams, dp, tp, counts) == -2 and untouched()
    # no view: 0, nothing is read or written
    assert render(h, 0, None, None, None, None) == 0 and render(h, 0, cams, dp, tp, counts) == 0 and untouched()
    assert render(h, 2, None, dp, tp, counts) == -2 and untouched()
    assert render(h, 2, cams, None, tp, counts) == -2 and untouched()
    assert render(h, 2, cams, (_P * 2)(depth[0].ctypes.data, None), tp, counts) == -2 and "view 1" in err() and untouched()
    for field, value, code in (("width", 0, -2), ("height", 0, -2), ("width", -3, -2), ("height", -1, -2), ("width", (1 << 24) + 1, -3), ("height", (1 << 24) + 1, -3)):
        bad = mr.hand_camera()
        setattr(bad, field, value)
        assert render(h, 2, (abi.Camera * 2)(cam, bad), dp, tp, counts) == code and "view 1" in err() and untouched(), (field, value)
    bad = mr.hand_camera()
    bad.width, bad.height = 1 << 16, 1 << 15   # 2^31 pixels: one too many
    assert render(h, 2, (abi.Camera * 2)(cam, bad), dp, tp, counts) == -3 and "2^31" in err() and untouched()
    bad0, bad3 = mr.hand_camera(), mr.hand_camera()
    bad0.width, bad3.width = (1 << 24) + 1, 0
    assert render(h, 2, (abi.Camera * 2)(bad0, bad3), dp, tp, counts) == -2 and untouched()   # every -2 of every view before any -3
    ms4 = (C.c_float * 4)(7, 7, 7, 7)
    assert fns["surface_render_ms"](None, ms4) == 0.0 and list(ms4) == [7, 7, 7, 7]
    assert fns["surface_render_ms"](h, ms4) == 0.0 and list(ms4) == [0, 0, 0, 0]   # nothing has run
    assert fns["surface_render_ms"](h, None) == 0.0
    work = (C.c_longlong * 2)(7, 7)
    assert fns["surface_render_work"](None, work) == -2 and fns["surface_render_work"](h, None) == -2 and list(work) == [7, 7]
    assert fns["surface_render_work"](h, work) == 0 and list(work) == [0, 0]
    fns["mesh_destroy"](h)


def test_a_mesh_without_a_finite_triangle_is_answered_on_the_host(mesh):
    nan_mesh = mr.mesh(np.array([[0, 0, 2], [1, np.nan, 2], [0, 1, 2], [np.inf, 0, 2]], F), [[0, 1, 2], [1, 2, 3]])
    empty = mr.mesh(np.zeros((0, 3), F), np.zeros((0, 3), np.int32))
    no_tri = mr.mesh(np.array([[0, 0, 2], [1, 0, 2]], F), np.zeros((0, 3), np.int32))
    cams = [mr.hand_camera(), mr.pinhole(1.0, 0.0, 0.0, 1, 1), mr.pinhole(4.0, 2.0, 1.5, 5, 4)]
    for m in (nan_mesh, empty, no_tri):
        with mesh.Mesh(m["xyz"], m["tri"]) as h:
            depths, tris = h.render_depth(cams, want_tri=True)   # no device on this machine: a launch would raise
            assert [d.shape for d in depths] == [(12, 16), (1, 1), (4, 5)] and all(d.dtype == F and (d == 0).all() for d in depths)
            assert all(t.dtype == np.int32 and (t == -1).all() for t in tris)
            assert h.last_render_counts == {"pairs": 0, "covered": 0, "large_pairs": 0}
            assert h.render_ms() == (0.0, {"init": 0.0, "small": 0.0, "large": 0.0, "resolve": 0.0})
            assert h.render_work() == {"box_pixels": 0, "atomics": 0}
            assert isinstance(h.render_depth(cams), list) and h.render_depth([]) == []
        want_d, want_t, want_c = mr.statement(m["xyz"], m["tri"], cams)
        assert all((d == 0).all() for d in want_d) and all((t == -1).all() for t in want_t) and want_c.tolist() == [0, 0]
    with mesh.Mesh(_hand_mesh()["xyz"], _hand_mesh()["tri"]) as h:
        bad = mr.hand_camera()
        bad.width = 0
        with pytest.raises(ValueError, match="surface_render_depth"):
            h.render_depth([bad])


# ---- the statement by hand ---------------------------------------------------------------------------------------------------------------
def test_fronto_parallel_triangle_is_the_closed_triangle_at_depth_two():
    """K = [[8, 0, 2], [0, 8, 1], [0, 0, 1]], R = I, a triangle at z = 2 whose corners project onto the pixels (2, 1), (12, 1), (2, 9):
    legs of 10 and 8 pixels.  The closed triangle holds the pixels with 4 (x - 2) + 5 (y - 1) <= 40, x >= 2, y >= 1: per row y = 1 .. 9
    that is floor((40 - 5 (y - 1)) / 4) + 1 = 11, 9, 8, 7, 6, 4, 3, 2, 1 pixels, 51 in all."""
    px = [(2, 1), (12, 1), (2, 9)]
    m = _hand_mesh()
    d, a, pairs, covered, _ = mr.view_statement(m["xyz"], m["tri"], mr.hand_camera())
    rows = [11, 9, 8, 7, 6, 4, 3, 2, 1]
    assert (d != 0).sum(1).tolist() == [0] + rows + [0, 0] and covered == 51 == sum(rows) and pairs == 1
    assert np.array_equal(d != 0, mr.closed_triangle_pixels(*px, mr.HAND_W, mr.HAND_H))
    assert mr.same_bits(d[d != 0], np.full(51, 2.0, F)) and np.array_equal(a, np.where(d != 0, 0, -1))
    for x, y in px + [(7, 1), (2, 5), (7, 5)]:   # the corners, and pixel centres on the three edges ((7, 5): 4 * 5 + 5 * 4 = 40)
        assert d[y, x] == 2.0
    assert d[5, 8] == 0 and d[0, 2] == 0 and d[1, 1] == 0 and d[1, 13] == 0
    for order in ([0, 2, 1], [1, 2, 0], [2, 1, 0]):   # the other winding and another first corner: the same map
        d2, a2, _, _, _ = mr.view_statement(m["xyz"], [order], mr.hand_camera())
        assert mr.same_bits(d2, d) and np.array_equal(a2, a)


@pytest.mark.parametrize("second", ([1, 3, 2], [1, 2, 3], [3, 2, 1], [2, 1, 3]))
def test_two_triangles_sharing_a_diagonal_cover_the_closed_quad_once(second):
    """the quad (2, 1), (12, 1), (2, 9), (12, 9) at z = 2 split along the diagonal (12, 1) - (2, 9), the second triangle in both
    orientations and from either end of the shared edge: the closed quad, 11 x 9 pixels, none missing; the pixel centres on the diagonal
    ((12, 1), (7, 5), (2, 9)) belong to both and go to the smaller index"""
    xyz = mr.at_pixels([(2, 1), (12, 1), (2, 9), (12, 9)], 2.0)
    d, a, pairs, covered, _ = mr.view_statement(xyz, [[0, 1, 2], second], mr.hand_camera())
    inside = np.zeros((mr.HAND_H, mr.HAND_W), bool)
    inside[1:10, 2:13] = True
    assert pairs == 2 and covered == 99 and np.array_equal(d != 0, inside) and mr.same_bits(d[inside], np.full(99, 2.0, F))
    first = mr.closed_triangle_pixels((2, 1), (12, 1), (2, 9), mr.HAND_W, mr.HAND_H)
    assert np.array_equal(a, np.where(first, 0, np.where(inside, 1, -1)))
    assert [a[y, x] for x, y in ((12, 1), (7, 5), (2, 9))] == [0, 0, 0]
    d2, a2, _, _, _ = mr.view_statement(xyz, [second, [0, 1, 2]], mr.hand_camera())   # the other order: the diagonal changes hands
    assert mr.same_bits(d2, d) and [a2[y, x] for x, y in ((12, 1), (7, 5), (2, 9))] == [0, 0, 0]
    second_px = mr.closed_triangle_pixels((12, 1), (2, 9), (12, 9), mr.HAND_W, mr.HAND_H)
    assert np.array_equal(a2, np.where(second_px, 0, np.where(inside, 1, -1)))


def test_ties_go_to_the_smaller_index_and_the_nearer_triangle_wins():
    px = [(2, 1), (12, 1), (2, 9)]
    near, far = mr.at_pixels(px, 2.0), mr.at_pixels(px, 3.0)
    cam = mr.hand_camera()
    d, a, _, covered, _ = mr.view_statement(near, [[0, 1, 2], [0, 1, 2], [2, 0, 1]], cam)   # coincident
    assert covered == 51 and (a[d != 0] == 0).all() and (d[d != 0] == 2).all()
    xyz = np.concatenate([near, far])
    for tri, winner in (([[0, 1, 2], [3, 4, 5]], 0), ([[3, 4, 5], [0, 1, 2]], 1)):
        d, a, pairs, covered, _ = mr.view_statement(xyz, tri, cam)
        assert pairs == 2 and covered == 51 and (a[d != 0] == winner).all() and (d[d != 0] == 2).all()
    # a farther triangle that is larger shows around the nearer one
    big = mr.at_pixels([(0, 0), (15, 0), (0, 11)], 3.0)
    d, a, _, _, _ = mr.view_statement(np.concatenate([near, big]), [[3, 4, 5], [0, 1, 2]], cam)
    assert d[5, 3] == 2 and a[5, 3] == 1 and d[0, 0] == 3 and a[0, 0] == 0 and d[11, 15] == 0 and a[11, 15] == -1


def test_degenerate_and_non_finite_triangles_cover_what_the_rules_say():
    """a == b == c: every normal is u x u = 0 exactly (u1*u2 - u2*u1), every E is 0, S = 0: no candidate.  a == b != c: nab = 0, and
    nca = qc x qa is nbc = qa x qc with every bit negated, so E1 = -E0 and E2 = 0: a candidate needs E0 = 0, and then S = 0: none.
    Collinear corners at z = 2 projecting onto (2, 1), (7, 5), (12, 9): det is 0 but for rounding, and here exactly 0 (small integers
    times powers of two), the three E vanish together on the line and S with them: none.  All three take part; a triangle with a
    non-finite vertex does not."""
    cam = mr.hand_camera()
    xyz = np.concatenate([mr.at_pixels([(2, 1), (7, 5), (12, 9), (12, 1)], 2.0), [[np.nan, 0, 2], [0, np.inf, 2], [0, 0, -np.inf]]]).astype(F)
    for tri, pairs in (([[0, 0, 0]], 1), ([[0, 0, 3]], 1), ([[3, 0, 0]], 1), ([[0, 1, 2]], 1), ([[0, 3, 4]], 0), ([[5, 0, 3]], 0), ([[0, 3, 6]], 0)):
        d, a, p, covered, _ = mr.view_statement(xyz, tri, cam)
        assert (p, covered) == (pairs, 0) and (d == 0).all() and (a == -1).all(), tri
    d, a, p, covered, _ = mr.view_statement(xyz, [[0, 0, 0], [4, 0, 3], [0, 3, 2], [0, 0, 3]], cam)   # among them one real triangle
    assert p == 3 and covered > 0 and (a[d != 0] == 2).all() and not np.isnan(d).any()


def test_the_camera_plane():
    cam = mr.pinhole(80.0, 47.5, 31.5, 96, 64)
    # wholly behind, and in the plane itself (max q.z = 0): no part
    for xyz in ([[-1, -1, -2], [1, -1, -3], [0, 1, -4]], [[-1, 0, 0], [1, 0, 0], [0, 1, 0]], [[-1, 0, 0], [1, 0, -1], [0, 1, 0]]):
        d, a, pairs, covered, _ = mr.view_statement(xyz, [[0, 1, 2]], cam)
        assert pairs == 0 and covered == 0 and (d == 0).all() and (a == -1).all()
    # crossing: two corners at z = +5, one at z = -5, seen from the origin.  The far edge projects onto row 15.5, columns 31.5 .. 63.5;
    # the visible part runs from there towards the camera plane, where it leaves the image downwards.
    xyz = [[-1, -1, 5], [1, -1, 5], [0, 2, -5]]
    d, a, pairs, covered, _ = mr.view_statement(xyz, [[0, 1, 2]], cam)
    got = d[d != 0]
    print(f"crossing: {covered} pixels, depths {got.min():.6f} .. {got.max():.6f}, rows {np.flatnonzero((d != 0).any(1))[[0, -1]]}")
    assert pairs == 1 and covered == CROSSING_PIXELS and (got > 0).all() and got.max() <= 5.0
    assert abs(float(got.min()) - CROSSING_NEAREST) <= 1e-6 and (d[:16] == 0).all() and (d[16:] != 0).any(1).all()
    # the exact depth on the triangle's axis of symmetry x = 0: the point (0, -1 + 3 s, 5 - 10 s) projects onto row 31.5 + 80 (3 s - 1) / (5 - 10 s)
    col = d[:, [47, 48]]
    for y in (16, 30, 63):
        s = (5 * (y - 31.5) + 80) / (240 + 10 * (y - 31.5))
        assert abs(col[y, 0] - (5 - 10 * s)) <= 0.08 and col[y, 0] == col[y, 1]   # half a pixel off the axis, in both columns alike


CROSSING_PIXELS = 3616   # re-derived with this statement
CROSSING_NEAREST = 0.720721


def test_watertight_height_field():
    """a 24 x 24 height field with alternating diagonals seen from four cameras that look into its interior: first the cameras are
    shown to see nothing but the field (every ray crosses the slab of the heights inside the field's outline), then no pixel is left
    uncovered, as built and with every third triangle's winding reversed; the two give the same depth maps"""
    cams = mr.height_field_cameras()
    assert len(cams) == 4 and all(mr.fills_image(c) for c in cams)
    maps = {}
    for rev in (0, 3):
        hf = mr.height_field(24, rev)
        assert len(hf["tri"]) == 2 * 23 * 23
        depths, tris, counts = mr.cached(("height field", rev), lambda: mr.statement(hf["xyz"], hf["tri"], cams))
        holes = [int((d == 0).sum()) for d in depths]
        print("holes", rev, holes)
        assert holes == [0, 0, 0, 0] and counts.tolist() == [4 * len(hf["tri"]), 4 * 96 * 64]
        assert all((t >= 0).all() for t in tris)
        maps[rev] = depths
    assert all(mr.same_bits(a, b) for a, b in zip(maps[0], maps[3]))


CUBE_DEVIATION = 5.85e-8   # measured with this statement: the rounding of the depth to fp32, 2^-24


def test_cube_against_the_analytic_ray_box_depth():
    cb = mr.cube()
    cams = mr.cube_cameras()
    assert len(cams) == 12
    depths, _, counts = mr.cached("cube", lambda: mr.statement(cb["xyz"], cb["tri"], cams))
    hits = missed = extra = 0
    worst = 0.0
    for c, d in zip(cams, depths):
        hit, miss, z = mr.ray_box(c, mr.CUBE_HALF, slack=1e-9)
        hits += int(hit.sum())
        missed += int((hit & (d == 0)).sum())
        extra += int((miss & (d != 0)).sum())
        worst = max(worst, float((np.abs(d[hit].astype(D) - z[hit]) / z[hit]).max()))
    print(f"cube: {hits} hits, {missed} missed, {extra} extra, largest relative deviation {worst:.3e}")
    assert hits > 10000 and missed == 0 and extra == 0
    assert worst <= 4 * CUBE_DEVIATION


def test_triangle_coverage_by_hand(mesh):
    maps = [np.array([[0, 0, -1], [2, 2, 2]], np.int32), np.array([[-1]], np.int32), np.array([[3, 3, 3, 3, 0]], np.int32)]
    cov = mesh.triangle_coverage(maps, 4)
    assert cov.dtype == np.int64 and cov.tolist() == [[2, 0, 3, 0], [0, 0, 0, 0], [1, 0, 0, 4]]
    assert mesh.triangle_coverage([], 3).shape == (0, 3) and mesh.triangle_coverage(maps[1:2], 0).shape == (1, 0)
    with pytest.raises(ValueError, match="triangle 3"):
        mesh.triangle_coverage(maps, 3)
    m = _hand_mesh()
    _, a, _, covered, _ = mr.view_statement(m["xyz"], m["tri"], mr.hand_camera())
    assert mesh.triangle_coverage([a], 1).tolist() == [[covered]]


# ---- tools/eval_depth.py --ground_truth_mesh through a stubbed renderer ----------------------------------------------------------------------
class _StubMesh:
    calls = []

    def __init__(self, xyz, tri, rgb=None, device=0):
        self.xyz, self.tri = np.ascontiguousarray(xyz, F).reshape(-1, 3), np.ascontiguousarray(tri, np.int32).reshape(-1, 3)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass

    def render_depth(self, cams, want_tri=False):
        cams = list(cams)
        _StubMesh.calls.append(len(cams))
        depths, _, counts = mr.statement(self.xyz, self.tri, cams)
        self.last_render_counts = {"pairs": int(counts[0]), "covered": int(counts[1]), "large_pairs": 0}
        return depths

    def render_ms(self):
        return 0.25, {"init": 0.0, "small": 0.25, "large": 0.0, "resolve": 0.0}


def test_eval_depth_against_a_mesh(pm, hostlib, mesh, tmp_path, capsys, monkeypatch):
    spec = importlib.util.spec_from_file_location("eval_depth_tool_mesh", os.path.join(ROOT, "tools", "eval_depth.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    depthmap = importlib.import_module("mp-mvs_amd.depthmap")
    W, H = 12, 9
    cams = pm.synth.scene_cameras(W, H, [(0, 0, 0), (0.2, 0, 0), (0, 0.2, 0)])
    rng = np.random.default_rng(3)
    imgs = [np.rint(rng.uniform(0, 255, (H, W))).astype(F) for _ in cams]
    dense = tmp_path / "dense"
    hostlib.write_dataset(str(dense), cams, imgs, [[1, 2], [0, 2], [0, 1]])
    # the ground truth: a wall across the views at z = 6 in the first camera's frame, given in a frame moved by (1, 2, 3)
    R0, t0 = np.array(cams[0].R[:], D).reshape(3, 3), np.array(cams[0].t[:], D)
    wall_cam = np.array([[-40, -40, 6], [40, -40, 6], [40, 40, 6], [-40, 40, 6]], D)
    wall = (np.linalg.inv(R0) @ (wall_cam - t0).T).T
    surface = tmp_path / "wall.ply"
    mesh.write_ply_mesh(str(surface), (wall - np.array([1, 2, 3])).astype(F), [[0, 1, 2], [0, 2, 3]])
    T = np.eye(4)
    T[:3, 3] = (1, 2, 3)
    np.savetxt(str(tmp_path / "T.txt"), T)
    est = [np.full((H, W), 6.0, F) + rng.normal(0, 0.05, (H, W)).astype(F) for _ in cams]
    for i in (0, 1):   # view 2 has no result folder: not scored, not rendered
        os.makedirs(dense / "MPMVS" / f"2333_{i:08d}")
        hostlib.write_dmb(str(dense / "MPMVS" / f"2333_{i:08d}" / "depths.dmb"), est[i])
    monkeypatch.setattr(mesh, "Mesh", _StubMesh)
    _StubMesh.calls = []
    argv = ["--dense_folder", str(dense), "--ground_truth_mesh", str(surface), "--transform", str(tmp_path / "T.txt"), "--tolerances", "0.02,0.1"]
    res = tool.main(argv)
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == res
    assert _StubMesh.calls == [2]   # all views in one call
    assert res["ground_truth"] == "rendered_mesh" and res["render_device_ms"] == 0.25
    assert res["render_counts"] == {"pairs": 4, "covered": 2 * W * H, "large_pairs": 0}
    gt = mr.statement((wall).astype(F), [[0, 1, 2], [0, 2, 3]], [depthmap.camera_at_size(c, W, H, W, H) for c in cams[:2]])[0]
    assert abs(float(gt[0][4, 6]) - 6.0) <= 1e-5
    want = [depthmap.score(est[i], gt[i], [0.02, 0.1]) for i in (0, 1)]
    assert res["views"]["00000000"] == want[0] and res["views"]["00000001"] == want[1] and res["pooled"] == depthmap.pool(want)
    assert 0 < want[0]["tolerances"][0]["within"] < want[0]["tolerances"][1]["within"]
    for bad in (argv + ["--splat", "1"], argv + ["--occl", "0.02"], argv + ["--ground_truth", "scan.ply"], argv + ["--gt_depth_dir", str(tmp_path), "--gt_format", "dmb"],
                argv[:2] + ["--ground_truth_mesh", str(tmp_path / "missing.ply")]):
        with pytest.raises(SystemExit):
            tool.main(bad)
    with pytest.raises(SystemExit, match="exactly one"):
        tool.main(argv[:2])


def test_check_program_under_the_host_sanitizers(tmp_path):
    """tools/mesh_render_check.cpp: the per-thread bodies of pm_raster.hpp replayed on the host in scrambled orders against a plain
    loop, under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program, thinned to a few seconds"""
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    exe = str(tmp_path / "mesh_render_check")
    subprocess.run([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                    "-I" + os.path.join(ROOT, "mp-mvs_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tools", "mesh_render_check.cpp")], check=True, cwd=str(tmp_path))
    run = subprocess.run([exe, "4"], capture_output=True, text=True, cwd=str(tmp_path))
    lines = run.stdout.strip().splitlines()
    assert run.returncode == 0 and lines[-1] == "all equal", run.stdout[-2000:] + run.stderr[-2000:]
    cases = lines[:-1]
    assert len(cases) >= 21 and all(ln.endswith(": equal") for ln in cases)
    assert sum("large 0:" in ln and "listed 0 of" not in ln for ln in cases) >= 7   # the large-triangle path ran,
    assert sum("(0 shared by blocks)" not in ln for ln in cases) >= 2               # its block-shared launch too
    assert sum("large 1073741824:" in ln and "listed 0 of" in ln for ln in cases) >= 7   # and the small one alone
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-2000:]
