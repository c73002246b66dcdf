"""mpmvs_simplify_mesh without a GPU: the symbols, every refusal (found before the device is touched, outputs untouched), what is
answered on the host, the numpy statement of mesh_simplify_common.py on cases worked out by hand, its invariances, the seeded sweep's
census, the tool's argument parsing and PLY reading up to the call, and the host check program under the sanitizers."""
import ctypes as C
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import mesh_clean_common as mc
import mesh_simplify_common as ms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mpmvs_simplify_mesh", "mpmvs_simplify_mesh_ms")
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
    f = fns["simplify_mesh"]
    PP = C.POINTER(_P)
    assert f.restype is C.c_longlong and f.argtypes == [_P, C.c_float, C.c_int, PP, PP, PP, C.POINTER(C.c_longlong), _P, PP, PP, PP, C.POINTER(C.c_longlong)]
    f = fns["simplify_mesh_ms"]
    assert f.restype is C.c_int and f.argtypes == [_P, C.POINTER(C.c_float)]
    # the clustering passes are shared, not copied: one definition each, included by both translation units
    csrc = os.path.join(ROOT, "mp-mvs_amd", "csrc")
    simp = open(os.path.join(csrc, "pm_simplify.hpp")).read()
    assert '#include "pm_voxel.hpp"' in simp and "void k_voxel_" not in simp and "void k_cloud_" not in simp and "void k_scan_" not in simp
    assert '#include "pm_simplify.hpp"' in open(os.path.join(csrc, "mpmvs_mesh.hip")).read()
    for header_name, kernels in (("pm_voxel.hpp", 5), ("pm_cloud.hpp", 6)):
        text = open(os.path.join(csrc, header_name)).read()
        assert len(re.findall(r"^inline __global__", text, re.M)) == kernels and not re.findall(r"^__global__", text, re.M)


def _handle(fns, m):
    xyz, tri, rgb = m["xyz"], m["tri"], m["rgb"]
    h = _P()
    rc = fns["mesh_create"](0, len(xyz), xyz.ctypes.data if len(xyz) else None, None if rgb is None else rgb.ctypes.data, len(tri), tri.ctypes.data if len(tri) else None,
                            C.byref(h))
    assert rc == 0
    return h


class _Outs:
    """the outputs of a call, filled with markers that a refusal must leave"""

    def __init__(self, n):
        self.px, self.pc, self.pt, self.pn, self.pp, self.ps = _P(0x11), _P(0x22), _P(0x33), _P(0x44), _P(0x55), _P(0x66)
        self.mo, self.counts, self.cluster_of = C.c_longlong(77), (C.c_longlong * 3)(7, 7, 7), np.full(max(n, 1), 7, np.int32)

    def args(self, color, **null):
        a = dict(xyz=C.byref(self.px), rgb=C.byref(self.pc) if color else None, tri=C.byref(self.pt), m=C.byref(self.mo), cluster_of=self.cluster_of.ctypes.data,
                 count=C.byref(self.pn), placed=C.byref(self.pp), src=C.byref(self.ps), counts=self.counts)
        a.update(null)
        return [a[k] for k in ("xyz", "rgb", "tri", "m", "cluster_of", "count", "placed", "src", "counts")]

    def untouched(self):
        return ((self.px.value, self.pc.value, self.pt.value, self.pn.value, self.pp.value, self.ps.value, self.mo.value) == (0x11, 0x22, 0x33, 0x44, 0x55, 0x66, 77)
                and list(self.counts) == [7, 7, 7] and bool((self.cluster_of == 7).all()))


def test_refusals_write_nothing_and_need_no_device(eng):
    _, fns = eng.load()
    err = lambda: fns["last_error"](None).decode()   # noqa: E731
    o = _Outs(4)
    assert fns["simplify_mesh"](None, 1.0, 1, *o.args(False)) == -2 and "mesh simplify" in err() and o.untouched()
    ms7 = (C.c_float * 7)(*([7.0] * 7))
    assert fns["simplify_mesh_ms"](None, ms7) == -2 and list(ms7) == [7.0] * 7
    for color in (False, True):
        m = mc.tetrahedra(3, 1, color=color)
        h = _handle(fns, m)
        o = _Outs(len(m["xyz"]))
        for cell in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
            assert fns["simplify_mesh"](h, cell, 1, *o.args(color)) == -2 and "cell" in err() and o.untouched(), cell
        for placement in (-1, 2, 7):
            assert fns["simplify_mesh"](h, 1.0, placement, *o.args(color)) == -2 and "placement" in err() and o.untouched()
        for null in ("xyz", "tri", "m"):
            assert fns["simplify_mesh"](h, 1.0, 1, *o.args(color, **{null: None})) == -2 and o.untouched(), null
        wrong = dict(rgb=None) if color else dict(rgb=C.byref(o.pc))
        assert fns["simplify_mesh"](h, 1.0, 0, *o.args(color, **wrong)) == -2 and "colour" in err() and o.untouched()
        assert fns["simplify_mesh_ms"](h, None) == -2
        assert fns["simplify_mesh_ms"](h, ms7) == 0 and list(ms7) == [0.0] * 7   # nothing has run
        fns["mesh_destroy"](h)
    # -3: the cell-span limit of the voxel call, and the text names the axis
    for axis in range(3):
        xyz = np.zeros((3, 3), F)
        xyz[1, axis] = 3.0e6    # 3e6 cells of edge 1 along this axis alone: more than 2^21
        xyz[2, (axis + 1) % 3] = 1000.0
        h = _handle(fns, mc._mesh(xyz, [[0, 1, 2]]))
        o = _Outs(3)
        assert fns["simplify_mesh"](h, 1.0, 1, *o.args(False)) == -3 and o.untouched()
        assert f"along {'xyz'[axis]}" in err() and "2^21" in err(), err()
        assert fns["simplify_mesh"](h, 0.5, 0, *o.args(False, cluster_of=None, count=None, placed=None, src=None, counts=None)) == -3 and o.untouched()
        fns["mesh_destroy"](h)


def test_span_limit_is_the_voxel_calls(eng):
    """the top cell may be 2^21 - 1 and no more: with the lowest vertex at a cell centre, a vertex 2^21 cells above it is refused"""
    _, fns = eng.load()
    xyz = np.array([[0, 0, 0], [0, 2.0 ** 21, 0], [np.nan, 0, 0]], F)
    h = _handle(fns, mc._mesh(xyz, np.zeros((0, 3), np.int32)))
    o = _Outs(3)
    assert fns["simplify_mesh"](h, 1.0, 0, *o.args(False)) == -3 and o.untouched() and "along y" in fns["last_error"](None).decode()
    fns["mesh_destroy"](h)


def test_nothing_to_do_is_answered_on_the_host(mesh):
    """n == 0 and a mesh without a finite vertex: no device is opened (this test runs without one)"""
    nan = np.full((4, 3), np.nan, F)
    nan[1] = [1, np.inf, 2]
    for rgb in (None, np.arange(12, dtype=np.uint8).reshape(4, 3)):
        for placement in ("mean", "quadric"):
            with mesh.Mesh(nan, [[0, 1, 2], [1, 1, 3]], rgb) as h:
                out = h.simplify(0.5, placement)
                assert out["xyz"].shape == (0, 3) and out["tri"].shape == (0, 3) and out["count"].shape == (0,) and out["placed"].shape == (0,)
                assert out["tri_src"].shape == (0,) and (out["rgb"] is None) == (rgb is None) and (rgb is None or out["rgb"].shape == (0, 3))
                assert out["cluster_of"].tolist() == [-1] * 4 and out["counts"] == {"non_finite": 2, "collapsed": 0, "duplicates": 0}
                assert all(v == 0.0 for v in h.simplify_ms().values()) and list(h.simplify_ms()) == list(mesh.SIMPLIFY_PASSES)
                ms.assert_same(out, ms.statement(mc._mesh(nan, [[0, 1, 2], [1, 1, 3]], rgb), 0.5, mesh.PLACEMENTS[placement]))
            with mesh.Mesh(np.zeros((0, 3), F), np.zeros((0, 3), np.int32), None if rgb is None else np.zeros((0, 3), np.uint8)) as h:
                out = h.simplify(0.5, placement)
                assert out["xyz"].shape == (0, 3) and out["tri"].shape == (0, 3) and out["cluster_of"].shape == (0,)
                assert out["counts"] == {"non_finite": 0, "collapsed": 0, "duplicates": 0}
    with mesh.Mesh(nan, [[0, 1, 2]]) as h:
        with pytest.raises(ValueError, match="placement"):
            h.simplify(1.0, "median")
        with pytest.raises(Exception, match="cell"):
            h.simplify(0.0)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.mark.parametrize("cell", ms.CUBE_CELLS)
def test_cube_corners_stay_corners_with_quadrics_only(cell):
    """six faces of 32 x 32 quads: a corner's cluster holds three planes, x = const, y = const and z = const, and their meeting point
    is the corner; the mean of the cluster's vertices lies inside the cube"""
    cu = ms.cube()
    q, mean = ms.statement(cu, cell, 1), ms.statement(cu, cell, 0)

    def nearest(w):   # L1 distance of every cube corner to the nearest output vertex, in cells
        return np.abs(w["xyz"].astype(D)[None] - ms.CUBE_CORNERS[:, None]).sum(2).min(1) / cell
    print("corner distance in cells: quadric", nearest(q).max(), "mean", nearest(mean).min(), nearest(mean).max())
    assert (nearest(q) <= 1e-5).all()          # the fp32 ulp at 1.0 is under 1e-6 cells here
    assert (nearest(mean) > 0.1).all()
    assert (q["placed"] == 1).all() and q["counts"]["duplicates"] == 0 and q["counts"]["non_finite"] == 0
    assert (mean["placed"] == 0).all() and np.array_equal(q["tri"], mean["tri"]) and np.array_equal(q["count"], mean["count"])
    # every output vertex of the quadric placement lies on the cube's surface: on a face, an edge or a corner
    d = np.minimum(np.abs(q["xyz"].astype(D)), np.abs(q["xyz"].astype(D) - 1.0)).min(1)
    assert d.max() <= 1e-5 * cell


def test_plane_is_placed_everywhere_and_stays_the_mean():
    p = ms.plane()
    for cell in (2.5, 1.0, 7.0):
        q, mean = ms.statement(p, cell, 1), ms.statement(p, cell, 0)
        assert (q["placed"] == 1).all() and len(q["placed"]) > 1
        ulp = np.abs(q["xyz"].view(np.int32).astype(np.int64) - mean["xyz"].view(np.int32).astype(np.int64))
        assert ulp.max() <= 1, ulp.max()   # one plane, one eigenvalue: the mean only moves along the normal, and it lies on the plane


def test_tent_falls_back_when_the_planes_meet_outside_the_cell():
    # s / c = 0.8 / 0.6: the planes meet at y = -0.4 * 0.8 / 0.6 = -0.533, outside the cell [-0.5, 0.5]: the mean of A and B, (0, 0, 0)
    w = ms.statement(ms.tent(0.8, 0.6), 1.0, 1)
    k = int(w["cluster_of"][1])
    assert w["cluster_of"][4] == k and w["count"][k] == 2 and w["T"][k] == 2
    assert w["placed"][k] == 2 and np.array_equal(_bits(w["xyz"][k]), _bits(ms.statement(ms.tent(0.8, 0.6), 1.0, 0)["xyz"][k]))
    assert np.abs(w["xyz"][k].astype(D)).max() < 1e-6
    assert w["placed"][int(w["cluster_of"][0])] == 0   # the anchor vertex: no triangle, no plane
    # s / c = 0.6 / 0.8: y = -0.3, inside
    w = ms.statement(ms.tent(0.6, 0.8), 1.0, 1)
    k = int(w["cluster_of"][1])
    assert w["placed"][k] == 1 and np.abs(w["xyz"][k].astype(D) - [0.0, -0.3, 0.0]).max() < 1e-6, w["xyz"][k]
    assert w["counts"] == {"non_finite": 0, "collapsed": 0, "duplicates": 0} and len(w["tri"]) == 2


def test_one_cell_and_no_merge():
    a = mc.anchor()
    w = ms.statement(a, 100.0, 1)   # a cell so large that everything is one cluster
    assert len(w["xyz"]) == 1 and w["tri"].shape == (0, 3) and w["counts"] == {"non_finite": 0, "collapsed": 816, "duplicates": 0} and w["count"].tolist() == [410]
    for placement in (0, 1):
        w = ms.statement(a, 2.0 ** -16, placement)   # a cell so small that nothing merges
        assert np.array_equal(w["tri"], a["tri"]) and np.array_equal(w["tri_src"], np.arange(816)) and np.array_equal(w["cluster_of"], np.arange(410))
        assert np.abs(w["xyz"].astype(D) - a["xyz"].astype(D)).max() <= 2.0 ** -16 and (w["count"] == 1).all()
    assert (w["placed"] != 0).all()   # every vertex of the sphere has its triangles' planes; in so small a cell many minimisers fall outside


def test_duplicates_and_degenerates_by_hand():
    w = ms.statement(ms.duplicates(), 1.0, 1)
    assert w["cluster_of"].tolist() == [0, 1, 2, 3]
    # the first of each key survives, in its own orientation: (1, 2, 0) and not (0, 1, 2); (3, 2, 1) and not (1, 2, 3)
    assert w["tri"].tolist() == [[1, 2, 0], [3, 2, 1]] and w["tri_src"].tolist() == [0, 6] and w["counts"] == {"non_finite": 0, "collapsed": 0, "duplicates": 6}
    w = ms.statement(ms.degenerate(), 1.0, 1)
    assert w["cluster_of"].tolist() == [0, 1, 2, -1, 3, 0]
    # (0, 0, 1) and (0, 5, 1) collapse (vertices 0 and 5 share a cell); (1, 3, 2) and (3, 3, 3) name the NaN vertex -- a repeated index
    # on a non-finite vertex counts as non-finite; (5, 2, 1) lands on the key of (0, 1, 2)
    assert w["counts"] == {"non_finite": 2, "collapsed": 2, "duplicates": 1} and w["tri"].tolist() == [[0, 1, 2], [1, 3, 2]] and w["tri_src"].tolist() == [0, 4]


def test_triangle_order_does_not_show_in_the_vertices():
    for m, cell in ((ms.cube(8), 0.3), (mc.anchor(), 1.7), (ms.sweep_case(5)["mesh"], ms.sweep_case(5)["cell"])):
        base = ms.statement(m, cell, 1)
        perm = np.random.default_rng(3).permutation(len(m["tri"]))
        got = ms.statement(mc._mesh(m["xyz"], m["tri"][perm], m["rgb"]), cell, 1)
        for k in ("xyz", "placed", "count", "cluster_of"):
            assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint8), np.ascontiguousarray(base[k]).view(np.uint8)), k
        assert got["counts"] == base["counts"] and len(got["tri"]) == len(base["tri"])


def test_a_power_of_two_scales_exactly():
    for m, cell in ((ms.cube(8), 0.3), (mc.anchor(), 1.7), (ms.tent(0.6, 0.8), 1.0)):
        base = ms.statement(m, cell, 1)
        assert (base["placed"] == 1).any()
        for p in (-40, 40):
            got = ms.statement(ms.scaled(m, p), float(F(cell)) * 2.0 ** p, 1)
            for k in ("tri", "placed", "cluster_of", "count", "tri_src"):
                assert np.array_equal(got[k], base[k]), (k, p)
            assert np.array_equal(got["xyz"].astype(D), base["xyz"].astype(D) * 2.0 ** p), p


def test_sweep_census():
    """conditions on the statement alone, so that the sweep cannot quietly degenerate"""
    c = ms.sweep_census()
    print(c)
    assert c["placed0"] >= 5 and c["placed1"] >= 5 and c["placed2"] >= 5
    assert c["duplicates"] >= 20 and c["collapsed"] >= 30
    assert c["non_finite"] >= 3 and 5 <= c["coloured"] <= 35


def test_tool_reads_its_arguments_and_its_ply_without_a_device(mesh, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        tool = importlib.import_module("simplify_mesh")
    finally:
        sys.path.pop(0)
    m = mc.tetrahedra(6, 2, color=True)
    src, dst = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    mesh.write_ply_mesh(src, m["xyz"], m["tri"], m["rgb"])
    args = tool.parse_args(["--input", src, "--output", dst, "--cell", "0.5"])
    assert (args.cell, args.placement, args.keep_unreferenced, args.normals, args.device) == (0.5, "quadric", False, False, 0)
    args = tool.parse_args(["--input", src, "--output", dst, "--cell", "2", "--placement", "mean", "--keep_unreferenced", "--normals"])
    assert (args.cell, args.placement, args.keep_unreferenced, args.normals) == (2.0, "mean", True, True)
    got, head = tool.load(args)   # up to the call; the call itself needs the device
    assert np.array_equal(_bits(got["xyz"]), _bits(m["xyz"])) and np.array_equal(got["tri"], m["tri"]) and np.array_equal(got["rgb"], m["rgb"])
    assert head == {"input": src, "n": len(m["xyz"]), "m": len(m["tri"]), "cell": 2.0, "placement": "mean"}
    for bad in (["--cell", "0"], ["--cell", "-1"], ["--cell", "nan"], ["--cell", "inf"], ["--cell", "1", "--placement", "median"], []):
        with pytest.raises(SystemExit):
            tool.parse_args(["--input", src, "--output", dst] + bad)
    args = tool.parse_args(["--input", str(tmp_path / "missing.ply"), "--output", dst, "--cell", "1"])
    with pytest.raises(SystemExit):
        tool.load(args)


def test_check_program_under_the_host_sanitizers(tmp_path):
    """tools/mesh_simplify_check.cpp: every new per-thread body replayed on the host in scrambled orders, the insert also with all probes
    interleaved at random, against plain loops, under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program"""
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    exe = str(tmp_path / "mesh_simplify_check")
    subprocess.run([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                    "-I" + os.path.join(ROOT, "mp-mvs_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tools", "mesh_simplify_check.cpp")], check=True, cwd=str(tmp_path))
    run = subprocess.run([exe], capture_output=True, text=True, cwd=str(tmp_path))
    lines = run.stdout.strip().splitlines()
    assert run.returncode == 0 and lines[-1] == "all equal", run.stdout[-2000:] + run.stderr[-2000:]
    cases = lines[:-1]
    assert len(cases) >= 30 and all(ln.endswith(": equal") for ln in cases)
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-2000:]
