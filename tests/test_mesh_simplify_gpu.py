"""mpmvs_simplify_mesh on the GPU against the numpy statement of mesh_simplify_common.py, bit for bit: both placements on the named
scenes, the shapes at which each kernel can still go wrong (a second round of the tile scan, 70 001 inserts on one slot in both
orders, 70 001 quadric terms on one cluster, runs of taken slots), the invariances, NULL optional outputs, the untouched handle, the
seeded sweep, mesh.simplify against the composed statements, and tools/simplify_mesh.py and tools/mesh_ply.py --simplify as fresh
child processes."""
import ctypes as C
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_clean_common as mc
import mesh_simplify_common as ms
import tsdf_sparse_common as sc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
D = np.float64
PLACEMENTS = ("mean", "quadric")


@pytest.fixture(scope="module")
def mesh(pm):
    return importlib.import_module("mp-mvs_amd.mesh")


@pytest.fixture(scope="module")
def cloud(pm):
    return importlib.import_module("mp-mvs_amd.cloud")


def _handle(mesh, m):
    return mesh.Mesh(m["xyz"], m["tri"], m["rgb"])


def _check(mesh, m, cell, what, placements=PLACEMENTS):
    """both placements on one handle against the statement -> the quadric result"""
    out = None
    with _handle(mesh, m) as h:
        for placement in placements:
            out = h.simplify(cell, placement)
            ms.assert_same(out, ms.statement(m, cell, mesh.PLACEMENTS[placement]), f"{what} {placement}")
    return out


def _coloured(m, seed=1):
    return mc._mesh(m["xyz"], m["tri"], np.random.default_rng(seed).integers(0, 256, m["xyz"].shape))


def test_mean_placement_is_the_voxel_downsampling_itself(mesh, cloud):
    """placement 0 against mpmvs_cloud_voxel_downsample on the same vertices: xyz, rgb, count and cluster_of"""
    for m, cell in ((_coloured(mc.anchor()), 1.3), (mc.plant_nonfinite(_coloured(mc.two_spheres())), 0.9), (mc.named_meshes()["tetrahedra"], 4.0), (ms.cube(), 0.07)):
        v = cloud.voxel_downsample(m["xyz"], cell, colors=m["rgb"], want_map=True)
        with _handle(mesh, m) as h:
            out = h.simplify(cell, "mean")
        assert np.array_equal(out["xyz"].view(np.uint32), v["xyz"].view(np.uint32)) and np.array_equal(out["count"], v["count"])
        assert np.array_equal(out["cluster_of"], v["voxel_of"]) and (m["rgb"] is None or np.array_equal(out["rgb"], v["colors"]))
        assert not out["placed"].any()


SCENES = {
    "anchor": lambda: (mc.anchor(), 1.3),
    "anchor_coloured_fine": lambda: (_coloured(mc.anchor()), 0.4),
    "two_spheres": lambda: (mc.two_spheres(), 1.1),
    "cube_0.25": lambda: (ms.cube(), 0.25),
    "cube_0.1": lambda: (ms.cube(), 0.1),
    "cube_0.07": lambda: (ms.cube(), 0.07),
    "tent_out": lambda: (ms.tent(0.8, 0.6), 1.0),
    "tent_in": lambda: (ms.tent(0.6, 0.8), 1.0),
    "plane": lambda: (ms.plane(), 2.5),
    "non_finite": lambda: (mc.plant_nonfinite(_coloured(mc.two_spheres())), 0.8),
    "duplicates": lambda: (ms.duplicates(), 1.0),
    "degenerate": lambda: (ms.degenerate(), 1.0),
    "one_cell": lambda: (mc.anchor(), 100.0),
    "no_merge": lambda: (mc.anchor(), 2.0 ** -16),
    "no_triangles": lambda: (mc._mesh(mc.anchor()["xyz"], np.zeros((0, 3), np.int32)), 1.0),
    "random_keys_4096_over_64": lambda: (ms.random_keys(), 1.0),
}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_scene_equals_the_statement(mesh, name):
    m, cell = SCENES[name]()
    out = _check(mesh, m, cell, name)
    if name.startswith("cube"):
        d = np.abs(out["xyz"].astype(D)[None] - ms.CUBE_CORNERS[:, None]).sum(2).min(1) / cell
        assert (d <= 1e-5).all() and (out["placed"] == 1).all()
    if name == "tent_out":
        assert out["placed"][out["cluster_of"][1]] == 2
    if name == "tent_in":
        assert out["placed"][out["cluster_of"][1]] == 1
    if name == "random_keys_4096_over_64":   # random triples over 64 clusters stand in for keys built to share one hash start
        assert out["counts"]["duplicates"] > 100 and len(out["tri"]) > 3000


def test_strip_past_the_first_round_of_the_tile_scan(mesh):
    """70 001 triangles that all survive: m' > 65 536 = 256 tiles of 256, so the scan of the tile totals carries into a second round"""
    m = ms.strip_far(70001)
    out = _check(mesh, m, 0.5, "strip")
    assert len(out["tri"]) == 70001 and np.array_equal(out["tri_src"], np.arange(70001)) and out["counts"] == {"non_finite": 0, "collapsed": 0, "duplicates": 0}


@pytest.mark.parametrize("reverse", (False, True))
def test_every_insert_on_one_slot(mesh, reverse):
    """70 001 triangles on one key in all six orientations: exactly index 0 survives, whether the smallest index arrives first or last"""
    m = ms.one_key(70001, reverse)
    out = _check(mesh, m, 1.0, "one key")
    assert out["tri_src"].tolist() == [0] and out["counts"]["duplicates"] == 70000 and len(out["xyz"]) == 4
    assert out["tri"].tolist() == [out["cluster_of"][m["tri"][0]].tolist()]


def test_fan_adds_70001_planes_to_one_cluster(mesh):
    m = ms.fan_hub(70001)
    out = _check(mesh, m, 0.5, "fan")
    assert out["count"][out["cluster_of"][0]] == 1 and ms.statement(m, 0.5, 1)["T"][out["cluster_of"][0]] == 70001


def test_power_of_two_and_triangle_order(mesh):
    for m, cell in ((ms.cube(8), 0.3), (mc.anchor(), 1.7)):
        with _handle(mesh, m) as h:
            base = h.simplify(cell, "quadric")
        for p in (-40, 40):
            sm, scell = ms.scaled(m, p), float(F(cell)) * 2.0 ** p
            got = _check(mesh, sm, scell, f"scaled {p}", ("quadric",))
            for k in ("tri", "placed", "cluster_of", "count", "tri_src"):
                assert np.array_equal(got[k], base[k]), (k, p)
            assert np.array_equal(got["xyz"].astype(D), base["xyz"].astype(D) * 2.0 ** p)
        perm = np.random.default_rng(3).permutation(len(m["tri"]))
        got = _check(mesh, mc._mesh(m["xyz"], m["tri"][perm], m["rgb"]), cell, "permuted", ("quadric",))
        for k in ("xyz", "placed", "count", "cluster_of"):
            assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint8), np.ascontiguousarray(base[k]).view(np.uint8)), k


def test_null_optional_outputs(mesh, engine):
    """out_cluster_of, out_count, out_placed, out_tri_src and counts NULL: the same vertices and triangles"""
    lib, fns = engine.load()
    lib.mpmvs_free.argtypes, lib.mpmvs_free.restype = [C.c_void_p], None
    m = _coloured(mc.anchor())
    want = ms.statement(m, 1.3, 1)
    with _handle(mesh, m) as h:
        px, pc, pt, mo = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_longlong(0)
        nc = fns["simplify_mesh"](h._h, 1.3, 1, C.byref(px), C.byref(pc), C.byref(pt), C.byref(mo), None, None, None, None, None)
        assert nc == len(want["xyz"]) and mo.value == len(want["tri"])
        xyz = np.ctypeslib.as_array(C.cast(px, C.POINTER(C.c_float)), (nc, 3)).copy()
        rgb = np.ctypeslib.as_array(C.cast(pc, C.POINTER(C.c_uint8)), (nc, 3)).copy()
        tri = np.ctypeslib.as_array(C.cast(pt, C.POINTER(C.c_int32)), (mo.value, 3)).copy()
        for p in (px, pc, pt):
            lib.mpmvs_free(p)
    assert np.array_equal(xyz.view(np.uint32), want["xyz"].view(np.uint32)) and np.array_equal(rgb, want["rgb"]) and np.array_equal(tri, want["tri"])


def test_two_calls_agree_and_the_handle_is_unchanged(mesh):
    m = _coloured(mc.two_spheres())
    with _handle(mesh, m) as h:
        before_cc, before_n = h.components(), h.normals()
        a, b = h.simplify(0.9, "quadric"), h.simplify(0.9, "quadric")
        ms.assert_same(b, a, "second call")
        t = h.simplify_ms()
        assert list(t) == list(mesh.SIMPLIFY_PASSES) and all(v > 0 for v in t.values()), t
        h.simplify(0.9, "mean")
        assert h.simplify_ms()["quadric_accumulate"] == 0.0
        after_cc, after_n = h.components(), h.normals()
        assert all(np.array_equal(x, y) for x, y in zip(after_cc[:3], before_cc[:3])) and after_cc[3] == before_cc[3]
        assert np.array_equal(after_n[0].view(np.uint32), before_n[0].view(np.uint32)) and after_n[1] == before_n[1]
        want = mc.want("two_spheres")
        assert np.array_equal(after_cc[0], want["label"]) and np.array_equal(after_n[0].view(np.uint32), want["normals"].view(np.uint32))


@pytest.mark.parametrize("k", range(ms.SWEEP_CASES))
def test_sweep(mesh, k):
    c = ms.sweep_case(k)
    with _handle(mesh, c["mesh"]) as h:
        for placement in PLACEMENTS:
            ms.assert_same(h.simplify(c["cell"], placement), ms.sweep_want(k, mesh.PLACEMENTS[placement]), f"sweep {k} {placement}")


def _composed(m, cell, placement, drop, normals):
    """mesh.simplify as the statements compose it"""
    w = ms.statement(m, cell, placement)
    out = dict(w, src=None, normals=None, normals_defined=None)
    if drop:
        sel = mc.select_statement({"xyz": w["xyz"], "tri": w["tri"], "rgb": w["rgb"]}, np.ones(len(w["xyz"]), np.uint8), True)
        out.update(xyz=sel["xyz"], rgb=sel["rgb"], tri=sel["tri"], src=sel["src"])
    if normals:
        out["normals"], out["normals_defined"] = mc.normals_statement(out["xyz"], out["tri"])
    return out


@pytest.mark.parametrize("drop,normals", [(True, True), (True, False), (False, True), (False, False)])
def test_simplify_composes_select_and_normals(mesh, drop, normals):
    loose = mc._mesh(np.array([[50, 50, 50], [51, 50, 50], [50.1, 50.1, 50]], F), [[0, 1, 2]])   # collapses into two clusters no triangle names
    for m, cell in ((mc.join(mc.anchor(), loose), 1.0), (mc.join(_coloured(mc.two_spheres()), _coloured(loose)), 1.4)):
        got = mesh.simplify(m, cell, "quadric", drop_unreferenced=drop, normals=normals)
        want = _composed(m, cell, 1, drop, normals)
        ms.assert_same(got, want, f"drop {drop} normals {normals}")
        for k in ("src", "normals"):
            assert (got[k] is None) == (want[k] is None) and (want[k] is None or np.array_equal(np.ascontiguousarray(got[k]).view(np.uint8), np.ascontiguousarray(want[k]).view(np.uint8))), k
        assert got["normals_defined"] == want["normals_defined"]
        if drop:
            assert len(got["xyz"]) == len(got["count"]) - 2 and "select_emit" in got["device_ms"]
        assert all(p in got["device_ms"] for p in mesh.SIMPLIFY_PASSES) and (("normals_finish" in got["device_ms"]) == normals)


# ---- the tools, as fresh child processes ---------------------------------------------------------------------------------------------
def _run(args):
    r = subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_simplify_mesh_tool(mesh, tmp_path):
    m = dict(mc.anchor(), rgb=np.random.default_rng(2).integers(0, 256, (410, 3)).astype(np.uint8))   # the TSDF sphere of the contract
    src, dst = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    mesh.write_ply_mesh(src, m["xyz"], m["tri"], m["rgb"])
    res = _run(["tools/simplify_mesh.py", "--input", src, "--output", dst, "--cell", "1.3", "--normals"])
    want = _composed(m, 1.3, 1, True, True)
    mesh.write_ply_mesh(str(tmp_path / "want.ply"), want["xyz"], want["tri"], want["rgb"], normals=want["normals"])
    assert open(dst, "rb").read() == open(str(tmp_path / "want.ply"), "rb").read()
    assert (res["n"], res["m"], res["n_out"], res["m_out"], res["clusters"]) == (410, 816, len(want["xyz"]), len(want["tri"]), len(want["count"]))
    assert res["m_out"] < res["m"] and res["n_out"] < res["n"]
    assert {k: res[k] for k in ("non_finite", "collapsed", "duplicates")} == want["counts"]
    assert res["placed"] == [int((want["placed"] == p).sum()) for p in range(3)] and res["normals_defined"] == want["normals_defined"]
    assert all(p in res["device_ms"] for p in mesh.SIMPLIFY_PASSES) and "wall" in res["seconds"] and res["placement"] == "quadric"
    res = _run(["tools/simplify_mesh.py", "--input", src, "--output", dst, "--cell", "1.3", "--placement", "mean", "--keep_unreferenced"])
    want = _composed(m, 1.3, 0, False, False)
    back = mesh.read_ply_mesh(dst)
    assert np.array_equal(back["xyz"].view(np.uint32), want["xyz"].view(np.uint32)) and np.array_equal(back["tri"], want["tri"]) and np.array_equal(back["rgb"], want["rgb"])
    assert back["normals"] is None and res["placed"] == [len(want["count"]), 0, 0] and res["n_out"] == res["clusters"]


def test_mesh_ply_tool_simplifies_after_the_cleaning(mesh, pm, hostlib, tmp_path):
    """the four-camera sphere as a dense folder: --simplify after --min_component and before --normals is the composed statement on the
    file the tool writes without it; off by default"""
    dims, origin, voxel, trunc, cams, depths, _ = sc.sphere_scene(pm)
    images = [np.full(d.shape + (3,), 30 + 50 * q, np.uint8) for q, d in enumerate(depths)]
    folder = str(tmp_path / "scene")
    hostlib.write_dataset(folder, cams, images, [[i] for i in range(4)], fmt="ppm")
    for i, d in enumerate(depths):
        os.makedirs(os.path.join(folder, "MPMVS", f"2333_{i:08d}"))
        hostlib.write_dmb(os.path.join(folder, "MPMVS", f"2333_{i:08d}", "depths.dmb"), d)
    hi = [origin[a] + (dims[a] - 1) * voxel for a in range(3)]
    common = ["--dense_folder", folder, "--voxel", str(voxel), "--trunc", str(trunc), "--min_weight", "1", "--bbox"] + [str(v) for v in list(origin) + hi]
    plain = _run(["tools/mesh_ply.py", "--output", str(tmp_path / "plain.ply"), "--min_component", "20"] + common)
    assert "simplified" not in plain
    m = mesh.read_ply_mesh(str(tmp_path / "plain.ply"))
    cell = 3.0 * voxel
    res = _run(["tools/mesh_ply.py", "--output", str(tmp_path / "simple.ply"), "--min_component", "20", "--simplify", str(cell), "--normals"] + common)
    want = _composed(m, cell, 1, True, True)
    mesh.write_ply_mesh(str(tmp_path / "want.ply"), want["xyz"], want["tri"], want["rgb"], normals=want["normals"])
    assert open(str(tmp_path / "simple.ply"), "rb").read() == open(str(tmp_path / "want.ply"), "rb").read()
    s = res["simplified"]
    assert s["triangles_in"] == len(m["tri"]) and s["vertices_in"] == len(m["xyz"]) and s["clusters"] == len(want["count"])
    assert res["triangles"] == len(want["tri"]) < len(m["tri"]) and res["vertices"] == len(want["xyz"]) and res["normals_defined"] == want["normals_defined"]
    assert {k: s[k] for k in ("non_finite", "collapsed", "duplicates")} == want["counts"]
    assert all(k in res["device_ms"] for k in ("simplify_cluster", "simplify_place", "simplify_emit", "cc_hook", "normals_finish", "integrate"))
