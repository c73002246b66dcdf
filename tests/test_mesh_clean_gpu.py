"""mpmvs_mesh_* on the GPU against the numpy statements of mesh_clean_common.py: components, area-weighted vertex normals and
select, bit for bit; remove_small_components and vertex_normals; the seeded sweep; tools/mesh_ply.py and tools/clean_mesh.py as
fresh child processes."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_clean_common as mc
import tsdf_sparse_common as sc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAMES = ("anchor", "two_spheres", "open_sphere", "strip4096_ascending", "strip4096_descending", "strip4096_scrambled", "fan8193", "fan8193_hub_last",
         "tetrahedra", "repeated", "strip255", "strip256", "strip257")


@pytest.fixture(scope="module")
def mesh(pm):
    return importlib.import_module("mp-mvs_amd.mesh")


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _handle(mesh, m):
    return mesh.Mesh(m["xyz"], m["tri"], m["rgb"])


def _components_equal(got, want):
    label, verts, tris, counts = got
    assert label.dtype == np.int32 and np.array_equal(label, want["label"])
    assert np.array_equal(verts, want["verts"]) and np.array_equal(tris, want["tris"])
    assert [counts[k] for k in ("components", "unnamed", "largest_triangles", "largest_label")] == want["counts"]


@pytest.mark.parametrize("name", NAMES)
def test_components_and_normals_equal_the_statements(mesh, name):
    m, want = mc.named_meshes()[name], mc.want(name)
    with _handle(mesh, m) as h:
        first = h.components()
        _components_equal(first, want)
        nrm, nd = h.normals()
        assert nd == want["n_defined"] and np.array_equal(bits(nrm), bits(want["normals"]))
        # NULL out_verts / out_tris: the same labels and counts
        label, verts, tris, counts = h.components(want_verts=False, want_tris=False)
        assert verts is None and tris is None and np.array_equal(label, want["label"]) and counts == first[3]
        # two calls give identical bytes
        again, nrm2 = h.components(), h.normals()
        assert all(np.array_equal(a, b) for a, b in zip(again[:3], first[:3])) and np.array_equal(bits(nrm2[0]), bits(nrm)) and nrm2[1] == nd
        ms = h.pass_ms()
        assert all(ms[k] > 0 for k in ("cc_hook", "cc_flatten", "cc_sizes", "normals_accumulate", "normals_finish")) and ms["select_emit"] == 0.0


def test_components_without_counts(mesh, pm):
    import ctypes as C
    eng = importlib.import_module("mp-mvs_amd.engine")
    _, fns = eng.load()
    m, want = mc.named_meshes()["tetrahedra"], mc.want("tetrahedra")
    with _handle(mesh, m) as h:
        label = np.empty(len(m["xyz"]), np.int32)
        assert fns["mesh_components"](h._h, label.ctypes.data, None, None, None) == 0 and np.array_equal(label, want["label"])
        counts = (C.c_longlong * 4)()
        assert fns["mesh_components"](h._h, label.ctypes.data, None, None, counts) == 0 and list(counts) == want["counts"]
        nrm = np.empty((len(m["xyz"]), 3), F)
        assert fns["mesh_normals"](h._h, nrm.ctypes.data, None) == 0 and np.array_equal(bits(nrm), bits(want["normals"]))


def test_normals_of_non_finite_and_cancelling_meshes(mesh):
    for base in ("anchor", "tetrahedra", "fan8193_hub_last", "fan8193"):
        m = mc.plant_nonfinite(mc.named_meshes()[base])   # vertex 0 is one of the planted
        want, nd = mc.normals_statement(m["xyz"], m["tri"])
        assert (nd == 0) if base == "fan8193" else (0 < nd < len(m["xyz"]))   # a fan around a non-finite hub has no finite triangle
        with _handle(mesh, m) as h:
            got, gd = h.normals()
            _components_equal(h.components(), mc.want(base))   # the components do not look at positions
        assert gd == nd and np.array_equal(bits(got), bits(want))
    xyz = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.25, 0.5, 3]], F)
    with mesh.Mesh(xyz, [[0, 1, 2], [0, 2, 1], [0, 1, 3], [1, 0, 3]]) as h:   # two cancelling pairs
        got, gd = h.normals()
    assert gd == 0 and not bits(got).any()


def test_normals_do_not_see_a_power_of_two(mesh):
    a, want = mc.anchor(), mc.want("anchor")
    for p in (-40, 40):
        with mesh.Mesh((a["xyz"].astype(np.float64) * 2.0 ** p).astype(F), a["tri"]) as h:
            got, nd = h.normals()
        assert nd == 410 and np.array_equal(bits(got), bits(want["normals"])), p


def positive_side(m, normals, vol, origin, voxel, step=1.0):
    """per vertex with a defined normal: the value f = sum / weight of the lattice point nearest to p + step * voxel * n, NaN where
    that point lies outside the volume or was never observed"""
    total, weight = vol["sum"], vol["weight"]
    with np.errstate(all="ignore"):
        f = np.where(weight > 0, total / np.maximum(weight, 1), np.nan)
    q = m["xyz"].astype(np.float64) + step * voxel * normals.astype(np.float64)
    idx = np.rint((q - np.array(origin, np.float64)) / voxel).astype(np.int64)
    inside = ((idx >= 0) & (idx < np.array(f.shape[::-1]))).all(1) & normals.any(1)
    out = np.full(len(q), np.nan)
    out[inside] = f[idx[inside, 2], idx[inside, 1], idx[inside, 0]]
    return out


def test_normals_of_a_volume_mesh_face_the_cameras(mesh, pm):
    """the sphere seen by four cameras into 24^3, end to end from Volume.mesh(): every defined normal points to the positive side of
    the volume, which is the side the cameras looked from.  The side is read off the volume itself: one voxel along the normal the
    nearest lattice point, where it was observed at all, has f > 0, and one voxel against it f is smaller.  (One voxel: the nearest
    lattice point is up to sqrt(3) / 2 = 0.87 voxels from the sample, so a shorter step could land on a lattice point across the
    surface; the truncation band is 3 voxels wide, so the step stays inside it.)  Scalar products with the directions to the camera
    centres or from the sphere's centre do not state this: on the statement's own mesh they are negative at 20 and 2 of the 1627
    vertices, all on the limb where the views end and the surface is seen edge-on."""
    dims, origin, voxel, trunc, cams, depths, cols = sc.sphere_scene(pm)
    with mesh.Volume(origin, voxel, dims, trunc, color=True) as v:
        v.integrate(cams, depths, cols)
        vol = v.get()
        m = v.mesh(1)
    assert len(m["tri"]) > 500
    want, nd = mc.normals_statement(m["xyz"], m["tri"])
    got, gd = mesh.vertex_normals(m)
    assert gd == nd == len(m["xyz"]) and np.array_equal(bits(got), bits(want))
    ahead, behind = positive_side(m, got, vol, origin, voxel, 1.0), positive_side(m, got, vol, origin, voxel, -1.0)
    seen = ~np.isnan(ahead)
    print("normals on the positive side:", int(seen.sum()), "of", len(seen), "vertices have an observed lattice point ahead,", int((seen & ~np.isnan(behind)).sum()), "on both sides")
    assert seen.sum() > len(seen) // 2           # the check is not empty
    assert (ahead[seen] > 0).all()
    both = seen & ~np.isnan(behind)
    assert (ahead[both] > behind[both]).all()


def _masks(m, want):
    n = len(m["xyz"])
    rng = np.random.default_rng(n)
    largest = want["counts"][3]
    return {"all": np.ones(n, np.uint8), "none": np.zeros(n, np.uint8), "random": (rng.random(n) < 0.7).astype(np.uint8) * 200,
            "all_but_largest": (want["label"] != largest).astype(np.uint8)}


@pytest.mark.parametrize("name", ("tetrahedra", "repeated", "two_spheres", "strip257"))
def test_select_equals_the_statement(mesh, name):
    m, want = mc.named_meshes()[name], mc.want(name)
    rgb = m["rgb"] if m["rgb"] is not None else (np.arange(3 * len(m["xyz"])) % 251).astype(np.uint8).reshape(-1, 3)
    for color in (True, False):
        mm = dict(m, rgb=rgb if color else None)
        with _handle(mesh, mm) as h:
            before = h.components()
            for mask_name, keep in _masks(mm, want).items():
                for drop in (False, True):
                    got, exp = h.select(keep, drop), mc.select_statement(mm, keep, drop)
                    assert mc.same_mesh(got, exp), (mask_name, drop, color)
                    assert np.array_equal(bits(got["xyz"]), bits(mm["xyz"][got["src"]]))   # src is consistent with xyz
            after = h.components()   # the handle is unchanged
            assert all(np.array_equal(a, b) for a, b in zip(after[:3], before[:3])) and after[3] == before[3]
            ms = h.pass_ms()
            assert ms["select_flag"] > 0 and ms["select_scan"] > 0


def test_select_across_the_second_round_of_the_tile_scan(mesh):
    """n = m = 70 001: 274 tiles of 256, so the scan of the tile totals carries into a second round; content in the first and last
    entries only, and every other vertex"""
    n = 70001
    xyz = (np.arange(3 * n, dtype=np.int64) % 8191).astype(F).reshape(n, 3)
    tri = np.stack([np.arange(n), (np.arange(n) + 1) % n, (np.arange(n) + 2) % n], 1).astype(np.int32)
    m = mc._mesh(xyz, tri)
    ends = np.zeros(n, np.uint8)
    ends[[0, 1, 2, n - 2, n - 1]] = 1   # triangles 0, n - 2 (n-2, n-1, 0) and n - 1 (n-1, 0, 1) survive
    with _handle(mesh, m) as h:
        for keep in (ends, (np.arange(n) % 2 == 0).astype(np.uint8), np.ones(n, np.uint8)):
            for drop in (False, True):
                assert mc.same_mesh(h.select(keep, drop), mc.select_statement(m, keep, drop)), drop
        got = h.select(ends, True)
    assert got["src"].tolist() == [0, 1, 2, n - 2, n - 1] and got["tri"].tolist() == [[0, 1, 2], [3, 4, 0], [4, 0, 1]]


@pytest.mark.parametrize("min_triangles,largest", [(1, None), (5, None), (10 ** 6, None), (1, 1), (2, 3), (1, 10 ** 4)])
def test_remove_small_components(mesh, min_triangles, largest):
    m = _joined()
    got = mesh.remove_small_components(m, min_triangles, largest)
    want = mc.clean_statement(m, min_triangles, largest)
    assert mc.same_mesh(got, want) and np.array_equal(got["keep"], want["keep"]) and np.array_equal(got["label"], want["label"])
    assert np.array_equal(got["tris"], want["tris"]) and [got["counts"][k] for k in ("components", "unnamed", "largest_triangles", "largest_label")] == want["counts"]
    nrm, nd = mesh.vertex_normals(got)
    wn, wd = mc.normals_statement(want["xyz"], want["tri"])
    assert nd == wd and np.array_equal(bits(nrm), bits(wn))


def _joined():
    t = mc.named_meshes()["tetrahedra"]
    return mc.join(mc._mesh(t["xyz"], t["tri"]), mc.anchor(), mc.repeated(), mc.two_spheres())


@pytest.mark.parametrize("k", range(mc.SWEEP_CASES))
def test_sweep(mesh, k):
    c, want = mc.sweep_case(k), mc.sweep_want(k)
    m = c["mesh"]
    with _handle(mesh, m) as h:
        _components_equal(h.components(), want)
        nrm, nd = h.normals()
        assert nd == want["n_defined"] and np.array_equal(bits(nrm), bits(want["normals"]))
        for drop in (False, True):
            assert mc.same_mesh(h.select(c["keep"], drop), want["select"][int(drop)]), drop


# ---- the tools, as fresh child processes ---------------------------------------------------------------------------------------------
def _run(args):
    r = subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_mesh_ply_tool_cleans_and_shades(mesh, pm, hostlib, tmp_path):
    """the four-camera sphere plus a small ball off to the side, as a dense folder: without the new flags the file of Volume.mesh and
    write_ply_mesh; with --min_component 20 --normals the statement's file"""
    dims, origin, voxel, trunc, cams, depths, _ = sc.sphere_scene(pm)
    from test_tsdf_gpu import _sphere_depth
    speck = np.array([0.42, 0.42, 1.62])
    depths = [np.where(_sphere_depth(c, speck, 0.06, 0.0) > 0, _sphere_depth(c, speck, 0.06, 0.0), d).astype(F) for c, d in zip(cams, depths)]
    images = [np.full(d.shape + (3,), 30 + 50 * q, np.uint8) for q, d in enumerate(depths)]   # grey: no question of channel order
    folder = str(tmp_path / "scene")
    hostlib.write_dataset(folder, cams, images, [[i] for i in range(4)], fmt="ppm")
    for i, d in enumerate(depths):
        os.makedirs(os.path.join(folder, "MPMVS", f"2333_{i:08d}"))
        hostlib.write_dmb(os.path.join(folder, "MPMVS", f"2333_{i:08d}", "depths.dmb"), d)
    hi = [origin[a] + (dims[a] - 1) * voxel for a in range(3)]
    common = ["--dense_folder", folder, "--voxel", str(voxel), "--trunc", str(trunc), "--min_weight", "1", "--bbox"] + [str(v) for v in list(origin) + hi]
    plain = _run(["tools/mesh_ply.py", "--output", str(tmp_path / "plain.ply")] + common)
    m = mesh.read_ply_mesh(str(tmp_path / "plain.ply"))
    assert m["normals"] is None and plain["triangles"] == len(m["tri"]) > 500 and "components" not in plain
    # the same views through the library in this process
    cams2 = [hostlib.read_camera(os.path.join(folder, "cams", f"{i:08d}_cam.txt")) for i in range(4)]
    for c in cams2:
        c.height, c.width = depths[0].shape
    with mesh.Volume(np.array(plain["origin"], F), voxel, plain["dims"], trunc, color=True) as v:
        v.integrate(cams2, depths, images)
        direct = v.mesh(1)
    mesh.write_ply_mesh(str(tmp_path / "direct.ply"), direct["xyz"], direct["tri"], direct["rgb"])
    assert open(str(tmp_path / "plain.ply"), "rb").read() == open(str(tmp_path / "direct.ply"), "rb").read()
    want = mc.clean_statement(m, 20)
    assert 0 < len(want["tri"]) < len(m["tri"]) and want["counts"][0] >= 2   # the scene has something to remove
    res = _run(["tools/mesh_ply.py", "--output", str(tmp_path / "clean.ply"), "--min_component", "20", "--normals"] + common)
    wn, wd = mc.normals_statement(want["xyz"], want["tri"])
    mesh.write_ply_mesh(str(tmp_path / "want.ply"), want["xyz"], want["tri"], want["rgb"], normals=wn)
    assert open(str(tmp_path / "clean.ply"), "rb").read() == open(str(tmp_path / "want.ply"), "rb").read()
    assert res["components"] == want["counts"][0] and res["largest_component"] == want["counts"][2] and res["normals_defined"] == wd
    assert res["removed_triangles"] == len(m["tri"]) - len(want["tri"]) and res["triangles"] == len(want["tri"]) and res["vertices"] == len(want["xyz"])
    assert all(k in res["device_ms"] for k in ("cc_hook", "normals_accumulate", "select_emit", "integrate", "mark"))


def test_clean_mesh_tool_keeps_the_largest(mesh, tmp_path):
    m = mc.join(mc.named_meshes()["tetrahedra"], dict(mc.anchor(), rgb=np.full((410, 3), 9, np.uint8)))
    src, dst = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    mesh.write_ply_mesh(src, m["xyz"], m["tri"], m["rgb"])
    res = _run(["tools/clean_mesh.py", "--input", src, "--output", dst, "--largest", "1", "--normals"])
    want = mc.clean_statement(m, 1, 1)
    wn, wd = mc.normals_statement(want["xyz"], want["tri"])
    assert len(want["tri"]) == 816
    mesh.write_ply_mesh(str(tmp_path / "want.ply"), want["xyz"], want["tri"], want["rgb"], normals=wn)
    assert open(dst, "rb").read() == open(str(tmp_path / "want.ply"), "rb").read()
    assert res["components"] == 301 and res["largest_component"] == 816 and res["removed_triangles"] == 1200 and res["normals_defined"] == wd == 410
