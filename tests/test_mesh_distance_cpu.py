"""mpmvs_surface_distance and mpmvs_surface_sample without a GPU: the symbols, the refusals that need no cloud handle (a cloud handle
opens its stream at create, so the refusals of a live pair are in test_mesh_distance_gpu.py) and what is answered on the host, the two
numpy statements of mesh_distance_common.py on cases worked out by hand, the distance statement against an independent formulation in
extended precision, the sweep's census, compare and evaluate_mesh on the statements through stubs for the device calls, the tool up
to the device call, and the host check program under the sanitizers."""
import ctypes as C
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import mesh_clean_common as mc
import mesh_distance_common as md
import mesh_simplify_common as msc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mpmvs_surface_distance", "mpmvs_surface_distance_ms", "mpmvs_surface_sample", "mpmvs_surface_sample_ms")
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
    PP = C.POINTER(_P)
    f = fns["surface_distance"]
    assert f.restype is C.c_int and f.argtypes == [_P, _P, C.c_float, _P, _P, C.POINTER(C.c_longlong)]
    f = fns["surface_sample"]
    assert f.restype is C.c_longlong and f.argtypes == [_P, C.c_float, PP, PP, PP, PP]
    for name in ("surface_distance_ms", "surface_sample_ms"):
        assert fns[name].restype is C.c_float and fns[name].argtypes == [_P, C.POINTER(C.c_float)]
    # the mesh section's own prefix keeps its six names, and the kernels live in a header of their own with host-and-device bodies
    assert len(set(re.findall(r"\b(mpmvs_mesh_[a-z0-9_]+)\s*\(", header))) == 6
    text = open(os.path.join(ROOT, "mp-mvs_amd", "csrc", "pm_surface.hpp")).read()
    assert len(re.findall(r"^inline __global__", text, re.M)) == 6 and not re.findall(r"^__global__", text, re.M)
    assert "void k_scan_" not in text   # the scan has no second copy


def _handle(fns, m):
    xyz, tri, rgb = m["xyz"], m["tri"], m["rgb"]
    h = _P()
    rc = fns["mesh_create"](0, len(xyz), xyz.ctypes.data if len(xyz) else None, None if rgb is None else rgb.ctypes.data, len(tri), tri.ctypes.data if len(tri) else None,
                            C.byref(h))
    assert rc == 0
    return h


def test_distance_refuses_null_handles_before_the_device(eng):
    _, fns = eng.load()
    err = lambda: fns["last_error"](None).decode()   # noqa: E731
    d2, tri, counts = np.full(4, 7, F), np.full(4, 7, np.int32), (C.c_longlong * 2)(7, 7)
    untouched = lambda: bool((d2 == 7).all() and (tri == 7).all()) and list(counts) == [7, 7]   # noqa: E731
    assert fns["surface_distance"](None, None, 1.0, d2.ctypes.data, tri.ctypes.data, counts) == -2 and "surface distance" in err() and untouched()
    h = _handle(fns, md.hand_mesh())
    assert fns["surface_distance"](h, None, 1.0, d2.ctypes.data, tri.ctypes.data, counts) == -2 and "handle" in err() and untouched()
    ms3 = (C.c_float * 3)(7, 7, 7)
    assert fns["surface_distance_ms"](None, ms3) == 0.0 and list(ms3) == [7, 7, 7]
    assert fns["surface_distance_ms"](h, ms3) == 0.0 and list(ms3) == [0, 0, 0]   # nothing has run
    assert fns["surface_distance_ms"](h, None) == 0.0
    fns["mesh_destroy"](h)


def test_sample_refusals_write_nothing_and_need_no_device(eng):
    _, fns = eng.load()
    err = lambda: fns["last_error"](None).decode()   # noqa: E731
    for color in (False, True):
        m = mc.tetrahedra(2, 0, color=color)
        h = _handle(fns, m)
        px, po, pc, pn = _P(0x11), _P(0x22), _P(0x33), _P(0x44)
        untouched = lambda: (px.value, po.value, pc.value, pn.value) == (0x11, 0x22, 0x33, 0x44)   # noqa: E731
        rgb = C.byref(pc) if color else None
        assert fns["surface_sample"](None, 1.0, C.byref(px), C.byref(po), rgb, C.byref(pn)) == -2 and "surface sample" in err() and untouched()
        for spacing in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
            assert fns["surface_sample"](h, spacing, C.byref(px), C.byref(po), rgb, C.byref(pn)) == -2 and "spacing" in err() and untouched(), spacing
        assert fns["surface_sample"](h, 1.0, None, C.byref(po), rgb, C.byref(pn)) == -2 and untouched()
        assert fns["surface_sample"](h, 1.0, C.byref(px), None, rgb, C.byref(pn)) == -2 and untouched()
        wrong = None if color else C.byref(pc)
        assert fns["surface_sample"](h, 1.0, C.byref(px), C.byref(po), wrong, C.byref(pn)) == -2 and "colour" in err() and untouched()
        ms3 = (C.c_float * 3)(7, 7, 7)
        assert fns["surface_sample_ms"](h, ms3) == 0.0 and list(ms3) == [0, 0, 0]
        fns["mesh_destroy"](h)


def test_sample_with_nothing_to_do_is_answered_on_the_host(mesh):
    nan_mesh = mc._mesh(np.array([[0, 0, 0], [1, np.nan, 0], [0, 1, 0], [np.inf, 0, 0]], F), [[0, 1, 2], [1, 2, 3]])
    empty = mc._mesh(np.zeros((0, 3), F), np.zeros((0, 3), np.int32))
    no_tri = mc._mesh(np.array([[0, 0, 0], [1, 0, 0]], F), np.zeros((0, 3), np.int32))
    for m in (nan_mesh, empty, no_tri):
        for rgb in (None, np.zeros((len(m["xyz"]), 3), np.uint8)):
            with mesh.Mesh(m["xyz"], m["tri"], rgb) as h:
                out = h.sample(0.5, want_normals=True)   # no device on this machine: a launch would raise
                assert out["xyz"].shape == (0, 3) and out["tri_of"].shape == (0,) and out["normals"].shape == (0, 3)
                assert (out["rgb"] is None) == (rgb is None)
                assert h.sample_ms() == {"total": 0.0, "count": 0.0, "scan": 0.0, "emit": 0.0}
            want = md.sample_statement(m["xyz"], m["tri"], 0.5, rgb, True)
            assert len(want["xyz"]) == 0


# ---- the distance statement by hand -------------------------------------------------------------------------------------------------------
def test_seven_regions_in_closed_form():
    A, B, Cc = md.HAND_TRI
    d, region, _ = md.pair_d2(A, B, Cc, md.HAND_POINTS)
    assert region.tolist() == [1, 2, 3, 4, 5, 6, 7]
    assert md.same_bits(d, md.HAND_D2)   # 6, 2, 25, 2, 4, 4, 4: all exact in these numbers
    d2, arg, counts = md.distance_statement(md.HAND_TRI, [[0, 1, 2]], md.HAND_POINTS, 3.0)
    assert d2.tolist() == [6, 2, np.inf, 2, 4, 4, 4] and arg.tolist() == [0, 0, -1, 0, 0, 0, 0] and counts.tolist() == [6, 7]   # 25 > 9


def test_on_the_surface_and_at_the_radius():
    on = np.array([[3, 4, 0], [0, 0, 0], [0, 4, 0], [1.5, 2, 0], [1.5, 4, 0], [0, 2, 0], [1, 3, 0]], F)   # corners, edge midpoints, the face
    d2, arg, counts = md.distance_statement(md.HAND_TRI, [[0, 1, 2]], on, 1e-3)
    assert (d2 == 0).all() and (arg == 0).all() and counts.tolist() == [7, 7]
    just = np.array([[1, 3, 2], [1, 3, np.nextafter(F(2), F(3))], [1, 3, -2], [1, 3, np.nextafter(F(-2), F(-3))]], F)
    d2, arg, _ = md.distance_statement(md.HAND_TRI, [[0, 1, 2]], just, 2.0)   # D == r2 is a candidate, one float beyond is none
    assert d2.tolist() == [4, np.inf, 4, np.inf] and arg.tolist() == [0, -1, 0, -1]


def test_ties_go_to_the_smallest_index_and_order_never_shows():
    tri = np.array([[2, 1, 0], [0, 1, 2], [0, 1, 2], [1, 2, 0]], np.int32)   # reversed, twice the same, rotated
    pts = np.concatenate([md.HAND_POINTS, [[np.nan, 0, 0]]]).astype(F)
    base = md.distance_statement(md.HAND_TRI, [[0, 1, 2]], pts, 10.0)
    d2, arg, counts = md.distance_statement(md.HAND_TRI, tri[1:3], pts, 10.0)
    assert md.same_bits(d2, base[0]) and arg.tolist() == [0] * 7 + [-1] and counts.tolist() == [7, 7]
    # a reversed or rotated copy may round differently, but where it attains the same D the smaller index is reported
    d2, arg, _ = md.distance_statement(md.HAND_TRI, tri, pts, 10.0)
    for i in range(7):
        each = [md.distance_statement(md.HAND_TRI, tri[t:t + 1], pts[i:i + 1], 10.0)[0][0] for t in range(4)]
        assert d2[i] == min(each) and arg[i] == each.index(min(each))
    perm = np.random.default_rng(1).permutation(len(pts))
    dp, ap, _ = md.distance_statement(md.HAND_TRI, tri, pts[perm], 10.0)
    assert md.same_bits(dp, d2[perm]) and np.array_equal(ap, arg[perm])


def test_degenerate_triangles_follow_the_sequence_literally():
    """a == b == c: ab = ac = 0, every s is 0, rule 1 applies: X = A, the distance to the point.  a == b != c: ab = 0, so s1 = s3 = s5 = 0
    and vc = vb = va = 0 exactly; rule 1 where s2 <= 0 (X = A), rule 2 where s4 <= 0 cannot come after it (s4 = s2 - |ac|^2 < s2), so
    elsewhere rule 3 divides 0 by 0: the pair yields a NaN and is no candidate.  No NaN reaches an output."""
    xyz = np.array([[0, 0, 0], [0, 0, 0], [2, 0, 0]], F)
    pts = np.array([[-1, 1, 0], [0, 3, 0], [1, 1, 0], [3, 0, 0]], F)
    d2, arg, counts = md.distance_statement(xyz, [[0, 0, 0]], pts, 10.0)
    assert d2.tolist() == [2, 9, 2, 9] and (arg == 0).all()
    d2, arg, counts = md.distance_statement(xyz, [[0, 1, 2]], pts, 10.0)
    assert d2.tolist() == [2, 9, np.inf, np.inf] and arg.tolist() == [0, 0, -1, -1] and counts.tolist() == [2, 4]
    d, region, _ = md.pair_d2(xyz[0], xyz[1], xyz[2], pts)
    assert region.tolist() == [1, 1, 3, 3] and np.isnan(d[2:]).all()
    assert not np.isnan(d2).any()


@pytest.mark.parametrize("p", (-40, 40))
def test_scaling_by_a_power_of_two(p):
    m, pts, radius = md.sweep_case(4)
    s = F(2.0) ** p
    d2, arg, counts = md.sweep_want(4)[:3]
    ds, as_, cs = md.distance_statement(m["xyz"] * s, m["tri"], pts * s, float(F(radius) * s))
    assert np.array_equal(as_, arg) and np.array_equal(cs, counts) and counts[0] > 0
    assert md.same_bits(ds, d2 * s * s)   # exact: every operation scales, no underflow or overflow at these sizes


def test_statement_against_an_independent_formulation():
    """the rule cascade in fp64 against plane projection / clamped segments in extended precision, over the sweep's pairs whose triangle
    has a smallest angle of at least 1 degree and whose point is off the surface (squared distance above 1e-20 of the squared size of
    the scene: on the surface both sides give rounding noise of their own).  The deviation is relative to the squared distance, so it
    grows as a point nears the surface: about 2^-53 * size / distance.  The largest measured on the build machine is 1.648e-13
    (DESIGN.md section 26.5); the bound asserted is 16 times that."""
    MEASURED = 1.648e-13
    worst, pairs, good = 0.0, 0, 0
    for k in range(md.SWEEP_CASES):
        m, pts, _ = md.sweep_case(k)
        P = m["xyz"][m["tri"]].astype(D)
        P = P[np.isfinite(P).all((1, 2))]
        q = pts[np.isfinite(pts).all(1)].astype(D)
        ok = md.smallest_angle_deg(P[:, 0], P[:, 1], P[:, 2]) >= 1.0
        pairs += len(P) * len(q)
        good += int(ok.sum()) * len(q)
        P = P[ok]
        _, _, X = md.pair_d2(P[:, None, 0], P[:, None, 1], P[:, None, 2], q[None])
        e = q[None] - X
        dd = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
        ref = md.independent_d2(P[:, None, 0], P[:, None, 1], P[:, None, 2], q[None])
        scale = np.maximum(ref, np.longdouble(1e-30) * (np.abs(q).max() ** 2))
        far = ref > np.longdouble(1e-20) * (np.abs(q).max() ** 2)   # on the surface both give rounding noise of their own
        worst = max(worst, float((np.abs(dd.astype(np.longdouble) - ref) / scale)[far].max()))
    print(f"largest relative deviation {worst:.3e} over {good} of {pairs} pairs")
    assert good >= 0.8 * pairs
    assert worst <= 16 * MEASURED


def test_sweep_census():
    c = md.sweep_census()
    print(c)
    assert c["regions"][0] == 0 and (c["regions"][1:] >= 100).all()   # every one of the seven regions among the candidates
    assert c["ties"] >= 20 and c["nan_pairs"] >= 100 and c["no_candidate"] >= 500 and c["with_candidate"] >= 500
    assert c["nonfinite_points"] >= 3 and c["nonfinite_triangles"] >= 3
    assert c["pairs"] >= 100000


# ---- the sample statement ---------------------------------------------------------------------------------------------------------------
def _literal_lattice(A, B, Cc, s):
    """the sub-triangles of the regular s-subdivision with their three corners averaged, row by row from A's side ... in barycentric
    thirds: corner (i, j) = (i * A + j * B + (s - i - j) * C) / s"""
    corner = lambda i, j: (i * A + j * B + (s - i - j) * Cc) / s   # noqa: E731
    out = []
    for i in range(s):
        for ell in range(2 * (s - i) - 1):
            j = ell // 2
            three = [corner(i, j), corner(i + 1, j), corner(i, j + 1)] if ell % 2 == 0 else [corner(i + 1, j), corner(i, j + 1), corner(i + 1, j + 1)]
            out.append(sum(three) / 3)
    return np.array(out)


@pytest.mark.parametrize("s", (1, 2, 3, 7))
def test_samples_are_the_centroids_of_the_subdivision(s):
    A, B, Cc = md.HAND_TRI.astype(D)
    spacing = F(5.0 / s)   # the longest edge is 5
    assert md.subdivisions(md.HAND_TRI, [[0, 1, 2]], spacing)[0][0] in (s, s + 1)
    spacing = F(np.nextafter(F(5.0 / s), F(9))) if md.subdivisions(md.HAND_TRI, [[0, 1, 2]], spacing)[0][0] != s else spacing
    out = md.sample_statement(md.HAND_TRI, [[0, 1, 2]], spacing)
    assert len(out["xyz"]) == s * s and (out["tri_of"] == 0).all()
    want = _literal_lattice(A, B, Cc, s)
    assert np.allclose(out["xyz"], want, rtol=0, atol=1e-6)   # in order
    assert len({tuple(np.round(p, 5)) for p in out["xyz"]}) == s * s   # and as a set: no sample twice
    na, nb, nc = md.lattice_numbers(s)
    assert (nc >= 1).all() and (na >= 1).all() and (nb >= 1).all() and ((na + nb + nc) == 3 * s).all()


def test_counts_nc_and_both_sides_of_an_integer_ratio():
    for s in range(1, 40):
        na, nb, nc = md.lattice_numbers(s)
        assert len(na) == s * s and nc.min() >= 1 and len(set(zip(na.tolist(), nb.tolist()))) == s * s
    below, above = np.nextafter(F(2.5), F(0)), np.nextafter(F(2.5), F(9))
    s_of = lambda h: int(md.subdivisions(md.HAND_TRI, [[0, 1, 2]], h)[0][0])   # noqa: E731
    assert (s_of(F(2.5)), s_of(below), s_of(above)) == (2, 3, 2)   # ratio == 2 exactly, just above it, just below it
    assert s_of(F(5.0)) == 1 and s_of(F(1e9)) == 1


def test_zero_size_triangle_colour_rounding_normals_and_the_limit():
    xyz = np.array([[0.3, -7.25, 1e-3], [3, 4, 0], [0, 0, 0], [0, 4, 0]], F)
    out = md.sample_statement(xyz, [[0, 0, 0]], 0.01, want_normals=True)
    assert md.same_bits(out["xyz"], xyz[:1]) and (out["normals"] == 0).all()   # its one vertex position, exactly; no normal
    # colours by hand: s = 1, the one sample is the centroid: (2 * (a + b + c) + 3) // 6
    rgb = np.array([[0, 0, 0], [255, 0, 1], [255, 1, 1], [255, 1, 2]], np.uint8)
    out = md.sample_statement(xyz, [[1, 2, 3]], 5.0, rgb, True)
    assert out["rgb"].tolist() == [[255, 1, 1]]   # (2*765+3)//6 = 255, (2*2+3)//6 = 1, (2*4+3)//6 = 1
    assert out["normals"].tolist() == [[0, 0, -1]] or out["normals"].tolist() == [[-0.0, 0.0, -1.0]]
    # s = 2 at the corner sample nearest A: weights (4, 1, 1) of 6: (2 * (4 a + b + c) + 6) // 12
    out = md.sample_statement(xyz, [[1, 2, 3]], 2.5, np.array([[0, 0, 0], [10, 200, 7], [20, 100, 8], [30, 50, 9]], np.uint8))
    na, nb, nc = md.lattice_numbers(2)
    k = int(np.flatnonzero((na == 4))[0])
    assert out["rgb"][k].tolist() == [(2 * (40 + 20 + 30) + 6) // 12, (2 * (800 + 100 + 50) + 6) // 12, (2 * (28 + 8 + 9) + 6) // 12]
    # the limit: 5 / spacing <= 4096 passes, above it the statement refuses and names the triangle
    assert len(md.sample_statement(xyz, [[0, 0, 0], [1, 2, 3]], 5.0 / 64)["xyz"]) == 1 + 64 * 64
    with pytest.raises(ValueError, match="triangle 1"):
        md.sample_statement(xyz, [[0, 0, 0], [1, 2, 3]], np.nextafter(F(5.0 / 4096), F(0)))


@pytest.mark.parametrize("scene", ("hand", "sphere", "cube"))
def test_covering_bound_holds(scene):
    """every point of a participating triangle lies within 2/3 * spacing of one of its samples: derived in include/mpmvs.h, not measured;
    20 000 random barycentric points per scene, by brute force"""
    m, spacing = {"hand": (md.hand_mesh(), 0.7), "sphere": (mc.anchor(), 0.2), "cube": (msc.cube(4), 0.11)}[scene]
    rng = np.random.default_rng(17)
    smp = md.sample_statement(m["xyz"], m["tri"], spacing)
    t = rng.integers(0, len(m["tri"]), 20000)
    b = rng.dirichlet((1, 1, 1), 20000)
    P = m["xyz"][m["tri"][t]].astype(D)
    x = (b[:, :, None] * P).sum(1)
    worst = 0.0
    order = np.argsort(t, kind="stable")
    starts = np.searchsorted(smp["tri_of"], np.arange(len(m["tri"]) + 1))
    for tt in np.unique(t):
        mine = order[np.searchsorted(t[order], tt):np.searchsorted(t[order], tt, "right")]
        s = smp["xyz"][starts[tt]:starts[tt + 1]].astype(D)
        d = np.sqrt(((x[mine, None] - s[None]) ** 2).sum(-1)).min(1)
        worst = max(worst, float(d.max()))
    assert worst <= 2.0 / 3.0 * float(F(spacing)) * (1 + 1e-6)   # the rounding of the samples to fp32


# ---- compare and evaluate_mesh on the statements, through stubs for the device calls ------------------------------------------------------------
class _StubCloud:
    def __init__(self, xyz, device=0):
        self.xyz, self.n = np.ascontiguousarray(xyz, F).reshape(-1, 3), len(xyz)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass

    def close(self):
        pass

    def nearest(self, q, radius, want_idx=True):
        q = np.ascontiguousarray(q, F)
        d = ((q[:, None].astype(D) - self.xyz[None].astype(D)) ** 2).sum(-1).astype(F)
        d2 = d.min(1)
        d2[d2 > F(radius) * F(radius)] = np.inf
        return d2, None

    def kernel_ms(self):
        return 0.0, 0.0


class _StubMesh(_StubCloud):
    def __init__(self, xyz, tri, rgb=None, device=0):
        self.xyz, self.tri = np.ascontiguousarray(xyz, F).reshape(-1, 3), np.ascontiguousarray(tri, np.int32).reshape(-1, 3)

    def sample(self, spacing, want_normals=False):
        return md.sample_statement(self.xyz, self.tri, spacing)

    def distance(self, cloud, radius, want_tri=True):
        d2, arg, _ = md.distance_statement(self.xyz, self.tri, cloud.xyz, radius)
        return (d2, arg) if want_tri else d2

    def sample_ms(self):
        return {"total": 0.0}

    def distance_ms(self):
        return {"total": 0.0}


@pytest.fixture()
def stubbed(mesh, monkeypatch):
    cloud = importlib.import_module("mp-mvs_amd.cloud")
    monkeypatch.setattr(mesh, "Mesh", _StubMesh)
    monkeypatch.setattr(cloud, "Cloud", _StubCloud)
    return mesh


def test_compare_of_a_cube_with_itself_and_with_a_moved_copy(stubbed):
    m = msc.cube(4)
    same = stubbed.compare(m, m, 0.2, 0.5)
    for k in ("a_to_b", "b_to_a"):
        assert same[k]["beyond"] == 0 and same[k]["n"] > 0 and same[k]["max"] <= 1e-7 and same[k]["mean"] <= 1e-7 and same[k]["rms"] <= 1e-7
    assert same["hausdorff"] <= 1e-7
    # moved by delta along x: the samples of the four faces along x slide in their planes (distance 0 but for the strip of width delta
    # that leaves the face: there the nearest point is the moved face's edge, at most delta away); those of the two faces across x are
    # exactly delta from the moved face's plane.  So the maximum is delta in both directions, and a sixth of the samples -- each face
    # has equally many -- are at delta or more... at exactly delta for one face; the other face's samples find the side faces nearer.
    delta = 0.125
    moved = dict(m, xyz=(m["xyz"] + np.array([delta, 0, 0], F)).astype(F))
    out = stubbed.compare(m, moved, 0.2, 0.5)
    for k in ("a_to_b", "b_to_a"):
        assert out[k]["beyond"] == 0 and abs(out[k]["max"] - delta) <= 1e-6
        assert 0 < out[k]["mean"] < out[k]["rms"] < delta
    assert abs(out["hausdorff"] - delta) <= 1e-6
    # beyond the radius: every sample of the face that moved away from the other cube by more than the radius
    out = stubbed.compare(m, dict(m, xyz=(m["xyz"] + np.array([2.0, 0, 0], F)).astype(F)), 0.2, 0.5)
    assert out["a_to_b"]["beyond"] == out["a_to_b"]["n"] and out["a_to_b"]["max"] is None and out["hausdorff"] is None


def test_evaluate_mesh_on_a_cube_and_its_own_samples(stubbed):
    m = msc.cube(4)
    gt = np.concatenate([md.sample_statement(m["xyz"], m["tri"], 0.1)["xyz"], [[np.nan, 0, 0]], [[0.5, 0.5, 1.3]]]).astype(F)
    timings = {}
    res = stubbed.evaluate_mesh(m, gt, [0.05, 0.2, 0.4], timings=timings)
    assert res["spacing"] == 0.05 and res["dropped_ground_truth"] == 1 and res["n_ground_truth"] == len(gt) - 1
    rows = res["tolerances"]
    assert [r["n_complete"] for r in rows] == [len(gt) - 2, len(gt) - 2, len(gt) - 1]   # the point 0.3 above the top face
    assert rows[-1]["accuracy"] == 1.0 and rows[0]["accuracy"] > 0.5 and {"sample_s", "accuracy_s", "completeness_s", "device_ms"} <= set(timings)
    with pytest.raises(ValueError):
        stubbed.evaluate_mesh(m, gt, [])
    with pytest.raises(ValueError):
        stubbed.evaluate_mesh(m, gt, [0.1], spacing=-1)


# ---- the tool up to the device call ---------------------------------------------------------------------------------------------------------
def test_tool_arguments_and_loading(mesh, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    tool = importlib.import_module("eval_mesh")
    hostlib = importlib.import_module("mp-mvs_amd.hostlib")
    m = msc.cube(2)
    a, b, scan = str(tmp_path / "a.ply"), str(tmp_path / "b.ply"), str(tmp_path / "scan.ply")
    mesh.write_ply_mesh(a, m["xyz"], m["tri"])
    mesh.write_ply_mesh(b, m["xyz"] + F(0.5), m["tri"])
    pts = md.sample_statement(m["xyz"], m["tri"], 0.3)["xyz"]
    mesh.write_ply_mesh(scan, pts, np.zeros((0, 3), np.int32))   # a PLY with vertices only reads as a cloud
    args = tool.parse_args(["--mesh", a, "--ground_truth", scan, "--tolerances", "0.1,0.02"])
    assert args.tolerances == [0.1, 0.02] and args.spacing == 0.02 and args.voxel is None
    mm, other, head = tool.load(args)
    assert md.same_bits(mm["xyz"], m["xyz"]) and md.same_bits(np.ascontiguousarray(other, F), pts) and head["m"] == len(m["tri"]) and head["tolerances"] == [0.1, 0.02]
    T = np.eye(4)
    T[:3, 3] = (1, 2, 3)
    np.savetxt(str(tmp_path / "T.txt"), T)
    args = tool.parse_args(["--mesh", a, "--ground_truth", scan, "--transform", str(tmp_path / "T.txt"), "--spacing", "0.25", "--voxel", "0.1"])
    assert md.same_bits(tool.load(args)[0]["xyz"], (m["xyz"] + np.array([1, 2, 3], F)).astype(F)) and args.spacing == 0.25
    args = tool.parse_args(["--mesh", a, "--reference_mesh", b, "--radius", "0.5"])
    assert args.spacing == 0.25 and args.tolerances is None
    mm, other, head = tool.load(args)
    assert md.same_bits(other["xyz"], m["xyz"] + F(0.5)) and head["radius"] == 0.5
    for bad in (["--ground_truth", scan, "--reference_mesh", b, "--radius", "1"], [], ["--reference_mesh", b], ["--reference_mesh", b, "--radius", "0"],
                ["--reference_mesh", b, "--radius", "nan"], ["--ground_truth", scan, "--radius", "1"], ["--ground_truth", scan, "--tolerances", "0.1,x"],
                ["--ground_truth", scan, "--tolerances", "0.1,-1"], ["--ground_truth", scan, "--spacing", "0"], ["--ground_truth", scan, "--voxel", "inf"],
                ["--reference_mesh", b, "--radius", "1", "--voxel", "0.1"]):
        with pytest.raises(SystemExit):
            tool.parse_args(["--mesh", a] + bad)
    with pytest.raises(SystemExit):
        tool.load(tool.parse_args(["--mesh", str(tmp_path / "missing.ply"), "--ground_truth", scan]))
    del hostlib


def test_check_program_under_the_host_sanitizers(tmp_path):
    """tools/mesh_distance_check.cpp: the per-thread bodies of pm_surface.hpp replayed on the host in scrambled orders against plain
    loops, under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program"""
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    exe = str(tmp_path / "mesh_distance_check")
    subprocess.run([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                    "-I" + os.path.join(ROOT, "mp-mvs_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tools", "mesh_distance_check.cpp")], check=True, cwd=str(tmp_path))
    run = subprocess.run([exe], capture_output=True, text=True, cwd=str(tmp_path))
    lines = run.stdout.strip().splitlines()
    assert run.returncode == 0 and lines[-1] == "all equal", run.stdout[-2000:] + run.stderr[-2000:]
    cases = lines[:-1]
    assert len(cases) >= 40 and all(ln.endswith(": equal") for ln in cases)
    assert sum("listed" in ln and " (0 of" not in ln for ln in cases) >= 10   # the large-triangle path ran
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-2000:]
