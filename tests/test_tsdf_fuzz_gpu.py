"""Seeded randomized parity sweeps of the TSDF family on the MI355X, bit for bit against the numpy statements of tsdf_common.py and
tsdf_sparse_common.py, on the cases of tests/tsdf_fuzz_common.py; tests/test_tsdf_fuzz_cpu.py asserts what those cases cover.
  A. integration: Volume against integrate_statement; SparseVolume against the masked statement and against the masked result of the
     dense Volume on the GPU -- lattices with ragged tiles and cut-off bricks, 1..19 views in 1..3 calls, boxes that the block test
     culls and boxes it nearly culls, bad depths, three colour modes, brick sets from allocate, from a random mask, or complete.
  B. mesh through set / set_bricks: random fields with invalid corners, NaN, infinite, denormal and signed-zero sums, colour means
     beyond a byte, brick masks; two cases above 65536 entries.
  C. lives of a sparse handle: allocate, integrate, set_bricks, mesh, reads and refused allocates in random order against a numpy
     model, the whole observable state compared after every operation.
Below the sweeps, named cases: the bound above which a view is not culled, NaN cameras, and 8, 9, 16 and 17 views in one call.

Comparison rule (tsdf_common.same_bits): equal bits wherever the statement's value is not NaN, NaN wherever it is; integers equal.

MPMVS_TSDF_FUZZ_CASES=N scales the sweeps (default 60: 60 + 60 + 30 cases).  The whole file on the MI355X, 150 cases and the five named
tests: 6.0 s (1.5 s of it the first library load); the slowest case 0.5 s (the first integration), every other at most 0.2 s."""
import importlib
import os

import numpy as np
import pytest

import tsdf_common as tc
import tsdf_fuzz_common as fz
import tsdf_sparse_common as sc

pytestmark = pytest.mark.gpu
F = np.float32
SCALE = os.environ.get("MPMVS_TSDF_FUZZ_CASES")


@pytest.fixture(scope="module")
def mesh(pm, engine):
    return importlib.import_module("mp-mvs_amd.mesh")


def _same_volume(got, want, where):
    """got: what Volume.get / SparseVolume.to_dense return; want: (sum, weight, color4 or None)"""
    assert tc.same_bits(got["sum"], want[0]), where
    assert np.array_equal(got["weight"], want[1]), where
    assert (want[2] is None and "color" not in got) or np.array_equal(got["color"], want[2]), where


def _same_bricks(got, dims, bricks, want, where):
    """got: what get_bricks returns; want: masked dense arrays"""
    assert np.array_equal(got["coords"], sc.brick_coords(bricks)), where
    assert tc.same_bits(got["sum"], sc.to_bricks(dims, bricks, want[0])), where
    assert np.array_equal(got["weight"], sc.to_bricks(dims, bricks, want[1])), where
    assert (want[2] is None and "color" not in got) or np.array_equal(got["color"], sc.to_bricks(dims, bricks, want[2])), where


def _same_mesh(got, want, where):
    assert tc.same_bits(got["xyz"], want["xyz"]), (where, got["xyz"].shape, want["xyz"].shape)
    assert got["tri"].dtype == np.int32 and np.array_equal(got["tri"], want["tri"]), (where, got["tri"].shape, want["tri"].shape)
    assert (got["rgb"] is None and want["rgb"] is None) or np.array_equal(got["rgb"], want["rgb"]), where


def _without_nan_triangles(m):
    """the triangles whose three vertices are numbers: a NaN position has no one bit pattern to look a triangle up by"""
    tri = np.asarray(m["tri"], np.int64).reshape(-1, 3)
    return {"xyz": m["xyz"], "tri": tri[~np.isnan(m["xyz"]).any(1)[tri].any(1)]}


def _integrate(v, c, call=slice(None)):
    v.integrate(c.cams[call], c.depths[call], None if c.images is None else c.images[call])


def _zero_bricks(v, dims, bricks):
    """installs `bricks`, all zero, through set_bricks"""
    n = int(bricks.sum())
    v.set_bricks(sc.brick_coords(bricks), np.zeros((n, 8, 8, 8), F), np.zeros((n, 8, 8, 8), np.int32))


# ---- A. integration -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(fz.n_cases("A", SCALE)))
def test_integrate_case(mesh, pm, k):
    c = fz.integrate_case(pm, k)
    want = fz.integrate_want(c)
    with mesh.Volume(c.origin, c.voxel, c.dims, c.trunc, color=c.images is not None) as d:
        for call in c.calls:
            _integrate(d, c, call)
        dense = d.get()
    _same_volume(dense, want, (k, "dense"))
    masked = sc.mask_dense(c.dims, c.bricks, *want)
    gpu_masked = sc.mask_dense(c.dims, c.bricks, dense["sum"], dense["weight"], dense.get("color"))
    with mesh.SparseVolume(c.origin, c.voxel, c.dims, c.trunc, color=c.images is not None, pad=c.pad) as v:
        if c.brick_mode == "allocate":
            v.allocate([c.cams[q] for q in c.alloc_views], [c.depths[q] for q in c.alloc_views])
        else:
            _zero_bricks(v, c.dims, c.bricks)
        assert np.array_equal(v.bricks(), sc.brick_coords(c.bricks)), (k, c.brick_mode)
        for call in c.calls:
            _integrate(v, c, call)
        got, back = v.get_bricks(), v.to_dense()
    _same_bricks(got, c.dims, c.bricks, masked, (k, "sparse against the masked statement"))
    _same_bricks(got, c.dims, c.bricks, gpu_masked, (k, "sparse against the masked dense volume"))
    _same_volume(back, masked, (k, "to_dense"))


# ---- B. mesh ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(fz.n_cases("B", SCALE)))
def test_mesh_case(mesh, k):
    c = fz.mesh_case(k)
    want_dense, want_sparse = fz.mesh_want(c)
    colour = c.color4 is not None
    with mesh.Volume(c.origin, c.voxel, c.dims, 1.0, color=colour) as v:
        v.set(c.total, c.weight, c.color4)
        dense, again = v.mesh(c.min_weight), v.mesh(c.min_weight)
    _same_mesh(dense, want_dense, (k, "dense"))
    _same_mesh(again, dense, (k, "dense, the second call"))
    coords, s, w, col = fz.brick_arrays(c.dims, c.bricks, c.total, c.weight, c.color4, garbage=True)
    with mesh.SparseVolume(c.origin, c.voxel, c.dims, 1.0, color=colour) as v:
        v.set_bricks(coords, s, w, col)
        _same_bricks(v.get_bricks(), c.dims, c.bricks, sc.mask_dense(c.dims, c.bricks, c.total, c.weight, c.color4), (k, "set_bricks"))
        sparse, again = v.mesh(c.min_weight), v.mesh(c.min_weight)
    _same_mesh(sparse, want_sparse, (k, "sparse"))
    _same_mesh(again, sparse, (k, "sparse, the second call"))
    assert sc.triangle_set(_without_nan_triangles(sparse)) <= sc.triangle_set(_without_nan_triangles(dense)), k


# ---- C. lives -----------------------------------------------------------------------------------------------------------------------
def _same_state(v, model, where, everything=False):
    c = model.c
    want = (model.total, model.weight, model.color4)
    assert np.array_equal(v.bricks(), sc.brick_coords(model.bricks)), where
    st = v.stats()
    assert st["bricks"] == model.n_bricks() == v.n_bricks() and st["max_bricks"] == c.max_bricks and st["grid_cells"] == model.bricks.size, where
    _same_bricks(v.get_bricks(), c.dims, model.bricks, want, where)
    if everything:
        _same_volume(v.to_dense(), want, where)


@pytest.mark.parametrize("k", range(fz.n_cases("C", SCALE)))
def test_life_of_a_sparse_handle(mesh, pm, k):
    c = fz.life_case(pm, k)
    model = fz.Model(c)
    with mesh.SparseVolume(c.origin, c.voxel, c.dims, c.trunc, color=c.with_color, pad=c.pad, max_bricks=c.max_bricks) as v:
        _same_state(v, model, (k, "fresh"))
        for step, op in enumerate(c.ops):
            where = (k, step, op[0])
            if op[0] == "allocate":
                v.allocate(*model.views(op[1])[:2])
            elif op[0] == "refused":
                with pytest.raises(ValueError, match="max_bricks"):
                    v.allocate(*model.views(op[1])[:2])
            elif op[0] == "integrate":
                v.integrate(*model.views(op[1]))
            elif op[0] == "set_bricks":
                v.set_bricks(*fz.brick_arrays(c.dims, op[1], op[2], op[3], op[4], garbage=True))
            elif op[0] == "mesh":
                got, want = v.mesh(op[1]), model.apply(op)
                _same_mesh(got, want, where)
            if op[0] != "mesh":
                model.apply(op)
            _same_state(v, model, where, everything=op[0] in ("read", "refused"))


# ---- named cases --------------------------------------------------------------------------------------------------------------------
def test_views_above_the_cull_bound_and_nan_cameras_are_evaluated(mesh, pm):
    """a camera 2^41 away and two cameras with a NaN entry are not culled (W.cull == 0) and sit in one chunk between ordinary views:
    the first contributes to every voxel, the other two to none, as the statement has it"""
    c = fz.cull_bound_case(pm)
    want = tc.integrate_statement(c.origin, c.voxel, c.dims, c.trunc, c.cams, c.depths, c.images)
    alone = {v: tc.integrate_statement(c.origin, c.voxel, c.dims, c.trunc, [c.cams[v]], [c.depths[v]]) for v in (c.far, c.nan_k, c.nan_r)}
    assert (alone[c.far][1] == 1).all() and not alone[c.nan_k][1].any() and not alone[c.nan_r][1].any()
    with mesh.Volume(c.origin, c.voxel, c.dims, c.trunc, color=True) as d:
        _integrate(d, c)
        _same_volume(d.get(), want, "dense")
    for v, w in alone.items():
        with mesh.Volume(c.origin, c.voxel, c.dims, c.trunc) as d:
            d.integrate([c.cams[v]], [c.depths[v]])
            _same_volume(d.get(), w, ("dense, alone", v))
    bricks = fz.all_bricks(c.dims)
    bricks[0, 1, 2] = False
    with mesh.SparseVolume(c.origin, c.voxel, c.dims, c.trunc, color=True) as v:
        _zero_bricks(v, c.dims, bricks)
        _integrate(v, c)
        _same_bricks(v.get_bricks(), c.dims, bricks, sc.mask_dense(c.dims, bricks, *want), "sparse")


@pytest.mark.parametrize("n", fz.FORCED_VIEWS)
def test_one_call_equals_single_view_calls_at_the_chunk_boundaries(mesh, pm, n):
    c = fz.chunk_case(pm, n)
    want = tc.integrate_statement(c.origin, c.voxel, c.dims, c.trunc, c.cams, c.depths, c.images)
    assert want[1].max() >= 2
    bricks = sc.allocate_statement(c.origin, c.voxel, c.dims, c.trunc, 1.0, c.cams, c.depths)
    got = {}
    for calls in ([slice(None)], [slice(q, q + 1) for q in range(n)]):
        with mesh.Volume(c.origin, c.voxel, c.dims, c.trunc, color=True) as d:
            for call in calls:
                _integrate(d, c, call)
            got["dense", len(calls)] = d.get()
        with mesh.SparseVolume(c.origin, c.voxel, c.dims, c.trunc, color=True, pad=1.0) as v:
            v.allocate(c.cams, c.depths)
            for call in calls:
                _integrate(v, c, call)
            got["sparse", len(calls)] = v.get_bricks()
    for key in ("sum", "weight", "color"):
        assert got["dense", 1][key].tobytes() == got["dense", n][key].tobytes() and got["sparse", 1][key].tobytes() == got["sparse", n][key].tobytes(), key
    _same_volume(got["dense", 1], want, "dense")
    _same_bricks(got["sparse", 1], c.dims, bricks, sc.mask_dense(c.dims, bricks, *want), "sparse")
