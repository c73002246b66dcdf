"""Parity sweep of the planar prior built on the device (mp-mvs_amd/csrc/pm_prior.hpp: k_prior_cells, k_prior_raster, k_prior_finish and
the task table of mpmvs_prior_from_triangles) against the host library (mp-mvs_amd/host/planar_prior.cpp), which DESIGN.md names as
the definition and which tests/test_prior_sweep_cpu.py and tests/test_reference_host_cpu.py pin to plain restatements and to the
reference's compiled code.  Every comparison is exact.

  vertices   the inputs on which the host picker is pinned to the reference (ref_common.vertex_inputs: ties, costs exactly on the
             constants of both rules, all-invalid cells, NaN, partial cells), both rules, every size
  the sweep  prior_common.draw: degenerate, collinear, duplicate, overlapping and border triangles, longest edges around one and two
             tasks of 64 rows, zero / negative / non-finite depths, depth ranges that end on a prior depth or one float inside it
  big cases  70 001 triangles (the task table built in chunks by host threads; a task count that is no multiple of 4), forwards and
             reversed; slivers of 4096, 8192 and 14 973 pixels, the last of which runs one row more than floor(L) + 3 in whole tasks;
             one of 46 341, whose squared edge no longer fits an int
  refusals   coordinates far outside the image, at once; an image side above 65 535"""
import ctypes
import time
from types import SimpleNamespace

import numpy as np
import pytest

import prior_common as pc
import ref_common as rc
from test_prior_gpu import blank_context

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def contexts(pm, engine):
    """get(case) -> a blank context of the case's size and camera; one per size, shared by the tests of this file and closed after them"""
    held = {}

    def get(c):
        key = (c.W, c.H, tuple(c.K))
        if key not in held:
            held[key] = blank_context(pm, engine, pc.make_cam(c), c.W, c.H)
        return held[key]

    yield get
    for gpu in held.values():
        gpu.close()
    held.clear()


def _vertex_case(w, h):
    return SimpleNamespace(W=w, H=h, K=[100.0, 0.0, w / 2, 0.0, 100.0, h / 2, 0.0, 0.0, 1.0])


@pytest.mark.parametrize("geom_rule", [False, True])
@pytest.mark.parametrize("kind", rc.VERTEX_INPUTS)
@pytest.mark.parametrize("w,h", rc.VERTEX_SIZES)
def test_device_vertices_equal_host_on_the_pinned_inputs(contexts, hostlib, w, h, kind, geom_rule):
    costs, geom = rc.vertex_inputs(w, h, kind)
    gpu = contexts(_vertex_case(w, h))
    gpu.set_state(None, costs)
    gpu.set_geom_costs(geom)
    want = hostlib.triangulate_vertices(costs, geom, geom_rule)
    got = gpu.prior_vertices(geom_rule)
    assert got.dtype == want.dtype and np.array_equal(got, want)
    if kind in ("ties", "invalid_cells_and_origin"):
        # a buffer smaller than the list: the count is still the full one, the buffer holds the head of the list
        assert len(want) >= 1
        cap = len(want) // 2 + 1
        out = np.full((cap + 1, 2), -7, np.int32)
        n = ctypes.c_int(0)
        assert gpu._f["prior_vertices"](gpu._ctx, 1 if geom_rule else 0, out.ctypes.data, cap, ctypes.byref(n)) == 0
        assert n.value == len(want) and np.array_equal(out[:cap], want[:cap]) and (out[cap] == -7).all()


def _same_prior(got, want, what):
    """(prior, mask) of the device against the host's: the mask exactly, the planes bit for bit where the host's value is no NaN and
    NaN where it is one, nothing but zeros where the mask is 0"""
    (p_dev, m_dev), (p_host, m_host) = got, want
    assert m_dev.shape == m_host.shape and p_dev.shape == p_host.shape
    diff = np.argwhere(m_dev != m_host)
    assert len(diff) == 0, (what, f"{len(diff)} mask pixels differ, the first (y, x) {diff[:8].tolist()}: device {m_dev[tuple(diff[:8].T)].tolist()}, host {m_host[tuple(diff[:8].T)].tolist()}")
    nan = np.isnan(p_host)
    assert np.array_equal(np.isnan(p_dev), nan), what
    assert np.array_equal(p_dev.view(np.uint32)[~nan], p_host.view(np.uint32)[~nan]), what
    assert not p_dev.view(np.uint32)[m_dev == 0].any(), what


def _both(pm, contexts, hostlib, c, tri=None, depth_range=None, planes=None):
    """((prior, mask) of the device, (prior, mask) of the host) for the case, or for the triangles, range or state given instead"""
    tri = c.tri if tri is None else tri
    planes = c.planes if planes is None else planes
    lo, hi = (c.depth_min, c.depth_max) if depth_range is None else depth_range
    gpu = contexts(c)
    gpu.set_state(planes, None)
    gpu.prior_from_triangles(pm.PatchMatchParams(num_images=2, depth_min=lo, depth_max=hi), tri)
    return gpu.get_prior(), hostlib.prior_from_triangles(pc.make_cam(c), tri, planes, lo, hi)[:2]


@pytest.mark.parametrize("case", range(pc.DEFAULT_CASES))
def test_sweep_device_prior_equals_host(pm, contexts, hostlib, case):
    c = pc.draw(case)
    got, want = _both(pm, contexts, hostlib, c)
    _same_prior(got, want, f"case {case}: {c.W} x {c.H}, {len(c.tri)} triangles, {sorted(c.tri_kinds)}, {sorted(c.depth_kinds)}, {c.range_kind}")
    # again on the same context, unbounded: the host's unbounded run, so nothing of the first call is left in the mask buffer
    got, want = _both(pm, contexts, hostlib, c, depth_range=(-pc.BIG, pc.BIG))
    _same_prior(got, want, f"case {case}, unbounded")
    if len(c.tri):
        assert (want[1] > 0).any()


def test_many_triangles_forwards_and_reversed(pm, contexts, hostlib):
    c = pc.many_triangles()
    n = len(c.tri)
    # over a state of one depth no pixel fails the range test: the raw labels
    raw = dict(planes=c.level, depth_range=(-pc.BIG, pc.BIG))
    got, want = _both(pm, contexts, hostlib, c, **raw)
    _same_prior(got, want, "70 001 triangles")
    fwd = got[1].astype(np.int64)
    assert (fwd > 0).mean() > 0.9 and fwd.max() > 65536
    got_r, want_r = _both(pm, contexts, hostlib, c, tri=c.tri[::-1], **raw)
    _same_prior(got_r, want_r, "70 001 triangles, reversed")
    back = np.where(got_r[1] > 0, n + 1 - got_r[1].astype(np.int64), 0)       # in labels of the forward list: now the FIRST triangle wins
    assert np.array_equal(back > 0, fwd > 0) and (back <= fwd).all()
    # forwards the largest index that covers a pixel, reversed the smallest (the host's, both): one triangle covers it where they agree
    once = (want[1] > 0) & (want[1] == np.where(want_r[1] > 0, n + 1 - want_r[1].astype(np.int64), 0))
    assert 0.02 < once.mean() < 0.98 and np.array_equal(back[once], fwd[once])
    # the case's own state and range: plane fit and finish kernel over labels above 65 536
    _same_prior(*_both(pm, contexts, hostlib, c), "70 001 triangles, ranged")


@pytest.mark.parametrize("k", range(len(pc.long_slivers())), ids=[f"{s.W}x{s.H}" for s in pc.long_slivers()])
def test_long_sliver_device_prior_equals_host(pm, contexts, hostlib, k):
    """14974x8 is the case a task table of floor(L) + 3 rows lost: the loop's row 14 976, the only one to reach pixel (14972, 0), lay
    past its last task (14 976 rows dispatched, 14 977 run)"""
    c = pc.long_slivers()[k]
    got, want = _both(pm, contexts, hostlib, c, depth_range=(-pc.BIG, pc.BIG))
    _same_prior(got, want, f"sliver {c.W} x {c.H}, unbounded")
    assert (want[1] == c.sliver + 1).sum() > c.L and len(np.unique(want[1])) > 4     # the sliver, and small triangles over and under it
    _same_prior(*_both(pm, contexts, hostlib, c), f"sliver {c.W} x {c.H}")


def test_sliver_whose_squared_edge_passes_int32(pm, contexts, hostlib):
    """46342 x 8: kernel and host formed the squared edge in an int, which wraps here.  The host's longest edge came out as NaN and it
    left one sample of the sliver (tests/test_prior_sweep_cpu.py pins it to the statement now); the kernel's build happened to form
    the product wide and already gave the whole sliver, which nothing promised.  One run: the host's half of 46 341^2 samples on one
    thread are most of this test's 2 s, and only at this width can the product wrap."""
    c = pc.wide_sliver()
    got, want = _both(pm, contexts, hostlib, c)
    _same_prior(got, want, f"sliver {c.W} x {c.H}")
    assert (want[1] == c.sliver + 1).sum() > 2 * c.L


def test_unchecked_coordinates_are_refused_at_once(pm, contexts):
    """a vertex far outside the image: refused with -2 before a row is counted for it (the row count of an edge of 1e8 px is a loop
    that never ends), also behind valid triangles and 70 000 times over"""
    c = pc.draw(0)
    gpu = contexts(c)
    prm = pm.PatchMatchParams(num_images=2, depth_min=1.0, depth_max=9.0)
    far = np.array([[[1, 1], [5, 2], [100000000, 3]]], np.int32)
    t0 = time.perf_counter()
    for tri in (far, np.concatenate([c.tri, far]), np.repeat(far, 70000, 0), np.array([[[1, 1], [2 ** 31 - 1, 2], [-2 ** 31, 3]]], np.int32)):
        with pytest.raises(RuntimeError, match="outside the image"):
            gpu.prior_from_triangles(prm, tri)
    assert time.perf_counter() - t0 < 1.0


def test_image_side_above_the_vertex_packing_is_refused(pm, contexts):
    """65536 x 2: (y << 16) | x no longer holds the vertices, and the row bound is stated up to 65 535; one column less is taken"""
    prm = pm.PatchMatchParams(num_images=2, depth_min=1.0, depth_max=9.0)
    tri = np.array([[[0, 0], [9, 1], [3, 1]]], np.int32)
    for w, h in ((65536, 2), (2, 65536)):
        gpu = contexts(_vertex_case(w, h))
        gpu.set_state(np.ones((h, w, 4), np.float32), None)
        with pytest.raises(RuntimeError, match="above 65535"):
            gpu.prior_from_triangles(prm, tri[:, :, ::-1] if h > w else tri)
    gpu = contexts(_vertex_case(65535, 2))
    gpu.set_state(np.ones((2, 65535, 4), np.float32), None)
    gpu.prior_from_triangles(prm, tri)
    assert (gpu.get_prior()[1] == 1).sum() >= 5
