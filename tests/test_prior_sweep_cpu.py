"""What the parity sweep of the device-built planar prior (tests/test_prior_sweep_gpu.py) stands on, without a GPU: the census of the
seeded cases, the host library (mp-mvs_amd/host/planar_prior.cpp, the definition the device is compared with) against the plain
restatements of tests/prior_common.py, and the row bound of the raster's task table (pm::prior_rows, csrc/pm_prior.hpp) against the
reference's fp32 loop, which runs more rows than floor(L) + 3 on long slivers (the planar-prior section)."""
import importlib
import os
import subprocess
import time
from types import SimpleNamespace

import numpy as np
import pytest

import prior_common as pc

hostlib = importlib.import_module("mp-mvs_amd.hostlib")
engine = importlib.import_module("mp-mvs_amd.engine")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_census_holds_and_draw_is_deterministic():
    count = pc.census()
    assert set(count) == set(pc.TRI_KINDS + pc.DEPTH_KINDS + pc.RANGE_KINDS)
    assert min(count.values()) >= pc.CENSUS_MIN, count
    cases = [pc.draw(k) for k in range(pc.DEFAULT_CASES)]
    assert any(len(c.tri) == 0 for c in cases) and max(len(c.tri) for c in cases) > 300
    assert sum(c.K[0] != c.K[4] for c in cases) == pc.DEFAULT_CASES // 2
    assert all(5 <= min(c.W, c.H) and (max(c.W, c.H) <= 160 or (c.case % 4 == 3 and min(c.W, c.H) <= 8)) for c in cases)
    for k in (0, 7, 30):
        a, b = pc.draw(k), pc._draw(k, pc.attempt())
        assert a is not b and (a.W, a.H, a.K, a.d0, a.depth_min, a.depth_max, a.range_kind) == (b.W, b.H, b.K, b.d0, b.depth_min, b.depth_max, b.range_kind)
        assert np.array_equal(a.tri, b.tri) and np.array_equal(a.planes, b.planes, equal_nan=True)
    # the fronto-parallel prior at d0 has depth d0 exactly: -w * fx / (fx * nz) with fl(d0 * fx) exact
    for c in cases:
        d0, fx = np.float32(c.d0), np.float32(c.K[0])
        assert float(d0) * float(fx) == float(d0 * fx) and (d0 * fx) / fx == d0


def test_big_cases_are_what_they_claim():
    m = pc.many_triangles()
    assert len(m.tri) == 70001 > 65536 and ((m.tri >= 0) & (m.tri < [m.W, m.H])).all()
    tasks = (engine.prior_rows(pc.longest_edge_sq(m.tri)).astype(np.int64) + pc.TASK_ROWS - 1) // pc.TASK_ROWS
    assert int(tasks.sum()) % 4 != 0                                   # a block of the raster kernel takes 4 tasks
    sl = pc.long_slivers()
    assert [s.L for s in sl[:3]] == [4096, 8192, 14973] and [(s.W, s.H) for s in sl[:3]] == [(4097, 8), (8193, 8), (14974, 8)]
    assert len(sl) == (3 if pc.whole_task_edge() is None else 4)
    for s in sl:
        assert pc.longest_edge_sq(s.tri)[s.sliver] == s.e and ((s.tri >= 0) & (s.tri < [s.W, s.H])).all()
    # from 14974 x 8 on the inputs can catch a table that stops at floor(L) + 3 rows: the loop runs past its last task
    for s in sl[2:]:
        assert pc.reference_rows(s.e) > pc.dispatched_rows_before(s.e), (s.L, pc.reference_rows(s.e), pc.dispatched_rows_before(s.e))
    assert (pc.reference_rows(sl[2].e), int(pc.dispatched_rows_before(sl[2].e))) == (14977, 14976)
    for s in sl[:2]:
        assert pc.reference_rows(s.e) <= s.L + 3


def _restricted(c, max_tri=40, max_w=60, max_h=40):
    """the case cut down to what the slow statements can do: the top-left window and the first triangles that lie inside it"""
    W, H = min(c.W, max_w), min(c.H, max_h)
    inside = ((c.tri >= 0) & (c.tri < [W, H])).all((1, 2))
    return W, H, c.tri[inside][:max_tri], np.ascontiguousarray(c.planes[:H, :W])


def _level(W, H, depth=5.0):
    planes = np.zeros((H, W, 4), np.float32)
    planes[..., 2], planes[..., 3] = -1.0, depth
    return planes


def test_host_raster_and_planes_equal_the_statements():
    """the first 12 cases of the sweep, cut down to 60 x 40 pixels and 40 triangles: labels exactly; planes to 1e-5 (the bar of
    tests/test_prior_golden_cpu.py) where the triangle has an area of at least 1 px^2 and finite depths in [1, 10]; elsewhere the positions
    of NaN, the sign rule and the fronto-parallel fallback"""
    n_tri = n_good = n_flat = n_nan = 0
    for k in range(12):
        c = pc.draw(k)
        W, H, tri, planes = _restricted(c)
        cam = pc.make_cam(SimpleNamespace(K=c.K, W=W, H=H))
        # raw labels: over a state of one depth every plane is the fronto-parallel one at that depth and no pixel fails the range test
        _, label, _ = hostlib.prior_from_triangles(cam, tri, _level(W, H), -pc.BIG, pc.BIG)
        assert np.array_equal(label, pc.raster_statement(W, H, tri)), k
        _, _, pl = hostlib.prior_from_triangles(cam, tri, planes, -pc.BIG, pc.BIG)
        assert pl.shape == (len(tri), 4)
        want, fallback = pc.plane_statement(cam, planes[..., 3], tri)
        d = planes[tri[..., 1], tri[..., 0], 3] if len(tri) else np.zeros((0, 3), np.float32)
        finite = np.isfinite(d).all(1)
        good = finite & (pc.area2(tri) >= 2) & (d >= 1.0).all(1) & (d <= 10.0).all(1)
        assert not fallback[good].any()
        assert np.abs(pl[good].astype(np.float64) - want[good]).max(initial=0.0) < 1e-5, k
        assert (pl[good, 3] > 0).all()
        # NaN exactly where the statement has it, and never from finite depths; the offset is never negative (reference :746-752)
        assert np.array_equal(np.isnan(pl), np.isnan(want)) and not np.isnan(pl[finite]).any(), k
        assert not (pl[:, 3] < 0).any()
        # the fallback: a repeated vertex gives no plane; the fronto-parallel one through the first vertex, facing the camera
        same = (tri[:, 0] == tri[:, 1]).all(1) | (tri[:, 0] == tri[:, 2]).all(1) | (tri[:, 1] == tri[:, 2]).all(1)
        assert fallback[same].all()
        assert np.array_equal(pl[fallback], want[fallback].astype(np.float32), equal_nan=True), k
        flat = fallback & finite
        d1 = d[flat, 0]
        assert np.array_equal(pl[flat], np.stack([0 * d1, 0 * d1, np.where(d1 < 0, 1, -1).astype(np.float32), np.abs(d1)], 1)), k
        n_tri, n_good, n_flat, n_nan = n_tri + len(tri), n_good + int(good.sum()), n_flat + int(flat.sum()), n_nan + int((~finite).sum())
    print(f"{n_tri} triangles: {n_good} with a plane to compare, {n_flat} on the fallback with finite depths, {n_nan} with a non-finite depth")
    assert n_tri >= 200 and n_good >= 50 and n_flat >= 10 and n_nan >= 10


def test_host_range_test_equals_the_statement_and_the_edge_decides():
    """every case of the sweep: the host's mask and prior under the case's range against the range test restated (the raw labels, the
    host's per-triangle planes, the prior depth in fp32, `<=` and `>=`); and where a pixel's prior depth is d0 exactly, a range that
    ends on d0 keeps it and one that ends a float inside drops it: in at least CENSUS_MIN cases of each of the four kinds"""
    f = np.float32
    decided = {kd: 0 for kd in pc.RANGE_KINDS if kd.endswith("d0")}
    for k in range(pc.DEFAULT_CASES):
        c = pc.draw(k)
        cam = pc.make_cam(c)
        _, raw, _ = hostlib.prior_from_triangles(cam, c.tri, _level(c.W, c.H), -pc.BIG, pc.BIG)
        prior, mask, pl = hostlib.prior_from_triangles(cam, c.tri, c.planes, c.depth_min, c.depth_max)
        on = raw > 0
        per_pixel = np.zeros((c.H, c.W, 4), f)
        per_pixel[on] = pl[raw[on] - 1]
        dd = pc.prior_depth_statement(c.K, per_pixel, c.W, c.H)

        def stated(lo, hi):
            with np.errstate(invalid="ignore"):
                keep = on & (dd <= f(hi)) & (dd >= f(lo))
            return np.where(keep, raw, 0).astype(np.uint32), np.where(keep[..., None], per_pixel, f(0))

        want_mask, want_prior = stated(c.depth_min, c.depth_max)
        assert np.array_equal(mask, want_mask), k
        assert np.array_equal(prior.view(np.uint32), want_prior.view(np.uint32)), k
        at_d0 = on & (dd == f(c.d0))
        if not at_d0.any():
            continue
        d0, above, below = float(f(c.d0)), float(np.nextafter(f(c.d0), f(np.inf))), float(np.nextafter(f(c.d0), f(-np.inf)))
        for (lo_a, hi_a), (lo_b, hi_b) in (((d0, pc.BIG), (above, pc.BIG)), ((-pc.BIG, d0), (-pc.BIG, below))):
            m_on = hostlib.prior_from_triangles(cam, c.tri, c.planes, lo_a, hi_a)[1]
            m_in = hostlib.prior_from_triangles(cam, c.tri, c.planes, lo_b, hi_b)[1]
            assert np.array_equal(m_on, stated(lo_a, hi_a)[0]) and np.array_equal(m_in, stated(lo_b, hi_b)[0]), k
            assert np.array_equal(m_on != m_in, at_d0) and (m_on[at_d0] == raw[at_d0]).all() and not m_in[at_d0].any(), k
        if c.range_kind in decided:
            decided[c.range_kind] += 1
    assert min(decided.values()) >= pc.CENSUS_MIN, decided


def test_host_raster_equals_the_statement_on_the_long_sliver():
    """the whole 14974 x 8 image, every one of the sliver's 14 977 rows restated (a few seconds)"""
    s = pc.long_slivers()[2]
    cam = pc.make_cam(s)
    _, label, _ = hostlib.prior_from_triangles(cam, s.tri, _level(s.W, s.H), -pc.BIG, pc.BIG)
    want = pc.raster_statement(s.W, s.H, s.tri)
    assert np.array_equal(label, want)
    # what a table of floor(L) + 3 rows in whole tasks loses: the rows past it label a pixel no earlier row reaches, and nothing overwrites it
    cut = int(pc.dispatched_rows_before(s.e))
    late = pc.raster_rows(s.W, s.H, s.tri[s.sliver], first_row=cut)
    lost = late & ~pc.raster_rows(s.W, s.H, s.tri[s.sliver], end_row=cut) & (want == s.sliver + 1)
    assert [tuple(p) for p in np.argwhere(lost)] == [(0, 14972)]


def test_host_raster_on_an_edge_whose_square_passes_int32():
    """46342 x 8: the squared edge 46 341^2 + 25 no longer fits an int32; formed in one, the longest edge came out as NaN and the
    sliver as a single sample.  The whole restatement would take minutes: the first three and the last 70 of the loop's 46 346 rows
    are restated, and the count of the sliver's pixels is compared with the triangle's area.  (The host run takes about 5 s: half
    of 46 341^2 samples on one thread.)"""
    s = pc.wide_sliver()
    assert 46340 ** 2 < 2 ** 31 < 46341 ** 2 and s.e == pc.longest_edge_sq(s.tri)[s.sliver]
    _, label, _ = hostlib.prior_from_triangles(pc.make_cam(s), s.tri, _level(s.W, s.H), -pc.BIG, pc.BIG)
    rows, own = pc.reference_rows(s.e), s.sliver + 1
    assert rows == 46346
    stated = pc.raster_rows(s.W, s.H, s.tri[s.sliver], end_row=3) | pc.raster_rows(s.W, s.H, s.tri[s.sliver], first_row=rows - 70)
    assert stated.sum() >= 75 and (label[stated] >= own).all()            # the sliver's label, or that of a later triangle over it
    assert (label[:, s.L - 7:][stated[:, s.L - 7:]] == own).all() and stated[0, s.L - 1]
    # the triangle (L, 0), (0, 5), (0, 0) holds the pixels with y <= 5 (1 - x / L): L (1 + 0.8 + 0.6 + 0.4 + 0.2) = 3 L of them, of
    # which the dozen small triangles, 40 columns wide, can hide at most 40 * 5
    assert 3 * s.L - 200 - 10 <= (label == own).sum() <= 3 * s.L + 10
    assert not (label[5:] == own).any()


def test_row_bound_covers_the_loop():
    """pm::prior_rows through mpmvs_prior_rows: never below the loop's count, never more than a task above"""
    L = np.arange(1, 65536, dtype=np.int64)
    e = np.concatenate([L * L, np.random.default_rng([pc.CASE_SEED, 3]).integers(0, 2 * 65535 ** 2, 100000)])
    got, want = engine.prior_rows(e).astype(np.int64), pc.reference_rows(e)
    print(f"bound - loop in [{(got - want).min()}, {(got - want).max()}]; loop - floor(L) in [{(want[:65535] - L).min()}, {(want[:65535] - L).max()}] for integer L")
    assert (got >= want).all(), e[got < want][:5]
    assert (got <= want + pc.TASK_ROWS).all(), e[got > want + pc.TASK_ROWS][:5]
    assert (want[:65535] > pc.dispatched_rows_before(L * L)).any()     # the rows dispatched before did not cover it
    with pytest.raises(RuntimeError):
        engine.prior_rows([-1])


def test_row_bound_refuses_edges_no_image_holds():
    """beyond 2 * 65535^2 the count is refused, at once: from L ~ 3.4e7 on p stops moving and the loop it counts never ends"""
    top = 2 * 65535 ** 2
    assert int(engine.prior_rows([top])[0]) == pc.reference_rows(top)
    t0 = time.perf_counter()
    for e in (top + 1, 10 ** 15, 10 ** 16, 2 ** 62):
        with pytest.raises(RuntimeError):
            engine.prior_rows([4, e, 9])
    assert time.perf_counter() - t0 < 1.0


def test_check_program_under_the_host_sanitizers(tmp_path):
    """tools/prior_rows_check.cpp: pm::prior_rows from the header itself, included without HIP, against the literal loop, under
    AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program (every 16th L and a 16th of the drawn e: the full ranges are
    test_row_bound_covers_the_loop's)"""
    exe = str(tmp_path / "prior_rows_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "mp-mvs_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tools", "prior_rows_check.cpp")], check=True, cwd=str(tmp_path))
    run = subprocess.run([exe, "16"], capture_output=True, text=True, cwd=str(tmp_path))
    lines = run.stdout.strip().splitlines()
    assert run.returncode == 0 and len(lines) == 6 and lines[-1] == "all covered", run.stdout[-2000:] + run.stderr[-2000:]
    assert all("below the loop 0, a task or more above 0" in ln for ln in lines[:4]) and lines[4].endswith(": refused")
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-2000:]
