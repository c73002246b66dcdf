"""Long-lived mpmvs_cloud handles on the MI355X: seeded random programs of nearest, knn, knn_self, normals, components, the two
align passes and render_depth on ONE handle per case (tests/cloud_seq_common.py), 9..12 radii against the eight grids a handle
keeps, so that grids are evicted, their buffers rebuilt for other radii and evicted radii asked for again.  After every step: the
result against the operation's statement under the rule of its own test file (every row, bit for bit); the build figure of the call
against a plain model of the cache (GridCacheModel: > 0 exactly on a miss); the handle's statistics (finite and slots never change,
cells and fullest are a function of the radius).  At the end of a program its first three grid-using steps run again on fresh
handles and must give the same bits.  tests/test_cloud_seq_cpu.py asserts what the programs cover.  Below the sweep, named cases:
the eviction order, two radii one ulp apart (as a neighbour's distance and as a cell border), aligners that outlive evictions, and the project's own callers (cloud.distances,
cloud.align) with ten radii on one handle.

A call that never reaches the grid (no queries, no sources, a render) is no request: the model is not asked and the figures must
stay what they were.

Against deliberately broken builds of cloud_grid (the key compared on the top 20 bits of the radius; the most recently used grid
evicted): every case of the sweep with a finite target fails on the build figure under either break, test_eviction_order and
test_aligners_across_eviction as well, test_radii_one_ulp_apart under the first, test_cascade_and_rounds_beyond_eight under the
second; the 166 older tests of the cloud operations pass under both.  Under the first break the results stay right on these inputs
(the kernels take r2 and the cell edge from the call's radius, and a grid built for an edge one ulp off files a point under
another cell only where it sits within a rounding of a cell border): the build figure is what shows a stale grid there, and
test_grid_of_the_neighbouring_radius_would_miss puts a point on such a border, where the first break loses the neighbour itself.

MPMVS_CLOUD_SEQ_CASES=N widens or narrows the sweep (default 24).  The whole file on the MI355X, 24 cases and the seven named
tests: 3.4 s (1.5 s of it the first library load); the slowest case takes 0.46 s (case 0, the first to touch the device), no
other test above 0.13 s."""
import importlib
import os

import numpy as np
import pytest

import align_common as ac
import align_plane_common as apc
import cloud_seq_common as sq
from cloud_common import assert_same, bits, brute_nearest
from cloud_seq_common import Step

pytestmark = pytest.mark.gpu
I4 = np.eye(4)


@pytest.fixture(scope="module")
def cloud(engine):
    return importlib.import_module("mp-mvs_amd.cloud")


def _figures(h):
    return h.kernel_ms()[1], h.knn_ms()[1], h.normals_ms()[1], h.components_ms()[1]


class Runner:
    """one Cloud over the targets of case c, its aligners, and the model beside them; step() runs one entry of a program and checks
    everything that can be checked after it"""

    def __init__(self, cloud, c):
        self.cloud, self.c = cloud, c
        self.h = cloud.Cloud(c.target)
        self.model = sq.GridCacheModel(c.n_fin > 0)
        self.aligners, self.slots, self.grid_stats, self.results = {}, None, {}, []
        assert self.h.stats() == dict(finite=0, cells=0, fullest=0, slots=0) and _figures(self.h) == (0, 0, 0, 0)

    def step(self, s):
        """-> (result, built)"""
        c, h = self.c, self.h
        if s.kind == "open":
            self.aligners[s.args["al"]] = sq.open_aligner(self.cloud, h, c, s.args["al"])
            return None, False
        if s.kind == "close":
            self.aligners.pop(s.args["al"]).close()
            return None, False
        what = f"case {c.k}, step {len(self.results)}"
        figures, stats = _figures(h), h.stats()
        got = sq.run_step(h, self.aligners, c, s)
        sq.assert_step_same(s, got, sq.expected(c, s), what)
        built = False
        if c.touches_grid(s):
            built = self.model.request(s.radius, s.kind)
            fig = sq.build_figure(h, s)
            assert (fig > 0) == built and fig >= 0, f"{what}: {s!r} reports build_ms {fig}, the model says {'build' if built else 'hit'}"
            assert h.kernel_ms()[1] == fig, what
            st = h.stats()
            if c.n_fin == 0:
                assert st == dict(finite=0, cells=0, fullest=0, slots=0), (what, st)
            else:
                self.slots = st["slots"] if self.slots is None else self.slots
                assert st["finite"] == c.n_fin and st["slots"] == self.slots and st["slots"] & (st["slots"] - 1) == 0, (what, st)
                assert 1 <= st["cells"] <= c.n_fin and 1 <= st["fullest"] <= c.n_fin, (what, st)
                assert self.grid_stats.setdefault(sq.rkey(s.radius), (st["cells"], st["fullest"])) == (st["cells"], st["fullest"]), (what, st)
        else:
            assert _figures(h) == figures and h.stats() == stats, f"{what}: {s!r} does not reach the grid and changed a figure"
        self.results.append((s, got, built))
        return got, built

    def close(self):
        for al in list(self.aligners.values()):
            al.close()
        self.h.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def check_fresh(cloud, c, s, got, grid_stats=None):
    """step s on a handle (and an aligner) of its own gives the bits the long-lived handle gave"""
    with cloud.Cloud(c.target) as h:
        aligners = {s.args["al"]: sq.open_aligner(cloud, h, c, s.args["al"])} if s.kind in sq.ALIGN_KINDS else {}
        again = sq.run_step(h, aligners, c, s)
        if c.touches_grid(s) and c.n_fin:
            assert sq.build_figure(h, s) > 0
            if grid_stats is not None:
                st = h.stats()
                assert grid_stats[sq.rkey(s.radius)] == (st["cells"], st["fullest"])
    sq.assert_step_same(s, again, got, f"case {c.k}, fresh handle")


@pytest.mark.parametrize("k", range(int(os.environ.get("MPMVS_CLOUD_SEQ_CASES", str(sq.DEFAULT_CASES)))))
def test_random_sequence(cloud, k):
    c = sq.case(k)
    want_builds = sq.replay(c)
    with Runner(cloud, c) as run:
        for i, s in enumerate(c.program):
            _, built = run.step(s)
            if s.kind in sq.KINDS:
                assert built == want_builds[i]["build"]
        assert len(run.results) == len(c.ops) and not run.aligners                        # no step skipped, both aligners closed
        assert run.model.builds == sum(1 for r in want_builds.values() if r["build"])
        grid_using = [(s, got) for s, got, _ in run.results if s.kind != "render"][:3]
        for s, got in grid_using:
            check_fresh(cloud, c, s, got, run.grid_stats)


# ---- named cases ------------------------------------------------------------------------------------------------------------------
def test_eviction_order(cloud):
    """eight radii fill the handle, each through another call (the seven operations that use a grid, and nearest without indices);
    then the least recently used one goes, not the oldest: r0 was touched, so the ninth radius takes r1's place"""
    c = sq.hand_case(1, 300, n_r=10)
    r = c.radii
    program = [Step("open", al=0), Step("open", al=1),
               Step("nearest", r[0], q=0, want_idx=True), Step("knn", r[1], q=1, k=5, want_idx=True), Step("knn_self", r[2], k=17, want_idx=True),
               Step("normals", r[3], k=16, orient=0, want_curvature=True), Step("components", r[4], want_size=True),
               Step("sums", r[5], al=0, T=1), Step("plane_sums", r[6], al=1, T=2), Step("nearest", r[7], q=1, want_idx=False),
               Step("knn", r[0], q=0, k=4, want_idx=True),                      # a hit, on the grid nearest built: r0 is now the most recent
               Step("components", r[8], want_size=True),                         # the ninth radius: a build in r1's buffers
               Step("normals", r[0], k=8, orient=1, want_curvature=True),        # r0 is still there
               Step("sums", r[1], al=0, T=0),                                    # r1 is not: a build, and r2 goes for it
               Step("knn_self", r[2], k=17, want_idx=True),                      # so r2 builds as well, and r3 goes
               Step("plane_sums", r[4], al=1, T=0), Step("nearest", r[8], q=0, want_idx=True),   # r4 .. r8 were never touched by this
               Step("close", al=0), Step("close", al=1)]
    assert all(len(a) > 0 for a in c.queries + c.sources)
    with Runner(cloud, c) as run:
        built = [b for s, b in ((s, run.step(s)[1]) for s in program) if s.kind in sq.KINDS]
        assert built == [True] * 8 + [False, True, False, True, True, False, False]
        assert run.model.lru == [sq.rkey(x) for x in (r[5], r[6], r[7], r[0], r[1], r[2], r[4], r[8])]
        same = [got for s, got, _ in run.results if s.kind == "knn_self"]
        sq.assert_step_same(program[4], same[1], same[0], "r2 rebuilt")


def test_radii_one_ulp_apart(cloud):
    """r = 0.25 and s = the float above it: s * s = 0.0625 + 2^-26 in fp32, more than r * r.  A point at distance s is a neighbour
    under the radius s and none under r, so a grid served under the wrong one of the two keys shows in every answer"""
    f = np.float32
    r = f(0.25)
    s = np.nextafter(r, f(1))
    assert s * s == f(0.0625) + f(2.0 ** -26) and s * s > r * r
    far = [100.0, 0.0, 0.0]
    # the plain pair: the query (s, 0, 0) beside the target (0, 0, 0)
    t1, q1 = np.array([[0, 0, 0], far], f), np.array([[s, 0, 0]], f)
    # the same with the query's mirror image (-s, 0, 0), so that (s, 0, 0) can be a point of the cloud for components
    t2, q2 = np.array([[0, 0, 0], [s, 0, 0], far], f), np.array([[-s, 0, 0]], f)
    for t, q in ((t1, q1), (t2, q2)):
        builds = []
        with cloud.Cloud(t) as h, cloud.Aligner(h, q) as al:
            for turn in range(10):
                for radius, found in ((float(s), True), (float(r), False)):
                    d2, idx = h.nearest(q, radius)
                    builds.append(h.kernel_ms()[1])
                    kd2, kidx, within = h.knn(q, radius, 1, want_within=True)
                    builds.append(h.knn_ms()[1])
                    label, size, counts = h.components(radius)
                    builds.append(h.components_ms()[1])
                    sums, frame = al.sums(radius, I4)
                    builds.append(h.kernel_ms()[1])
                    what = (len(t), turn, radius)
                    assert bits(d2)[0] == (bits(s * s) if found else bits(f(np.inf))) and idx[0] == (0 if found else -1), what
                    assert bits(kd2)[0, 0] == bits(d2)[0] and kidx[0, 0] == idx[0] and within[0] == int(found), what
                    assert sums[0] == int(found), what
                    if len(t) == 3:
                        assert label.tolist() == ([0, 0, 2] if found else [0, 1, 2]) and counts[1] == (2 if found else 3), what
                    else:
                        assert label.tolist() == [0, 1], what
                    c = sq.SeqCase(target=t, queries=[q], sources=[q], transforms=[I4])
                    for step, got in ((Step("nearest", radius, q=0), (d2, idx)), (Step("knn", radius, q=0, k=1), (kd2, kidx, within)),
                                      (Step("components", radius), (label, size, counts)), (Step("sums", radius, al=0, T=0), (sums, frame))):
                        sq.assert_step_same(step, got, sq.expected(c, step), str(what))
        first = [b > 0 for b in builds]
        assert first == [True, False, False, False, True] + [False] * 75, first    # the first use of each radius builds, nothing after it


def test_grid_of_the_neighbouring_radius_would_miss(cloud):
    """cloud_seq_common.border_scene(): 2^18 cells from the grid's corner the cell borders of the radii 0.25 and nextafter(0.25)
    are a float apart, and the target P is filed under another cell in each grid.  Asked at s and then at r, the search at r
    finds P only in a grid built for r: here a grid kept under the wrong one of the two keys changes the answer itself"""
    t, q, r, s, N = sq.border_scene()
    c = sq.SeqCase(target=t, queries=[q], sources=[q], transforms=[I4])
    with cloud.Cloud(t) as h, cloud.Aligner(h, q) as al:
        for turn in range(3):
            for radius in (s, r):
                for step, call, figure in ((Step("nearest", radius, q=0), lambda: h.nearest(q, radius), lambda: h.kernel_ms()[1]),
                                           (Step("knn", radius, q=0, k=1), lambda: h.knn(q, radius, 1, want_within=True), lambda: h.knn_ms()[1]),
                                           (Step("sums", radius, al=0, T=0), lambda: al.sums(radius, I4), lambda: h.kernel_ms()[1])):
                    got = call()
                    sq.assert_step_same(step, got, sq.expected(c, step), f"turn {turn}")
                    assert (figure() > 0) == (turn == 0 and step.kind == "nearest"), (turn, step)
                    assert h.stats()["cells"] == 2
                    if step.kind == "nearest":
                        assert got[1][0] == 1 and got[0][0] <= np.float32(r) * np.float32(r)
                    if step.kind == "sums":
                        assert got[0][0] == 1


def test_aligners_across_eviction(cloud):
    """two aligners on one target, ten radii in turn, twice: with eight grids every pass finds its radius evicted and rebuilds it in
    the buffers of another; the aligners hold no grid of their own, so the sums are those of the statement every time"""
    c = sq.hand_case(2, 257, n_r=10)
    assert all(len(a) > 0 for a in c.sources)
    with Runner(cloud, c) as run:
        run.step(Step("open", al=0))
        run.step(Step("open", al=1))
        rounds = []
        for _ in range(2):
            rounds.append([])
            for i, r in enumerate(c.radii):
                s = Step("plane_sums", r, al=1, T=i % 3) if i % 2 else Step("sums", r, al=0, T=i % 3)
                got, built = run.step(s)
                assert built
                rounds[-1].append((s, got))
        for (s, a), (_, b) in zip(*rounds):
            sq.assert_step_same(s, b, a, "round two")
        assert run.model.evictions == 12 and sum(1 for _, got in rounds[0] if got[0][0] > 0) >= 5
        a0, a1 = run.aligners[0], run.aligners[1]
        run.h.close()                              # the Cloud first: it closes its aligners
        assert a0._h is None and a1._h is None and run.h._h is None
        a0.close()
        a1.close()


def _chain(cloud, c_target, src, T0, radii, **kw):
    """the rounds of align(radii=radii), one call and one fresh Cloud each"""
    T, report = T0, []
    for r in sorted(radii, reverse=True):
        with cloud.Cloud(c_target) as fresh:
            T, rep = cloud.align(src, fresh, T0=T, radii=[r], **kw)
        report += rep
    return T, report


@pytest.mark.parametrize("what", ["distances", "point", "plane"])
def test_cascade_and_rounds_beyond_eight(cloud, what):
    """the project's own callers with ten radii on one handle: cloud.distances (a grid per tolerance) and cloud.align (a grid per
    round); afterwards the first radius is gone from the handle"""
    if what == "distances":
        g = np.arange(30, dtype=np.float64) * 0.01
        gt = np.stack(list(np.meshgrid(g, g, indexing="ij")) + [np.zeros((30, 30))], -1).reshape(-1, 3).astype(np.float32)
        gt = np.concatenate([gt, np.array([[50.0 + i, 50.0, 50.0] for i in range(5)], np.float32)])    # five points nothing is near: every level runs
        rng = np.random.default_rng(4)
        out = (rng.uniform(5, 9, (40, 3)) * rng.choice([-1, 1], (40, 3))).astype(np.float32)
        lift = rng.uniform(0.0005, 0.03, (900, 1)) * np.array([0, 0, 1.0])
        rec = np.concatenate([gt[:900] + lift.astype(np.float32), out]).astype(np.float32)
        tol = [0.02, 0.001, 0.0035, 0.002, 0.0027, 0.005, 0.0075, 0.011, 0.0142, 0.017]
        for qs, ts in ((rec, gt), (gt, rec)):
            levels = []
            with cloud.Cloud(ts) as c_t:
                d = cloud.distances(qs, c_t, tol, on_level=lambda t, n, c: levels.append((t, n, c.kernel_ms()[1])))
                assert [lv[0] for lv in levels] == sorted(tol) and all(lv[2] > 0 for lv in levels) and all(lv[1] > 0 for lv in levels)
                assert levels[-1][1] < levels[0][1]                # the cascade resolved queries on its way
                c_t.nearest(qs[:5], max(tol))
                assert c_t.kernel_ms()[1] == 0                     # the last level's grid is there
                got = c_t.nearest(qs, min(tol))
                assert c_t.kernel_ms()[1] > 0                      # the first level's is not: ten radii went through eight places
            bd2, bidx = brute_nearest(ts, qs, max(tol))
            assert np.array_equal(bits(d), bits(np.sqrt(bd2))) and 0 < np.isinf(d).sum() < len(d)
            assert_same(got, brute_nearest(ts, qs, min(tol)))
        return
    radii = [0.2, 0.16, 0.13, 0.1, 0.08, 0.065, 0.05, 0.04, 0.035, 0.03]
    if what == "point":
        target, src, _, T0 = ac.icp_scene()
        kw = dict(method="point", max_iter=3)
        stated = lambda r, M: cloud.icp_loop(lambda rr, MM: ac.brute_sums(target, src, MM, rr), r, M, True, 3, e(r))
    else:
        target, normals, src, _, T0 = apc.plane_scene()
        kw = dict(method="plane", target_normals=normals, max_iter=3)
        stated = lambda r, M: cloud.plane_icp_loop(lambda rr, MM: apc.plane_sums(target, normals, src, MM, rr), r, M, True, 3, e(r))
    with cloud.Cloud(target) as c_t:
        e = lambda r: float(c_t.frame(r)[3]) * 2.0 ** -20
        T, report = cloud.align(src, c_t, T0=T0, radii=radii, **kw)
        c_t.nearest(src[:5], radii[-1])
        assert c_t.kernel_ms()[1] == 0                             # the last round's grid is there
        got = c_t.nearest(src, radii[0])
        assert c_t.kernel_ms()[1] > 0                              # the first round's was evicted
        M = ac.m34(T0)
        for r, row in zip(radii, report):                          # the statement's loop, round by round
            res = stated(r, M)
            M = res[0]
            assert row["radius"] == r and (row["passes"], row["inliers"]) == res[1:3] and row["rmse"] == res[-1]
            assert what == "point" or row["rmse_plane"] == res[3]
        assert np.array_equal(T[:3], M) and all(row["inliers"] > 100 for row in report)
    assert_same(got, brute_nearest(target, src, radii[0]))
    T2, report2 = _chain(cloud, target, src, T0, radii, **kw)
    assert T.tobytes() == T2.tobytes() and report == report2
    assert not np.array_equal(T, T0)
