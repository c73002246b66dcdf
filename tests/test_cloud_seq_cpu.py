"""What the cloud-handle sweep of tests/test_cloud_seq_gpu.py covers, asserted without a GPU: the generator of
tests/cloud_seq_common.py reaches every operation, the eviction branch, re-requests of evicted radii, hits on grids another
operation built, both radii of a one-ulp pair, align passes on aligners that have seen an eviction, and the edge sizes; the cache
model answers a hand-written sequence and the round-robin that never hits; and every statement of the default cases runs.

The statements of the 24 default cases (995 steps, 916 distinct results after memoisation) take 1.2 s on one CPU core
(test_every_statement_of_the_default_cases_runs prints the figure)."""
import time

import numpy as np

import cloud_seq_common as sq

CASES = sq.DEFAULT_CASES


def _cases():
    return [sq.case(k) for k in range(CASES)]


def test_case_is_a_pure_function_of_k():
    c = sq.case(3)
    sq._cache.pop(3)
    d = sq.case(3)
    assert c is not d and c.attempt == d.attempt
    assert c.target.tobytes() == d.target.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(c.queries + c.sources, d.queries + d.sources))
    assert c.radii == d.radii and [repr(s) for s in c.program] == [repr(s) for s in d.program]


def test_cases_stay_within_their_stated_ranges():
    for c in _cases():
        assert 1 <= len(c.target) <= 400 and all(len(a) <= 300 for a in c.queries + c.sources)
        assert 9 <= len(c.radii) <= 12 and len({sq.rkey(r) for r in c.radii}) == len(c.radii)
        lo, hi = (np.float32(r) for r in c.ulp_pair)
        assert np.nextafter(lo, np.float32(np.inf)) == hi and lo != hi
        assert all(c.extent / r < 2.0 ** 12 for r in c.radii)
        assert 30 <= len(c.ops) <= 50
        assert all(s.radius is None or s.radius in c.radii for s in c.program)
        for s in c.ops:
            if "k" in s.args:
                assert s.args["k"] in sq.KS and (s.kind != "normals" or s.args["k"] >= 2)
        opened, closed = [s.args["al"] for s in c.program if s.kind == "open"], [s.args["al"] for s in c.program if s.kind == "close"]
        assert sorted(opened) == sorted(closed) == [0, 1]
        assert all(int(cam.width) <= 48 and int(cam.height) <= 36 for cam in c.cams)
        assert (c.n_fin == 0) == c.no_finite
        if c.no_finite:
            assert not np.isfinite(c.target).all(1).any()


def test_generator_covers_what_the_sweep_is_for():
    cases = _cases()
    kinds = {k: sum(1 for c in cases for s in c.ops if s.kind == k) for k in sq.KINDS}
    print(kinds)
    assert all(v >= 20 for v in kinds.values()), kinds
    ks = {s.args["k"] for c in cases for s in c.ops if "k" in s.args}
    assert ks == set(sq.KS)
    assert {s.args["orient"] for c in cases for s in c.ops if s.kind == "normals"} == {0, 1, 2}
    assert {s.args["T"] for c in cases for s in c.ops if s.kind in sq.ALIGN_KINDS} == {0, 1, 2}
    open_since = 0
    for c in cases:
        real = list(sq.replay(c).values())
        model = list(sq.replay(c, finite=True).values())          # the program's radius sequence, were the target finite
        assert any(r["evicts"] for r in real) == (not c.no_finite), c.k
        assert not c.no_finite or not any(r["build"] for r in real), c.k
        assert any(r["rerequest"] for r in model), c.k
        assert any(r["hit_on_other_kind"] for r in model), c.k
        used = {sq.rkey(s.radius) for s in c.program if c.touches_grid(s)}
        assert all(sq.rkey(r) in used for r in c.ulp_pair), c.k
        open_since += sum(1 for r in real if r["open_since_eviction"])
        # radii come back both soon and late: some gap between two uses of one radius is at most 3 steps, some at least 12
        seq = [sq.rkey(s.radius) for s in c.ops if s.radius is not None]
        gaps = [j - i for i in range(len(seq)) for j in range(i + 1, len(seq)) if seq[j] == seq[i] and seq[i] not in seq[i + 1:j]]
        assert min(gaps) <= 3 and max(gaps) >= 12, (c.k, sorted(gaps))
    print(f"{open_since} align passes ran on an aligner opened before an eviction")
    assert open_since >= 20
    counts = {len(c.target) for c in cases}
    assert {1, 255, 256, 257} <= counts, sorted(counts)
    assert sum(1 for c in cases if c.offset) >= 3 and sum(1 for c in cases if c.no_finite) >= 2
    assert sum(1 for c in cases if c.offset and not c.no_finite) >= 3
    # the spoiled rows are in the arrays the calls get
    bad_t = sum(1 for c in cases if not c.no_finite and not np.isfinite(c.target).all())
    dup_t = sum(1 for c in cases if len(np.unique(c.target[np.isfinite(c.target).all(1)], axis=0)) < c.n_fin)
    bad_q = sum(1 for c in cases if any(not np.isfinite(a).all() for a in c.queries + c.sources))
    empty = sum(1 for c in cases for s in c.ops if s.kind != "render" and not c.touches_grid(s))
    print(f"targets with non-finite rows in {bad_t} cases, with duplicates in {dup_t}; non-finite queries or sources in {bad_q}; "
          f"{empty} steps without a query or a source")
    assert bad_t >= 8 and dup_t >= 8 and bad_q >= 8 and empty >= 5


def test_model_on_a_hand_written_sequence():
    a, b, c, d, e, f, g, h, i = (0.1 * n for n in range(1, 10))
    m = sq.GridCacheModel()
    got = [m.request(r) for r in (a, b, c, a, d, e, f, g, h, i, a, b)]
    #       a     b     c     a      d     e     f     g     h     i: evicts b  a      b: evicts c
    assert got == [True, True, True, False, True, True, True, True, True, True, False, True]
    assert m.lru == [sq.rkey(r) for r in (d, e, f, g, h, i, a, b)] and m.evicted == [sq.rkey(c)]
    assert (m.builds, m.hits, m.evictions) == (10, 2, 2)
    # the key is the bits of the fp32 radius: one ulp apart is another grid, and a double that rounds to the same float is the same
    m = sq.GridCacheModel()
    r = np.float32(0.25)
    assert m.request(float(r)) and m.request(float(np.nextafter(r, np.float32(1)))) and not m.request(0.25 + 2.0 ** -40)
    assert not m.request(float(r)) and m.builds == 2
    # no finite point: never a build, nothing kept
    m = sq.GridCacheModel(finite=False)
    assert not any(m.request(0.1 * n) for n in range(1, 12)) and m.lru == [] and m.builds == 0


def test_model_round_robin_never_hits():
    m = sq.GridCacheModel()
    assert all(m.request(0.01 * (1 + n % 10)) for n in range(50))
    assert m.hits == 0 and m.evictions == 42 and len(m.lru) == 8
    m = sq.GridCacheModel()
    assert [m.request(0.01 * (1 + n % 8)) for n in range(24)] == [True] * 8 + [False] * 16      # eight fit


def test_border_scene_is_what_a_stale_grid_would_get_wrong():
    """the inputs of test_cloud_seq_gpu.py::test_grid_of_the_neighbouring_radius_would_miss: the statement finds P from Q under both
    radii, P's cell differs between the two grids, and from Q's cell in the grid of r the cell P has in the grid of s is out of reach"""
    t, q, r, s, N = sq.border_scene()
    assert np.float32(s) == np.nextafter(np.float32(r), np.float32(1)) and N >= 1 << 18 and N + 2 < 1 << 21
    for radius in (r, s):
        d2, idx = sq.cc.brute_nearest(t, q, radius)
        assert idx[0] == 1 and d2[0] == (q[0, 0] - t[1, 0]) ** 2 and d2[0] <= np.float32(r) * np.float32(r)
    assert sq.cell(t[1, 0], 0, r) == N and sq.cell(t[1, 0], 0, s) == N - 1
    assert sq.cell(q[0, 0], 0, r) == N + 1 and abs(sq.cell(q[0, 0], 0, r) - sq.cell(t[1, 0], 0, s)) == 2
    assert abs(sq.cell(q[0, 0], 0, s) - sq.cell(t[1, 0], 0, r)) <= 1          # the other way round nothing is lost


def test_every_statement_of_the_default_cases_runs():
    t0 = time.perf_counter()
    steps = distinct = 0
    for c in _cases():
        for s in c.ops:
            want = sq.expected(c, s)
            sq.assert_step_same(s, _as_got(s, want), want)          # the comparison rules accept every expected result as it is
            steps += 1
        distinct += len(c.memo)
    dt = time.perf_counter() - t0
    print(f"{steps} steps, {distinct} distinct results, statements {dt:.1f} s")
    # results are not vacuous: most searches find something, and not everything
    found = [np.isfinite(sq.expected(c, s)[0]).mean() for c in _cases() for s in c.ops if s.kind == "nearest" and c.touches_grid(s) and not c.no_finite]
    assert 0.05 < np.mean(found) < 0.95, np.mean(found)
    pairs = [int(sq.expected(c, s)[0][0]) for c in _cases() for s in c.ops if s.kind in sq.ALIGN_KINDS]
    assert sum(1 for p in pairs if p > 0) >= len(pairs) // 3, pairs
    comps = [int(sq.expected(c, s)[2][1]) for c in _cases() for s in c.ops if s.kind == "components" and not c.no_finite]
    assert sum(1 for n in comps if n > 1) >= len(comps) // 2, comps
    # the pair one ulp apart is no formality: the statements are evaluated at both radii as different keys
    c = sq.case(0)
    assert len({sq.rkey(r) for r in c.ulp_pair}) == 2


def _as_got(s, want):
    """an expected result in the layout the library's call returns"""
    if s.kind == "render":
        return want
    return tuple(want)
