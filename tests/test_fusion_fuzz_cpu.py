"""What the fusion sweep of tests/test_fusion_fuzz_gpu.py covers, asserted on the oracle alone (no GPU): the generator of
tests/fusion_fuzz_common.py reaches every slot count, size edge, bad value and flag combination the sweep exists for, few of its
cases are empty, the two orders differ on most of them, the oracle is deterministic on them, and on the cases the reference's
compiled RunFusion can take, oracle mode 1 still writes the reference's file byte for byte."""
import importlib

import numpy as np

import fusion_fuzz_common as fz
import ref_common as rc

CASES = fz.DEFAULT_CASES
_runs = {}


def _oracle_runs(pm, oracle):
    """per case the oracle's (cloud, valid, masks) in snapshot order (mode 0) and in reference order (mode 2); computed once"""
    if not _runs:
        for k in range(CASES):
            c = fz.case(pm, k)
            _runs[k] = (oracle.fuse(*c.args(), sky=c.sky), oracle.fuse(*c.args(), sky=c.sky, reference_order=True))
    return _runs


def test_generator_covers_what_the_sweep_is_for(pm):
    cases = [fz.case(pm, k) for k in range(CASES)]
    slots = {s for c in cases for s in c.slots()}
    assert {1, 2, 6, 7, 17, 32, 33} <= slots and max(slots) == 33, sorted(slots)
    count = lambda pred: sum(1 for c in cases if pred(c))
    seen = {
        "mixed sizes": count(lambda c: len(set(c.sizes)) > 1),
        "a non-estimated source larger than every estimated image": count(lambda c: c.larger_unestimated_source()),
        "colour + sky": count(lambda c: c.colour and c.sky is not None),
        "static criterion": count(lambda c: not c.dynamic),
        "NaN and zero normals": count(lambda c: c.bad_normals),
        "34 or 35 images": count(lambda c: c.n >= 34),
    }
    for name in fz.BAD_DEPTHS:
        seen["depth " + name] = count(lambda c: name in c.bad_depths)
    print(seen)
    assert all(v >= 10 for v in seen.values()), seen
    # the bad values are where the generator says: in the arrays the entry points get
    for c in cases[:20]:
        flat = np.concatenate([d.ravel() for d in c.depths])
        found = {"zero": (flat == 0).any(), "negative": (flat == -1).any(), "nan": np.isnan(flat).any(), "+inf": (flat == np.inf).any(),
                 "-inf": (flat == -np.inf).any(), "denormal": ((flat > 0) & (flat < 1e-38)).any(), "huge": (flat == np.float32(1e30)).any()}
        assert {n for n, f in found.items() if f} == c.bad_depths
    widths, heights = {w for c in cases for w, _ in c.sizes}, {h for c in cases for _, h in c.sizes}
    assert set(fz.SPECIAL_W) <= widths and set(fz.SPECIAL_H) <= heights
    assert all(sum(c.pixels(i) for i in range(c.n)) <= fz.MAX_PIXELS for c in cases)
    # lists are permutations, not ascending runs: slot order and image order differ
    assert count(lambda c: any(s != sorted(s) for s in c.sources)) >= CASES // 2
    assert count(lambda c: c.clean) >= 10


def test_few_cases_are_vacuous_and_both_orders_are_exercised(pm, oracle):
    runs = _oracle_runs(pm, oracle)
    points = np.array([len(runs[k][0][0]) for k in range(CASES)])
    print(f"points per case in snapshot order: none in {int((points == 0).sum())} of {CASES}, fewer than 100 in {int((points < 100).sum())}, "
          f"median {int(np.median(points))}, most {int(points.max())}")
    assert (points < 100).sum() <= 0.10 * CASES
    differ = 0
    for k in range(CASES):
        (c0, _, m0), (c2, _, m2) = runs[k]
        differ += len(c0) != len(c2) or not all(np.array_equal(a, b) for a, b in zip(m0, m2))
    print(f"snapshot and reference order differ in point count or masks in {differ} of {CASES} cases")
    assert differ >= 0.80 * CASES
    # the sweep's bad values reach the outputs: some clouds hold NaN (normals) and non-finite coordinates
    assert sum(1 for k in range(CASES) if np.isnan(runs[k][0][0]).any()) >= 10


def test_oracle_is_deterministic_on_the_cases(pm, oracle):
    runs = _oracle_runs(pm, oracle)
    for k in range(CASES):
        c = fz.case(pm, k)
        cloud, valid, masks = oracle.fuse(*c.args(), sky=c.sky)
        want = runs[k][0]
        assert cloud.tobytes() == want[0].tobytes(), k
        assert all(a.tobytes() == b.tobytes() for a, b in zip(valid, want[1])) and all(a.tobytes() == b.tobytes() for a, b in zip(masks, want[2])), k


def test_literal_mode_writes_the_compiled_references_file(pm, oracle):
    """the byte-for-byte pin of tests/test_reference_host_cpu.py on inputs it has not seen: the first ten clean cases (every image
    estimated, finite depths and normals, B,G,R colours) -- mixed sizes, permuted lists of up to 32 sources, one-row and
    one-pixel images, zero, negative, denormal and huge depths, sky masks, both criteria"""
    fusion = importlib.import_module("mp-mvs_amd.fusion")
    clean = [c for c in (fz.case(pm, k) for k in range(CASES)) if c.clean][:10]
    assert len(clean) == 10
    total = 0
    for c in clean:
        assert all(c.est) and c.colour and all(np.isfinite(d).all() for d in c.depths) and all(np.isfinite(m).all() for m in c.normals)
        fc = rc.FuseCase(f"fuzz_{c.k}", c.cams, c.depths, c.normals, c.cols, c.cols, c.sky, c.sources, c.dynamic)
        _, want = fc.reference()
        got = fc.oracle_records(oracle, fusion, 1)
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), (c.k, len(got), len(want))
        total += len(want)
    print(f"{total} records in the ten clean cases")
    assert total >= 10 * 100        # ten cases at the bar of the vacuity test


def test_cap_case_has_pixels_consistent_with_all_32_sources(pm, oracle):
    """what makes the 33-entry track of tests/test_fusion_fuzz_gpu.py::test_the_cap possible, measured per source: image 0 against
    the list [s, z] with z an image of all-zero depth (the last slot is not visited while nothing is consistent yet, so s must not
    be last), for each of its 32 sources"""
    c = fz.cap_case(pm)
    assert c.slots()[0] == 33 and len(set(c.sizes)) == 2
    z = c.n - 1
    depths = list(c.depths)
    depths[z] = np.zeros_like(depths[z])
    est = [True] + [False] * (c.n - 1)
    every = np.ones(c.depths[0].shape, bool)
    for s in c.sources[0]:
        _, valid, _ = oracle.fuse(c.cams, est, depths, c.normals, c.cols, [[s, z]] + [[]] * (c.n - 1), True)
        every &= valid[0].astype(bool)
    print(f"{int(every.sum())} pixels of image 0 are consistent with each of its 32 sources")
    assert every.sum() >= 1
