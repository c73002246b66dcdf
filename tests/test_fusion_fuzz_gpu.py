"""Seeded randomized parity sweep of the depth-map fusion on the MI355X: every entry point (mpmvs_fuse, mpmvs_fuse_ply,
mpmvs_fuse_ply_tracks) in both orders against the oracle, on the cases of tests/fusion_fuzz_common.py -- mixed image sizes, view
lists of 1 to 33 slots in random order, sizes at the edges of k_fuse's tile, non-finite and denormal depths, NaN and zero
normals, estimate flags, sky masks, both criteria; tests/test_fusion_fuzz_cpu.py asserts that the cases cover this.  Below the
sweep, named cases: the 33-slot cap, lists the library rejects, duplicate sources, resident contexts of two sizes.

Comparison rule (fusion_fuzz_common.same_bits): equal bits wherever the oracle's value is not NaN, NaN wherever it is.

MPMVS_FUSE_FUZZ_CASES=N widens or narrows the sweep (default 150).  The whole file on the MI355X, 150 cases and the four named
tests: 7.8 s (1.4 s of it the first library load), no case above 0.3 s."""
import importlib
import os

import numpy as np
import pytest

import fusion_fuzz_common as fz
import ref_common as rc
from test_fusion_cpu import _scene
from test_fusion_tracks_gpu import check_track_structure, points_from_tracks

pytestmark = pytest.mark.gpu


def _equal_lists(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def check_case(oracle, c, min_points=0):
    """every entry point in both orders on one case; returns per order what fuse_ply_tracks and fuse gave"""
    fusion = importlib.import_module("mp-mvs_amd.fusion")
    out = {}
    for ref in (False, True):
        kw = dict(sky=c.sky, reference_order=ref)
        want = oracle.fuse(*c.args(), **kw)
        cloud, valid, masks = fusion.fuse(*c.args(), **kw)
        assert len(want[0]) >= min_points
        assert fz.same_bits(cloud, want[0]), (c.k, ref, len(cloud), len(want[0]))
        assert _equal_lists(valid, want[1]) and _equal_lists(masks, want[2]), (c.k, ref)
        rec, masks_ply = fusion.fuse_ply(*c.args(), **kw)
        assert fz.same_records(rec, fusion.ply_records(cloud)) and _equal_lists(masks_ply, masks), (c.k, ref)
        trec, off, img, pix, masks_tr = fusion.fuse_ply_tracks(*c.args(), **kw)
        assert fz.same_records(trec, rec) and _equal_lists(masks_tr, masks), (c.k, ref)
        r = dict(cams=c.cams, depths=c.depths, normals=c.normals, cols=[fusion._as_u8(x) for x in c.cols], neigh=c.sources, sky=c.sky, dyn=c.dynamic,
                 rec=trec, off=off, img=img, pix=pix, valid=valid, cloud=cloud)
        check_track_structure(r)
        with np.errstate(all="ignore"):        # infinite depths: inf - inf in the restated backprojection, as on the device
            again = points_from_tracks(r)
        assert fz.same_bits(again, cloud), (c.k, ref)     # the defining property: the track alone reproduces all nine floats
        out[ref] = r
    return out


@pytest.mark.parametrize("k", range(int(os.environ.get("MPMVS_FUSE_FUZZ_CASES", str(fz.DEFAULT_CASES)))))
def test_random_case(pm, oracle, engine, k):
    check_case(oracle, fz.case(pm, k))


# ---- named cases ------------------------------------------------------------------------------------------------------------------
def _entry_points(fusion, c, **kw):
    """the five entry points as calls that raise RuntimeError("... (-2)") on a refusal"""
    none = [None] * c.n
    a = c.args()
    return {
        "mpmvs_fuse": lambda: fusion.fuse(*a, sky=c.sky, **kw),
        "mpmvs_fuse_ply": lambda: fusion.fuse_ply(*a, sky=c.sky, **kw),
        "mpmvs_fuse_ctx": lambda: fusion.fuse_ctx(a[0], a[1], none, *a[2:], sky=c.sky, **kw),
        "mpmvs_fuse_ply_ctx": lambda: fusion.fuse_ply(*a, sky=c.sky, ctxs=none, **kw),
        "mpmvs_fuse_ply_tracks": lambda: fusion.fuse_ply_tracks(*a, sky=c.sky, **kw),
    }


def _refused_everywhere(fusion, c, **kw):
    for ref in (False, True):
        for name, call in _entry_points(fusion, c, reference_order=ref, **kw).items():
            with pytest.raises(RuntimeError, match=r"\(-2\)"):
                call()


def test_the_cap(pm, oracle, engine):
    """33 slots: slot 32 is bit 31 of the track's slot word.  At least one point of image 0 was averaged from all 32 sources, and
    its track reproduces it; one slot more is refused by every entry point"""
    fusion = importlib.import_module("mp-mvs_amd.fusion")
    c = fz.cap_case(pm)
    out = check_case(oracle, c, min_points=1000)
    for ref in (False, True):
        r = out[ref]
        length = np.diff(r["off"])
        full = np.flatnonzero((r["img"][r["off"][:-1]] == 0) & (length == 33))
        print(f"{'reference' if ref else 'snapshot'} order: {len(full)} points of image 0 have a 33-entry track")
        assert len(full) >= 1
        p = int(full[0])
        entries = r["img"][r["off"][p]:r["off"][p + 1]]
        assert entries.tolist() == [0] + c.sources[0]
        assert fz.same_bits(points_from_tracks(r)[p], r["cloud"][p])
    over = fz.FuzzCase(**{**c.__dict__, "sources": [list(range(1, 34))] + c.sources[1:]})
    assert over.slots()[0] == 34
    _refused_everywhere(fusion, over)
    assert len(fusion.fuse_ply(*c.args())[0]) == len(out[False]["rec"])           # and the device is still usable


def _six(pm):
    sc, cams, depths, normals, grays, neigh = _scene(pm, size=(64, 48))
    g8 = [np.clip(np.rint(g), 0, 255).astype(np.uint8) for g in grays]
    return fz.FuzzCase(k="64x48", cams=cams, est=[True] * 6, depths=depths, normals=normals, cols=g8, sky=None, sources=neigh, dynamic=True,
                       sizes=[(64, 48)] * 6)


def test_short_lists(pm, oracle, engine):
    """an estimated image with an empty list and a list that does not start with its image are refused (-2) before anything is
    launched, by the library and by the oracle; a list of the image alone is legal and gives no point"""
    fusion = importlib.import_module("mp-mvs_amd.fusion")
    c = _six(pm)
    whole = [[i] + list(s) for i, s in enumerate(c.sources)]
    empty = whole[:2] + [[]] + whole[3:]
    headless = whole[:2] + [list(c.sources[2])] + whole[3:]
    for lists in (empty, headless):
        _refused_everywhere(fusion, c, lists=lists)
        for mode in (dict(), dict(reference_order=True), dict(sequential_literal=True)):
            with pytest.raises(RuntimeError, match=r"\(-2\)"):
                oracle.fuse(*c.args(), lists=lists, **mode)
    # an image that is not estimated may come without a list
    resting = fz.FuzzCase(**{**c.__dict__, "est": [True, True, False, True, True, True]})
    want = oracle.fuse(*resting.args(), lists=empty)
    got = fusion.fuse(*resting.args(), lists=empty)
    assert len(want[0]) > 100 and fz.same_result(got, want)
    # the image alone: no point of its own, and everything else as the oracle has it
    alone = fz.FuzzCase(**{**c.__dict__, "sources": c.sources[:2] + [[]] + c.sources[3:]})
    out = check_case(oracle, alone, min_points=100)
    for ref in (False, True):
        assert out[ref]["valid"][2].sum() == 0 and (out[ref]["img"][out[ref]["off"][:-1]] != 2).all()


def test_duplicate_sources_are_refused(pm, engine):
    """96x72_32_sources of ref_common names every source six times: legal for the reference's sequential loop, refused here"""
    fusion = importlib.import_module("mp-mvs_amd.fusion")
    cases = rc.fusion_cases(pm)
    case = cases["96x72_32_sources"]
    est = [True] * case.n
    with pytest.raises(RuntimeError, match=r"\(-2\)"):
        fusion.fuse_ply(case.cams, est, case.depths, case.normals, case.ours, case.sources, case.dynamic)
    good = cases["96x72_dynamic"]
    rec, _ = fusion.fuse_ply(good.cams, est, good.depths, good.normals, good.ours, good.sources, good.dynamic)
    assert len(rec) > 1000


def test_resident_contexts_of_two_sizes(pm, engine):
    """mpmvs_fuse_ctx / mpmvs_fuse_ply_ctx over six contexts, three at 64 x 48 and three at 48 x 36, equal the host-array entry
    points on the maps get() returns, in both orders; a context of another size than its camera is refused"""
    fusion = importlib.import_module("mp-mvs_amd.fusion")
    sizes = [(64, 48), (48, 36)]
    scenes = {}
    for size in sizes:
        scenes[size], neigh = pm.synth.make_grid_scene(size[0], size[1], 3, 2, spacing=0.4, rot_deg=1.0, quantize=True)
    mine = [sizes[i % 2] for i in range(6)]
    cams = [scenes[mine[i]].views[i].cam for i in range(6)]
    imgs = [scenes[mine[i]].views[i].image for i in range(6)]
    ctxs, depths, normals = [], [], []
    for i in range(6):
        sc = scenes[mine[i]]            # the Run() of image i sees its sources at its own size
        h = engine.create(0)
        ids = [i] + neigh[i]
        h.set_views([sc.views[j].cam for j in ids], [sc.views[j].image for j in ids])
        dmin, dmax = pm.synth.kernel_depth_range(cams[i])
        h.run(pm.PatchMatchParams(num_images=len(ids), depth_min=float(dmin), depth_max=float(dmax), max_scale=1), 100 + i)
        planes, _ = h.get()
        assert planes.shape == (mine[i][1], mine[i][0], 4)
        ctxs.append(h)
        depths.append(planes[..., 3].copy())
        normals.append(planes[..., :3].copy())
    est, none = [True] * 6, [None] * 6
    for ref in (False, True):
        want = fusion.fuse(cams, est, depths, normals, imgs, neigh, reference_order=ref)
        want_rec, _ = fusion.fuse_ply(cams, est, depths, normals, imgs, neigh, reference_order=ref)
        print(f"{'reference' if ref else 'snapshot'} order: {len(want[0])} points from single-pass maps of two sizes")
        assert len(want[0]) > 50          # the oracle's Run(), bit-identical to the kernels, gives 64 and 61 points on these maps
        got = fusion.fuse_ctx(cams, est, ctxs, none, none, imgs, neigh, reference_order=ref)
        assert fz.same_result(got, want)
        rec, masks = fusion.fuse_ply(cams, est, none, none, imgs, neigh, reference_order=ref, ctxs=ctxs)
        assert fz.same_records(rec, want_rec) and _equal_lists(masks, want[2])
    swapped = [ctxs[1], ctxs[0]] + ctxs[2:]                  # image 0 (64 x 48) behind a 48 x 36 context
    with pytest.raises(RuntimeError, match=r"\(-2\)"):
        fusion.fuse_ctx(cams, est, swapped, none, none, imgs, neigh)
    with pytest.raises(RuntimeError, match=r"\(-2\)"):
        fusion.fuse_ply(cams, est, none, none, imgs, neigh, ctxs=swapped)
