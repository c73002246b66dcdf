"""Fusion on the MI355X (mpmvs_fuse) against the oracle's snapshot formulation: bit exact."""
import importlib

import numpy as np
import pytest

from test_fusion_cpu import _colours_and_sky, _scene

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("use_dynamic", [True, False])
def test_fusion_bit_exact(pm, oracle, engine, use_dynamic):
    fusion = importlib.import_module("mp-mvs_amd.fusion")
    sc, cams, depths, normals, grays, neigh = _scene(pm, size=(128, 96))
    depths[2][10:30, 20:60] = 0.0
    est = [True, True, False, True, True, True]
    cg, vg, mg = fusion.fuse(cams, est, depths, normals, grays, neigh, use_dynamic)
    cc, vc, mc = oracle.fuse(cams, est, depths, normals, grays, neigh, use_dynamic)
    assert len(cg) == len(cc) and len(cg) > 1000
    assert np.array_equal(cg, cc)
    for a, b in zip(vg, vc):
        assert np.array_equal(a, b)
    for a, b in zip(mg, mc):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("use_sky", [False, True])
def test_fusion_colour_and_sky_bit_exact(pm, oracle, engine, use_sky):
    fusion = importlib.import_module("mp-mvs_amd.fusion")
    sc, cams, depths, normals, grays, neigh = _scene(pm, size=(128, 96))
    cols, sky = _colours_and_sky(grays)
    sky = sky if use_sky else None
    cg, vg, mg = fusion.fuse(cams, [True] * 6, depths, normals, cols, neigh, sky=sky)
    cc, vc, mc = oracle.fuse(cams, [True] * 6, depths, normals, cols, neigh, sky=sky)
    assert len(cg) > 1000 and np.array_equal(cg, cc)
    assert all(np.array_equal(a, b) for a, b in zip(vg, vc)) and all(np.array_equal(a, b) for a, b in zip(mg, mc))
    assert np.ptp(cg[:, 6] - cg[:, 7]) > 10        # three distinct channels came through


def test_fusion_of_estimated_maps(pm, oracle, engine):
    """end of the pipeline: depth/normal maps estimated by the HIP path (photometric pass per
    image) fused on the GPU == the same maps fused by the oracle; points lie on the surface"""
    fusion = importlib.import_module("mp-mvs_amd.fusion")
    sc, neigh = pm.synth.make_grid_scene(128, 96, 3, 2, spacing=0.4, rot_deg=1.0, quantize=True)
    cams = [v.cam for v in sc.views]
    imgs = [v.image for v in sc.views]
    depths, normals = [], []
    for i in range(6):
        h = engine.create(0)
        ids = [i] + neigh[i]
        h.set_views([cams[j] for j in ids], [imgs[j] for j in ids])
        dmin, dmax = pm.synth.kernel_depth_range(cams[i])
        h.run(pm.PatchMatchParams(num_images=len(ids), depth_min=float(dmin), depth_max=float(dmax), max_scale=1), 100 + i)
        planes, _ = h.get()
        depths.append(planes[..., 3].copy())
        normals.append(planes[..., :3].copy())
    cg, vg, mg = fusion.fuse(cams, [True] * 6, depths, normals, imgs, neigh)
    cc, vc, mc = oracle.fuse(cams, [True] * 6, depths, normals, imgs, neigh)
    assert np.array_equal(cg, cc) and all(np.array_equal(a, b) for a, b in zip(mg, mc))
    err = np.abs(cg[:, 2] - pm.synth.height_field(cg[:, 0].astype(np.float64), cg[:, 1].astype(np.float64)))
    assert len(cg) > 300 and np.median(err) < 0.05   # 128x96 single-pass estimates: few pixels meet 1 % / 10 degrees


@pytest.mark.parametrize("reference_order", [False, True])
def test_fusion_from_resident_contexts_equals_the_host_array_path(pm, engine, reference_order):
    """mpmvs_fuse_ctx / mpmvs_fuse_ply_ctx read depth and normal maps straight from the PatchMatch contexts that estimated them (no
    19 B per pixel upload; reference flow: Run() -> depths.dmb / normals.dmb -> RunFusion, src/PatchMatch.cpp:610-633 -> :334-336):
    the same points, masks and PLY records, bit for bit, as the host-array entry points on the maps mpmvs_get returns -- with every
    image resident, with a mix of resident and host images, and after a pipelined Run(); a context without a finished Run() is refused."""
    fusion = importlib.import_module("mp-mvs_amd.fusion")
    sc, neigh = pm.synth.make_grid_scene(128, 96, 3, 2, spacing=0.4, rot_deg=1.0, quantize=True)
    cams = [v.cam for v in sc.views]
    imgs = [v.image for v in sc.views]
    cols = [np.stack([np.asarray(g, np.uint8), 255 - np.asarray(g, np.uint8), np.asarray(g, np.uint8) // 2], -1) for g in imgs]
    ctxs, depths, normals = [], [], []
    for i in range(6):
        h = engine.create(0)
        ids = [i] + neigh[i]
        h.set_views([cams[j] for j in ids], [imgs[j] for j in ids])
        dmin, dmax = pm.synth.kernel_depth_range(cams[i])
        prm = pm.PatchMatchParams(num_images=len(ids), depth_min=float(dmin), depth_max=float(dmax), max_scale=1)
        if i % 2:   # every other image through the pipelined Run()
            planes, costs = np.empty((96, 128, 4), np.float32), np.empty((96, 128), np.float32)
            h.run_into_async(prm, 100 + i, planes, costs)
            h.wait()
        else:
            h.run(prm, 100 + i)
            planes, _ = h.get()
        ctxs.append(h)
        depths.append(planes[..., 3].copy())
        normals.append(planes[..., :3].copy())
    est = [True] * 6
    want_pts, want_valid, want_masks = fusion.fuse(cams, est, depths, normals, cols, neigh, reference_order=reference_order)
    want_rec, _ = fusion.fuse_ply(cams, est, depths, normals, cols, neigh, reference_order=reference_order)
    assert len(want_pts) > 300
    none = [None] * 6
    mixed = [c if k in (0, 3, 4) else None for k, c in enumerate(ctxs)]
    for which, cx, dd, nn in (("all resident", ctxs, none, none), ("mixed", mixed, depths, normals)):
        pts, valid, masks = fusion.fuse_ctx(cams, est, cx, dd, nn, cols, neigh, reference_order=reference_order)
        assert np.array_equal(pts, want_pts), which
        assert all(np.array_equal(a, b) for a, b in zip(valid, want_valid)) and all(np.array_equal(a, b) for a, b in zip(masks, want_masks)), which
        rec, masks2 = fusion.fuse_ply(cams, est, dd, nn, cols, neigh, reference_order=reference_order, ctxs=cx)
        assert np.array_equal(rec, want_rec) and all(np.array_equal(a, b) for a, b in zip(masks2, want_masks)), which
    # a context that has not completed a Run() at this size holds no maps to fuse
    fresh = engine.create(0)
    fresh.set_views([cams[j] for j in [0] + neigh[0]], [imgs[j] for j in [0] + neigh[0]])
    with pytest.raises(RuntimeError, match="-2"):
        fusion.fuse_ctx(cams, est, [fresh] + ctxs[1:], none, none, cols, neigh)


@pytest.mark.parametrize("use_sky", [False, True])
def test_fuse_ply_records_equal_uncompacted_path(pm, oracle, engine, use_sky, size=(131, 97)):
    """mpmvs_fuse_ply (device-side compaction into PLY vertex records) == the records built from mpmvs_fuse's per-pixel
    outputs == those built from the oracle's cloud, in the reference's PointCloud order; sizes that are not block multiples"""
    fusion = importlib.import_module("mp-mvs_amd.fusion")
    sc, cams, depths, normals, grays, neigh = _scene(pm, size=size)
    cols, sky = _colours_and_sky(grays)
    depths[1][5:9, 7:40] = np.inf                      # non-finite coordinates are written as 0 (reference :176-179)
    est = [True, True, False, True, True, True]
    sky = sky if use_sky else None
    rec, masks = fusion.fuse_ply(cams, est, depths, normals, cols, neigh, sky=sky)
    cloud, _, masks2 = fusion.fuse(cams, est, depths, normals, cols, neigh, sky=sky)
    cloud_o, _, _ = oracle.fuse(cams, est, depths, normals, cols, neigh, sky=sky)
    assert rec.shape == (len(cloud), 27) and len(cloud) > 1000
    assert np.array_equal(rec, fusion.ply_records(cloud)) and np.array_equal(rec, fusion.ply_records(cloud_o))
    assert all(np.array_equal(a, b) for a, b in zip(masks, masks2))
    rec0, _ = fusion.fuse_ply(cams, [False] * 6, depths, normals, cols, neigh)
    assert rec0.shape == (0, 27)


# 257 x 256 = 65 792 pixels = 257 blocks of 256: one block of block totals into the second round of the totals scan
# (pm_scan.hpp), for the compaction's sum and below for the used_list's "last valid"
def test_fuse_ply_records_above_65536_pixels(pm, oracle, engine):
    test_fuse_ply_records_equal_uncompacted_path(pm, oracle, engine, False, size=(257, 256))


def test_fusion_rejects_view_ids_that_do_not_exist(pm, engine):
    """a malformed pair.txt can name an image past the last one: mpmvs_fuse must refuse it (rc -2) before it indexes anything"""
    fusion = importlib.import_module("mp-mvs_amd.fusion")
    sc, cams, depths, normals, grays, neigh = _scene(pm, size=(64, 48))
    for bad in (6, -1, 1 << 20):
        broken = [list(s) for s in neigh]
        broken[3][1] = bad
        with pytest.raises(RuntimeError, match=r"\(-2\)"):
            fusion.fuse(cams, [True] * 6, depths, normals, grays, broken)
    cg, _, _ = fusion.fuse(cams, [True] * 6, depths, normals, grays, neigh)   # and the device is still usable afterwards
    assert len(cg) > 100


@pytest.mark.parametrize("variant", ["dynamic", "static", "colour+sky"])
def test_reference_order_fusion_bit_exact(pm, oracle, engine, variant, size=(160, 120)):
    """MPMVS_FUSE_REFERENCE_ORDER: the reference's order-dependent result (pixel-by-pixel in-place masks and the used_list that
    is never reset, ref src/PatchMatch.cpp:382,416,470-495) computed on the GPU as a parallel fixpoint == the sequential loop of
    the oracle (mode 2), bit for bit"""
    fusion = importlib.import_module("mp-mvs_amd.fusion")
    sc, cams, depths, normals, grays, neigh = _scene(pm, size=size)
    depths[2][10:30, 20:60] = 0.0
    cols, sky = grays, None
    if variant == "colour+sky":
        cols, sky = _colours_and_sky(grays)
    dyn = variant != "static"
    est = [True, True, False, True, True, True]
    cg, vg, mg = fusion.fuse(cams, est, depths, normals, cols, neigh, dyn, sky=sky, reference_order=True)
    total, worst = fusion.fuse_passes()
    cc, vc, mc = oracle.fuse(cams, est, depths, normals, cols, neigh, dyn, sky=sky, reference_order=True)
    assert len(cg) == len(cc) and len(cg) > 1000
    assert np.array_equal(cg, cc)
    assert all(np.array_equal(a, b) for a, b in zip(vg, vc)) and all(np.array_equal(a, b) for a, b in zip(mg, mc))
    assert 5 <= total and 2 <= worst <= 200          # a fixpoint needs at least a confirming pass per image; chains stay short
    print(f"reference-order fusion, {variant}: {total} passes over 5 images, at most {worst} for one image")
    # and it is NOT the snapshot result (otherwise this test would prove nothing)
    cs, vs, ms = fusion.fuse(cams, est, depths, normals, cols, neigh, dyn, sky=sky)
    assert len(cs) != len(cg) or not all(np.array_equal(a, b) for a, b in zip(ms, mg))
    # records path (device-side compaction) gives the same points
    rec, _ = fusion.fuse_ply(cams, est, depths, normals, cols, neigh, dyn, sky=sky, reference_order=True)
    assert np.array_equal(rec, fusion.ply_records(cg))


def test_reference_order_fusion_above_65536_pixels(pm, oracle, engine):
    test_reference_order_fusion_bit_exact(pm, oracle, engine, "dynamic", size=(257, 256))
