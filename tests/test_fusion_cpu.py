"""Fusion on the CPU oracle: the snapshot formulation the GPU implements
against analytic ground truth and against the reference's literal sequential order."""
import numpy as np
import pytest

from fusion_fuzz_common import analytic_normals


def _scene(pm, noise=0.002, n_grid=(3, 2), size=(96, 72), seed=0):
    sc, neigh = pm.synth.make_grid_scene(size[0], size[1], n_grid[0], n_grid[1], spacing=0.4, rot_deg=1.0, quantize=True)
    rng = np.random.default_rng(seed)
    cams = [v.cam for v in sc.views]
    depths, normals = [], []
    for v in sc.views:
        d = v.gt_depth * (1.0 + noise * rng.standard_normal(v.gt_depth.shape)).astype(np.float32)
        depths.append(d)
        normals.append(analytic_normals(pm, v))
    grays = [v.image for v in sc.views]
    return sc, cams, depths, normals, grays, neigh


def test_snapshot_fusion_reconstructs_the_surface(pm, oracle):
    sc, cams, depths, normals, grays, neigh = _scene(pm)
    cloud, valid, masks = oracle.fuse(cams, [True] * len(cams), depths, normals, grays, neigh)
    assert len(cloud) > 0.5 * depths[0].size
    err = np.abs(cloud[:, 2] - pm.synth.height_field(cloud[:, 0].astype(np.float64), cloud[:, 1].astype(np.float64)))
    assert np.median(err) < 0.01 and (err < 0.05).mean() > 0.99          # world units, surface at z ~ 5
    assert np.allclose(np.linalg.norm(cloud[:, 3:6], axis=1), 1.0, atol=0.02)
    assert cloud[:, 6:].min() >= 0 and cloud[:, 6:].max() <= 255
    # a pixel consumed by an EARLIER image's point is masked and produces no point of its own;
    # checkable on the last image, whose mask can only have been set by earlier images
    assert masks[-1].sum() > 0 and not (valid[-1].astype(bool) & masks[-1].astype(bool)).any()
    # the first image sees empty masks: it fuses every pixel that is consistent with a neighbour
    assert valid[0].mean() > 0.8
    # holes and inconsistent depths produce nothing
    depths2 = [d.copy() for d in depths]
    depths2[0][:, :20] = 0.0
    depths2[0][:, 40:50] *= 1.2
    _, valid2, _ = oracle.fuse(cams, [True] * len(cams), depths2, normals, grays, neigh)
    assert valid2[0][:, :20].sum() == 0 and valid2[0][:, 41:49].mean() < 0.05


def test_estimate_flag_and_static_criterion(pm, oracle):
    sc, cams, depths, normals, grays, neigh = _scene(pm)
    est = [True, False, True, True, True, True]
    cloud, valid, _ = oracle.fuse(cams, est, depths, normals, grays, neigh, use_dynamic=False)   # num_consistent >= 2 (ref :476)
    assert valid[1].sum() == 0 and valid[0].sum() > 0


def test_snapshot_vs_reference_sequential_order(pm, oracle):
    """how far the parallel formulation is from the reference's order-dependent loop: the
    first image is identical up to libm-vs-canonical rounding; over the whole scene the
    point count differs by a few percent (intra-image mask races + the stale used_list)"""
    sc, cams, depths, normals, grays, neigh = _scene(pm)
    c0, v0, m0 = oracle.fuse(cams, [True] * 6, depths, normals, grays, neigh)
    c1, v1, m1 = oracle.fuse(cams, [True] * 6, depths, normals, grays, neigh, sequential_literal=True)
    assert abs(len(c0) - len(c1)) / len(c1) < 0.05
    z0 = np.abs(c0[:, 2] - pm.synth.height_field(c0[:, 0].astype(np.float64), c0[:, 1].astype(np.float64)))
    z1 = np.abs(c1[:, 2] - pm.synth.height_field(c1[:, 0].astype(np.float64), c1[:, 1].astype(np.float64)))
    assert abs(np.median(z0) - np.median(z1)) < 2e-3
    agree = (v0[0] == v1[0]).mean()
    assert agree > 0.97


def _colours_and_sky(grays, seed=3):
    """B,G,R images derived from the grey ones and a sky mask per image (top rows + scattered pixels)"""
    rng = np.random.default_rng(seed)
    cols = [np.stack([g, 255 - g, (g * 0.5 + 20)], -1).round().astype(np.uint8) for g in grays]
    sky = []
    for k, g in enumerate(grays):
        m = np.zeros(g.shape, np.uint8)
        m[: 6 + 2 * k] = 255
        m[rng.random(g.shape) < 0.02] = 1            # any value > 0 counts (reference :385)
        sky.append(m)
    sky[2] = None                                     # an image without a mask
    return cols, sky


def test_colour_and_sky_mask(pm, oracle):
    """colour = mean of the B,G,R values of the consistent pixels (reference :394,:448-450,:466-468); a sky pixel is masked when
    ITS image is fused (:385-388): it produces no point and is no longer available to later images, but earlier images
    may still have used it"""
    sc, cams, depths, normals, grays, neigh = _scene(pm)
    cols, sky = _colours_and_sky(grays)
    cloud_g, valid_g, _ = oracle.fuse(cams, [True] * 6, depths, normals, grays, neigh)
    cloud_c, valid_c, _ = oracle.fuse(cams, [True] * 6, depths, normals, cols, neigh)
    assert all(np.array_equal(a, b) for a, b in zip(valid_g, valid_c)) and np.array_equal(cloud_g[:, :6], cloud_c[:, :6])
    assert np.allclose(cloud_c[:, 6], cloud_g[:, 6], atol=1e-3)                        # channel 0 is the grey image itself
    assert np.allclose(cloud_c[:, 7], 255 - cloud_g[:, 6], atol=1e-2)                  # averaging is linear
    cloud_s, valid_s, masks_s = oracle.fuse(cams, [True] * 6, depths, normals, cols, neigh, sky=sky)
    for k in range(6):
        if sky[k] is None:
            continue
        on = sky[k] > 0
        assert valid_s[k][on].sum() == 0 and masks_s[k][on].all()
    assert np.array_equal(valid_s[0][sky[0] == 0], valid_c[0][sky[0] == 0])            # image 0 sees no mask but its own sky
    assert len(cloud_s) < len(cloud_c)
    # literal sequential order agrees on sky handling
    _, valid_l, masks_l = oracle.fuse(cams, [True] * 6, depths, normals, cols, neigh, sky=sky, sequential_literal=True)
    for k in range(6):
        if sky[k] is not None:
            assert valid_l[k][sky[k] > 0].sum() == 0 and masks_l[k][sky[k] > 0].all()


# Oracle mode 2 (the reference's order in the canonical acos / exp / sqrtf: what the GPU's reference-order mode equals bit for bit)
# against the reference's loop in libm arithmetic -- oracle mode 1 here, the reference's compiled RunFusion itself in
# tests/test_reference_host_cpu.py and tests/test_reference_gpu.py.  Only a threshold decision that falls between a canonical
# function and libm's can differ, and it would cascade through the masks.  Measured on the nine cases of
# tests/ref_common.py::fusion_cases (8 000 to 80 000 points each) against the compiled reference: no point count differs and no
# record differs, in any case.  The bars are twice the worst measured value, relative to the reference's count.
REFERENCE_ORDER_COUNT_BAR = 2 * 0.0        # |M2 - M| / M
REFERENCE_ORDER_RECORDS_BAR = 2 * 0.0      # share of the 27-byte records (here: of the per-pixel decisions) one side has and the other lacks


def test_reference_order_in_canonical_arithmetic(pm, oracle):
    """oracle mode 2 = the reference's sequential order (in-place masks, persistent used_list) in the canonical arithmetic: what
    the GPU's MPMVS_FUSE_REFERENCE_ORDER mode reproduces.  Against the literal (libm) restatement of that loop only isolated
    threshold decisions may flip; against the snapshot formulation the known few-percent deviation shows."""
    sc, cams, depths, normals, grays, neigh = _scene(pm)
    c1, v1, m1 = oracle.fuse(cams, [True] * 6, depths, normals, grays, neigh, sequential_literal=True)
    c2, v2, m2 = oracle.fuse(cams, [True] * 6, depths, normals, grays, neigh, reference_order=True)
    c0, v0, m0 = oracle.fuse(cams, [True] * 6, depths, normals, grays, neigh)
    assert abs(len(c2) - len(c1)) <= REFERENCE_ORDER_COUNT_BAR * len(c1)
    assert np.mean([np.mean(a == b) for a, b in zip(v1, v2)]) >= 1.0 - REFERENCE_ORDER_RECORDS_BAR
    assert len(c0) != len(c2)                      # the two formulations do differ on this scene
    assert np.array_equal(v0[0], v2[0]) is False or np.array_equal(m0[1], m2[1]) is False
