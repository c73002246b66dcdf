"""The sky-segmentation engine (mpmvs_skyseg_*) on the MI355X against the float64 checker of skyseg_common.

Accuracy criterion, the same for every net: per blob e = max|x - x64| / max|x64| over every element of every blob; the control
A = the largest e of torch-CPU float32 against float64 on the same net and input; asserted: e_hip <= 8 * A for every blob, and on
the final output max|p - p64| <= 8 x the float32 checker's.  (Both sides are fp32 sums of up to 1152 products in different orders;
8 is the margin over a maximum of ~1e7 elements, a missed tap or a half-precision input lands at >= 1000 * A.)"""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import skyseg_common as sc

pytestmark = pytest.mark.gpu

MARGIN = 8.0


def _check(engine, tmp_path, graph, out, x, seed, fmt="fp16", stem="net"):
    """loads the net, runs it in keep mode, compares every blob; returns the reusing-mode output"""
    import torch
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    layers = graph.emit()
    pp, bp = sc.write_pair(tmp_path, layers, seed=seed, fmt=fmt, stem=stem)
    b64 = sc.evaluate(pp, bp, x, torch.float64)
    b32 = sc.evaluate(pp, bp, x, torch.float32)
    e32 = sc.blob_errors(b32, b64)
    A = max(e32.values())  # over all blobs of the file
    h, w = x.shape[1:]
    net = engine.SkySeg(pp, bp, h, w, out)
    try:
        plain = net.run(x)
        net.set_keep(True)
        kept = net.run(x)
        assert np.array_equal(plain, kept), "keep mode and reuse mode differ"
        live = sc.live_blobs(layers, out)
        got = {}
        for name in b64:  # every blob of the file: only the outputs of layers dropped at load (nothing depends on them) may be refused
            try:
                got[name] = net.blob(name)
            except engine.SkySegError as e:
                assert e.code == -34 and name not in live, (name, e.code)
        assert live <= set(got)
        b64 = {k: v for k, v in b64.items() if k in got}
        assert np.array_equal(got[out], kept)
        eh = sc.blob_errors(got, b64)
        worst = max(eh, key=lambda k: eh[k])
        out_hip = float(np.abs(kept.astype(np.float64) - b64[out]).max())
        out_32 = float(np.abs(b32[out].astype(np.float64) - b64[out]).max())
        print(f"skyseg accuracy {stem} seed {seed}: A = {A:.3e}, worst blob {worst} e = {eh[worst]:.3e} ({eh[worst] / max(A, 1e-300):.2f} A); "
              f"output |p - p64| hip {out_hip:.3e} vs fp32 {out_32:.3e} ({out_hip / max(out_32, 1e-300):.2f} x); {len(b64)} blobs, {net.launches} launches, "
              f"{net.ms()[0]:.3f} ms")
        bad = {k: v for k, v in eh.items() if v > MARGIN * A}
        assert not bad, f"blobs beyond {MARGIN} A = {MARGIN * A:.3e}: {sorted(bad.items(), key=lambda kv: -kv[1])[:5]}"
        assert out_hip <= MARGIN * out_32, (out_hip, out_32)
        net.set_keep(False)
        again = net.run(x)
        assert np.array_equal(again, plain), "two runs differ"
        return plain
    finally:
        net.close()


@pytest.mark.parametrize("cin", [3, 6, 16, 32, 64, 128])
@pytest.mark.parametrize("size", [(37, 53), (12, 12)])
def test_convolutions_every_dilation_and_width(engine, tmp_path, cin, size):
    """dilation 1 2 4 8 x outputs 64 16 1 on cin channels, Concat of three runs with an odd total, add, the 1x1 sigmoid layer"""
    g, out = sc.net_convs(cin, *size)
    _check(engine, tmp_path, g, out, sc.noise_image(cin, *size, seed=cin), seed=cin, fmt="mixed", stem=f"convs{cin}")


@pytest.mark.parametrize("cin,couts", [(3, (64, 16, 1)), (128, (64, 1)), (32, (64, 16))])
def test_convolutions_at_full_size(engine, tmp_path, cin, couts):
    g, out = sc.net_convs(cin, 384, 384, dils=(1, 2), couts=couts)
    _check(engine, tmp_path, g, out, sc.smooth_image(cin, 384, 384, seed=1), seed=100 + cin, stem=f"full{cin}")


@pytest.mark.parametrize("size", [(37, 53), (12, 12), (64, 33), (5, 1)])
def test_pool_interp_add_concat(engine, tmp_path, size):
    """ceil-mode pooling on odd sizes down to 1 x 1, Interp from 1-pixel inputs and by non-integer ratios, add, Concat of 2 and 6"""
    g, out = sc.net_ops(*size)
    _check(engine, tmp_path, g, out, sc.noise_image(3, *size, seed=5), seed=7, fmt="mixed", stem="ops")


def test_one_pixel_wide_input_and_live_sigmoid(engine, tmp_path):
    g, out = sc.net_thin()
    _check(engine, tmp_path, g, out, sc.noise_image(3, 9, 1, seed=2), seed=3, fmt="fp32", stem="thin")


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("kind", ["smooth", "noise"])
def test_full_topology_synthetic_weights(engine, tmp_path, seed, kind):
    """U^2-Net-small as the real .param lists it (test_skyseg_cpu ties the builder to the file), seeded weights, 384 x 384, all blobs"""
    g, out = sc.u2net_small()
    x = sc.smooth_image(3, 384, 384, seed) if kind == "smooth" else sc.noise_image(3, 384, 384, seed)
    p = _check(engine, tmp_path, g, out, x, seed=seed, stem=f"u2net_{kind}")
    assert p.shape == (1, 384, 384) and 0.0 <= p.min() and p.max() <= 1.0


def test_two_nets_alternating_equal_their_solo_results(engine, tmp_path):
    ga, oa = sc.net_convs(16, 37, 53)
    gb, ob = sc.net_ops(37, 53)
    pa = sc.write_pair(tmp_path, ga.emit(), seed=1, stem="a")
    pb = sc.write_pair(tmp_path, gb.emit(), seed=2, stem="b")
    xa, xb = sc.noise_image(16, 37, 53, 1), sc.noise_image(3, 37, 53, 2)
    na = engine.SkySeg(*pa, 37, 53, oa)
    solo_a = na.run(xa)
    na.close()
    nb = engine.SkySeg(*pb, 37, 53, ob)
    solo_b = nb.run(xb)
    nb.close()
    na, nb = engine.SkySeg(*pa, 37, 53, oa), engine.SkySeg(*pb, 37, 53, ob)
    for _ in range(3):
        assert np.array_equal(na.run(xa), solo_a)
        assert np.array_equal(nb.run(xb), solo_b)
    na.close()
    nb.close()


@pytest.mark.parametrize("size", [(384, 384), (1200, 1600), (4032, 6048), (1203, 1601)])
def test_run_u8_is_preprocessing_then_run(engine, tmp_path, size):
    """run_u8 == the numpy restatement of pyrDown loop / resize / normalise followed by run, bit for bit"""
    h, w = size
    g, out = sc.net_convs(3, 384, 384, dils=(1,), couts=(16, 1))
    pp, bp = sc.write_pair(tmp_path, g.emit(), seed=4)
    rs = np.random.RandomState(h)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([(xx * 255 // max(w - 1, 1)), (yy * 255 // max(h - 1, 1)), ((xx + yy) % 256)], -1).astype(np.int32)
    img = np.clip(img + rs.randint(-20, 21, img.shape), 0, 255).astype(np.uint8)
    net = engine.SkySeg(pp, bp, 384, 384, out)
    want_in = sc.preprocess_u8(img)
    assert np.array_equal(net.preprocess_u8(img), want_in)
    got = net.run_u8(img)
    assert np.array_equal(got, net.run(want_in))
    padded = np.zeros((h, w + 5, 3), np.uint8)  # a row pitch larger than the row
    padded[:, :w] = img
    assert np.array_equal(net.run_u8(padded[:, :w]), got)
    net.close()


def _u8(a):
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def test_generate_sky_masks_equals_the_composition_by_hand(pm, engine, tmp_path):
    """GenerateSkyRegionMask over a folder of colour JPEGs (one above 768 x 768: the pyrDown loop; one above the image-size cap)
    == run_u8 -> ResizeLinear -> mpmvs_sky_bilateral composed here through the C ABI, bit for bit, for both files of every image"""
    hostlib = importlib.import_module("mp-mvs_amd.hostlib")
    fusion = importlib.import_module("mp-mvs_amd.fusion")
    scene, neigh = pm.synth.make_grid_scene(96, 72, 3, 1, spacing=0.4, quantize=True)
    cams = [v.cam for v in scene.views]
    sizes = [(72, 96), (150, 200), (780, 800)]
    cols = []
    for k, (h, w) in enumerate(sizes):
        yy, xx = np.mgrid[0:h, 0:w]
        r = 128 + 120 * np.sin(xx / (7.0 + 3 * k)) * np.cos(yy / 11.0) + 60 * (yy < h / 3)
        cols.append(_u8(np.stack([r, 255 - r / 2, 40 + (xx + yy) % 160], -1)))   # R,G,B for the files
    hostlib.write_dataset(str(tmp_path), cams, cols, neigh, fmt="jpg", jpeg_options=dict(quality=95, subsampling=2))
    model = tmp_path / "model"
    pp, bp = sc.write_brightness_model(model)
    cap = 600
    assert hostlib.generate_sky_masks(tmp_path, model, max_image_size=cap) == 3
    net = engine.SkySeg(pp, bp, 384, 384, "1959")
    fractions = []
    for i, (h, w) in enumerate(sizes):
        bgr = hostlib.read_image(tmp_path / "images" / f"{i:08d}.jpg", 3)
        assert bgr.shape == (h, w, 3)
        prob = net.run_u8(bgr)[0]
        if h > cap or w > cap:   # reference src/PatchMatch.cpp:24-32
            f = min(np.float32(cap) / np.float32(w), np.float32(cap) / np.float32(h))
            w2, h2 = int(round(float(np.float32(w) * f))), int(round(float(np.float32(h) * f)))
            bgr = np.stack([_u8(hostlib.resize_linear(bgr[..., c].astype(np.float32), w2, h2)) for c in range(3)], -1)
        else:
            w2, h2 = w, h
        mask = hostlib.resize_linear(prob, w2, h2)
        refined = fusion.sky_bilateral(bgr, mask)
        d = tmp_path / "MPMVS" / f"2333_{i:08d}"
        coarse_file, refine_file = hostlib.read_image(d / "skymask.pgm", 1), hostlib.read_image(d / "skymask_refine.pgm", 1)
        assert coarse_file.shape == (h2, w2)
        assert np.array_equal(coarse_file, _u8(np.float32(255) * mask))
        assert np.array_equal(refine_file, np.where(refined > 0, 255, 0).astype(np.uint8))
        fractions.append(float((refine_file > 0).mean()))
    print("sky fractions of the refined masks:", fractions)
    assert all(0.02 < f < 0.98 for f in fractions), fractions   # the stand-in model follows the image: both classes occur
    net.close()
    with pytest.raises(RuntimeError):
        hostlib.generate_sky_masks(tmp_path, tmp_path / "no_model_here")


def test_main_flow_generates_the_masks_with_sky_model(pm, engine, tmp_path):
    """tools/mpmvs_main.py --sky-model: `Sky segment: 1` with no mask brought from outside -> masks by the network, PLY with the
    masks in use"""
    import json
    import subprocess
    import sys
    hostlib = importlib.import_module("mp-mvs_amd.hostlib")
    scene, neigh = pm.synth.make_grid_scene(160, 120, 3, 2, spacing=0.4, rot_deg=1.0, quantize=True)
    cams = [v.cam for v in scene.views]
    cols = [np.stack([g, 255 - g, g // 2 + 20], -1).astype(np.uint8) for g in (np.asarray(v.image).astype(np.uint8) for v in scene.views)]
    hostlib.write_dataset(str(tmp_path), cams, cols, neigh, fmt="jpg", jpeg_options=dict(quality=97, subsampling=0))
    model = tmp_path / "model"
    sc.write_brightness_model(model)
    cfg = tmp_path / "config.yaml"
    cfg.write_text(f'%YAML:1.0\n---\nInput-folder: "{tmp_path}"\nOutput-folder: "{tmp_path}"\nGeometric consistency iterations: 1\nPlaner prior: 1\n'
                   'Geometric consistency planer prior: 0\nSky segment: 1\nUse dynamic_consistency to fuse: 1\n'
                   'Max source images num: 20\nMax image size: 3200\n')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "mpmvs_main.py"), "--config", str(cfg), "--seed", "7", "--sky-model", str(model)],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    assert rep["sky_masks"] == 6 and rep["fused_points"] > 500
    body = open(rep["ply"], "rb").read().split(b"end_header\n", 1)[1]
    assert len(body) == rep["fused_points"] * 27
    sky_pixels = 0
    for i in range(6):
        d = tmp_path / "MPMVS" / f"2333_{i:08d}"
        assert (d / "skymask.pgm").exists() and (d / "depths.dmb").exists()
        sky_pixels += int((hostlib.read_image(d / "skymask_refine.pgm", 1) > 0).sum())
    assert sky_pixels > 0
    # the masks are in use: fusing the same maps without them gives more points, with them the same count again
    assert hostlib.fuse_folder(tmp_path, sky_seg=True) == rep["fused_points"] < hostlib.fuse_folder(tmp_path, sky_seg=False)


def test_argument_errors_and_failed_loads_leave_nothing_behind(engine, tmp_path):
    import torch
    g, out = sc.net_convs(3, 12, 12, dils=(1,), couts=(16,))
    layers = g.emit()
    pp, bp = sc.write_pair(tmp_path, layers, seed=1)
    net = engine.SkySeg(pp, bp, 12, 12, out)
    with pytest.raises(engine.SkySegError) as e:
        net.run(np.zeros((3, 12, 13), np.float32))
    assert e.value.code == -2
    with pytest.raises(engine.SkySegError) as e:
        net.run_u8(np.zeros((8, 8), np.uint8))
    assert e.value.code == -2
    net.run(np.zeros((3, 12, 12), np.float32))
    with pytest.raises(engine.SkySegError) as e:
        net.blob(out)  # no keep mode
    assert e.value.code == -33
    net.set_keep(True)
    with pytest.raises(engine.SkySegError) as e:
        net.blob(out)  # keep mode, but no run since
    assert e.value.code == -33
    net.run(np.zeros((3, 12, 12), np.float32))
    assert net.blob(out).shape == (1, 12, 12)
    with pytest.raises(engine.SkySegError) as e:
        net.blob("no_such_blob")
    assert e.value.code == -34 and "no_such_blob" in e.value.text
    net.close()
    with pytest.raises(engine.SkySegError) as e:
        engine.SkySeg(pp, bp, 12, 12, out, device=99)
    assert e.value.code == -100
    # a .bin cut short after the graph was accepted: twenty failing loads, free memory must not keep falling
    big, bout = sc.net_convs(64, 96, 96)
    bp_, bb_ = sc.write_pair(tmp_path, big.emit(), seed=2, stem="big")
    raw = open(bb_, "rb").read()
    open(bb_, "wb").write(raw[: len(raw) - 100])
    free = []
    for i in range(20):
        with pytest.raises(engine.SkySegError) as e:
            engine.SkySeg(bp_, bb_, 96, 96, bout)
        assert e.value.code == -29
        free.append(torch.cuda.mem_get_info(0)[0])
    assert free[-1] >= free[1], free  # the first failure may park buffers in the pool once; after that nothing moves


def test_real_weights_on_the_probe_image(engine, tmp_path):
    """with MPMVS_SKY_MODEL naming the directory of the real pair: the same criterion on the real weights"""
    d = os.environ.get("MPMVS_SKY_MODEL")
    if not d:
        pytest.skip("MPMVS_SKY_MODEL is not set")
    import torch
    pp, bp = os.path.join(d, "skysegsmall_sim-opt-fp16.param"), os.path.join(d, "skysegsmall_sim-opt-fp16.bin")
    x = sc.probe_sky_image()
    b64 = sc.evaluate(pp, bp, x, torch.float64)
    b32 = sc.evaluate(pp, bp, x, torch.float32)
    A = max(sc.blob_errors(b32, b64).values())
    net = engine.SkySeg(pp, bp, 384, 384, "1959")
    net.set_keep(True)
    p = net.run(x)
    keep = sc.live_blobs(sc.read_param(pp)[2], "1959")  # all but the six dead side sigmoids
    live = {k: v for k, v in b64.items() if k in keep}
    assert len(b64) - len(live) == 6
    eh = sc.blob_errors({k: net.blob(k) for k in live}, live)
    print(f"real weights: A = {A:.3e}, worst e = {max(eh.values()):.3e}, sky fraction {(p > 0.5).mean():.3f}")
    assert max(eh.values()) <= MARGIN * A
    assert np.abs(p.astype(np.float64) - b64["1959"]).max() <= MARGIN * np.abs(b32["1959"].astype(np.float64) - b64["1959"]).max()
    assert 0.3 < (p > 0.5).mean() < 0.6
    net.close()
