"""Undistortion on the GPU: mpmvs_undistort_u8 against the host statement bit for bit, the converter with undistort=True on
the recorded fixture, and PatchMatch + fusion on a scene seen through SIMPLE_RADIAL cameras."""
import importlib
import os
import threading

import numpy as np
import pytest

from colmap_common import FIXTURE
from undistort_common import (MODELS, export_colmap_sr, gt_fraction, model_params, quat_rotation, read_cam_text, render_distorted,
                              render_pinhole, rotmat2qvec, sr_output_camera)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def colmap(pm, engine):
    return importlib.import_module("mp-mvs_amd.colmap")


def pinhole_of(name, prm):
    one = name in ("SIMPLE_PINHOLE", "SIMPLE_RADIAL", "RADIAL", "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE")
    return (prm[0], prm[0], prm[1], prm[2]) if one else (prm[0], prm[1], prm[2], prm[3])


def both(engine, hostlib, img, name, prm, dst):
    g, gok = engine.undistort_u8(img, name, prm, dst, valid=True)
    h, hok = hostlib.undistort_u8(img, MODELS.index(name), prm, dst, valid=True)
    assert g.shape == h.shape and g.tobytes() == h.tobytes(), (name, img.shape, dst)
    assert gok.tobytes() == hok.tobytes(), (name, img.shape, dst)
    g2 = engine.undistort_u8(img, name, prm, dst)   # without the mask: the same bytes
    assert g2.tobytes() == g.tobytes()
    return g, gok


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("name", MODELS)
def test_device_equals_host(engine, hostlib, name, channels):
    rng = np.random.default_rng(100 * MODELS.index(name) + channels)
    for w, h in ((65, 17), (37, 23), (256, 3), (1, 1)):
        prm = model_params(name, w, h)
        img = rng.integers(0, 256, (h, w) + ((3,) if channels == 3 else ()), dtype=np.uint8)
        fx, fy, cx, cy = pinhole_of(name, prm)
        dsts = [((fx, fy, cx, cy), w, h),                                        # the source's own pinhole and size
                ((fx / 2, fy / 2, cx / 2, cy / 2), max(1, w // 2), max(1, h // 2)),  # smaller than the source
                ((1.5 * fx, 1.5 * fy, 1.5 * cx + 0.3, 1.5 * cy), (3 * w) // 2 + 1, (3 * h) // 2 + 2),  # larger
                ((fx / 4, fy / 4, cx, cy), 2 * w + 1, 2 * h + 3)]                 # most pixels have no source
        if w > 1:
            for blank in (0.0, 1.0):
                dsts.append(engine.undistort_camera(name, prm, w, h, blank))
        for dst in dsts:
            out, ok = both(engine, hostlib, img, name, prm, dst)
            assert not out[ok == 0].any()
        if w > 1:
            assert ok.any()
            _, ok = both(engine, hostlib, img, name, prm, dsts[3])
            assert 0 < ok.mean() < 0.5
        # a padded pitch: the view of a wider buffer
        wide = rng.integers(0, 256, (h, w + 7) + ((3,) if channels == 3 else ()), dtype=np.uint8)
        wide[:, :w] = img
        assert engine.undistort_u8(wide[:, :w], name, prm, dsts[0]).tobytes() == engine.undistort_u8(img, name, prm, dsts[0]).tobytes()


@pytest.mark.parametrize("name", ["SIMPLE_RADIAL", "OPENCV_FISHEYE", "THIN_PRISM_FISHEYE"])
def test_device_equals_host_fullsize(engine, hostlib, name):
    rng = np.random.default_rng(5)
    w, h = 1600, 1200
    prm = model_params(name, w, h)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    dst = engine.undistort_camera(name, prm, w, h)
    out, ok = both(engine, hostlib, img, name, prm, dst)
    assert ok.mean() > 0.9 and engine.load()[1]["undistort_kernel_ms"]() > 0
    grey = img[..., 1]
    both(engine, hostlib, grey, name, prm, engine.undistort_camera(name, prm, w, h, 1.0))


def test_two_threads_agree_with_one(engine, hostlib):
    rng = np.random.default_rng(9)
    jobs = []
    for k, name in enumerate(["OPENCV", "RADIAL_FISHEYE", "FOV", "FULL_OPENCV"]):
        w, h = 301 + 17 * k, 211 + 5 * k
        prm = model_params(name, w, h)
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        jobs.append((img, name, prm, engine.undistort_camera(name, prm, w, h, 0.5)))
    single = [engine.undistort_u8(*j).tobytes() for j in jobs]
    got = [[None] * len(jobs) for _ in range(2)]
    errors = []

    def work(t):
        try:
            for _ in range(3):
                for k in (range(len(jobs)) if t == 0 else reversed(range(len(jobs)))):
                    got[t][k] = engine.undistort_u8(*jobs[k]).tobytes()
        except Exception as e:   # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors
    assert got[0] == single and got[1] == single


def test_error_codes(engine):
    _, fns = engine.load()
    img = np.zeros((6, 8, 3), np.uint8)
    out = np.zeros((6, 8, 3), np.uint8)
    prm = np.array([10.0, 4.0, 3.0, 0.01])
    pin = np.array([10.0, 10.0, 4.0, 3.0])
    call = lambda dev=0, src=img.ctypes.data, o=out.ctypes.data: fns["undistort_u8"](dev, src, 3, 8, 6, 0, 2, prm.ctypes.data, 4, pin.ctypes.data, 8, 6, o, None)
    assert call() == 0
    assert call(dev=engine.device_count() + 3) == -100 and call(dev=-1) == -100
    assert call(src=None) == -2 and call(o=None) == -2
    assert call() == 0   # the refused calls leave the library usable


def test_convert_undistort_on_the_fixture(colmap, engine, hostlib, tmp_path, capsys):
    """the recorded model: the images of the SIMPLE_RADIAL camera are warped (grey JPEG -> .pgm) and share one output
    camera, the PINHOLE camera's images are copied byte for byte; no warning"""
    out = tmp_path / "out"
    colmap.convert(FIXTURE, out, undistort=True)
    assert "warning" not in capsys.readouterr().err
    m = colmap.read_model(os.path.join(FIXTURE, "sparse"))
    cams = colmap.undistorted_cameras(m)
    index = {int(c): k for k, c in enumerate(m.cam_id)}
    warped = 0
    for i, name in enumerate(m.names):
        k = index[int(m.image_cam[i])]
        Kn, w, h = cams[int(m.image_cam[i])]
        _, K = read_cam_text(out / "cams" / ("%08d_cam.txt" % i))
        assert np.array_equal(K, Kn)
        src = os.path.join(FIXTURE, "images", name)
        if colmap.is_distorted(m, k):
            warped += 1
            got = hostlib.read_image(out / "images" / ("%08d.pgm" % i), 1)
            assert got.shape == (h, w)
            cname, prm = colmap.camera_params(m, k)
            exp = hostlib.undistort_u8(hostlib.read_image(src, 1), MODELS.index(cname), prm, ((Kn[0, 0], Kn[1, 1], Kn[0, 2], Kn[1, 2]), w, h))
            assert np.array_equal(got, exp)
        else:
            assert (out / "images" / ("%08d.jpg" % i)).read_bytes() == open(src, "rb").read()
    assert 0 < warped < len(m.names)
    # a colour image of another format goes through PIL and comes out as .ppm in R,G,B order; a wrong size is refused by name
    from PIL import Image
    png = tmp_path / "png"
    png.mkdir()
    rgb = np.random.default_rng(3).integers(0, 256, (48, 64, 3), dtype=np.uint8)
    m.names = [n.replace(".jpg", ".png") for n in m.names]
    for name in m.names:
        Image.fromarray(rgb).save(png / name)
    colmap.undistort_images(m, str(png), str(tmp_path / "png_out"), cams)
    i = next(i for i in range(len(m.names)) if colmap.is_distorted(m, index[int(m.image_cam[i])]))
    Kn, w, h = cams[int(m.image_cam[i])]
    cname, prm = colmap.camera_params(m, index[int(m.image_cam[i])])
    exp = hostlib.undistort_u8(rgb, MODELS.index(cname), prm, ((Kn[0, 0], Kn[1, 1], Kn[0, 2], Kn[1, 2]), w, h))
    assert (tmp_path / "png_out" / ("%08d.ppm" % i)).read_bytes() == b"P6\n%d %d\n255\n" % (w, h) + exp.tobytes()
    # colour .ppm and .jpg sources go through the host library's reader (B,G,R) and come out as .ppm in R,G,B order
    for ext in (".ppm", ".jpg"):
        d = tmp_path / ("in" + ext[1:])
        d.mkdir()
        m.names = [os.path.splitext(n)[0] + ext for n in m.names]
        for name in m.names:
            if ext == ".ppm":
                (d / name).write_bytes(b"P6\n64 48\n255\n" + rgb.tobytes())
            else:
                Image.fromarray(rgb).save(d / name, "JPEG", quality=95, subsampling=0)
        colmap.undistort_images(m, str(d), str(tmp_path / ("out" + ext[1:])), cams)
        src_rgb = rgb if ext == ".ppm" else np.ascontiguousarray(hostlib.read_image(d / m.names[i], 3)[..., ::-1])
        if ext == ".jpg":   # the decoded channels are in the order they were written in (the red plane nearest the red plane)
            assert np.abs(src_rgb.astype(int) - rgb).mean() < np.abs(src_rgb[..., ::-1].astype(int) - rgb).mean() / 2
        exp = hostlib.undistort_u8(src_rgb, MODELS.index(cname), prm, ((Kn[0, 0], Kn[1, 1], Kn[0, 2], Kn[1, 2]), w, h))
        assert (tmp_path / ("out" + ext[1:]) / ("%08d.ppm" % i)).read_bytes() == b"P6\n%d %d\n255\n" % (w, h) + exp.tobytes()
    m.names = [os.path.splitext(n)[0] + ".png" for n in m.names]
    Image.fromarray(rgb[:40]).save(png / m.names[i])
    with pytest.raises(ValueError, match=m.names[i]):
        colmap.undistort_images(m, str(png), str(tmp_path / "bad_out"), cams)


# ---- PatchMatch on a scene seen through distorted cameras -----------------------------------------------------------
def test_patchmatch_on_undistorted_scene(pm, colmap, hostlib, tmp_path):
    """(a) the pinhole views rendered at the undistorted cameras, (b) convert(undistort=True) of the distorted renders,
    (c) convert(undistort=False) of them, scored against the distorted renders' own depth.

    The three shares of pixels within 5 % of GT depth are printed; DESIGN.md section 12.6 records what is known of them.  Whether
    (b) stays within the 0.02 that tests/test_colmap_gpu.py grants a loss-free conversion is reported, not asserted."""
    synth = pm.synth
    W, H, k = 96, 72, -0.2
    f, cx, cy = 0.9 * W, W / 2.0, H / 2.0
    fs = W / 1600.0
    sc, neigh = synth.make_grid_scene(W, H, 3, 2, spacing=0.5, rot_deg=1.0, quantize=True)
    dist = [render_distorted(synth, v, W, H, f, cx, cy, k, fs) for v in sc.views]
    pin, ow, oh = sr_output_camera(f, cx, cy, k, W, H)
    dense = tmp_path / "dense"
    assert export_colmap_sr(dist, str(dense), f, cx, cy, k) > 500
    # the converter's output camera is the one the test's own statement of the rule gives
    m = colmap.read_model(str(dense / "sparse"))
    Kn, cw, ch = colmap.undistorted_cameras(m)[1]
    assert (cw, ch) == (ow, oh) and np.abs(np.array([Kn[0, 0], Kn[1, 1], Kn[0, 2], Kn[1, 2]]) - np.array(pin)).max() <= 1e-9
    # (a) the yardstick
    Kp = np.array([[pin[0], 0, pin[2]], [0, pin[1], pin[3]], [0, 0, 1.0]])
    direct = [render_pinhole(synth, v, pin, ow, oh, fs) for v in sc.views]
    cams_a = [pm.make_camera(Kp, v.R, -v.R @ v.C, oh, ow, 3.0, 8.0) for v in sc.views]
    fa, fb, fc = tmp_path / "a", tmp_path / "b", tmp_path / "c"
    hostlib.write_dataset(str(fa), cams_a, [v.image for v in direct], neigh)
    colmap.convert(str(dense), str(fb), undistort=True)
    colmap.convert(str(dense), str(fc), undistort=False)
    assert sorted(os.listdir(fb / "images")) == ["%08d.pgm" % i for i in range(6)]
    for i, v in enumerate(sc.views):
        E, K = read_cam_text(fb / "cams" / ("%08d_cam.txt" % i))
        assert np.abs(K - Kp).max() <= 1e-9
        # the export states the rotation as a quaternion: of the fp32-rounded, not exactly orthonormal R that is the nearest
        # rotation (1e-8 away), which the converter must hand on within 1e-9; the yardstick's file holds fp32 values
        assert np.abs(E[:3, :3] - quat_rotation(rotmat2qvec(v.R))).max() <= 1e-9 and np.abs(E[:3, 3] - (-v.R @ v.C)).max() <= 1e-9
        ca, cb = hostlib.read_camera(fa / "cams" / ("%08d_cam.txt" % i)), hostlib.read_camera(fb / "cams" / ("%08d_cam.txt" % i))
        assert list(ca.K) == list(cb.K) and np.abs(np.array(ca.R) - np.array(cb.R)).max() <= 1e-6
        img = hostlib.read_pgm(fb / "images" / ("%08d.pgm" % i))
        assert img.shape == (oh, ow)
        inner = np.abs(img - direct[i].image)[4:-4, 4:-4]
        print(f"view {i}: undistorted image against the direct render, mean abs difference {inner.mean():.2f} grey levels")
    kw = dict(device=0, geom_iterations=1, planar_prior=True, geom_planar_prior=True, max_scale=1, seed=4242)
    for folder in (fa, fb, fc):
        hostlib.run_folder(folder, **kw)
    f_a, f_b, f_c = gt_fraction(hostlib, fa, direct), gt_fraction(hostlib, fb, direct), gt_fraction(hostlib, fc, dist)
    print(f"within 5 % of GT depth: (a) pinhole renders {f_a:.4f}, (b) undistorted {f_b:.4f}, (c) distortion ignored {f_c:.4f}; "
          f"(a) - (b) = {f_a - f_b:.4f} (a loss-free conversion is granted 0.02)")
    assert f_c <= f_a - 0.10, "the scene must make ignoring the distortion costly, or it tests nothing"
    assert f_b >= (f_a + f_c) / 2
    n = hostlib.fuse_folder(fb, device=0)
    assert n > 0 and os.path.getsize(fb / "MPMVS" / "MPMVS_model.ply") > 0
