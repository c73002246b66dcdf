"""Undistortion of COLMAP camera models, the parts without a GPU: the shared model header (atan, forward maps, inverse), the
output-camera rule and the host statement of the warp (mpmvs_host_undistort_u8) against the independent numpy fixture
(tests/golden/make_undistort_golden.py), and the converter's unchanged default."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

from colmap_common import FIXTURE, check_cams, parse_pairs
from undistort_common import BLANKS, DISTORTED, MODELS, TABLE, border_points, golden, model_params


@pytest.fixture(scope="module")
def colmap(pm):
    return importlib.import_module("mp-mvs_amd.colmap")


@pytest.fixture(scope="module")
def G():
    return golden()


def test_atan_matches_numpy(hostlib):
    """2e-15: a coordinate error eps px moves a value by at most 510 eps; the 1e-6 tie band of the warp test therefore needs
    eps < 2e-9 px, normalised 2e-14 at f = 1e5"""
    rng = np.random.default_rng(7)
    x = np.concatenate([np.linspace(0, 50, 200001), rng.uniform(0, 50, 100000), rng.uniform(0.9, 1.1, 50000),
                        [1.0, np.nextafter(1.0, 0), np.nextafter(1.0, 2), 0.0, 1e-300, 1e-30, 1e-16, 1e-12, 1e-8, 1e-4, 50.0],
                        10.0 ** rng.uniform(-20, 0, 20000)])
    x = np.concatenate([x, -x])
    got = hostlib.undistort_atan(x)
    err = np.abs(got - np.arctan(x))
    print("atan: max abs error %.3g at x = %r" % (err.max(), x[np.argmax(err)]))
    assert err.max() <= 2e-15
    tiny = np.abs(x) < 1e-8
    assert np.array_equal(got[tiny], x[tiny])   # atan(x) = x to the last bit there


@pytest.mark.parametrize("name", DISTORTED)
def test_forward_matches_fixture(hostlib, G, name):
    xy = hostlib.undistort_forward(MODELS.index(name), G["params_" + name], G["fwd_uv"])
    err = np.abs(xy - G["fwd_xy_" + name]).max()
    print(f"{name}: forward map max error {err:.3g} px")
    assert err <= 1e-12


@pytest.mark.parametrize("name", MODELS)
def test_inverse_returns_to_border_points(hostlib, G, name):
    w, h = (int(v) for v in G["size"])
    prm = G["params_" + name] if name in DISTORTED else np.array(model_params(name, w, h))
    p = border_points(w, h)
    uv = hostlib.undistort_inverse(MODELS.index(name), prm, p)
    back = hostlib.undistort_forward(MODELS.index(name), prm, uv)
    err = np.abs(back - p).max()
    print(f"{name}: forward(inverse(p)) max error {err:.3g} px")
    assert err <= 1e-9


@pytest.mark.parametrize("name", DISTORTED)
def test_output_camera_matches_fixture(engine, G, name):
    w, h = (int(v) for v in G["size"])
    for b, blank in enumerate(BLANKS):
        exp = G["cam_%s_%d" % (name, b)]
        pin, ow, oh = engine.undistort_camera(name, G["params_" + name], w, h, blank)
        assert (ow, oh) == (int(exp[4]), int(exp[5])), (name, blank)
        assert np.abs(np.array(pin) - exp[:4]).max() <= 1e-9


def test_output_camera_table(engine):
    for name, prm, blank, size in TABLE:
        pin, ow, oh = engine.undistort_camera(name, prm, 640, 480, blank)
        assert (ow, oh) == size, (name, prm, blank)
        assert pin[2] == pytest.approx(316.75 * ow / 640, abs=1e-9) and pin[3] == pytest.approx(241.5 * oh / 480, abs=1e-9)
        assert pin[0] == prm[0] and pin[1] == (prm[1] if name == "OPENCV_FISHEYE" else prm[0])
    # the limits of the scale act on each axis
    _, ow, oh = engine.undistort_camera("SIMPLE_RADIAL", [600.0, 316.75, 241.5, -0.15], 640, 480, 1.0, 0.2, 1.05)
    assert (ow, oh) == (672, 504)
    _, ow, oh = engine.undistort_camera("SIMPLE_RADIAL", [600.0, 316.75, 241.5, 0.1], 640, 480, 0.0, 0.99, 2.0)
    assert (ow, oh) == (633, 475)


def test_pinhole_output_camera_is_the_source(engine):
    assert engine.undistort_camera("PINHOLE", [500.0, 480.0, 31.5, 20.25], 64, 40) == ((500.0, 480.0, 31.5, 20.25), 64, 40)
    assert engine.undistort_camera(0, [500.0, 31.5, 20.25], 64, 40, 1.0) == ((500.0, 500.0, 31.5, 20.25), 64, 40)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("name", DISTORTED)
def test_warp_matches_fixture(hostlib, G, name, channels):
    img = G["image%d" % channels]
    for b in range(len(BLANKS)):
        cam = G["cam_%s_%d" % (name, b)]
        dst = (cam[:4], int(cam[4]), int(cam[5]))
        out, ok = hostlib.undistort_u8(img if channels == 3 else img[..., 0], MODELS.index(name), G["params_" + name], dst, valid=True)
        val, valid = G["val%d_%s_%d" % (channels, name, b)], G["valid_%s_%d" % (name, b)]
        assert np.array_equal(ok, valid), (name, b)
        assert valid.any()
        out = out.reshape(val.shape)
        assert not out[valid == 0].any()
        clear = (np.abs(val - np.floor(val) - 0.5) > 1e-6) & (valid[..., None] == 1)
        excluded = 1.0 - clear.sum() / float((valid == 1).sum() * channels)
        print(f"{name} blank {BLANKS[b]} c{channels}: {excluded:.2e} of the valid values lie in the tie band")
        assert excluded <= 1e-3
        assert np.array_equal(out[clear], np.floor(val[clear] + 0.5).astype(np.uint8)), (name, b)


ONE_F = ("SIMPLE_PINHOLE", "SIMPLE_RADIAL", "RADIAL")


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("name", ["SIMPLE_PINHOLE", "PINHOLE", "SIMPLE_RADIAL", "RADIAL", "OPENCV", "FULL_OPENCV", "FOV"])
def test_no_distortion_is_the_identity(hostlib, name, generic):
    """a pinhole camera, or a model whose distortion parameters are all zero, onto itself: the input bytes, last row and
    column included.  (The *_FISHEYE models are no pinhole at zero parameters.)  With a focal length that is a power of two
    fx * ((X + 0.5 - cx) / fx) + cx - 0.5 is X exactly; with a generic one it may miss X by an ulp, which the blend absorbs
    everywhere but can put a pixel of the outermost row or column just outside the strict validity rule."""
    rng = np.random.default_rng(11)
    w, h = 37, 23
    prm = np.array(model_params(name, w, h))
    nf = 3 if name in ONE_F else 4
    prm[nf:] = 0.0
    if not generic:
        prm[:nf] = [64.0, 18.25, 11.75] if nf == 3 else [64.0, 32.0, 18.25, 11.75]
    pin = (prm[0], prm[0] if nf == 3 else prm[1], prm[nf - 2], prm[nf - 1])
    for ch in (1, 3):
        img = rng.integers(0, 256, (h, w, ch), dtype=np.uint8)
        out, ok = hostlib.undistort_u8(img[..., 0] if ch == 1 else img, MODELS.index(name), prm, (pin, w, h), valid=True)
        out = out.reshape(h, w, ch)
        if generic:
            assert ok[1:-1, 1:-1].all()
            assert np.array_equal(out[ok == 1], img[ok == 1])
        else:
            assert ok.all()
            assert np.array_equal(out, img)


def test_padded_pitch_and_strided_views(hostlib, G):
    name = "OPENCV"
    cam = G["cam_%s_%d" % (name, 0)]
    dst = (cam[:4], int(cam[4]), int(cam[5]))
    img = G["image3"]
    wide = np.zeros((img.shape[0], img.shape[1] + 5, 3), np.uint8)
    wide[:, :img.shape[1]] = img
    a = hostlib.undistort_u8(img, MODELS.index(name), G["params_" + name], dst)
    b = hostlib.undistort_u8(wide[:, :img.shape[1]], MODELS.index(name), G["params_" + name], dst)
    assert np.array_equal(a, b)


def test_argument_errors(hostlib, engine):
    lib = hostlib.load()
    _, fns = engine.load()
    img = np.zeros((6, 8, 3), np.uint8)
    out = np.full((6, 8, 3), 77, np.uint8)
    prm = np.array([10.0, 4.0, 3.0, 0.01])
    pin = np.array([10.0, 10.0, 4.0, 3.0])

    def host(src=img.ctypes.data, ch=3, w=8, h=6, pitch=0, mid=2, p=prm.ctypes.data, n=4, k=pin.ctypes.data, dw=8, dh=6, o=out.ctypes.data):
        return lib.mpmvs_host_undistort_u8(src, ch, w, h, pitch, mid, p, n, k, dw, dh, o, None)

    def dev(src=img.ctypes.data, ch=3, w=8, h=6, pitch=0, mid=2, p=prm.ctypes.data, n=4, k=pin.ctypes.data, dw=8, dh=6, o=out.ctypes.data):
        return fns["undistort_u8"](0, src, ch, w, h, pitch, mid, p, n, k, dw, dh, o, None)

    assert host() == 0
    bad_f = np.array([0.0, 4.0, 3.0, 0.01])
    nan_k = np.array([10.0, 4.0, 3.0, np.nan])
    bad_pin = np.array([10.0, -1.0, 4.0, 3.0])
    for call in (host, dev):   # every refusal comes before anything else happens: no device is needed to get it
        out[:] = 77
        assert call(src=None) == -2 and call(o=None) == -2 and call(k=None) == -2 and call(p=None) == -2
        assert call(ch=2) == -2 and call(ch=0) == -2 and call(w=0) == -2 and call(h=-1) == -2 and call(dw=0) == -2 and call(dh=0) == -2
        assert call(pitch=23) == -2
        assert call(mid=11) == -2 and call(mid=-1) == -2 and call(n=3) == -2 and call(n=5) == -2 and call(mid=3) == -2
        assert call(p=bad_f.ctypes.data) == -2 and call(p=nan_k.ctypes.data) == -2 and call(k=bad_pin.ctypes.data) == -2
        assert (out == 77).all()
    k4 = np.zeros(4)
    ow, oh = C.c_int(5), C.c_int(5)

    def cam(mid=2, p=prm.ctypes.data, n=4, w=8, h=6, blank=0.0, lo=0.2, hi=2.0, k=k4.ctypes.data, pw=C.byref(ow), ph=C.byref(oh)):
        return fns["undistort_camera"](mid, p, n, w, h, blank, lo, hi, k, pw, ph)

    assert cam() == 0 and ow.value > 0 and oh.value > 0
    assert cam(mid=11) == -2 and cam(mid=-3) == -2 and cam(n=3) == -2 and cam(p=None) == -2 and cam(k=None) == -2 and cam(pw=None) == -2
    assert cam(w=0) == -2 and cam(h=0) == -2 and cam(p=bad_f.ctypes.data) == -2 and cam(p=nan_k.ctypes.data) == -2
    assert cam(blank=-0.1) == -2 and cam(blank=1.1) == -2 and cam(lo=0.0) == -2 and cam(lo=1.5, hi=1.0) == -2 and cam(blank=float("nan")) == -2
    with pytest.raises(ValueError):
        engine.undistort_camera("RADIAL", [1.0, 2.0, 3.0], 8, 6)


def test_undistorted_cameras_of_the_fixture(colmap):
    """the recorded model has one SIMPLE_RADIAL camera with k = 0.0125: its output camera follows the rule, a pinhole camera
    and a camera without distortion keep K and size"""
    m = colmap.read_model(os.path.join(FIXTURE, "sparse"))
    cams = colmap.undistorted_cameras(m)
    K = colmap.intrinsics(m, warn=False)
    seen = False
    for k, cid in enumerate(m.cam_id):
        Kn, w, h = cams[int(cid)]
        if colmap.is_distorted(m, k):
            seen = True
            assert Kn[0, 0] == K[int(cid)][0, 0] and Kn[1, 1] == K[int(cid)][1, 1]
            assert (w, h) != (int(m.cam_width[k]), int(m.cam_height[k]))
            assert Kn[0, 2] == pytest.approx(K[int(cid)][0, 2] * w / m.cam_width[k], abs=1e-9)
        else:
            assert np.array_equal(Kn, K[int(cid)]) and (w, h) == (int(m.cam_width[k]), int(m.cam_height[k]))
    assert seen


def test_image_decoding_for_the_warp(colmap, hostlib, tmp_path):
    """grey against colour is read from the JPEG frame header; colour comes back in R,G,B order from .ppm and .jpg"""
    from PIL import Image
    rng = np.random.default_rng(5)
    rgb = np.repeat(np.repeat(rng.integers(0, 256, (6, 8, 3), dtype=np.uint8), 8, 0), 8, 1)   # 48 x 64, flat 8 x 8 blocks
    (tmp_path / "c.ppm").write_bytes(b"P6\n64 48\n255\n" + rgb.tobytes())
    (tmp_path / "g.pgm").write_bytes(b"P5\n64 48\n255\n" + rgb[..., 0].tobytes())
    Image.fromarray(rgb).save(tmp_path / "c.jpg", "JPEG", quality=98, subsampling=0)
    Image.fromarray(rgb).save(tmp_path / "p.jpg", "JPEG", quality=98, subsampling=0, progressive=True)
    Image.fromarray(rgb[..., 0]).save(tmp_path / "g.jpg", "JPEG", quality=98)
    assert colmap._jpeg_components(tmp_path / "c.jpg") == 3 and colmap._jpeg_components(tmp_path / "p.jpg") == 3
    assert colmap._jpeg_components(tmp_path / "g.jpg") == 1
    assert colmap._jpeg_components(os.path.join(FIXTURE, "images", "img_002.jpg")) == 1
    assert np.array_equal(colmap._decode(str(tmp_path / "c.ppm"), "c.ppm"), rgb)
    assert np.array_equal(colmap._decode(str(tmp_path / "g.pgm"), "g.pgm"), rgb[..., 0])
    for name in ("c.jpg", "p.jpg"):
        a = colmap._decode(str(tmp_path / name), name)
        assert a.shape == rgb.shape and np.abs(a.astype(int) - rgb).max() <= 6   # R,G,B, not B,G,R
    g = colmap._decode(str(tmp_path / "g.jpg"), "g.jpg")
    assert g.shape == (48, 64) and np.abs(g.astype(int) - rgb[..., 0]).max() <= 6


def test_zero_parameter_fisheye_is_copied_with_a_warning(colmap, tmp_path, capsys):
    """a *_FISHEYE camera whose parameters are all zero is copied like a pinhole, as the contract says, but not silently"""
    m = colmap.read_model(os.path.join(FIXTURE, "sparse"))
    for k in range(len(m.cam_id)):
        m.cam_model[k] = colmap.CAMERA_MODELS.index("OPENCV_FISHEYE")
        m.cam_params[k] = [60.0, 60.0, 31.5, 23.5] + [0.0] * 8
    cams = colmap.undistorted_cameras(m)
    colmap.undistort_images(m, os.path.join(FIXTURE, "images"), str(tmp_path / "out"), cams)
    err = capsys.readouterr().err
    assert "fisheye" in err and "copied" in err
    for i, name in enumerate(m.names):
        assert (tmp_path / "out" / ("%08d.jpg" % i)).read_bytes() == open(os.path.join(FIXTURE, "images", name), "rb").read()


def test_convert_default_is_unchanged(colmap, tmp_path, monkeypatch, capsys):
    """undistort=False: the files of the recorded conversion and the warning, with the recorded view selection in place of
    the GPU's"""
    exp = os.path.join(FIXTURE, "expected_d192")
    ids, scores = parse_pairs(os.path.join(exp, "pair.txt"))
    monkeypatch.setattr(colmap, "select_views", lambda model, num_view=20, device=0: (ids, scores))
    out = tmp_path / "out"
    times = colmap.convert(FIXTURE, out, undistort=False)
    assert set(times) == {"read", "select", "cams", "pairs", "images"}
    assert "distortion parameters of camera(s)" in capsys.readouterr().err
    check_cams(out / "cams", os.path.join(exp, "cams"), 14)
    assert (out / "pair.txt").read_bytes() == open(os.path.join(exp, "pair.txt"), "rb").read()
    m = colmap.read_model(os.path.join(FIXTURE, "sparse"))
    assert sorted(os.listdir(out / "images")) == ["%08d.jpg" % i for i in range(14)]
    for i, name in enumerate(m.names):
        assert (out / "images" / ("%08d.jpg" % i)).read_bytes() == open(os.path.join(FIXTURE, "images", name), "rb").read()
    out2 = tmp_path / "out2"
    colmap.convert(FIXTURE, out2)   # the default is undistort=False
    for i in range(14):
        assert (out2 / "cams" / ("%08d_cam.txt" % i)).read_bytes() == (out / "cams" / ("%08d_cam.txt" % i)).read_bytes()
