"""The tracks of the fused points (mpmvs_fuse_ply_tracks, include/mpmvs.h "Tracks") on the MI355X: which pixels of which images
every point was averaged from, as CSR in the PLY's point order.  The defining property is checked in full: the track alone
reproduces all nine floats of its point, bit for bit, with a plain numpy fp32 statement of the fusion's arithmetic."""
import ctypes as C
import importlib

import numpy as np
import pytest

from test_fusion_cpu import _colours_and_sky, _scene

pytestmark = pytest.mark.gpu

# (width, height), dynamic consistency, reference order, colour + sky.  96 x 72 is the scene of the CPU tests; 131 x 97 is no
# multiple of the 256-pixel tile; 320 x 240 = 76 800 pixels = 300 tiles takes the totals scan into its second round; the
# reference order runs at the size of its own test.  The view lists of this scene are not in ascending image order (image 0:
# [1, 3, 4, 2, 5]), so slot order and image order differ.
CASES = [(size, dyn, False, sky) for size in ((96, 72), (131, 97), (320, 240)) for dyn in (True, False) for sky in (False, True)] + \
        [((160, 120), dyn, True, sky) for dyn in (True, False) for sky in (False, True)]
IDS = ["%dx%d-%s-%s-%s" % (s[0], s[1], "dynamic" if d else "static", "reference" if r else "snapshot", "colour+sky" if k else "grey") for s, d, r, k in CASES]
_cache = {}


def _inputs(pm, size, colour_sky):
    key = ("in", size, colour_sky)
    if key not in _cache:
        fusion = importlib.import_module("mp-mvs_amd.fusion")
        sc, cams, depths, normals, grays, neigh = _scene(pm, size=size)
        if size != (96, 72):                       # the 96 x 72 scene stays whole: its point and length counts are asserted
            depths[2][10:30, 20:60] = 0.0
        est = [True] * 6 if size == (96, 72) else [True, True, False, True, True, True]
        cols, sky = _colours_and_sky(grays) if colour_sky else (grays, None)
        _cache[key] = dict(cams=cams, depths=depths, normals=normals, cols=[fusion._as_u8(c) for c in cols], sky=sky, neigh=neigh, est=est)
    return _cache[key]


def _case(pm, case):
    """the three entry points on one case, computed once and shared by the tests below (nothing changes them)"""
    if case not in _cache:
        fusion = importlib.import_module("mp-mvs_amd.fusion")
        size, dyn, ref, colour_sky = case
        a = _inputs(pm, size, colour_sky)
        args = (a["cams"], a["est"], a["depths"], a["normals"], a["cols"], a["neigh"], dyn)
        kw = dict(sky=a["sky"], reference_order=ref)
        rec, off, img, pix, masks = fusion.fuse_ply_tracks(*args, **kw)
        rec0, masks0 = fusion.fuse_ply(*args, **kw)
        cloud, valid, _ = fusion.fuse(*args, **kw)
        _cache[case] = dict(a, rec=rec, off=off, img=img, pix=pix, masks=masks, rec0=rec0, masks0=masks0, cloud=cloud, valid=valid,
                            dyn=dyn, ref=ref)
        for v in (rec, off, img, pix, cloud):
            v.setflags(write=False)
    return _cache[case]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_records_and_masks_equal_fuse_ply(pm, engine, case):
    r = _case(pm, case)
    assert r["rec"].shape == r["rec0"].shape and r["rec"].tobytes() == r["rec0"].tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(r["masks"], r["masks0"]))
    assert len(r["rec"]) > 1000


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_track_structure(pm, engine, case):
    check_track_structure(_case(pm, case))


def check_track_structure(r):
    """r: the inputs (cams, depths, neigh, sky, dyn) and, of one call each, fuse_ply_tracks' rec / off / img / pix and fuse's valid;
    shared with tests/test_fusion_fuzz_gpu.py"""
    off, img, pix = r["off"], r["img"], r["pix"]
    m = len(r["rec"])
    assert off.dtype == np.int64 and img.dtype == np.int32 and pix.dtype == np.int32
    assert off.shape == (m + 1,) and off[0] == 0 and (np.diff(off) > 0).all() and off[-1] == len(img) == len(pix)
    # first entries: the pixel that produced the point, image then raster order, as the uncompacted fuse() reports them
    want_i = np.concatenate([np.full(int(v.sum()), i, np.int32) for i, v in enumerate(r["valid"])])
    want_t = np.concatenate([np.flatnonzero(v) for v in r["valid"]]).astype(np.int32)
    assert np.array_equal(img[off[:-1]], want_i) and np.array_equal(pix[off[:-1]], want_t)
    # every entry names a view of the producing image's list, in strictly ascending slot order (slot 0 = the image itself)
    n = len(r["cams"])
    slot = np.full((n, n), -1, np.int64)
    for i in range(n):
        for j, s in enumerate([i] + list(r["neigh"][i])):
            slot[i, s] = j
    length = np.diff(off)
    owner = np.repeat(want_i, length)
    sl = slot[owner, img]
    first = np.zeros(len(img), bool)
    first[off[:-1]] = True
    assert (sl[first] == 0).all() and (sl[~first] >= 1).all()
    assert (np.diff(sl)[~first[1:]] > 0).all()
    # pixels are in range and have a depth
    npx = np.array([c.width * c.height for c in r["cams"]])
    assert (pix >= 0).all() and (pix < npx[img]).all()
    for s in range(n):
        assert (r["depths"][s].reshape(-1)[pix[img == s]] > 0).all()
    lo = 2 if r["dyn"] else 3
    assert m == 0 or (length.min() >= lo and length.max() <= max(len(x) for x in r["neigh"]) + 1)
    if r["sky"] is not None:
        for i in range(n):
            if r["sky"][i] is not None:
                assert not (r["sky"][i].reshape(-1)[want_t[want_i == i]] > 0).any()


def _backproject(cam, depth, q):
    """backproject of pm_device.hpp restated: pixel q (raster index at the image's own width) at its depth -> world, fp32"""
    f = np.float32
    K, R, Cc = [f(v) for v in cam.K], [f(v) for v in cam.R], [f(v) for v in cam.C]
    x, y = (q % cam.width).astype(f), (q // cam.width).astype(f)
    d = depth.reshape(-1)[q].astype(f)
    X0 = (d * (x - K[2])) / K[0]
    X1 = (d * (y - K[5])) / K[4]
    X2 = d
    t0 = (R[0] * X0 + R[3] * X1) + R[6] * X2
    t1 = (R[1] * X0 + R[4] * X1) + R[7] * X2
    t2 = (R[2] * X0 + R[5] * X1) + R[8] * X2
    return np.stack([t0 + Cc[0], t1 + Cc[1], t2 + Cc[2]], -1)


def _nine(r, img, pix):
    """position, normal, colour (fp32) of the entries (img, pix)"""
    out = np.zeros((len(img), 9), np.float32)
    for s in range(len(r["cams"])):
        k = img == s
        q = pix[k]
        out[k, 0:3] = _backproject(r["cams"][s], r["depths"][s], q)
        out[k, 3:6] = r["normals"][s].reshape(-1, 3)[q]
        col = r["cols"][s]
        out[k, 6:9] = col.reshape(-1, 3)[q] if col.ndim == 3 else col.reshape(-1)[q][:, None]
    return out


def points_from_tracks(r):
    """sequential fp32 adds in track order and one division; shared with tests/test_fusion_fuzz_gpu.py"""
    off, img, pix = r["off"], r["img"], r["pix"]
    length = np.diff(off)
    terms = _nine(r, img, pix)
    acc = terms[off[:-1]].copy()
    for k in range(1, int(length.max()) if len(length) else 0):
        has = length > k
        acc[has] = acc[has] + terms[off[:-1][has] + k]
    return acc / length.astype(np.float32)[:, None]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_track_alone_reproduces_the_point_bit_for_bit(pm, engine, case):
    """the defining property: sequential fp32 adds in track order and one division give all nine floats of fuse()'s out_points9"""
    r = _case(pm, case)
    got = points_from_tracks(r)
    assert got.dtype == np.float32 and got.shape == r["cloud"].shape
    differ = (got.view(np.uint32) != np.ascontiguousarray(r["cloud"]).view(np.uint32)).any(1)
    print(f"{int(differ.sum())} of {len(got)} points differ")
    assert not differ.any()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_tracks_against_masks(pm, engine, case):
    """snapshot: the entries after the first are exactly the pixels the points mark (plus the sky pixels of the estimated images);
    reference order: the masks also hold the carried used_list entries, so they contain that"""
    r = _case(pm, case)
    off, img, pix = r["off"], r["img"], r["pix"]
    first = np.zeros(len(img), bool)
    first[off[:-1]] = True
    for s, cam in enumerate(r["cams"]):
        want = np.zeros(cam.width * cam.height, bool)
        want[pix[(img == s) & ~first]] = True
        if r["est"][s] and r["sky"] is not None and r["sky"][s] is not None:
            want |= r["sky"][s].reshape(-1) > 0
        got = r["masks"][s].reshape(-1) == 1
        assert (got[want]).all() if r["ref"] else np.array_equal(got, want), s


@pytest.mark.parametrize("case", [c for c in CASES if c[0] == (96, 72)], ids=[i for c, i in zip(CASES, IDS) if c[0] == (96, 72)])
def test_tracks_are_not_vacuous(pm, engine, case):
    """the scene produces thousands of points and every track length many times (a float64 sketch of the snapshot loop gives
    8 156 / 7 319 points at this size, every length at least 450 times)"""
    r = _case(pm, case)
    length = np.diff(r["off"])
    counts = {k: int((length == k).sum()) for k in range(2, 7)}
    print(len(length), "points; track lengths", counts)
    assert len(length) >= 4000
    for k in range(2 if r["dyn"] else 3, 7):
        assert counts[k] >= 100, (k, counts)


def test_tracks_from_resident_contexts_equal_the_host_array_path(pm, engine):
    """the ctxs form: maps that are still resident in the contexts that estimated them give the same four arrays"""
    fusion = importlib.import_module("mp-mvs_amd.fusion")
    sc, neigh = pm.synth.make_grid_scene(128, 96, 3, 2, spacing=0.4, rot_deg=1.0, quantize=True)
    cams = [v.cam for v in sc.views]
    imgs = [v.image for v in sc.views]
    ctxs, depths, normals = [], [], []
    for i in range(6):
        h = engine.create(0)
        ids = [i] + neigh[i]
        h.set_views([cams[j] for j in ids], [imgs[j] for j in ids])
        dmin, dmax = pm.synth.kernel_depth_range(cams[i])
        h.run(pm.PatchMatchParams(num_images=len(ids), depth_min=float(dmin), depth_max=float(dmax), max_scale=1), 100 + i)
        planes, _ = h.get()
        ctxs.append(h)
        depths.append(planes[..., 3].copy())
        normals.append(planes[..., :3].copy())
    est = [True] * 6
    mixed = [c if k in (0, 3, 4) else None for k, c in enumerate(ctxs)]
    for ref in (False, True):
        want = fusion.fuse_ply_tracks(cams, est, depths, normals, imgs, neigh, reference_order=ref)
        assert len(want[0]) > 300
        for cx, dd, nn in ((ctxs, [None] * 6, [None] * 6), (mixed, depths, normals)):
            got = fusion.fuse_ply_tracks(cams, est, dd, nn, imgs, neigh, reference_order=ref, ctxs=cx)
            assert all(np.array_equal(a, b) for a, b in zip(got[:4], want[:4]))
            assert all(np.array_equal(a, b) for a, b in zip(got[4], want[4]))


def test_empty_cloud_and_null_pointer(pm, engine):
    fusion = importlib.import_module("mp-mvs_amd.fusion")
    a = _inputs(pm, (96, 72), False)
    args = (a["cams"], [False] * 6, a["depths"], a["normals"], a["cols"], a["neigh"])
    rec, off, img, pix, _ = fusion.fuse_ply_tracks(*args)      # the four buffers were returned and freed
    assert rec.shape == (0, 27) and off.tolist() == [0] and len(img) == 0 and len(pix) == 0
    # a NULL track_off is refused before anything is allocated
    lib, _ = engine.load()
    fn = lib.mpmvs_fuse_ply_tracks
    outs = []

    def call(*x):
        rec_p, img_p, pix_p = C.POINTER(C.c_ubyte)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)()
        outs.extend([rec_p, img_p, pix_p])
        return int(fn(*x[:4], None, *x[4:-3], C.byref(rec_p), None, C.byref(img_p), C.byref(pix_p), x[-1]))

    with pytest.raises(RuntimeError, match=r"\(-2\)"):
        fusion.call_fuse(call, (0,), a["cams"], a["est"], a["depths"], a["normals"], a["cols"], a["neigh"])
    assert len(outs) == 3 and not any(bool(p) for p in outs)


def test_fuse_folder_writes_the_visibility_file(pm, engine, hostlib, tmp_path):
    """RunFusion(write_vis) over a folder: MPMVS_model.ply.vis == write_vis on fuse_ply_tracks' output for the same inputs, byte
    for byte, beside an unchanged PLY; without the flag no such file"""
    fusion = importlib.import_module("mp-mvs_amd.fusion")
    sc, cams, depths, normals, grays, neigh = _scene(pm, size=(96, 72))
    cols = [np.stack([g, 255 - g, g // 2 + 20], -1).astype(np.uint8) for g in (np.asarray(x).astype(np.uint8) for x in grays)]   # R,G,B for the files
    hostlib.write_dataset(str(tmp_path), cams, cols, neigh, fmt="ppm")
    for i in range(6):
        d = tmp_path / "MPMVS" / f"2333_{i:08d}"
        d.mkdir(parents=True)
        hostlib.write_dmb(d / "depths.dmb", depths[i])
        hostlib.write_dmb(d / "normals.dmb", normals[i])
    ply, vis = tmp_path / "MPMVS" / "MPMVS_model.ply", tmp_path / "MPMVS" / "MPMVS_model.ply.vis"
    n0 = hostlib.fuse_folder(tmp_path)
    plain = ply.read_bytes()
    assert n0 > 1000 and not vis.exists()
    assert hostlib.fuse_folder(tmp_path, write_vis=True) == n0 and ply.read_bytes() == plain
    bgr = [hostlib.read_image(tmp_path / "images" / f"{i:08d}.ppm", 3) for i in range(6)]
    file_cams = []
    for i in range(6):
        c = hostlib.read_camera(tmp_path / "cams" / f"{i:08d}_cam.txt")
        c.height, c.width = depths[i].shape
        file_cams.append(c)
    rec, off, img, pix, _ = fusion.fuse_ply_tracks(file_cams, [True] * 6, depths, normals, bgr, neigh)
    assert len(rec) == n0 and rec.tobytes() == plain.split(b"end_header\n", 1)[1]
    want = tmp_path / "want.vis"
    fusion.write_vis(want, off, img)
    assert vis.read_bytes() == want.read_bytes()
    off2, img2 = fusion.read_vis(vis)
    assert np.array_equal(off2, off) and np.array_equal(img2, img)
