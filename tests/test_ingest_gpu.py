"""The 8-bit image entry on the GPU (include/mpmvs.h: mpmvs_set_views_u8, mpmvs_resize_u8; csrc/pm_ingest.hpp): views handed in as
the bytes an image file decoded to, at the file's size, and shrunk on the device.  The entry is defined by equivalence with
mpmvs_set_views on the fp32 images F_i = (float)bytes, or ResizeLinear((float)bytes) as host/PatchMatchHost.cpp states it where
the sizes differ -- so everything here is compared bit for bit (np.array_equal) unless a test says otherwise."""
import copy
import importlib
import os
import subprocess
import sys
import textwrap

import ctypes as C
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 20240311
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------
# 1 + 2: the probe
# ---------------------------------------------------------------------------
RESIZE_CASES = [  # (src_w, src_h, dst_w, dst_h)
    (207, 154, 80, 60), (126, 195, 65, 100),
    (320, 240, 100, 200),     # non-uniform
    (96, 64, 96, 64),         # identity size
    (101, 67, 100, 66),       # ratio near 1
    (40, 30, 97, 71),         # an enlargement
    (1, 57, 1, 20), (1, 57, 9, 20),   # 1-pixel-wide sources
    (83, 1, 31, 1), (83, 1, 31, 5),   # 1-pixel-high sources
    (2, 2, 1, 1),
]


@pytest.mark.parametrize("sw,sh,dw,dh", RESIZE_CASES)
def test_probe_equals_host_resize_linear(engine, hostlib, sw, sh, dw, dh):
    b = np.random.default_rng(sw * 1000 + sh).integers(0, 256, (sh, sw), dtype=np.uint8)
    got = engine.resize_u8(b, dw, dh)
    want = hostlib.resize_linear(b.astype(np.float32), dw, dh)
    assert got.shape == (dh, dw) and got.dtype == np.float32
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {got.size} pixels differ, max |d| {np.abs(got - want).max()}"


def test_probe_honours_the_pitch(engine, hostlib):
    """a strided source: rows of 207 bytes inside rows of 256"""
    big = np.random.default_rng(5).integers(0, 256, (154, 256), dtype=np.uint8)
    view = big[:, 11:218]
    assert view.strides == (256, 1) and not view.flags.c_contiguous
    got = engine.resize_u8(view, 80, 60)
    assert np.array_equal(got, hostlib.resize_linear(np.ascontiguousarray(view).astype(np.float32), 80, 60))


def test_probe_at_the_real_size(engine, hostlib):
    """one 24-Mpix photograph shrunk to the shipped limit: 6048 x 4032 -> 3200 x 2133"""
    b = np.random.default_rng(6).integers(0, 256, (4032, 6048), dtype=np.uint8)
    got = engine.resize_u8(b, 3200, 2133)
    want = hostlib.resize_linear(b.astype(np.float32), 3200, 2133)
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {got.size} pixels differ"


def test_probe_equals_independent_fixture(engine):
    """tests/golden/resize_u8_golden_v1.npz (torch bilinear in float64, computed without this repository; the target size by
    the reference's rounding rule, src/PatchMatch.cpp:898-903).  Tolerance: 1e-5 of the 0..255 range, as the fp32 fixture's
    replay in test_host_cpu.py (fp32 interpolation against float64 rounded once).  test_ingest_cpu.py replays the same file
    through the host's ResizeLinear, which tells a bad fixture from a bad kernel."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "resize_u8_golden_v1.npz"))
    assert int(z["n"]) >= 4
    for k in range(int(z["n"])):
        src, want, mx = z[f"src{k}"], z[f"dst{k}"], int(z[f"max{k}"])
        assert src.dtype == np.uint8
        rows, cols = src.shape
        f = min(np.float32(mx) / np.float32(cols), np.float32(mx) / np.float32(rows))
        new_cols, new_rows = int(np.floor(np.float32(cols) * f + np.float32(0.5))), int(np.floor(np.float32(rows) * f + np.float32(0.5)))
        assert (new_rows, new_cols) == want.shape
        got = engine.resize_u8(src, new_cols, new_rows)
        err = np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
        print(f"case {k}: max |difference| {err}")
        assert err <= 255.0 * 1e-5, f"case {k}: max |difference| {err}"


# ---------------------------------------------------------------------------
# 3 - 5: the entry against mpmvs_set_views on F_i
# ---------------------------------------------------------------------------
def scaled_cam(c, new_w, new_h):
    """the camera of a view shrunk to new_w x new_h: K scaled as PatchMatchInit does (reference src/PatchMatch.cpp:905-915)"""
    k = copy.copy(c)
    sx, sy = np.float32(new_w) / np.float32(c.width), np.float32(new_h) / np.float32(c.height)
    K = np.array(list(c.K), np.float32)
    K[0], K[2], K[4], K[5] = K[0] * sx, K[2] * sx, K[4] * sy, K[5] * sy
    for j in range(9):
        k.K[j] = float(K[j])
    k.width, k.height = new_w, new_h
    return k


def to_bytes(images):
    out = [im.astype(np.uint8) for im in images]
    for b, im in zip(out, images):
        assert np.array_equal(b.astype(np.float32), im), "quantize=True images are 8-bit exact"
    return out


def equivalent_floats(hostlib, cams, bytes_):
    """F_i of the entry's contract"""
    return [b.astype(np.float32) if b.shape == (c.height, c.width) else hostlib.resize_linear(b.astype(np.float32), c.width, c.height)
            for c, b in zip(cams, bytes_)]


def params_for(pm, cams, **kw):
    dmin, dmax = pm.synth.kernel_depth_range(cams[0])
    return pm.PatchMatchParams(num_images=len(cams), depth_min=float(dmin), depth_max=float(dmax), **kw)


def run_get(h, prm, seed, geom=False):
    planes = np.empty((h.H, h.W, 4), np.float32)
    costs = np.empty((h.H, h.W), np.float32)
    g = np.empty((h.H, h.W), np.float32) if geom else None
    h.run_into(prm, seed, planes, costs, g)
    return {"planes": planes, "costs": costs, "sel": h.get_selected_views(), **({"geom": g} if geom else {})}


def assert_same_results(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape, f"{what}: {k} shape"
        assert np.array_equal(a[k], b[k], equal_nan=(a[k].dtype.kind == "f")), f"{what}: {k} differs on {int((a[k] != b[k]).sum())} elements"


def both_entries(engine, hostlib, cams, bytes_, prm, seed=SEED, force_f32=False, overwrite=False):
    """-> (context filled by set_views_u8, context filled by set_views with F_i, their results of one Run())"""
    F = equivalent_floats(hostlib, cams, bytes_)
    a, b = engine.create(0), engine.create(0)
    if force_f32:
        a.set_texture_format(True)
        b.set_texture_format(True)
    mine = [x.copy() for x in bytes_]
    a.set_views_u8(cams, mine)
    if overwrite:   # the bytes were read before the call returned
        for x in mine:
            x[...] = 255 - x
    b.set_views(cams, F)
    assert (a.H, a.W, a.n_img) == (b.H, b.W, b.n_img)
    assert a.texture_format() == b.texture_format()
    ra, rb = run_get(a, prm, seed), run_get(b, prm, seed)
    return a, b, ra, rb


@pytest.fixture(scope="module")
def scene160(pm):
    sc = pm.synth.make_problem_scene(160, 120, n_src=3, spacing=0.4, quantize=True)
    return sc.problem(0, [1, 2, 3])


def test_entry_nothing_resampled_takes_u8_texels_and_equals_oracle(pm, oracle, engine, hostlib, scene160):
    cams, imgs = scene160
    prm = params_for(pm, cams, max_scale=1)
    a, b, ra, rb = both_entries(engine, hostlib, cams, to_bytes(imgs), prm)
    assert a.texture_format() == "u8"
    assert_same_results(ra, rb, "bytes at the cameras' size")
    cpu = oracle.create()
    cpu.set_views(cams, imgs)
    cpu.run(prm, SEED)
    cp, cc = cpu.get()
    assert_same_results(ra, {"planes": cp, "costs": cc, "sel": cpu.get_selected_views()}, "against the oracle")


def test_entry_all_views_shrunk(pm, engine, hostlib, scene160):
    """160 x 120 -> 100 x 75, the case of test_oversized_images_are_shrunk_once_and_k_follows"""
    cams, imgs = scene160
    small = [scaled_cam(c, 100, 75) for c in cams]
    prm = params_for(pm, small, max_scale=1)
    a, b, ra, rb = both_entries(engine, hostlib, small, to_bytes(imgs), prm)
    assert a.texture_format() == "f32" and (a.H, a.W) == (75, 100)
    assert_same_results(ra, rb, "all views shrunk")
    assert np.isfinite(ra["planes"]).all() and (ra["costs"] < 2.0).mean() > 0.5, "a real reconstruction, not an empty one"


@pytest.mark.parametrize("which", ["reference", "sources"])
def test_entry_reference_or_sources_shrunk(pm, engine, hostlib, scene160, which):
    """only the reference image resampled (the sources keep the 8-byte texels), and only the sources (the reference image is
    padded from its bytes, all sources take fp32 texels)"""
    cams, imgs = scene160
    F_small = [hostlib.resize_linear(im, 100, 75) for im in imgs]
    b_small = [np.clip(np.rint(f), 0, 255).astype(np.uint8) for f in F_small]     # 8-bit images at the small size
    shrink = [which == "reference"] + [which == "sources"] * 3
    use_cams = [scaled_cam(c, 100, 75) for c in cams]
    bytes_ = [full if s else sm for s, full, sm in zip(shrink, to_bytes(imgs), b_small)]
    prm = params_for(pm, use_cams, max_scale=1)
    a, b, ra, rb = both_entries(engine, hostlib, use_cams, bytes_, prm)
    assert a.texture_format() == ("u8" if which == "reference" else "f32")
    assert_same_results(ra, rb, which + " shrunk")


def test_entry_sources_of_different_source_sizes(pm, engine, hostlib, scene160):
    """one Problem whose sources come at 160 x 120, at 200 x 150 and at the running size 100 x 75 (the one that is not resampled
    takes fp32 texels with the others)"""
    cams, imgs = scene160
    big = pm.synth.make_problem_scene(200, 150, n_src=3, spacing=0.4, quantize=True)   # the same cameras at another resolution
    bcams, bimgs = big.problem(0, [1, 2, 3])
    use_cams = [scaled_cam(cams[0], 100, 75), scaled_cam(cams[1], 100, 75), scaled_cam(bcams[2], 100, 75), scaled_cam(cams[3], 100, 75)]
    b3 = np.clip(np.rint(hostlib.resize_linear(imgs[3], 100, 75)), 0, 255).astype(np.uint8)
    bytes_ = [to_bytes(imgs)[0], to_bytes(imgs)[1], to_bytes(bimgs)[2], b3]
    assert [x.shape for x in bytes_] == [(120, 160), (120, 160), (150, 200), (75, 100)]
    prm = params_for(pm, use_cams, max_scale=1)
    a, b, ra, rb = both_entries(engine, hostlib, use_cams, bytes_, prm)
    assert a.texture_format() == "f32"
    assert_same_results(ra, rb, "mixed source sizes")


def test_entry_fp32_forced(pm, engine, hostlib, scene160):
    cams, imgs = scene160
    prm = params_for(pm, cams, max_scale=1)
    a, b, ra, rb = both_entries(engine, hostlib, cams, to_bytes(imgs), prm, force_f32=True)
    assert a.texture_format() == "f32"
    assert_same_results(ra, rb, "fp32 forced, nothing resampled")
    small = [scaled_cam(c, 100, 75) for c in cams]
    prm = params_for(pm, small, max_scale=1)
    a, b, ra, rb = both_entries(engine, hostlib, small, to_bytes(imgs), prm, force_f32=True)
    assert_same_results(ra, rb, "fp32 forced, all views shrunk")


def test_entry_geometric_pass_on_shrunk_views(pm, engine, hostlib, scene160):
    """a geometric-consistency Run() with source depth maps on top of the photometric one, all views shrunk"""
    cams, imgs = scene160
    sc = pm.synth.make_problem_scene(160, 120, n_src=3, spacing=0.4, quantize=True)
    small = [scaled_cam(c, 100, 75) for c in cams]
    prm = params_for(pm, small, max_scale=1)
    a, b, ra, rb = both_entries(engine, hostlib, small, to_bytes(imgs), prm)
    assert_same_results(ra, rb, "photometric")
    rng = np.random.default_rng(11)
    depths = [hostlib.resize_linear(sc.views[i].gt_depth, 100, 75) * (1.0 + 0.005 * rng.standard_normal((75, 100))).astype(np.float32) for i in (1, 2, 3)]
    prm.geom_consistency = True
    prm.max_iterations = 2
    for h in (a, b):
        h.set_src_depths(depths)
    ga, gb = run_get(a, prm, SEED + 1, geom=True), run_get(b, prm, SEED + 1, geom=True)
    assert_same_results(ga, gb, "geometric")
    assert not np.array_equal(ga["planes"], ra["planes"])


def test_entry_reads_the_bytes_before_it_returns(pm, engine, hostlib, scene160):
    """the caller's arrays are overwritten right after set_views_u8 has returned (the uploads are still only enqueued)"""
    cams, imgs = scene160
    prm = params_for(pm, cams, max_scale=1)
    a, b, ra, rb = both_entries(engine, hostlib, cams, to_bytes(imgs), prm, overwrite=True)
    assert_same_results(ra, rb, "nothing resampled, bytes overwritten")
    small = [scaled_cam(c, 100, 75) for c in cams]
    prm = params_for(pm, small, max_scale=1)
    a, b, ra, rb = both_entries(engine, hostlib, small, to_bytes(imgs), prm, overwrite=True)
    assert_same_results(ra, rb, "all views shrunk, bytes overwritten")


def test_entry_honours_row_strides(pm, engine, hostlib, scene160):
    cams, imgs = scene160
    small = [scaled_cam(c, 100, 75) for c in cams]
    prm = params_for(pm, small, max_scale=1)
    wide = []
    for x in to_bytes(imgs):
        w = np.full((120, 192), 77, np.uint8)
        w[:, 16:176] = x
        wide.append(w[:, 16:176])
    F = equivalent_floats(hostlib, small, to_bytes(imgs))
    a, b = engine.create(0), engine.create(0)
    a.set_views_u8(small, wide)
    b.set_views(small, F)
    assert_same_results(run_get(a, prm, SEED), run_get(b, prm, SEED), "strided bytes")


_CHILD = """
import importlib, sys
import numpy as np
sys.path.insert(0, {root!r})
pm = importlib.import_module("mp-mvs_amd")
engine = importlib.import_module("mp-mvs_amd.engine")
z = np.load({inp!r})
n = int(z["n"])
cams = [pm.Camera.from_buffer_copy(z[f"cam{{i}}"].tobytes()) for i in range(n)]
bytes_ = [z[f"img{{i}}"] for i in range(n)]
prm = pm.PatchMatchParams.from_buffer_copy(z["prm"].tobytes())
h = engine.create(0)
h.set_views_u8(cams, bytes_)
planes = np.empty((h.H, h.W, 4), np.float32)
costs = np.empty((h.H, h.W), np.float32)
h.run_into(prm, int(z["seed"]), planes, costs)
np.savez({out!r}, planes=planes, costs=costs, sel=h.get_selected_views(), fmt=np.array(h.texture_format()))
"""


def _in_child_with_stage_mb(tmp_path, cams, bytes_, prm, name):
    inp, out = str(tmp_path / (name + "_in.npz")), str(tmp_path / (name + "_out.npz"))
    np.savez(inp, n=len(cams), seed=SEED, prm=np.frombuffer(bytes(prm), np.uint8),
             **{f"cam{i}": np.frombuffer(bytes(c), np.uint8) for i, c in enumerate(cams)}, **{f"img{i}": b for i, b in enumerate(bytes_)})
    env = dict(os.environ, MPMVS_STAGE_MB="1")
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(_CHILD.format(root=ROOT, inp=inp, out=out))], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    z = np.load(out)
    return {"planes": z["planes"], "costs": z["costs"], "sel": z["sel"]}, str(z["fmt"])


def test_entry_grouped_staging(pm, engine, hostlib, scene160, tmp_path):
    """MPMVS_STAGE_MB=1 in a fresh process (the variable is read per call; a fresh process keeps it away from everything else):
    the 160 x 120 -> 100 x 75 Problem, and one whose source bytes exceed the limit -- 4 views of 800 x 600 bytes go through the
    1 MB stage in groups of two -- against mpmvs_set_views on F_i in this process."""
    cams, imgs = scene160
    small = [scaled_cam(c, 100, 75) for c in cams]
    prm = params_for(pm, small, max_scale=1)
    got, fmt = _in_child_with_stage_mb(tmp_path, small, to_bytes(imgs), prm, "small")
    b = engine.create(0)
    b.set_views(small, equivalent_floats(hostlib, small, to_bytes(imgs)))
    assert fmt == b.texture_format() == "f32"
    assert_same_results(got, run_get(b, prm, SEED), "grouped staging, 160 x 120")

    sc = pm.synth.make_problem_scene(800, 600, n_src=3, spacing=0.4, quantize=True)
    cams, imgs = sc.problem(0, [1, 2, 3])
    small = [scaled_cam(c, 500, 375) for c in cams]
    prm = params_for(pm, small, max_scale=0, max_iterations=1)
    assert sum(im.size for im in imgs) > 1 << 20
    got, fmt = _in_child_with_stage_mb(tmp_path, small, to_bytes(imgs), prm, "large")
    b.set_views(small, equivalent_floats(hostlib, small, to_bytes(imgs)))
    assert_same_results(got, run_get(b, prm, SEED), "grouped staging, 800 x 600")


# ---------------------------------------------------------------------------
# 6: errors
# ---------------------------------------------------------------------------
def test_entry_errors_are_reported_and_leave_the_context_usable(pm, engine, hostlib, scene160):
    cams, imgs = scene160
    bytes_ = to_bytes(imgs)
    n = len(cams)
    _, fns = engine.load()
    h = engine.create(0)
    cam_arr = (pm.Camera * n)(*cams)

    def call(n_views, images, ws, hs, pitches):
        ptrs = (C.POINTER(C.c_ubyte) * n)(*[im.ctypes.data_as(C.POINTER(C.c_ubyte)) if im is not None else None for im in images])
        rc = fns["set_views_u8"](h._ctx, n_views, cam_arr, ptrs, (C.c_int * n)(*ws), (C.c_int * n)(*hs), (C.c_size_t * n)(*pitches))
        return rc, fns["last_error"](h._ctx)

    ok_w, ok_h, ok_p = [160] * n, [120] * n, [160] * n
    bad = {
        "NULL image": call(n, [bytes_[0], None] + bytes_[2:], ok_w, ok_h, ok_p),
        "pitch < width": call(n, bytes_, ok_w, ok_h, [160, 159, 160, 160]),
        "zero source width": call(n, bytes_, [160, 160, 0, 160], ok_h, ok_p),
        "zero source height": call(n, bytes_, ok_w, [0] + [120] * (n - 1), ok_p),
        "n < 2": call(1, bytes_, ok_w, ok_h, ok_p),
    }
    for what, (rc, msg) in bad.items():
        assert rc < 0, what
        assert msg, what + ": empty mpmvs_last_error"
    with pytest.raises(RuntimeError, match="set_views"):
        h.run(params_for(pm, cams), 1)      # none of them left a Problem behind
    prm = params_for(pm, cams, max_scale=1)
    h.set_views_u8(cams, bytes_)
    ref = engine.create(0)
    ref.set_views(cams, imgs)
    assert_same_results(run_get(h, prm, SEED), run_get(ref, prm, SEED), "valid Problem after the refused ones")


def test_resize_probe_refuses_bad_arguments(engine):
    _, fns = engine.load()
    b = np.zeros((4, 4), np.uint8)
    out = np.zeros((2, 2), np.float32)
    assert fns["resize_u8"](0, b.ctypes.data, 4, 4, 3, 2, 2, out.ctypes.data) < 0      # pitch < width
    assert fns["resize_u8"](0, b.ctypes.data, 0, 4, 4, 2, 2, out.ctypes.data) < 0
    assert fns["resize_u8"](0, b.ctypes.data, 4, 4, 4, 0, 2, out.ctypes.data) < 0
    assert fns["resize_u8"](0, None, 4, 4, 4, 2, 2, out.ctypes.data) < 0


# ---------------------------------------------------------------------------
# 7: the folder pipeline
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["pgm", "jpg"])
def test_folder_pipeline_bytes_equal_host_float_images(pm, engine, hostlib, tmp_path, fmt):
    """A folder of oversized views (160 x 120, max_image_size 100 -> 100 x 75) through the pass schedule: the Scenes keep the
    decoded bytes and the device shrinks them (the default) against MPMVS_HOST_FLOAT_IMAGES=1, which widens them, shrinks them
    with the host's ResizeLinear and takes mpmvs_set_views as before.  Two geometric passes follow the photometric one: they
    adopt the contexts the pass before left resident, which are recognised by the byte buffers they were filled from."""
    sc, neigh = pm.synth.make_grid_scene(160, 120, 3, 2, spacing=0.4, rot_deg=1.0, quantize=True)
    cams = [v.cam for v in sc.views]
    imgs = [v.image for v in sc.views]
    hostlib.write_dataset(str(tmp_path), cams, imgs, neigh, fmt=fmt)
    kw = dict(devices=(0,), workers=2, geom_iterations=2, planar_prior=True, geom_planar_prior=True, max_scale=1, seed=321, max_image_size=100)
    assert "MPMVS_HOST_FLOAT_IMAGES" not in os.environ
    got = hostlib.run_folder_jacobi_in_memory(tmp_path, 6, 75, 100, **kw)
    os.environ["MPMVS_HOST_FLOAT_IMAGES"] = "1"
    try:
        want = hostlib.run_folder_jacobi_in_memory(tmp_path, 6, 75, 100, **kw)
    finally:
        del os.environ["MPMVS_HOST_FLOAT_IMAGES"]
    for name, g, w in zip(("depths", "normals", "costs"), got, want):
        assert np.array_equal(g, w), f"{name}: {int((g != w).sum())} elements differ"
    assert np.isfinite(got[0]).all() and (got[0] > 0).all()
    gt = hostlib.resize_linear(sc.views[0].gt_depth, 100, 75)
    assert (np.abs(got[0][0] - gt) / gt < 0.05).mean() > 0.7, "a real reconstruction"
