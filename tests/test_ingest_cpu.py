"""CPU side of the 8-bit image entry (include/mpmvs.h: mpmvs_set_views_u8, mpmvs_resize_u8): the fixture that the GPU probe is
held against, replayed through the host statement of the resampling, and what can be said about the entry without a device."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_byte_fixture_replays_through_host_resize_linear(hostlib):
    """tests/golden/resize_u8_golden_v1.npz (tests/golden/make_resize_u8_golden.py: torch bilinear, align_corners=False, no
    antialias, float64, computed without this repository) against ResizeLinear on the widened bytes -- the definition of what
    mpmvs_resize_u8 computes.  Tolerance: 1e-5 of the 0..255 range, as test_resize_linear_equals_independent_fixture.  If this
    passes and the GPU replay (test_ingest_gpu.py) fails, the kernel is wrong, not the fixture."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "resize_u8_golden_v1.npz"))
    assert int(z["n"]) >= 4
    for k in range(int(z["n"])):
        src, want, mx = z[f"src{k}"], z[f"dst{k}"], int(z[f"max{k}"])
        assert src.dtype == np.uint8 and want.dtype == np.float32
        rows, cols = src.shape
        f = min(np.float32(mx) / np.float32(cols), np.float32(mx) / np.float32(rows))
        new_cols, new_rows = int(np.floor(np.float32(cols) * f + np.float32(0.5))), int(np.floor(np.float32(rows) * f + np.float32(0.5)))
        assert (new_rows, new_cols) == want.shape
        got = hostlib.resize_linear(src.astype(np.float32), new_cols, new_rows)
        err = np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
        assert err <= 255.0 * 1e-5, f"case {k}: max |difference| {err}"


def test_identity_size_resampling_returns_the_bytes(hostlib):
    """the contract's F_i = (float)bytes for equal sizes is what the formula gives as well: ratio 1 puts every sample on a pixel"""
    b = np.random.default_rng(1).integers(0, 256, (37, 53), dtype=np.uint8)
    assert np.array_equal(hostlib.resize_linear(b.astype(np.float32), 53, 37), b.astype(np.float32))


def test_byte_entry_is_exported_and_bound(pm):
    """the symbols are in the library, in engine.ALL_SYMBOLS, and bound with the signatures of include/mpmvs.h"""
    import importlib
    engine = importlib.import_module("mp-mvs_amd.engine")
    lib, fns = engine.load()
    for name in ("mpmvs_set_views_u8", "mpmvs_resize_u8"):
        assert name in engine.ALL_SYMBOLS
        assert hasattr(lib, name)
    assert len(fns["set_views_u8"].argtypes) == 7 and len(fns["resize_u8"].argtypes) == 8
    header = open(os.path.join(ROOT, "include", "mpmvs.h")).read()
    assert "int mpmvs_set_views_u8(" in header and "int mpmvs_resize_u8(" in header
    assert callable(getattr(engine.HipPatchMatch, "set_views_u8")) and callable(engine.resize_u8)


def test_probe_refuses_bad_arguments_before_it_touches_a_device(pm):
    """argument checks come first: these return without a HIP call, so they hold on a machine without a GPU"""
    import importlib
    engine = importlib.import_module("mp-mvs_amd.engine")
    _, fns = engine.load()
    b = np.zeros((4, 4), np.uint8)
    out = np.zeros((2, 2), np.float32)
    assert fns["resize_u8"](0, b.ctypes.data, 4, 4, 3, 2, 2, out.ctypes.data) == -2      # pitch < width
    assert fns["resize_u8"](0, b.ctypes.data, 0, 4, 4, 2, 2, out.ctypes.data) == -2
    assert fns["resize_u8"](0, b.ctypes.data, 4, 4, 4, 2, 0, out.ctypes.data) == -2
    assert fns["resize_u8"](0, None, 4, 4, 4, 2, 2, out.ctypes.data) == -2
    assert fns["resize_u8"](0, b.ctypes.data, 1 << 16, 1 << 16, 0, 2, 2, out.ctypes.data) == -3   # 2^32 source bytes
