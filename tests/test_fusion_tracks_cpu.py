"""COLMAP's point-visibility file (fused.ply.vis) as mp-mvs_amd/fusion.py writes and reads it: little endian, uint64 number of
points, then per point uint32 k and k x uint32 image index.  No GPU involved."""
import importlib
import struct

import numpy as np
import pytest

# three points with tracks of 2, 3 and 2 images
OFF = np.array([0, 2, 5, 7], np.int64)
IMG = np.array([0, 3, 0, 4, 1, 2, 0], np.int32)


def test_write_vis_bytes(pm, tmp_path):
    fusion = importlib.import_module("mp-mvs_amd.fusion")
    p = tmp_path / "fused.ply.vis"
    fusion.write_vis(p, OFF, IMG)
    assert p.read_bytes() == struct.pack("<Q", 3) + struct.pack("<3I", 2, 0, 3) + struct.pack("<4I", 3, 0, 4, 1) + struct.pack("<3I", 2, 2, 0)
    # an empty cloud is the count alone
    fusion.write_vis(p, np.zeros(1, np.int64), np.zeros(0, np.int32))
    assert p.read_bytes() == struct.pack("<Q", 0) and len(p.read_bytes()) == 8
    with pytest.raises(ValueError):
        fusion.write_vis(p, np.array([0, 2, 5]), IMG)          # offsets that do not end at the number of entries


def test_read_vis_round_trip(pm, tmp_path):
    fusion = importlib.import_module("mp-mvs_amd.fusion")
    p = tmp_path / "fused.ply.vis"
    fusion.write_vis(p, OFF, IMG)
    off, img = fusion.read_vis(p)
    assert off.dtype == np.int64 and img.dtype == np.int32 and np.array_equal(off, OFF) and np.array_equal(img, IMG)
    fusion.write_vis(p, np.zeros(1, np.int64), np.zeros(0, np.int32))
    off, img = fusion.read_vis(p)
    assert off.tolist() == [0] and len(img) == 0
    # a larger random file, and files that are cut short or too long
    rng = np.random.default_rng(5)
    length = rng.integers(2, 34, 500)
    big_off = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
    big_img = rng.integers(0, 1000, int(big_off[-1])).astype(np.int32)
    fusion.write_vis(p, big_off, big_img)
    off, img = fusion.read_vis(p)
    assert np.array_equal(off, big_off) and np.array_equal(img, big_img)
    raw = p.read_bytes()
    for bad in (raw[:-4], raw + b"\0\0\0\0", raw[:6]):
        p.write_bytes(bad)
        with pytest.raises(ValueError):
            fusion.read_vis(p)


def test_write_vis_image_ids(pm, tmp_path):
    """image_ids[our index] is the number written (a converter that numbered the images differently)"""
    fusion = importlib.import_module("mp-mvs_amd.fusion")
    p = tmp_path / "fused.ply.vis"
    ids = [11, 12, 15, 20, 31]
    fusion.write_vis(p, OFF, IMG, image_ids=ids)
    assert p.read_bytes() == struct.pack("<Q", 3) + struct.pack("<3I", 2, 11, 20) + struct.pack("<4I", 3, 11, 31, 12) + struct.pack("<3I", 2, 15, 11)
    off, img = fusion.read_vis(p)
    assert np.array_equal(off, OFF) and img.tolist() == [ids[k] for k in IMG]


def test_tracks_entry_is_declared_and_exported(pm):
    """mpmvs_fuse_ply_tracks is in the header, in both libraries and in engine.ALL_SYMBOLS; the host library exports the folder form"""
    engine = importlib.import_module("mp-mvs_amd.engine")
    hostlib = importlib.import_module("mp-mvs_amd.hostlib")
    assert "mpmvs_fuse_ply_tracks" in engine.ALL_SYMBOLS
    lib, _ = engine.load()
    lib_q8, _ = engine.load_variant(engine.LIB_Q8_PATH)
    assert hasattr(lib, "mpmvs_fuse_ply_tracks") and hasattr(lib_q8, "mpmvs_fuse_ply_tracks")
    assert "mpmvs_host_fuse_folder_vis" in hostlib.SYMBOLS and hasattr(hostlib.load(), "mpmvs_host_fuse_folder_vis")
