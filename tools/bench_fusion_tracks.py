#!/usr/bin/env python3
"""What the tracks cost: mpmvs_fuse_ply against mpmvs_fuse_ply_tracks on 8 synthetic views of 1600 x 1200 with 7 sources each,
snapshot formulation and reference order, in one process, warmed, the variants alternating round by round.  Per variant the
device time of the kernels and copies between the call's events (mpmvs_fuse_kernel_ms) and the wall time of the Python call,
as median [min, max] over the rounds, and the bytes the track path moves in addition.

  tools/bench_fusion_tracks.py [--rounds 7] [--baseline-lib build/libmpmvs_hip_parent.so] [--out FILE]

--baseline-lib: another build of the library (the parent commit's) whose mpmvs_fuse_ply joins the alternation: the plain path
must not have become slower, i.e. differ by no more than the baseline's own spread."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def fuse_ply_with(lib, fusion, *args, **kw):
    """fusion.fuse_ply through the mpmvs_fuse_ply of a given build of the library"""
    fn = lib.mpmvs_fuse_ply
    fn.argtypes = [C.c_int] + fusion.FUSE_ARGTYPES_TAIL[:-3] + [C.POINTER(C.POINTER(C.c_ubyte)), C.POINTER(C.POINTER(C.c_ubyte))]
    fn.restype = C.c_longlong
    lib.mpmvs_free.argtypes = [C.c_void_p]
    lib.mpmvs_free.restype = None
    lib.mpmvs_fuse_kernel_ms.restype = C.c_float
    out = {}

    def call(*a):
        rec = C.POINTER(C.c_ubyte)()
        count = fn(*a[:-3], C.byref(rec), a[-1])
        if count < 0:
            return int(count)
        out["records"] = np.ctypeslib.as_array(rec, shape=(count, 27)).copy()
        lib.mpmvs_free(rec)
        return 0

    fusion.call_fuse(call, (0,), *args, **kw)
    return out["records"], float(lib.mpmvs_fuse_kernel_ms())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pm = importlib.import_module("mp-mvs_amd")
    fusion = importlib.import_module("mp-mvs_amd.fusion")
    engine = importlib.import_module("mp-mvs_amd.engine")
    from test_fusion_cpu import _scene
    sc, cams, depths, normals, grays, neigh = _scene(pm, n_grid=(4, 2), size=(1600, 1200))
    cols = [np.stack([g, 255 - g, g // 2], -1).astype(np.uint8) for g in (np.asarray(x).astype(np.uint8) for x in grays)]
    args = (cams, [True] * 8, depths, normals, cols, neigh)
    lib, _ = engine.load()
    base = engine.load_variant(os.path.abspath(a.baseline_lib))[0] if a.baseline_lib else None
    result = {"images": 8, "size": [1600, 1200], "sources": len(neigh[0]), "rounds": a.rounds}
    for ref in (False, True):
        kw = dict(reference_order=ref)
        variants = {"fuse_ply": lambda: fuse_ply_with(lib, fusion, *args, **kw)}
        if base is not None:
            variants["fuse_ply_baseline_build"] = lambda: fuse_ply_with(base, fusion, *args, **kw)

        def tracks():
            r = fusion.fuse_ply_tracks(*args, **kw)
            tracks.last = r
            return r[0], fusion.last_kernel_ms()
        variants["fuse_ply_tracks"] = tracks
        times = {k: {"kernel_ms": [], "wall_ms": []} for k in variants}
        records = {}
        for rnd in range(a.rounds + 1):            # round 0 warms every variant
            for name, fn in variants.items():
                t0 = time.perf_counter()
                rec, kms = fn()
                wall = (time.perf_counter() - t0) * 1e3
                records[name] = rec
                if rnd:
                    times[name]["kernel_ms"].append(kms)
                    times[name]["wall_ms"].append(wall)
        _, off, img, pix, _ = tracks.last
        mode = {"points": int(len(records["fuse_ply"])), "entries": int(off[-1]),
                "records_equal": all(np.array_equal(r, records["fuse_ply"]) for r in records.values()),
                # per point an int64 offset, per entry two int32 to the host; on the device per pixel the slot bits, the length and
                # its scan (3 x 4 B written, read once more), per accepted pixel and used slot the source pixel (snapshot only)
                "extra_bytes_to_host": int(8 * (len(off)) + 8 * off[-1])}
        for name, t in times.items():
            mode[name] = {k: {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3), "max": round(float(np.max(v)), 3)} for k, v in t.items()}
        if ref:
            mode["passes"] = fusion.fuse_passes()
        result["reference_order" if ref else "snapshot"] = mode
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
