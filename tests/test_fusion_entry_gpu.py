"""The five fusion entry points (mpmvs_fuse, _fuse_ctx, _fuse_ply, _fuse_ply_ctx, _fuse_ply_tracks; include/mpmvs.h) through the raw
ctypes handle: every refusal returns its code and writes nothing (csrc/pm_fusion_host.hpp, fuse_check_request; the entry points'
own NULL checks), and the forms that are one another agree byte for byte.  Three images of 33 x 9: one column over k_fuse's
32 x 8 tile and one row over."""
import ctypes as C
import importlib

import numpy as np
import pytest

from test_fusion_cpu import _scene

pytestmark = pytest.mark.gpu

W, H, N = 33, 9, 3
SLOTS = 33                      # pm_fusion.hpp: kMaxFuseNgb
FORMS = ("fuse", "fuse_ctx", "ply", "ply_ctx", "ply_tracks")
SENTINEL, STALE = 0xA5, 0xDEAD0  # the fill of the output arrays; the value of the out pointers, never followed
GOOD = [[0, 1, 2], [1, 0, 2], [2, 1]]
_cache = {}


def _images(pm):
    if "in" not in _cache:
        fusion = importlib.import_module("mp-mvs_amd.fusion")
        _, cams, depths, normals, grays, _ = _scene(pm, n_grid=(N, 1), size=(W, H))
        _cache["in"] = (cams, [np.ascontiguousarray(d, np.float32) for d in depths], [np.ascontiguousarray(x, np.float32) for x in normals],
                        [fusion._as_u8(g) for g in grays])
    return _cache["in"]


def _call(engine, pm, form, lists=GOOD, estimate=None, flags=1, *, n=None, channels=1, size=None, off=None, null=()):
    """One raw call.  lists: the complete view lists (image k's own data is image k % 3's); off: the offsets to hand over instead of
    those of `lists`; size: (w, h) written into every camera; null: names of pointer arguments to pass as NULL.
    Returns rc and everything the call could have written."""
    lib, _ = engine.load()
    cams3, depths, normals, grays = _images(pm)
    m = len(lists)                                   # images there are arrays for
    n = m if n is None else n
    Camera = type(cams3[0])
    cams = (Camera * max(m, 1))()
    for k in range(m):
        C.memmove(C.byref(cams[k]), C.byref(cams3[k % N]), C.sizeof(Camera))
        if size is not None:
            cams[k].width, cams[k].height = size
    ids = [s for l in lists for s in l]
    off = list(np.cumsum([0] + [len(l) for l in lists])) if off is None else off
    est = [1] * m if estimate is None else [int(e) for e in estimate]
    fptr = lambda arrs: (C.c_void_p * max(m, 1))(*[arrs[k % N].ctypes.data for k in range(m)])
    valid = [np.full((H, W), SENTINEL, np.uint8) for _ in range(m)]
    pts = [np.full((H, W, 9), np.float32(-7.5)) for _ in range(m)]
    masks = [np.full((H, W), SENTINEL, np.uint8) for _ in range(m)]
    optr = lambda arrs: (C.c_void_p * max(m, 1))(*[a.ctypes.data for a in arrs])
    a = dict(cams=cams, estimate=(C.c_int * max(m, 1))(*est), depths=fptr(depths), normals=fptr(normals), colors=fptr(grays),
             src_off=(C.c_int * len(off))(*[int(o) for o in off]), src_ids=(C.c_int * max(len(ids), 1))(*ids),
             out_valid=optr(valid), out_points9=optr(pts), out_masks=optr(masks))
    ptrs = {k: C.c_void_p(STALE) for k in ("records", "track_off", "track_image", "track_pixel")}
    a.update({k: C.byref(v) for k, v in ptrs.items()})
    for k in null:
        a[k] = None
    ctx = (None,) if form in ("fuse_ctx", "ply_ctx", "ply_tracks") else ()
    head = (0, n, a["cams"], a["estimate"], *ctx, a["depths"], a["normals"], a["colors"], channels, None, a["src_off"], a["src_ids"], flags)
    tail = {"fuse": ("out_valid", "out_points9", "out_masks"), "fuse_ctx": ("out_valid", "out_points9", "out_masks"), "ply": ("records", "out_masks"),
            "ply_ctx": ("records", "out_masks"), "ply_tracks": ("records", "track_off", "track_image", "track_pixel", "out_masks")}[form]
    fn = getattr(lib, "mpmvs_fuse" + {"fuse": "", "fuse_ctx": "_ctx", "ply": "_ply", "ply_ctx": "_ply_ctx", "ply_tracks": "_ply_tracks"}[form])
    fn.restype = C.c_int if form in ("fuse", "fuse_ctx") else C.c_longlong
    fn.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 2 + [C.c_void_p] * len(ctx) + [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + \
                  [C.c_void_p] * len(tail)
    rc = int(fn(*head, *[a[k] for k in tail]))
    r = dict(rc=rc, valid=valid, pts=pts, masks=masks, ptrs={k: v.value for k, v in ptrs.items()}, written=tail)
    if rc >= 0 and "records" in tail:
        lib.mpmvs_free.argtypes, lib.mpmvs_free.restype = [C.c_void_p], None
        r["records"] = C.string_at(ptrs["records"].value, rc * 27)
        if form == "ply_tracks":
            r["off"] = np.frombuffer(C.string_at(ptrs["track_off"].value, (rc + 1) * 8), np.int64)
            r["entries"] = C.string_at(ptrs["track_image"].value, int(r["off"][-1]) * 4) + C.string_at(ptrs["track_pixel"].value, int(r["off"][-1]) * 4)
        for k in tail:
            if k != "out_masks":
                lib.mpmvs_free(ptrs[k].value)
    return r


def _untouched(r):
    """nothing the call was handed has been written"""
    return (all((x == SENTINEL).all() for x in r["valid"] + r["masks"]) and all((p == np.float32(-7.5)).all() for p in r["pts"]) and
            all(v == STALE for v in r["ptrs"].values()))


WIDE = [list(range(SLOTS))] + [[k] for k in range(1, SLOTS + 1)]              # 34 images, image 0 with 33 slots
WIDER = [list(range(SLOTS + 1))] + [[k] for k in range(1, SLOTS + 1)]         # ... with 34
# name, code, keyword arguments of _call: the table of tools/fuse_lists_check.cpp, here through every entry point
REFUSED = [
    ("n = 0", -1, dict(n=0)),
    ("channels 2", -1, dict(channels=2)),
    ("src_off NULL", -2, dict(null=("src_off",))),
    ("src_ids NULL", -2, dict(null=("src_ids",))),
    ("src_off[0] = 1", -2, dict(off=[1, 3, 6, 8])),
    ("descending offsets", -2, dict(off=[0, 3, 2, 8])),
    ("a list that does not start with its own image", -2, dict(lists=[[0, 1, 2], [0, 2], [2, 1]])),
    ("an estimated image with an empty list", -2, dict(lists=[[0, 1, 2], [], [2, 1]])),
    ("kMaxFuseNgb + 1 slots", -2, dict(lists=WIDER, estimate=[1] + [0] * SLOTS)),
    ("id -1", -2, dict(lists=[[0, 1, 2], [1, -1], [2, 1]])),
    ("id n", -2, dict(lists=[[0, 1, 2], [1, 3], [2, 1]])),
    ("an id twice", -2, dict(lists=[[0, 1, 2], [1, 0, 2, 0], [2, 1]])),
    ("the image itself among its sources", -2, dict(lists=[[0, 1, 2], [1, 0, 1], [2, 1]])),
    ("channels 2 and src_off NULL", -1, dict(channels=2, null=("src_off",))),
    ("n = 0 and src_ids NULL", -1, dict(n=0, null=("src_ids",))),
    # 46341 x 46341 pixels x 1 slot is past the int range of a track's offsets; the earlier codes still win
    ("past the track bound and an id twice", -2, dict(size=(46341, 46341), lists=[[0, 1, 1], [1, 0], [2, 1]])),
    ("past the track bound and channels 2", -1, dict(size=(46341, 46341), channels=2)),
]


@pytest.mark.parametrize("form", FORMS)
def test_refused_lists_return_their_code_and_write_nothing(pm, engine, form):
    for name, code, kw in REFUSED:
        for flags in (1, 3):
            r = _call(engine, pm, form, flags=flags, **kw)
            assert r["rc"] == code, (name, flags, r["rc"])
            assert _untouched(r), (name, flags)


def test_track_bound_is_refused_where_tracks_are_asked_for(pm, engine):
    """-3 from mpmvs_fuse_ply_tracks alone.  The forms without tracks accept such a request and would go on to allocate it, so their
    half of this row is checked on the host only (tools/fuse_lists_check.cpp)"""
    r = _call(engine, pm, "ply_tracks", size=(46341, 46341))
    assert r["rc"] == -3 and _untouched(r)
    r = _call(engine, pm, "ply_tracks", size=(46340, 46340), lists=[[0], [1, 0], [2]])     # 2 slots of 46340^2
    assert r["rc"] == -3 and _untouched(r)
    r = _call(engine, pm, "ply_tracks", size=(46341, 46341), null=("track_image",))       # the entry point's own check comes first
    assert r["rc"] == -2 and _untouched(r)


def test_null_outputs_are_refused_first(pm, engine):
    """the entry points' own checks: -1 for a missing output pointer, -2 for a missing track pointer, before the lists are read"""
    bad = dict(lists=[[0, 1, 1], [1, 0], [2, 1]])                     # would be -2
    for form in ("fuse", "fuse_ctx"):
        for k in ("out_valid", "out_points9", "out_masks"):
            for kw in ({}, bad, dict(n=0)):
                r = _call(engine, pm, form, null=(k,), **kw)
                assert r["rc"] == -1 and _untouched(r), (form, k, kw)
    for form in ("ply", "ply_ctx", "ply_tracks"):
        for kw in ({}, bad):
            r = _call(engine, pm, form, null=("records",), **kw)
            assert r["rc"] == -1 and _untouched(r), (form, kw)
    for k in ("track_off", "track_image", "track_pixel"):
        for kw in ({}, dict(n=0), dict(channels=2)):                  # -2 here wins over the request's -1: the pointers are checked first
            r = _call(engine, pm, "ply_tracks", null=(k,), **kw)
            assert r["rc"] == -2 and _untouched(r), (k, kw)
        r = _call(engine, pm, "ply_tracks", null=("records", k))
        assert r["rc"] == -1 and _untouched(r), k


@pytest.mark.parametrize("reference_order", [False, True], ids=["snapshot", "reference"])
def test_the_five_forms_agree_byte_for_byte(pm, engine, reference_order):
    flags = 1 | (2 if reference_order else 0)
    r = {form: _call(engine, pm, form, flags=flags) for form in FORMS}
    assert r["fuse"]["rc"] == 0 and r["fuse_ctx"]["rc"] == 0
    count = int(sum(v.sum() for v in r["fuse"]["valid"]))
    assert count > 100 and all(set(np.unique(v)) <= {0, 1} for v in r["fuse"]["valid"])
    for k in ("valid", "pts", "masks"):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(r["fuse"][k], r["fuse_ctx"][k])), k
    for form in ("ply", "ply_ctx", "ply_tracks"):
        assert r[form]["rc"] == count, form
        assert r[form]["records"] == r["ply"]["records"], form
        assert all(a.tobytes() == b.tobytes() for a, b in zip(r[form]["masks"], r["fuse"]["masks"])), form
        assert all((x == SENTINEL).all() for x in r[form]["valid"])               # not among this form's outputs
    fusion = importlib.import_module("mp-mvs_amd.fusion")
    cloud = np.concatenate([p[v.astype(bool)] for p, v in zip(r["fuse"]["pts"], r["fuse"]["valid"])], 0)
    assert fusion.ply_records(cloud).tobytes() == r["ply"]["records"]
    off = r["ply_tracks"]["off"]
    assert off[0] == 0 and (np.diff(off) >= 2).all() and len(r["ply_tracks"]["entries"]) == 8 * int(off[-1])


def test_accepted_ends(pm, engine):
    """an unestimated image with an empty list, and kMaxFuseNgb slots exactly, through every entry point"""
    for form in FORMS:
        r = _call(engine, pm, form, lists=[[0, 1, 2], [], [2, 1]], estimate=[1, 0, 1])
        assert r["rc"] >= 0, form
        r = _call(engine, pm, form, lists=WIDE, estimate=[1] + [0] * SLOTS)
        assert r["rc"] >= 0, form
        r = _call(engine, pm, form, lists=WIDER, estimate=[0, 1] + [0] * (SLOTS - 1))          # 34 slots on an image that is not estimated
        assert r["rc"] >= 0, form
