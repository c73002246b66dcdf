"""Depth-map fusion front end: marshals a scene into the flat C
signature shared by `mpmvs_fuse` (HIP, include/mpmvs.h) and, in tests, the oracle's
`orc_fuse`, and compacts the per-pixel outputs into the point list the reference
builds (reference src/PatchMatch.cpp:369-495: image order, then raster order)."""
import ctypes as C

import numpy as np

from ._abi import Camera

_PP_F = C.POINTER(C.POINTER(C.c_float))
_PP_U8 = C.POINTER(C.POINTER(C.c_ubyte))
FUSE_ARGTYPES_TAIL = [C.c_int, C.POINTER(Camera), C.POINTER(C.c_int), _PP_F, _PP_F, _PP_U8, C.c_int, _PP_U8, C.POINTER(C.c_int), C.POINTER(C.c_int),
                      C.c_int, _PP_U8, _PP_F, _PP_U8]


def _as_u8(x):
    x = np.asarray(x)
    return np.ascontiguousarray(x if x.dtype == np.uint8 else np.clip(np.rint(x), 0, 255).astype(np.uint8))


FUSE_DYNAMIC_CONSISTENCY, FUSE_REFERENCE_ORDER = 1, 2   # include/mpmvs.h


def call_fuse(fn, lead_args, cams, estimate, depths, normals, colors, sources, use_dynamic=True, sky=None, reference_order=False, ctxs=None, lists=None):
    """fn(*lead_args, n, cams, estimate, [ctxs,] depths, normals, colors, channels, sky, src_off, src_ids, use_dynamic, valid, points9, masks)
    colors[k]: HxW grey or HxWx3 B,G,R (8 bit; floats are rounded); sky: None or per image None / HxW uint8 mask;
    sources[k] = source-view ids of image k (without k itself).  ctxs (the *_ctx entry points): per image None or the HipPatchMatch
    handle whose last Run() estimated it -- depths[k] / normals[k] may then be None.  lists: the complete view lists exactly as
    the C entry takes them (own image included; `sources` is then not read) -- for callers that must hand over a malformed one.  Returns
    (points [M, 9] in image-then-raster order, valid list, masks list)."""
    n = len(cams)
    shapes = [(cams[k].height, cams[k].width) for k in range(n)]
    has_ctx = [ctxs is not None and ctxs[k] is not None for k in range(n)]
    d = [None if has_ctx[k] else np.ascontiguousarray(depths[k], np.float32) for k in range(n)]
    nm = [None if has_ctx[k] else np.ascontiguousarray(normals[k], np.float32) for k in range(n)]
    g = [_as_u8(x) for x in colors]
    cch = 3 if (n and g[0].ndim == 3) else 1
    for k in range(n):
        assert has_ctx[k] or (d[k].shape == shapes[k] and nm[k].shape == shapes[k] + (3,))
        assert g[k].shape == (shapes[k] + (3,) if cch == 3 else shapes[k])
    skyp = None
    if sky is not None:
        sk = [None if m is None else _as_u8(m) for m in sky]
        for k in range(n):
            assert sk[k] is None or sk[k].shape == shapes[k]
        skyp = (C.POINTER(C.c_ubyte) * n)(*[None if m is None else m.ctypes.data_as(C.POINTER(C.c_ubyte)) for m in sk])
    ids, off = [], [0]
    for k in range(n):
        ids += [int(s) for s in lists[k]] if lists is not None else [k] + list(sources[k])
        off.append(len(ids))
    valid = [np.zeros(sh, np.uint8) for sh in shapes]
    pts = [np.zeros(sh + (9,), np.float32) for sh in shapes]
    masks = [np.zeros(sh, np.uint8) for sh in shapes]
    fp = lambda arrs: (C.POINTER(C.c_float) * n)(*[None if a is None else a.ctypes.data_as(C.POINTER(C.c_float)) for a in arrs])
    up = lambda arrs: (C.POINTER(C.c_ubyte) * n)(*[a.ctypes.data_as(C.POINTER(C.c_ubyte)) for a in arrs])
    ctx_arg = () if ctxs is None else ((C.c_void_p * n)(*[None if c is None else c._ctx for c in ctxs]),)
    rc = fn(*lead_args, n, (Camera * n)(*cams), (C.c_int * n)(*[1 if e else 0 for e in estimate]), *ctx_arg, fp(d), fp(nm), up(g), cch, skyp,
            (C.c_int * (n + 1))(*off), (C.c_int * max(len(ids), 1))(*ids),
            (FUSE_DYNAMIC_CONSISTENCY if use_dynamic else 0) | (FUSE_REFERENCE_ORDER if reference_order else 0), up(valid), fp(pts), up(masks))
    if rc != 0:
        raise RuntimeError(f"fuse failed ({rc})")
    cloud = np.concatenate([p[v.astype(bool)] for p, v in zip(pts, valid)], 0) if n else np.zeros((0, 9), np.float32)
    return cloud, valid, masks


def fuse(cams, estimate, depths, normals, colors, sources, use_dynamic=True, device=0, sky=None, reference_order=False, lists=None):
    """fusion on the MI355X (mpmvs_fuse); reference_order: the reference's sequential masking order instead of the snapshot formulation"""
    from . import engine
    lib, _ = engine.load()
    fn = lib.mpmvs_fuse
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] + FUSE_ARGTYPES_TAIL
    return call_fuse(fn, (int(device),), cams, estimate, depths, normals, colors, sources, use_dynamic, sky, reference_order, lists=lists)


def fuse_ctx(cams, estimate, ctxs, depths, normals, colors, sources, use_dynamic=True, device=0, sky=None, reference_order=False, lists=None):
    """mpmvs_fuse_ctx: fusion of maps that are still resident in the contexts that estimated them (ctxs[k] a HipPatchMatch handle, or None
    and depths[k] / normals[k] host arrays)"""
    from . import engine
    lib, _ = engine.load()
    fn = lib.mpmvs_fuse_ctx
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] + FUSE_ARGTYPES_TAIL[:3] + [C.POINTER(C.c_void_p)] + FUSE_ARGTYPES_TAIL[3:]
    return call_fuse(fn, (int(device),), cams, estimate, depths, normals, colors, sources, use_dynamic, sky, reference_order, ctxs=ctxs, lists=lists)


def fuse_passes():
    """(total, max per image) fixpoint passes of the last reference_order call"""
    from . import engine
    lib, _ = engine.load()
    lib.mpmvs_fuse_passes.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.mpmvs_fuse_passes.restype = None
    a, b = C.c_int(0), C.c_int(0)
    lib.mpmvs_fuse_passes(C.byref(a), C.byref(b))
    return a.value, b.value


def ply_records(cloud):
    """[M, 9] points (x y z nx ny nz c0 c1 c2, colour B,G,R) -> [M, 27] uint8 PLY vertex records as the reference writes them
    (src/PatchMatch.cpp:145-198): non-finite coordinates zeroed, red green blue = (uchar)(int) of c2 c1 c0"""
    cloud = np.ascontiguousarray(cloud, np.float32)
    xyz = cloud[:, :3].copy()
    big = np.float32(3.402823466e+38)
    fin = (xyz[:, 0] < big) & (xyz[:, 0] > -big) & (xyz[:, 1] < big) & (xyz[:, 1] > -big) & (xyz[:, 2] < big) & (xyz[:, 2] >= -big)
    xyz[~fin] = 0
    rec = np.empty((len(cloud), 27), np.uint8)
    rec[:, :12] = xyz.view(np.uint8).reshape(-1, 12)
    rec[:, 12:24] = np.ascontiguousarray(cloud[:, 3:6]).view(np.uint8).reshape(-1, 12)
    rec[:, 24:27] = cloud[:, [8, 7, 6]].astype(np.int32).astype(np.uint8)
    return rec


def fuse_ply(cams, estimate, depths, normals, colors, sources, use_dynamic=True, device=0, sky=None, reference_order=False, ctxs=None, lists=None):
    """mpmvs_fuse_ply: fusion with device-side compaction; returns ([M, 27] uint8 PLY vertex records, masks list).
    With ctxs (per image a HipPatchMatch handle or None): mpmvs_fuse_ply_ctx, the resident maps are not uploaded"""
    from . import engine
    lib, _ = engine.load()
    if ctxs is None:
        fn = lib.mpmvs_fuse_ply
        fn.argtypes = [C.c_int] + FUSE_ARGTYPES_TAIL[:-3] + [C.POINTER(C.POINTER(C.c_ubyte)), _PP_U8]
    else:
        fn = lib.mpmvs_fuse_ply_ctx
        fn.argtypes = [C.c_int] + FUSE_ARGTYPES_TAIL[:3] + [C.POINTER(C.c_void_p)] + FUSE_ARGTYPES_TAIL[3:-3] + [C.POINTER(C.POINTER(C.c_ubyte)), _PP_U8]
    fn.restype = C.c_longlong
    lib.mpmvs_free.argtypes = [C.c_void_p]
    lib.mpmvs_free.restype = None
    out = {}

    def call(*args):
        # args = (device, n, cams, estimate, depths, normals, colors, ch, sky, off, ids, dyn, valid, points9, masks) from call_fuse
        rec = C.POINTER(C.c_ubyte)()
        count = fn(*args[:-3], C.byref(rec), args[-1])
        if count < 0:
            return int(count)
        out["records"] = np.ctypeslib.as_array(rec, shape=(count, 27)).copy() if count else np.zeros((0, 27), np.uint8)
        lib.mpmvs_free(rec)
        return 0

    _, _, masks = call_fuse(call, (int(device),), cams, estimate, depths, normals, colors, sources, use_dynamic, sky, reference_order, ctxs=ctxs, lists=lists)
    return out["records"], masks


def fuse_ply_tracks(cams, estimate, depths, normals, colors, sources, use_dynamic=True, device=0, sky=None, reference_order=False, ctxs=None, lists=None):
    """mpmvs_fuse_ply_tracks: fuse_ply that also returns every point's track (include/mpmvs.h) as CSR in the point order of the
    records: (records [M, 27] uint8, track_off [M + 1] int64, track_image [E] int32, track_pixel [E] int32, masks list).  Point p was
    averaged from pixels track_pixel[track_off[p]:track_off[p + 1]] (raster index, at each image's own width) of images
    track_image[...]; the first entry is the pixel that produced it.  ctxs as in fuse_ply (None: host arrays only)."""
    from . import engine
    lib, _ = engine.load()
    fn = lib.mpmvs_fuse_ply_tracks
    fn.argtypes = [C.c_int] + FUSE_ARGTYPES_TAIL[:3] + [C.POINTER(C.c_void_p)] + FUSE_ARGTYPES_TAIL[3:-3] + [
        C.POINTER(C.POINTER(C.c_ubyte)), C.POINTER(C.POINTER(C.c_longlong)), C.POINTER(C.POINTER(C.c_int32)), C.POINTER(C.POINTER(C.c_int32)), _PP_U8]
    fn.restype = C.c_longlong
    lib.mpmvs_free.argtypes = [C.c_void_p]
    lib.mpmvs_free.restype = None
    out = {}

    def call(*args):
        # args from call_fuse: (device, n, cams, estimate, [ctxs,] depths, ..., dyn, valid, points9, masks); the entry always takes ctxs
        head = args[:-3] if ctxs is not None else args[:4] + (None,) + args[4:-3]
        rec, off = C.POINTER(C.c_ubyte)(), C.POINTER(C.c_longlong)()
        img, pix = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)()
        count = fn(*head, C.byref(rec), C.byref(off), C.byref(img), C.byref(pix), args[-1])
        if count < 0:
            return int(count)
        out["records"] = np.ctypeslib.as_array(rec, shape=(count, 27)).copy() if count else np.zeros((0, 27), np.uint8)
        out["off"] = np.ctypeslib.as_array(off, shape=(count + 1,)).astype(np.int64)
        entries = int(out["off"][-1])
        out["image"] = np.ctypeslib.as_array(img, shape=(entries,)).copy() if entries else np.zeros(0, np.int32)
        out["pixel"] = np.ctypeslib.as_array(pix, shape=(entries,)).copy() if entries else np.zeros(0, np.int32)
        for p in (rec, off, img, pix):
            lib.mpmvs_free(p)
        return 0

    _, _, masks = call_fuse(call, (int(device),), cams, estimate, depths, normals, colors, sources, use_dynamic, sky, reference_order, ctxs=ctxs, lists=lists)
    return out["records"], out["off"], out["image"], out["pixel"], masks


def write_vis(path, track_off, track_image, image_ids=None):
    """COLMAP's point-visibility file (fused.ply.vis, read by its Delaunay mesher beside fused.ply), little endian: uint64 number of
    points, then per point uint32 k and k x uint32 image index -- here the images of the point's track, in track order.
    image_ids (optional): image_ids[our index] is the number written; default the index itself."""
    off = np.asarray(track_off, np.int64)
    img = np.asarray(track_image, np.int64)
    if off.ndim != 1 or len(off) < 1 or off[0] != 0 or off[-1] != len(img) or (np.diff(off) < 0).any():
        raise ValueError("track_off must be non-decreasing offsets from 0 to len(track_image)")
    if image_ids is not None:
        img = np.asarray(image_ids, np.int64)[img]
    if len(img) and (img.min() < 0 or img.max() > 0xffffffff):
        raise ValueError("image indices must fit uint32")
    n = len(off) - 1
    body = np.empty(n + len(img), "<u4")
    at = off[:-1] + np.arange(n)                      # where each point's count goes
    body[at] = np.diff(off)
    keep = np.ones(len(body), bool)
    keep[at] = False
    body[keep] = img
    with open(path, "wb") as f:
        f.write(np.uint64(n).astype("<u8").tobytes())
        f.write(body.tobytes())


def read_vis(path):
    """the file write_vis writes -> (track_off [M + 1] int64, image indices [E] int32 as stored)"""
    raw = open(path, "rb").read()
    if len(raw) < 8 or (len(raw) - 8) % 4:
        raise ValueError("not a point-visibility file")
    n = int(np.frombuffer(raw, "<u8", 1)[0])
    body = np.frombuffer(raw, "<u4", offset=8).astype(np.int64)
    off = np.zeros(n + 1, np.int64)
    at = 0
    for p in range(n):                                # the counts are only reachable one after the other
        if at >= len(body):
            raise ValueError("truncated point-visibility file")
        off[p + 1] = off[p] + body[at]
        at += 1 + int(body[at])
    if at != len(body):
        raise ValueError("point-visibility file has the wrong length")
    keep = np.ones(len(body), bool)
    keep[off[:-1] + np.arange(n)] = False
    return off, body[keep].astype(np.int32)


def last_kernel_ms():
    from . import engine
    lib, _ = engine.load()
    lib.mpmvs_fuse_kernel_ms.restype = C.c_float
    return float(lib.mpmvs_fuse_kernel_ms())


def sky_bilateral(bgr, mask, device=0):
    """joint-bilateral refinement of a coarse sky-probability mask on the MI355X (mpmvs_sky_bilateral;
    reference SkySegment/src/SkyRegionDetect.cu:3-66).  bgr: HxWx3 uint8, mask: HxW fp32 -> HxW fp32 of 255 / 0"""
    from . import engine
    lib, _ = engine.load()
    fn = lib.mpmvs_sky_bilateral
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    bgr = np.ascontiguousarray(bgr, np.uint8)
    mask = np.ascontiguousarray(mask, np.float32)
    if bgr.shape != mask.shape + (3,):
        raise ValueError("bgr must be HxWx3 and mask HxW")
    out = np.empty(mask.shape, np.float32)
    rc = fn(int(device), bgr.ctypes.data, mask.ctypes.data, out.ctypes.data, mask.shape[0], mask.shape[1])
    if rc != 0:
        raise RuntimeError(f"mpmvs_sky_bilateral failed ({rc})")
    return out


def last_sky_kernel_ms():
    from . import engine
    lib, _ = engine.load()
    lib.mpmvs_sky_kernel_ms.restype = C.c_float
    return float(lib.mpmvs_sky_kernel_ms())
