"""ctypes binding of the C++ host layer (host/libmpmvs_host.so): the planar-prior
construction of ProcessProblem (reference src/PatchMatch.cpp:532-604) and the
single-Problem pass schedule (reference src/main.cpp:20-41)."""
import ctypes as C
import os

import numpy as np

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "host", "libmpmvs_host.so")
SYMBOLS = ["mpmvs_host_triangulate_vertices", "mpmvs_host_delaunay", "mpmvs_host_build_prior", "mpmvs_host_run_pipeline",
           "mpmvs_host_write_dmb", "mpmvs_host_read_dmb", "mpmvs_host_read_camera", "mpmvs_host_sample_list", "mpmvs_host_read_pgm",
           "mpmvs_host_run_folder", "mpmvs_host_resize_linear", "mpmvs_host_write_ply", "mpmvs_host_fuse_folder", "mpmvs_host_read_image",
           "mpmvs_host_decode_jpeg", "mpmvs_host_refine_sky_masks", "mpmvs_host_run_folder_jacobi", "mpmvs_host_prior_from_triangles", "mpmvs_host_run_folder_jacobi_fused",
           "mpmvs_host_generate_sky_masks", "mpmvs_host_sky_preprocess", "mpmvs_host_pyrdown8", "mpmvs_host_undistort_u8", "mpmvs_host_undistort_atan",
           "mpmvs_host_undistort_forward", "mpmvs_host_undistort_inverse", "mpmvs_host_undistort_threads", "mpmvs_host_fuse_folder_vis"]
_cache = {}


def load():
    if "lib" not in _cache:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"host library not built: {LIB_PATH} (run __graft_entry__.build())")
        lib = C.CDLL(LIB_PATH)
        P = C.c_void_p
        lib.mpmvs_host_triangulate_vertices.restype = C.c_int
        lib.mpmvs_host_triangulate_vertices.argtypes = [C.c_int, C.c_int, P, P, C.c_int, P, C.c_int]
        lib.mpmvs_host_delaunay.restype = C.c_int
        lib.mpmvs_host_delaunay.argtypes = [C.c_int, C.c_int, P, C.c_int, P, C.c_int]
        lib.mpmvs_host_build_prior.restype = C.c_int
        lib.mpmvs_host_build_prior.argtypes = [C.POINTER(_abi.Camera), C.c_int, C.c_int, P, P, P, C.c_int, C.c_float, C.c_float, P, P]
        lib.mpmvs_host_prior_from_triangles.restype = C.c_int
        lib.mpmvs_host_prior_from_triangles.argtypes = [C.POINTER(_abi.Camera), C.c_int, C.c_int, P, C.c_int, P, C.c_float, C.c_float, P, P, P]
        lib.mpmvs_host_run_pipeline.restype = C.c_int
        lib.mpmvs_host_run_pipeline.argtypes = [C.c_int, C.c_int, C.POINTER(_abi.Camera), C.POINTER(C.POINTER(C.c_float)), C.c_int, C.c_int,
                                                C.c_int, C.c_int, C.c_uint64, C.POINTER(C.POINTER(C.c_float)), P, P, P, C.c_int]
        lib.mpmvs_host_write_dmb.restype = C.c_int
        lib.mpmvs_host_write_dmb.argtypes = [C.c_char_p, P, C.c_int, C.c_int, C.c_int]
        lib.mpmvs_host_read_dmb.restype = C.c_int
        lib.mpmvs_host_read_dmb.argtypes = [C.c_char_p, P, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        lib.mpmvs_host_read_camera.restype = C.c_int
        lib.mpmvs_host_read_camera.argtypes = [C.c_char_p, C.POINTER(_abi.Camera)]
        lib.mpmvs_host_sample_list.restype = C.c_int
        lib.mpmvs_host_sample_list.argtypes = [C.c_char_p, C.c_int, C.c_int, P, C.c_int]
        lib.mpmvs_host_read_pgm.restype = C.c_int
        lib.mpmvs_host_read_pgm.argtypes = [C.c_char_p, P, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        lib.mpmvs_host_run_folder.restype = C.c_int
        lib.mpmvs_host_run_folder.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int]
        lib.mpmvs_host_run_folder_jacobi.restype = C.c_int
        lib.mpmvs_host_run_folder_jacobi.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int]
        lib.mpmvs_host_run_folder_jacobi_fused.restype = C.c_long
        lib.mpmvs_host_run_folder_jacobi_fused.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int,
                                                           C.c_int, C.c_int, C.c_int]
        lib.mpmvs_host_fuse_folder.restype = C.c_long
        lib.mpmvs_host_fuse_folder.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int]
        lib.mpmvs_host_fuse_folder_vis.restype = C.c_long
        lib.mpmvs_host_fuse_folder_vis.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        lib.mpmvs_host_refine_sky_masks.restype = C.c_int
        lib.mpmvs_host_refine_sky_masks.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int]
        lib.mpmvs_host_read_image.restype = C.c_int
        lib.mpmvs_host_read_image.argtypes = [C.c_char_p, C.c_int, P, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        lib.mpmvs_host_decode_jpeg.restype = C.c_int
        lib.mpmvs_host_decode_jpeg.argtypes = [C.c_char_p, C.c_size_t, C.c_int, P, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        lib.mpmvs_host_write_ply.restype = C.c_int
        lib.mpmvs_host_write_ply.argtypes = [C.c_char_p, P, C.c_int]
        lib.mpmvs_host_resize_linear.restype = C.c_int
        lib.mpmvs_host_resize_linear.argtypes = [P, C.c_int, C.c_int, P, C.c_int, C.c_int]
        lib.mpmvs_host_generate_sky_masks.restype = C.c_int
        lib.mpmvs_host_generate_sky_masks.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int]
        lib.mpmvs_host_sky_preprocess.restype = C.c_int
        lib.mpmvs_host_sky_preprocess.argtypes = [P, C.c_int, C.c_int, C.c_int, C.c_int, P]
        lib.mpmvs_host_pyrdown8.restype = C.c_int
        lib.mpmvs_host_pyrdown8.argtypes = [P, C.c_int, C.c_int, C.c_int, P]
        lib.mpmvs_host_undistort_u8.restype = C.c_int
        lib.mpmvs_host_undistort_u8.argtypes = [P, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int, P, C.c_int, P, C.c_int, C.c_int, P, P]
        lib.mpmvs_host_undistort_threads.restype = C.c_int
        lib.mpmvs_host_undistort_threads.argtypes = []
        lib.mpmvs_host_undistort_atan.restype = None
        lib.mpmvs_host_undistort_atan.argtypes = [P, C.c_int, P]
        lib.mpmvs_host_undistort_forward.restype = C.c_int
        lib.mpmvs_host_undistort_forward.argtypes = [C.c_int, P, C.c_int, P, C.c_int, P]
        lib.mpmvs_host_undistort_inverse.restype = C.c_int
        lib.mpmvs_host_undistort_inverse.argtypes = [C.c_int, P, C.c_int, P, C.c_int, P]
        _cache["lib"] = lib
    return _cache["lib"]


def triangulate_vertices(costs, geom_costs=None, geom_planar_prior=False):
    lib = load()
    costs = np.ascontiguousarray(costs, np.float32)
    h, w = costs.shape
    g = np.ascontiguousarray(geom_costs, np.float32) if geom_costs is not None else None
    cap = 3 * ((h + 4) // 5) * ((w + 4) // 5) + 8
    out = np.empty((cap, 2), np.int32)
    n = lib.mpmvs_host_triangulate_vertices(w, h, costs.ctypes.data, g.ctypes.data if g is not None else None,
                                            1 if geom_planar_prior else 0, out.ctypes.data, cap)
    return out[:n].copy()


def delaunay(w, h, points):
    lib = load()
    pts = np.ascontiguousarray(points, np.int32).reshape(-1, 2)
    cap = 2 * len(pts) + 8
    out = np.empty((cap, 3, 2), np.int32)
    n = lib.mpmvs_host_delaunay(w, h, pts.ctypes.data, len(pts), out.ctypes.data, cap)
    assert 0 <= n <= cap
    return out[:n]


def build_prior(cam, planes, costs, geom_costs, geom_planar_prior, depth_min, depth_max):
    """(prior planes HxWx4, mask HxW u32, number of triangles)"""
    lib = load()
    planes = np.ascontiguousarray(planes, np.float32)
    costs = np.ascontiguousarray(costs, np.float32)
    h, w = costs.shape
    g = np.ascontiguousarray(geom_costs, np.float32) if geom_costs is not None else None
    prior = np.zeros((h, w, 4), np.float32)
    mask = np.zeros((h, w), np.uint32)
    n = lib.mpmvs_host_build_prior(C.byref(cam), w, h, planes.ctypes.data, costs.ctypes.data, g.ctypes.data if g is not None else None,
                                   1 if geom_planar_prior else 0, float(depth_min), float(depth_max), prior.ctypes.data, mask.ctypes.data)
    return prior, mask, n


def prior_from_triangles(cam, tri_pts, planes, depth_min, depth_max):
    """raster + plane fit + depth-range test for an explicit triangle list [n][3][2] (labels 1..n in that order):
    (prior planes HxWx4, mask HxW u32, per-triangle planes nx4)"""
    lib = load()
    planes = np.ascontiguousarray(planes, np.float32)
    h, w = planes.shape[:2]
    t = np.ascontiguousarray(tri_pts, np.int32).reshape(-1, 6)
    prior = np.zeros((h, w, 4), np.float32)
    mask = np.zeros((h, w), np.uint32)
    pl = np.zeros((len(t), 4), np.float32)
    n = lib.mpmvs_host_prior_from_triangles(C.byref(cam), w, h, t.ctypes.data, len(t), planes.ctypes.data, float(depth_min), float(depth_max),
                                            prior.ctypes.data, mask.ctypes.data, pl.ctypes.data)
    if n < 0:
        raise RuntimeError("prior_from_triangles failed")
    return prior, mask, pl[:n]


def run_pipeline(device, cams, images, max_scale, geom_iterations, planar_prior, geom_planar_prior, seed, src_depths=None, max_image_size=0, out_size=None):
    """one Problem through the reference's pass schedule on the HIP path; returns depth, normal, cost.
    max_image_size > 0: larger images are shrunk as PatchMatchInit does (out_size = (h, w) of the shrunk reference image)"""
    lib = load()
    n = len(cams)
    imgs = [np.ascontiguousarray(im, np.float32) for im in images]
    cam_arr = (_abi.Camera * n)(*cams)
    ptrs = (C.POINTER(C.c_float) * n)(*[im.ctypes.data_as(C.POINTER(C.c_float)) for im in imgs])
    dptr = None
    if src_depths is not None:
        ds = [np.ascontiguousarray(d, np.float32) for d in src_depths]
        dptr = (C.POINTER(C.c_float) * (n - 1))(*[d.ctypes.data_as(C.POINTER(C.c_float)) for d in ds])
    h, w = out_size if out_size is not None else imgs[0].shape
    depth = np.empty((h, w), np.float32)
    normal = np.empty((h, w, 3), np.float32)
    cost = np.empty((h, w), np.float32)
    rc = lib.mpmvs_host_run_pipeline(int(device), n, cam_arr, ptrs, int(max_scale), int(geom_iterations), 1 if planar_prior else 0,
                                     1 if geom_planar_prior else 0, int(seed), dptr, depth.ctypes.data, normal.ctypes.data, cost.ctypes.data, int(max_image_size))
    if rc != 0:
        raise RuntimeError(f"mpmvs_host_run_pipeline failed ({rc})")
    return depth, normal, cost


# ---- file formats (reference src/utility.cpp:193-308, src/PatchMatch.cpp:67-143) ------------
def write_dmb(path, arr):
    a = np.ascontiguousarray(arr, np.float32)
    h, w = a.shape[:2]
    nb = 1 if a.ndim == 2 else a.shape[2]
    if load().mpmvs_host_write_dmb(str(path).encode(), a.ctypes.data, h, w, nb) != 0:
        raise RuntimeError(f"cannot write {path}")


def read_dmb(path):
    lib = load()
    h, w, nb = C.c_int(), C.c_int(), C.c_int()
    if lib.mpmvs_host_read_dmb(str(path).encode(), None, 0, C.byref(h), C.byref(w), C.byref(nb)) != 0:
        raise RuntimeError(f"cannot read {path}")
    out = np.empty((h.value, w.value, nb.value), np.float32)
    lib.mpmvs_host_read_dmb(str(path).encode(), out.ctypes.data, out.size, C.byref(h), C.byref(w), C.byref(nb))
    return out[..., 0] if nb.value == 1 else out


def read_camera(path):
    cam = _abi.Camera()
    load().mpmvs_host_read_camera(str(path).encode(), C.byref(cam))
    return cam


def sample_list(folder, max_src=20, max_size=3200):
    """pair.txt -> list of (estimate, refID, srcID list with srcID[0] == refID)"""
    lib = load()
    n = lib.mpmvs_host_sample_list(str(folder).encode(), max_src, max_size, None, 0)
    buf = np.empty(n, np.int32)
    lib.mpmvs_host_sample_list(str(folder).encode(), max_src, max_size, buf.ctypes.data, n)
    out, k = [], 1
    for _ in range(int(buf[0])):
        est, ref, cnt = int(buf[k]), int(buf[k + 1]), int(buf[k + 2])
        out.append((bool(est), ref, [int(v) for v in buf[k + 3:k + 3 + cnt]]))
        k += 3 + cnt
    return out


def read_pgm(path):
    lib = load()
    h, w = C.c_int(), C.c_int()
    if lib.mpmvs_host_read_pgm(str(path).encode(), None, 0, C.byref(h), C.byref(w)) != 0:
        raise RuntimeError(f"cannot read {path}")
    out = np.empty((h.value, w.value), np.float32)
    lib.mpmvs_host_read_pgm(str(path).encode(), out.ctypes.data, out.size, C.byref(h), C.byref(w))
    return out


def read_image(path, channels=1):
    """what cv::imread(path, GRAYSCALE / COLOR) hands the reference: uint8 HxW or HxWx3 (B,G,R); JPEG, PGM or PPM"""
    lib = load()
    h, w = C.c_int(), C.c_int()
    if lib.mpmvs_host_read_image(str(path).encode(), channels, None, 0, C.byref(h), C.byref(w)) != 0:
        raise RuntimeError(f"cannot read {path}")
    out = np.empty((h.value, w.value) + ((3,) if channels == 3 else ()), np.uint8)
    lib.mpmvs_host_read_image(str(path).encode(), channels, out.ctypes.data, out.size, C.byref(h), C.byref(w))
    return out


def decode_jpeg(data, channels=1):
    lib = load()
    data = bytes(data)
    h, w = C.c_int(), C.c_int()
    if lib.mpmvs_host_decode_jpeg(data, len(data), channels, None, 0, C.byref(h), C.byref(w)) != 0:
        raise RuntimeError("JPEG decode failed")
    out = np.empty((h.value, w.value) + ((3,) if channels == 3 else ()), np.uint8)
    lib.mpmvs_host_decode_jpeg(data, len(data), channels, out.ctypes.data, out.size, C.byref(h), C.byref(w))
    return out


def run_folder(folder, device=0, max_src=20, geom_iterations=2, planar_prior=True, geom_planar_prior=True, max_scale=2, seed=12345,
               max_image_size=3200):
    rc = load().mpmvs_host_run_folder(str(folder).encode(), device, max_src, geom_iterations, 1 if planar_prior else 0,
                                      1 if geom_planar_prior else 0, max_scale, seed, max_image_size)
    if rc != 0:
        raise RuntimeError(f"run_folder failed ({rc})")


def run_folder_jacobi(folder, devices=(0,), workers=3, max_src=20, geom_iterations=2, planar_prior=True, geom_planar_prior=True, max_scale=2, seed=12345,
                      max_image_size=3200):
    """the pass loops over a dataset folder in Jacobi order with `workers` host threads over `devices` (see scene_io.h);
    returns the number of Problems per pass"""
    dev = (C.c_int * len(devices))(*devices)
    rc = load().mpmvs_host_run_folder_jacobi(str(folder).encode(), dev, len(devices), workers, max_src, geom_iterations, 1 if planar_prior else 0,
                                             1 if geom_planar_prior else 0, max_scale, seed, max_image_size)
    if rc < 0:
        raise RuntimeError(f"run_folder_jacobi failed ({rc})")
    return rc


def run_folder_jacobi_fused(folder, devices=(0,), workers=3, max_src=20, geom_iterations=2, planar_prior=True, geom_planar_prior=True, max_scale=2, seed=12345,
                            max_image_size=3200, use_dynamic=True, sky_seg=False, write_maps=True):
    """run_folder_jacobi followed by the reference's last step, RunFusion, out of the Problems' resident contexts (no upload of the
    final depth / normal maps) -> <folder>/MPMVS/MPMVS_model.ply; returns the number of fused points"""
    dev = (C.c_int * len(devices))(*devices)
    n = load().mpmvs_host_run_folder_jacobi_fused(str(folder).encode(), dev, len(devices), workers, max_src, geom_iterations, 1 if planar_prior else 0,
                                                  1 if geom_planar_prior else 0, max_scale, seed, max_image_size, 1 if use_dynamic else 0,
                                                  1 if sky_seg else 0, 1 if write_maps else 0)
    if n < 0:
        raise RuntimeError(f"run_folder_jacobi_fused failed ({n})")
    return n


def run_folder_jacobi_in_memory(folder, n, height, width, devices=(0,), workers=3, max_src=20, geom_iterations=2, planar_prior=True, geom_planar_prior=True,
                                max_scale=2, seed=12345, max_image_size=3200):
    """run_folder_jacobi without result files: returns (depths [n][H][W], normals [n][H][W][3], costs [n][H][W]) of the last pass"""
    lib = load()
    dev = (C.c_int * len(devices))(*devices)
    depth = np.zeros((n, height, width), np.float32)
    normal = np.zeros((n, height, width, 3), np.float32)
    cost = np.zeros((n, height, width), np.float32)
    FP = C.POINTER(C.c_float)
    dp = (FP * n)(*[depth[i].ctypes.data_as(FP) for i in range(n)])
    np_ = (FP * n)(*[normal[i].ctypes.data_as(FP) for i in range(n)])
    cp = (FP * n)(*[cost[i].ctypes.data_as(FP) for i in range(n)])
    fn = lib.mpmvs_host_run_folder_jacobi_mem
    fn.restype = C.c_int
    fn.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int, C.POINTER(FP), C.POINTER(FP),
                   C.POINTER(FP), C.c_int]
    rc = fn(str(folder).encode(), dev, len(devices), workers, max_src, geom_iterations, 1 if planar_prior else 0, 1 if geom_planar_prior else 0, max_scale, seed,
            max_image_size, dp, np_, cp, n)
    if rc < 0:
        raise RuntimeError(f"run_folder_jacobi (in memory) failed ({rc})")
    return depth, normal, cost


def write_dataset(folder, cams, images, sources, scores=None, fmt="pgm", jpeg_options=None):
    """a scene in the reference's input layout: images/%08d.<fmt>, cams/%08d_cam.txt
    (MVSNet style, reference src/PatchMatch.cpp:109-143), pair.txt (reference :67-107).
    fmt: "pgm" (grey, HxW), "ppm" (HxWx3 R,G,B) or "jpg" (either; written with PIL, test/tool use only)"""
    import os
    os.makedirs(os.path.join(folder, "images"), exist_ok=True)
    os.makedirs(os.path.join(folder, "cams"), exist_ok=True)
    for i, (cam, img) in enumerate(zip(cams, images)):
        a = np.asarray(img)
        assert np.array_equal(a, np.rint(a)) and a.min() >= 0 and a.max() <= 255, "image files hold 8-bit images"
        path = os.path.join(folder, "images", f"{i:08d}.{fmt}")
        if fmt == "jpg":
            from PIL import Image
            Image.fromarray(a.astype(np.uint8)).save(path, "JPEG", **(jpeg_options or {"quality": 95}))
        else:
            assert (fmt == "pgm" and a.ndim == 2) or (fmt == "ppm" and a.ndim == 3)
            with open(path, "wb") as f:
                f.write(b"P%d\n%d %d\n255\n" % (5 if fmt == "pgm" else 6, a.shape[1], a.shape[0]))
                f.write(a.astype(np.uint8).tobytes())
        R, t, K = list(cam.R), list(cam.t), list(cam.K)
        with open(os.path.join(folder, "cams", f"{i:08d}_cam.txt"), "w") as f:
            f.write("extrinsic\n")
            for r in range(3):
                f.write(" ".join(repr(float(np.float32(v))) for v in (R[3 * r], R[3 * r + 1], R[3 * r + 2], t[r])) + "\n")
            f.write("0.0 0.0 0.0 1.0\n\nintrinsic\n")
            for r in range(3):
                f.write(" ".join(repr(float(np.float32(v))) for v in K[3 * r:3 * r + 3]) + "\n")
            f.write(f"\n{float(np.float32(cam.depth_min))!r} 0.01 192 {float(np.float32(cam.depth_max))!r}\n")
    with open(os.path.join(folder, "pair.txt"), "w") as f:
        f.write(f"{len(sources)}\n")
        for i, src in enumerate(sources):
            sc = scores[i] if scores is not None else [100.0 - k for k in range(len(src))]
            f.write(f"{i}\n{len(src)} " + " ".join(f"{s} {v}" for s, v in zip(src, sc)) + "\n")


def resize_linear(img, new_w, new_h):
    a = np.ascontiguousarray(img, np.float32)
    out = np.empty((new_h, new_w), np.float32)
    load().mpmvs_host_resize_linear(a.ctypes.data, a.shape[1], a.shape[0], out.ctypes.data, new_w, new_h)
    return out


def write_ply(path, points9):
    """binary PLY of fused points (reference src/PatchMatch.cpp:145-198)"""
    a = np.ascontiguousarray(points9, np.float32).reshape(-1, 9)
    load().mpmvs_host_write_ply(str(path).encode(), a.ctypes.data, len(a))


def refine_sky_masks(folder, device=0, max_src=20, max_image_size=3200):
    """<folder>/MPMVS/2333_<id>/skymask.* (coarse, 255 x probability) -> skymask_refine.pgm; returns the number written"""
    n = load().mpmvs_host_refine_sky_masks(str(folder).encode(), device, max_src, max_image_size)
    if n < 0:
        raise RuntimeError("refine_sky_masks failed")
    return int(n)


def generate_sky_masks(folder, model_dir, device=0, max_src=20, max_image_size=3200):
    """GenerateSkyRegionMask: the segmentation network (model_dir/skysegsmall_sim-opt-fp16.{param,bin}) on every image of the
    folder, then the refinement of the fp32 mask -> skymask.pgm and skymask_refine.pgm per image; returns the number done.
    Runs on the GPU; there is no CPU path."""
    n = load().mpmvs_host_generate_sky_masks(str(folder).encode(), str(model_dir).encode(), device, max_src, max_image_size)
    if n < 0:
        raise RuntimeError("generate_sky_masks failed")
    return int(n)


def sky_preprocess(bgr, net_h=384, net_w=384):
    """the host statement of the network's preprocessing: uint8 [h, w, 3] B,G,R -> float32 [3, net_h, net_w]; no device involved"""
    im = np.ascontiguousarray(bgr, np.uint8)
    assert im.ndim == 3 and im.shape[2] == 3
    out = np.empty((3, net_h, net_w), np.float32)
    if load().mpmvs_host_sky_preprocess(im.ctypes.data, im.shape[0], im.shape[1], net_h, net_w, out.ctypes.data) != 0:
        raise RuntimeError("sky_preprocess failed")
    return out


def pyrdown8(img):
    """cv::pyrDown to (w // 2, h // 2) of a uint8 [h, w] or [h, w, c] image as the host states it"""
    im = np.ascontiguousarray(img, np.uint8)
    ch = 1 if im.ndim == 2 else im.shape[2]
    out = np.empty((im.shape[0] // 2, im.shape[1] // 2) + (() if im.ndim == 2 else (ch,)), np.uint8)
    if load().mpmvs_host_pyrdown8(im.ctypes.data, im.shape[0], im.shape[1], ch, out.ctypes.data) != 0:
        raise RuntimeError("pyrdown8 failed")
    return out


def undistort_u8(img, model_id, params, dst, valid=False, pitch=None):
    """the host statement of the undistortion warp (mpmvs_host_undistort_u8), arguments as engine.undistort_u8 with a numeric
    model id; no device involved"""
    im = np.asarray(img)
    assert im.dtype == np.uint8 and im.ndim in (2, 3)
    ch = 1 if im.ndim == 2 else im.shape[2]
    if im.strides[-1] != 1 or (im.ndim == 3 and im.strides[1] != ch) or im.strides[0] < im.shape[1] * ch:
        im = np.ascontiguousarray(im)
    prm = np.ascontiguousarray(params, np.float64).reshape(-1)
    k, dw, dh = dst
    k = np.ascontiguousarray(k, np.float64)
    out = np.empty((int(dh), int(dw)) + im.shape[2:], np.uint8)
    ok = np.empty((int(dh), int(dw)), np.uint8) if valid else None
    rc = load().mpmvs_host_undistort_u8(im.ctypes.data, ch, im.shape[1], im.shape[0], im.strides[0] if pitch is None else pitch, int(model_id),
                                        prm.ctypes.data, len(prm), k.ctypes.data, int(dw), int(dh), out.ctypes.data, ok.ctypes.data if valid else None)
    if rc != 0:
        raise ValueError(f"mpmvs_host_undistort_u8 refused its arguments ({rc})")
    return (out, ok) if valid else out


def undistort_threads():
    """the size of the OpenMP team undistort_u8 runs on"""
    return int(load().mpmvs_host_undistort_threads())


def undistort_atan(x):
    """probe: the atan of csrc/pm_undistort_model.hpp (+ - * / sqrt only) on a float64 array"""
    a = np.ascontiguousarray(x, np.float64)
    out = np.empty_like(a)
    load().mpmvs_host_undistort_atan(a.ctypes.data, a.size, out.ctypes.data)
    return out


def _undistort_points(fn, model_id, params, pts):
    prm = np.ascontiguousarray(params, np.float64).reshape(-1)
    a = np.ascontiguousarray(pts, np.float64).reshape(-1, 2)
    out = np.empty_like(a)
    if fn(int(model_id), prm.ctypes.data, len(prm), a.ctypes.data, len(a), out.ctypes.data) != 0:
        raise ValueError("unknown camera model or wrong parameter count")
    return out


def undistort_forward(model_id, params, uv):
    """probe: normalised pinhole coordinates [n, 2] -> image points [n, 2] of the distorted camera"""
    return _undistort_points(load().mpmvs_host_undistort_forward, model_id, params, uv)


def undistort_inverse(model_id, params, xy):
    """probe: image points [n, 2] -> normalised pinhole coordinates [n, 2] (the Newton inverse the output camera uses)"""
    return _undistort_points(load().mpmvs_host_undistort_inverse, model_id, params, xy)


def fuse_folder(folder, device=0, max_src=20, use_dynamic=True, sky_seg=False, write_vis=False):
    """RunFusion over a processed dataset folder -> <folder>/MPMVS/MPMVS_model.ply; returns the point count.
    write_vis: also <folder>/MPMVS/MPMVS_model.ply.vis, per point the images of its track (COLMAP's point-visibility format; ids as in pair.txt)"""
    if write_vis:
        n = load().mpmvs_host_fuse_folder_vis(str(folder).encode(), device, max_src, 1 if use_dynamic else 0, 1 if sky_seg else 0, 1)
    else:
        n = load().mpmvs_host_fuse_folder(str(folder).encode(), device, max_src, 1 if use_dynamic else 0, 1 if sky_seg else 0)
    if n < 0:
        raise RuntimeError("fuse_folder failed")
    return int(n)
