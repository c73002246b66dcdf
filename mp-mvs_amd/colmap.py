"""COLMAP sparse model -> the MVSNet-style folder the pipeline reads (cams/%08d_cam.txt, pair.txt, images/%08d.*): the
outputs of the reference's colmap2mvsnet_acm.py, with the model read in C++ (host/colmap_io.cpp) and the view selection
on the GPU (mpmvs_view_select, csrc/pm_viewsel.hpp).  Contract: DESIGN.md section 11.  With undistort=True the images of
distorted cameras are resampled to pinhole cameras on the GPU first (mpmvs_undistort_u8, csrc/pm_undistort.hpp; DESIGN.md
section 12), the step COLMAP's image_undistorter does.  CLI: tools/colmap2mvs.py."""
import ctypes as C
import os
import shutil
import sys
import time
from dataclasses import dataclass
from typing import List

import numpy as np

from . import hostlib

# COLMAP's camera models by id, with the names of their parameters (the reference's param_type table)
CAMERA_MODELS = ["SIMPLE_PINHOLE", "PINHOLE", "SIMPLE_RADIAL", "RADIAL", "OPENCV", "OPENCV_FISHEYE", "FULL_OPENCV", "FOV",
                 "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE", "THIN_PRISM_FISHEYE"]
PARAMS = {
    "SIMPLE_PINHOLE": ["f", "cx", "cy"],
    "PINHOLE": ["fx", "fy", "cx", "cy"],
    "SIMPLE_RADIAL": ["f", "cx", "cy", "k"],
    "SIMPLE_RADIAL_FISHEYE": ["f", "cx", "cy", "k"],
    "RADIAL": ["f", "cx", "cy", "k1", "k2"],
    "RADIAL_FISHEYE": ["f", "cx", "cy", "k1", "k2"],
    "OPENCV": ["fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2"],
    "OPENCV_FISHEYE": ["fx", "fy", "cx", "cy", "k1", "k2", "k3", "k4"],
    "FULL_OPENCV": ["fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "k4", "k5", "k6"],
    "FOV": ["fx", "fy", "cx", "cy", "omega"],
    "THIN_PRISM_FISHEYE": ["fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "k4", "sx1", "sy1"],
}
MAX_IMAGES = 32768   # MPMVS_VIEW_SELECT_MAX_IMAGES


@dataclass
class Model:
    """A sparse model as flat arrays; images in ascending image_id order (index i = rank of the id)."""
    cam_id: np.ndarray       # (C,) int32
    cam_model: np.ndarray    # (C,) int32, index into CAMERA_MODELS
    cam_width: np.ndarray    # (C,) int64
    cam_height: np.ndarray   # (C,) int64
    cam_params: np.ndarray   # (C, 12) float64, zero padded
    image_id: np.ndarray     # (N,) int32
    qvec: np.ndarray         # (N, 4) float64
    tvec: np.ndarray         # (N, 3) float64
    image_cam: np.ndarray    # (N,) int32 camera id
    names: List[str]
    obs_off: np.ndarray      # (N + 1,) int64 offsets into obs_pt
    obs_pt: np.ndarray       # (obs,) int32: each image's point3D_ids in file order as indices into point_id / xyz, -1 for none
    point_id: np.ndarray     # (P,) int64
    xyz: np.ndarray          # (P, 3) float64

    @property
    def n_images(self):
        return len(self.image_id)


def _host():
    lib = hostlib.load()
    if not hasattr(lib, "_colmap_bound"):
        P = C.c_void_p
        lib.mpmvs_host_colmap_read.restype = C.c_void_p
        lib.mpmvs_host_colmap_read.argtypes = [C.c_char_p, C.c_char_p, P, C.c_char_p, C.c_int]
        lib.mpmvs_host_colmap_fill.restype = C.c_int
        lib.mpmvs_host_colmap_fill.argtypes = [P] * 15
        lib.mpmvs_host_colmap_free.restype = None
        lib.mpmvs_host_colmap_free.argtypes = [P]
        lib._colmap_bound = True
    return lib


def read_model(sparse_dir, ext=None):
    """cameras / images / points3D of `sparse_dir`; ext ".bin" or ".txt", None: .bin if cameras.bin exists, else .txt"""
    if ext is None:
        ext = ".bin" if os.path.exists(os.path.join(sparse_dir, "cameras.bin")) else ".txt"
    lib = _host()
    sizes = np.zeros(5, np.int64)
    err = C.create_string_buffer(1024)
    h = lib.mpmvs_host_colmap_read(str(sparse_dir).encode(), ext.encode(), sizes.ctypes.data, err, len(err))
    if not h:
        raise ValueError(f"COLMAP model {sparse_dir} ({ext}): {err.value.decode(errors='replace')}")
    nc, ni, no, npt, nb = (int(v) for v in sizes)
    m = Model(np.zeros(nc, np.int32), np.zeros(nc, np.int32), np.zeros(nc, np.int64), np.zeros(nc, np.int64), np.zeros((nc, 12)),
              np.zeros(ni, np.int32), np.zeros((ni, 4)), np.zeros((ni, 3)), np.zeros(ni, np.int32), [], np.zeros(ni + 1, np.int64),
              np.zeros(no, np.int32), np.zeros(npt, np.int64), np.zeros((npt, 3)))
    names = np.zeros(max(nb, 1), np.uint8)
    try:
        lib.mpmvs_host_colmap_fill(h, *(a.ctypes.data for a in (m.cam_id, m.cam_model, m.cam_width, m.cam_height, m.cam_params, m.image_id,
                                                               m.qvec, m.tvec, m.image_cam, names, m.obs_off, m.obs_pt, m.point_id, m.xyz)))
    finally:
        lib.mpmvs_host_colmap_free(h)
    m.names = [s.decode() for s in names[:nb].tobytes().split(b"\0")[:ni]]
    return m


def qvec2rotmat(q):
    """(..., 4) quaternions (w, x, y, z) -> (..., 3, 3) rotations, COLMAP's formula and operation order"""
    q = np.asarray(q, np.float64)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0] = 1 - 2 * y ** 2 - 2 * z ** 2
    R[..., 0, 1] = 2 * x * y - 2 * w * z
    R[..., 0, 2] = 2 * z * x + 2 * w * y
    R[..., 1, 0] = 2 * x * y + 2 * w * z
    R[..., 1, 1] = 1 - 2 * x ** 2 - 2 * z ** 2
    R[..., 1, 2] = 2 * y * z - 2 * w * x
    R[..., 2, 0] = 2 * z * x - 2 * w * y
    R[..., 2, 1] = 2 * y * z + 2 * w * x
    R[..., 2, 2] = 1 - 2 * x ** 2 - 2 * y ** 2
    return R


def extrinsics(model):
    """(N, 4, 4) world -> camera [R t; 0 0 0 1]"""
    E = np.zeros((model.n_images, 4, 4))
    E[:, :3, :3] = qvec2rotmat(model.qvec)
    E[:, :3, 3] = model.tvec
    E[:, 3, 3] = 1
    return E


def centers(model):
    """(N, 3) camera centres -R^T t"""
    E = extrinsics(model)
    return -np.matmul(E[:, :3, :3].transpose(0, 2, 1), E[:, :3, 3:4])[:, :, 0]


def intrinsics(model, warn=True):
    """{camera id: 3x3 K} from fx fy cx cy (f for both where the model has one); distortion is ignored, as the reference does"""
    out, distorted = {}, []
    for cid, mid, prm in zip(model.cam_id, model.cam_model, model.cam_params):
        name = CAMERA_MODELS[mid]
        d = dict(zip(PARAMS[name], prm[:len(PARAMS[name])]))
        if "f" in d:
            d["fx"] = d["fy"] = d["f"]
        out[int(cid)] = np.array([[d["fx"], 0, d["cx"]], [0, d["fy"], d["cy"]], [0, 0, 1]])
        if any(v != 0 for k, v in d.items() if k not in ("f", "fx", "fy", "cx", "cy")):
            distorted.append(int(cid))
    if warn and distorted:
        print(f"warning: distortion parameters of camera(s) {distorted} are non-zero and are ignored: the input should be "
              "COLMAP's undistorted dense folder", file=sys.stderr)
    return out


def camera_params(model, k):
    """(model name, its parameters in file order) of the k-th camera"""
    name = CAMERA_MODELS[model.cam_model[k]]
    return name, model.cam_params[k][:len(PARAMS[name])]


def is_distorted(model, k):
    """the k-th camera has a distortion parameter that is not zero"""
    name, prm = camera_params(model, k)
    return any(v != 0 for n, v in zip(PARAMS[name], prm) if n not in ("f", "fx", "fy", "cx", "cy"))


def undistorted_cameras(model, blank_pixels=0.0, min_scale=0.2, max_scale=2.0):
    """{camera id: (3x3 K', W', H')}: the pinhole camera each camera's images are undistorted to (mpmvs_undistort_camera);
    a pinhole camera and a camera whose distortion parameters are all zero keep their K and size"""
    from . import engine
    K = intrinsics(model, warn=False)
    out = {}
    for k, cid in enumerate(model.cam_id):
        w, h = int(model.cam_width[k]), int(model.cam_height[k])
        if is_distorted(model, k):
            name, prm = camera_params(model, k)
            (fx, fy, cx, cy), w, h = engine.undistort_camera(name, prm, w, h, blank_pixels, min_scale, max_scale)
            out[int(cid)] = (np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]]), w, h)
        else:
            out[int(cid)] = (K[int(cid)], w, h)
    return out


def depth_ranges(model, max_d=192, interval_scale=1.0, K=None):
    """(N, 4): depth_min, interval, depth_num, depth_max per image, the reference's expressions over the z of the image's
    observed points (with multiplicity, -1 skipped) in its camera frame"""
    E = extrinsics(model)
    K = intrinsics(model, warn=False) if K is None else K
    out = np.zeros((model.n_images, 4))
    for i in range(model.n_images):
        pts = model.obs_pt[model.obs_off[i]:model.obs_off[i + 1]]
        pts = pts[pts >= 0]
        ph = np.concatenate([model.xyz[pts], np.ones((len(pts), 1))], 1)
        zs = np.sort(np.matmul(ph, E[i].T)[:, 2])
        n = len(zs)
        dmin = zs[int(n * .01)] * 0.75
        dmax = zs[int(n * .99)] * 1.25
        if max_d == 0:   # inverse-depth sampling: one pixel at depth_min (the reference's supplementary formula)
            Ki = np.linalg.inv(K[int(model.image_cam[i])])
            R, t = E[i, :3, :3], E[i, :3, 3]
            Kc = K[int(model.image_cam[i])]
            P1 = np.matmul(np.linalg.inv(R), np.matmul(Ki, [Kc[0, 2], Kc[1, 2], 1]) * dmin - t)
            P2 = np.matmul(np.linalg.inv(R), np.matmul(Ki, [Kc[0, 2] + 1, Kc[1, 2], 1]) * dmin - t)
            num = (1 / dmin - 1 / dmax) / (1 / dmin - 1 / (dmin + np.linalg.norm(P2 - P1)))
        else:
            num = max_d
        out[i] = (dmin, (dmax - dmin) / (num - 1) / interval_scale, num, dmax)
    return out


def cam_text(E, K, rng):
    """one %08d_cam.txt: str(float) per element with a trailing space, as the reference writes it"""
    s = "extrinsic\n" + "".join("".join(str(float(v)) + " " for v in row) + "\n" for row in E)
    s += "\nintrinsic\n" + "".join("".join(str(float(v)) + " " for v in row) + "\n" for row in K)
    return s + "\n%f %f %f %f\n" % tuple(rng)


def write_cams(model, save_folder, max_d=192, interval_scale=1.0, K=None):
    """save_folder/cams/%08d_cam.txt for every image (no GPU needed); K: {camera id: 3x3} in place of the model's own
    intrinsics (the undistorted cameras)"""
    K = intrinsics(model) if K is None else K
    E = extrinsics(model)
    rngs = depth_ranges(model, max_d, interval_scale, K)
    d = os.path.join(save_folder, "cams")
    os.makedirs(d, exist_ok=True)
    for i in range(model.n_images):
        with open(os.path.join(d, "%08d_cam.txt" % i), "w") as f:
            f.write(cam_text(E[i], K[int(model.image_cam[i])], rngs[i]))


def write_pairs(path, ids, scores):
    """pair.txt: N, then per image "i" and "num_view id score id score ... " (each pair followed by a space)"""
    ids, scores = np.asarray(ids), np.asarray(scores)
    with open(path, "w") as f:
        f.write("%d\n" % len(ids))
        for i in range(len(ids)):
            f.write("%d\n%d " % (i, ids.shape[1]) + "".join("%d %d " % (k, s) for k, s in zip(ids[i], scores[i])) + "\n")


def view_select(centers_, xyz, obs_off, obs_pt, num_view, device=0, counts=False):
    """mpmvs_view_select on host arrays: (ids, scores) of shape (N, num_view); with counts=True also the (N, N) shared /
    small counts of every pair i < j (upper triangle)"""
    from . import engine
    _, fns = engine.load()
    c = np.ascontiguousarray(centers_, np.float64).reshape(-1, 3)
    x = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
    off = np.ascontiguousarray(obs_off, np.int64)
    pt = np.ascontiguousarray(obs_pt, np.int32)
    n = len(c)
    if len(off) != n + 1 or off[-1] != len(pt):
        raise ValueError("obs_off must hold N + 1 offsets ending at len(obs_pt)")
    ids = np.zeros((n, num_view), np.int32)
    sc = np.zeros((n, num_view), np.int32)
    sh = np.zeros((n, n), np.uint32) if counts else None
    sm = np.zeros((n, n), np.uint32) if counts else None
    rc = fns["view_select"](device, n, c.ctypes.data, len(x), x.ctypes.data, off.ctypes.data, pt.ctypes.data, num_view, ids.ctypes.data,
                            sc.ctypes.data, sh.ctypes.data if counts else None, sm.ctypes.data if counts else None)
    if rc == -2:
        raise ValueError(f"view selection: {n} images, more than the {MAX_IMAGES} the dense accumulators allow")
    if rc != 0:
        raise RuntimeError(f"mpmvs_view_select failed ({rc})")
    return (ids, sc, sh, sm) if counts else (ids, sc)


def select_views(model, num_view=20, device=0):
    """per image the min(num_view, N - 1) best images by the reference's score: (ids, scores), each (N, num_view)"""
    return view_select(centers(model), model.xyz, model.obs_off, model.obs_pt, min(num_view, model.n_images - 1), device)


def _write_pnm(path, a):
    with open(path, "wb") as f:
        f.write(b"P%d\n%d %d\n255\n" % (5 if a.ndim == 2 else 6, a.shape[1], a.shape[0]))
        f.write(np.ascontiguousarray(a, np.uint8).tobytes())


def _decode_pil(src, name):
    """uint8 [h, w] (grey) or [h, w, 3] (R,G,B) of an image file PIL reads"""
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError(f"{name}: images other than JPEG are decoded with PIL, which is not installed") from e
    with Image.open(src) as im:
        if im.mode in ("L", "I;16", "I", "1"):
            return np.asarray(im.convert("L"))
        return np.asarray(im.convert("RGB"))


def _copy_image(src, name, out_dir, i):
    if os.path.splitext(name)[1] in (".jpg", ".jpeg", ".JPG"):
        shutil.copyfile(src, os.path.join(out_dir, "%08d.jpg" % i))
        return
    a = _decode_pil(src, name)
    _write_pnm(os.path.join(out_dir, "%08d.%s" % (i, "pgm" if a.ndim == 2 else "ppm")), a)


def copy_images(model, image_dir, out_dir):
    """images/%08d.jpg: JPEG files byte for byte; other formats decoded with PIL and written losslessly as .pgm / .ppm"""
    os.makedirs(out_dir, exist_ok=True)
    for i, name in enumerate(model.names):
        _copy_image(os.path.join(image_dir, name), name, out_dir, i)


def _jpeg_components(path):
    """number of colour components of a JPEG file (its frame header), 0 if none is found.  A plain walk over the marker
    segments: fill bytes (0xFF padding) in front of a marker, or a marker without a length field in front of the frame header,
    end it with 0, which the caller takes as colour -- right for a colour file; a grey file of that rare kind is then warped
    and written with three equal channels, which the pipeline reads like a grey image."""
    with open(path, "rb") as f:
        d = f.read()
    k = 2
    while k + 4 <= len(d) and d[k] == 0xFF:
        marker, size = d[k + 1], int.from_bytes(d[k + 2:k + 4], "big")
        if 0xC0 <= marker <= 0xCF and marker not in (0xC4, 0xC8, 0xCC):   # any start-of-frame marker
            return d[k + 9] if k + 9 < len(d) else 0
        if marker == 0xDA:
            break
        k += 2 + size
    return 0


def _decode(src, name):
    """uint8 [h, w] (grey) or [h, w, 3] (R,G,B): JPEG / PGM / PPM through the host library's reader, other formats through PIL"""
    ext = os.path.splitext(name)[1].lower()
    if ext in (".jpg", ".jpeg", ".pgm", ".ppm"):
        grey = ext == ".pgm" or (ext != ".ppm" and _jpeg_components(src) == 1)
        if grey:
            return hostlib.read_image(src, 1)
        return np.ascontiguousarray(hostlib.read_image(src, 3)[..., ::-1])   # B,G,R -> R,G,B
    return _decode_pil(src, name)


def undistort_images(model, image_dir, out_dir, cams, device=0):
    """images/%08d.pgm / .ppm: every image of a distorted camera warped to its camera of `cams` (undistorted_cameras) on the
    GPU and written losslessly; the images of the other cameras are copied as copy_images copies them"""
    from . import engine
    os.makedirs(out_dir, exist_ok=True)
    index = {int(cid): k for k, cid in enumerate(model.cam_id)}
    fisheye = [int(cid) for k, cid in enumerate(model.cam_id) if "FISHEYE" in CAMERA_MODELS[model.cam_model[k]] and not is_distorted(model, k)]
    if fisheye:
        print(f"warning: camera(s) {fisheye} are fisheye models whose distortion parameters are all zero; their images are copied as "
              "they are, although such a camera is no pinhole", file=sys.stderr)
    for i, name in enumerate(model.names):
        src = os.path.join(image_dir, name)
        k = index[int(model.image_cam[i])]
        if not is_distorted(model, k):
            _copy_image(src, name, out_dir, i)
            continue
        a = _decode(src, name)
        w, h = int(model.cam_width[k]), int(model.cam_height[k])
        if a.shape[:2] != (h, w):
            raise ValueError(f"{name}: the image is {a.shape[1]} x {a.shape[0]}, its camera {int(model.cam_id[k])} is {w} x {h}")
        Kn, ow, oh = cams[int(model.cam_id[k])]
        cname, prm = camera_params(model, k)
        out = engine.undistort_u8(a, cname, prm, ((Kn[0, 0], Kn[1, 1], Kn[0, 2], Kn[1, 2]), ow, oh), device)
        _write_pnm(os.path.join(out_dir, "%08d.%s" % (i, "pgm" if out.ndim == 2 else "ppm")), out)


def convert(dense_folder, save_folder, max_d=192, interval_scale=1.0, model_ext=None, num_view=20, device=0, overwrite=False,
            undistort=False, blank_pixels=0.0, min_scale=0.2, max_scale=2.0):
    """dense_folder/{images,sparse} -> save_folder/{cams,images,pair.txt}; returns the stage times (s).  Refuses to touch
    non-empty save_folder/images or /cams unless overwrite=True (which removes them first).  undistort=True: the cameras
    written are the pinhole cameras of undistorted_cameras(blank_pixels, min_scale, max_scale) and the images of distorted
    cameras are warped to them on the GPU (images/%08d.pgm / .ppm); the default expects COLMAP's undistorted dense folder."""
    cam_dir, img_dir = os.path.join(save_folder, "cams"), os.path.join(save_folder, "images")
    for d in (cam_dir, img_dir):
        if os.path.isdir(d) and os.listdir(d):
            if not overwrite:
                raise FileExistsError(f"{d} exists and is not empty (pass overwrite=True / --overwrite to replace it)")
            shutil.rmtree(d)
    os.makedirs(save_folder, exist_ok=True)
    times = {}
    t = time.perf_counter()
    model = read_model(os.path.join(dense_folder, "sparse"), model_ext)
    times["read"] = time.perf_counter() - t
    t = time.perf_counter()
    ids, scores = select_views(model, num_view, device)
    times["select"] = time.perf_counter() - t
    t = time.perf_counter()
    cams = undistorted_cameras(model, blank_pixels, min_scale, max_scale) if undistort else None
    write_cams(model, save_folder, max_d, interval_scale, {cid: c[0] for cid, c in cams.items()} if undistort else None)
    times["cams"] = time.perf_counter() - t
    t = time.perf_counter()
    write_pairs(os.path.join(save_folder, "pair.txt"), ids, scores)
    times["pairs"] = time.perf_counter() - t
    t = time.perf_counter()
    if undistort:
        undistort_images(model, os.path.join(dense_folder, "images"), img_dir, cams, device)
    else:
        copy_images(model, os.path.join(dense_folder, "images"), img_dir)
    times["images"] = time.perf_counter() - t
    return times
