"""Shared helpers of the undistortion tests: the recorded fixture (tests/golden/make_undistort_golden.py), parameter sets of
all 11 camera models, and the end-to-end scene -- the grid scene rendered through SIMPLE_RADIAL cameras, its COLMAP export
and the pinhole yardstick at the undistorted cameras."""
import os
from dataclasses import dataclass

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "undistort_golden_v1.npz")
MODELS = ["SIMPLE_PINHOLE", "PINHOLE", "SIMPLE_RADIAL", "RADIAL", "OPENCV", "OPENCV_FISHEYE", "FULL_OPENCV", "FOV",
          "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE", "THIN_PRISM_FISHEYE"]
DISTORTED = MODELS[2:]
BLANKS = [0.0, 0.5, 1.0]

# the cross-check table of DESIGN.md section 12 (640 x 480)
_SR, _FE = [600.0, 316.75, 241.5], [300.0, 300.0, 316.75, 241.5, -0.02, 0.01, -0.003, 0.0005]
TABLE = [("SIMPLE_RADIAL", _SR + [-0.15], 0.0, (669, 491)), ("SIMPLE_RADIAL", _SR + [-0.15], 1.0, (695, 521)),
         ("SIMPLE_RADIAL", _SR + [0.1], 0.0, (614, 459)), ("SIMPLE_RADIAL", _SR + [0.1], 1.0, (622, 472)),
         ("OPENCV_FISHEYE", _FE, 0.0, (1103, 624)), ("OPENCV_FISHEYE", _FE, 1.0, (1280, 960))]


def golden():
    return np.load(GOLDEN)


def model_params(name, w, h):
    """moderate parameters of camera model `name` for a w x h image (file order)"""
    f, cx, cy = 0.95 * w, 0.49 * w + 0.3, 0.51 * h - 0.2
    one, two = [f, cx, cy], [f, 0.97 * f, cx, cy]
    return {
        "SIMPLE_PINHOLE": one, "PINHOLE": two, "SIMPLE_RADIAL": one + [-0.12], "RADIAL": one + [0.09, -0.03],
        "OPENCV": two + [-0.11, 0.04, 0.006, -0.004], "OPENCV_FISHEYE": two + [-0.03, 0.012, -0.004, 0.0007],
        "FULL_OPENCV": two + [0.08, -0.02, 0.004, -0.005, 0.01, 0.03, -0.01, 0.002], "FOV": two + [0.7],
        "SIMPLE_RADIAL_FISHEYE": one + [0.05], "RADIAL_FISHEYE": one + [-0.04, 0.015],
        "THIN_PRISM_FISHEYE": two + [-0.05, 0.012, 0.004, -0.003, -0.002, 0.0004, 0.003, -0.002],
    }[name]


def border_points(w, h):
    """the image points the output-camera rule sends through the inverse"""
    ys, xs = np.arange(h) + 0.5, np.arange(w) + 0.5
    return np.concatenate([np.stack([np.full(h, 0.5), ys], -1), np.stack([np.full(h, w - 0.5), ys], -1),
                           np.stack([xs, np.full(w, 0.5)], -1), np.stack([xs, np.full(w, h - 0.5)], -1)])


# ---- end to end: a scene seen through SIMPLE_RADIAL cameras -----------------------------------------------------------------
# Pixel conventions: a COLMAP camera puts the centre of pixel i at i + 0.5, the synthetic renderer and the pipeline's cams at i.
# The converter hands COLMAP's principal point to the pipeline as it is (the reference's converter does the same), so for the
# normalised coordinates (u, v) of the COLMAP camera the scene ray is (u - 0.5 / f, v - 0.5 / f, 1): with it, the pinhole
# camera (f, cx', cy') of the undistorted image, read in the pipeline's convention, is exact.
def sr_distort(k, u, v):
    r2 = u * u + v * v
    return u + u * k * r2, v + v * k * r2


def sr_undistort(k, xd, yd):
    """the tests' own Newton inverse of SIMPLE_RADIAL (radial: solve r (1 + k r^2) = rd for r)"""
    rd = np.sqrt(xd * xd + yd * yd)
    r = rd.copy()
    for _ in range(60):
        r = r - (r * (1 + k * r * r) - rd) / (1 + 3 * k * r * r)
    s = np.where(rd > 0, r / np.where(rd > 0, rd, 1.0), 1.0)
    return xd * s, yd * s


def sr_output_camera(f, cx, cy, k, w, h, blank=0.0, min_scale=0.2, max_scale=2.0):
    """the UndistortCamera rule restated for SIMPLE_RADIAL: ((f, f, cx', cy'), W', H')"""
    ys, xs = np.arange(h) + 0.5, np.arange(w) + 0.5
    inv_x = lambda x, y: f * sr_undistort(k, (x - cx) / f, (y - cy) / f)[0] + cx
    inv_y = lambda x, y: f * sr_undistort(k, (x - cx) / f, (y - cy) / f)[1] + cy
    left, right = inv_x(np.full(h, 0.5), ys), inv_x(np.full(h, w - 0.5), ys)
    top, bottom = inv_y(xs, np.full(w, 0.5)), inv_y(xs, np.full(w, h - 0.5))
    min_sx = min(cx / (cx - left.min()), (w - 0.5 - cx) / (right.max() - cx))
    max_sx = max(cx / (cx - left.max()), (w - 0.5 - cx) / (right.min() - cx))
    min_sy = min(cy / (cy - top.min()), (h - 0.5 - cy) / (bottom.max() - cy))
    max_sy = max(cy / (cy - top.max()), (h - 0.5 - cy) / (bottom.min() - cy))
    sx = min(max(1 / (min_sx * blank + max_sx * (1 - blank)), min_scale), max_scale)
    sy = min(max(1 / (min_sy * blank + max_sy * (1 - blank)), min_scale), max_scale)
    ow, oh = int(max(1.0, sx * w)), int(max(1.0, sy * h))
    return (f, f, cx * ow / w, cy * oh / h), ow, oh


@dataclass
class RView:
    image: np.ndarray      # (H, W) float32, integers 0 .. 255
    gt_depth: np.ndarray   # (H, W) float32, depth along the camera z axis
    R: np.ndarray
    C: np.ndarray


def render_rays(synth, ru, rv, R, C, seed, fs):
    """synth's renderer for explicit camera-frame rays (ru, rv, 1): (image rounded to integers, depth)"""
    rc = np.stack([ru, rv, np.ones_like(ru)], -1)
    rw = rc @ R
    d = np.full(ru.shape, 5.0)
    for _ in range(24):
        d = (synth.height_field(C[0] + d * rw[..., 0], C[1] + d * rw[..., 1]) - C[2]) / rw[..., 2]
    img = synth.albedo(C[0] + d * rw[..., 0], C[1] + d * rw[..., 1], seed, fs)
    return np.rint(img.astype(np.float32)).astype(np.float32), d.astype(np.float32)


def render_distorted(synth, v, w, h, f, cx, cy, k, fs):
    """view v (R, C) through the SIMPLE_RADIAL camera (f, cx, cy, k) of a cameras file"""
    i, j = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    u, q = sr_undistort(k, (i + 0.5 - cx) / f, (j + 0.5 - cy) / f)
    img, d = render_rays(synth, u - 0.5 / f, q - 0.5 / f, v.R, v.C, synth.SCENE_SEED, fs)
    return RView(img, d, v.R, v.C)


def render_pinhole(synth, v, pin, w, h, fs):
    """view v (R, C) through the pinhole (fx, fy, cx, cy) in the pipeline's convention (pixel centres at integers)"""
    i, j = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    img, d = render_rays(synth, (i - pin[2]) / pin[0], (j - pin[3]) / pin[1], v.R, v.C, synth.SCENE_SEED, fs)
    return RView(img, d, v.R, v.C)


def rotmat2qvec(R):
    w = np.sqrt(max(0.0, 1.0 + np.trace(R))) / 2
    q = np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])
    return q / np.linalg.norm(q)


def quat_rotation(q):
    """the rotation matrix of the unit quaternion (w, x, y, z)"""
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def export_colmap_sr(views, dense, f, cx, cy, k, stride=3):
    """the distorted renders as a COLMAP dense folder: ONE shared SIMPLE_RADIAL camera, PNG images, points = GT-depth
    back-projections observed where they project inside a view and agree with that view's GT depth (1 %)"""
    from PIL import Image
    os.makedirs(os.path.join(dense, "images"))
    os.makedirs(os.path.join(dense, "sparse"))
    H, W = views[0].image.shape
    ids = [10 + 7 * i for i in range(len(views))]
    obs = [[] for _ in views]
    pts = []
    for v in views:
        ii, jj = np.meshgrid(np.arange(1, W - 1, stride, dtype=np.float64), np.arange(1, H - 1, stride, dtype=np.float64))
        d = v.gt_depth[jj.astype(int), ii.astype(int)].astype(np.float64)
        u, q = sr_undistort(k, (ii + 0.5 - cx) / f, (jj + 0.5 - cy) / f)
        ray = np.stack([u - 0.5 / f, q - 0.5 / f, np.ones_like(u)], -1) * d[..., None]
        for x in ray.reshape(-1, 3) @ v.R + v.C:
            seen = []
            for j, w in enumerate(views):
                pc = w.R @ (x - w.C)
                if pc[2] <= 0:
                    continue
                xd, yd = sr_distort(k, pc[0] / pc[2] + 0.5 / f, pc[1] / pc[2] + 0.5 / f)
                px, py = f * xd + cx, f * yd + cy   # COLMAP image coordinates: pixel index + 0.5
                iu, iq = int(np.floor(px)), int(np.floor(py))
                if 0 <= iu < W and 0 <= iq < H and abs(w.gt_depth[iq, iu] - pc[2]) < 0.01 * pc[2]:
                    seen.append((j, px, py))
            if len(seen) >= 2:
                for j, px, py in seen:
                    obs[j].append((px, py, len(pts)))
                pts.append(x)
    with open(os.path.join(dense, "sparse", "cameras.txt"), "w") as fh:
        fh.write("1 SIMPLE_RADIAL %d %d %r %r %r %r\n" % (W, H, float(f), float(cx), float(cy), float(k)))
    with open(os.path.join(dense, "sparse", "images.txt"), "w") as fh:
        for i, v in enumerate(views):
            q = rotmat2qvec(v.R)
            t = -v.R @ v.C
            name = "view_%d.png" % i
            fh.write("%d %s %s 1 %s\n" % (ids[i], " ".join(repr(float(x)) for x in q), " ".join(repr(float(x)) for x in t), name))
            fh.write(" ".join("%r %r %d" % (float(a), float(b), n + 1) for a, b, n in obs[i]) + "\n")
            Image.fromarray(v.image.astype(np.uint8)).save(os.path.join(dense, "images", name))
    with open(os.path.join(dense, "sparse", "points3D.txt"), "w") as fh:
        for n, x in enumerate(pts):
            fh.write("%d %r %r %r 0 0 0 0.5\n" % (n + 1, *(float(c) for c in x)))
    return len(pts)


def read_cam_text(path):
    """(4x4 extrinsic, 3x3 intrinsic) of a %08d_cam.txt as float64"""
    tok = open(path).read().split()
    e = tok.index("extrinsic") + 1
    i = tok.index("intrinsic") + 1
    return np.array([float(t) for t in tok[e:e + 16]]).reshape(4, 4), np.array([float(t) for t in tok[i:i + 9]]).reshape(3, 3)


def gt_fraction(hostlib, folder, views):
    """share of pixels whose depth is within 5 % of the view's GT depth"""
    fr = []
    for i, v in enumerate(views):
        d = hostlib.read_dmb(os.path.join(folder, "MPMVS", "2333_%08d" % i, "depths.dmb"))
        fr.append(np.abs(d - v.gt_depth) / v.gt_depth < 0.05)
    return float(np.mean(fr))
