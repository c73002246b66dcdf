"""Writes undistort_golden_v1.npz: an independent numpy float64 statement of the undistortion contract
-- COLMAP's camera models with np.arctan / np.tan, its own Newton inverse, the UndistortCamera rule and the bilinear warp.
Imports nothing of this repository.  Run: python tests/golden/make_undistort_golden.py"""
import os

import numpy as np

MODELS = ["SIMPLE_PINHOLE", "PINHOLE", "SIMPLE_RADIAL", "RADIAL", "OPENCV", "OPENCV_FISHEYE", "FULL_OPENCV", "FOV",
          "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE", "THIN_PRISM_FISHEYE"]
ONE_F = {"SIMPLE_PINHOLE", "SIMPLE_RADIAL", "RADIAL", "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE"}
THETA = {"SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE", "THIN_PRISM_FISHEYE"}

W, H = 24, 18
F1 = [23.0, 11.7, 9.2]                 # f cx cy
F2 = [23.0, 22.1, 11.7, 9.2]           # fx fy cx cy
# the 9 distorted models with moderate parameters
CASES = {
    "SIMPLE_RADIAL": F1 + [-0.12],
    "RADIAL": F1 + [0.09, -0.03],
    "OPENCV": F2 + [-0.11, 0.04, 0.006, -0.004],
    "OPENCV_FISHEYE": F2 + [-0.03, 0.012, -0.004, 0.0007],
    "FULL_OPENCV": F2 + [0.08, -0.02, 0.004, -0.005, 0.01, 0.03, -0.01, 0.002],
    "FOV": F2 + [0.7],
    "SIMPLE_RADIAL_FISHEYE": F1 + [0.05],
    "RADIAL_FISHEYE": F1 + [-0.04, 0.015],
    "THIN_PRISM_FISHEYE": F2 + [-0.05, 0.012, 0.004, -0.003, -0.002, 0.0004, 0.003, -0.002],
}
BLANKS = [0.0, 0.5, 1.0]


def split(name, p):
    p = [float(v) for v in p]
    if name in ONE_F:
        return p[0], p[0], p[1], p[2], p[3:]
    return p[0], p[1], p[2], p[3], p[4:]


def theta_coords(u, v):
    r = np.sqrt(u * u + v * v)
    big = r > 1e-12
    s = np.where(big, np.arctan(r) / np.where(big, r, 1.0), 1.0)
    return u * s, v * s


def distort_theta(name, k, uu, vv):
    t2 = uu * uu + vv * vv
    if name == "SIMPLE_RADIAL_FISHEYE":
        rad = k[0] * t2
        return uu + uu * rad, vv + vv * rad
    if name == "RADIAL_FISHEYE":
        rad = k[0] * t2 + k[1] * t2 ** 2
        return uu + uu * rad, vv + vv * rad
    k1, k2, p1, p2, k3, k4, sx1, sy1 = k
    rad = k1 * t2 + k2 * t2 ** 2 + k3 * t2 ** 3 + k4 * t2 ** 4
    du = uu * rad + 2 * p1 * uu * vv + p2 * (t2 + 2 * uu * uu) + sx1 * t2
    dv = vv * rad + 2 * p2 * uu * vv + p1 * (t2 + 2 * vv * vv) + sy1 * t2
    return uu + du, vv + dv


def distort(name, k, u, v):
    """normalised pinhole -> normalised distorted point"""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    r2 = u * u + v * v
    if name in ("SIMPLE_PINHOLE", "PINHOLE"):
        return u, v
    if name == "SIMPLE_RADIAL":
        rad = k[0] * r2
        return u + u * rad, v + v * rad
    if name == "RADIAL":
        rad = k[0] * r2 + k[1] * r2 * r2
        return u + u * rad, v + v * rad
    if name == "OPENCV":
        k1, k2, p1, p2 = k
        rad = k1 * r2 + k2 * r2 * r2
        return (u + u * rad + 2 * p1 * u * v + p2 * (r2 + 2 * u * u), v + v * rad + 2 * p2 * u * v + p1 * (r2 + 2 * v * v))
    if name == "FULL_OPENCV":
        k1, k2, p1, p2, k3, k4, k5, k6 = k
        rad = (1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3) / (1 + k4 * r2 + k5 * r2 ** 2 + k6 * r2 ** 3)
        return (u * rad + 2 * p1 * u * v + p2 * (r2 + 2 * u * u), v * rad + 2 * p2 * u * v + p1 * (r2 + 2 * v * v))
    if name == "OPENCV_FISHEYE":
        r = np.sqrt(r2)
        big = r > 1e-12
        th = np.arctan(r)
        thd = th * (1 + k[0] * th ** 2 + k[1] * th ** 4 + k[2] * th ** 6 + k[3] * th ** 8)
        s = np.where(big, thd / np.where(big, r, 1.0), 1.0)
        return u * s, v * s
    if name == "FOV":
        w = k[0]
        T = np.tan(w / 2)
        if w * w < 1e-12:
            f = w * w * r2 / 3 - w * w / 12 + 1
        else:
            r = np.sqrt(r2)
            small = r2 < 1e-12
            f = np.where(small, -2 * T * (4 * r2 * T * T - 3) / (3 * w), np.arctan(2 * T * r) / (np.where(small, 1.0, r) * w))
        return u * f, v * f
    uu, vv = theta_coords(u, v)
    return distort_theta(name, k, uu, vv)


def forward(name, params, u, v):
    fx, fy, cx, cy, k = split(name, params)
    xn, yn = distort(name, k, u, v)
    return fx * xn + cx, fy * yn + cy


def newton(g, tx, ty):
    """solve g(p) = t, vectorised: central differences, steps max(1e-15, |1e-6 p|), 100 iterations at most"""
    px, py = tx.copy(), ty.copy()
    for _ in range(100):
        s0, s1 = np.maximum(1e-15, np.abs(1e-6 * px)), np.maximum(1e-15, np.abs(1e-6 * py))
        gx, gy = g(px, py)
        ax, ay = g(px - s0, py)
        bx, by = g(px + s0, py)
        cx, cy = g(px, py - s1)
        dx, dy = g(px, py + s1)
        j00, j01, j10, j11 = (bx - ax) / (2 * s0), (dx - cx) / (2 * s1), (by - ay) / (2 * s0), (dy - cy) / (2 * s1)
        det = j00 * j11 - j01 * j10
        ex, ey = gx - tx, gy - ty
        stx, sty = (j11 * ex - j01 * ey) / det, (j00 * ey - j10 * ex) / det
        px, py = px - stx, py - sty
        if np.all(stx * stx + sty * sty < 1e-20):
            break
    return px, py


def cam_from_img(name, params, x, y):
    fx, fy, cx, cy, k = split(name, params)
    tx, ty = (np.asarray(x, np.float64) - cx) / fx, (np.asarray(y, np.float64) - cy) / fy
    if name in ("SIMPLE_PINHOLE", "PINHOLE"):
        return tx, ty
    if name in THETA:
        uu, vv = newton(lambda a, b: distort_theta(name, k, a, b), tx, ty)
        th = np.sqrt(uu * uu + vv * vv)
        big = th > 1e-12
        s = np.where(big, np.tan(th) / np.where(big, th, 1.0), 1.0)
        return uu * s, vv * s
    return newton(lambda a, b: distort(name, k, a, b), tx, ty)


def output_camera(name, params, w, h, blank=0.0, min_scale=0.2, max_scale=2.0, scales=None):
    fx, fy, cx, cy, _ = split(name, params)
    if name in ("SIMPLE_PINHOLE", "PINHOLE"):
        return (fx, fy, cx, cy), w, h
    ys, xs = np.arange(h) + 0.5, np.arange(w) + 0.5
    left = fx * cam_from_img(name, params, np.full(h, 0.5), ys)[0] + cx
    right = fx * cam_from_img(name, params, np.full(h, w - 0.5), ys)[0] + cx
    top = fy * cam_from_img(name, params, xs, np.full(w, 0.5))[1] + cy
    bottom = fy * cam_from_img(name, params, xs, np.full(w, h - 0.5))[1] + cy
    min_sx = min(cx / (cx - left.min()), (w - 0.5 - cx) / (right.max() - cx))
    min_sy = min(cy / (cy - top.min()), (h - 0.5 - cy) / (bottom.max() - cy))
    max_sx = max(cx / (cx - left.max()), (w - 0.5 - cx) / (right.min() - cx))
    max_sy = max(cy / (cy - top.max()), (h - 0.5 - cy) / (bottom.min() - cy))
    sx = min(max(1 / (min_sx * blank + max_sx * (1 - blank)), min_scale), max_scale)
    sy = min(max(1 / (min_sy * blank + max_sy * (1 - blank)), min_scale), max_scale)
    if scales is not None:
        scales.extend([sx * w, sy * h])
    ow, oh = int(max(1.0, sx * w)), int(max(1.0, sy * h))
    return (fx, fy, cx * ow / w, cy * oh / h), ow, oh


def warp(img, name, params, pin, ow, oh):
    """(fp64 values [oh, ow, c], valid [oh, ow]) of the byte image [h, w, c]"""
    h, w, _ = img.shape
    X, Y = np.meshgrid(np.arange(ow, dtype=np.float64), np.arange(oh, dtype=np.float64))
    x, y = forward(name, params, (X + 0.5 - pin[2]) / pin[0], (Y + 0.5 - pin[3]) / pin[1])
    sx, sy = x - 0.5, y - 0.5
    valid = (sx >= 0) & (sx <= w - 1) & (sy >= 0) & (sy <= h - 1)
    sxc, syc = np.where(valid, sx, 0.0), np.where(valid, sy, 0.0)
    x0, y0 = np.floor(sxc).astype(int), np.floor(syc).astype(int)
    ax, ay = (sxc - x0)[..., None], (syc - y0)[..., None]
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    s = img.astype(np.float64)
    top = s[y0, x0] + ax * (s[y0, x1] - s[y0, x0])
    bot = s[y1, x0] + ax * (s[y1, x1] - s[y1, x0])
    val = top + ay * (bot - top)
    return np.where(valid[..., None], val, 0.0), valid.astype(np.uint8)


# the cross-check table of the contract (640 x 480)
TABLE = [("SIMPLE_RADIAL", [600.0, 316.75, 241.5, -0.15], 0.0, (669, 491)), ("SIMPLE_RADIAL", [600.0, 316.75, 241.5, -0.15], 1.0, (695, 521)),
         ("SIMPLE_RADIAL", [600.0, 316.75, 241.5, 0.1], 0.0, (614, 459)), ("SIMPLE_RADIAL", [600.0, 316.75, 241.5, 0.1], 1.0, (622, 472)),
         ("OPENCV_FISHEYE", [300.0, 300.0, 316.75, 241.5, -0.02, 0.01, -0.003, 0.0005], 0.0, (1103, 624)),
         ("OPENCV_FISHEYE", [300.0, 300.0, 316.75, 241.5, -0.02, 0.01, -0.003, 0.0005], 1.0, (1280, 960))]


def main():
    for name, params, blank, size in TABLE:
        _, ow, oh = output_camera(name, params, 640, 480, blank)
        assert (ow, oh) == size, (name, params, blank, ow, oh, size)
    rng = np.random.default_rng(20261017)
    out = {"image3": rng.integers(0, 256, (H, W, 3), dtype=np.uint8), "image1": rng.integers(0, 256, (H, W, 1), dtype=np.uint8),
           "blanks": np.array(BLANKS), "size": np.array([W, H]), "fwd_uv": rng.uniform(-0.8, 0.8, (200, 2))}
    out["fwd_uv"][:3] = [[0, 0], [1e-14, -1e-14], [1e-7, 0]]
    scales = []
    for name, params in CASES.items():
        out["params_" + name] = np.array(params, np.float64)
        out["fwd_xy_" + name] = np.stack(forward(name, params, out["fwd_uv"][:, 0], out["fwd_uv"][:, 1]), -1)
        for b, blank in enumerate(BLANKS):
            pin, ow, oh = output_camera(name, params, W, H, blank, scales=scales)
            out["cam_%s_%d" % (name, b)] = np.array(list(pin) + [ow, oh], np.float64)
            for c in (1, 3):
                val, valid = warp(out["image%d" % c], name, params, pin, ow, oh)
                out["val%d_%s_%d" % (c, name, b)] = val
                out["valid_%s_%d" % (name, b)] = valid
    scales = np.array(scales)
    # the truncation to a size must not hang on the last bits of the inverse
    assert np.all(np.abs(scales - np.rint(scales)) >= 1e-6), scales[np.abs(scales - np.rint(scales)) < 1e-6]
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "undistort_golden_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(CASES) * len(BLANKS), "cameras")


if __name__ == "__main__":
    main()
