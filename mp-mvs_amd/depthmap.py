"""Depth maps against ground truth, per view: the score of an estimated map, readers for two
ground-truth file formats, and the camera of a map that is smaller than its image.  numpy on the host: a view is a few
megabytes.  The ground truth of a scan comes from cloud.Cloud.render_depth (the GPU z-buffer render); tools/eval_depth.py puts
the pieces together."""
import copy
import re

import numpy as np


def score(est, gt, tolerances, relative=False):
    """One estimated depth map against its ground truth.

    G = the pixels where gt is finite and > 0; E = those of G where est is finite and > 0.  err = |est - gt| in fp32; the bound
    of tolerance t is t (fp32), or t * gt (an fp32 product) with relative=True; within = the number of E pixels with
    err <= bound (inclusive).  Returns {"n_gt", "n_est", "relative", "median_error" (of err over E in fp64, None if E is empty),
    "tolerances": [{"tolerance", "within", "completeness" = within / n_gt, "accuracy" = within / n_est}]}; a share with an
    empty denominator is 0."""
    est, gt = np.asarray(est, np.float32), np.asarray(gt, np.float32)
    if est.shape != gt.shape:
        raise ValueError(f"the estimate is {est.shape}, the ground truth {gt.shape}")
    with np.errstate(invalid="ignore"):
        G = np.isfinite(gt) & (gt > 0)
        E = G & np.isfinite(est) & (est > 0)
    e, g = est[E], gt[E]
    err = np.abs(e - g)
    res = {"n_gt": int(G.sum()), "n_est": int(E.sum()), "relative": bool(relative),
           "median_error": float(np.median(err.astype(np.float64))) if err.size else None, "tolerances": []}
    for t in tolerances:
        bound = np.float32(t) * g if relative else np.float32(t)
        res["tolerances"].append({"tolerance": float(t), "within": int((err <= bound).sum())})
    return _shares(res)


def _shares(res):
    for r in res["tolerances"]:
        r["completeness"] = r["within"] / res["n_gt"] if res["n_gt"] else 0.0
        r["accuracy"] = r["within"] / res["n_est"] if res["n_est"] else 0.0
    return res


def pool(scores):
    """the score of all views together: the counts of score() summed, the shares from the sums (no pooled median)"""
    scores = list(scores)
    if not scores:
        return {"n_gt": 0, "n_est": 0, "tolerances": []}
    tol = [r["tolerance"] for r in scores[0]["tolerances"]]
    for s in scores:
        if [r["tolerance"] for r in s["tolerances"]] != tol or s.get("relative") != scores[0].get("relative"):
            raise ValueError("the scores were taken at different tolerances")
    res = {"n_gt": sum(s["n_gt"] for s in scores), "n_est": sum(s["n_est"] for s in scores), "relative": scores[0].get("relative", False),
           "tolerances": [{"tolerance": t, "within": sum(s["tolerances"][k]["within"] for s in scores)} for k, t in enumerate(tol)]}
    return _shares(res)


def _clean(a):
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(a) & (a > 0), a, np.float32(0.0)).astype(np.float32)


def read_eth3d_depth(path, width, height):
    """ETH3D's raw ground-truth depth file: width * height little-endian fp32 values, row-major, nothing else -> float32 [H, W];
    non-finite and non-positive values (the files mark "no depth" with inf) become 0.  ValueError on any other size."""
    with open(path, "rb") as f:
        data = f.read()
    if width <= 0 or height <= 0 or len(data) != width * height * 4:
        raise ValueError(f"{path}: {len(data)} bytes, a {width} x {height} fp32 map has {width * height * 4}")
    return _clean(np.frombuffer(data, "<f4").reshape(height, width))


def read_colmap_map(path):
    """COLMAP's depth / normal map file: the ASCII header "W&H&C&", then W * H * C little-endian fp32 values, row-major with
    the channel last -> float32 [H, W] for C = 1, [H, W, C] otherwise (values as stored).  ValueError on a malformed header or a
    body of another size."""
    with open(path, "rb") as f:
        data = f.read()
    m = re.match(rb"(\d{1,9})&(\d{1,9})&(\d{1,9})&", data)
    if not m:
        raise ValueError(f"{path}: no 'W&H&C&' header")
    w, h, c = (int(v) for v in m.groups())
    body = len(data) - m.end()
    if w <= 0 or h <= 0 or c <= 0 or body != w * h * c * 4:
        raise ValueError(f"{path}: header {w}&{h}&{c}& needs {w * h * c * 4} bytes, the file holds {body}")
    a = np.frombuffer(data, "<f4", w * h * c, m.end()).astype(np.float32)
    return a.reshape(h, w) if c == 1 else a.reshape(h, w, c)


def write_colmap_map(path, arr):
    """the inverse of read_colmap_map"""
    a = np.ascontiguousarray(arr, "<f4")
    h, w = a.shape[:2]
    c = 1 if a.ndim == 2 else a.shape[2]
    with open(path, "wb") as f:
        f.write(b"%d&%d&%d&" % (w, h, c))
        f.write(a.tobytes())


def camera_at_size(cam, image_w, image_h, map_w, map_h):
    """the camera of a map_w x map_h map of an image_w x image_h view, as fusion rescales it: sx = map_w / (float)image_w and
    sy likewise in fp32; K[0] and K[2] times sx, K[4] and K[5] times sy (fp32 products); width and height the map's"""
    out = copy.copy(cam)   # a ctypes structure: its own buffer
    sx = np.float32(map_w) / np.float32(image_w)
    sy = np.float32(map_h) / np.float32(image_h)
    for k, s in ((0, sx), (2, sx), (4, sy), (5, sy)):
        out.K[k] = float(np.float32(cam.K[k]) * s)
    out.width, out.height = int(map_w), int(map_h)
    return out
