"""Writes tests/golden/colmap_v1: a small COLMAP dense folder (images/ + sparse/ as both .txt and .bin) for the converter
tests, and -- given --reference <colmap2mvsnet_acm.py> -- the reference converter's outputs for it (expected_d192/,
expected_d0/: cams/ and pair.txt).  The reference runs in a child process on the CPU with two shims: an empty stand-in
`cv2` module (every fixture image is a .jpg, which it copies without OpenCV) and np.asscalar = a.item() (removed in
NumPy 1.23).

    python tests/golden/make_colmap_golden.py [--reference path/to/colmap2mvsnet_acm.py]

The model: 14 images with non-contiguous ids written out of order, a PINHOLE and a SIMPLE_RADIAL camera, 700 points,
-1 entries and duplicated ids in some images' point lists, two nearly co-located cameras (their many shared points
are zeroed by the 1-degree rule), and no triangulation angle within 1e-6 degrees of 1 degree."""
import argparse
import os
import shutil
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "colmap_v1")
W, H = 64, 48


def _colmap():
    import importlib
    root = os.path.dirname(os.path.dirname(HERE))
    if root not in sys.path:
        sys.path.insert(0, root)
    return importlib.import_module("mp-mvs_amd.colmap")


def rotmat2qvec(R):
    """rotation -> unit quaternion (w, x, y, z), w >= 0 (Shepperd's method)"""
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    else:
        k = int(np.argmax(np.diag(R)))
        i, j = (k + 1) % 3, (k + 2) % 3
        s = np.sqrt(1.0 + R[k, k] - R[i, i] - R[j, j]) * 2
        q = [0.0] * 4
        q[0] = (R[j, i] - R[i, j]) / s
        q[1 + k] = 0.25 * s
        q[1 + i] = (R[i, k] + R[k, i]) / s
        q[1 + j] = (R[j, k] + R[k, j]) / s
    q = np.array(q)
    q /= np.linalg.norm(q)
    return -q if q[0] < 0 else q


def look_at(c, target):
    z = target - c
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return np.stack([x, y, z])


def make_model(seed=7):
    rng = np.random.default_rng(seed)
    n = 14
    ids = np.sort(rng.choice(np.arange(1, 300), n, replace=False))
    ang = np.linspace(-0.9, 0.9, n - 1)
    cen = [np.array([6 * np.sin(a), 0.3 * np.cos(3 * a), -6 * np.cos(a)]) for a in ang]
    cen.insert(5, cen[4] + np.array([0.012, -0.004, 0.003]))   # nearly co-located with image 4
    cams = {3: ("PINHOLE", [58.5, 57.25, 32.0, 24.0]), 7: ("SIMPLE_RADIAL", [60.0, 31.5, 23.5, 0.0125])}
    imgs = []
    for i in range(n):
        R = look_at(cen[i], rng.normal(0, 0.2, 3))
        q = np.round(rotmat2qvec(R), 9)
        q /= np.linalg.norm(q)
        Rq = _colmap().qvec2rotmat(q)
        t = np.round(-Rq @ cen[i], 6)
        imgs.append(dict(id=int(ids[i]), q=q, t=t, cam=3 if i % 3 else 7, name="img_%03d.jpg" % ids[i], pts=[]))
    npts = 700
    xyz = np.round(rng.uniform(-1.5, 1.5, (npts, 3)), 3)
    pids = rng.choice(np.arange(1, 100000), npts, replace=False)
    for k in range(npts):
        m = int(rng.choice([2, 2, 2, 3, 3, 4]))
        if k < 120:   # the co-located pair sees these, with 0-2 other images
            sees = [4, 5] + list(rng.choice([i for i in range(n) if i not in (4, 5)], m - 2, replace=False))
        else:
            sees = list(rng.choice(n, m, replace=False))
        for i in sees:
            imgs[i]["pts"].append(k)
    for i, im in enumerate(imgs):
        p = list(rng.permutation(im["pts"]))
        if i in (2, 9):   # duplicated ids in the list
            p += p[:5]
        for _ in range(int(rng.integers(3, 8))):   # entries without a 3D point
            p.insert(int(rng.integers(0, len(p) + 1)), -1)
        im["pts"] = p
    return cams, imgs, pids, xyz


def check_angles(imgs, xyz):
    """every triangulation angle the score counts stays 1e-6 degrees away from 1 degree"""
    colmap = _colmap()
    order = sorted(range(len(imgs)), key=lambda i: imgs[i]["id"])
    C = [-(colmap.qvec2rotmat(imgs[i]["q"]).T @ imgs[i]["t"]) for i in order]
    sets = [set(p for p in imgs[i]["pts"] if p >= 0) for i in order]
    worst = 1e9
    for a in range(len(order)):
        for b in range(a + 1, len(order)):
            for p in sets[a] & sets[b]:
                u, v = C[a] - xyz[p], C[b] - xyz[p]
                th = np.degrees(np.arccos(u @ v / np.linalg.norm(u) / np.linalg.norm(v)))
                worst = min(worst, abs(th - 1.0))
    assert worst > 1e-6, worst
    return worst


def write_txt(d, cams, imgs, pids, xyz):
    with open(os.path.join(d, "cameras.txt"), "w") as f:
        f.write("# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n")
        for cid, (model, prm) in cams.items():
            f.write("%d %s %d %d %s\n" % (cid, model, W, H, " ".join(repr(float(v)) for v in prm)))
    track = {}
    with open(os.path.join(d, "images.txt"), "w") as f:
        f.write("# Image list with two lines of data per image:\n#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME\n"
                "#   POINTS2D[] as (X, Y, POINT3D_ID)\n")
        for im in imgs[::-1][3:] + imgs[::-1][:3]:   # not in id order
            f.write("%d %s %s %d %s\n" % (im["id"], " ".join(repr(float(v)) for v in im["q"]), " ".join(repr(float(v)) for v in im["t"]),
                                          im["cam"], im["name"]))
            f.write(" ".join("%.1f %.1f %d" % (1.5 + (j * 7) % W, 2.5 + (j * 5) % H, pids[p] if p >= 0 else -1) for j, p in enumerate(im["pts"])) + "\n")
            for j, p in enumerate(im["pts"]):
                if p >= 0:
                    track.setdefault(p, []).append((im["id"], j))
    with open(os.path.join(d, "points3D.txt"), "w") as f:
        f.write("# 3D point list with one line of data per point:\n#   POINT3D_ID, X, Y, Z, R, G, B, ERROR, TRACK[] as (IMAGE_ID, POINT2D_IDX)\n")
        for k in range(len(pids)):
            f.write("%d %s 0 0 0 0.5 %s\n" % (pids[k], " ".join(repr(float(v)) for v in xyz[k]), " ".join("%d %d" % t for t in track.get(k, []))))
    return track


def write_bin(d, cams, imgs, pids, xyz, track):
    models = {"PINHOLE": 1, "SIMPLE_RADIAL": 2}
    with open(os.path.join(d, "cameras.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(cams)))
        for cid, (model, prm) in cams.items():
            f.write(struct.pack("<iiQQ", cid, models[model], W, H) + struct.pack("<%dd" % len(prm), *prm))
    with open(os.path.join(d, "images.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(imgs)))
        for im in imgs[::-1][3:] + imgs[::-1][:3]:
            f.write(struct.pack("<i4d3di", im["id"], *im["q"], *im["t"], im["cam"]) + im["name"].encode() + b"\0")
            f.write(struct.pack("<Q", len(im["pts"])))
            for j, p in enumerate(im["pts"]):
                f.write(struct.pack("<ddq", 1.5 + (j * 7) % W, 2.5 + (j * 5) % H, int(pids[p]) if p >= 0 else -1))
    with open(os.path.join(d, "points3D.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(pids)))
        for k in range(len(pids)):
            tr = track.get(k, [])
            f.write(struct.pack("<Q3d3Bd", int(pids[k]), *xyz[k], 128, 128, 128, 0.5) + struct.pack("<Q", len(tr)))
            f.write(b"".join(struct.pack("<ii", *t) for t in tr))


def write_images(d, imgs):
    from PIL import Image
    os.makedirs(d, exist_ok=True)
    yy, xx = np.mgrid[0:H, 0:W]
    for k, im in enumerate(imgs):
        a = (96 + 60 * np.sin(xx / (5.0 + k) + yy / 9.0)).astype(np.uint8)
        Image.fromarray(a).save(os.path.join(d, im["name"]), "JPEG", quality=40)


def run_reference(script, dense, max_d, dest):
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "cv2.py"), "w").close()
        save = os.path.join(tmp, "out")
        code = ("import sys, runpy, numpy as np\n"
                "np.asscalar = lambda a: a.item()\n"
                "sys.argv = [sys.argv[1], '--dense_folder', sys.argv[2], '--save_folder', sys.argv[3], '--max_d', sys.argv[4], '--model_ext', '.txt']\n"
                "runpy.run_path(sys.argv[0], run_name='__main__')\n")
        env = dict(os.environ, PYTHONPATH=tmp, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
        subprocess.check_call([sys.executable, "-c", code, script, dense, save, str(max_d)], env=env, stdout=subprocess.DEVNULL)
        if os.path.exists(dest):
            shutil.rmtree(dest)
        os.makedirs(dest)
        shutil.copytree(os.path.join(save, "cams"), os.path.join(dest, "cams"))
        shutil.copyfile(os.path.join(save, "pair.txt"), os.path.join(dest, "pair.txt"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None, help="the reference's colmap2mvsnet_acm.py: record its outputs too")
    a = ap.parse_args()
    cams, imgs, pids, xyz = make_model()
    print("closest angle to 1 degree: %.3g degrees away" % check_angles(imgs, xyz))
    sparse = os.path.join(OUT, "sparse")
    os.makedirs(sparse, exist_ok=True)
    track = write_txt(sparse, cams, imgs, pids, xyz)
    write_bin(sparse, cams, imgs, pids, xyz, track)
    write_images(os.path.join(OUT, "images"), imgs)
    if a.reference:
        for max_d in (192, 0):
            run_reference(os.path.abspath(a.reference), OUT, max_d, os.path.join(OUT, "expected_d%d" % max_d))


if __name__ == "__main__":
    main()
