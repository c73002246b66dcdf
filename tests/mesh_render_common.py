"""mpmvs_surface_render_depth as a plain statement in numpy fp64, written from include/mpmvs.h (statement 7 of the mesh section), one
numpy operation per step of the contract, with np.minimum on the uint64 keys; and the scenes of test_mesh_render_cpu.py and
test_mesh_render_gpu.py.  numpy evaluates every operation on its own and rounds it to fp64: there is no contraction."""
import importlib

import numpy as np

F = np.float32
D = np.float64
NONE = np.uint64(0x7f800000ffffffff)


def abi():
    return importlib.import_module("mp-mvs_amd._abi")


def camera(K, R, t, w, h):
    return abi().make_camera(K, R, t, h, w, 0.1, 100.0)


def pinhole(f, cx, cy, w, h, R=None, t=(0, 0, 0)):
    return camera([[f, 0, cx], [0, f, cy], [0, 0, 1]], np.eye(3) if R is None else R, t, w, h)


def look_at(eye, target, f, w, h, up=(0, 0, 1), skew=0.0, third=(0.0, 0.0, 1.0)):
    """a camera at `eye` whose z axis points at `target`; skew and a third row of K other than (0, 0, 1) on request"""
    eye, target, up = np.asarray(eye, D), np.asarray(target, D), np.asarray(up, D)
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, up)
    if np.linalg.norm(x) < 1e-9:
        x = np.cross(z, np.array([1.0, 0, 0]))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    K = [[f, skew, (w - 1) / 2], [0, f, (h - 1) / 2], list(third)]
    return camera(K, R, -R @ eye, w, h)


def cam_arrays(c):
    return (np.array(c.K[:], F).astype(D), np.array(c.R[:], F).astype(D), np.array(c.t[:], F).astype(D), int(c.width), int(c.height))


def _cross(u, v):
    return np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)


def image_vertices(xyz, tri, cam):
    """q [m, vertex, component] in fp64 and the mask of the triangles that take part"""
    K, R, t, _, _ = cam_arrays(cam)
    P = np.ascontiguousarray(xyz, F).reshape(-1, 3).astype(D)[np.ascontiguousarray(tri, np.int64).reshape(-1, 3)]
    p0, p1, p2 = P[..., 0], P[..., 1], P[..., 2]
    X = [((R[3 * j] * p0 + R[3 * j + 1] * p1) + R[3 * j + 2] * p2) + t[j] for j in range(3)]
    q = np.stack([(K[3 * j] * X[0] + K[3 * j + 1] * X[1]) + K[3 * j + 2] * X[2] for j in range(3)], -1)
    part = np.isfinite(q).all((1, 2)) & (q[:, :, 2].max(1) > 0) if len(q) else np.zeros(0, bool)
    return q, part


def view_statement(xyz, tri, cam, budget=1 << 20):
    """-> (depth float32 [H, W], tri int32 [H, W], pairs taking part, covered pixels, keys uint64 [H, W])"""
    _, _, _, W, H = cam_arrays(cam)
    keys = np.full((H, W), NONE, np.uint64)
    with np.errstate(all="ignore"):
        q, part = image_vertices(xyz, tri, cam)
        idx = np.flatnonzero(part)
        x = np.arange(W, dtype=D)[None, None, :]
        y = np.arange(H, dtype=D)[None, :, None]
        step = max(1, budget // (W * H))
        for s in range(0, len(idx), step):
            i = idx[s:s + step]
            qa, qb, qc = q[i, 0], q[i, 1], q[i, 2]
            nbc, nca, nab = _cross(qb, qc), _cross(qc, qa), _cross(qa, qb)
            det = (qa[:, 0] * nbc[:, 0] + qa[:, 1] * nbc[:, 1]) + qa[:, 2] * nbc[:, 2]
            zlo = np.minimum(np.minimum(qa[:, 2], qb[:, 2]), qc[:, 2])[:, None, None]
            zhi = np.maximum(np.maximum(qa[:, 2], qb[:, 2]), qc[:, 2])[:, None, None]
            E = [(x * n[:, 0, None, None] + y * n[:, 1, None, None]) + n[:, 2, None, None] for n in (nbc, nca, nab)]
            S = (E[0] + E[1]) + E[2]
            cand = (((E[0] >= 0) & (E[1] >= 0) & (E[2] >= 0)) | ((E[0] <= 0) & (E[1] <= 0) & (E[2] <= 0))) & (S != 0)
            z = det[:, None, None] / S
            z = np.where(z < zlo, zlo, z)
            z = np.where(z > zhi, zhi, z)
            zf = z.astype(F)
            covered = cand & np.isfinite(zf) & (zf > 0)
            key = (zf.view(np.uint32).astype(np.uint64) << np.uint64(32)) | i.astype(np.uint64)[:, None, None]
            key = np.where(covered, key, NONE)
            keys = np.minimum(keys, key.min(0))
    none = keys == NONE
    depth = (keys >> np.uint64(32)).astype(np.uint32).view(F).copy()
    depth[none] = 0
    arg = (keys & np.uint64(0xffffffff)).astype(np.uint32).view(np.int32).copy()   # 0xffffffff: -1
    return depth, arg, int(part.sum()), int((~none).sum()), keys


def statement(xyz, tri, cams):
    """-> (depths, tris, counts int64 [2]) over the views"""
    depths, tris, counts = [], [], np.zeros(2, np.int64)
    for c in cams:
        d, a, p, n, _ = view_statement(xyz, tri, c)
        depths.append(d)
        tris.append(a)
        counts += (p, n)
    return depths, tris, counts


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def mesh(xyz, tri):
    return {"xyz": np.ascontiguousarray(xyz, F).reshape(-1, 3), "tri": np.ascontiguousarray(tri, np.int32).reshape(-1, 3), "rgb": None}


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
HAND_W, HAND_H, HAND_F, HAND_C = 16, 12, 8.0, (2.0, 1.0)


def hand_camera():
    return pinhole(HAND_F, HAND_C[0], HAND_C[1], HAND_W, HAND_H)


def at_pixels(px, z):
    """the points of depth z that the hand camera projects onto the pixel coordinates px [n, 2]: exact in fp32 for small integers"""
    px = np.asarray(px, D)
    return np.stack([(px[:, 0] - HAND_C[0]) * z / HAND_F, (px[:, 1] - HAND_C[1]) * z / HAND_F, np.full(len(px), z)], 1).astype(F)


def closed_triangle_pixels(a, b, c, w, h):
    """the integer pixels of the closed triangle with integer corners, by exact integer arithmetic: written on its own"""
    out = np.zeros((h, w), bool)
    area = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
    for y in range(h):
        for x in range(w):
            e = [(q[0] - p[0]) * (y - p[1]) - (q[1] - p[1]) * (x - p[0]) for p, q in ((a, b), (b, c), (c, a))]
            out[y, x] = area != 0 and (all(v >= 0 for v in e) or all(v <= 0 for v in e))
    return out


def height_field(n=24, reverse_every=0):
    """an n x n grid of vertices over [-1, 1]^2 with a smooth height, two triangles per quad with alternating diagonals; with
    reverse_every = k every k-th triangle has its winding reversed"""
    g = np.linspace(-1, 1, n)
    X, Y = np.meshgrid(g, g)
    Z = 0.15 * np.sin(2.5 * X) * np.cos(1.7 * Y)
    xyz = np.stack([X, Y, Z], -1).reshape(-1, 3)
    tri = []
    for j in range(n - 1):
        for i in range(n - 1):
            a, b, c, d = j * n + i, j * n + i + 1, (j + 1) * n + i, (j + 1) * n + i + 1
            tri += [[a, b, d], [a, d, c]] if (i + j) % 2 == 0 else [[a, b, c], [b, d, c]]
    tri = np.array(tri, np.int32)
    if reverse_every:
        tri[::reverse_every] = tri[::reverse_every, ::-1]
    return mesh(xyz, tri)


def height_field_cameras(w=96, h=64):
    """four cameras above the field that look into its interior from so near that the field fills the image"""
    out = []
    for eye, target in (((0.0, 0.0, 0.6), (0.05, 0.02, 0.0)), ((0.3, -0.2, 0.5), (0.2, -0.05, 0.0)), ((-0.35, 0.3, 0.45), (-0.2, 0.2, 0.0)), ((0.1, 0.4, 0.55), (0.0, 0.25, 0.0))):
        out.append(look_at(eye, target, 80.0, w, h, up=(0, 1, 0)))
    return out


def fills_image(cam, lo=-0.15, hi=0.15, half=1.0):
    """every pixel's ray meets the planes z = hi and z = lo inside |x|, |y| < half: a graph over [-half, half]^2 with heights in
    [lo, hi] is crossed by every ray, so it fills the image.  Written without the renderer."""
    K, R, t, W, H = cam_arrays(cam)
    Ri = np.linalg.inv(R.reshape(3, 3))
    o = -Ri @ t
    x, y = np.meshgrid(np.arange(W, dtype=D), np.arange(H, dtype=D))
    d = np.einsum("ij,hwj->hwi", Ri @ np.linalg.inv(K.reshape(3, 3)), np.stack([x, y, np.ones_like(x)], -1))
    ok = d[..., 2] < 0   # looking down
    for zp in (lo, hi):
        s = (zp - o[2]) / d[..., 2]
        p = o + s[..., None] * d
        ok &= (s > 0) & (np.abs(p[..., 0]) < half) & (np.abs(p[..., 1]) < half)
    return bool(ok.all()) and o[2] > hi


CUBE_HALF = float(F(0.7))   # the vertices are fp32: the analytic box is the one they span


def cube():
    s = CUBE_HALF
    xyz = np.array([[x, y, z] for z in (-s, s) for y in (-s, s) for x in (-s, s)], F)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    tri = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    return mesh(xyz, tri)


def cube_cameras(n=12, w=64, h=48, seed=5):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        eye = d * rng.uniform(2.0, 4.0)
        out.append(look_at(eye, rng.uniform(-0.2, 0.2, 3), rng.uniform(40.0, 70.0), w, h))
    return out


def ray_box(cam, half, slack=1e-9):
    """per pixel of a camera with K's third row (0, 0, 1): the depth (along the camera's z axis) at which its ray enters the box
    [-half, half]^3, by the slab test in fp64 on the camera's own fp32 numbers -> (hit, miss, depth): hit where the ray passes the
    box by more than `slack` in the slab parameter, miss where it stays out by more than that; silhouette ties are in neither"""
    K, R, t, W, H = cam_arrays(cam)
    K, R = K.reshape(3, 3), R.reshape(3, 3)
    Ri = np.linalg.inv(R)   # not the transpose: R rounded to fp32 is orthonormal only to 1e-7
    o = -Ri @ t
    x, y = np.meshgrid(np.arange(W, dtype=D), np.arange(H, dtype=D))
    d_cam = np.einsum("ij,hwj->hwi", np.linalg.inv(K), np.stack([x, y, np.ones_like(x)], -1))   # z component 1: the parameter is the depth
    d = np.einsum("ij,hwj->hwi", Ri, d_cam)
    with np.errstate(all="ignore"):
        t1, t2 = (-half - o) / d, (half - o) / d
    near, far = np.minimum(t1, t2).max(-1), np.maximum(t1, t2).min(-1)
    hit = (far - near > slack) & (far > slack)
    miss = (near - far > slack) | (far < -slack)
    return hit, miss, np.where(near > 0, near, far)


def soup(seed):
    """a seeded triangle soup of 50 to 2000 triangles around the origin, 1 % of its vertices non-finite, with repeated indices, and
    four cameras: inside, outside, looking away, and a tiny image"""
    rng = np.random.default_rng(1000 + seed)
    m = int(rng.integers(50, 2001))
    n = max(3, m // 2)
    xyz = rng.uniform(-1.5, 1.5, (n, 3)).astype(F)
    bad = rng.random(n) < 0.01
    xyz[bad, rng.integers(0, 3, int(bad.sum()))] = rng.choice([np.nan, np.inf, -np.inf], int(bad.sum()))
    centre = rng.integers(0, n, m)
    tri = np.stack([centre, rng.integers(0, n, m), rng.integers(0, n, m)], 1).astype(np.int32)
    near = rng.random(m) < 0.7   # most triangles small: a corner and two vertices near it
    local = (xyz[centre][:, None] + rng.normal(0, 0.08, (m, 2, 3))).astype(F)
    xyz = np.concatenate([xyz, local.reshape(-1, 3)])
    tri[near, 1] = n + 2 * np.flatnonzero(near)
    tri[near, 2] = n + 2 * np.flatnonzero(near) + 1
    rep = rng.random(m) < 0.03
    tri[rep, 1] = tri[rep, 0]
    sizes = [(1, 1), (5, 4), (50, 37), (96, 64)]
    w, h = sizes[seed % 4]
    f = float(rng.uniform(0.6, 1.4) * w)
    cams = [look_at(rng.uniform(-0.3, 0.3, 3), rng.uniform(-1, 1, 3), f, w, h),                                   # inside
            look_at((3.0, 0.4, 0.3), (0, 0, 0), f, w, h, skew=0.01 * f, third=(1e-4, -2e-4, 1.0)),                 # outside
            look_at((4.0, 0.0, 0.0), (8.0, 0.1, 0.0), f, w, h)]                                                    # looking away
    w2, h2 = sizes[(seed + 1) % 4]
    cams.append(look_at(rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3), float(w2), w2, h2))
    return mesh(xyz, tri), cams


SOUP_CASES = 24

_cache = {}


def cached(name, make):
    """a reference computed once and shared among the tests that need it; never changed"""
    if name not in _cache:
        _cache[name] = make()
    return _cache[name]
