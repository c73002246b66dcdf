"""The observer contract of include/mpmvs.h as a plain numpy statement: fp32 throughout, one rounded
operation per step of the contract, np.minimum.at for the maps.  The GPU tests compare with array_equal, no tolerance anywhere."""
import numpy as np

f32 = np.float32
INF = f32(np.inf)


def locate(p, S, R):
    """per point of p [n, 3] for the scanner at S: (takes part, face, px, py, z); face / px / py are 0 where it takes no part"""
    p, S = np.ascontiguousarray(p, f32).reshape(-1, 3), np.asarray(S, f32)
    row = np.arange(len(p))
    with np.errstate(all="ignore"):
        d = p - S                        # one fp32 subtraction per axis
        A = np.abs(d)
        fin = np.isfinite(p).all(1)
        m = np.argmax(np.where(fin[:, None], A, f32(0)), 1)   # the lowest axis that attains the maximum
        z = A[row, m]
        part = fin & np.isfinite(z) & (z > 0)
        zs = np.where(part, z, f32(1))
        db, dc = np.where(part, d[row, (m + 1) % 3], f32(0)), np.where(part, d[row, (m + 2) % 3], f32(0))
        h = f32(R) * f32(0.5)
        qb, qc = db / zs, dc / zs        # correctly rounded quotients
        tb, tc = h * qb, h * qc
        x, y = tb + h, tc + h
    assert x.dtype == f32 and y.dtype == f32 and z.dtype == f32
    px = np.where(x >= f32(R), R - 1, x.astype(np.int64))
    py = np.where(y >= f32(R), R - 1, y.astype(np.int64))
    face = 2 * m + (d[row, m] < 0)
    assert ((px >= 0) & (px < R) & (py >= 0) & (py < R))[part].all()
    return part, np.where(part, face, 0), np.where(part, px, 0), np.where(part, py, 0), z


def window_min(Zc, w):
    """Zn of a [6, R, R] map: the minimum over the (2 w + 1)^2 window clipped to the face"""
    R = Zc.shape[1]
    pad = np.full((6, R + 2 * w, R + 2 * w), INF, f32)
    pad[:, w:w + R, w:w + R] = Zc
    Zn = Zc.copy()
    for dy in range(2 * w + 1):
        for dx in range(2 * w + 1):
            Zn = np.minimum(Zn, pad[:, dy:dy + R, dx:dx + R])
    return Zn


def maps(scan, scanners, R, w, owner=None):
    """(Zc, Zn), each float32 [n_scanners, 6, R, R]"""
    scanners = np.asarray(scanners, f32).reshape(-1, 3)
    Zc = np.full((len(scanners), 6, R, R), INF, f32)
    for j, S in enumerate(scanners):
        part, f, px, py, z = locate(scan, S, R)
        if owner is not None:
            part = part & (np.asarray(owner) == j)
        np.minimum.at(Zc[j], (f[part], py[part], px[part]), z[part])
    return Zc, np.stack([window_min(Z, w) for Z in Zc])


def classify(q, scanners, Zn, rel, ab, placed=None):
    """(free int32 [n], covered int32 [n]) of the queries q against Zn [n_scanners, 6, R, R]; placed: [locate(q, S, R) for S in
    scanners], for a caller that classifies the same queries at several margins"""
    scanners = np.asarray(scanners, f32).reshape(-1, 3)
    R = Zn.shape[2]
    n = len(np.asarray(q).reshape(-1, 3))
    free, cov = np.zeros(n, np.int32), np.zeros(n, np.int32)
    m1 = f32(1.0) - f32(rel)
    for j, S in enumerate(scanners):
        part, f, px, py, z = placed[j] if placed is not None else locate(q, S, R)
        zn = Zn[j][f, py, px]
        c = part & np.isfinite(zn)
        with np.errstate(all="ignore"):
            lhs, rhs = z + f32(ab), zn * m1
        assert lhs.dtype == f32 and rhs.dtype == f32
        free += c & (lhs < rhs)
        cov += c
    return free, cov


def junk_cloud(rng, n, scanners, lo=-2.0, hi=2.0):
    """n points in a box with about 1 % NaN / +-inf / 1e30 / 3e38 coordinates, and points that equal a scanner (z == 0)"""
    xyz = rng.uniform(lo, hi, (n, 3)).astype(f32)
    bad = rng.choice(n, max(n // 100, 1), replace=False)
    vals = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 3e38, -3e38], f32)
    xyz[bad, rng.integers(0, 3, len(bad))] = vals[rng.integers(0, len(vals), len(bad))]
    at = rng.choice(n, min(n, 4 * len(scanners)), replace=False)
    xyz[at] = np.asarray(scanners, f32).reshape(-1, 3)[np.arange(len(at)) % len(scanners)]
    return xyz


def room():
    """the end-to-end scene: a 0.02 lattice on the six inside walls of [-1, 1]^3 with a 0.4 x 0.4 opening in the +x wall (60 806
    points), one scanner, and the four groups of reconstruction points"""
    g = np.arange(-1, 1.0001, 0.02)
    U, V = (a.ravel() for a in np.meshgrid(g, g, indexing="ij"))
    walls = []
    for ax in range(3):
        for s in (-1.0, 1.0):
            P = np.zeros((len(U), 3))
            P[:, ax], P[:, (ax + 1) % 3], P[:, (ax + 2) % 3] = s, U, V
            if ax == 0 and s == 1.0:
                P = P[~((np.abs(P[:, 1]) < 0.2) & (np.abs(P[:, 2]) < 0.2))]
            walls.append(P)
    scan = np.concatenate(walls).astype(f32)
    assert len(scan) == 60806
    S = np.array([0.2, -0.1, 0.3], f32)
    rng = np.random.default_rng(7)

    def shell(n, r0, r1, c):
        v = rng.normal(size=(n, 3))
        v /= np.linalg.norm(v, axis=1)[:, None]
        return (c + v * rng.uniform(r0, r1, (n, 1))).astype(f32)

    floaters = shell(500, 0.05, 0.5, S)
    outside = shell(500, 4.0, 6.0, np.zeros(3))
    t = rng.uniform(1.5, 4.0, (200, 1))
    target = np.stack([np.ones(200), rng.uniform(-0.1, 0.1, 200), rng.uniform(-0.1, 0.1, 200)], 1)
    through = (S + (target - S) * t).astype(f32)
    return scan, S, floaters, outside, through
