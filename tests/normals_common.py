"""The plain-loop statement of mpmvs_cloud_normals (include/mpmvs.h) in numpy, shared by test_normals_cpu.py
and test_normals_gpu.py.  Built on knn_common.brute_knn; everything after the list is fp64 and vectorised over the points with
elementwise + - * / sqrt and np.where masks only (numpy does not fuse, so the bits are the scalar loop's); the sums run in an
explicit loop over the list position (np.sum is not sequential)."""
import numpy as np

from knn_common import bits, brute_knn

SWEEPS = 8
PAIRS = ((0, 1, 2), (0, 2, 1), (1, 2, 0))   # p, q and the third index r


def scatter(e, m):
    """(C: {(a, b): float64 [n]} for a <= b) of the offsets e float64 [n, k, 3] (neighbour minus point), the first m [n] of each
    row counting: the sums in list order, the first term initialising"""
    n, k, _ = e.shape
    s = [np.zeros(n) for _ in range(3)]
    Q = {(a, b): np.zeros(n) for a in range(3) for b in range(a, 3)}
    for j in range(k):
        on = j < m
        for a in range(3):
            s[a] = np.where(on, e[:, j, a] if j == 0 else s[a] + e[:, j, a], s[a])
        for (a, b) in Q:
            t = e[:, j, a] * e[:, j, b]
            Q[(a, b)] = np.where(on, t if j == 0 else Q[(a, b)] + t, Q[(a, b)])
    w = (m + 1).astype(np.float64)
    return {(a, b): Q[(a, b)] - (s[a] * s[b]) / w for (a, b) in Q}


def jacobi(C, sweeps=SWEEPS):
    """(d: three float64 [n], V: 3 x 3 lists of float64 [n], off-diagonals left) after `sweeps` cyclic sweeps of the contract"""
    n = len(C[(0, 0)])
    A = {key: val.copy() for key, val in C.items()}
    V = [[np.full(n, 1.0 if i == j else 0.0) for j in range(3)] for i in range(3)]

    def key(a, b):
        return (a, b) if a <= b else (b, a)

    for _ in range(sweeps):
        for p, q, r in PAIRS:
            apq = A[key(p, q)]
            on = apq != 0.0
            theta = (A[(q, q)] - A[(p, p)]) / (2.0 * apq)
            t = np.where(theta < 0.0, -1.0, 1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
            c = 1.0 / np.sqrt(t * t + 1.0)
            s = t * c
            app, aqq = A[(p, p)] - t * apq, A[(q, q)] + t * apq
            arp, arq = A[key(r, p)], A[key(r, q)]
            nrp, nrq = c * arp - s * arq, s * arp + c * arq
            A[(p, p)], A[(q, q)] = np.where(on, app, A[(p, p)]), np.where(on, aqq, A[(q, q)])
            A[key(p, q)] = np.where(on, 0.0, apq)
            A[key(r, p)], A[key(r, q)] = np.where(on, nrp, arp), np.where(on, nrq, arq)
            for i in range(3):
                vp, vq = V[i][p], V[i][q]
                V[i][p], V[i][q] = np.where(on, c * vp - s * vq, vp), np.where(on, s * vp + c * vq, vq)
    return [A[(0, 0)], A[(1, 1)], A[(2, 2)]], V, [A[(0, 1)], A[(0, 2)], A[(1, 2)]]


def pick(d, V, m):
    """(defined bool [n], n: three float64 [n] canonically signed, curvature float64 [n], smallest eigenvalue float64 [n])"""
    d0, d1, d2 = d
    i0 = np.where(d0 <= d1, np.where(d0 <= d2, 0, 2), np.where(d1 <= d2, 1, 2))
    dmin = np.where(i0 == 0, d0, np.where(i0 == 1, d1, d2))
    o1, o2 = np.where(i0 == 0, d1, d0), np.where(i0 == 2, d1, d2)
    dmid = np.where(o1 < o2, o1, o2)
    pos = [np.where(v > 0.0, v, 0.0) for v in d]
    tr = (pos[0] + pos[1]) + pos[2]
    defined = (m >= 2) & (dmid > 0.0)
    nv = [np.where(i0 == 0, V[i][0], np.where(i0 == 1, V[i][1], V[i][2])) for i in range(3)]
    f = [np.abs(v) for v in nv]
    lead = np.where(f[0] >= f[1], np.where(f[0] >= f[2], nv[0], nv[2]), np.where(f[1] >= f[2], nv[1], nv[2]))
    flip = lead < 0.0
    nv = [np.where(flip, -v, v) for v in nv]
    curv = np.where(dmin > 0.0, dmin, 0.0) / tr
    return defined, nv, curv, dmin


def finish(defined, nv, curv, p, viewpoint=None, reference=None):
    """the sign by a viewpoint or by reference normals, the roundings to fp32 and the undefined rows"""
    if viewpoint is not None or reference is not None:
        if viewpoint is not None:
            v = np.asarray(viewpoint, np.float64)
            w = [v[a] - p[:, a] for a in range(3)]
        else:
            ref = np.ascontiguousarray(reference, np.float32).astype(np.float64)
            w = [ref[:, a] for a in range(3)]
        dot = (nv[0] * w[0] + nv[1] * w[1]) + nv[2] * w[2]
        flip = dot < 0.0
        nv = [np.where(flip, -c, c) for c in nv]
    normals = np.stack([np.where(defined, c, 0.0) for c in nv], 1).astype(np.float32)
    curvature = np.where(defined, curv, np.inf).astype(np.float32)
    return normals, curvature


def fit(e, m, p=None, viewpoint=None, reference=None):
    """the statement from the offsets on: (normals float32 [n, 3], curvature float32 [n]); p float64 [n, 3], the points, is needed
    with a viewpoint only"""
    with np.errstate(all="ignore"):
        d, V, _ = jacobi(scatter(e, m))
        defined, nv, curv, _ = pick(d, V, m)
        return finish(defined, nv, curv, p, viewpoint, reference)


def offsets(xyz, idx, rows=None):
    """(e float64 [n, k, 3], p float64 [n, 3]): the neighbours of the list idx [n, k] minus their point, exact in fp64; entries
    without a neighbour (-1) hold the point's own offset 0 and are never counted"""
    x = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    own = np.arange(len(x)) if rows is None else np.asarray(rows, np.int64)
    p = x[own].astype(np.float64)
    nb = x[np.where(idx >= 0, idx, own[:, None])].astype(np.float64)
    with np.errstate(invalid="ignore"):
        return nb - p[:, None, :], p


def statement_normals(xyz, radius, k=16, viewpoint=None, reference=None, self_rows=None, knn=None):
    """-> (normals float32 [n, 3], curvature float32 [n], within int32 [n]) as Cloud.normals(want_within=True); with self_rows (an
    index array) only those rows; reference then holds those rows' normals.  knn: a brute_knn answer for this k to reuse."""
    d2, idx, within = brute_knn(xyz, None, radius, k, self_rows=self_rows) if knn is None else knn
    e, p = offsets(xyz, idx, self_rows)
    m = np.minimum(within, k)
    normals, curvature = fit(e, m, p, viewpoint, reference)
    return normals, curvature, within


def assert_normals_same(got, want, what=""):
    """the bits of the normals and of the curvature, within exact; whichever of curvature and within `got` holds"""
    gn, gc = got[0], got[1]
    gw = got[2] if len(got) > 2 else None
    wn, wc, ww = want
    assert gn.shape == wn.shape and gn.dtype == np.float32, f"{what}: normals {gn.dtype} {gn.shape} against {wn.shape}"
    bad = (bits(gn) != bits(wn)).any(1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {len(wn)} normals differ in bits; first at {np.flatnonzero(bad)[0]}: {gn[bad][0]} against {wn[bad][0]}"
    if gc is not None:
        assert gc.shape == wc.shape and gc.dtype == np.float32
        bad = bits(gc) != bits(wc)
        assert not bad.any(), f"{what}: {int(bad.sum())} of {len(wc)} curvatures differ in bits; first at {np.flatnonzero(bad)[0]}: {gc[bad][0]} against {wc[bad][0]}"
    if gw is not None:
        assert gw.dtype == np.int32 and np.array_equal(gw, ww), f"{what}: {int((gw != ww).sum())} of {len(ww)} within differ"


def sphere_scene():
    """(xyz float32 [3000, 3], centre float64 [3]): points on a unit sphere about (3, -2, 1) with a radial jitter of +-0.002"""
    rng = np.random.default_rng(5)
    centre = np.array([3.0, -2.0, 1.0])
    u = rng.normal(size=(3000, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    r = 1.0 + rng.uniform(-0.002, 0.002, 3000)
    return (centre + u * r[:, None]).astype(np.float32), centre


def angle_to(normals, axis):
    """degrees between each normal and `axis` ([3] or [n, 3]), sign ignored"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a, axis=-1, keepdims=True)
    n = normals.astype(np.float64)
    cr = np.linalg.norm(np.cross(n, a), axis=1)
    return np.degrees(np.arctan2(cr, np.abs((n * a).sum(1))))
