"""Statements 5 and 6 of the mesh section of include/mpmvs.h in numpy, written from the header text and not from the kernels: the capped
point-to-triangle distance (distance_statement) and the surface samples (sample_statement); an independent formulation of the distance
in np.longdouble; the scenes and the seeded sweep that the CPU and the GPU tests share."""
import functools

import numpy as np

import mesh_clean_common as mc
import mesh_simplify_common as msc

F = np.float32
D = np.float64
INF_BITS = 0x7f800000


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def pair_d2(A, B, Cc, q):
    """the rule cascade on broadcastable float64 arrays [..., 3] -> (D float32, region 1..7, X float64)"""
    A, B, Cc, q = (np.asarray(v, D) for v in (A, B, Cc, q))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        ab, ac, ap, bp, cp = B - A, Cc - A, q - A, q - B, q - Cc
        s1, s2, s3, s4, s5, s6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
        vc, vb, va = s1 * s4 - s3 * s2, s5 * s2 - s1 * s6, s3 * s6 - s5 * s4
        full = np.broadcast(ab, ap).shape
        c1 = (s1 <= 0) & (s2 <= 0)
        c2 = (s3 >= 0) & (s4 <= s3)
        c3 = (vc <= 0) & (s1 >= 0) & (s3 <= 0)
        c4 = (s6 >= 0) & (s5 <= s6)
        c5 = (vb <= 0) & (s2 >= 0) & (s6 <= 0)
        c6 = (va <= 0) & ((s4 - s3) >= 0) & ((s5 - s6) >= 0)
        v3 = (s1 / (s1 - s3))[..., None]
        w5 = (s2 / (s2 - s6))[..., None]
        w6 = ((s4 - s3) / ((s4 - s3) + (s5 - s6)))[..., None]
        den = (va + vb) + vc
        v7, w7 = (vb / den)[..., None], (vc / den)[..., None]
        X = (A + v7 * ab) + w7 * ac
        region = np.full(full[:-1], 7, np.int8)
        for cond, x, r in ((c6, B + w6 * (Cc - B), 6), (c5, A + w5 * ac, 5), (c4, Cc, 4), (c3, A + v3 * ab, 3), (c2, B, 2), (c1, A, 1)):   # the first rule wins
            X = np.where(cond[..., None], np.broadcast_to(x, full), X)
            region = np.where(cond, np.int8(r), region)
        e = q - X
        dd = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
        return dd.astype(F), region, X


def distance_statement(xyz, tri, pts, radius, want_census=False, chunk=64):
    """the plain loop of statement 5 -> (d2 float32 [N], tri int32 [N], counts (2,)) [, census]"""
    xyz, pts = np.ascontiguousarray(xyz, F).reshape(-1, 3), np.ascontiguousarray(pts, F).reshape(-1, 3)
    tri = np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
    r2 = F(radius) * F(radius)
    n = len(pts)
    best, arg = np.full(n, np.inf, F), np.full(n, -1, np.int32)
    p_ok = np.isfinite(pts).all(1)
    t_ok = np.isfinite(xyz[tri]).all((1, 2)) if len(tri) else np.zeros(0, bool)
    census = {"regions": np.zeros(8, np.int64), "ties": 0, "pairs": 0, "nan_pairs": 0}
    q = pts[p_ok].astype(D)
    rows = np.flatnonzero(p_ok)
    ids = np.flatnonzero(t_ok)
    for c0 in range(0, len(ids), chunk):
        t = ids[c0:c0 + chunk]
        P = xyz[tri[t]].astype(D)   # [T, 3 corners, 3]
        d, region, _ = pair_d2(P[:, None, 0], P[:, None, 1], P[:, None, 2], q[None])
        with np.errstate(invalid="ignore"):
            cand = d <= r2
        masked = np.where(cand, d, F(np.inf))
        any_c = cand.any(0)
        low = masked.min(0) if len(t) else np.full(len(q), np.inf, F)
        attain = cand & (masked == low[None])
        first = t[np.argmax(attain, 0)]
        better = any_c & ((low < best[rows]) | (arg[rows] < 0))   # a later chunk has larger indices: it needs a strictly smaller D
        best[rows[better]], arg[rows[better]] = low[better], first[better]
        if want_census:
            census["regions"] += np.bincount(region[cand].ravel(), minlength=8)
            census["ties"] += int((attain.sum(0) > 1).sum())
            census["pairs"] += d.size
            census["nan_pairs"] += int(np.isnan(d).sum())
    counts = np.array([int((arg >= 0).sum()), int(p_ok.sum())], np.int64)
    return (best, arg, counts, census) if want_census else (best, arg, counts)


def subdivisions(xyz, tri, spacing):
    """s per triangle (0: a non-finite vertex, no sample) and the ratio, as statement 6 forms them"""
    xyz, tri = np.ascontiguousarray(xyz, F).reshape(-1, 3), np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
    P = xyz[tri].astype(D)
    ok = np.isfinite(P).all((1, 2))
    l2 = np.zeros(len(tri))
    with np.errstate(invalid="ignore"):
        for a, b in ((0, 1), (1, 2), (2, 0)):
            dlt = P[:, b] - P[:, a]
            l2 = np.maximum(l2, np.where(ok, (dlt[:, 0] * dlt[:, 0] + dlt[:, 1] * dlt[:, 1]) + dlt[:, 2] * dlt[:, 2], 0.0))
        ratio = np.sqrt(l2) / D(F(spacing))
    s = np.where(ok, np.maximum(1, np.ceil(np.where(ratio <= 4096, ratio, 0)).astype(np.int64)), 0)
    return s, np.where(ok, ratio, 0.0)


def lattice_numbers(s):
    """(na, nb, nc) int64 [s*s] in the order of k"""
    k = np.arange(s * s, dtype=np.int64)
    u = s * s - 1 - k
    g = np.floor(np.sqrt(u.astype(D))).astype(np.int64)
    g = np.where(g * g > u, g - 1, g)
    g = np.where((g + 1) * (g + 1) <= u, g + 1, g)
    i = s - 1 - g
    ell = k - (2 * s * i - i * i)
    j = ell >> 1
    odd = (ell & 1) == 1
    na, nb = np.where(odd, 3 * i + 2, 3 * i + 1), np.where(odd, 3 * j + 2, 3 * j + 1)
    return na, nb, 3 * s - na - nb


def sample_statement(xyz, tri, spacing, rgb=None, want_normals=False):
    """the plain loop of statement 6 -> {"xyz", "tri_of", "rgb", "normals"}; ValueError where the header says -3"""
    xyz, tri = np.ascontiguousarray(xyz, F).reshape(-1, 3), np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
    s_all, ratio = subdivisions(xyz, tri, spacing)
    bad = np.flatnonzero(~(ratio <= 4096))
    if len(bad):
        raise ValueError(f"triangle {bad[0]}")
    if int((s_all * s_all).sum()) > 1 << 30:
        raise ValueError(f"{int((s_all * s_all).sum())} samples")
    out_x, out_t, out_c, out_n = [], [], [], []
    for t in np.flatnonzero(s_all > 0):
        s = int(s_all[t])
        A, B, Cc = (xyz[tri[t, c]].astype(D) for c in range(3))
        na, nb, nc = lattice_numbers(s)
        fa, fb, fc = na.astype(D)[:, None], nb.astype(D)[:, None], nc.astype(D)[:, None]
        out_x.append((((fa * A + fb * B) + fc * Cc) / D(3 * s)).astype(F))
        out_t.append(np.full(s * s, t, np.int32))
        if rgb is not None:
            ca, cb, cc = (rgb[tri[t, c]].astype(np.int64) for c in range(3))
            out_c.append(((2 * (na[:, None] * ca + nb[:, None] * cb + nc[:, None] * cc) + 3 * s) // (2 * 3 * s)).astype(np.uint8))
        if want_normals:
            u, w = B - A, Cc - A
            C3 = np.array([u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]])
            with np.errstate(over="ignore", invalid="ignore"):
                L = np.sqrt((C3[0] * C3[0] + C3[1] * C3[1]) + C3[2] * C3[2])
                nh = (C3 / L).astype(F) if (L > 0 and np.isfinite(L)) else np.zeros(3, F)
            out_n.append(np.broadcast_to(nh, (s * s, 3)))
    cat = lambda parts, shape, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(shape, dt)   # noqa: E731
    return {"xyz": cat(out_x, (0, 3), F), "tri_of": cat(out_t, (0,), np.int32), "rgb": cat(out_c, (0, 3), np.uint8) if rgb is not None else None,
            "normals": cat(out_n, (0, 3), F) if want_normals else None}


def same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))


# ---- an independent formulation, in extended precision ---------------------------------------------------------------------------------
def independent_d2(A, B, Cc, q):
    """np.longdouble [...]: the minimum of the plane projection where its barycentrics are inside, and else of the three clamped
    segment distances; no rule cascade"""
    L = np.longdouble
    A, B, Cc, q = (np.asarray(v, D).astype(L) for v in (A, B, Cc, q))
    dot = lambda u, v: (u * v).sum(-1)   # noqa: E731

    def seg(P, Q):
        d = Q - P
        t = np.clip(dot(q - P, d) / dot(d, d), 0, 1)[..., None]
        e = q - (P + t * d)
        return dot(e, e)
    best = np.minimum(np.minimum(seg(A, B), seg(B, Cc)), seg(Cc, A))
    u, w = B - A, Cc - A
    n = np.cross(u, w)
    nn = dot(n, n)
    p = q - A
    # barycentrics of the projection
    b1 = dot(np.cross(p, w), n) / nn
    b2 = dot(np.cross(u, p), n) / nn
    inside = (b1 >= 0) & (b2 >= 0) & (b1 + b2 <= 1)
    plane = dot(p, n) ** 2 / nn
    return np.where(inside, np.minimum(best, plane), best)


def smallest_angle_deg(A, B, Cc):
    A, B, Cc = (np.asarray(v, D) for v in (A, B, Cc))
    out = np.full(np.broadcast(A, B).shape[:-1], 180.0)
    for P, Q, R in ((A, B, Cc), (B, Cc, A), (Cc, A, B)):
        u, w = Q - P, R - P
        with np.errstate(invalid="ignore", divide="ignore"):   # a corner repeated: no angle, and the triangle does not qualify
            c = (u * w).sum(-1) / np.sqrt((u * u).sum(-1) * (w * w).sum(-1))
        out = np.minimum(out, np.nan_to_num(np.degrees(np.arccos(np.clip(c, -1, 1))), nan=0.0))
    return out


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------
HAND_TRI = np.array([[3, 4, 0], [0, 0, 0], [0, 4, 0]], F)   # A, B, C: the 3-4-5 triangle, the right angle at C
# one point in each of the seven regions, in rule order, with its squared distance in closed form
HAND_POINTS = np.array([[4, 5, 2], [-1, -1, 0], [5.5, -1, 0], [-1, 5, 0], [1.5, 6, 0], [-2, 2, 0], [1, 3, 2]], F)
HAND_D2 = np.array([6, 2, 25, 2, 4, 4, 4], F)


def hand_mesh():
    return mc._mesh(HAND_TRI, [[0, 1, 2]])


@functools.lru_cache(maxsize=None)
def sphere_shell(n=5000, seed=7):
    """the anchor sphere and n points in a shell around its surface, up to 0.6 from it"""
    m = mc.anchor()
    rng = np.random.default_rng(seed)
    centre, radius = np.array(mc.ANCHOR[1]), mc.ANCHOR[2]
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pts = centre + d * (radius + rng.uniform(-0.6, 0.6, (n, 1)))
    return m, pts.astype(F)


SPHERE_RADII = (0.05, 0.3, 1.0)   # the middle one leaves some of the shell without a candidate


@functools.lru_cache(maxsize=None)
def cube_voronoi(q=8):
    """the cube of mesh_simplify_common and points in the Voronoi regions of its faces, edges and vertices (outside), and inside"""
    m = msc.cube(q)
    rng = np.random.default_rng(11)
    pts = [rng.uniform(-0.4, 1.4, (1500, 3))]
    for off in (-0.25, 1.25):   # face, edge and vertex regions hit on purpose
        base = rng.uniform(0.05, 0.95, (300, 3))
        for k in (1, 2, 3):
            p = base.copy()
            p[:, :k] = off + rng.uniform(-0.1, 0.1, (300, k))
            pts.append(p)
    return m, np.concatenate(pts).astype(F)


def spanning_triangle(n=4000, seed=3):
    """one triangle over a whole cloud of points near its plane; with the radius 1/200 of its edge its cell range is large"""
    rng = np.random.default_rng(seed)
    tri_xyz = np.array([[-1, -1, 0.1], [9, -1, -0.1], [-1, 9, 0.05]], F)
    pts = np.concatenate([rng.uniform(0, 6, (n, 2)), rng.normal(0, 0.03, (n, 1))], 1).astype(F)
    return mc._mesh(tri_xyz, [[0, 1, 2]]), pts, 10.0 / 200


def far_outside(seed=5):
    """a mesh that reaches far outside the cloud's box on every side, with triangles wholly outside it too"""
    rng = np.random.default_rng(seed)
    v = np.concatenate([rng.uniform(-50, 50, (60, 3)), rng.uniform(-1, 1, (60, 3)), rng.uniform(200, 300, (6, 3))]).astype(F)
    t = np.concatenate([rng.integers(0, 120, (80, 3)), [[120, 121, 122], [123, 124, 125]]]).astype(np.int32)
    pts = rng.uniform(-1, 1, (2000, 3)).astype(F)
    return mc._mesh(v, t), pts, 0.5


# ---- the seeded sweep ----------------------------------------------------------------------------------------------------------------------
SWEEP_CASES = 24
SWEEP_SEED = 2026


@functools.lru_cache(maxsize=None)
def sweep_case(k):
    """(mesh dict, points float32 [n, 3], radius): random well-shaped triangles in a box with points around them; some cases add exact
    duplicates and reversed copies of triangles (ties), slivers, non-finite vertices and points, points on vertices and edges"""
    rng = np.random.default_rng([SWEEP_SEED, k])
    nt, npts = int(rng.integers(1, 60)), int(rng.integers(1, 400))
    size = float(2.0 ** rng.integers(-3, 4))
    centre = rng.uniform(-1, 1, (nt, 1, 3)) * size * 2
    # corners on a circle of a random plane, at least 25 degrees apart: well shaped
    ang = np.sort(rng.uniform(0, 2 * np.pi, (nt, 3)), 1)
    ang[:, 1] = np.maximum(ang[:, 1], ang[:, 0] + 0.45)
    ang[:, 2] = np.maximum(ang[:, 2], ang[:, 1] + 0.45)
    e1 = rng.normal(size=(nt, 3))
    e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
    e2 = np.cross(e1, rng.normal(size=(nt, 3)))
    e2 /= np.linalg.norm(e2, axis=1, keepdims=True)
    rad = rng.uniform(0.2, 1.0, (nt, 1, 1)) * size
    corners = centre + rad * (np.cos(ang)[..., None] * e1[:, None] + np.sin(ang)[..., None] * e2[:, None])
    xyz = corners.reshape(-1, 3).astype(F)
    tri = np.arange(3 * nt, dtype=np.int32).reshape(-1, 3)
    extra = []
    if k % 3 == 0:   # ties: the same triangle again, and reversed
        pick = rng.integers(0, nt, max(1, nt // 4))
        extra += [tri[pick], tri[pick][:, ::-1]]
    if k % 4 == 1:   # slivers and a point triangle: below the 1 degree mark, a minority
        extra.append(np.stack([tri[:2, 0], tri[:2, 0], tri[:2, 1]], 1))
        extra.append(np.stack([tri[:1, 0], tri[:1, 0], tri[:1, 0]], 1))
    if extra:
        tri = np.concatenate([tri] + extra).astype(np.int32)
    pts = (centre[rng.integers(0, nt, npts), 0] + rng.normal(0, 0.7, (npts, 3)) * size)
    on = rng.integers(0, npts, max(1, npts // 10))
    pts[on] = xyz[rng.integers(0, len(xyz), len(on))]   # exactly on vertices
    pts = pts.astype(F)
    if k % 5 == 2:
        xyz = xyz.copy()
        xyz[rng.integers(0, len(xyz)), rng.integers(0, 3)] = [np.nan, np.inf, -np.inf][k % 3]
        pts[rng.integers(0, npts), rng.integers(0, 3)] = np.nan
    order = rng.permutation(len(tri))
    radius = float(F(size * rng.choice([0.05, 0.3, 1.5])))
    return mc._mesh(xyz, tri[order]), pts, radius


@functools.lru_cache(maxsize=None)
def sweep_want(k):
    m, pts, radius = sweep_case(k)
    return distance_statement(m["xyz"], m["tri"], pts, radius, want_census=True)


def sweep_census():
    tot = {"regions": np.zeros(8, np.int64), "ties": 0, "pairs": 0, "nan_pairs": 0, "no_candidate": 0, "nonfinite_points": 0, "nonfinite_triangles": 0, "with_candidate": 0}
    for k in range(SWEEP_CASES):
        m, pts, _ = sweep_case(k)
        d2, arg, counts, c = sweep_want(k)
        for key in ("regions", "ties", "pairs", "nan_pairs"):
            tot[key] = tot[key] + c[key]
        tot["no_candidate"] += int(counts[1] - counts[0])
        tot["with_candidate"] += int(counts[0])
        tot["nonfinite_points"] += int(len(pts) - counts[1])
        tot["nonfinite_triangles"] += int((~np.isfinite(m["xyz"][m["tri"]]).all((1, 2))).sum())
    return tot
