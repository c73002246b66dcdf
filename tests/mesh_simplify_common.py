"""mpmvs_simplify_mesh: statement 4 of include/mpmvs.h in numpy -- voxel_common.statement for the clusters, normals_common.jacobi for
the sweeps, np.add.at on int64 for the sums, a dict for the triangle keys -- the scenes and the seeded sweep's generator, shared by
test_mesh_simplify_cpu.py and test_mesh_simplify_gpu.py.  Nothing here calls the library."""
import functools

import numpy as np

import mesh_clean_common as mc
import normals_common as nc
import voxel_common as vc

F = np.float32
D = np.float64
FIX = float(1 << 30)
_mesh = mc._mesh


def _grid_terms(xyz, cell):
    """(o float64 [3], e, t float64 [n, 3], c float64 [n, 3], fin bool [n]) of the voxel statement; rows of non-finite vertices are
    not to be read"""
    x = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    e = float(F(cell))
    fin = np.isfinite(x).all(1)
    o = x[fin].min(0).astype(D) - 0.5 * e
    with np.errstate(all="ignore"):
        t = (x.astype(D) - o) / e
        c = np.floor(t)
    return o, e, t, c, fin


def statement(m, cell, placement=1):
    """-> {"xyz", "rgb", "tri", "cluster_of", "count", "placed", "tri_src", "counts"} as Mesh.simplify, plus "T" (the planes per
    cluster, int64) for the tests that reason about them"""
    xyz = np.ascontiguousarray(m["xyz"], F).reshape(-1, 3)
    tri = np.asarray(m["tri"], np.int64).reshape(-1, 3)
    rgb = m.get("rgb")
    v = vc.statement(xyz, cell, colors=rgb)
    cluster_of = v["voxel_of"]
    k_n = len(v["count"])
    out = {"xyz": v["xyz"].copy(), "rgb": v["colors"] if rgb is not None else None, "cluster_of": cluster_of, "count": v["count"],
           "placed": np.zeros(k_n, np.uint8), "T": np.zeros(k_n, np.int64)}
    if placement == 1 and k_n and len(tri):
        _place(out, xyz, tri, cell, v)
    # C: the triangles
    cl = cluster_of.astype(np.int64)[tri] if len(tri) else np.zeros((0, 3), np.int64)
    non_finite = (cl < 0).any(1)
    collapsed = ~non_finite & ((cl[:, 0] == cl[:, 1]) | (cl[:, 1] == cl[:, 2]) | (cl[:, 0] == cl[:, 2]))
    alive = ~non_finite & ~collapsed
    seen, kept = {}, []
    for t in np.flatnonzero(alive).tolist():
        key = tuple(sorted(cl[t].tolist()))
        if key not in seen:
            seen[key] = t
            kept.append(t)
    kept = np.array(kept, np.int64).reshape(-1)
    out["tri"] = cl[kept].astype(np.int32).reshape(-1, 3)
    out["tri_src"] = kept.astype(np.int32)
    out["counts"] = {"non_finite": int(non_finite.sum()), "collapsed": int(collapsed.sum()), "duplicates": int(alive.sum()) - len(kept)}
    return out


def _place(out, xyz, tri, cell, v):
    """B: the quadrics and the representatives, written into out["xyz"], out["placed"], out["T"]"""
    o, e, t, c, fin = _grid_terms(xyz, cell)
    cluster_of = v["voxel_of"].astype(np.int64)
    k_n = len(v["count"])
    tf = tri[fin[tri].all(1)]
    P = xyz.astype(D)
    with np.errstate(all="ignore"):
        u, w = P[tf[:, 1]] - P[tf[:, 0]], P[tf[:, 2]] - P[tf[:, 0]]
        Cx, Cy, Cz = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
        L = np.sqrt((Cx * Cx + Cy * Cy) + Cz * Cz)
        good = (L > 0) & np.isfinite(L)
    tf, L = tf[good], L[good]
    nh = [Cx[good] / L, Cy[good] / L, Cz[good] / L]
    pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    Q, R, T = np.zeros((k_n, 6), np.int64), np.zeros((k_n, 3), np.int64), np.zeros(k_n, np.int64)
    qq = [np.rint((nh[i] * nh[j]) * FIX).astype(np.int64) for i, j in pairs]
    for corner in range(3):
        vert = tf[:, corner]
        k = cluster_of[vert]
        q = (t[vert] - c[vert]) - 0.5
        delta = (nh[0] * q[:, 0] + nh[1] * q[:, 1]) + nh[2] * q[:, 2]
        for p in range(6):
            np.add.at(Q[:, p], k, qq[p])
        for i in range(3):
            np.add.at(R[:, i], k, np.rint((nh[i] * delta) * FIX).astype(np.int64))
        np.add.at(T, k, 1)
    out["T"] = T
    # the position sums of the voxel statement, once more: it does not hand them out
    S = np.zeros((k_n, 3), np.int64)
    idx = np.flatnonzero(fin)
    np.add.at(S, cluster_of[idx], np.rint((t[idx] - c[idx]) * FIX).astype(np.int64))
    cnt = v["count"].astype(D)
    x0 = [S[:, a].astype(D) / (cnt * FIX) - 0.5 for a in range(3)]
    A = {pr: Q[:, p].astype(D) / FIX for p, pr in enumerate(pairs)}
    r = [R[:, i].astype(D) / FIX for i in range(3)]
    with np.errstate(all="ignore"):
        d, V, _ = nc.jacobi(A)
        lmax = d[0]
        lmax = np.where(d[1] > lmax, d[1], lmax)
        lmax = np.where(d[2] > lmax, d[2], lmax)

        def a(i, j):
            return A[(i, j) if i <= j else (j, i)]
        g = [r[i] - ((a(i, 0) * x0[0] + a(i, 1) * x0[1]) + a(i, 2) * x0[2]) for i in range(3)]
        y = [np.where(d[j] > 1e-3 * lmax, ((V[0][j] * g[0] + V[1][j] * g[1]) + V[2][j] * g[2]) / d[j], 0.0) for j in range(3)]
        x = [x0[i] + ((V[i][0] * y[0] + V[i][1] * y[1]) + V[i][2] * y[2]) for i in range(3)]
        inside = (np.abs(x[0]) <= 0.5) & (np.abs(x[1]) <= 0.5) & (np.abs(x[2]) <= 0.5)
        placed = np.where(T == 0, 0, np.where(~(lmax > 0), 2, np.where(inside, 1, 2))).astype(np.uint8)
        cv = c[v["first"]]
        pos = np.stack([(o[i] + (cv[:, i] + (0.5 + x[i])) * e) for i in range(3)], 1).astype(F)
    out["placed"] = placed
    out["xyz"][placed == 1] = pos[placed == 1]


KEYS = ("xyz", "rgb", "tri", "cluster_of", "count", "placed", "tri_src", "counts")


def assert_same(got, want, what=""):
    """every output of Mesh.simplify against the statement, by shape, dtype and bits"""
    for k in KEYS:
        g, w = got[k], want[k]
        if k == "counts":
            assert g == w, f"{what} counts: {g} against {w}"
            continue
        if w is None:
            assert g is None, f"{what} {k}: not None"
            continue
        assert g is not None and g.dtype == w.dtype and g.shape == w.shape, f"{what} {k}: {None if g is None else (g.dtype, g.shape)} against {w.dtype} {w.shape}"
        if np.ascontiguousarray(g).tobytes() != np.ascontiguousarray(w).tobytes():
            gb, wb = np.ascontiguousarray(g).view(np.uint8).reshape(len(g), -1), np.ascontiguousarray(w).view(np.uint8).reshape(len(w), -1)
            bad = np.flatnonzero((gb != wb).any(1))
            raise AssertionError(f"{what} {k}: {len(bad)} of {len(g)} rows differ in bits; first at {bad[0]}: {g[bad[0]]!r} against {w[bad[0]]!r}")


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
CUBE_CELLS = (0.25, 0.1, 0.07)
CUBE_CORNERS = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], D)


@functools.lru_cache(maxsize=None)
def cube(q=32):
    """the unit cube as six faces of q x q quads, each face with vertices of its own (6 (q + 1)^2 vertices, 12 q^2 triangles), wound
    counter-clockwise seen from outside; every coordinate is a multiple of 1 / q, exact in fp32"""
    s = np.arange(q + 1) / q
    b, a = np.meshgrid(s, s, indexing="ij")
    a, b = a.ravel(), b.ravel()
    i, j = np.meshgrid(np.arange(q), np.arange(q), indexing="ij")
    v = (i * (q + 1) + j).ravel()
    quad = np.concatenate([np.stack([v, v + 1, v + q + 2], 1), np.stack([v, v + q + 2, v + q + 1], 1)])   # counter-clockwise in (a, b)
    xyz, tri = [], []
    for axis in range(3):
        for side in (0, 1):
            p = np.empty((len(a), 3))
            p[:, axis] = side
            p[:, (axis + 1) % 3], p[:, (axis + 2) % 3] = a, b   # (a, b, axis) is right-handed: the normal is +axis
            xyz.append(p)
            tri.append((quad if side else quad[:, [0, 2, 1]]) + len(a) * len(tri))
    return _mesh(np.concatenate(xyz), np.concatenate(tri))


def plane(nx=23, ny=17, z=3.25):
    return mc.grid(nx, ny, z)


def tent(s, c):
    """the fallback case: A and B share the cell about (0, 0, 0) (cell = 1; the anchor vertex 0 puts the cell centres on the
    integers); the planes of the two triangles meet at x = 0, y = -0.4 s / c"""
    A, B = np.array([-0.4, 0, 0]), np.array([0.4, 0, 0])
    xyz = np.array([[-2, -2, -1], A, A + [0, 0, 1], A + 2 * np.array([c, -s, 0]), B, B - 2 * np.array([c, s, 0]), B + [0, 0, 1]])
    return _mesh(xyz, [[1, 2, 3], [4, 5, 6]])


def duplicates():
    """all six orders of the triple (0, 1, 2), then (1, 2, 3) twice, on four vertices far apart"""
    xyz = np.array([[0, 0, 0], [10, 0, 0], [0, 10, 0], [10, 10, 5]], F)
    tri = [[1, 2, 0], [0, 1, 2], [2, 0, 1], [0, 2, 1], [2, 1, 0], [1, 0, 2], [3, 2, 1], [1, 2, 3]]
    return _mesh(xyz, tri)


def degenerate():
    """a repeated index, a NaN vertex, and two good triangles that land on one key at cell 1 (vertices 0 and 5 share a cell)"""
    xyz = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [np.nan, 1, 1], [4, 4, 1], [0.25, 0.25, 0]], F)
    tri = [[0, 1, 2], [0, 0, 1], [1, 3, 2], [5, 2, 1], [1, 4, 2], [0, 5, 1], [3, 3, 3]]
    return _mesh(xyz, tri)


def strip_far(k):
    """k triangles in a strip whose vertices are a cell apart at cell 0.5: all survive"""
    return mc.strip(k, "scrambled")


def one_key(k, reverse=False):
    """k triangles over three clusters in all six orientations: three bundles of vertices, each inside one cell of edge 1 (the last
    vertex, which no triangle names, puts the cell centres on the integers)"""
    rng = np.random.default_rng(7)
    per = 50
    centre = np.array([[0, 0, 0], [5, 0, 0], [0, 5, 1]], D)
    xyz = np.concatenate([(centre[:, None, :] + rng.uniform(-0.3, 0.3, (3, per, 3))).reshape(-1, 3), [[-1, -1, -1]]])
    perms = np.array([[0, 1, 2], [1, 2, 0], [2, 0, 1], [0, 2, 1], [2, 1, 0], [1, 0, 2]])
    which = perms[np.arange(k) % 6]
    tri = which * per + rng.integers(0, per, (k, 3))
    return _mesh(xyz, tri[::-1] if reverse else tri)


def fan_hub(k):
    """k triangles about one hub whose rim vertices lie in other cells at cell 0.5: k quadric terms for the hub's cluster"""
    return mc.fan(k)


def random_keys(k=4096, clusters=64, seed=9):
    """k random triples over `clusters` vertices a cell apart: many duplicates and long runs of taken slots"""
    rng = np.random.default_rng(seed)
    g = np.arange(clusters)
    xyz = np.stack([g % 8, g // 8, 0.25 * (g % 3)], 1) * 2.0
    return _mesh(xyz, rng.integers(0, clusters, (k, 3)))


def scaled(m, p):
    """the mesh with every coordinate times 2^p, exactly"""
    x = (m["xyz"].astype(D) * 2.0 ** p).astype(F)
    assert np.array_equal(x.astype(D), m["xyz"].astype(D) * 2.0 ** p)
    return _mesh(x, m["tri"], m["rgb"])


# ---- the seeded sweep ----------------------------------------------------------------------------------------------------------------
SWEEP_CASES = 40
SWEEP_SEED = 2025


@functools.lru_cache(maxsize=None)
def sweep_case(k):
    """random index mesh k: n in 1..3000, m in 0..4n, every triangle's indices inside a random window, the vertices uniform in a box
    (every fourth mesh flat along one axis; some with non-finite vertices, some coloured), the cell 0.05, 0.1, 0.2 or 0.5 of the box
    -> {"mesh", "cell"}"""
    rng = np.random.default_rng([SWEEP_SEED, k])
    n = int(rng.integers(1, 3001)) if k % 8 else int(rng.integers(1, 40))
    m = int(rng.integers(0, 4 * n + 1))
    width = max(1, min(n, int(rng.integers(3, max(4, n // 2 + 1)))))
    start = rng.integers(0, n - width + 1, m)
    tri = start[:, None] + rng.integers(0, width, (m, 3))
    box = float(rng.choice([1e-2, 1.0, 50.0]))
    # the index is a walk through the box, so that a window of indices is a neighbourhood in space as on a real mesh
    step = rng.normal(0.0, box * float(rng.choice([0.01, 0.05, 0.3])), (n, 3))
    pos = np.cumsum(step, 0)
    pos = (pos - pos.min(0)) / max(float((pos.max(0) - pos.min(0)).max()), 1e-30) * box + rng.uniform(-box, box, 3)
    if k % 4 == 1:
        pos[:, int(rng.integers(0, 3))] = float(rng.uniform(-box, box))   # flat: every plane is the same, one eigenvalue
    xyz = pos.astype(F)
    if rng.random() < 0.1 or k % 10 == 3:
        xyz[rng.random(n) < 0.1, int(rng.integers(0, 3))] = np.nan
    rgb = rng.integers(0, 256, (n, 3)) if rng.random() < 0.5 else None
    cell = float(F(float(rng.choice([0.05, 0.1, 0.2, 0.5])) * box))
    return {"mesh": _mesh(xyz, tri, rgb), "cell": cell}


@functools.lru_cache(maxsize=None)
def sweep_want(k, placement):
    c = sweep_case(k)
    return statement(c["mesh"], c["cell"], placement)


def sweep_census():
    """what the CPU test asserts, on the statement alone: in how many cases each thing occurs, and the cluster totals"""
    out = {"placed0": 0, "placed1": 0, "placed2": 0, "duplicates": 0, "collapsed": 0, "non_finite": 0, "coloured": 0,
           "clusters0": 0, "clusters1": 0, "clusters2": 0}
    for k in range(SWEEP_CASES):
        w = sweep_want(k, 1)
        for p in range(3):
            out[f"placed{p}"] += bool((w["placed"] == p).any())
            out[f"clusters{p}"] += int((w["placed"] == p).sum())
        out["duplicates"] += w["counts"]["duplicates"] > 0
        out["collapsed"] += w["counts"]["collapsed"] > 0
        out["non_finite"] += w["counts"]["non_finite"] > 0
        out["coloured"] += w["rgb"] is not None
    return {k: int(v) for k, v in out.items()}
