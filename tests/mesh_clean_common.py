"""mpmvs_mesh_*: the three statements of include/mpmvs.h in numpy (a plain union-find, np.add.at on int64, fp64 as the header
writes it), the keep rule of remove_small_components, the scene builders and the seeded sweep's generator, shared by
test_mesh_clean_cpu.py and test_mesh_clean_gpu.py.  Nothing here calls the library."""
import functools
import math

import numpy as np

import tsdf_common as tc
import tsdf_sparse_common as sc

F = np.float32
D = np.float64


def _mesh(xyz, tri, rgb=None):
    m = {"xyz": np.ascontiguousarray(xyz, F).reshape(-1, 3), "tri": np.ascontiguousarray(tri, np.int32).reshape(-1, 3),
         "rgb": None if rgb is None else np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)}
    for v in m.values():
        if v is not None:
            v.setflags(write=False)
    return m


# ---- statement 1 -------------------------------------------------------------------------------------------------------------------
def components_statement(n, tri):
    """-> (label int32 [n], verts int32 [n], tris int32 [n], counts [4]): a plain sequential union-find over the triangles"""
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    parent = list(range(n))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    for a, b, c in tri.tolist():
        for other in (b, c):
            ra, rb = find(a), find(other)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)   # the smaller index stays the root: the root is the smallest of its class
    label = np.array([find(v) for v in range(n)], np.int64).reshape(n)
    verts_of = np.bincount(label, minlength=n)
    tris_of = np.bincount(label[tri[:, 0]], minlength=n) if len(tri) else np.zeros(n, np.int64)
    verts, tris = verts_of[label], tris_of[label]
    named = np.zeros(n, bool)
    named[tri.reshape(-1)] = True
    roots = np.flatnonzero(tris_of > 0)
    if len(roots):
        best = int(roots[np.argmax(tris_of[roots])])   # argmax: the first of equals, and the roots ascend
        counts = [len(roots), int((~named).sum()), int(tris_of[best]), best]
    else:
        counts = [0, n, 0, -1]
    return label.astype(np.int32), verts.astype(np.int32), tris.astype(np.int32), counts


# ---- statement 2 -------------------------------------------------------------------------------------------------------------------
def normal_scale(xyz, m):
    """-> (scale, e, b, ext); scale = 0.0 where every normal is zero"""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    fin = np.isfinite(xyz).all(1)
    if not fin.any() or m == 0:
        return 0.0, None, None, 0.0
    P = xyz[fin].astype(D)
    ext = float((P.max(0) - P.min(0)).max())
    if ext == 0.0:
        return 0.0, None, None, 0.0
    B = 2.0 * (ext * ext)
    _, e = math.frexp(B)
    b = 0
    while (1 << b) < max(m, 1):
        b += 1
    return math.ldexp(1.0, 61 - b - e), e, b, ext


def normals_statement(xyz, tri, sums=False):
    """-> (float32 [n, 3], n_defined); with `sums` also the int64 sums S"""
    xyz, tri = np.asarray(xyz, F).reshape(-1, 3), np.asarray(tri, np.int64).reshape(-1, 3)
    n = len(xyz)
    scale = normal_scale(xyz, len(tri))[0]
    S = np.zeros((n, 3), np.int64)
    if scale != 0.0:
        fin = np.isfinite(xyz).all(1)
        t = tri[fin[tri].all(1)]
        P = xyz.astype(D)
        with np.errstate(all="ignore"):
            u, w = P[t[:, 1]] - P[t[:, 0]], P[t[:, 2]] - P[t[:, 0]]
            C = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
            Fk = np.rint(C * scale).astype(np.int64)   # rint: to nearest even
        assert (np.abs(Fk) < (1 << 61)).all()
        for k in range(3):
            np.add.at(S, t[:, k], Fk)
    x = S.astype(D)
    length = np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2])
    defined = length > 0
    out = np.zeros((n, 3), F)
    out[defined] = (x[defined] / length[defined, None]).astype(F)
    return (out, int(defined.sum()), S) if sums else (out, int(defined.sum()))


# ---- statement 3 -------------------------------------------------------------------------------------------------------------------
def select_statement(m, keep, drop_unreferenced=True):
    """-> {"xyz", "rgb", "tri", "src"}"""
    xyz, tri, rgb = m["xyz"], np.asarray(m["tri"], np.int64).reshape(-1, 3), m.get("rgb")
    keep = np.asarray(keep).reshape(-1) != 0
    tkeep = keep[tri].all(1) if len(tri) else np.zeros(0, bool)
    vkeep = keep.copy()
    if drop_unreferenced:
        named = np.zeros(len(xyz), bool)
        named[tri[tkeep].reshape(-1)] = True
        vkeep &= named
    new = np.cumsum(vkeep) - 1
    return {"xyz": xyz[vkeep], "rgb": None if rgb is None else rgb[vkeep], "tri": new[tri[tkeep]].astype(np.int32).reshape(-1, 3),
            "src": np.flatnonzero(vkeep).astype(np.int32)}


def keep_statement(label, tris, min_triangles=1, largest=None):
    """the components with at least min_triangles (and at least one) triangles; with largest=K the K largest of them by triangle
    count, ties to the smaller label; written with a sort over tuples, not as mesh.rank_components does it"""
    roots = [(-int(tris[v]), v) for v in range(len(label)) if label[v] == v and tris[v] >= max(min_triangles, 1)]
    if largest is not None:
        roots = sorted(roots)[:largest]
    good = {v for _, v in roots}
    return np.array([int(l) in good for l in label], bool).reshape(len(label))


def clean_statement(m, min_triangles=1, largest=None):
    label, _, tris, counts = components_statement(len(m["xyz"]), m["tri"])
    keep = keep_statement(label, tris, min_triangles, largest)
    out = select_statement(m, keep, True)
    out.update(keep=keep, label=label, tris=tris, counts=counts)
    return out


def same_mesh(got, want):
    if (got["rgb"] is None) != (want["rgb"] is None):
        return False
    return bool(got["xyz"].shape == want["xyz"].shape and np.array_equal(got["xyz"].view(np.uint32), np.ascontiguousarray(want["xyz"]).view(np.uint32))
                and np.array_equal(got["tri"], want["tri"]) and got["tri"].dtype == np.int32 and np.array_equal(got["src"], want["src"])
                and (want["rgb"] is None or np.array_equal(got["rgb"], want["rgb"])))


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
ANCHOR = ((10, 9, 8), (4.3, 3.9, 3.4), 2.7)


@functools.lru_cache(maxsize=None)
def anchor():
    """the anchor of the TSDF contract: 410 vertices, 816 triangles, one closed sphere"""
    f, w = tc.sphere_volume(*ANCHOR)
    m = tc.mesh_statement(f, w, None, ANCHOR[0], (0, 0, 0), 1.0)
    return _mesh(m["xyz"], m["tri"])


@functools.lru_cache(maxsize=None)
def two_spheres():
    fa, _ = tc.sphere_volume((12, 7, 7), (3.2, 3, 3), 2.1)
    fb, w = tc.sphere_volume((12, 7, 7), (7.9, 3, 3), 2.1)
    m = tc.mesh_statement(np.minimum(fa, fb), w, None, (12, 7, 7), (0, 0, 0), 1.0)
    return _mesh(m["xyz"], m["tri"])


@functools.lru_cache(maxsize=None)
def open_sphere():
    """the 17 x 17 x 9 sphere with one brick removed: a mesh with a boundary"""
    dims, centre, radius = sc.SHIFTED
    f, w = tc.sphere_volume(dims, centre, radius)
    part = np.ones((2, 3, 3), bool)
    part[0, 1, 1] = False
    m = sc.sparse_mesh_statement(f, w, None, dims, (0, 0, 0), 1.0, part)
    return _mesh(m["xyz"], m["tri"])


def strip(k, numbering, seed=5):
    """k triangles in a zig-zag strip over k + 2 vertices, the vertices numbered ascending, descending or scrambled along it"""
    n = k + 2
    pos = np.stack([np.arange(n) // 2, np.arange(n) % 2, 0.01 * np.arange(n)], 1).astype(F)
    tri = np.stack([np.arange(k), np.arange(k) + 1, np.arange(k) + 2], 1)
    tri[1::2] = tri[1::2][:, [1, 0, 2]]   # a consistent winding
    perm = {"ascending": np.arange(n), "descending": np.arange(n)[::-1], "scrambled": np.random.default_rng(seed).permutation(n)}[numbering]
    xyz = np.empty_like(pos)
    xyz[perm] = pos
    return _mesh(xyz, perm[tri])


def fan(k, hub_first=True):
    """k triangles around one vertex: contention on one root and, for the normals, on one address"""
    ang = np.arange(k + 1) * (2.0 * np.pi / (k + 1))
    rim = np.stack([np.cos(ang), np.sin(ang), 0.05 * np.sin(7 * ang)], 1)
    xyz = np.concatenate([[[0.0, 0.0, 0.3]], rim]) if hub_first else np.concatenate([rim, [[0.0, 0.0, 0.3]]])
    hub, first = (0, 1) if hub_first else (k + 1, 0)
    tri = np.stack([np.full(k, hub), first + np.arange(k), first + np.arange(k) + 1], 1)
    return _mesh(xyz, tri)


TET = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]])   # counter-clockwise seen from outside for the corners below
TET_XYZ = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], D)


def tetrahedra(count, unnamed=0, seed=11, color=False):
    """`count` closed tetrahedra at random places with `unnamed` vertices no triangle names mixed in, under a random permutation of
    the vertex numbers"""
    rng = np.random.default_rng(seed)
    pos = (TET_XYZ[None] * rng.uniform(0.2, 1.0, (count, 1, 1)) + rng.uniform(-20, 20, (count, 1, 3))).reshape(-1, 3)
    tri = (TET[None] + 4 * np.arange(count)[:, None, None]).reshape(-1, 3)
    pos = np.concatenate([pos, rng.uniform(-20, 20, (unnamed, 3))])
    n = len(pos)
    perm = rng.permutation(n)
    xyz = np.empty((n, 3), F)
    xyz[perm] = pos
    tri = perm[tri][rng.permutation(len(tri))]
    return _mesh(xyz, tri, rng.integers(0, 256, (n, 3)) if color else None)


def repeated():
    """triangles that name a vertex twice or three times among ordinary ones; vertex 9 is named only by (9, 9, 9), 10 by nothing"""
    xyz = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5], [3, 0, 0], [4, 0, 0], [3, 1, 0], [6, 6, 6], [7, 6, 6], [9, 9, 9], [5, 5, 5]], F)
    tri = np.array([[0, 1, 2], [1, 3, 2], [2, 2, 4], [5, 6, 5], [7, 8, 8], [9, 9, 9], [4, 5, 6]])
    return _mesh(xyz, tri)


def grid(nx, ny, z=0.0):
    """a planar nx x ny grid of vertices, two counter-clockwise (seen from +z) triangles per cell"""
    j, i = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    xyz = np.stack([i.ravel(), j.ravel(), np.full(nx * ny, z)], 1)
    v = (j[:-1, :-1] * nx + i[:-1, :-1]).ravel()
    tri = np.concatenate([np.stack([v, v + 1, v + nx + 1], 1), np.stack([v, v + nx + 1, v + nx], 1)])
    return _mesh(xyz, tri)


def plant_nonfinite(m, share=0.05, seed=3):
    rng = np.random.default_rng(seed)
    xyz = m["xyz"].copy()
    bad = rng.random(len(xyz)) < share
    bad[0] = True
    xyz[bad, rng.integers(0, 3, int(bad.sum()))] = rng.choice([np.nan, np.inf, -np.inf], int(bad.sum()))
    return _mesh(xyz, m["tri"], m["rgb"])


def join(*meshes):
    """the meshes side by side in one index space"""
    off = np.cumsum([0] + [len(m["xyz"]) for m in meshes])
    rgb = None if any(m["rgb"] is None for m in meshes) else np.concatenate([m["rgb"] for m in meshes])
    return _mesh(np.concatenate([m["xyz"] for m in meshes]), np.concatenate([m["tri"] + o for m, o in zip(meshes, off)]), rgb)


@functools.lru_cache(maxsize=None)
def named_meshes():
    out = {"anchor": anchor(), "two_spheres": two_spheres(), "open_sphere": open_sphere(), "fan8193": fan(8193), "fan8193_hub_last": fan(8193, False),
           "tetrahedra": tetrahedra(300, 50, color=True), "repeated": repeated()}
    for numbering in ("ascending", "descending", "scrambled"):
        out["strip4096_" + numbering] = strip(4096, numbering)
    for m in (255, 256, 257):
        out[f"strip{m}"] = strip(m, "scrambled", seed=m)
    return out


@functools.lru_cache(maxsize=None)
def want(name):
    """the statements of a named mesh, computed once: {"label", "verts", "tris", "counts", "normals", "n_defined"}"""
    m = named_meshes()[name]
    label, verts, tris, counts = components_statement(len(m["xyz"]), m["tri"])
    normals, nd = normals_statement(m["xyz"], m["tri"])
    out = {"label": label, "verts": verts, "tris": tris, "counts": counts, "normals": normals, "n_defined": nd}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ---- the seeded sweep ----------------------------------------------------------------------------------------------------------------
SWEEP_CASES = 40
SWEEP_SEED = 2024


@functools.lru_cache(maxsize=None)
def sweep_case(k):
    """random index mesh k: n in 1..3000, m in 0..4n, every triangle's indices drawn inside a random window of random width (narrow
    windows give hundreds of components, wide ones a single one); every tenth-ish mesh has repeated indices, non-finite vertices;
    colours or none; a random keep mask -> {"mesh", "keep", "drop"}"""
    rng = np.random.default_rng([SWEEP_SEED, k])
    n = int(rng.integers(1, 3001)) if k % 8 else int(rng.integers(1, 40))
    kind = k % 4   # 0: wide windows and many triangles, 1: narrow windows, 2: mixed widths, 3: few triangles
    m = int(rng.integers(0, 4 * n + 1))
    if kind == 0:
        m = max(m, 3 * n)
    if kind == 3:
        m = m // 8
    width = {0: n, 1: int(rng.integers(3, 8)), 2: int(rng.integers(3, max(4, n // 4 + 1))), 3: n}[kind]
    width = max(1, min(width, n))
    start = rng.integers(0, n - width + 1, m)
    if kind == 1:
        start = start // width * width   # disjoint windows: one component per window at most
    tri = start[:, None] + rng.integers(0, width, (m, 3))
    if rng.random() < 0.1 or k % 10 == 7:
        rep = rng.random(m) < 0.3
        tri[rep, 2] = tri[rep, int(rng.integers(0, 2))]
    xyz = rng.normal(0.0, float(rng.choice([1e-3, 1.0, 1e4])), (n, 3)).astype(F)
    if k % 5 == 2:
        xyz[:, 2] = 0.0        # planar: coincident and collinear triangles cancel or vanish
        xyz[:, :2] = np.round(xyz[:, :2] / np.abs(xyz[:, :2]).max() * 2)
    if rng.random() < 0.1 or k % 10 == 3:
        bad = rng.random(n) < 0.1
        xyz[bad, 0] = np.nan
    rgb = rng.integers(0, 256, (n, 3)) if rng.random() < 0.5 else None
    keep = (rng.random(n) < rng.choice([0.2, 0.6, 0.95])).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8)
    return {"mesh": _mesh(xyz, tri, rgb), "keep": keep}


@functools.lru_cache(maxsize=None)
def sweep_want(k):
    c = sweep_case(k)
    m = c["mesh"]
    label, verts, tris, counts = components_statement(len(m["xyz"]), m["tri"])
    normals, nd = normals_statement(m["xyz"], m["tri"])
    return {"label": label, "verts": verts, "tris": tris, "counts": counts, "normals": normals, "n_defined": nd,
            "select": [select_statement(m, c["keep"], d) for d in (False, True)]}


def sweep_census():
    """what the CPU test asserts, on the statement alone"""
    out = {"one_component": 0, "over_100_components": 0, "unnamed_vertices": 0, "zero_normal_on_named": 0, "drop_changes": 0, "repeated": 0, "non_finite": 0,
           "coloured": 0, "empty": 0}
    for k in range(SWEEP_CASES):
        m, w = sweep_case(k)["mesh"], sweep_want(k)
        named = np.zeros(len(m["xyz"]), bool)
        named[m["tri"].reshape(-1)] = True
        out["one_component"] += w["counts"][0] == 1 and w["counts"][1] == 0
        out["over_100_components"] += w["counts"][0] > 100
        out["unnamed_vertices"] += w["counts"][1] > 0
        out["zero_normal_on_named"] += bool((named & ~w["normals"].any(1)).any())
        out["drop_changes"] += len(w["select"][0]["xyz"]) != len(w["select"][1]["xyz"])
        t = m["tri"]
        out["repeated"] += bool(len(t) and ((t[:, 0] == t[:, 1]) | (t[:, 1] == t[:, 2]) | (t[:, 0] == t[:, 2])).any())
        out["non_finite"] += bool(not np.isfinite(m["xyz"]).all())
        out["coloured"] += m["rgb"] is not None
        out["empty"] += len(t) == 0
    return {k: int(v) for k, v in out.items()}
