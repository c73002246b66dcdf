"""The plain statements of mpmvs_tsdf_integrate and mpmvs_tsdf_mesh (include/mpmvs.h) in numpy fp32, shared by
test_tsdf_cpu.py, test_tsdf_gpu.py and tools/bench_tsdf.py.  numpy rounds every fp32 operation on its own (no contraction) and divides
correctly rounded, which is the arithmetic of the contract.  The orientation table is built here from the midpoint rule in floating
point, independently of the integer construction in csrc/pm_tsdf.hpp."""
import itertools

import numpy as np

F = np.float32
SLOTS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]   # (x, y, z) offsets of the edges a voxel owns
PERMS = list(itertools.permutations(range(3)))                                          # lexicographic: xyz xzy yxz yzx zxy zyx


def tet_vertices(t):
    """the four corners (x, y, z in 0 / 1) of tetrahedron t of a cell: v0 = 000, v1 = v0 + e_a, v2 = v1 + e_b, v3 = 111"""
    v, c = [(0, 0, 0)], [0, 0, 0]
    for a in PERMS[t]:
        c[a] = 1
        v.append(tuple(c))
    return v


def case_triangles(inside):
    """inside: four booleans in tetrahedron vertex order -> the triangles as lists of three (p, q) vertex pairs, before orientation"""
    ins = [p for p in range(4) if inside[p]]
    out = [p for p in range(4) if not inside[p]]
    if len(ins) == 1:
        return [[(ins[0], o) for o in out]]
    if len(ins) == 3:
        return [[(a, out[0]) for a in ins]]
    if len(ins) == 2:
        (a, b), (c, d) = ins, out
        return [[(a, c), (a, d), (b, d)], [(a, c), (b, d), (b, c)]]
    return []


def _flip_table():
    """[t][m] -> one boolean per triangle of case m (bit p of m: vertex p inside): swap its last two vertices.  The midpoint rule:
    (p1 - p0) x (p2 - p0) must point from the mean of the inside corners to the mean of the outside corners with every vertex at the
    midpoint of its edge."""
    table = []
    for t in range(6):
        V = np.array(tet_vertices(t), np.float64)
        row = []
        for m in range(16):
            inside = [bool((m >> p) & 1) for p in range(4)]
            flips = []
            for tri in case_triangles(inside):
                P = [0.5 * (V[p] + V[q]) for p, q in tri]
                direction = V[[p for p in range(4) if not inside[p]]].mean(0) - V[[p for p in range(4) if inside[p]]].mean(0)
                dot = float(np.dot(np.cross(P[1] - P[0], P[2] - P[0]), direction))
                assert abs(dot) > 1e-9, (t, m)
                flips.append(dot < 0)
            row.append(flips)
        table.append(row)
    return table


FLIP = _flip_table()


def cam_arrays(cam):
    return np.array(cam.K, F), np.array(cam.R, F), np.array(cam.t, F), int(cam.width), int(cam.height)


def positions(origin, voxel, dims):
    """P_a = (float)((double)origin[a] + (double)i * (double)voxel) per axis"""
    return [(np.float64(F(origin[a])) + np.arange(dims[a], dtype=np.float64) * np.float64(F(voxel))).astype(F) for a in range(3)]


def project(cam, Px, Py, Pz):
    """steps 1 and 3 of the statement for arrays of positions -> (z, fu, fv), fp32; fu and fv are meaningless where z <= 0"""
    K, R, t, _, _ = cam_arrays(cam)
    Px, Py, Pz = (np.asarray(v, F) for v in (Px, Py, Pz))
    with np.errstate(all="ignore"):
        xc = ((R[0] * Px + R[1] * Py) + R[2] * Pz) + t[0]
        yc = ((R[3] * Px + R[4] * Py) + R[5] * Pz) + t[1]
        z = ((R[6] * Px + R[7] * Py) + R[8] * Pz) + t[2]
        fu = ((K[0] * xc) / z + K[2]) + F(0.5)
        fv = ((K[4] * yc) / z + K[5]) + F(0.5)
    return z, fu, fv


def integrate_statement(origin, voxel, dims, trunc, cams, depths, colors=None, state=None):
    """the volume after the views in order, from `state` = (sum, weight, color4) or from zero -> (sum float32 [nz, ny, nx],
    weight int32 [nz, ny, nx], color4 uint32 [nz, ny, nx, 4] or None)"""
    nx, ny, nz = dims
    px, py, pz = positions(origin, voxel, dims)
    Pz, Py, Px = np.meshgrid(pz, py, px, indexing="ij")
    trunc = F(trunc)
    if state is None:
        total, weight = np.zeros((nz, ny, nx), F), np.zeros((nz, ny, nx), np.int32)
        color4 = np.zeros((nz, ny, nx, 4), np.uint32) if colors is not None else None
    else:
        total, weight, color4 = state[0].copy(), state[1].copy(), None if state[2] is None else state[2].copy()
    with np.errstate(all="ignore"):
        for v, cam in enumerate(cams):
            W, H = int(cam.width), int(cam.height)
            z, fu, fv = project(cam, Px, Py, Pz)
            ok = z > 0
            ok &= (fu >= 0) & (fu < F(W)) & (fv >= 0) & (fv < F(H))
            ix = np.where(ok, np.floor(fu), 0).astype(np.int64)
            iy = np.where(ok, np.floor(fv), 0).astype(np.int64)
            depth = np.ascontiguousarray(depths[v], F).reshape(H, W)
            d = depth[iy, ix]
            ok &= np.isfinite(d) & (d > 0)
            s = d - z
            ok &= ~(s < -trunc)
            total = np.where(ok, total + np.minimum(F(1.0), s / trunc), total).astype(F)
            weight = weight + ok.astype(np.int32)
            if colors is not None:
                paint = ok & (s <= trunc)
                img = np.asarray(colors[v], np.uint8)
                pix = img[iy, ix].astype(np.uint32)
                if img.ndim == 2:
                    pix = np.stack([pix, pix, pix], -1)
                color4[..., :3] += np.where(paint[..., None], pix, 0).astype(np.uint32)
                color4[..., 3] += paint.astype(np.uint32)
    return total, weight, color4


def mesh_statement(total, weight, color4, dims, origin, voxel, min_weight=1, details=False):
    """-> {"xyz": float32 [n, 3], "rgb": uint8 [n, 3] or None, "tri": int32 [m, 3]}; with `details` also what a census asks for:
    "keys" (owner linear index * 7 + slot per vertex), "val" (float32 [n, 3], the colour values in B, G, R order before the byte, or
    None), "tri_cell" and "tri_case" (per triangle the cell's linear index and tetrahedron * 16 + inside mask)"""
    nx, ny, nz = dims
    total, weight = np.asarray(total, F).reshape(nz, ny, nx), np.asarray(weight, np.int32).reshape(nz, ny, nx)
    valid = weight >= min_weight
    with np.errstate(all="ignore"):
        f = np.where(valid, total / np.where(valid, weight, 1).astype(F), F(0)).astype(F)
    inside = valid & (f < 0)
    tris, tri_cell, tri_case = [], [], []   # three (owner linear index * 7 + slot) keys each
    if nx > 1 and ny > 1 and nz > 1:
        some_in = np.zeros((nz - 1, ny - 1, nx - 1), bool)
        some_out = np.zeros_like(some_in)
        for dz, dy, dx in itertools.product((0, 1), repeat=3):
            blk = (slice(dz, nz - 1 + dz), slice(dy, ny - 1 + dy), slice(dx, nx - 1 + dx))
            some_in |= inside[blk]
            some_out |= valid[blk] & ~inside[blk]
        tets = [tet_vertices(t) for t in range(6)]
        for k, j, i in zip(*np.nonzero(some_in & some_out)):   # ascending cell linear index
            for t in range(6):
                c = [(i + d[0], j + d[1], k + d[2]) for d in tets[t]]
                if not all(valid[q[2], q[1], q[0]] for q in c):
                    continue
                ins = [bool(inside[q[2], q[1], q[0]]) for q in c]
                m = sum(1 << p for p in range(4) if ins[p])
                for r, tri in enumerate(case_triangles(ins)):
                    keys = []
                    for p, q in tri:   # always from the lower tetrahedron vertex A to the higher one B = A + off
                        A, B = c[min(p, q)], c[max(p, q)]
                        slot = SLOTS.index((B[0] - A[0], B[1] - A[1], B[2] - A[2]))
                        keys.append(((A[2] * ny + A[1]) * nx + A[0]) * 7 + slot)
                    if FLIP[t][m][r]:
                        keys = [keys[0], keys[2], keys[1]]
                    tris.append(keys)
                    tri_cell.append((k * ny + j) * nx + i)
                    tri_case.append(t * 16 + m)
    tri_keys = np.array(tris, np.int64).reshape(-1, 3)
    vert_keys = np.unique(tri_keys)   # owner ascending, then slot ascending
    tri = np.searchsorted(vert_keys, tri_keys).astype(np.int32)
    owner, slot = vert_keys // 7, vert_keys % 7
    off = np.array(SLOTS, np.int64)[slot]
    ia = np.stack([owner % nx, (owner // nx) % ny, owner // (nx * ny)], 1)
    ib = ia + off
    pos = positions(origin, voxel, dims)
    fa, fb = f[ia[:, 2], ia[:, 1], ia[:, 0]], f[ib[:, 2], ib[:, 1], ib[:, 0]]
    with np.errstate(all="ignore"):
        t = fa / (fa - fb)
        xyz = np.empty((len(owner), 3), F)
        for a in range(3):
            pa, pb = pos[a][ia[:, a]], pos[a][ib[:, a]]
            xyz[:, a] = pa + t * (pb - pa)
        rgb = vals = None
        if color4 is not None:
            color4 = np.asarray(color4, np.uint32).reshape(nz, ny, nx, 4)
            ca, cb = color4[ia[:, 2], ia[:, 1], ia[:, 0]], color4[ib[:, 2], ib[:, 1], ib[:, 0]]
            has_a, has_b = ca[:, 3] > 0, cb[:, 3] > 0
            rgb, vals = np.empty((len(owner), 3), np.uint8), np.empty((len(owner), 3), F)
            for c in range(3):   # sums are B, G, R; the bytes go out R, G, B
                ma = ca[:, c].astype(F) / np.where(has_a, ca[:, 3], 1).astype(F)
                mb = cb[:, c].astype(F) / np.where(has_b, cb[:, 3], 1).astype(F)
                val = np.where(has_a & has_b, ma + t * (mb - ma), np.where(has_a, ma, np.where(has_b, mb, F(128)))).astype(F)
                rgb[:, 2 - c], vals[:, c] = color_byte(val), val
    out = {"xyz": xyz, "rgb": rgb, "tri": tri}
    if details:
        out.update(keys=vert_keys, val=vals, tri_cell=np.array(tri_cell, np.int64), tri_case=np.array(tri_case, np.int64))
    return out


def color_byte(val):
    """the colour byte of the contract: with v = val + 0.5f, 255 where v >= 255, (int)v where v >= 0, else 0 (a NaN included)"""
    with np.errstate(all="ignore"):
        v = (np.asarray(val, F) + F(0.5)).astype(F)
        mid = v >= 0
        return np.where(v >= F(255), 255, np.where(mid, np.where(mid, v, F(0)).astype(np.int32), 0)).astype(np.uint8)


def same_bits(got, want):
    """the comparison rule of the TSDF sweeps (that of fusion_fuzz_common.same_bits): equal bits wherever `want` is not NaN, NaN
    wherever it is; the payload of a NaN is not part of the contract"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype != np.float32:
        return bool(np.array_equal(got, want))
    nan = np.isnan(want)
    return bool(np.isnan(got[nan]).all() and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))


def sphere_volume(dims, centre, radius):
    """sum = (float)(distance to `centre` - radius) in fp64, weight 1 everywhere: the anchor of the contract is
    sphere_volume((10, 9, 8), (4.3, 3.9, 3.4), 2.7)"""
    nx, ny, nz = dims
    k, j, i = np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    f = (np.sqrt((i - centre[0]) ** 2 + (j - centre[1]) ** 2 + (k - centre[2]) ** 2) - radius).astype(F)
    return f, np.ones((nz, ny, nx), np.int32)


def topology(tri):
    """-> dict: V, E, F, euler, every directed half-edge once ("no_repeat"), every half-edge has exactly one opposite ("closed"),
    every half-edge has at most one opposite and none repeats ("manifold_with_boundary")"""
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    a = np.concatenate([tri[:, 0], tri[:, 1], tri[:, 2]])
    b = np.concatenate([tri[:, 1], tri[:, 2], tri[:, 0]])
    n = int(tri.max()) + 1 if len(tri) else 0
    half = a * max(n, 1) + b
    opposite = b * max(n, 1) + a
    uniq, counts = np.unique(half, return_counts=True)
    no_repeat = bool((counts == 1).all()) and bool((a != b).all())
    has_opposite = np.isin(opposite, uniq)
    undirected = np.unique(np.minimum(a, b) * max(n, 1) + np.maximum(a, b))
    V, E, Fc = len(np.unique(tri)), len(undirected), len(tri)
    return {"V": V, "E": E, "F": Fc, "euler": V - E + Fc, "no_repeat": no_repeat, "closed": no_repeat and bool(has_opposite.all()),
            "manifold_with_boundary": no_repeat}


def signed_volume(xyz, tri):
    """positive when the triangles are counter-clockwise seen from outside"""
    p = np.asarray(xyz, np.float64)[np.asarray(tri, np.int64)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)
