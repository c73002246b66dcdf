"""The brick-sparse TSDF volume's statements in numpy (include/mpmvs.h, statements A and B), shared by
test_tsdf_sparse_cpu.py, test_tsdf_sparse_gpu.py and tools/bench_tsdf.py: statement A (which bricks mpmvs_tsdf_allocate marks) in fp32
as numpy rounds it, the mask that statement B puts on the dense arrays of tsdf_common.py, and the renumbering of mesh_statement's
output into brick-major order.  The renumbering finds every vertex's owner and every triangle's cell on its own, from the volume:
mesh_statement does not return them."""
import numpy as np

import tsdf_common as tc

F = np.float32
D = np.float64
# a sphere (dims, centre, radius for tsdf_common.sphere_volume) across the corner where eight bricks of a 3 x 3 x 2 grid meet; the
# anchor of the dense contract has every owner in one brick
SHIFTED = ((17, 17, 9), (8.2, 7.9, 4.1), 3.7)


def brick_grid(dims):
    """(bx, by, bz)"""
    return tuple((int(n) + 7) // 8 for n in dims)


def n_samples(trunc, voxel):
    return max(1, int(np.ceil(4.0 * float(F(trunc)) / float(F(voxel)))))


def allocate_statement(origin, voxel, dims, trunc, pad, cams, depths, bricks=None):
    """statement A -> bool [bz, by, bx]: the bricks allocated after the views, from `bricks` or from none"""
    bx, by, bz = brick_grid(dims)
    out = np.zeros((bz, by, bx), bool) if bricks is None else np.array(bricks, bool).reshape(bz, by, bx).copy()
    n_s = n_samples(trunc, voxel)
    step = (2.0 * D(F(trunc))) / D(n_s)
    o, vox, pad = [F(v) for v in origin], F(voxel), F(pad)
    with np.errstate(all="ignore"):
        for cam, depth in zip(cams, depths):
            K, R, t, W, H = tc.cam_arrays(cam)
            d = np.ascontiguousarray(depth, F).reshape(H, W)
            iy, ix = np.nonzero(np.isfinite(d) & (d > 0))
            d = d[iy, ix]
            fx, fy = ix.astype(F) - K[2], iy.astype(F) - K[5]
            for m in range(n_s + 1):
                z = ((d.astype(D) - D(F(trunc))) + D(m) * step).astype(F)                      # 1
                xc, yc = (fx * z) / K[0], (fy * z) / K[4]                                        # 2
                a, b, c = xc - t[0], yc - t[1], z - t[2]                                         # 3
                P = [(R[0] * a + R[3] * b) + R[6] * c, (R[1] * a + R[4] * b) + R[7] * c, (R[2] * a + R[5] * b) + R[8] * c]
                g = [(P[q] - o[q]) / vox for q in range(3)]                                      # 4
                ok = (z > 0) & np.isfinite(g[0]) & np.isfinite(g[1]) & np.isfinite(g[2])
                lo, hi = [], []
                for q in range(3):                                                               # 5
                    l, h = np.floor(g[q] - pad).astype(D), np.floor(g[q] + pad).astype(D)        # integers: exact in fp64
                    ok &= ~((h < 0) | (l > dims[q] - 1))
                    lo.append(np.clip(np.where(ok, l, 0), 0, dims[q] - 1).astype(np.int64) >> 3)
                    hi.append(np.clip(np.where(ok, h, 0), 0, dims[q] - 1).astype(np.int64) >> 3)
                lo, hi = [v[ok] for v in lo], [v[ok] for v in hi]
                if not len(lo[0]):
                    continue
                span = [int((hi[q] - lo[q]).max()) for q in range(3)]
                for dz in range(span[2] + 1):
                    for dy in range(span[1] + 1):
                        for dx in range(span[0] + 1):
                            I, J, Kb = lo[0] + dx, lo[1] + dy, lo[2] + dz
                            sel = (I <= hi[0]) & (J <= hi[1]) & (Kb <= hi[2])
                            out[Kb[sel], J[sel], I[sel]] = True
    return out


def brick_coords(bricks):
    """bool [bz, by, bx] -> int32 [n, 3] (I, J, K) in ascending linear index"""
    K, J, I = np.nonzero(bricks)
    return np.stack([I, J, K], 1).astype(np.int32)


def bricks_from_coords(dims, coords):
    bx, by, bz = brick_grid(dims)
    out = np.zeros((bz, by, bx), bool)
    c = np.asarray(coords, np.int64).reshape(-1, 3)
    out[c[:, 2], c[:, 1], c[:, 0]] = True
    return out


def voxel_exists(dims, bricks):
    """bool [nz, ny, nx]: the voxel's brick is allocated"""
    nx, ny, nz = dims
    return np.repeat(np.repeat(np.repeat(np.asarray(bricks, bool), 8, 0), 8, 1), 8, 2)[:nz, :ny, :nx]


def mask_dense(dims, bricks, total, weight, color4=None):
    """statement B: the dense arrays with every non-existing voxel zeroed"""
    nx, ny, nz = dims
    ex = voxel_exists(dims, bricks)
    total = np.where(ex, np.asarray(total, F).reshape(nz, ny, nx), F(0)).astype(F)
    weight = np.where(ex, np.asarray(weight, np.int32).reshape(nz, ny, nx), 0).astype(np.int32)
    if color4 is not None:
        color4 = np.where(ex[..., None], np.asarray(color4, np.uint32).reshape(nz, ny, nx, 4), 0).astype(np.uint32)
    return total, weight, color4


def to_bricks(dims, bricks, arr):
    """dense [nz, ny, nx(, 4)] -> [n, 8, 8, 8(, 4)] in brick-major order, cut-off voxels 0: what get_bricks returns"""
    nx, ny, nz = dims
    bx, by, bz = brick_grid(dims)
    arr = np.asarray(arr)
    pad = [(0, 8 * bz - nz), (0, 8 * by - ny), (0, 8 * bx - nx)] + [(0, 0)] * (arr.ndim - 3)
    big = np.pad(arr, pad)
    coords = brick_coords(bricks)
    out = np.zeros((len(coords), 8, 8, 8) + arr.shape[3:], arr.dtype)
    for r, (I, J, K) in enumerate(coords):
        out[r] = big[8 * K:8 * K + 8, 8 * J:8 * J + 8, 8 * I:8 * I + 8]
    return out


def brick_major_index(dims, bricks, linear):
    """dense linear voxel indices -> rank * 512 + local index, -1 where the voxel does not exist"""
    nx, ny, nz = dims
    bricks = np.asarray(bricks, bool)
    rank = np.where(bricks, np.cumsum(bricks.reshape(-1)).reshape(bricks.shape) - 1, -1)
    linear = np.asarray(linear, np.int64)
    i, j, k = linear % nx, (linear // nx) % ny, linear // (nx * ny)
    r = rank[k >> 3, j >> 3, i >> 3]
    return np.where(r >= 0, r * 512 + (((k & 7) * 8 + (j & 7)) * 8 + (i & 7)), -1)


def mesh_structure(total, weight, dims, min_weight=1):
    """-> (vertex keys owner * 7 + slot, ascending; the cell linear index of every triangle, in mesh_statement's order), found
    from the volume with array operations: the edges that emitting tetrahedra cross and the triangles each cell emits"""
    nx, ny, nz = dims
    total, weight = np.asarray(total, F).reshape(nz, ny, nx), np.asarray(weight, np.int32).reshape(nz, ny, nx)
    if min(nx, ny, nz) < 2:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    valid = weight >= min_weight
    with np.errstate(all="ignore"):
        inside = valid & ((total / np.where(valid, weight, 1).astype(F)) < 0)

    def at(a, c):
        return a[c[2]:nz - 1 + c[2], c[1]:ny - 1 + c[1], c[0]:nx - 1 + c[0]]

    counts = np.zeros((nz - 1, ny - 1, nx - 1), np.int64)
    keys = []
    for t in range(6):
        tv = tc.tet_vertices(t)
        ins = [at(inside, c) for c in tv]
        ni = sum(x.astype(np.int64) for x in ins)
        emit = at(valid, tv[0]) & at(valid, tv[1]) & at(valid, tv[2]) & at(valid, tv[3]) & (ni > 0) & (ni < 4)
        counts += np.where(emit, np.where(ni == 2, 2, 1), 0)
        for p in range(3):
            for q in range(p + 1, 4):
                kk, jj, ii = np.nonzero(emit & (ins[p] ^ ins[q]))
                A, B = tv[p], tv[q]
                slot = tc.SLOTS.index((B[0] - A[0], B[1] - A[1], B[2] - A[2]))
                keys.append((((kk + A[2]) * ny + jj + A[1]) * nx + ii + A[0]) * 7 + slot)
    kk, jj, ii = np.meshgrid(np.arange(nz - 1), np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
    cell = ((kk * ny + jj) * nx + ii).reshape(-1)
    return np.unique(np.concatenate(keys)).astype(np.int64), np.repeat(cell, counts.reshape(-1))


def renumber_brick_major(mesh, total, weight, dims, bricks, min_weight=1):
    """mesh_statement's output for (total, weight) -- already masked by `bricks` -- with vertices ordered by (brick-major index of the
    owner, slot) and triangles by (brick-major index of the cell, tetrahedron, triangle)"""
    vert_keys, tri_cell = mesh_structure(total, weight, dims, min_weight)
    assert len(vert_keys) == len(mesh["xyz"]) and len(tri_cell) == len(mesh["tri"])
    owner = brick_major_index(dims, bricks, vert_keys // 7)
    cell = brick_major_index(dims, bricks, tri_cell)
    assert (owner >= 0).all() and (cell >= 0).all()   # an owner and the corner 000 of an emitting cell are valid, so they exist
    perm = np.argsort(owner * 7 + vert_keys % 7, kind="stable")
    inv = np.empty(len(perm), np.int64)
    inv[perm] = np.arange(len(perm))
    order = np.argsort(cell, kind="stable")
    tri = inv[np.asarray(mesh["tri"], np.int64)][order].astype(np.int32).reshape(-1, 3)
    return {"xyz": mesh["xyz"][perm], "rgb": None if mesh["rgb"] is None else mesh["rgb"][perm], "tri": tri}


def sparse_mesh_statement(total, weight, color4, dims, origin, voxel, bricks, min_weight=1):
    """statement B for the mesh: the dense statement on the masked volume, renumbered"""
    total, weight, color4 = mask_dense(dims, bricks, total, weight, color4)
    m = tc.mesh_statement(total, weight, color4, dims, origin, voxel, min_weight)
    return renumber_brick_major(m, total, weight, dims, bricks, min_weight)


def band_voxels(origin, voxel, dims, trunc, cams, depths):
    """bool [nz, ny, nx]: the voxel has a contribution with |s| <= trunc from some view, by the steps of integrate_statement"""
    px, py, pz = tc.positions(origin, voxel, dims)
    Pz, Py, Px = np.meshgrid(pz, py, px, indexing="ij")
    band = np.zeros(Px.shape, bool)
    with np.errstate(all="ignore"):
        for cam, depth in zip(cams, depths):
            W, H = int(cam.width), int(cam.height)
            z, fu, fv = tc.project(cam, Px, Py, Pz)
            ok = (z > 0) & (fu >= 0) & (fu < F(W)) & (fv >= 0) & (fv < F(H))
            ix, iy = np.where(ok, np.floor(fu), 0).astype(np.int64), np.where(ok, np.floor(fv), 0).astype(np.int64)
            d = np.ascontiguousarray(depth, F).reshape(H, W)[iy, ix]
            ok &= np.isfinite(d) & (d > 0)
            band |= ok & (np.abs(d - z) <= F(trunc))
    return band


def triangle_set(mesh):
    """the triangles as a set of 36-byte position triples, each rotated to start at its smallest vertex: comparable between meshes
    whose vertices are numbered differently"""
    p = np.ascontiguousarray(mesh["xyz"], F)[np.asarray(mesh["tri"], np.int64).reshape(-1, 3)].view(np.uint32).reshape(-1, 3, 3)
    out = set()
    for t in p:
        rows = [r.tobytes() for r in t]
        s = rows.index(min(rows))
        out.add(rows[s] + rows[(s + 1) % 3] + rows[(s + 2) % 3])
    return out


def sphere_scene(pm):
    """the end-to-end scene of test_tsdf_gpu.py: a sphere seen by four cameras into 24^3 voxels (3^3 bricks) -> (dims, origin, voxel,
    trunc, cams, depths, colours)"""
    from test_tsdf_gpu import _sphere_depth
    dims, origin, voxel, trunc = (24, 24, 24), (-0.6, -0.6, 1.4), 0.05, 0.15
    centre, radius = np.array([0.0, 0.0, 2.0]), 0.4
    cams, depths, cols = [], [], []
    for q, (cx, cy) in enumerate(((-0.9, 0.0), (0.9, 0.1), (0.0, -0.9), (0.1, 0.9))):
        C = np.array([cx, cy, 0.2])
        zax = (centre - C) / np.linalg.norm(centre - C)
        xax = np.cross([0.0, 1.0, 0.0] if abs(zax[1]) < 0.5 else [1.0, 0.0, 0.0], zax)
        xax /= np.linalg.norm(xax)
        R = np.stack([xax, np.cross(zax, xax), zax])
        K = np.array([[70.0, 0, 39.5], [0, 70.0, 29.5], [0, 0, 1]])
        cam = pm.make_camera(K, R, -R @ C, 60, 80, 0.5, 20.0)
        cams.append(cam)
        depths.append(_sphere_depth(cam, centre, radius, background=0.0))
        cols.append(np.full(depths[-1].shape + (3,), (40 * q, 255 - 60 * q, 90), np.uint8))
    return dims, origin, voxel, trunc, cams, depths, cols
