"""Seeded random inputs of the TSDF family -- the dense volume, the brick-sparse volume and their marching tetrahedra (include/mpmvs.h,
DESIGN.md sections 22 and 23) -- shared by tests/test_tsdf_fuzz_cpu.py (what the sweeps cover, on the numpy statements alone) and
tests/test_tsdf_fuzz_gpu.py (the sweeps on the MI355X).  Every case is a pure function of k: default_rng((seed, k)).

Sweep A, integrate_case(pm, k): a lattice shaped to the 64 x 4 tile (even k) or to the 8^3 brick (odd k), 1..19 views (8, 9, 16 and 17
forced in every third case) of 8..39 pixels per side scattered around and inside the volume, each looking at a point of it, depth maps
of a plane or a sphere through the volume with noise and planted patches of bad values, colour none / B,G,R / grey, the view list cut
into 1..3 calls, and a brick set that is allocated from a subset of the views, a random mask, or everything.
Sweep B, mesh_case(k): volumes for set / set_bricks -- a random field with weights in -2..3, planted special sums, colour sums with
counts 0..3 and some means above 255, a brick mask.
Sweep C, life_case(pm, k): 6..12 operations (and up to two refused allocates more) on one sparse handle, with the numpy model that says what the handle must hold after each.
Named cases: the cull bound and the chunk boundaries.

box_live_many is tsdf_box_live of csrc/pm_tsdf.hpp restated in numpy fp32.  It serves the census (which boxes the cases cull, and how
nearly) and a soundness check on the CPU; the device is judged by the bits of the volume alone."""
import numpy as np

import tsdf_common as tc
import tsdf_sparse_common as sc

F = np.float32
SEED_A, SEED_B, SEED_C = 22001, 22002, 22003
DEFAULT_CASES = {"A": 60, "B": 60, "C": 30}      # what the sweeps run unless MPMVS_TSDF_FUZZ_CASES scales them; the census is over these
TILE_X, TILE_Y, CHUNK = 64, 4, 8                 # kTsdfTileX, kTsdfTileY, kTsdfChunk of csrc/pm_tsdf.hpp
CULL_BOUND = F(2.0 ** 40)                        # kTsdfCullBound
BAD_DEPTHS = {"zero": 0.0, "negative": -1.0, "nan": np.nan, "+inf": np.inf, "denormal": 1e-40}
PADS = (0.0, 0.5, 1.0, 8.0)
# planted in the sums of sweep B: exact zeros of both signs, denormals (1e-42 / 3 stays a denormal: inside iff negative, which a flushed
# quotient would lose; the smallest denormal / 3 rounds to a zero: outside whatever its sign), infinities and NaN
SPECIAL_SUMS = {"+0": 0.0, "-0": -0.0, "+1e-42": 1e-42, "-1e-42": -1e-42, "+1e-45": 1e-45, "-1e-45": -1e-45, "+inf": np.inf, "-inf": -np.inf,
                "nan": np.nan}
_cache = {}


def n_cases(sweep, scale=None):
    """the default count of a sweep, or with MPMVS_TSDF_FUZZ_CASES = N that count times N / 60"""
    base = DEFAULT_CASES[sweep]
    return base if scale is None else max(1, (base * int(scale)) // 60)


class Case:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _freeze(arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)


# ---- the block test in numpy --------------------------------------------------------------------------------------------------------
def cull_allowed(cam, pos):
    """W.cull as TsdfChunk::upload sets it: every camera entry the test reads and every |P| of the lattice at most 2^40 (false for a NaN)"""
    K, R, t, _, _ = tc.cam_arrays(cam)
    pmax = max(max(abs(F(p[0])), abs(F(p[-1]))) for p in pos)
    with np.errstate(all="ignore"):
        return bool(pmax <= CULL_BOUND) and bool(all(abs(x) <= CULL_BOUND for x in list(R) + list(t) + [K[0], K[2], K[4], K[5]]))


def _axis_dead(k0, k2, c0, c1, z0, z1, size):
    a0, a1 = k0 * c0, k0 * c1
    q0 = a0 / z0
    q1 = q0
    for q in (a0 / z1, a1 / z0, a1 / z1):
        q0, q1 = np.where(q < q0, q, q0), np.where(q > q1, q, q1)
    f0, f1 = (q0 + k2) + F(0.5), (q1 + k2) + F(0.5)
    return (f1 < 0) | (f0 >= F(size))


def box_live_many(cam, pos, boxes):
    """boxes: int [n, 6] = (i0, i1, j0, j1, k0, k1), inclusive -> an array of "behind" | "image" | "live".  Every operation is an fp32
    numpy operation rounded on its own: the corner positions, the ranges of xc, yc and z over the (4 or) 8 corners -- a box of one layer
    names each corner twice, which leaves the ranges as they are --, z1 <= 0, !(z0 > 0), then per axis the four quotients."""
    K, R, t, W, H = tc.cam_arrays(cam)
    boxes = np.asarray(boxes, np.int64).reshape(-1, 6)
    out = np.full(len(boxes), "live", object)
    if not cull_allowed(cam, pos) or not len(boxes):
        return out
    lo = hi = None
    with np.errstate(all="ignore"):
        for corner in range(8):
            px, py, pz = pos[0][boxes[:, corner & 1]], pos[1][boxes[:, 2 + ((corner >> 1) & 1)]], pos[2][boxes[:, 4 + (corner >> 2)]]
            c = np.stack([((R[3 * r] * px + R[3 * r + 1] * py) + R[3 * r + 2] * pz) + t[r] for r in range(3)])
            lo, hi = (c, c) if lo is None else (np.where(c < lo, c, lo), np.where(c > hi, c, hi))
        behind = hi[2] <= 0
        unsure = ~(lo[2] > 0)
        dead = _axis_dead(K[0], K[2], lo[0], hi[0], lo[2], hi[2], W) | _axis_dead(K[4], K[5], lo[1], hi[1], lo[2], hi[2], H)
    out[~behind & ~unsure & dead] = "image"
    out[behind] = "behind"
    return out


def box_live_statement(cam, pos, box):
    return str(box_live_many(cam, pos, [box])[0])


def tile_boxes(dims):
    """the 64 x 4 x 1 tiles of k_tsdf_integrate, cut to the lattice"""
    nx, ny, nz = dims
    return np.array([(i0, min(i0 + TILE_X, nx) - 1, j0, min(j0 + TILE_Y, ny) - 1, k, k)
                     for k in range(nz) for j0 in range(0, ny, TILE_Y) for i0 in range(0, nx, TILE_X)], np.int64)


def brick_boxes(dims):
    """the boxes of all bricks of the grid, ascending by linear index, cut to the lattice"""
    nx, ny, nz = dims
    return np.array([(i0, min(i0 + 8, nx) - 1, j0, min(j0 + 8, ny) - 1, k0, min(k0 + 8, nz) - 1)
                     for k0 in range(0, nz, 8) for j0 in range(0, ny, 8) for i0 in range(0, nx, 8)], np.int64)


def in_image(cam, pos):
    """bool [nz, ny, nx]: the voxel passes steps 2 and 4 of the statement"""
    Pz, Py, Px = np.meshgrid(pos[2], pos[1], pos[0], indexing="ij")
    z, fu, fv = tc.project(cam, Px, Py, Pz)
    with np.errstate(all="ignore"):
        return (z > 0) & (fu >= 0) & (fu < F(cam.width)) & (fv >= 0) & (fv < F(cam.height))


def count_in_boxes(mask, boxes):
    return np.array([int(mask[b[4]:b[5] + 1, b[2]:b[3] + 1, b[0]:b[1] + 1].sum()) for b in boxes], np.int64)


# ---- scenes -------------------------------------------------------------------------------------------------------------------------
def _patch(rng, h, w):
    """a random rectangle of about a quarter of each side, at least one pixel"""
    ph, pw = max(1, h // 4), max(1, w // 4)
    y, x = int(rng.integers(0, h - ph + 1)), int(rng.integers(0, w - pw + 1))
    return slice(y, y + ph), slice(x, x + pw)


def _camera(pm, rng, C, T, w, h, f):
    """a camera of w x h pixels at C whose axis passes through T, rolled at random"""
    zax = T - C
    if np.linalg.norm(zax) < 1e-6:
        zax = np.array([0.0, 0.0, 1.0])
    zax = zax / np.linalg.norm(zax)
    while True:
        xax = np.cross(rng.standard_normal(3), zax)
        if np.linalg.norm(xax) > 1e-3:
            break
    xax /= np.linalg.norm(xax)
    R = np.stack([xax, np.cross(zax, xax), zax])
    K = np.array([[f, 0, 0.5 * (w - 1) + rng.uniform(-2, 2)], [0, f * rng.uniform(0.9, 1.1), 0.5 * (h - 1) + rng.uniform(-2, 2)], [0, 0, 1]])
    return pm.make_camera(K, R, -R @ C, h, w, 0.05, 50.0)


def _depth_map(rng, cam, centre, extent, voxel, kind):
    """depth along the camera's z axis per pixel centre of a random plane, or of a sphere in front of that plane, through the volume;
    fp64 -> fp32, with noise of a third of a voxel; 0 where the ray misses or the depth is not in (0, 1000)"""
    from test_tsdf_gpu import _sphere_depth
    K, R, t = np.array(cam.K, np.float64).reshape(3, 3), np.array(cam.R, np.float64).reshape(3, 3), np.array(cam.t, np.float64)
    W, H = int(cam.width), int(cam.height)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ray = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], -1)
    Q = centre + rng.uniform(-0.3, 0.3, 3) * extent
    n = R @ rng.standard_normal(3)
    with np.errstate(all="ignore"):
        d = (n @ (R @ Q + t)) / (ray @ n)
        d = np.where(np.isfinite(d) & (d > 0) & (d < 1e3), d, 0.0)
        if kind == "sphere":
            s = _sphere_depth(cam, Q, float(rng.uniform(0.15, 0.4)) * float(extent.max()), background=0.0).astype(np.float64)
            d = np.where(s > 0, s, d)
        d = np.where(d > 0, d + rng.standard_normal(d.shape) * voxel / 3.0, 0.0)
    return d.astype(F)


def _scene(pm, rng, dims, n_views, inside_every=4):
    """origin, voxel, trunc and n_views cameras with depth maps and B,G,R images.  Centres are scattered around the volume's centre at
    0.6 of its largest extent, so some sit inside it; every `inside_every`-th is put inside the volume on purpose (boxes behind it)"""
    voxel = float(F(rng.uniform(0.02, 0.06)))
    origin = tuple(float(F(x)) for x in rng.uniform(-1.0, 1.0, 3))
    trunc = float(F(voxel * rng.uniform(1.5, 4.0)))
    extent = voxel * (np.array(dims, np.float64) - 1)
    centre = np.array(origin, np.float64) + 0.5 * extent
    cams, depths, cols, bad = [], [], [], []
    for q in range(n_views):
        w, h = int(rng.integers(8, 40)), int(rng.integers(8, 40))
        if inside_every and q % inside_every == inside_every - 1:
            C = centre + rng.uniform(-0.45, 0.45, 3) * extent
        else:
            C = centre + rng.standard_normal(3) * 0.6 * extent.max()
        T = centre + rng.uniform(-0.5, 0.5, 3) * extent
        cam = _camera(pm, rng, C, T, w, h, float(rng.uniform(10.0, 80.0)))
        d = _depth_map(rng, cam, centre, extent, voxel, "sphere" if rng.random() < 0.5 else "plane")
        names = rng.choice(list(BAD_DEPTHS), 2, replace=False)
        for name in names:
            d[_patch(rng, h, w)] = F(BAD_DEPTHS[name])
        cams.append(cam)
        depths.append(d)
        cols.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        bad.append(tuple(name for name in BAD_DEPTHS if (np.isnan(d).any() if name == "nan" else (d == F(BAD_DEPTHS[name])).any())))
    _freeze(depths + cols)
    return origin, voxel, trunc, cams, depths, cols, bad


def _random_bricks(rng, dims, share):
    bx, by, bz = sc.brick_grid(dims)
    return rng.random((bz, by, bx)) < share


def all_bricks(dims):
    bx, by, bz = sc.brick_grid(dims)
    return np.ones((bz, by, bx), bool)


# ---- sweep A ------------------------------------------------------------------------------------------------------------------------
FORCED_VIEWS = (8, 9, 16, 17)     # one chunk exactly, one more, two chunks exactly, one more


def integrate_case(pm, k):
    """-> Case: dims, origin, voxel, trunc, cams, depths, images (None, B,G,R or grey), bad (the planted kinds per view), calls (the
    slices of the view list, one per integrate call), brick_mode ("allocate" | "mask" | "all"), pad, alloc_views, bricks (bool grid)"""
    if ("A", k) in _cache:
        return _cache["A", k]
    rng = np.random.default_rng((SEED_A, k))
    if k % 2 == 0:
        dims = (int(rng.integers(65, 201)), int(rng.integers(5, 14)), int(rng.integers(2, 7)))
    else:
        dims = (int(rng.integers(9, 42)), int(rng.integers(9, 27)), int(rng.integers(2, 20)))
    n = FORCED_VIEWS[(k // 3) % 4] if k % 3 == 0 else int(rng.integers(1, 20))
    origin, voxel, trunc, cams, depths, cols, bad = _scene(pm, rng, dims, n)
    color = ("none", "bgr", "grey")[k % 3]
    images = None if color == "none" else cols if color == "bgr" else [np.ascontiguousarray(c[..., 1]) for c in cols]
    n_calls = min(n, 1 + (k // 6) % 3)
    cuts = sorted(int(c) for c in rng.choice(np.arange(1, n), n_calls - 1, replace=False)) if n_calls > 1 else []
    calls = [slice(a, b) for a, b in zip([0] + cuts, cuts + [n])]
    brick_mode = ("allocate", "mask", "all")[(k // 18 + k) % 3]
    pad, alloc_views = float(rng.choice(PADS)), []
    if brick_mode == "allocate":
        alloc_views = sorted(int(v) for v in rng.choice(n, max(1, n // 2), replace=False))
        bricks = sc.allocate_statement(origin, voxel, dims, trunc, pad, [cams[v] for v in alloc_views], [depths[v] for v in alloc_views])
    elif brick_mode == "mask":
        bricks = _random_bricks(rng, dims, 0.6)
    else:
        bricks = all_bricks(dims)
    c = Case(k=k, dims=dims, origin=origin, voxel=voxel, trunc=trunc, cams=cams, depths=depths, images=images, color=color, bad=bad, calls=calls,
             brick_mode=brick_mode, pad=pad, alloc_views=alloc_views, bricks=bricks)
    _cache["A", k] = c
    return c


def integrate_want(c):
    """the dense statement of case c, computed once"""
    if ("A want", c.k) not in _cache:
        _cache["A want", c.k] = tc.integrate_statement(c.origin, c.voxel, c.dims, c.trunc, c.cams, c.depths, c.images)
    return _cache["A want", c.k]


# ---- sweep B ------------------------------------------------------------------------------------------------------------------------
BIG_DIMS = {29: (130, 129, 4), 59: (70, 41, 25)}     # above 65536 entries: more than 256 scan tiles, and more than 128 bricks


def brick_arrays(dims, bricks, total, weight, color4, garbage=True):
    """what set_bricks takes: (coords, sum, weight, color4 or None) in brick-major order; with `garbage` the entries of voxels that dims
    cut off hold values that would change the mesh if they were used"""
    masked = sc.mask_dense(dims, bricks, total, weight, color4)
    s, w = sc.to_bricks(dims, bricks, masked[0]), sc.to_bricks(dims, bricks, masked[1])
    c = None if color4 is None else sc.to_bricks(dims, bricks, masked[2])
    if garbage:
        cut = ~sc.to_bricks(dims, bricks, np.ones(tuple(dims)[::-1], bool))
        s, w = np.where(cut, F(-1.5), s).astype(F), np.where(cut, 5, w).astype(np.int32)
        if c is not None:
            c = np.where(cut[..., None], 9, c).astype(np.uint32)
    return sc.brick_coords(bricks), s, w, c


def _field(rng, shape):
    """a random field that is no sphere: a few waves of random direction plus white noise of random strength"""
    nz, ny, nx = shape
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    f = np.zeros(shape)
    for _ in range(3):
        q = rng.uniform(-1.2, 1.2, 3)
        f += np.sin(q[0] * i + q[1] * j + q[2] * k + rng.uniform(0, 6.3))
    return f / 3.0 + rng.uniform(0.05, 1.0) * rng.standard_normal(shape)


def _volume_content(rng, shape, min_weight, with_color, plant=0.04):
    """sum, weight, color4 of a random volume: weights -2..3 with most voxels valid for `min_weight`, special sums planted under weight
    `min_weight` and under weight 3, colour counts 0..3 and some colour means far above 255"""
    nz, ny, nx = shape
    f = _field(rng, shape)
    p_valid = float(rng.uniform(0.75, 0.97))
    weight = np.where(rng.random(shape) < p_valid, rng.integers(min_weight, 4, shape), rng.integers(-2, min_weight, shape)).astype(np.int32)
    total = (f * np.maximum(weight, 1)).astype(F)
    names = list(SPECIAL_SUMS)
    at = rng.random(shape) < plant
    pick = rng.integers(0, len(names), shape)
    for q, name in enumerate(names):
        total[at & (pick == q)] = F(SPECIAL_SUMS[name])
    weight[at] = np.where(rng.random(shape) < 0.5, min_weight, 3)[at]
    color4 = None
    if with_color:
        cnt = rng.integers(0, 4, shape).astype(np.uint32)
        color4 = np.empty(shape + (4,), np.uint32)
        for c in range(3):
            mean = np.where(rng.random(shape) < 0.1, rng.integers(256, 100000, shape), rng.integers(0, 256, shape))
            color4[..., c] = mean.astype(np.uint32) * cnt
        color4[..., 3] = cnt
    return total, weight, color4


def mesh_case(k):
    """-> Case: dims, origin, voxel, total, weight, color4 (or None), min_weight, bricks, brick_mode ("all" | "none" | "mask")"""
    if ("B", k) in _cache:
        return _cache["B", k]
    rng = np.random.default_rng((SEED_B, k))
    min_weight = 1 + k % 3
    with_color = (k // 3) % 2 == 0
    big = BIG_DIMS.get(k % 60)
    corner = k % 4 == 1      # more than one brick along every axis: cells whose corners lie in eight bricks
    dims = big or ((int(rng.integers(9, 20)), int(rng.integers(9, 18)), int(rng.integers(9, 11))) if corner else
                   (int(rng.integers(2, 20)), int(rng.integers(2, 18)), int(rng.integers(2, 11))))
    nx, ny, nz = dims
    if big:      # random content in two slabs, at the first and at the last entries; nothing valid between them
        total, weight = np.zeros((nz, ny, nx), F), np.zeros((nz, ny, nx), np.int32)
        color4 = np.zeros((nz, ny, nx, 4), np.uint32) if with_color else None
        for slab in ((slice(0, min(nz, 4)), slice(0, 12), slice(0, 18)), (slice(max(0, nz - 4), nz), slice(ny - 11, ny), slice(nx - 19, nx))):
            shape = tuple(len(range(*s.indices(n))) for s, n in zip(slab, (nz, ny, nx)))
            s, w, c = _volume_content(rng, shape, min_weight, with_color)
            total[slab], weight[slab] = s, w
            if with_color:
                color4[slab] = c
    else:
        total, weight, color4 = _volume_content(rng, (nz, ny, nx), min_weight, with_color)
    brick_mode = ("all" if k % 60 == 29 else "mask") if big else "none" if k % 20 == 19 else "all" if k % 5 == 0 or k % 8 == 1 else "mask"
    bricks = all_bricks(dims) if brick_mode == "all" else ~all_bricks(dims) if brick_mode == "none" else _random_bricks(rng, dims, 0.7)
    origin, voxel = tuple(float(F(x)) for x in rng.uniform(-2.0, 2.0, 3)), float(F(rng.uniform(0.02, 0.5)))
    _freeze([total, weight, color4, bricks])
    c = Case(k=k, dims=dims, origin=origin, voxel=voxel, total=total, weight=weight, color4=color4, min_weight=min_weight, bricks=bricks,
             brick_mode=brick_mode, big=bool(big))
    _cache["B", k] = c
    return c


def mesh_want(c):
    """(the dense statement with details, the sparse statement) of case c, computed once"""
    if ("B want", c.k) not in _cache:
        dense = tc.mesh_statement(c.total, c.weight, c.color4, c.dims, c.origin, c.voxel, c.min_weight, details=True)
        sparse = sc.sparse_mesh_statement(c.total, c.weight, c.color4, c.dims, c.origin, c.voxel, c.bricks, c.min_weight)
        _cache["B want", c.k] = (dense, sparse)
    return _cache["B want", c.k]


def tet_cases(valid, inside):
    """bool [nz, ny, nx] each -> per tetrahedron t (all four corners valid [cells], the inside mask m [cells])"""
    nz, ny, nx = valid.shape
    at = lambda a, c: a[c[2]:nz - 1 + c[2], c[1]:ny - 1 + c[1], c[0]:nx - 1 + c[0]]
    out = []
    for t in range(6):
        tv = tc.tet_vertices(t)
        allv = at(valid, tv[0]) & at(valid, tv[1]) & at(valid, tv[2]) & at(valid, tv[3])
        m = sum(at(inside, tv[p]).astype(np.int64) << p for p in range(4))
        out.append((allv, m))
    return out


def corner_values(total, weight, min_weight):
    """(valid, f, inside) of the mesh statement"""
    valid = np.asarray(weight) >= min_weight
    with np.errstate(all="ignore"):
        f = np.where(valid, np.asarray(total, F) / np.where(valid, weight, 1).astype(F), F(0)).astype(F)
    return valid, f, valid & (f < 0)


# ---- sweep C ------------------------------------------------------------------------------------------------------------------------
OPS = ("allocate", "integrate", "set_bricks", "mesh", "read", "refused")


class Model:
    """what a sparse handle must hold: `bricks` (bool grid) and the masked dense arrays"""

    def __init__(self, c):
        self.c = c
        nx, ny, nz = c.dims
        self.bricks = ~all_bricks(c.dims)
        self.total, self.weight = np.zeros((nz, ny, nx), F), np.zeros((nz, ny, nx), np.int32)
        self.color4 = np.zeros((nz, ny, nx, 4), np.uint32) if c.with_color else None

    def views(self, ids):
        c = self.c
        return [c.cams[v] for v in ids], [c.depths[v] for v in ids], [c.cols[v] for v in ids] if c.with_color else None

    def after_allocate(self, ids):
        c = self.c
        cams, depths, _ = self.views(ids)
        return sc.allocate_statement(c.origin, c.voxel, c.dims, c.trunc, c.pad, cams, depths, bricks=self.bricks)

    def apply(self, op):
        """changes the state as the handle's call does; a mesh returns its statement"""
        c, kind = self.c, op[0]
        if kind == "allocate":
            self.bricks = self.after_allocate(op[1])     # existing bricks keep their contents, new ones are zero: the arrays stay
        elif kind == "integrate":
            cams, depths, cols = self.views(op[1])
            state = (self.total, self.weight, self.color4)
            self.total, self.weight, self.color4 = sc.mask_dense(c.dims, self.bricks, *tc.integrate_statement(c.origin, c.voxel, c.dims, c.trunc, cams, depths,
                                                                                                              cols, state=state))
        elif kind == "set_bricks":
            _, bricks, total, weight, color4 = op
            self.bricks = bricks.copy()
            self.total, self.weight, self.color4 = sc.mask_dense(c.dims, bricks, total, weight, color4)
            if c.with_color and color4 is None:
                self.color4 = np.zeros(self.total.shape + (4,), np.uint32)
        elif kind == "mesh":
            return sc.sparse_mesh_statement(self.total, self.weight, self.color4, c.dims, c.origin, c.voxel, self.bricks, op[1])
        return None

    def n_bricks(self):
        return int(self.bricks.sum())


def _moves(old, new):
    """an allocate from `old` to `new` moves an old brick: a new brick has a lower linear index than an old one"""
    o, n = np.flatnonzero(old.reshape(-1)), np.flatnonzero((new & ~old).reshape(-1))
    return bool(len(o) and len(n) and n.min() < o.max())


def life_case(pm, k):
    """-> Case: the scene (dims, origin, voxel, trunc, pad, cams, depths, cols, with_color), max_bricks and ops, a list of
    ("allocate", views) | ("integrate", views) | ("set_bricks", bricks, sum, weight, color4) | ("mesh", min_weight) | ("read",) |
    ("refused", views): an allocate that needs more than max_bricks.  Brick sets only are simulated here (the contents are the model's
    business); moves, refusals and zero_start are what the census counts."""
    if ("C", k) in _cache:
        return _cache["C", k]
    rng = np.random.default_rng((SEED_C, k))
    dims = (int(rng.integers(9, 34)), int(rng.integers(9, 27)), int(rng.integers(2, 18)))
    n_views = int(rng.integers(5, 11))
    origin, voxel, trunc, cams, depths, cols, _ = _scene(pm, rng, dims, n_views)
    c = Case(k=k, dims=dims, origin=origin, voxel=voxel, trunc=trunc, cams=cams, depths=depths, cols=cols, with_color=k % 2 == 1,
             pad=float(rng.choice(PADS[:3])))
    grid = all_bricks(dims)
    subset = lambda lo: sorted(int(v) for v in rng.choice(n_views, int(rng.integers(lo, max(lo + 1, n_views // 2 + 1))), replace=False))
    model = Model(c)           # its brick set is all that is used here
    zero_start = k % 5 == 0
    n_ops = int(rng.integers(6, 13))
    plan = ["integrate"] if zero_start else ["allocate"]
    plan += [str(x) for x in rng.choice(["allocate", "integrate", "set_bricks", "mesh", "read"], n_ops - 1, p=[0.3, 0.22, 0.16, 0.16, 0.16])]
    if zero_start:
        plan[1] = "allocate"
    capped = k % 6 != 5        # five lives in six have a cap below the whole grid
    cap_at = int(rng.integers(1 if zero_start else 0, n_ops // 2)) if capped else None
    max_bricks, ops, moves, refusals, peak, forced = int(grid.sum()), [], 0, 0, 0, 0
    for step, kind in enumerate(plan):
        if kind == "allocate":
            ids = subset(1)
            new = model.after_allocate(ids)
            if int(new.sum()) > max_bricks:
                ops.append(("refused", ids))
                refusals += 1
            else:
                moves += _moves(model.bricks, new)
                model.bricks = new
                ops.append(("allocate", ids))
        elif kind == "set_bricks":
            if rng.random() < 0.5 and model.bricks.any():      # the upper half of the present set: the next allocate moves bricks
                lin = np.flatnonzero(model.bricks.reshape(-1))
                bricks = np.zeros(grid.size, bool)
                bricks[lin[len(lin) // 2:]] = True
                bricks = bricks.reshape(grid.shape)
            else:
                bricks = _random_bricks(rng, dims, float(rng.uniform(0.0, 0.7)))
            lin = np.flatnonzero(bricks.reshape(-1))
            if len(lin) > max_bricks:                           # set_bricks is refused above max_bricks too: stay below
                drop = rng.choice(lin, len(lin) - max_bricks, replace=False)
                bricks.reshape(-1)[drop] = False
            nx, ny, nz = dims
            total, weight, color4 = _volume_content(rng, (nz, ny, nx), 1, c.with_color and rng.random() < 0.7, plant=0.01)
            _freeze([bricks, total, weight, color4])
            model.bricks = bricks.copy()
            ops.append(("set_bricks", bricks, total, weight, color4))
        elif kind == "integrate":
            ops.append(("integrate", subset(1)))
        elif kind == "mesh":
            ops.append(("mesh", int(rng.integers(1, 4))))
        else:
            ops.append(("read",))
        peak = max(peak, int(model.bricks.sum()))
        if capped and step == cap_at:
            # max_bricks = the largest count so far, reached at some step up to here (the handle has it from its creation); an allocate of
            # every view then asks for more wherever the views reach bricks that the set does not have
            max_bricks = max(1, peak)
        if capped and step >= cap_at and forced < 2:
            ids = list(range(n_views))
            if int(model.after_allocate(ids).sum()) > max_bricks:
                forced += 1
                ops.append(("refused", ids))
                refusals += 1
    c.__dict__.update(ops=ops, max_bricks=max_bricks, moves=moves, refusals=refusals, forced=forced, zero_start=zero_start)
    _cache["C", k] = c
    return c


# ---- named cases --------------------------------------------------------------------------------------------------------------------
def cull_bound_case(pm):
    """A 20 x 10 x 9 lattice and five views in one chunk: two ordinary ones around a camera with t[2] = 2^41 whose depth map holds 2^41
    (not culled: W.cull == 0; z == 2^41 exactly, s == 0, so every voxel that lands in its image gains weight 1 and sum 0), one with a
    NaN in K[2] and one with a NaN in R[4] (not culled either, and no voxel passes step 2 or 4).  -> Case with `far`, `nan_k`, `nan_r`:
    the three views' positions"""
    if "cull" in _cache:
        return _cache["cull"]
    rng = np.random.default_rng((SEED_A, 10 ** 6))
    dims = (20, 10, 9)
    origin, voxel, trunc, cams, depths, cols, _ = _scene(pm, rng, dims, 5, inside_every=0)
    big = float(2.0 ** 41)
    far = pm.make_camera(np.array([[20.0, 0, 9.5], [0, 20.0, 7.5], [0, 0, 1]]), np.eye(3), np.array([0.1, -0.2, big]), 16, 20, 0.05, 50.0)
    cams[1], depths[1], cols[1] = far, np.full((16, 20), big, F), rng.integers(0, 256, (16, 20, 3), dtype=np.uint8)
    cams[3].K[2] = float("nan")
    cams[4].R[4] = float("nan")
    c = Case(k="cull", dims=dims, origin=origin, voxel=voxel, trunc=trunc, cams=cams, depths=depths, images=cols, far=1, nan_k=3, nan_r=4)
    _cache["cull"] = c
    return c


def chunk_case(pm, n):
    """n views (8, 9, 16 or 17) into a 70 x 9 x 3 lattice: one call must equal n single-view calls"""
    if ("chunk", n) in _cache:
        return _cache["chunk", n]
    rng = np.random.default_rng((SEED_A, 10 ** 6 + n))
    dims = (70, 9, 3)
    origin, voxel, trunc, cams, depths, cols, _ = _scene(pm, rng, dims, n)
    c = Case(k=f"chunk{n}", dims=dims, origin=origin, voxel=voxel, trunc=trunc, cams=cams, depths=depths, images=cols)
    _cache["chunk", n] = c
    return c
