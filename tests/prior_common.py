"""The device half of the planar prior (mp-mvs_amd/csrc/pm_prior.hpp; reference src/PatchMatch.cpp:554-595, :723-755) restated in plain
numpy, and the seeded cases of its parity sweep; shared by tests/test_prior_sweep_cpu.py (the statements against the host library, the
row bound of the task table, what the sweep covers) and tests/test_prior_sweep_gpu.py (the device against the host library).  Nothing
here calls the library; draw(k) and the named big cases are pure functions.

reference_rows(e)   how many p-rows `for (float p = 0; p < 1.0; p += step)` runs for a longest edge of integer square e, with
                    step = (float)(1.0 / (float)sqrt(e)) and sequential fp32 additions, literally.  The additions inside one binade
                    all round the same way, so the count drifts away from floor(L) + 2 as L grows: the task table of
                    mpmvs_prior_from_triangles must cover this count, not L.
raster_statement    the barycentric stepping, labels k + 1, the largest label wins; plane_statement: the plane through the three
                    back-projected vertices.  Slow: small cases only.
draw(k)             one case of the sweep: W, H in 5..160 (every fourth a thin strip), 0..400 triangles mixed from TRI_KINDS, a state
                    whose .w (the depth) at the vertex pixels is mixed from DEPTH_KINDS, a camera with fx != fy in half of the cases,
                    and a depth range out of RANGE_KINDS.  The case's d0 and fx are chosen so that fl(d0 * fx) is exact: the
                    fronto-parallel plane through three vertices of depth d0 then has prior depth d0 exactly at every pixel, and a
                    range that ends on d0, or one float inside it, is decided by the <= / >= of k_prior_finish alone.
census()            how many of the default cases hold each kind; the drawing is repeated with the attempt number in the seed until
                    every kind occurs in at least CENSUS_MIN cases."""
import importlib
import math
from types import SimpleNamespace

import numpy as np

CASE_SEED = 5640
DEFAULT_CASES = 48
CENSUS_MIN = 3
TASK_ROWS = 64                           # p-rows per raster task (one wave)
TRI_KINDS = ("small", "duplicate", "point", "two_equal", "collinear", "last_col_row", "border_sliver", "task_edge", "overlap")
DEPTH_KINDS = ("uniform", "const", "zero", "negative", "nan", "inf")
RANGE_KINDS = ("unbounded", "interior", "min_eq_d0", "max_eq_d0", "min_above_d0", "max_below_d0")
TASK_EDGE_ROWS = (63, 64, 65, 127, 128, 129)      # floor(L) + 3 on both sides of one and two tasks
BIG = 3.0e38
_f32 = np.float32
_cache = {}


# ---- the row count of the reference's loop ------------------------------------------------------------------------------------------------
def edge_step(e):
    """(L, step) as the reference forms them: L = (float)sqrt((double)e), step = (float)(1.0 / L)"""
    e = np.asarray(e, np.int64)
    L = np.sqrt(e.astype(np.float64)).astype(np.float32)
    with np.errstate(divide="ignore"):
        step = (1.0 / L.astype(np.float64)).astype(np.float32)
    return L, step


def reference_rows(e):
    """rows of `for (float p = 0; p < 1.0; p += step)` per entry of e (a scalar gives an int).  One fp32 addition per row and entry:
    the entries are sorted by e, a larger e has a smaller step and (rounding is monotone) never a larger p after the same number of
    additions, so the entries still running are a suffix of the sorted array and only that suffix is added to."""
    e = np.asarray(e, np.int64)
    flat = e.reshape(-1)
    order = np.argsort(flat, kind="stable")
    _, step = edge_step(flat[order])
    p = np.zeros(len(flat), np.float32)
    rows = np.zeros(len(flat), np.int64)
    start, k = 0, 0
    while start < len(flat):
        k += 1                                          # row k - 1 ran (p < 1 held); the addition after it:
        p[start:] += step[start:]
        while start < len(flat) and not p[start] < 1.0:
            rows[start] = k
            start += 1
    out = np.empty(len(flat), np.int64)
    out[order] = rows
    return int(out[0]) if e.ndim == 0 else out.reshape(e.shape)


def dispatched_rows_before(e):
    """what the task table covered before the bound was corrected: (int)sqrt(e) + 3 rows, in whole tasks"""
    r = np.floor(np.sqrt(np.asarray(e, np.int64).astype(np.float64))).astype(np.int64) + 3
    return TASK_ROWS * ((r + TASK_ROWS - 1) // TASK_ROWS)


def longest_edge_sq(tri):
    """[n] int64: the largest squared edge length of triangles [n][3][2]"""
    t = np.asarray(tri, np.int64).reshape(-1, 3, 2)
    d = np.stack([t[:, 0] - t[:, 1], t[:, 0] - t[:, 2], t[:, 1] - t[:, 2]], 1)
    return (d * d).sum(-1).max(1) if len(t) else np.zeros(0, np.int64)


# ---- the statements -------------------------------------------------------------------------------------------------------------------------
def _steps(e):
    """the values p (and q) takes: 0, step, fl(step + step), ... while below 1, as fp32"""
    _, step = edge_step(e)
    seq, p = [], _f32(0.0)
    while p < 1.0:
        seq.append(p)
        with np.errstate(invalid="ignore"):
            p = _f32(p + step)
    return np.array(seq, np.float32)


def raster_rows(W, H, tri3, first_row=0, end_row=None):
    """the pixels (y, x) one triangle [3][2] touches in its p-rows first_row .. end_row - 1 (all: None), as a bool image (reference :564-570:
    x = p * x1 + q * x2 in fp32, plus (1.0 - p - q) * x3 in double, truncated; samples outside the image are dropped as the host
    and the device drop them)"""
    (x1, y1), (x2, y2), (x3, y3) = (tuple(int(v) for v in p) for p in np.asarray(tri3).reshape(3, 2))
    seq = _steps(longest_edge_sq([tri3])[0])
    hit = np.zeros((H, W), bool)
    s64 = seq.astype(np.float64)
    for p in seq[first_row:end_row]:
        q = seq[s64 < 1.0 - float(p)]
        rest = 1.0 - float(p) - q.astype(np.float64)
        x = ((p * _f32(x1) + q * _f32(x2)).astype(np.float64) + rest * x3).astype(np.int64)
        y = ((p * _f32(y1) + q * _f32(y2)).astype(np.float64) + rest * y3).astype(np.int64)
        ok = (x >= 0) & (y >= 0) & (x < W) & (y < H)
        hit[y[ok], x[ok]] = True
    return hit


def raster_statement(W, H, tri):
    """[H][W] uint32 raw labels: triangle k writes k + 1 over what is there (the last triangle wins)"""
    label = np.zeros((H, W), np.uint32)
    for k, t in enumerate(np.asarray(tri).reshape(-1, 3, 2)):
        label[raster_rows(W, H, t)] = k + 1
    return label


def plane_statement(cam, depths, tri):
    """([n][4] float64, [n] bool): per triangle the unit normal and offset of the plane through its vertices, back-projected as
    reference :200-209 does (fp32: depth * (x - cx) / fx), the cross product and all that follows in float64, the offset made
    positive (:746-752); and whether the fallback was taken: where the cross product has no length above 1e-30 (a repeated vertex,
    collinear points in space, or a NaN from a non-finite depth) the plane is the fronto-parallel one through the first vertex."""
    K = [_f32(v) for v in cam.K]
    tri = np.asarray(tri).reshape(-1, 3, 2)
    out, fallback = np.zeros((len(tri), 4)), np.zeros(len(tri), bool)
    with np.errstate(all="ignore"):
        for k, t in enumerate(tri):
            X = []
            for x, y in t:
                d = _f32(depths[y, x])
                X.append(np.array([d * (_f32(x) - K[2]) / K[0], d * (_f32(y) - K[5]) / K[4], d], np.float64))
            u, v = X[1] - X[0], X[2] - X[0]
            n = np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]])
            norm = np.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
            if not norm > 1e-30:
                n, norm, fallback[k] = np.array([0.0, 0.0, -1.0]), 1.0, True
            off = -(n[0] * X[0][0] + n[1] * X[0][1] + n[2] * X[0][2])
            if off < 0:
                norm = -norm
            out[k, :3], out[k, 3] = n / norm, off / norm
    return out, fallback


def prior_depth_statement(K, planes4, W, H):
    """[H][W] float32: the depth of the per-pixel planes [H][W][4] at their own pixels, the fp32 operations of reference :650-653 in
    their order: -w * fx / ((x - cx) * nx + (fx / fy) * (y - cy) * ny + fx * nz)"""
    K0, K2, K4, K5 = (_f32(K[i]) for i in (0, 2, 4, 5))
    x, y = np.arange(W, dtype=np.float32)[None, :], np.arange(H, dtype=np.float32)[:, None]
    pl = np.asarray(planes4, np.float32)
    with np.errstate(all="ignore"):
        return -pl[..., 3] * K0 / ((x - K2) * pl[..., 0] + (K0 / K4) * (y - K5) * pl[..., 1] + K0 * pl[..., 2])


def area2(tri):
    """[n] int64: twice the area of triangles [n][3][2]"""
    t = np.asarray(tri, np.int64).reshape(-1, 3, 2)
    u, v = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
    return np.abs(u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0])


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
def make_cam(c):
    """the case's camera (test_prior_golden_cpu.make_cam: K, identity rotation)"""
    return importlib.import_module("test_prior_golden_cpu").make_cam(c.K, c.W, c.H)


def _pt(rng, W, H):
    return [int(rng.integers(0, W)), int(rng.integers(0, H))]


def _near(rng, W, H, a, r):
    return [int(np.clip(a[0] + rng.integers(-r, r + 1), 0, W - 1)), int(np.clip(a[1] + rng.integers(-r, r + 1), 0, H - 1))]


def _triangle(rng, kind, W, H, have, patch):
    """one triangle [3][2] of `kind` (a list of them for "overlap"); None if the image cannot hold one"""
    if kind == "small":
        a = _pt(rng, W, H)
        return [a, _near(rng, W, H, a, 6), _near(rng, W, H, a, 6)]
    if kind == "duplicate":
        if not have:
            return None
        t = have[int(rng.integers(0, len(have)))]
        return [t[i] for i in ((1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0), (1, 0, 2))[int(rng.integers(0, 5))]]
    if kind == "point":
        a = _pt(rng, W, H)
        return [a, a, a]
    if kind == "two_equal":
        a = _pt(rng, W, H)
        b = _near(rng, W, H, a, 9)
        return [[a, a, b], [a, b, a], [b, a, a]][int(rng.integers(0, 3))]
    if kind == "collinear":
        a, d = _pt(rng, W, H), [int(v) for v in rng.integers(-3, 4, 2)]
        m = [int(v) for v in rng.permutation(np.arange(-4, 5))[:2]]
        t = [a] + [[a[0] + k * d[0], a[1] + k * d[1]] for k in m]
        return t if all(0 <= x < W and 0 <= y < H for x, y in t) else None
    if kind == "last_col_row":
        a = [[W - 1, int(rng.integers(0, H))], [int(rng.integers(0, W)), H - 1], [W - 1, H - 1]][int(rng.integers(0, 3))]
        b, c = _near(rng, W, H, a, 5), _near(rng, W, H, a, 5)
        b[0], c[1] = (W - 1 if rng.random() < 0.5 else b[0]), (H - 1 if rng.random() < 0.5 else c[1])
        return [a, b, c]
    if kind == "border_sliver":
        side, off = int(rng.integers(0, 4)), int(rng.integers(0, 3))
        if side < 2:                                    # along the top or bottom row, the whole width
            y, x = (0 if side == 0 else H - 1), int(rng.integers(0, W))
            t = [[0, y], [W - 1, y], [x, min(H - 1, off) if side == 0 else max(0, H - 1 - off)]]
        else:
            x, y = (0 if side == 2 else W - 1), int(rng.integers(0, H))
            t = [[x, 0], [x, H - 1], [min(W - 1, off) if side == 2 else max(0, W - 1 - off), y]]
        return [t[i] for i in rng.permutation(3)]
    if kind == "task_edge":
        want = int(rng.choice(TASK_EDGE_ROWS)) - 3
        dx, dy = np.meshgrid(np.arange(W), np.arange(H))
        fits = np.argwhere(np.floor(np.sqrt((dx * dx + dy * dy).astype(np.float64))) == want)
        if not len(fits):
            return None
        dy, dx = (int(v) for v in fits[int(rng.integers(0, len(fits)))])
        x0, y0 = int(rng.integers(0, W - dx)), int(rng.integers(0, H - dy))
        a, b = ([x0, y0], [x0 + dx, y0 + dy]) if rng.random() < 0.5 else ([x0 + dx, y0], [x0, y0 + dy])
        c = _near(rng, W, H, a if rng.random() < 0.5 else b, 4)
        t = [a, b, c]
        if math.floor(math.sqrt(int(longest_edge_sq([t])[0]))) != want:      # the third vertex made a longer edge
            t = [a, b, a]
        return [t[i] for i in rng.permutation(3)]
    if kind == "overlap":                               # 50 triangles over one 6 x 6 patch
        px, py = patch
        return [[[px + int(v[0]), py + int(v[1])] for v in rng.integers(0, 6, (3, 2))] for _ in range(50)]
    raise ValueError(kind)


def _depth_kind(d3):
    """the kind a triangle's three vertex depths make (after every write to the map)"""
    if np.isnan(d3).any():
        return "nan"
    if np.isinf(d3).any():
        return "inf"
    if (d3 < 0).any():
        return "negative"
    if (d3 == 0).any():
        return "zero"
    return "const" if d3[0] == d3[1] == d3[2] else "uniform"


def _draw(k, attempt):
    rng = np.random.default_rng([CASE_SEED, attempt, k])
    c = SimpleNamespace(case=k, attempt=attempt)
    if k % 4 == 3:                                      # a thin strip, lying or standing
        long_side, thin = int(rng.integers(200, 301)), int(rng.integers(5, 9))
        c.W, c.H = (long_side, thin) if (k // 4) % 2 == 0 else (thin, long_side)
    else:
        c.W, c.H = int(rng.integers(5, 161)), int(rng.integers(5, 161))
    W, H = c.W, c.H
    # fx a multiple of 1/2 and d0 a multiple of 1/4: fl(d0 * fx) is exact, so a fronto-parallel prior at d0 has depth d0 exactly
    fx = float(rng.integers(100, 400)) / 2.0
    fy = fx if k % 2 == 0 else float(rng.integers(100, 400)) / 2.0
    c.K = [fx, 0.0, float(rng.uniform(0.3, 0.7)) * W, 0.0, fy, float(rng.uniform(0.3, 0.7)) * H, 0.0, 0.0, 1.0]
    c.d0 = float(rng.integers(8, 37)) / 4.0
    n = 0 if k % 16 == 5 else int(rng.integers(1, 401))
    kinds = [kd for kd in TRI_KINDS if rng.random() < 0.5] or ["small"]
    tris, held = [], set()
    patch = (int(rng.integers(0, W - 5)), int(rng.integers(0, H - 5))) if W >= 6 and H >= 6 else None
    guard = 0
    while len(tris) < n and guard < 4 * n + 8:
        guard += 1
        kind = kinds[int(rng.integers(0, len(kinds)))]
        if kind == "overlap" and (patch is None or "overlap" in held or len(tris) + 50 > n):
            kind = "small"
        t = _triangle(rng, kind, W, H, tris, patch)
        if t is None:
            continue
        held.add(kind)
        tris += t if kind == "overlap" else [t]
    c.tri = np.array(tris, np.int32).reshape(-1, 3, 2)
    assert len(c.tri) <= 400 and ((c.tri >= 0) & (c.tri < [W, H])).all()
    c.tri_kinds = held
    # the state: random normals, depths uniform in [1, 10]; then per triangle one of the case's depth kinds at its vertex pixels
    planes = rng.normal(size=(H, W, 4)).astype(np.float32)
    planes[..., 3] = rng.uniform(1.0, 10.0, (H, W)).astype(np.float32)
    c.range_kind = RANGE_KINDS[int(rng.integers(0, len(RANGE_KINDS)))]
    dkinds = [kd for kd in DEPTH_KINDS[1:] if rng.random() < 0.4]
    if c.range_kind.endswith("d0") and "const" not in dkinds:
        dkinds.append("const")
    special = {"zero": 0.0, "negative": -float(rng.uniform(0.5, 5.0)), "nan": np.nan, "inf": np.inf}
    for t in c.tri:
        if not dkinds or rng.random() < 0.4:
            continue
        kd = dkinds[int(rng.integers(0, len(dkinds)))]
        if kd == "const":
            planes[t[:, 1], t[:, 0], 3] = c.d0
        else:
            v = t[int(rng.integers(0, 3))]
            planes[v[1], v[0], 3] = special[kd]
    c.planes = planes
    c.depth_kinds = {_depth_kind(planes[t[:, 1], t[:, 0], 3]) for t in c.tri}
    d0 = _f32(c.d0)
    c.depth_min, c.depth_max = {
        "unbounded": (-BIG, BIG), "interior": (float(rng.uniform(1.5, 4.0)), float(rng.uniform(6.0, 9.5))),
        "min_eq_d0": (float(d0), BIG), "max_eq_d0": (-BIG, float(d0)),
        "min_above_d0": (float(np.nextafter(d0, _f32(np.inf))), BIG), "max_below_d0": (-BIG, float(np.nextafter(d0, _f32(-np.inf))))}[c.range_kind]
    return c


def _census(attempt):
    count = {kd: 0 for kd in TRI_KINDS + DEPTH_KINDS + RANGE_KINDS}
    for k in range(DEFAULT_CASES):
        c = _draw(k, attempt)
        for kd in c.tri_kinds | c.depth_kinds | ({c.range_kind} if len(c.tri) else set()):
            count[kd] += 1
    return count


def attempt():
    """the first attempt number at which the default cases hold every kind at least CENSUS_MIN times"""
    if "attempt" not in _cache:
        for a in range(100):
            if min(_census(a).values()) >= CENSUS_MIN:
                _cache["attempt"] = a
                break
        else:
            raise AssertionError("no drawing of the default cases holds every kind")
    return _cache["attempt"]


def census():
    return _census(attempt())


def draw(k):
    if ("case", k) not in _cache:
        _cache["case", k] = _draw(k, attempt())
    return _cache["case", k]


# ---- the named big cases ---------------------------------------------------------------------------------------------------------------------
def _flat_state(W, H, seed):
    """normals towards the camera, depths uniform in [1, 10] (seed None: 5 everywhere)"""
    planes = np.zeros((H, W, 4), np.float32)
    planes[..., 2] = -1.0
    planes[..., 3] = 5.0 if seed is None else np.random.default_rng([CASE_SEED, seed]).uniform(1.0, 10.0, (H, W)).astype(np.float32)
    return planes


def many_triangles():
    """70 001 triangles with edges of at most 6 px on 320 x 240: above the 65 536 triangles from which the task table is built by
    host threads in chunks, one task each, so the task count (70 001) is no multiple of the 4 tasks of a block"""
    if "many" not in _cache:
        rng = np.random.default_rng([CASE_SEED, 70001])
        W, H, n = 320, 240, 70001
        a = np.stack([rng.integers(0, W - 4, n), rng.integers(0, H - 4, n)], 1)
        tri = (a[:, None, :] + rng.integers(0, 5, (n, 3, 2))).astype(np.int32)     # inside a 5 x 5 box: no edge above sqrt(32) < 6
        assert longest_edge_sq(tri).max() <= 36 and (dispatched_rows_before(longest_edge_sq(tri)) == TASK_ROWS).all()
        _cache["many"] = SimpleNamespace(W=W, H=H, K=[250.0, 0.0, 160.0, 0.0, 240.5, 120.0, 0.0, 0.0, 1.0], tri=tri, planes=_flat_state(W, H, 1), level=_flat_state(W, H, None),
                                         depth_min=2.0, depth_max=9.0)
    return _cache["many"]


def whole_task_edge():
    """the smallest L <= 65 534 whose sliver (L, 0), (0, 5), (0, 0) runs a whole task of rows more than were dispatched before the
    bound was corrected, or None"""
    if "whole" not in _cache:
        L = np.arange(1, 65535, dtype=np.int64)
        e = L * L + 25
        over = reference_rows(e) - dispatched_rows_before(e) >= TASK_ROWS
        _cache["whole"] = int(L[over][0]) if over.any() else None
    return _cache["whole"]


def _sliver_case(L):
    """a (L + 1) x 8 image: a dozen small triangles near (L, 0), the far end of the sliver (L, 0), (0, 5), (0, 0) that sits in the
    middle of the list: it overwrites six of them and the other six overwrite it; they stay 8 columns away from the end itself, where
    the sliver's last rows land"""
    rng = np.random.default_rng([CASE_SEED, L])
    W, H = L + 1, 8
    small = [[[L - int(v[0]), int(v[1])] for v in zip(rng.integers(8, 48, 3), rng.integers(0, 8, 3))] for _ in range(12)]
    tri = np.array(small[:6] + [[[L, 0], [0, 5], [0, 0]]] + small[6:], np.int32)
    return SimpleNamespace(W=W, H=H, L=L, sliver=6, K=[float(L), 0.0, 0.5 * L, 0.0, float(L), 4.0, 0.0, 0.0, 1.0], tri=tri, planes=_flat_state(W, H, L),
                           depth_min=1.5, depth_max=9.5, e=int(L) * int(L) + 25)


SLIVER_EDGES = (4096, 8192, 14973)       # 14973: the smallest integer edge with a height of 5 whose loop outruns the rows dispatched before


def long_slivers():
    """one image per entry; the last is whole_task_edge()'s, where there is one"""
    if "slivers" not in _cache:
        edges = list(SLIVER_EDGES) + ([whole_task_edge()] if whole_task_edge() is not None else [])
        _cache["slivers"] = [_sliver_case(L) for L in edges]
    return _cache["slivers"]


def wide_sliver():
    """a 46342 x 8 image of the same make: the first edge whose square, 46 341^2 = 2 147 488 281, no longer fits an int32, which the
    reference's pow(dx, 2) never notices"""
    if "wide" not in _cache:
        _cache["wide"] = _sliver_case(46341)
    return _cache["wide"]
