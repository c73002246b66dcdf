"""Seeded random programs of operations on one long-lived mpmvs_cloud handle, shared by tests/test_cloud_seq_cpu.py (what the
sweep covers, on the statements alone) and tests/test_cloud_seq_gpu.py (the sweep on the MI355X); a plain model of the handle's
grid cache (cloud_grid in csrc/mpmvs_cloud.hip); and the expected result of every step from the statements the
operations already have.  case(k) is a pure function of k.

What a case varies: a target of 1..400 points (weight on 1, 2, 255, 256, 257: the edges of the 256-thread blocks of insert,
scatter, qbin and query), two query and two source clouds of 0..300 points, rows with NaN or +-inf in one coordinate, exact
duplicates, the whole scene offset by 1000.25, an anisotropic box, three magnitudes; one case in eight has no finite target at all
(every call is answered on the host and nothing is ever built).  9..12 radii per case, among them one pair one ulp apart; a program
of 30..50 steps over nearest, knn, knn_self, normals, components, the two align passes and render_depth, with two aligners (one
with normals) opened and closed at random points.  The radius of a step is drawn with the model at hand: a recent radius (a hit,
often on a grid another kind of operation built), a radius the model has evicted (a rebuild in a reused buffer), or any of the
pool; a program that leaves one of these out is drawn again (the attempt number enters the seed)."""
import importlib

import numpy as np

import align_common as ac
import align_plane_common as apc
import cloud_common as cc
import components_common as cmp_c
import knn_common as kc
import normals_common as nc
import render_common as rc

CASE_SEED = 9100
DEFAULT_CASES = 24                      # what the sweep runs unless MPMVS_CLOUD_SEQ_CASES says otherwise; the coverage test is over these
MAX_GRIDS = 8                           # kCloudMaxGrids
EDGE_COUNTS = (1, 2, 255, 256, 257)
KS = (1, 4, 5, 8, 16, 17, 32)           # both sides of the list sizes 4, 8, 16, 32 of k_knn_list
KINDS = ("nearest", "knn", "knn_self", "normals", "components", "sums", "plane_sums", "render")
ALIGN_KINDS = ("sums", "plane_sums")
OFFSET = 1000.25
BAD = (np.nan, np.inf, -np.inf)
_cache = {}


def rkey(radius):
    """the cache's key: the bits of the radius as the library receives it"""
    return np.float32(radius).tobytes()


class GridCacheModel:
    """The contract of cloud_grid: at most MAX_GRIDS radii, keyed on their fp32 bits; a hit refreshes recency; a miss takes a free
    place or that of the least recently used radius.  request(r) -> True for a build.  A target without a finite point never
    builds and keeps nothing.  Calls that do not reach the grid (render_depth; a search without queries; a pass without sources)
    must not be passed to request().  `tag` names who asks; after a request, `last` is ("hit", tag of the builder) or
    ("build", key of the evicted radius or None)."""

    def __init__(self, finite=True, capacity=MAX_GRIDS):
        self.finite, self.capacity = finite, capacity
        self.lru = []          # keys, least recently used first
        self.builder = {}      # key -> tag of the request that built it
        self.evicted = []      # keys evicted and not resident, oldest first
        self.builds = self.hits = self.evictions = 0
        self.last = None

    def resident(self, radius):
        return rkey(radius) in self.lru

    def request(self, radius, tag=None):
        if not self.finite:
            self.last = None
            return False
        k = rkey(radius)
        if k in self.lru:
            self.lru.remove(k)
            self.lru.append(k)
            self.hits += 1
            self.last = ("hit", self.builder[k])
            return False
        gone = None
        if len(self.lru) == self.capacity:
            gone = self.lru.pop(0)
            del self.builder[gone]
            self.evicted.append(gone)
            self.evictions += 1
        if k in self.evicted:
            self.evicted.remove(k)
        self.lru.append(k)
        self.builder[k] = tag
        self.builds += 1
        self.last = ("build", gone)
        return True


class Step:
    """one entry of a program.  kind: one of KINDS, or "open" / "close" (of aligner `al`).  radius: a float that is exact in fp32
    (None for render, open and close).  args: the rest, per kind (see run order in expected())"""

    def __init__(self, kind, radius=None, **args):
        self.kind, self.radius, self.args = kind, radius, args

    def __repr__(self):
        return f"Step({self.kind}, {self.radius}, {self.args})"

    def key(self):
        """what the result depends on"""
        a = {k: v for k, v in self.args.items() if not k.startswith("want_")}
        return (self.kind, self.radius, tuple(sorted(a.items())))


class SeqCase:
    def __init__(self, **kw):
        self.__dict__.update(kw)
        self.memo = {}

    @property
    def ops(self):
        return [s for s in self.program if s.kind in KINDS]

    def touches_grid(self, s):
        """whether the call reaches cloud_grid on a target with finite points: not a render, not a search without queries, not a
        pass without sources"""
        if s.kind == "render" or s.kind not in KINDS:
            return False
        if s.kind in ("nearest", "knn"):
            return len(self.queries[s.args["q"]]) > 0
        if s.kind in ALIGN_KINDS:
            return len(self.sources[s.args["al"]]) > 0
        return True


def _f32(x):
    return float(np.float32(x))


def _draw_count(rng, lo, hi, special):
    return int(rng.choice(special)) if rng.random() < 0.4 else int(rng.integers(lo, hi + 1))


def _spoil(rng, a, share):
    """exact duplicates of other rows, then rows with NaN or +-inf in one coordinate"""
    n = len(a)
    if n >= 2:
        m = int(rng.binomial(n, share))
        dst, src = rng.integers(0, n, m), rng.integers(0, n, m)
        a[dst] = a[src]
    m = int(rng.binomial(n, share))
    rows = rng.integers(0, n, m) if n else np.zeros(0, int)
    a[rows, rng.integers(0, 3, m)] = rng.choice(np.array(BAD, np.float32), m)
    return a


def _near(rng, base, lo, box, n, jitter):
    """n points: half around rows of `base` (any row, finite or not), half uniform in the box grown by a fifth"""
    a = lo + (rng.random((n, 3)) * 1.4 - 0.2) * box
    if len(base) and n:
        pick = rng.random(n) < 0.5
        a[pick] = base[rng.integers(0, len(base), int(pick.sum()))].astype(np.float64) + rng.normal(0, jitter, (int(pick.sum()), 3))
    return np.ascontiguousarray(a, np.float32)


def _about(T, c):
    """the similarity T turning and scaling about the point c"""
    T = T.copy()
    T[:3, 3] += c - T[:3, :3] @ c
    return T


def _camera(rng, centre, extent, width, height, angle):
    _abi = importlib.import_module("mp-mvs_amd._abi")
    R = ac.similarity(rng, angle, 1.0, 0.0)[:3, :3]
    C = centre + R.T @ np.array([0.0, 0.0, -2.0 * extent]) + rng.normal(0, 0.05 * extent, 3)   # two extents in front of the cloud
    f = 0.9 * max(width, height)
    K = np.array([[f, 0, 0.5 * (width - 1)], [0, f, 0.5 * (height - 1)], [0, 0, 1]])
    return _abi.make_camera(K, R, -R @ C, height, width, 0.1 * extent, 10.0 * extent)


def _scene(rng, n_t, offset=0.0, no_finite=False, n_r=None):
    """the clouds, radii (n_r of them; 9..12 if None), transforms, normals and cameras of a case with n_t targets"""
    scale = float(rng.choice([1.0, 0.03, 20.0]))
    box = scale * np.array([1.0, 1.0, float(rng.choice([1.0, 0.3, 0.05]))])
    lo = np.full(3, offset)
    target = _spoil(rng, np.ascontiguousarray(lo + rng.random((n_t, 3)) * box, np.float32), 0.04)
    if no_finite:
        target[np.arange(n_t), rng.integers(0, 3, n_t)] = rng.choice(np.array(BAD, np.float32), n_t)
    fin = target[np.isfinite(target).all(1)]
    extent = float((fin.max(0) - fin.min(0)).max()) if len(fin) else 0.0
    if extent == 0.0:
        extent = scale
    # the radius at which a ball holds about 40 of the finite points, at most the extent; the pool spans a factor of eight below it
    r40 = (40.0 / (4.19 * max(len(fin), 1) / float(np.prod(box)))) ** (1.0 / 3.0)
    r_max = min(r40, extent)
    n_r = int(rng.integers(9, 13)) if n_r is None else n_r
    radii =[np.float32(r_max * 8.0 ** -u) for u in rng.random(n_r - 1)]
    pair = int(rng.integers(0, n_r - 1))
    radii.insert(pair + 1, np.nextafter(radii[pair], np.float32(np.inf)))
    radii = [float(r) for r in radii]
    assert len({rkey(r) for r in radii}) == n_r and all(_f32(r) == r for r in radii)
    assert all(extent / r < 2.0 ** 12 for r in radii)          # the span check allows 2^21 cells per axis
    r_mid = float(np.median(radii))
    queries = [_spoil(rng, _near(rng, target, lo, box, _draw_count(rng, 0, 300, (0, 1, 255, 256, 257)), 0.5 * r_mid), 0.03) for _ in range(2)]
    sources = [_spoil(rng, _near(rng, target, lo, box, _draw_count(rng, 0, 300, (0, 1, 63, 64, 65, 256, 257)), 0.3 * r_mid), 0.03) for _ in range(2)]
    centre = lo + 0.5 * box
    transforms = [np.eye(4)] + [_about(ac.similarity(rng, rng.uniform(0, 0.05), rng.uniform(0.97, 1.03), rng.uniform(0, 0.3 * r_mid)), centre) for _ in range(2)]
    al_normals = rng.normal(size=(n_t, 3)).astype(np.float32)              # of aligner 1; any length, some rows taking no part
    bad = rng.random(n_t) < 0.05
    al_normals[bad] = rng.choice(np.array([0.0, np.nan, np.inf], np.float32), (int(bad.sum()), 1))
    reference = rng.normal(size=(n_t, 3)).astype(np.float32)               # of normals() with orient 2
    viewpoint = centre + np.array([0.3, -0.2, 3.0]) * extent
    cams = [_camera(rng, centre, extent, w, h, a) for (w, h), a in zip(((48, 36), (17, 9), (1, 1)), (0.0, 0.2, 0.1))]
    return dict(no_finite=no_finite, offset=offset, target=target, n_fin=len(fin), extent=extent, radii=radii, ulp_pair=(radii[pair], radii[pair + 1]),
                queries=queries, sources=sources, transforms=transforms, al_normals=al_normals, reference=reference, viewpoint=viewpoint, cams=cams)


def _program(rng, c):
    """the steps, with "open" and "close" entries between them; the radii drawn against a model of a target with finite points"""
    n = int(rng.integers(30, 51))
    opens = [int(rng.integers(0, n // 2)) for _ in range(2)]
    closes = [int(rng.integers(o + 3, n + 1)) for o in opens]
    model, recent, open_now, prog = GridCacheModel(), [], set(), []
    for i in range(n + 1):
        for al in range(2):
            if closes[al] == i:
                prog.append(Step("close", al=al))
                open_now.discard(al)
            if opens[al] == i:
                prog.append(Step("open", al=al))
                open_now.add(al)
        if i == n:
            break
        kinds = list(KINDS[:5]) + ["render"] + (["sums"] * 2 if open_now else []) + (["plane_sums"] * 2 if 1 in open_now else [])
        kind = str(rng.choice(kinds))
        if kind == "render":
            picked = sorted(rng.choice(3, int(rng.integers(1, 4)), replace=False).tolist())
            prog.append(Step("render", cams=tuple(picked), splat=int(rng.integers(0, 3)), occl_rel=float(rng.choice([0.0, 0.02]))))
            continue
        u = rng.random()
        if u < 0.3 and recent:
            radius = recent[int(rng.integers(0, len(recent)))]
        elif u < 0.55 and model.evicted:
            radius = float(np.frombuffer(model.evicted[int(rng.integers(0, len(model.evicted)))], np.float32)[0])
        else:
            radius = c.radii[int(rng.integers(0, len(c.radii)))]
        if kind == "nearest":
            s = Step(kind, radius, q=int(rng.integers(0, 2)), want_idx=bool(rng.random() < 0.8))
        elif kind == "knn":
            s = Step(kind, radius, q=int(rng.integers(0, 2)), k=int(rng.choice(KS)), want_idx=bool(rng.random() < 0.8))
        elif kind == "knn_self":
            s = Step(kind, radius, k=int(rng.choice(KS)), want_idx=bool(rng.random() < 0.8))
        elif kind == "normals":
            s = Step(kind, radius, k=int(rng.choice(KS[1:])), orient=int(rng.integers(0, 3)), want_curvature=bool(rng.random() < 0.8))
        elif kind == "components":
            s = Step(kind, radius, want_size=bool(rng.random() < 0.8))
        elif kind == "sums":
            s = Step(kind, radius, al=int(rng.choice(sorted(open_now))), T=int(rng.integers(0, 3)))
        else:
            s = Step(kind, radius, al=1, T=int(rng.integers(0, 3)))
        prog.append(s)
        if c.touches_grid(s):
            model.request(radius, kind)
            recent = ([radius] + [r for r in recent if r != radius])[:3]
    return prog


def replay(c, finite=None):
    """the model run over the program -> per op step (index into c.program) a dict: build, hit_on_other_kind, rerequest (of a
    radius evicted before), evicts, open_since_eviction (an align pass whose aligner was opened before some eviction)"""
    model = GridCacheModel(c.n_fin > 0 if finite is None else finite)
    opened_at, out = {}, {}
    for i, s in enumerate(c.program):
        if s.kind == "open":
            opened_at[s.args["al"]] = model.evictions
        elif s.kind == "close":
            del opened_at[s.args["al"]]
        elif c.touches_grid(s):
            was_evicted = rkey(s.radius) in model.evicted
            build = model.request(s.radius, s.kind)
            out[i] = dict(build=build, hit_on_other_kind=bool(model.last and model.last[0] == "hit" and model.last[1] != s.kind),
                          rerequest=build and was_evicted, evicts=bool(model.last and model.last[0] == "build" and model.last[1] is not None),
                          open_since_eviction=s.kind in ALIGN_KINDS and model.evictions > opened_at[s.args["al"]])
        elif s.kind in KINDS:
            out[i] = dict(build=False, hit_on_other_kind=False, rerequest=False, evicts=False, open_since_eviction=False)
    assert not opened_at, "an aligner is left open"
    return out


def covers(c):
    """what every program must contain, on the model of a target with finite points"""
    rows = replay(c, finite=True).values()
    used = {rkey(s.radius) for s in c.program if c.touches_grid(s)}
    return (any(r["evicts"] for r in rows) and any(r["rerequest"] for r in rows) and any(r["hit_on_other_kind"] for r in rows)
            and all(rkey(r) in used for r in c.ulp_pair))


def hand_case(seed, n_t, program=(), **kw):
    """a case of the named tests: the scene of _scene under a seed of its own, the program written by hand"""
    c = SeqCase(k=f"hand{seed}", attempt=0, **_scene(np.random.default_rng([CASE_SEED, 1000000 + seed]), n_t, **kw))
    c.program = list(program)
    return c


def case(k):
    if k not in _cache:
        rng = np.random.default_rng([CASE_SEED, k])
        # the first cases take the edge counts in turn; every eighth has no finite target; every third is offset
        n_t = EDGE_COUNTS[k] if k < len(EDGE_COUNTS) else _draw_count(rng, 1, 400, EDGE_COUNTS)
        scene = _scene(rng, n_t, OFFSET if k % 3 == 1 else 0.0, k % 8 == 7)
        for attempt in range(100):
            c = SeqCase(k=k, attempt=attempt, **scene)
            c.program = _program(np.random.default_rng([CASE_SEED, k, attempt]), c)
            if covers(c):
                break
        else:
            raise AssertionError(f"case {k}: no program with an eviction, a re-request, a shared hit and the one-ulp pair in 100 draws")
        _cache[k] = c
    return _cache[k]


def cell(x, mn, radius):
    """cloud_cell of csrc/pm_cloud.hpp for a coordinate inside the grid: floor(((double)x - mn) / edge), edge = radius * (1 + 2^-10)"""
    return int(np.floor((float(np.float32(x)) - float(mn)) / (float(np.float32(radius)) * (1.0 + 2.0 ** -10))))


def border_scene():
    """(targets float32 [2, 3], query float32 [1, 3], r, s, N): r = 0.25, s the float above it; the targets are the origin (the grid's
    corner) and P = (x_p, 0, 0), the query is Q = (x_q, 0, 0), about 2^18 cells out, where the two edges' cell borders are a
    float apart.  P lies in cell N of the grid of r and in cell N - 1 of the grid of s; Q lies in cell N + 1 of the grid of r
    and |Q - P| <= r.  A search at r that is served the grid of s looks at the cells N .. N + 2 and misses P."""
    f = np.float32
    r = f(0.25)
    s = np.nextafter(r, f(1))
    er, es = float(r) * (1.0 + 2.0 ** -10), float(s) * (1.0 + 2.0 ** -10)
    for N in range(1 << 18, (1 << 18) + 4096):
        xp = f(N * es)
        while float(xp) >= N * es:
            xp = np.nextafter(xp, f(-np.inf))                  # the largest float in cell N - 1 of s
        xq = f((N + 1) * er)
        while float(xq) < (N + 1) * er:
            xq = np.nextafter(xq, f(np.inf))                   # the smallest float in cell N + 1 of r
        d = xq - xp
        if (cell(xp, 0, r), cell(xp, 0, s), cell(xq, 0, r), cell(xq, 0, s)) == (N, N - 1, N + 1, N) and d * d <= r * r:
            return np.array([[0, 0, 0], [xp, 0, 0]], f), np.array([[xq, 0, 0]], f), float(r), float(s), N
    raise AssertionError("no such pair of floats")


# ---- the expected result of a step, from the statements; none depends on history ---------------------------------------------------
def _state(c, s):
    r, a = s.radius, s.args
    if s.kind == "nearest":
        return cc.brute_nearest(c.target, c.queries[a["q"]], r)
    if s.kind == "knn":
        return kc.brute_knn(c.target, c.queries[a["q"]], r, a["k"])
    if s.kind == "knn_self":
        return kc.brute_knn(c.target, None, r, a["k"])
    if s.kind == "normals":
        return nc.statement_normals(c.target, r, a["k"], c.viewpoint if a["orient"] == 1 else None, c.reference if a["orient"] == 2 else None)
    if s.kind == "components":
        return cmp_c.statement_components(c.target, r)
    if s.kind == "sums":
        return ac.brute_sums(c.target, c.sources[a["al"]], c.transforms[a["T"]], r)
    if s.kind == "plane_sums":
        return apc.plane_sums(c.target, c.al_normals, c.sources[a["al"]], c.transforms[a["T"]], r)
    if s.kind == "render":
        return rc.render_statement(c.target, [c.cams[v] for v in a["cams"]], a["splat"], a["occl_rel"])
    raise ValueError(s.kind)


def expected(c, s):
    key = s.key()
    if key not in c.memo:
        c.memo[key] = _state(c, s)
    return c.memo[key]


def assert_step_same(s, got, want, what=""):
    """the comparison rule of the operation's own tests: every row, bit for bit"""
    what = f"{what} {s!r}"
    if s.kind == "nearest":
        cc.assert_same(got, want)
    elif s.kind in ("knn", "knn_self"):
        kc.assert_knn_same(got, want, what)
    elif s.kind == "normals":
        nc.assert_normals_same(got, want, what)
    elif s.kind == "components":
        cmp_c.assert_components_same(got, want, what)
    elif s.kind in ALIGN_KINDS:
        assert got[0].dtype == np.int64 and got[0].shape == want[0].shape and np.array_equal(got[0], want[0]), (what, got[0] - want[0])
        assert np.array_equal(got[1], want[1]), (what, got[1], want[1])
    elif s.kind == "render":
        rc.assert_same(got[0], got[1], want[0], want[1])
    else:
        raise ValueError(s.kind)


# ---- running a step on the library (the GPU tests) -----------------------------------------------------------------------------------
def open_aligner(cloud, handle, c, al):
    a = cloud.Aligner(handle, c.sources[al])
    if al == 1:
        a.set_normals(c.al_normals)
    return a


def run_step(handle, aligners, c, s):
    """the call of step s on the Cloud `handle` (aligners: {id: Aligner}) -> what assert_step_same compares"""
    r, a = s.radius, s.args
    if s.kind == "nearest":
        return handle.nearest(c.queries[a["q"]], r, want_idx=a["want_idx"])
    if s.kind == "knn":
        return handle.knn(c.queries[a["q"]], r, a["k"], want_idx=a["want_idx"], want_within=True)
    if s.kind == "knn_self":
        return handle.knn_self(r, a["k"], want_idx=a["want_idx"], want_within=True)
    if s.kind == "normals":
        return handle.normals(r, a["k"], viewpoint=c.viewpoint if a["orient"] == 1 else None, reference=c.reference if a["orient"] == 2 else None,
                              want_curvature=a["want_curvature"], want_within=True)
    if s.kind == "components":
        return handle.components(r, want_size=a["want_size"])
    if s.kind == "sums":
        return aligners[a["al"]].sums(r, c.transforms[a["T"]])
    if s.kind == "plane_sums":
        return aligners[a["al"]].plane_sums(r, c.transforms[a["T"]])
    if s.kind == "render":
        return handle.render_depth([c.cams[v] for v in a["cams"]], a["splat"], a["occl_rel"], want_idx=True)
    raise ValueError(s.kind)


def build_figure(handle, s):
    """the build ms the step's operation reports; an align pass reports through the target's kernel_ms()"""
    if s.kind in ("knn", "knn_self"):
        return handle.knn_ms()[1]
    if s.kind == "normals":
        return handle.normals_ms()[1]
    if s.kind == "components":
        return handle.components_ms()[1]
    return handle.kernel_ms()[1]
