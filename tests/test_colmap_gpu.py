"""COLMAP converter on the GPU: mpmvs_view_select against a vectorised numpy point-major statement, the fixture end to
end against the reference converter's recorded outputs, and PatchMatch + fusion on a converted synthetic scene."""
import importlib
import os

import numpy as np
import pytest

from colmap_common import FIXTURE, angle, check_cams, expected_order, literal_score, parse_pairs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def colmap(pm, engine):
    return importlib.import_module("mp-mvs_amd.colmap")


# ---- kernel against numpy -------------------------------------------------------------------------------------------
def random_model(rng, n, n_points, long_tracks=0, long_len=640):
    """point-major random model -> per-image lists (shuffled, with duplicates and -1 entries); clustered centres put
    many angles under one degree"""
    clusters = rng.normal(0, 4.0, (max(1, n // 8), 3))
    C = clusters[rng.integers(0, len(clusters), n)] + rng.normal(0, 0.02, (n, 3))
    xyz = rng.normal(0, 1.0, (n_points, 3)) + np.array([0, 0, 30.0])
    lists = [[] for _ in range(n)]
    loners = set(rng.choice(n, max(1, n // 10), replace=False).tolist()) if n > 2 else set()
    others = np.array([i for i in range(n) if i not in loners] or list(range(n)))
    for p in range(n_points):
        if p < long_tracks:
            sees = rng.choice(n, long_len, replace=n < long_len)
        else:
            sees = rng.choice(others, min(len(others), int(rng.integers(1, 9))), replace=False)
        for i in sees:
            lists[int(i)].append(p)
            if rng.random() < 0.05:   # duplicate entry
                lists[int(i)].append(p)
    extra = n_points
    xyz = np.concatenate([xyz, rng.normal(0, 1.0, (len(loners), 3))])
    for i in loners:   # images that share no point: each sees one point of its own
        lists[i].append(extra)
        extra += 1
    for i in range(n):
        lst = list(rng.permutation(lists[i])) + [-1] * int(rng.integers(0, 4))
        lists[i] = list(rng.permutation(lst))
    off = np.cumsum([0] + [len(l) for l in lists]).astype(np.int64)
    pts = np.array(sum(lists, []), np.int32)
    return C, xyz, off, pts


def numpy_counts(C, xyz, off, pts):
    """shared / small (upper triangle) by pair events per point: for each point, its distinct images a < b, adding
    the multiplicity of a"""
    n = len(C)
    img = np.repeat(np.arange(n), np.diff(off))
    keep = pts >= 0
    img, pt = img[keep], pts[keep].astype(np.int64)
    key, mult = np.unique(pt * n + img, return_counts=True)
    p, im = key // n, key % n
    starts = np.flatnonzero(np.r_[True, p[1:] != p[:-1]])
    ends = np.r_[starts[1:], len(p)]
    A, B, M, P = [], [], [], []
    for s, e in zip(starts, ends):
        L = e - s
        if L < 2:
            continue
        ia, ib = np.triu_indices(L, 1)
        A.append(im[s + ia]), B.append(im[s + ib]), M.append(mult[s + ia]), P.append(np.full(len(ia), p[s]))
    shared = np.zeros((n, n), np.uint64)
    small = np.zeros((n, n), np.uint64)
    if A:
        A, B, M, P = (np.concatenate(v) for v in (A, B, M, P))
        th = angle(C[A], C[B], xyz[P])
        np.add.at(shared, (A, B), M.astype(np.uint64))
        np.add.at(small, (A, B), (M * (th < 1)).astype(np.uint64))
    return shared, small


def rule_selection(shared, small, num_view):
    S = np.where((shared == 0) | (small >= (3 * shared) // 4 + 1), 0, shared).astype(np.int64)
    S = S + S.T
    ids = np.array([expected_order(S[i], num_view) for i in range(len(S))]).reshape(len(S), num_view)
    return ids, np.take_along_axis(S, ids, 1)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 300, 2500])
def test_view_select_matches_numpy(colmap, n):
    rng = np.random.default_rng(1000 + n)
    n_points = {1: 20, 2: 40}.get(n, 3 * n)
    C, xyz, off, pts = random_model(rng, n, n_points, long_tracks=3 if n >= 64 else 0)
    num_view = n if n <= 2 else min(20, n - 1)
    ids, sc, sh, sm = colmap.view_select(C, xyz, off, pts, num_view, counts=True)
    esh, esm = numpy_counts(C, xyz, off, pts)
    assert np.array_equal(sh.astype(np.uint64), esh) and np.array_equal(sm.astype(np.uint64), esm)
    if n >= 64:
        lens = np.bincount(pts[pts >= 0])
        assert lens.max() >= 600 and (sm > 0).any() and ((sh > 0) & (sm == 0)).any()
        assert (np.tril(sh) == 0).all()
    eids, esc = rule_selection(esh, esm, num_view)
    assert np.array_equal(ids, eids) and np.array_equal(sc, esc)
    ids2, sc2, sh2, sm2 = colmap.view_select(C, xyz, off, pts, num_view, counts=True)
    assert ids2.tobytes() == ids.tobytes() and sc2.tobytes() == sc.tobytes() and sh2.tobytes() == sh.tobytes() and sm2.tobytes() == sm.tobytes()


# point counts at the edges of the track-offset scan (pm_scan.hpp, tiles of 256): the last partial tile, one full tile, one
# point into the next, and 256 * 256 + 1 = one tile of tile totals into the second round of the totals scan
@pytest.mark.parametrize("n_points", [255, 256, 257, 65537])
def test_view_select_at_scan_edges(colmap, n_points):
    """64 images, every point seen by exactly two distinct images: the pair list is the model itself"""
    n, num_view = 64, 20
    rng = np.random.default_rng(2000 + n_points)
    clusters = rng.normal(0, 4.0, (8, 3))
    C = clusters[rng.integers(0, 8, n)] + rng.normal(0, 0.02, (n, 3))
    xyz = rng.normal(0, 1.0, (n_points, 3)) + np.array([0, 0, 30.0])
    a = rng.integers(0, n, n_points)
    b = (a + rng.integers(1, n, n_points)) % n
    a, b = np.minimum(a, b), np.maximum(a, b)
    # per-image lists in a shuffled order
    img, pt = np.concatenate([a, b]), np.tile(np.arange(n_points, dtype=np.int32), 2)
    order = rng.permutation(2 * n_points)
    order = order[np.argsort(img[order], kind="stable")]
    off = np.concatenate([[0], np.cumsum(np.bincount(img, minlength=n))]).astype(np.int64)
    pts = np.ascontiguousarray(pt[order])
    ids, sc, sh, sm = colmap.view_select(C, xyz, off, pts, num_view, counts=True)
    esh = np.zeros((n, n), np.uint64)
    esm = np.zeros((n, n), np.uint64)
    np.add.at(esh, (a, b), np.uint64(1))
    np.add.at(esm, (a, b), (angle(C[a], C[b], xyz) < 1).astype(np.uint64))
    assert esh.sum() == n_points and esm.any() and ((esh > 0) & (esm == 0)).any()
    assert np.array_equal(sh.astype(np.uint64), esh) and np.array_equal(sm.astype(np.uint64), esm)
    eids, esc = rule_selection(esh, esm, num_view)
    assert np.array_equal(ids, eids) and np.array_equal(sc, esc)


def test_view_select_argument_errors(engine):
    _, fns = engine.load()
    C = np.zeros((4, 3))
    xyz = np.zeros((2, 3))
    off = np.array([0, 1, 2, 3, 4], np.int64)
    pts = np.array([0, 1, 0, -1], np.int32)
    ids = np.zeros(64, np.int32)
    sc = np.zeros(64, np.int32)
    call = lambda n=4, c=C.ctypes.data, o=off.ctypes.data, p=pts.ctypes.data, nv=3, out=ids.ctypes.data, np_=2: fns["view_select"](
        0, n, c, np_, xyz.ctypes.data, o, p, nv, out, sc.ctypes.data, None, None)
    assert call() == 0
    assert call(c=None) == -1 and call(o=None) == -1 and call(p=None) == -1 and call(out=None) == -1
    assert call(nv=5) == -1 and call(nv=-1) == -1 and call(n=0) == -1
    assert call(np_=1) == -1   # point index 1 out of range
    bad = np.array([0, 2, 1, 3, 4], np.int64)
    assert call(o=bad.ctypes.data) == -1
    assert call(n=32769) == -2


# ---- fixture end to end ---------------------------------------------------------------------------------------------
def compare_pairs(got, exp):
    gi, gs = parse_pairs(got)
    ei, es = parse_pairs(exp)
    assert gi.shape == ei.shape
    for i in range(len(gi)):
        assert np.array_equal(gs[i], es[i]), i
        for s in np.unique(es[i]):
            g, e = set(gi[i][gs[i] == s]), set(ei[i][es[i] == s])
            if s == es[i][-1]:   # the cut-off group: the ids chosen from the tie
                assert g <= set(np.flatnonzero(_full_row_scores(exp, i) == s)), (i, s)
            else:
                assert g == e, (i, s)


_rows = {}


def _full_row_scores(exp, i):
    """every image's score in row i, from the recorded model (the cut-off group may continue past the list)"""
    if exp not in _rows:
        colmap = importlib.import_module("mp-mvs_amd.colmap")
        m = colmap.read_model(os.path.join(FIXTURE, "sparse"), ".txt")
        C = colmap.centers(m)
        lists = [m.obs_pt[m.obs_off[k]:m.obs_off[k + 1]] for k in range(m.n_images)]
        S = np.zeros((m.n_images, m.n_images), np.int64)
        for a in range(m.n_images):
            for b in range(a + 1, m.n_images):
                S[a, b] = S[b, a] = literal_score(lists[a], lists[b], C[a], C[b], m.xyz)
        _rows[exp] = S
    return _rows[exp][i]


@pytest.mark.parametrize("ext", [".txt", ".bin"])
@pytest.mark.parametrize("max_d", [192, 0])
def test_convert_fixture(colmap, tmp_path, ext, max_d):
    out = tmp_path / "out"
    times = colmap.convert(FIXTURE, out, max_d=max_d, model_ext=ext)
    assert set(times) == {"read", "select", "cams", "pairs", "images"}
    exp = os.path.join(FIXTURE, "expected_d%d" % max_d)
    compare_pairs(str(out / "pair.txt"), os.path.join(exp, "pair.txt"))
    check_cams(out / "cams", os.path.join(exp, "cams"), 14)
    assert sorted(os.listdir(out / "images")) == ["%08d.jpg" % i for i in range(14)]
    with pytest.raises(FileExistsError):
        colmap.convert(FIXTURE, out, max_d=max_d, model_ext=ext)
    colmap.convert(FIXTURE, out, max_d=max_d, model_ext=ext, overwrite=True)


# ---- PatchMatch on a converted synthetic scene ----------------------------------------------------------------------
def rotmat2qvec(R):
    w = np.sqrt(max(0.0, 1.0 + np.trace(R))) / 2
    q = np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])
    return q / np.linalg.norm(q)


def export_colmap(sc, dense, stride=3):
    """the scene as a COLMAP dense folder: one PINHOLE camera per view, PNG images, points = GT-depth back-projections
    observed where they project inside a view and agree with that view's GT depth (1 %)"""
    from PIL import Image
    os.makedirs(os.path.join(dense, "images"))
    os.makedirs(os.path.join(dense, "sparse"))
    H, W = sc.views[0].image.shape
    ids = [10 + 7 * i for i in range(len(sc.views))]
    obs = [[] for _ in sc.views]
    pts = []
    for i, v in enumerate(sc.views):
        uu, vv = np.meshgrid(np.arange(1, W - 1, stride, dtype=np.float64), np.arange(1, H - 1, stride, dtype=np.float64))
        d = v.gt_depth[vv.astype(int), uu.astype(int)].astype(np.float64)
        ray = np.stack([(uu - v.K[0, 2]) / v.K[0, 0], (vv - v.K[1, 2]) / v.K[1, 1], np.ones_like(uu)], -1) * d[..., None]
        X = (ray.reshape(-1, 3) - 0) @ v.R + v.C   # R^T (d K^-1 x) + C
        for x in X:
            seen = []
            for j, w in enumerate(sc.views):
                pc = w.R @ (x - w.C)
                if pc[2] <= 0:
                    continue
                u, q = w.K[0, 0] * pc[0] / pc[2] + w.K[0, 2], w.K[1, 1] * pc[1] / pc[2] + w.K[1, 2]
                iu, iq = int(round(u)), int(round(q))
                if 0 <= iu < W and 0 <= iq < H and abs(w.gt_depth[iq, iu] - pc[2]) < 0.01 * pc[2]:
                    seen.append((j, u, q))
            if len(seen) >= 2:
                for j, u, q in seen:
                    obs[j].append((u, q, len(pts)))
                pts.append(x)
    with open(os.path.join(dense, "sparse", "cameras.txt"), "w") as f:
        for i, v in enumerate(sc.views):
            f.write("%d PINHOLE %d %d %r %r %r %r\n" % (i + 1, W, H, *(float(k) for k in (v.K[0, 0], v.K[1, 1], v.K[0, 2], v.K[1, 2]))))
    with open(os.path.join(dense, "sparse", "images.txt"), "w") as f:
        for i, v in enumerate(sc.views):
            q = rotmat2qvec(v.R)
            t = -v.R @ v.C
            name = "view_%d.png" % i
            f.write("%d %s %s %d %s\n" % (ids[i], " ".join(repr(float(x)) for x in q), " ".join(repr(float(x)) for x in t), i + 1, name))
            f.write(" ".join("%r %r %d" % (float(u), float(q_), k + 1) for u, q_, k in obs[i]) + "\n")
            Image.fromarray(v.image.astype(np.uint8)).save(os.path.join(dense, "images", name))
    with open(os.path.join(dense, "sparse", "points3D.txt"), "w") as f:
        for k, x in enumerate(pts):
            f.write("%d %r %r %r 0 0 0 0.5\n" % (k + 1, *(float(c) for c in x)))
    return len(pts)


def _gt_fraction(hostlib, folder, sc):
    fr = []
    for i, v in enumerate(sc.views):
        d = hostlib.read_dmb(os.path.join(folder, "MPMVS", "2333_%08d" % i, "depths.dmb"))
        fr.append(np.abs(d - v.gt_depth) / v.gt_depth < 0.05)
    return float(np.mean(fr))


def test_patchmatch_on_converted_scene(pm, colmap, hostlib, tmp_path):
    sc, neigh = pm.synth.make_grid_scene(64, 48, 3, 2, spacing=0.5, rot_deg=1.0, quantize=True)
    direct = tmp_path / "direct"
    hostlib.write_dataset(str(direct), [v.cam for v in sc.views], [v.image for v in sc.views], neigh)
    dense, conv = tmp_path / "dense", tmp_path / "conv"
    assert export_colmap(sc, str(dense)) > 500
    colmap.convert(str(dense), str(conv))
    assert sorted(os.listdir(conv / "images")) == ["%08d.pgm" % i for i in range(6)]
    for i, v in enumerate(sc.views):   # lossless: the pixels the direct folder holds
        assert np.array_equal(hostlib.read_pgm(conv / "images" / ("%08d.pgm" % i)), v.image)
    lst = hostlib.sample_list(conv)
    assert all(len(src) == 6 for _, _, src in lst)   # every other view shares points with a score
    kw = dict(device=0, geom_iterations=1, planar_prior=True, geom_planar_prior=True, max_scale=1, seed=4242)
    hostlib.run_folder(direct, **kw)
    hostlib.run_folder(conv, **kw)
    f_direct, f_conv = _gt_fraction(hostlib, direct, sc), _gt_fraction(hostlib, conv, sc)
    print(f"within 5 % of GT depth: direct {f_direct:.4f}, converted {f_conv:.4f}")
    assert f_conv >= f_direct - 0.02
    n = hostlib.fuse_folder(conv, device=0)
    assert n > 0 and os.path.getsize(conv / "MPMVS" / "MPMVS_model.ply") > 0
