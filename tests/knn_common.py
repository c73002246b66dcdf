"""The brute-force statements of mpmvs_cloud_knn and mpmvs_cloud_outliers (include/mpmvs.h) in numpy,
shared by test_knn_cpu.py and test_knn_gpu.py.  The distances are fp32 per operation in the order the contract states, as in
cloud_common.py (numpy does not fuse); the mean and the statistics are fp64, the k square roots added in an explicit loop over j
(np.sum is not sequential)."""
import numpy as np

NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
FIX = float(1 << 30)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def brute_knn(targets, queries, radius, k, chunk=512, self_rows=None):
    """(d2 float32 [n_q, k], idx int32 [n_q, k], within int32 [n_q]): per query the min(k, candidates) smallest keys
    (d2 bits << 32) | index over the finite targets with d2 <= r2, ascending, the rest +inf / -1; within = the number of all
    candidates.  queries=None: the targets themselves, target i not being a candidate of query i (by index); with self_rows (an
    index array) only those rows of that answer."""
    t = np.ascontiguousarray(targets, np.float32).reshape(-1, 3)
    self_mode = queries is None
    own = np.arange(len(t)) if self_rows is None else np.asarray(self_rows, np.int64)
    q = t[own] if self_mode else np.ascontiguousarray(queries, np.float32).reshape(-1, 3)
    r2 = np.float32(radius) * np.float32(radius)
    nq, nt = len(q), len(t)
    d2_out = np.full((nq, k), np.inf, np.float32)
    idx_out = np.full((nq, k), -1, np.int32)
    within = np.zeros(nq, np.int32)
    if nt == 0 or nq == 0:
        return d2_out, idx_out, within
    t_ok = np.isfinite(t).all(1)
    q_ok = np.isfinite(q).all(1)
    index = np.arange(nt, dtype=np.uint64)
    with np.errstate(all="ignore"):
        for b in range(0, nq, chunk):
            qq = q[b:b + chunk]
            dx = qq[:, None, 0] - t[None, :, 0]
            dy = qq[:, None, 1] - t[None, :, 1]
            dz = qq[:, None, 2] - t[None, :, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == np.float32
            cand = (d2 <= r2) & t_ok[None, :] & q_ok[b:b + chunk, None]
            if self_mode:
                cand[np.arange(len(qq)), own[b:b + chunk]] = False
            within[b:b + chunk] = cand.sum(1)
            key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | index[None, :]
            key = np.where(cand, key, NO_KEY)
            kk = min(k, nt)
            if kk < nt:
                key = np.partition(key, kk - 1, axis=1)[:, :kk]
            key = np.sort(key, axis=1)
            found = key != NO_KEY
            d2_out[b:b + chunk, :kk] = np.where(found, (key >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(np.inf))
            idx_out[b:b + chunk, :kk] = np.where(found, (key & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    return d2_out, idx_out, within


def first_k(full, k):
    """the answer for k from the answer for a larger k: the k smallest of the sorted keys are a prefix of the larger list, and
    within does not depend on k"""
    d2, idx, within = full
    return np.ascontiguousarray(d2[:, :k]), np.ascontiguousarray(idx[:, :k]), within


def assert_knn_same(got, want, what=""):
    """array_equal on the d2 bits, on idx and on within, whichever `got` holds; no tolerance"""
    gd, gi = got[0], got[1]
    gw = got[2] if len(got) > 2 else None
    wd, wi, ww = want
    assert gd.shape == wd.shape and gd.dtype == np.float32, f"{what}: d2 {gd.dtype} {gd.shape} against {wd.shape}"
    bad = (bits(gd) != bits(wd)).any(1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {len(wd)} d2 rows differ; first at {np.flatnonzero(bad)[0]}: {gd[bad][0]} against {wd[bad][0]}"
    if gi is not None:
        assert gi.shape == wi.shape and gi.dtype == np.int32
        bad = (gi != wi).any(1)
        assert not bad.any(), f"{what}: {int(bad.sum())} of {len(wi)} idx rows differ; first at {np.flatnonzero(bad)[0]}: {gi[bad][0]} against {wi[bad][0]}"
    if gw is not None:
        assert gw.dtype == np.int32 and np.array_equal(gw, ww), f"{what}: {int((gw != ww).sum())} of {len(ww)} within differ"


def mean_distance(d2, within, k):
    """float32 [n]: (float)(s / k), s the fp64 sum of the k square roots in ascending list order; +inf below k candidates"""
    n = len(d2)
    mean = np.full(n, np.inf, np.float32)
    dense = within >= k
    if dense.any():
        d = d2[dense].astype(np.float64)
        s = np.sqrt(d[:, 0])
        for j in range(1, k):
            s = s + np.sqrt(d[:, j])
        mean[dense] = (s / float(k)).astype(np.float32)
    return mean


def statistics(mean, radius, std_ratio):
    """(c, S1, S2, mu, sigma, T) of the finite entries of `mean`, in the contract's arithmetic"""
    r = float(np.float32(radius))
    fin = np.isfinite(mean)
    c = int(fin.sum())
    a = mean[fin].astype(np.float64) / r
    S1 = int(np.rint(a * FIX).astype(np.int64).sum())
    S2 = int(np.rint((a * a) * FIX).astype(np.int64).sum())
    if c == 0:
        return 0, 0, 0, 0.0, 0.0, 0.0
    den = float(c) * FIX
    mu = float(np.float64(np.int64(S1)) / np.float64(den))
    var = float(np.float64(np.int64(S2)) / np.float64(den) - np.float64(mu) * np.float64(mu))
    sigma = float(np.sqrt(np.float64(max(0.0, var))))
    T = float("inf") if np.isinf(std_ratio) else float((np.float64(mu) + np.float64(std_ratio) * np.float64(sigma)) * np.float64(r))
    return c, S1, S2, mu, sigma, T


def statement_outliers(xyz, radius, k=16, std_ratio=2.0, min_within=0):
    """-> {"keep", "mean_dist", "within", "counts", "stats"} as cloud.remove_outliers"""
    x = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    r = float(np.float32(radius))
    d2, _, within = brute_knn(x, None, radius, k)
    mean = mean_distance(d2, within, k)
    c, _, _, mu, sigma, T = statistics(mean, radius, std_ratio)
    with np.errstate(invalid="ignore"):
        keep = np.isfinite(mean) & (mean.astype(np.float64) <= T) & (within >= min_within)
    finite = int(np.isfinite(x).all(1).sum())
    return {"keep": keep, "mean_dist": mean, "within": within, "counts": np.array([finite, c, int(keep.sum())], np.int64),
            "stats": np.array([mu * r, sigma * r, T], np.float64)}


def assert_outliers_same(got, want, what=""):
    assert set(got) == set(want), f"{what}: {sorted(got)} against {sorted(want)}"
    for key in ("keep", "mean_dist", "within", "counts", "stats"):
        g, w = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what} {key}: {g.dtype} {g.shape} against {w.dtype} {w.shape}"
        same = g.view(np.uint8) == w.view(np.uint8)
        assert same.all(), f"{what} {key}: {int((~same.reshape(len(g), -1).all(1)).sum())} of {len(g)} differ in bits: {g!r} against {w!r}"


def property_scene():
    """(xyz float32 [1661, 3] shuffled, plane bool [1661]): a 40 x 40 plane grid of spacing 0.01 with 0.002 jitter, 60 flying points
    0.03 - 0.23 above it, and one far point"""
    rng = np.random.default_rng(17)
    g = np.arange(40) * 0.01
    plane = np.stack([*np.meshgrid(g, g, indexing="ij"), np.zeros((40, 40))], -1).reshape(-1, 3) + rng.uniform(-0.002, 0.002, (1600, 3))
    fly = np.stack([rng.uniform(0, 0.39, 60), rng.uniform(0, 0.39, 60), rng.uniform(0.03, 0.23, 60)], 1)
    far = np.array([[5.0, 5.0, 5.0]])
    x = np.concatenate([plane, fly, far]).astype(np.float32)
    is_plane = np.arange(len(x)) < 1600
    perm = rng.permutation(len(x))
    return x[perm], is_plane[perm]
