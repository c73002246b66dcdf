"""The plain statements of mpmvs_cloud_components and of cloud.remove_small_clusters (include/mpmvs.h) in
numpy, shared by test_components_cpu.py and test_components_gpu.py.  Adjacency is fp32 per operation in the order the contract
states, chunked as in knn_common.brute_knn (numpy does not fuse); the components come from a plain Python union-find over the
np.nonzero edges."""
import numpy as np


def adjacent_pairs(xyz, radius, chunk=512):
    """(i, j) int64 arrays of all adjacent pairs with j < i: both points finite and d2 = (dx*dx + dy*dy) + dz*dz <= r2 in fp32"""
    x = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    r2 = np.float32(radius) * np.float32(radius)
    ok = np.isfinite(x).all(1)
    ii, jj = [], []
    with np.errstate(all="ignore"):
        for b in range(0, len(x), chunk):
            q = x[b:b + chunk]
            dx = q[:, None, 0] - x[None, :, 0]
            dy = q[:, None, 1] - x[None, :, 1]
            dz = q[:, None, 2] - x[None, :, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == np.float32
            adj = (d2 <= r2) & ok[None, :] & ok[b:b + chunk, None]
            i, j = np.nonzero(adj)
            i = i + b
            lower = j < i
            ii.append(i[lower])
            jj.append(j[lower])
    return (np.concatenate(ii), np.concatenate(jj)) if ii else (np.zeros(0, np.int64), np.zeros(0, np.int64))


def statement_components(xyz, radius):
    """(label int32 [n], size int32 [n], counts int64 [4]) as Cloud.components"""
    x = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = len(x)
    ok = np.isfinite(x).all(1)
    up = list(range(n))

    def root(v):
        while up[v] != v:
            up[v] = up[up[v]]
            v = up[v]
        return v

    for i, j in zip(*(a.tolist() for a in adjacent_pairs(x, radius))):
        a, b = root(i), root(j)
        if a != b:
            up[max(a, b)] = min(a, b)   # the smaller root stays: a root is the smallest index of its set
    label = np.array([root(i) if ok[i] else -1 for i in range(n)], np.int32).reshape(n)
    members = np.bincount(label[ok], minlength=max(n, 1))
    size = np.where(ok, members[np.maximum(label, 0)], 0).astype(np.int32)
    roots = np.flatnonzero(label == np.arange(n))
    counts = np.array([int(ok.sum()), len(roots), 0, -1], np.int64)
    if len(roots):
        best = roots[np.argmax(size[roots])]   # argmax returns the first of equals: the smallest label
        counts[2], counts[3] = size[best], best
    return label, size, counts


def statement_small_clusters(xyz, radius, min_size=2, largest=None):
    """-> {"keep", "label", "size", "counts"} as cloud.remove_small_clusters, the keep rule written as a loop"""
    label, size, counts = statement_components(xyz, radius)
    n = len(label)
    comps = sorted((-int(size[r]), int(r)) for r in range(n) if label[r] == r)   # by size descending, then label ascending
    allowed = {r for _, r in (comps if largest is None else comps[:largest])}
    keep = np.array([label[i] >= 0 and size[i] >= min_size and int(label[i]) in allowed for i in range(n)], bool).reshape(n)
    return {"keep": keep, "label": label, "size": size, "counts": counts}


def assert_components_same(got, want, what=""):
    """array_equal on label, size (where `got` holds one) and counts; no tolerance"""
    for name, g, w in zip(("label", "size", "counts"), got, want):
        if g is None:
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what} {name}: {g.dtype} {g.shape} against {w.dtype} {w.shape}"
        bad = g != w
        assert not bad.any(), f"{what} {name}: {int(bad.sum())} of {len(w)} differ; first at {np.flatnonzero(bad)[0]}: {g[bad][0]} against {w[bad][0]}"


def cluster_scene():
    """(xyz float32 shuffled, plane bool, blob bool): knn_common.property_scene()'s plane, flying points and far point, plus three
    blobs of 40 points each 0.2 above the plane -- the detached clusters the outlier rules keep"""
    from knn_common import property_scene
    x, plane = property_scene()
    rng = np.random.default_rng(23)
    blobs = np.concatenate([np.array([cx, cy, 0.2]) + rng.uniform(-0.012, 0.012, (40, 3)) for cx, cy in ((0.08, 0.1), (0.2, 0.3), (0.33, 0.12))])
    x = np.concatenate([x, blobs.astype(np.float32)])
    is_plane = np.concatenate([plane, np.zeros(120, bool)])
    is_blob = np.arange(len(x)) >= len(plane)
    perm = rng.permutation(len(x))
    return x[perm], is_plane[perm], is_blob[perm]
