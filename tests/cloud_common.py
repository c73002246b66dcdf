"""The brute-force statement of mpmvs_cloud_nearest (include/mpmvs.h) in numpy fp32, shared by the
cloud tests.  numpy does not fuse, and every operation below is one fp32 operation in the order the contract states."""
import numpy as np


def brute_nearest(targets, queries, radius, chunk=256):
    """(d2 float32 [n_q], idx int32 [n_q]): the smallest d2 <= r2 over the finite targets and the smallest index attaining it;
    inf / -1 where there is none or the query is not finite"""
    t = np.ascontiguousarray(targets, np.float32).reshape(-1, 3)
    q = np.ascontiguousarray(queries, np.float32).reshape(-1, 3)
    r2 = np.float32(radius) * np.float32(radius)
    d2_out = np.full(len(q), np.inf, np.float32)
    idx_out = np.full(len(q), -1, np.int32)
    if len(t) == 0 or len(q) == 0:
        return d2_out, idx_out
    t_ok = np.isfinite(t).all(1)
    q_ok = np.isfinite(q).all(1)
    with np.errstate(all="ignore"):
        for b in range(0, len(q), chunk):
            qq = q[b:b + chunk]
            dx = qq[:, None, 0] - t[None, :, 0]
            dy = qq[:, None, 1] - t[None, :, 1]
            dz = qq[:, None, 2] - t[None, :, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == np.float32
            cand = (d2 <= r2) & t_ok[None, :] & q_ok[b:b + chunk, None]
            d2 = np.where(cand, d2, np.float32(np.inf))
            k = np.argmin(d2, axis=1)   # the first, i.e. smallest, index of the minimum
            any_c = cand.any(1)
            rows = np.arange(len(qq))
            d2_out[b:b + chunk] = np.where(any_c, d2[rows, k], np.float32(np.inf))
            idx_out[b:b + chunk] = np.where(any_c, k, -1)
    return d2_out, idx_out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same(got, want):
    """array_equal on the d2 bits and on idx; no tolerance"""
    (gd, gi), (wd, wi) = got, want
    assert np.array_equal(bits(gd), bits(wd)), f"{int((bits(gd) != bits(wd)).sum())} of {len(wd)} d2 differ"
    if gi is not None:
        assert np.array_equal(gi, wi), f"{int((gi != wi).sum())} of {len(wi)} idx differ"
