"""The plain statement of mpmvs_cloud_voxel_downsample (include/mpmvs.h) in numpy: fp64 floor, np.rint (round to nearest even),
int64 np.add.at, the voxels numbered by np.unique and a stable sort on the first member index.  Shared by test_voxel_cpu.py and
test_voxel_gpu.py; assert_same compares the bits of every output array."""
import numpy as np

AXIS_CELLS = 1 << 21
FIX = float(1 << 30)


def statement(xyz, voxel, normals=None, colors=None):
    """-> {"xyz", "count", "first", "voxel_of"} plus "normals" / "colors" when given, as cloud.voxel_downsample(want_map=True)"""
    x = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = len(x)
    e = float(np.float32(voxel))
    ok = np.isfinite(x).all(1)
    idx = np.flatnonzero(ok)
    out = {"voxel_of": np.full(n, -1, np.int32)}
    if len(idx) == 0:
        out.update(xyz=np.empty((0, 3), np.float32), count=np.empty(0, np.int32), first=np.empty(0, np.int32))
        if normals is not None:
            out["normals"] = np.empty((0, 3), np.float32)
        if colors is not None:
            out["colors"] = np.empty((0, 3), np.uint8)
        return out
    p = x[idx]
    mn = p.min(0)                                   # fp32
    o = mn.astype(np.float64) - 0.5 * e
    t = (p.astype(np.float64) - o) / e
    c = np.floor(t)
    assert (c >= 0).all() and (c < AXIS_CELLS).all(), "the statement's cell-span limit"
    ci = c.astype(np.int64)
    key = ci[:, 0] | (ci[:, 1] << 21) | (ci[:, 2] << 42)
    _, first_pos, inv, count = np.unique(key, return_index=True, return_inverse=True, return_counts=True)   # first_pos: the first occurrence
    order = np.argsort(first_pos, kind="stable")    # voxels by first appearance
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    v = rank[inv.reshape(-1)]
    m = len(order)
    out["voxel_of"][idx] = v.astype(np.int32)
    out["first"] = idx[first_pos[order]].astype(np.int32)
    cnt = count[order].astype(np.int64)
    out["count"] = cnt.astype(np.int32)
    S = np.zeros((m, 3), np.int64)
    np.add.at(S, v, np.rint((t - c) * FIX).astype(np.int64))
    cv = c[first_pos[order]]                        # the cell of every voxel
    den = cnt.astype(np.float64)[:, None] * FIX
    out["xyz"] = (o + (cv + S.astype(np.float64) / den) * e).astype(np.float32)
    if normals is not None:
        nr = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)[idx]
        good = np.isfinite(nr).all(1)
        N = np.zeros((m, 3), np.int64)
        np.add.at(N, v[good], np.rint(np.clip(nr[good].astype(np.float64), -1.0, 1.0) * FIX).astype(np.int64))
        Nd = N.astype(np.float64)
        L = np.sqrt((Nd[:, 0] * Nd[:, 0] + Nd[:, 1] * Nd[:, 1]) + Nd[:, 2] * Nd[:, 2])
        res = np.zeros((m, 3), np.float32)
        nz = L != 0
        res[nz] = (Nd[nz] / L[nz, None]).astype(np.float32)
        out["normals"] = res
    if colors is not None:
        col = np.ascontiguousarray(colors, np.uint8).reshape(-1, 3)[idx]
        Cs = np.zeros((m, 3), np.int64)
        np.add.at(Cs, v, col.astype(np.int64))
        out["colors"] = ((2 * Cs + cnt[:, None]) // (2 * cnt[:, None])).astype(np.uint8)
    return out


def assert_same(got, want, what=""):
    """every array of `want` that `got` should hold, compared by shape, dtype and bits"""
    for k, w in want.items():
        if k == "voxel_of" and k not in got:
            continue
        assert k in got, f"{what}: no {k!r} in the result"
        g = got[k]
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what} {k}: {g.dtype} {g.shape} against {w.dtype} {w.shape}"
        gb, wb = np.ascontiguousarray(g).view(np.uint8), np.ascontiguousarray(w).view(np.uint8)
        if not np.array_equal(gb, wb):
            bad = np.flatnonzero((gb.reshape(len(g), -1) != wb.reshape(len(w), -1)).any(1))
            raise AssertionError(f"{what} {k}: {len(bad)} of {len(g)} rows differ in bits; first at {bad[0]}: {g[bad[0]]!r} against {w[bad[0]]!r}")
    for k in got:
        assert k in want, f"{what}: unexpected {k!r} in the result"
