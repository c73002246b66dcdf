"""mpmvs_cloud_voxel_downsample without a GPU: the symbols, every error found before the device is touched, the empty results,
the numpy statement of voxel_common.py against exact rational arithmetic, and evaluate() leaving the entry point alone unless
it is asked for a voxel size."""
import ctypes as C
import importlib
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from voxel_common import statement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mpmvs_cloud_voxel_downsample", "mpmvs_cloud_voxel_ms", "mpmvs_cloud_voxel_pass_ms")


@pytest.fixture(scope="module")
def eng(pm):
    return importlib.import_module("mp-mvs_amd.engine")


@pytest.fixture(scope="module")
def cloud(pm):
    return importlib.import_module("mp-mvs_amd.cloud")


def test_symbols_declared_exported_and_bound(eng):
    header = open(os.path.join(ROOT, "include", "mpmvs.h")).read()
    declared = set(re.findall(r"\b(mpmvs_[a-z0-9_]+)\s*\(", header))
    lib, fns = eng.load()
    lib_q8, fns_q8 = eng.load_variant(eng.LIB_Q8_PATH)
    for name in NEW:
        assert name in declared and name in eng.ALL_SYMBOLS
        assert hasattr(lib, name) and hasattr(lib_q8, name)
        assert name[len("mpmvs_"):] in fns and name[len("mpmvs_"):] in fns_q8
    assert fns["cloud_voxel_downsample"].restype is C.c_longlong and len(fns["cloud_voxel_downsample"].argtypes) == 12
    # the library follows the header: the cloud unit includes it, and the objects depend on what they include (generated dependencies)
    csrc = os.path.join(ROOT, "mp-mvs_amd", "csrc")
    assert '#include "pm_voxel.hpp"' in open(os.path.join(csrc, "mpmvs_cloud.hip")).read()
    makefile = open(os.path.join(csrc, "Makefile")).read()
    assert "mpmvs_cloud" in makefile and "-MMD" in makefile and "-include $(OBJS:.o=.d)" in makefile


class Call:
    """the raw entry point with sentinel out pointers, so that "set to NULL" shows"""

    def __init__(self, fns):
        self.f = fns
        self.p = [C.c_void_p(0xdead0) for _ in range(5)]

    def __call__(self, n, xyz, voxel, normals=None, rgb=None, out=(True, None, None, True, True), vmap=None, device=0):
        outs = []
        for k, want in enumerate(out):
            if want is None:
                want = (k == 1 and normals is not None) or (k == 2 and rgb is not None)
            outs.append(C.byref(self.p[k]) if want else None)
        ptr = lambda a: a.ctypes.data if a is not None else None
        return self.f["cloud_voxel_downsample"](device, n, ptr(xyz), ptr(normals), ptr(rgb), voxel, *outs, ptr(vmap))

    def error(self):
        msg = self.f["last_error"](None)
        return msg.decode() if msg else ""


def test_bad_arguments_are_minus_2_without_a_device(eng):
    _, fns = eng.load()
    x = np.zeros((4, 3), np.float32)
    nr = np.zeros((4, 3), np.float32)
    col = np.zeros((4, 3), np.uint8)
    call = Call(fns)
    assert call(4, None, 0.1) == -2                                   # NULL xyz with n > 0
    assert call(-1, x, 0.1) == -2                                     # negative n
    for v in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert call(4, x, v) == -2, v
        assert "voxel" in call.error()
    for k in (0, 3, 4):                                               # NULL out_xyz, out_count, out_first
        out = [True, None, None, True, True]
        out[k] = False
        assert call(4, x, 0.1, out=tuple(out)) == -2, k
    assert call(4, x, 0.1, normals=nr, out=(True, False, None, True, True)) == -2
    assert call(4, x, 0.1, rgb=col, out=(True, None, False, True, True)) == -2
    # a bad device is not looked at before the arguments are
    assert call(4, None, 0.1, device=12345) == -2


def test_limits_are_minus_3_without_a_device(eng):
    _, fns = eng.load()
    call = Call(fns)
    x = np.zeros((2, 3), np.float32)
    assert call((1 << 31), x, 0.1) == -3 and "2^31" in call.error()   # refused on the count alone: the array is not read
    for k in (0, 3, 4):
        assert call.p[k].value is None                                # a failure leaves every out pointer it was given NULL
    # the cell-span limit: the lowest point sits at the centre of cell 0, so a point 2^21 voxels above it falls into cell 2^21
    y = np.zeros((2, 3), np.float32)
    y[1] = float((1 << 21) - 1)
    assert call(2, y, 1.0, device=12345) == -100                      # the last cell that fits: accepted, and only then is the device looked for
    for axis in range(3):
        x = np.zeros((3, 3), np.float32)
        x[1, axis] = float((1 << 21))
        x[2] = np.nan
        assert call(3, x, 1.0) == -3
        text = call.error()
        assert "along " + "xyz"[axis] in text and "2^21" in text and "extent / voxel = " in text, text
        assert f"{float(1 << 21):.6g}" in text, text                 # the ratio
        for k in (0, 3, 4):
            assert call.p[k].value is None


def test_more_than_2_pow_29_finite_points_is_minus_3_without_a_device(eng):
    """the table's limit.  The input is 6 GiB of zeros that are never written: a read-only anonymous mapping, every page of which
    is the kernel's zero page, so the test takes address space and the host's pass over the points (about 3 s), not memory."""
    import mmap
    _, fns = eng.load()
    n = (1 << 29) + 1
    MAP_NORESERVE = getattr(mmap, "MAP_NORESERVE", 0x4000)
    mm = mmap.mmap(-1, n * 12, flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS | MAP_NORESERVE, prot=mmap.PROT_READ)
    try:
        x = np.frombuffer(mm, np.float32)
        call = Call(fns)
        assert call(n, x, 1.0, device=12345) == -3 and "2^29" in call.error()
        assert all(call.p[k].value is None for k in (0, 3, 4))
        del x
    finally:
        mm.close()


def test_empty_results_need_no_device(eng, cloud):
    _, fns = eng.load()
    call = Call(fns)
    assert call(0, None, 0.5) == 0
    assert all(p.value is None for p in call.p[:1] + call.p[3:])
    call = Call(fns)
    x = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan] * 3], np.float32)
    vmap = np.full(4, 7, np.int32)
    nr = np.ones((4, 3), np.float32)
    col = np.ones((4, 3), np.uint8)
    assert call(4, x, 0.5, normals=nr, rgb=col, vmap=vmap, device=12345) == 0
    assert all(p.value is None for p in call.p)
    assert (vmap == -1).all()
    assert fns["cloud_voxel_ms"]() == 0.0
    r = cloud.voxel_downsample(x, 0.5, normals=nr, colors=col, want_map=True)
    assert r["xyz"].shape == (0, 3) and r["normals"].shape == (0, 3) and r["colors"].shape == (0, 3) and r["colors"].dtype == np.uint8
    assert r["count"].shape == (0,) and r["first"].shape == (0,) and (r["voxel_of"] == -1).all()
    assert cloud.last_voxel_ms() == 0.0
    with pytest.raises(ValueError, match="finite and positive"):
        cloud.voxel_downsample(np.zeros((1, 3), np.float32), -1.0)


# ---- the statement against exact arithmetic ---------------------------------------------------------------------------------
def _rn(q):
    """the fp64 nearest (ties to even) to the rational q: int / int true division is correctly rounded"""
    q = Fraction(q)
    return q.numerator / q.denominator


def _fix(q):
    return round(Fraction(q) * (1 << 30))   # round() of a Fraction: ties to even


def _exact_sqrt(d):
    r = math.sqrt(d)
    if d > 0:   # r is the fp64 nearest to the root: d lies between the squares of the midpoints to r's neighbours
        lo, hi = (Fraction(r) + Fraction(math.nextafter(r, 0.0))) / 2, (Fraction(r) + Fraction(math.nextafter(r, math.inf))) / 2
        assert lo * lo <= Fraction(d) <= hi * hi
    return r


def exact_statement(x, voxel, normals, colors):
    """the contract of include/mpmvs.h point by point, every fp64 operation as the correctly rounded exact result"""
    e = float(np.float32(voxel))
    part = [i for i in range(len(x)) if all(math.isfinite(float(v)) for v in x[i])]
    mn = [min(float(x[i][a]) for i in part) for a in range(3)]
    o = [_rn(Fraction(mn[a]) - Fraction(e) / 2) for a in range(3)]   # 0.5 * e is exact
    cells, vox = {}, []
    voxel_of = [-1] * len(x)
    for i in part:
        t = [_rn(Fraction(_rn(Fraction(float(x[i][a])) - Fraction(o[a]))) / Fraction(e)) for a in range(3)]
        c = tuple(math.floor(Fraction(ta)) for ta in t)
        if c not in cells:
            cells[c] = len(vox)
            vox.append({"c": c, "first": i, "count": 0, "S": [0, 0, 0], "N": [0, 0, 0], "C": [0, 0, 0]})
        v = vox[cells[c]]
        voxel_of[i] = cells[c]
        v["count"] += 1
        for a in range(3):
            v["S"][a] += _fix(Fraction(t[a]) - c[a])   # t - floor(t) is exact in fp64
        nr = [float(k) for k in normals[i]]
        if all(math.isfinite(k) for k in nr):
            for a in range(3):
                v["N"][a] += _fix(max(-1.0, min(1.0, nr[a])))
        for k in range(3):
            v["C"][k] += int(colors[i][k])
    out = {"xyz": [], "normals": [], "colors": [], "count": [v["count"] for v in vox], "first": [v["first"] for v in vox], "voxel_of": voxel_of}
    for v in vox:
        den = _rn(Fraction(v["count"]) * (1 << 30))
        pos = []
        for a in range(3):
            mean = _rn(Fraction(_rn(v["S"][a])) / Fraction(den))
            inner = _rn(Fraction(float(v["c"][a])) + Fraction(mean))
            pos.append(np.float32(_rn(Fraction(o[a]) + Fraction(_rn(Fraction(inner) * Fraction(e))))))
        out["xyz"].append(pos)
        N = [_rn(k) for k in v["N"]]
        sq = [_rn(Fraction(k) * Fraction(k)) for k in N]
        L = _exact_sqrt(_rn(Fraction(_rn(Fraction(sq[0]) + Fraction(sq[1]))) + Fraction(sq[2])))
        out["normals"].append([np.float32(0.0) if L == 0 else np.float32(_rn(Fraction(k) / Fraction(L))) for k in N])
        out["colors"].append([(2 * k + v["count"]) // (2 * v["count"]) for k in v["C"]])
    return out


def test_statement_equals_exact_arithmetic_on_50_points():
    rng = np.random.default_rng(16)
    x = (rng.random((50, 3)) * 1.5 + 1000.0).astype(np.float32)
    x[10:20] = x[0:10]                     # duplicates
    x[20:25] = x[0] + np.float32(0.01) * rng.random((5, 3)).astype(np.float32)
    x[7] = [np.nan, 1, 2]
    x[33, 2] = np.inf
    nr = rng.normal(size=(50, 3)).astype(np.float32)
    nr /= np.linalg.norm(nr, axis=1, keepdims=True)
    nr[3, 1] = np.nan
    nr[12] = -nr[2]                        # x[12] == x[2]: opposite normals in one voxel
    nr[40] *= 3                            # components beyond +-1 are clamped
    col = rng.integers(0, 256, (50, 3), dtype=np.uint8)
    voxel = 0.3
    got = statement(x, voxel, nr, col)
    want = exact_statement(x, voxel, nr, col)
    assert 20 < len(want["count"]) < 50
    assert got["count"].tolist() == want["count"] and got["first"].tolist() == want["first"] and got["voxel_of"].tolist() == want["voxel_of"]
    assert got["colors"].tolist() == want["colors"]
    assert np.array_equal(got["xyz"].view(np.uint32), np.array(want["xyz"], np.float32).view(np.uint32))
    assert np.array_equal(got["normals"].view(np.uint32), np.array(want["normals"], np.float32).view(np.uint32))
    # the centroid is the fp64 mean of the members to within half an fp32 ulp plus the 2^-31 voxel of the fixed point
    for v in range(len(want["count"])):
        mem = x[np.array(want["voxel_of"]) == v].astype(np.float64)
        assert np.all(np.abs(got["xyz"][v].astype(np.float64) - mem.mean(0)) <= 0.5 * np.spacing(np.float32(1001.5)) + voxel * 2.0 ** -30)


def test_statement_border_rule():
    """the origin is mn - voxel / 2: mn sits at the centre of cell 0, mn + (k + 1/2) voxel is the border between the cells k and
    k + 1 and belongs to the upper one, its fp32 neighbour below to the lower one; a point on a cell centre mn + k voxel stays
    with its cell, as do both of its fp32 neighbours"""
    voxel = np.float32(0.25)
    for shift in (np.float32(0.0), np.float32(1000.25)):
        mn = np.float32(2.0) + shift
        k = np.arange(6, dtype=np.float32)
        borders = (mn + (k + np.float32(0.5)) * voxel).astype(np.float32)
        centres = (mn + (k + np.float32(1.0)) * voxel).astype(np.float32)
        below, above = (lambda a: np.nextafter(a, np.float32(-np.inf))), (lambda a: np.nextafter(a, np.float32(np.inf)))
        pts = np.concatenate([[mn], borders, below(borders), above(borders), centres, below(centres), above(centres)]).astype(np.float32)
        x = np.full((len(pts), 3), mn, np.float32)
        x[:, 0] = pts
        cell = statement(x, voxel)["voxel_of"]
        assert cell[0] == 0 and list(cell[1:7]) == [1, 2, 3, 4, 5, 6]
        assert list(cell[7:13]) == [0, 1, 2, 3, 4, 5] and list(cell[13:19]) == [1, 2, 3, 4, 5, 6]
        assert list(cell[19:25]) == list(cell[25:31]) == list(cell[31:37]) == [1, 2, 3, 4, 5, 6]


# ---- evaluate ----------------------------------------------------------------------------------------------------------------
def test_evaluate_without_voxel_never_calls_the_entry_point(eng, cloud, monkeypatch):
    _, fns = eng.load()
    calls = []

    def fake(device, n, *rest):
        calls.append(n)
        return 0   # "no occupied voxel": every out pointer stays NULL

    class FakeCloud:
        def __init__(self, xyz, device=0):
            self.n = len(xyz)

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            pass

    monkeypatch.setitem(fns, "cloud_voxel_downsample", fake)
    monkeypatch.setattr(cloud, "Cloud", FakeCloud)
    monkeypatch.setattr(cloud, "distances", lambda q, c, tol, on_level=None: np.zeros(len(q), np.float32))
    a, b = np.zeros((5, 3), np.float32), np.ones((7, 3), np.float32)
    res = cloud.evaluate(a, b, [0.1])
    assert calls == []
    assert res["n_reconstruction"] == 5 and res["n_ground_truth"] == 7
    assert not {"voxel", "n_reconstruction_in", "n_ground_truth_in"} & set(res)
    res = cloud.evaluate(a, b, [0.1], voxel=0.5)
    assert calls == [5, 7]
    assert (res["voxel"], res["n_reconstruction_in"], res["n_ground_truth_in"]) == (0.5, 5, 7) and res["n_reconstruction"] == 0
    with pytest.raises(ValueError):
        cloud.evaluate(a, b, [0.1], voxel=0.0)
