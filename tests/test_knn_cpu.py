"""mpmvs_cloud_knn and mpmvs_cloud_outliers without a GPU: the symbols, every error found before the device is touched, the empty
results, and the numpy statement of knn_common.py against exact rational arithmetic."""
import ctypes as C
import importlib
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from knn_common import brute_knn, mean_distance, property_scene, statement_outliers, statistics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mpmvs_cloud_knn", "mpmvs_cloud_knn_ms", "mpmvs_cloud_outliers", "mpmvs_cloud_outliers_ms")


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
    assert fns["cloud_knn"].restype is C.c_int and len(fns["cloud_knn"].argtypes) == 8
    assert fns["cloud_outliers"].restype is C.c_longlong and len(fns["cloud_outliers"].argtypes) == 12
    assert re.search(r"#define\s+MPMVS_KNN_MAX_K\s+32\b", header)
    # the library follows the header: the cloud unit includes it, and the objects depend on what they include (generated dependencies)
    csrc = os.path.join(ROOT, "mp-mvs_amd", "csrc")
    assert '#include "pm_knn.hpp"' in open(os.path.join(csrc, "mpmvs_cloud.hip")).read()
    makefile = open(os.path.join(csrc, "Makefile")).read()
    assert "mpmvs_cloud" in makefile and "-MMD" in makefile and "-include $(OBJS:.o=.d)" in makefile


class Call:
    """the raw mpmvs_cloud_outliers with outputs that show what was written"""

    def __init__(self, fns, n):
        self.f = fns
        self.keep = np.full(max(n, 1), 7, np.uint8)
        self.mean = np.full(max(n, 1), 7.0, np.float32)
        self.within = np.full(max(n, 1), 7, np.int32)
        self.counts = (C.c_longlong * 3)(7, 7, 7)
        self.stats = (C.c_double * 3)(7.0, 7.0, 7.0)

    def __call__(self, n, xyz, radius=0.1, k=4, std_ratio=2.0, min_within=0, keep=True, device=0):
        return self.f["cloud_outliers"](device, n, xyz.ctypes.data if xyz is not None else None, radius, k, std_ratio, min_within,
                                        self.keep.ctypes.data if keep else None, self.mean.ctypes.data, self.within.ctypes.data, self.counts, self.stats)

    def error(self):
        msg = self.f["last_error"](None)
        return msg.decode() if msg else ""


BAD_DEVICE = 12345


def test_outliers_bad_arguments_are_minus_2_without_a_device(eng):
    _, fns = eng.load()
    x = np.zeros((4, 3), np.float32)
    call = Call(fns, 4)
    # a bad device is not looked at before the arguments are
    assert call(4, None, device=BAD_DEVICE) == -2                         # NULL xyz with n > 0
    assert call(-1, x, device=BAD_DEVICE) == -2                           # negative n
    for r in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert call(4, x, radius=r, device=BAD_DEVICE) == -2, r
        assert "radius" in call.error()
    for k in (0, -1, 33, 1 << 20):
        assert call(4, x, k=k, device=BAD_DEVICE) == -2, k
        assert "k must lie in [1, 32]" in call.error()
    for s in (-1.0, -0.0001, float("nan"), -float("inf")):
        assert call(4, x, std_ratio=s, device=BAD_DEVICE) == -2, s
        assert "std_ratio" in call.error()
    assert call(4, x, min_within=-1, device=BAD_DEVICE) == -2 and "min_within" in call.error()
    assert call(4, x, keep=False, device=BAD_DEVICE) == -2                # NULL out_keep with n > 0
    assert (call.keep == 7).all() and (call.mean == 7.0).all() and (call.within == 7).all()   # a refusal writes nothing
    # the arguments are fine: only now is the device looked for
    assert call(4, x, device=BAD_DEVICE) == -100
    assert call(4, x, std_ratio=float("inf"), k=1, device=BAD_DEVICE) == -100
    assert call(4, x, k=32, min_within=5, std_ratio=0.0, device=BAD_DEVICE) == -100


def test_outliers_limits_are_minus_3_without_a_device(eng):
    _, fns = eng.load()
    call = Call(fns, 4)
    x = np.zeros((2, 3), np.float32)
    assert call(1 << 31, x, device=BAD_DEVICE) == -3 and "2^31" in call.error()   # refused on the count alone: the array is not read
    assert call(1 << 31, x, k=0, device=BAD_DEVICE) == -2                         # -2 comes first
    # the cell-span limit of the grid of this radius
    for axis in range(3):
        x = np.zeros((3, 3), np.float32)
        x[1, axis] = 1.0e6
        x[2] = np.nan
        assert call(3, x, radius=0.1, device=BAD_DEVICE) == -3
        text = call.error()
        assert "along " + "xyz"[axis] in text and "2^21" in text and "extent / radius = " in text, text
        assert f"{1.0e6 / float(np.float32(0.1)):.6g}" in text, text          # the ratio
        assert call(3, x, radius=1000.0, device=BAD_DEVICE) == -100            # fits: accepted, and only then is the device looked for
    assert (call.keep == 7).all()


def test_outliers_more_than_2_pow_29_finite_points_is_minus_3_without_a_device(eng):
    """the table's limit, on 6 GiB of zeros that are never written: a read-only anonymous mapping of the kernel's zero page (as in
    test_voxel_cpu.py), so the test takes address space and the host's pass over the points, not memory"""
    import mmap
    _, fns = eng.load()
    n = (1 << 29) + 1
    MAP_NORESERVE = getattr(mmap, "MAP_NORESERVE", 0x4000)
    mm = mmap.mmap(-1, n * 12, flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS | MAP_NORESERVE, prot=mmap.PROT_READ)
    try:
        x = np.frombuffer(mm, np.float32)
        call = Call(fns, 1)
        assert call(n, x, radius=1.0, device=BAD_DEVICE) == -3 and "2^29" in call.error()
        assert (call.keep == 7).all()
        del x
    finally:
        mm.close()


def test_outliers_empty_results_need_no_device(eng, cloud):
    _, fns = eng.load()
    call = Call(fns, 4)
    assert call(0, None, device=BAD_DEVICE) == 0
    assert list(call.counts) == [0, 0, 0] and list(call.stats) == [0.0, 0.0, 0.0] and (call.keep == 7).all()
    x = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan] * 3], np.float32)
    call = Call(fns, 4)
    assert call(4, x, device=BAD_DEVICE) == 0
    assert not call.keep.any() and np.isposinf(call.mean).all() and not call.within.any()
    assert list(call.counts) == [0, 0, 0] and list(call.stats) == [0.0, 0.0, 0.0]
    assert fns["cloud_outliers_ms"]() == 0.0
    # NULL mean, within, counts and stats are legal
    keep = np.full(4, 7, np.uint8)
    assert fns["cloud_outliers"](BAD_DEVICE, 4, x.ctypes.data, 0.1, 4, 2.0, 0, keep.ctypes.data, None, None, None, None) == 0 and not keep.any()
    r = cloud.remove_outliers(x, 0.1, device=BAD_DEVICE)
    assert r["keep"].dtype == bool and not r["keep"].any() and np.isposinf(r["mean_dist"]).all() and not r["within"].any()
    assert r["counts"].tolist() == [0, 0, 0] and r["stats"].tolist() == [0.0, 0.0, 0.0] and cloud.last_outliers_ms() == 0.0
    r = cloud.remove_outliers(np.zeros((0, 3), np.float32), 0.1)
    assert r["keep"].shape == (0,) and r["mean_dist"].shape == (0,) and r["within"].shape == (0,)
    want = statement_outliers(x, 0.1)
    assert all(np.array_equal(r0, want[k0]) for k0, r0 in cloud.remove_outliers(x, 0.1, device=BAD_DEVICE).items())
    for bad in ({"radius": -1.0}, {"radius": 0.1, "k": 0}, {"radius": 0.1, "k": 33}, {"radius": 0.1, "std_ratio": -1.0}, {"radius": 0.1, "min_within": -1}):
        with pytest.raises(ValueError):
            cloud.remove_outliers(np.zeros((2, 3), np.float32), **bad)
    with pytest.raises(RuntimeError):
        cloud.remove_outliers(np.zeros((2, 3), np.float32), 0.1, device=BAD_DEVICE)


def test_knn_null_cloud_is_minus_2(eng):
    _, fns = eng.load()
    q = np.zeros((2, 3), np.float32)
    d2 = np.full((2, 4), 7.0, np.float32)
    assert fns["cloud_knn"](None, 0.1, 4, 2, q.ctypes.data, d2.ctypes.data, None, None) == -2
    assert (d2 == 7.0).all()
    assert fns["cloud_knn_ms"](None, None) == 0.0


# ---- the statement against exact arithmetic ---------------------------------------------------------------------------------
def _rn(q):
    """the fp64 nearest (ties to even) to the rational q: int / int true division is correctly rounded"""
    q = Fraction(q)
    return q.numerator / q.denominator


def _rn32(q):
    """the fp32 nearest to the rational q, for results that are representable or far from a tie in fp64 (checked)"""
    d = _rn(q)
    f = np.float32(d)
    lo, hi = np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))
    q = Fraction(q)
    assert abs(q - Fraction(float(f))) <= abs(q - Fraction(float(lo))) and abs(q - Fraction(float(f))) <= abs(q - Fraction(float(hi)))
    return f


def _fix(q):
    return round(Fraction(q) * (1 << 30))   # round() of a Fraction: ties to even


def _exact_sqrt(d):
    r = math.sqrt(d)
    if d > 0:   # r is the fp64 nearest to the root: d lies between the squares of the midpoints to r's neighbours
        lo, hi = (Fraction(r) + Fraction(math.nextafter(r, 0.0))) / 2, (Fraction(r) + Fraction(math.nextafter(r, math.inf))) / 2
        assert lo * lo <= Fraction(d) <= hi * hi
    return r


def exact_statement(x, radius, k, std_ratio, min_within):
    """the contract of include/mpmvs.h point by point, every floating-point operation as the correctly rounded exact result"""
    r32 = np.float32(radius)
    r2 = _rn32(Fraction(float(r32)) ** 2)
    r = float(r32)
    n = len(x)
    fin = [all(math.isfinite(float(v)) for v in x[i]) for i in range(n)]
    mean, within, rows = [], [], []
    for i in range(n):
        keys = []
        if fin[i]:
            for j in range(n):
                if j == i or not fin[j]:
                    continue
                d = [_rn32(Fraction(float(x[i][a])) - Fraction(float(x[j][a]))) for a in range(3)]
                sq = [_rn32(Fraction(float(v)) ** 2) for v in d]
                d2 = _rn32(Fraction(float(_rn32(Fraction(float(sq[0])) + Fraction(float(sq[1]))))) + Fraction(float(sq[2])))
                if d2 <= r2:
                    keys.append((float(d2), j))
        keys.sort()
        within.append(len(keys))
        rows.append(keys[:k])
        if len(keys) < k:
            mean.append(np.float32(np.inf))
            continue
        s = _exact_sqrt(keys[0][0])
        for e in range(1, k):
            s = _rn(Fraction(s) + Fraction(_exact_sqrt(keys[e][0])))
        mean.append(_rn32(Fraction(_rn(Fraction(s) / k))))   # the fp64 quotient, then one rounding to fp32
    dense = [i for i in range(n) if math.isfinite(float(mean[i]))]
    c = len(dense)
    a = [_rn(Fraction(float(mean[i])) / Fraction(r)) for i in dense]
    S1 = sum(_fix(v) for v in a)
    S2 = sum(_fix(_rn(Fraction(v) * Fraction(v))) for v in a)
    if c:
        den = c * (1 << 30)
        mu = _rn(Fraction(_rn(S1)) / den)
        var = _rn(Fraction(_rn(Fraction(_rn(S2)) / den)) - Fraction(_rn(Fraction(mu) * Fraction(mu))))
        sigma = _exact_sqrt(max(0.0, var))
        T = math.inf if math.isinf(std_ratio) else _rn(Fraction(_rn(Fraction(mu) + Fraction(_rn(Fraction(std_ratio) * Fraction(sigma))))) * Fraction(r))
    else:
        mu = sigma = T = 0.0
    keep = [math.isfinite(float(mean[i])) and float(mean[i]) <= T and within[i] >= min_within for i in range(n)]
    return {"rows": rows, "mean": mean, "within": within, "c": c, "S1": S1, "S2": S2, "mu": mu, "sigma": sigma, "T": T, "keep": keep,
            "finite": sum(fin)}


@pytest.fixture(scope="module")
def thirty():
    rng = np.random.default_rng(17)
    x = (rng.random((30, 3)) * 0.2 + 100.0).astype(np.float32)
    x[10:14] = x[0:4]                     # duplicates: neighbours at d2 = 0, ordered by index
    x[7] = [np.nan, 1, 2]
    x[21, 2] = np.inf
    x[29] = 150.0                         # isolated
    return x


@pytest.mark.parametrize("k,std_ratio,min_within", [(3, 1.0, 0), (5, 2.0, 12), (1, float("inf"), 3)])
def test_statement_equals_exact_arithmetic_on_30_points(thirty, k, std_ratio, min_within):
    x, radius = thirty, 0.12
    want = exact_statement(x, radius, k, std_ratio, min_within)
    d2, idx, within = brute_knn(x, None, radius, k)
    assert within.tolist() == want["within"] and max(want["within"]) > k and min(want["within"]) == 0
    for i, row in enumerate(want["rows"]):
        assert idx[i, :len(row)].tolist() == [j for _, j in row] and (idx[i, len(row):] == -1).all()
        assert np.array_equal(d2[i, :len(row)].view(np.uint32), np.array([d for d, _ in row], np.float32).view(np.uint32))
        assert np.isposinf(d2[i, len(row):]).all()
    mean = mean_distance(d2, within, k)
    assert np.array_equal(mean.view(np.uint32), np.array(want["mean"], np.float32).view(np.uint32))
    c, S1, S2, mu, sigma, T = statistics(mean, radius, std_ratio)
    assert (c, S1, S2) == (want["c"], want["S1"], want["S2"]) and 5 < c < 28
    assert (mu, sigma, T) == (want["mu"], want["sigma"], want["T"])
    got = statement_outliers(x, radius, k, std_ratio, min_within)
    assert got["keep"].tolist() == want["keep"] and got["counts"].tolist() == [want["finite"], c, sum(want["keep"])]
    r = float(np.float32(radius))
    assert got["stats"].tolist() == [mu * r, sigma * r, T]
    assert 0 < sum(want["keep"]) < c or math.isinf(std_ratio)


def test_statement_property_scene():
    """the filter does what it is for: nearly every plane point stays, no flying or far point does"""
    x, plane = property_scene()
    got = statement_outliers(x, 0.05, 8, 2.0)
    print("plane kept", got["keep"][plane].mean(), "others kept", int(got["keep"][~plane].sum()))
    assert got["keep"][plane].mean() > 0.95 and got["keep"][~plane].sum() == 0
