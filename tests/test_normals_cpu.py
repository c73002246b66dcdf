"""mpmvs_cloud_normals without a GPU: the symbols, the refusal of a NULL cloud, and the numpy statement of normals_common.py against
a second writing in scalar Python floats (bit for bit), against np.linalg.eigh, on exact cases and on the two property scenes."""
import ctypes as C
import importlib
import math
import os
import re

import numpy as np
import pytest

from knn_common import bits, brute_knn, property_scene
from normals_common import angle_to, fit, jacobi, offsets, pick, scatter, sphere_scene, statement_normals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mpmvs_cloud_normals", "mpmvs_cloud_normals_ms")


@pytest.fixture(scope="module")
def eng(pm):
    return importlib.import_module("mp-mvs_amd.engine")


def test_symbols_declared_exported_and_bound(eng):
    header = open(os.path.join(ROOT, "include", "mpmvs.h")).read()
    declared = set(re.findall(r"\b(mpmvs_[a-z0-9_]+)\s*\(", header))
    lib, fns = eng.load()
    lib_q8, fns_q8 = eng.load_variant(eng.LIB_Q8_PATH)
    for name in NEW:
        assert name in declared and name in eng.ALL_SYMBOLS
        assert hasattr(lib, name) and hasattr(lib_q8, name)
        assert name[len("mpmvs_"):] in fns and name[len("mpmvs_"):] in fns_q8
    assert fns["cloud_normals"].restype is C.c_int and len(fns["cloud_normals"].argtypes) == 9
    assert fns["cloud_normals_ms"].restype is C.c_float and len(fns["cloud_normals_ms"].argtypes) == 2
    # the library follows the header: the cloud unit includes it, and the objects depend on what they include (generated dependencies)
    csrc = os.path.join(ROOT, "mp-mvs_amd", "csrc")
    assert '#include "pm_normals.hpp"' in open(os.path.join(csrc, "mpmvs_cloud.hip")).read()
    makefile = open(os.path.join(csrc, "Makefile")).read()
    assert "mpmvs_cloud" in makefile and "-MMD" in makefile and "-include $(OBJS:.o=.d)" in makefile
    cloud = importlib.import_module("mp-mvs_amd.cloud")
    assert callable(cloud.Cloud.normals) and callable(cloud.Cloud.normals_ms) and callable(cloud.estimate_normals)


def test_null_cloud_is_minus_2(eng):
    _, fns = eng.load()
    out = np.full((2, 3), 7.0, np.float32)
    assert fns["cloud_normals"](None, 0.1, 16, 0, None, None, out.ctypes.data, None, None) == -2
    assert "cloud normals" in fns["last_error"](None).decode()
    assert (out == 7.0).all()
    assert fns["cloud_normals_ms"](None, None) == 0.0


# ---- the statement a second time, in scalar Python floats ------------------------------------------------------------------------
def scalar_normal(p, nbrs, view=None, ref=None):
    """the loop of include/mpmvs.h for one point p (3 floats) and its m neighbours in list order -> (normal 3 x fp32, curvature fp32)"""
    undefined = ([np.float32(0.0)] * 3, np.float32(np.inf))
    m = len(nbrs)
    if m < 2:
        return undefined
    s, Q = [0.0] * 3, [[0.0] * 3 for _ in range(3)]
    for j, q in enumerate(nbrs):
        e = [float(q[a]) - float(p[a]) for a in range(3)]
        for a in range(3):
            s[a] = e[a] if j == 0 else s[a] + e[a]
            for b in range(a, 3):
                Q[a][b] = e[a] * e[b] if j == 0 else Q[a][b] + e[a] * e[b]
    A = [[0.0] * 3 for _ in range(3)]
    for a in range(3):
        for b in range(a, 3):
            A[a][b] = A[b][a] = Q[a][b] - (s[a] * s[b]) / float(m + 1)
    V = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    for _ in range(8):
        for pp, qq, r in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
            apq = A[pp][qq]
            if apq == 0.0:
                continue
            theta = (A[qq][qq] - A[pp][pp]) / (2.0 * apq)
            t = (-1.0 if theta < 0.0 else 1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
            c = 1.0 / math.sqrt(t * t + 1.0)
            sn = t * c
            A[pp][pp], A[qq][qq] = A[pp][pp] - t * apq, A[qq][qq] + t * apq
            A[pp][qq] = A[qq][pp] = 0.0
            arp, arq = A[r][pp], A[r][qq]
            A[r][pp] = A[pp][r] = c * arp - sn * arq
            A[r][qq] = A[qq][r] = sn * arp + c * arq
            for i in range(3):
                vp, vq = V[i][pp], V[i][qq]
                V[i][pp], V[i][qq] = c * vp - sn * vq, sn * vp + c * vq
    d = [A[0][0], A[1][1], A[2][2]]
    i0 = 0
    for a in (1, 2):
        if d[a] < d[i0]:
            i0 = a
    dmid = min(d[a] for a in range(3) if a != i0)
    if not dmid > 0.0:
        return undefined
    pos = [v if v > 0.0 else 0.0 for v in d]
    tr = (pos[0] + pos[1]) + pos[2]
    n = [V[a][i0] for a in range(3)]
    lead = 0
    for a in (1, 2):
        if abs(n[a]) > abs(n[lead]):
            lead = a
    if n[lead] < 0.0:
        n = [-v for v in n]
    w = None
    if view is not None:
        w = [float(view[a]) - float(p[a]) for a in range(3)]
    if ref is not None:
        w = [float(ref[a]) for a in range(3)]
    if w is not None:
        dot = (n[0] * w[0] + n[1] * w[1]) + n[2] * w[2]
        if dot < 0.0:
            n = [-v for v in n]
    return [np.float32(v) for v in n], np.float32(pos[i0] / tr)


@pytest.fixture(scope="module")
def two_hundred():
    """200 points: a noisy plane patch, a blob, duplicates, a line, non-finite and isolated points"""
    rng = np.random.default_rng(23)
    plane = np.stack([rng.random(90) * 0.5, rng.random(90) * 0.5, 0.01 * rng.normal(size=90)], 1) + 50.0
    blob = rng.random((80, 3)) * 0.3 - 7.0
    line = np.stack([np.arange(10) * 0.0625, np.zeros(10), np.zeros(10)], 1) + 20.0
    rest = rng.random((20, 3)) * 0.1
    x = np.concatenate([plane, blob, line, rest]).astype(np.float32)
    x[100:104] = x[90:94]                  # duplicates
    x[195] = [np.nan, 0, 0]
    x[196, 1] = np.inf
    x[197] = 500.0                         # isolated
    x[198], x[199] = 600.0, 600.0          # a pair: one neighbour each, on the point
    return x


@pytest.mark.parametrize("k", [2, 5, 16])
def test_statement_equals_the_scalar_loop(two_hundred, k):
    x, radius = two_hundred, 0.15
    rng = np.random.default_rng(k)
    view = np.array([50.2, 50.1, 49.0])
    ref = rng.normal(size=x.shape).astype(np.float32)
    ref[5] = np.nan
    ref[6] = 0.0
    d2, idx, within = brute_knn(x, None, radius, k)
    assert within.min() == 0 and within.max() > k and (within == 1).any()
    modes = {"canonical": {}, "viewpoint": {"viewpoint": view}, "reference": {"reference": ref}}
    seen_defined = seen_undefined = 0
    for name, kw in modes.items():
        nrm, curv, w = statement_normals(x, radius, k, **kw)
        assert np.array_equal(w, within)
        for i in range(len(x)):
            nbrs = [x[j] for j in idx[i] if j >= 0]
            want_n, want_c = scalar_normal(x[i], nbrs, view if name == "viewpoint" else None, ref[i] if name == "reference" else None)
            assert np.array_equal(bits(nrm[i]), bits(np.array(want_n, np.float32))), (name, i, nrm[i], want_n)
            assert bits(curv[i : i + 1])[0] == bits(np.array([want_c], np.float32))[0], (name, i, curv[i], want_c)
            seen_defined += bool(np.isfinite(curv[i]))
            seen_undefined += not np.isfinite(curv[i])
    assert seen_defined > 300 and seen_undefined > 15
    can = statement_normals(x, radius, k)[0]
    vw = statement_normals(x, radius, k, viewpoint=view)[0]
    assert (bits(can) != bits(vw)).any(1).sum() > 10       # the viewpoint does flip some


# ---- the statement against LAPACK ------------------------------------------------------------------------------------------
# Measured with this file on 36 000 neighbourhoods (the cases below): the sine measure |n x n_ref| (l1 - l0) / l2 is 5.9e-16 at
# most, the eigenvalue measure |d_i0 - l0| / l2 is 9.3e-16 at most (relative to the largest eigenvalue: eigh promises no more for
# the smallest one).  Asserted at 16 x that, the project's margin for another LAPACK build.  (6.7e-16 was seen for the sine on
# 250 000 cases of another draw.)
SINE_MEASURED, EIG_MEASURED = 5.9e-16, 9.3e-16


def neighbourhoods(rng, count, k, noise):
    """offsets of k neighbours [count, k, 3]: a randomly oriented plane patch with `noise` across it, or isotropic (noise None)"""
    if noise is None:
        return rng.normal(size=(count, k, 3)) * 0.05
    e = np.concatenate([rng.uniform(-1, 1, (count, k, 2)), noise * rng.normal(size=(count, k, 1))], 2) * 0.05
    q, _ = np.linalg.qr(rng.normal(size=(count, 3, 3)))
    return np.einsum("nkj,nij->nki", e, q)


def test_statement_against_eigh():
    rng = np.random.default_rng(31)
    worst_sine = worst_eig = 0.0
    for k in (4, 16, 32):
        for noise in (1e-6, 1e-4, 1e-2, 0.3, None, None):
            e = neighbourhoods(rng, 2000, k, noise)
            m = np.full(len(e), k)
            with np.errstate(all="ignore"):
                Cm = scatter(e, m)
                d, V, off = jacobi(Cm)
                defined, nv, _, dmin = pick(d, V, m)
            assert defined.all() and not any(o.any() for o in off)          # all off-diagonals exactly 0 after 8 sweeps
            M = np.empty((len(e), 3, 3))
            for (a, b), val in Cm.items():
                M[:, a, b] = M[:, b, a] = val
            lam, vec = np.linalg.eigh(M)
            n = np.stack(nv, 1)
            sine = np.linalg.norm(np.cross(n, vec[:, :, 0]), axis=1) * (lam[:, 1] - lam[:, 0]) / lam[:, 2]
            eig = np.abs(dmin - lam[:, 0]) / lam[:, 2]
            assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 1e-15
            worst_sine, worst_eig = max(worst_sine, float(sine.max())), max(worst_eig, float(eig.max()))
    print(f"sine measure {worst_sine:.3g}, eigenvalue measure {worst_eig:.3g}")
    assert worst_sine <= 16 * SINE_MEASURED and worst_eig <= 16 * EIG_MEASURED


def test_eight_sweeps_are_enough():
    """8 and 12 sweeps give identical bits, and the early exit cannot show"""
    rng = np.random.default_rng(32)
    e = np.concatenate([neighbourhoods(rng, 1500, 16, s) for s in (1e-6, 1e-3, 0.3, None)])
    m = np.full(len(e), 16)
    with np.errstate(all="ignore"):
        Cm = scatter(e, m)
        d8, V8, _ = jacobi(Cm, 8)
        d12, V12, _ = jacobi(Cm, 12)
    for a, b in zip(d8 + [v for row in V8 for v in row], d12 + [v for row in V12 for v in row]):
        assert a.tobytes() == b.tobytes()


# ---- exact cases -------------------------------------------------------------------------------------------------------------
def lattice():
    g = np.arange(3, dtype=np.float32)
    return np.stack([*np.meshgrid(g, g, indexing="ij"), np.zeros((3, 3), np.float32)], -1).reshape(-1, 3) + np.float32(4.0)


def test_lattice_is_exact():
    x = lattice()
    nrm, curv, within = statement_normals(x, 1.5, 8)
    assert within.tolist() == [3, 5, 3, 5, 8, 5, 3, 5, 3]
    for i in range(9):                                        # the centre, the edges and the corners
        assert nrm[i].tolist() == [0.0, 0.0, 1.0] and not bits(nrm[i, :2]).any() and bits(curv)[i] == 0
    # the whole lattice as neighbourhood: the corner's sums do not vanish, the scatter matrix is still diagonal
    nrm, curv, _ = statement_normals(x, 3.0, 8)
    assert nrm[0].tolist() == [0.0, 0.0, 1.0] and nrm[4].tolist() == [0.0, 0.0, 1.0] and not curv.any()


def test_signs():
    x = lattice()
    up = np.array([0.0, 0.0, 1.0], np.float32)
    assert np.array_equal(statement_normals(x, 1.5, 8, viewpoint=[5.0, 5.0, 9.0])[0], np.tile(up, (9, 1)))
    below = statement_normals(x, 1.5, 8, viewpoint=[5.0, 5.0, -9.0])[0]
    assert np.array_equal(below, np.tile(-up, (9, 1))) and (bits(below) >> 31).all()          # every component negated
    assert np.array_equal(bits(statement_normals(x, 1.5, 8, viewpoint=[100.0, -3.0, 4.0])[0]), bits(np.tile(up, (9, 1))))   # in the plane: dot == 0
    ref = np.tile(np.array([0.3, 0.1, -2.0], np.float32), (9, 1))
    ref[2] = [0.0, 0.0, 1.0]
    ref[3] = np.nan                                           # keeps the canonical sign
    ref[4] = [1.0, 1.0, 0.0]                                  # dot == 0: keeps it
    ref[5] = 0.0
    got = statement_normals(x, 1.5, 8, reference=ref)[0]
    assert (got[[2, 3, 4, 5], 2] == 1.0).all() and (got[[0, 1, 6, 7, 8], 2] == -1.0).all()
    # canonical: the component of the largest magnitude is positive, whatever the plane
    rng = np.random.default_rng(8)
    e = neighbourhoods(rng, 3000, 8, 0.01)
    nrm, curv = fit(e, np.full(3000, 8))
    lead = np.take_along_axis(nrm, np.abs(nrm).argmax(1)[:, None], 1)
    assert (lead > 0).all() and np.isfinite(curv).all()


def test_undefined_cases():
    zero, inf = [0.0, 0.0, 0.0], np.float32(np.inf)

    def undefined(x, radius=1.0, k=4, rows=None):
        nrm, curv, within = statement_normals(np.array(x, np.float32), radius, k)
        rows = range(len(nrm)) if rows is None else rows
        return all(nrm[i].tolist() == zero and not bits(nrm[i]).any() and curv[i] == inf for i in rows), within

    assert undefined([[1, 2, 3]])[0]                                                  # n = 1
    assert undefined([[1, 2, 3], [1, 2, 3.5]])[0]                                     # one neighbour
    ok, within = undefined([[1, 2, 3]] * 6)                                           # all neighbours on the point
    assert ok and (within == 5).all()
    ok, within = undefined([[j * 0.25, 7, -2] for j in range(7)], k=6)                # an exact line along an axis
    assert ok and within.max() == 6
    ok, within = undefined([[j * 0.25, j * 0.25, 3] for j in range(5)], radius=2.0)   # and along a diagonal: one exact rotation
    assert ok
    ok, within = undefined([[np.nan, 0, 0], [0, 0, 0], [0.1, 0, 0], [0, 0.1, 0], [0, np.inf, 0]], rows=[0, 4])
    assert ok and within.tolist() == [0, 2, 2, 2, 0]
    nrm, curv, _ = statement_normals(np.array([[0, 0, 0], [0.5, 0, 0], [0, 0.5, 0]], np.float32), 1.0, 2)   # two neighbours off a line: defined
    assert (np.abs(nrm[:, 2]) == 1.0).all() and not curv.any()


# ---- the property scenes -----------------------------------------------------------------------------------------------------
def test_plane_scene():
    x, plane = property_scene()
    nrm, curv, within = statement_normals(x, 0.05, 16)
    ang = angle_to(nrm[plane], [0.0, 0.0, 1.0])
    print(f"plane scene: max {ang.max():.2f} deg, median {np.median(ang):.2f} deg")
    assert np.isfinite(curv[plane]).all() and plane.sum() == 1600 and ang.max() < 15.0


def test_sphere_scene():
    x, centre = sphere_scene()
    nrm, curv, within = statement_normals(x, 0.2, 16, viewpoint=centre)
    radial = centre - x.astype(np.float64)
    ang = angle_to(nrm, radial)
    print(f"sphere scene: max {ang.max():.2f} deg")
    assert np.isfinite(curv).all() and ang.max() < 15.0 and ((nrm * radial).sum(1) > 0).all()
