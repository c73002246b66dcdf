"""The observer (mpmvs_observer_*, cloud.Observer) as far as it goes without a GPU: the symbols, the
refusals that need no device, the statement of tests/observe_common.py by hand, the arithmetic of score_observed, the reader of
the scans' MeshLab project file and the --scanners file of tools/eval_ply.py."""
import ctypes as C
import importlib
import importlib.util
import os
import re

import numpy as np
import pytest

import observe_common as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NAMES = ("create", "classify", "maps", "stats", "ms", "destroy")


@pytest.fixture(scope="module")
def cloud(pm):
    return importlib.import_module("mp-mvs_amd.cloud")


def test_symbols_declared_exported_and_bound(pm):
    header = open(os.path.join(ROOT, "include", "mpmvs.h")).read()
    declared = set(re.findall(r"\b(mpmvs_[a-z0-9_]+)\s*\(", header))
    engine = importlib.import_module("mp-mvs_amd.engine")
    lib, fns = engine.load()
    lib_q8, fns_q8 = engine.load_variant(engine.LIB_Q8_PATH)
    for n in NAMES:
        name = "mpmvs_observer_" + n
        assert name in declared, f"{name} is not declared in include/mpmvs.h"
        assert hasattr(lib, name) and hasattr(lib_q8, name), f"{name} is not exported by both libraries"
        assert "observer_" + n in fns and "observer_" + n in fns_q8 and name in engine.ALL_SYMBOLS, f"{name} is not bound"
    for macro, value in (("MPMVS_OBSERVE_MAX_SCANNERS", 64), ("MPMVS_OBSERVE_MAX_FACE", 4096), ("MPMVS_OBSERVE_MAX_WINDOW", 8)):
        assert re.search(rf"#define {macro} {value}\b", header)


def test_refusals_without_a_device(pm):
    """every check that needs neither a cloud nor an observer handle comes before the handle is looked at, so a NULL handle
    shows it: the code, and the text that names the argument"""
    engine = importlib.import_module("mp-mvs_amd.engine")
    _, fns = engine.load()

    def err():
        return (fns["last_error"](None) or b"").decode()

    S = np.zeros((64, 3), f32)
    h = C.c_void_p(None)

    def create(n=1, s=S, R=8, w=1, out=True):
        return fns["observer_create"](None, n, s.ctypes.data if s is not None else None, None, R, w, C.byref(h) if out else None)

    assert create(out=False) == -2 and create(s=None) == -2
    for n in (0, -1, 65):
        assert create(n=n) == -2 and "scanners" in err(), n
    for bad in (np.nan, np.inf, -np.inf):
        s = S.copy()
        s[2, 1] = bad
        assert create(n=3, s=s) == -2 and "scanner 2" in err()
        assert create(n=2, s=s) == -2 and "no scan" in err()   # beyond the scanners in use: only the NULL scan is left to refuse
    for R in (0, -1, 4097):
        assert create(R=R) == -2 and "face_size" in err(), R
    for w in (-1, 9):
        assert create(w=w) == -2 and "window" in err(), w
    assert create(n=64, R=4096) == -3 and "2^31" in err()
    assert create(n=22, R=4096) == -3                        # 22 * 6 * 2^24 = 2^31 + 2^26
    assert create(n=21, R=4096) == -2 and "no scan" in err()   # within the limit: the NULL scan is next
    assert create(n=64, R=4097) == -2                         # -2 comes first
    assert create() == -2 and "no scan" in err() and h.value is None

    q = np.zeros((4, 3), f32)
    out = np.zeros(4, np.int32)

    def classify(n=4, qp=q, rel=0.02, ab=0.0, free=out):
        return fns["observer_classify"](None, n, qp.ctypes.data if qp is not None else None, rel, ab, free.ctypes.data if free is not None else None, None)

    for rel in (-0.01, 1.0, 1.5, np.nan, np.inf):
        assert classify(rel=rel) == -2 and "rel" in err(), rel
    for ab in (-1e-6, np.nan, np.inf):
        assert classify(ab=ab) == -2 and "abs_margin" in err(), ab
    assert classify(n=-1) == -2 and classify(qp=None) == -2 and classify(free=None) == -2
    assert classify(n=1 << 31) == -3 and "2^31" in err()     # refused on the count alone: the array is not read
    assert classify(n=(1 << 31) - 1) == -2 and "no handle" in err()
    assert classify(n=0) == -2 and "no handle" in err()
    assert fns["observer_maps"](None, 0, out.ctypes.data) == -2
    assert fns["observer_stats"](None, (C.c_longlong * 2)()) == -2
    assert fns["observer_ms"](None, None) == 0.0
    fns["observer_destroy"](None)


def test_statement_by_hand():
    for Z in (f32(2.5), f32(1e-3), f32(3e38)):
        S = np.zeros(3, f32)
        Zc, Zn = oc.maps(np.array([[Z, 0, 0]], f32), S, 1, 0)
        assert Zn.shape == (1, 6, 1, 1) and Zn[0, 0, 0, 0] == Z and np.isinf(Zn[0, 1:]).all() and np.array_equal(Zc, Zn)
        below = np.nextafter(Z, f32(0))
        q = np.array([[below, 0, 0], [Z, 0, 0], [np.nextafter(Z, f32(np.inf)), 0, 0], [-below, 0, 0], [np.nan, 0, 0], [0, 0, 0]], f32)
        free, cov = oc.classify(q, S, Zn, 0.0, 0.0)
        assert free.tolist() == [1, 0, 0, 0, 0, 0] and cov.tolist() == [1, 1, 1, 0, 0, 0]
    for R in (1, 2, 3, 8, 64):   # the tie d = (1, 1, 0): the lowest axis wins, and x == R is clamped into the last pixel
        part, f, px, py, z = oc.locate(np.array([[1, 1, 0], [-1, 1, 1], [0, -1, 1], [0, 0, -2]], f32), np.zeros(3, f32), R)
        assert part.all() and f.tolist() == [0, 1, 3, 5] and z.tolist() == [1, 1, 1, 2]
        assert (px[0], py[0]) == (R - 1, R // 2) and (px[1], py[1]) == (R - 1, R - 1) and (px[2], py[2]) == (R - 1, R // 2) and (px[3], py[3]) == (R // 2, R // 2)
    # the window stays on its face, and a difference that overflows takes no part
    Zc, Zn = oc.maps(np.array([[1, 0.9, 0], [3e38, 0, 0]], f32), np.array([[0, 0, 0], [-3e38, 0, 0]], f32), 4, 1)
    assert np.isfinite(Zc[0]).sum() == 2 and Zc[0, 0, 2, 3] == 1 and Zc[0, 0, 2, 2] == f32(3e38)
    assert np.isfinite(Zn[0]).sum() == 9 and np.isfinite(Zn[0, 0, 1:, 1:]).sum() == 9 and (Zn[0, 0, 1:, 2:] == 1).all()
    assert np.isfinite(Zc[1]).sum() == 1 and Zc[1, 0, 2, 2] == f32(3e38)   # 3e38 - -3e38 overflows: only the first point is there


def test_score_observed_by_hand(cloud):
    inf = np.inf
    d_rec = np.array([0.0, 0.01, 0.05, 0.05, 0.06, 0.2, 0.3, inf, inf, inf, 0.049, 0.11], f32)
    free = np.array([0, 1, 0, 2, 1, 0, 3, 0, 1, 0, 0, 64])
    d_gt = np.array([0.01, 0.2, inf, 0.05], f32)
    res = cloud.score_observed(d_rec, d_gt, free, [0.05, 0.1], (1, 2))
    plain = cloud.score(d_rec, d_gt, [0.05, 0.1], (1, 2))
    new = {"n_free_inaccurate", "n_unobserved", "accuracy_observed", "f1_observed"}
    for row, old in zip(res["tolerances"], plain["tolerances"]):
        assert set(row) == set(old) | new and {k: row[k] for k in old} == old
    assert {k: v for k, v in res.items() if k != "tolerances"} == {k: v for k, v in plain.items() if k != "tolerances"}
    a, b = res["tolerances"]
    # at 0.05: accurate 0, 0.01, 0.05, 0.05, 0.049; beyond it and seen through: 0.06, 0.3, inf (free 1), 0.11; beyond and unseen: 0.2, inf, inf
    assert (a["n_accurate"], a["n_free_inaccurate"], a["n_unobserved"]) == (5, 4, 3)
    assert a["accuracy"] == 5 / 12 and a["accuracy_observed"] == 5 / 9 and a["completeness"] == 0.5
    assert a["f1_observed"] == 2 * (5 / 9) * 0.5 / (5 / 9 + 0.5)
    assert (b["n_accurate"], b["n_free_inaccurate"], b["n_unobserved"]) == (6, 3, 3) and b["accuracy_observed"] == 6 / 9
    none = cloud.score_observed(np.array([inf, 1.0], f32), np.zeros(0, f32), [0, 0], [0.05])["tolerances"][0]
    assert (none["n_unobserved"], none["accuracy_observed"], none["f1_observed"]) == (2, 0.0, 0.0)   # the empty denominator
    with pytest.raises(ValueError):
        cloud.score_observed(d_rec, d_gt, free[:5], [0.05])


MLP = """<!DOCTYPE MeshLabDocument>
<MeshLabProject>
 <MeshGroup>
  <MLMesh label="scan1.ply" filename="scan1.ply">
   <MLMatrix44>
1 0 0 0.5
0 1 0 -2
0 0 1 3.25
0 0 0 1
</MLMatrix44>
  </MLMesh>
  <MLMesh label="second" filename="sub/scan2.ply">
   <MLMatrix44>0 -1 0 1e1 1 0 0 2 0 0 1 -3 0 0 0 1</MLMatrix44>
  </MLMesh>
 </MeshGroup>
 <RasterGroup/>
</MeshLabProject>
"""


def test_read_scan_alignment(cloud, tmp_path):
    p = tmp_path / "scan_alignment.mlp"
    p.write_text(MLP)
    got = cloud.read_scan_alignment(str(p))
    assert [g[0] for g in got] == ["scan1.ply", "sub/scan2.ply"] and all(g[1].shape == (4, 4) and g[1].dtype == np.float64 for g in got)
    assert got[0][1][:3, 3].tolist() == [0.5, -2.0, 3.25] and np.array_equal(got[0][1][:3, :3], np.eye(3))
    assert got[1][1].tolist() == [[0, -1, 0, 10], [1, 0, 0, 2], [0, 0, 1, -3], [0, 0, 0, 1]]
    for name, text in (("cut.mlp", MLP[:200]), ("short.mlp", MLP.replace("0 0 0 1\n</MLMatrix44>", "</MLMatrix44>")), ("word.mlp", MLP.replace("3.25", "x")),
                       ("noname.mlp", MLP.replace(' filename="scan1.ply"', "")), ("nomatrix.mlp", MLP.replace("MLMatrix44", "Other")),
                       ("empty.mlp", "<MeshLabProject><MeshGroup/></MeshLabProject>"), ("nan.mlp", MLP.replace("1e1", "nan"))):
        bad = tmp_path / name
        bad.write_text(text)
        with pytest.raises(ValueError):
            cloud.read_scan_alignment(str(bad))


def test_eval_ply_scanners_file(pm, tmp_path):
    spec = importlib.util.spec_from_file_location("eval_ply_tool", os.path.join(ROOT, "tools", "eval_ply.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    p = tmp_path / "scanners.txt"
    p.write_text("# scanner positions\n0.2 -0.1 0.3\n\n  1e1\t2 3   # the second\n#4 5 6\n-7 8.5 9")
    got = tool.read_scanners(str(p))
    assert got.dtype == f32 and got.tolist() == [[f32(0.2), f32(-0.1), f32(0.3)], [10, 2, 3], [-7, 8.5, 9]]
    for text in ("1 2\n", "1 2 3 4\n", "1 2 x\n", "1 2 nan\n", "# nothing\n", ""):
        p.write_text(text)
        with pytest.raises(SystemExit):
            tool.read_scanners(str(p))
