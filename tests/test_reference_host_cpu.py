"""The oracle's fusion and the host's vertex picker against the reference's OWN host code compiled here (oracle/ref_host_driver.cpp
over oracle/ref_shim/host_standin.h, see tests/ref_common.py): RunFusion with the reference's PLY writer, and
PatchMatchCUDA::GetTriangulateVertices.

Fusion: oracle mode 1 (oracle/fusion_oracle.cpp, the literal sequential restatement) must write the file the reference writes,
byte for byte -- point count, order and all 27 bytes of every record -- under the build whose cv::Vec3f `/=` divides; under the
build whose `/=` multiplies by the fp32 reciprocal only the averaged normal may move, by one ulp.  Mode 2 -- the same order in the
canonical arithmetic, which the GPU's reference-order mode equals bit for bit (tests/test_fusion_gpu.py) -- is measured against
the same file and held to the named bars of tests/test_fusion_cpu.py.

Vertices: mp-mvs_amd/host/planar_prior.cpp (which csrc/pm_prior.hpp's k_prior_cells equals bit for bit, tests/test_prior_gpu.py)
must return the reference's vertex list, under both rules.

NaN and infinite depths stay out: the reference's int() of a NaN coordinate is undefined behaviour.  A missing library is an
error (tests/ref_common.py), never a skip."""
import importlib

import numpy as np
import pytest

import ref_common as rc
from test_fusion_cpu import REFERENCE_ORDER_COUNT_BAR, REFERENCE_ORDER_RECORDS_BAR

CASES = ["96x72_dynamic", "96x72_static", "96x72_grey", "96x72_colour_sky", "131x97", "257x256", "96x72_and_64x48", "96x72_32_sources",
         "96x72_zero_and_negative_depth"]


@pytest.fixture(scope="module")
def fusion():
    return importlib.import_module("mp-mvs_amd.fusion")


@pytest.fixture(scope="module")
def cases(pm):
    got = rc.fusion_cases(pm)
    assert sorted(got) == sorted(CASES)
    return got


@pytest.mark.parametrize("name", CASES)
def test_literal_fusion_writes_the_reference_file(cases, oracle, fusion, name):
    case = cases[name]
    _, want = case.reference()
    got = case.oracle_records(oracle, fusion, 1)
    print(f"{name}: the reference fuses {len(want)} points, oracle mode 1 {len(got)}")
    assert len(want) > 1000                      # holds for every case, the long-list and two-size ones included (7 569 at the least)
    assert got.shape == want.shape
    assert np.array_equal(got, want), f"{int((got != want).any(1).sum())} of {len(want)} records differ"


@pytest.mark.parametrize("name", CASES)
def test_literal_fusion_vs_reciprocal_build(cases, oracle, fusion, name):
    """the build whose Vec3f `/=` multiplies by 1.f / s: positions, colours, count and order as before, every normal component
    within one ulp (a / s against a * (1 / s): the reciprocal is rounded once, the product once)"""
    case = cases[name]
    _, want = case.reference(rcp=True)
    got = case.oracle_records(oracle, fusion, 1)
    assert got.shape == want.shape
    assert np.array_equal(got[:, :12], want[:, :12]) and np.array_equal(got[:, 24:], want[:, 24:])
    a, b = (np.ascontiguousarray(r[:, 12:24]).view(np.float32) for r in (got, want))
    ulp = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
    assert (np.sign(a) == np.sign(b)).all() and ulp.max() <= 1
    print(f"{name}: {int((ulp > 0).any(1).sum())} of {len(want)} normals differ from the reciprocal build, by at most {int(ulp.max())} ulp")


def test_the_truncation_path_ran(cases):
    """int(x + 0.5f) truncates (-1, 0) to pixel 0: pixels whose source coordinate lands there exist in the scenes as they are"""
    counts = {name: cases[name].truncated_pixels() for name in CASES}
    print("pixel / source pairs with a coordinate + 0.5 in (-1, 0):", counts)
    assert sum(1 for v in counts.values() if v > 0) >= 2


@pytest.mark.parametrize("name", CASES)
def test_reference_order_canonical_vs_reference(cases, oracle, fusion, name):
    """oracle mode 2 = what the GPU's reference-order mode computes, against the reference's file"""
    case = cases[name]
    _, want = case.reference()
    got = case.oracle_records(oracle, fusion, 2)
    d_count, d_rec = rc.cloud_difference(got, want)
    print(f"{name}: mode 2 against the compiled reference: count {len(got)} / {len(want)} (relative difference {d_count:.2e}), records only one side has {d_rec:.2e}")
    assert d_count <= REFERENCE_ORDER_COUNT_BAR and d_rec <= REFERENCE_ORDER_RECORDS_BAR
    assert REFERENCE_ORDER_COUNT_BAR <= 0.002 and REFERENCE_ORDER_RECORDS_BAR <= 0.002


def test_ply_header_bytes(cases, hostlib, tmp_path):
    """the header the reference writes == the header of host/scene_io.cpp's writer for the same point count; and the records of the
    writer == fusion.ply_records: B,G,R -> red green blue, (char)(int) truncation"""
    header, want = cases["96x72_colour_sky"].reference()
    pts = np.zeros((len(want), 9), np.float32)
    pts[:, :6] = np.ascontiguousarray(want[:, :24]).view(np.float32)
    pts[:, 6:9] = want[:, [26, 25, 24]].astype(np.float32) + np.float32(0.75)      # any fraction truncates to the same byte
    path = tmp_path / "ours.ply"
    hostlib.write_ply(path, pts)
    raw = open(path, "rb").read()
    assert raw[:len(header)] == header
    assert np.array_equal(np.frombuffer(raw, np.uint8, offset=len(header)).reshape(-1, rc.PLY_RECORD), want)


# ---- vertices -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom_rule", [False, True])
@pytest.mark.parametrize("kind", rc.VERTEX_INPUTS)
@pytest.mark.parametrize("w,h", rc.VERTEX_SIZES)
def test_host_vertices_equal_the_reference(hostlib, w, h, kind, geom_rule):
    costs, geom = rc.vertex_inputs(w, h, kind)
    want = rc.ref_vertices(costs, geom, geom_rule)
    got = hostlib.triangulate_vertices(costs, geom, geom_rule)
    ncells = ((w + 4) // 5) * ((h + 4) // 5)
    if kind == "all_invalid":
        assert len(want) == 0
    else:
        assert 0.3 * ncells < len(want) < 2.1 * ncells
    if kind == "invalid_cells_and_origin" and geom_rule:
        assert (want == 0).all(1).sum() >= 3            # the never-assigned (0, 0) points of the first cell
    assert got.shape == want.shape and np.array_equal(got, want)


def test_vertex_inputs_hold_what_they_promise():
    w, h = 85, 75
    costs, geom = rc.vertex_inputs(w, h, "ties")
    cells = costs.reshape(h // 5, 5, w // 5, 5).transpose(0, 2, 1, 3).reshape(-1, 25)
    low3 = np.sort(np.where(cells < 1.0, cells, np.inf), 1)[:, :4]
    assert (low3[:, 0] == low3[:, 1]).sum() > 5 and (low3[:, 1] == low3[:, 2]).sum() > 5 and (low3[:, 2] == low3[:, 3]).sum() > 5
    costs, geom = rc.vertex_inputs(w, h, "exact")
    assert all((costs == np.float32(v)).sum() > 50 for v in (0.1, 0.2, 1.0, 2.0)) and (geom == np.float32(0.4)).sum() > 50
    costs, _ = rc.vertex_inputs(w, h, "invalid_cells_and_origin")
    assert (costs.reshape(h // 5, 5, w // 5, 5).min((1, 3)) >= 2.0).sum() > 20
    costs, _ = rc.vertex_inputs(w, h, "nan")
    assert 10 < np.isnan(costs).sum() < 200


def test_a_nan_cost_silences_its_cell_under_the_geometric_rule(hostlib):
    """std::max(cost_sum, 0.2f) returns its NaN first argument: no vertex passes in a cell that holds a NaN cost"""
    w, h = 85, 75
    costs, geom = rc.vertex_inputs(w, h, "nan")
    got = hostlib.triangulate_vertices(costs, geom, True)
    nan_cell = np.isnan(costs.reshape(h // 5, 5, w // 5, 5)).any((1, 3))
    assert nan_cell.sum() > 10 and not nan_cell[got[:, 1] // 5, got[:, 0] // 5].any()
    clean = hostlib.triangulate_vertices(np.nan_to_num(costs, nan=1.5), geom, True)
    assert len(clean) > len(got)                         # cells that would otherwise have had a vertex
