"""The HIP kernels against the reference's OWN device code compiled for the host (oracle/_ref/libmpmvs_ref.so, built by
__graft_entry__.build() where the reference tree is present; see tests/ref_common.py), directly: no transcription in between.

tests/test_reference_cpu.py pins the oracle's literal modes to that code bit for bit, and tests/test_literal_gpu.py measures the
kernels against those modes at full size; here the two ends of that chain meet on one small scene (96x64, 4 source views):
the bars are the ones of test_literal_gpu.py, imported by name.  The checks themselves live in ref_common, because
test_reference_cpu.py runs the same ones on the oracle's canonical mode -- bit-identical to the kernels -- as the prediction of
this file.  A missing library fails; the reference tree itself is never read.

Below them, the reference's HOST code (libmpmvs_ref_host.so: RunFusion with its PLY writer, GetTriangulateVertices) against
mpmvs_fuse_ply and the device's vertex picker; tests/test_reference_host_cpu.py is the CPU half of that chain."""
import importlib

import numpy as np
import pytest

import ref_common as rc
import test_literal_gpu as bars
from test_fusion_cpu import REFERENCE_ORDER_COUNT_BAR, REFERENCE_ORDER_RECORDS_BAR
from test_prior_golden_cpu import make_cam
from test_prior_gpu import blank_context

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def direct(pm):
    return rc.Direct(pm)


@pytest.fixture(scope="module")
def gpu(direct, engine):
    return direct.attach(engine.create(0))


def test_eval_ncc_vs_compiled_reference(pm, direct, gpu):
    rc.check_ncc_direct(pm, direct, gpu, bars)


def test_eval_geom_vs_compiled_reference(pm, direct, gpu):
    rc.check_geom_direct(pm, direct, gpu)


def test_homography_vs_compiled_reference(pm, direct, gpu):
    rc.check_homography_direct(pm, direct, gpu)


def test_init_and_one_black_update_vs_compiled_reference(pm, oracle, direct, gpu):
    """InitializeScore with the same draws: identical planes (photometric), costs inside the T1 bars; then one BlackPixelUpdate per mode
    from an identical state: the T2 cost assertions.  The flip rate is printed beside the control -- the reference's IEEE build
    against its own contracted build, two real compiles -- and recorded in DESIGN.md 3.65; the ratio is not asserted."""
    rc.check_steps_direct(pm, oracle, direct, gpu, bars)


# ---- the reference's host code ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["96x72_colour_sky", "257x256", "96x72_and_64x48", "96x72_zero_and_negative_depth", "96x72_grey", "96x72_static"])
def test_fuse_ply_vs_compiled_reference(pm, oracle, engine, name):
    """the whole chain in one place: mpmvs_fuse_ply in reference order == oracle mode 2, every byte (as tests/test_fusion_gpu.py
    asserts on other scenes); against the file the reference's RunFusion writes, inside the named bars of tests/test_fusion_cpu.py;
    and the default snapshot formulation within the 5 % of test_snapshot_vs_reference_sequential_order"""
    fusion = importlib.import_module("mp-mvs_amd.fusion")
    case = rc.fusion_cases(pm)[name]
    _, want = case.reference()
    est = [True] * case.n
    got, _ = fusion.fuse_ply(case.cams, est, case.depths, case.normals, case.ours, case.sources, case.dynamic, sky=case.sky, reference_order=True)
    assert np.array_equal(got, case.oracle_records(oracle, fusion, 2))
    d_count, d_rec = rc.cloud_difference(got, want)
    print(f"{name}: fuse_ply in reference order against the compiled reference: count {len(got)} / {len(want)} (relative difference {d_count:.2e}), "
          f"records only one side has {d_rec:.2e}")
    assert len(want) > 1000 and d_count <= REFERENCE_ORDER_COUNT_BAR and d_rec <= REFERENCE_ORDER_RECORDS_BAR
    snap, _ = fusion.fuse_ply(case.cams, est, case.depths, case.normals, case.ours, case.sources, case.dynamic, sky=case.sky)
    print(f"{name}: snapshot formulation {len(snap)} points, {abs(len(snap) - len(want)) / len(want):.4f} from the reference's count")
    assert abs(len(snap) - len(want)) / len(want) < 0.05


@pytest.mark.parametrize("w,h", rc.VERTEX_SIZES)
def test_device_vertices_equal_the_reference(pm, engine, w, h):
    """k_prior_cells + scan + scatter == GetTriangulateVertices, both rules, every input of tests/test_reference_host_cpu.py"""
    ctx = blank_context(pm, engine, make_cam([100, 0, w / 2, 0, 100, h / 2, 0, 0, 1], w, h), w, h)
    for kind in rc.VERTEX_INPUTS:
        costs, geom = rc.vertex_inputs(w, h, kind)
        ctx.set_state(None, costs)
        ctx.set_geom_costs(geom)
        for geom_rule in (False, True):
            want = rc.ref_vertices(costs, geom, geom_rule)
            got = ctx.prior_vertices(geom_rule)
            assert got.shape == want.shape and np.array_equal(got, want), (kind, geom_rule, len(got), len(want))
