"""The HIP kernels against the reference's OWN device code compiled for the host (oracle/_ref/libmpmvs_ref.so, built by
__graft_entry__.build() where the reference tree is present; see tests/ref_common.py), directly: no transcription in between.

tests/test_reference_cpu.py pins the oracle's literal modes to that code bit for bit, and tests/test_literal_gpu.py measures the
kernels against those modes at full size; here the two ends of that chain meet on one small scene (96x64, 4 source views):
the bars are the ones of test_literal_gpu.py, imported by name.  The checks themselves live in ref_common, because
test_reference_cpu.py runs the same ones on the oracle's canonical mode -- bit-identical to the kernels -- as the prediction of
this file.  A missing library fails; the reference tree itself is never read."""
import pytest

import ref_common as rc
import test_literal_gpu as bars

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
