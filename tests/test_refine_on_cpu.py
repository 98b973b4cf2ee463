"""Every frame's pose refined against the map (refine.hip.h and its host code in analysis_host.hip.h), compiled UNMODIFIED against the CPU
stand-in of the HIP runtime (tests/cpp/simt_emu, as in tests/test_align_on_cpu.py) and checked by tests/test_gpu_refine.py itself: byte for
byte against evalmap.refine_poses on a thinned small world (host and device scans, a caller map and the handle's), every frame size, the
ties, the gate, the frozen frame, the dropped points, the errors and the struct layout.  No GPU needed."""
import pytest

import simt

pytestmark = pytest.mark.timeout(3600)


@pytest.fixture(scope="module")
def simt_lib(tmp_path_factory):
    return simt.build_simt_lib(tmp_path_factory.mktemp("simt_refine"))


def test_the_pose_refinement_passes_its_gpu_tests_on_the_cpu_stand_in(simt_lib):
    # everything but the steps after the call: three minutes of stepping on the stand-in, and what they check -- an analysis in the
    # evaluator's scratch between announced steps -- tests/test_align_on_cpu.py runs there for the same scratch
    simt.run_gpu_tests_on_stand_in(simt_lib, "test_gpu_refine.py", "not leaves_later", 12)  # 4 small world + 8 others
