"""The point-to-plane pose refinement (refine_plane.hip.h and its host code in analysis_host.hip.h), compiled UNMODIFIED against the CPU
stand-in of the HIP runtime (tests/cpp/simt_emu, as in tests/test_refine_on_cpu.py) and checked by tests/test_gpu_refine_plane.py itself:
byte for byte against evalmap.refine_poses_plane on the designed lattices (host and device scans, a caller map and the handle's), every
frame size, the curvature gate, the map points without a normal, the frozen frame, the dropped points, the far frame, the one-point
frame, the ties, the errors and the struct layout.  No GPU needed."""
import pytest

import simt

pytestmark = pytest.mark.timeout(3600)


@pytest.fixture(scope="module")
def simt_lib(tmp_path_factory):
    return simt.build_simt_lib(tmp_path_factory.mktemp("simt_refine_plane"))


def test_the_plane_refinement_passes_its_gpu_tests_on_the_cpu_stand_in(simt_lib):
    # everything but the steps after the call, as tests/test_refine_on_cpu.py: what they check -- an analysis in the evaluator's scratch
    # between announced steps -- tests/test_align_on_cpu.py runs on the stand-in for the same scratch
    simt.run_gpu_tests_on_stand_in(simt_lib, "test_gpu_refine_plane.py", "not leaves_later", 13)  # 4 lattices + 9 others
