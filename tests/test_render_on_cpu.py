"""The bird's-eye renderer (erasor_amd/csrc/render.hip.h and its host code in analysis_host.hip.h), compiled UNMODIFIED against the CPU stand-in
of the HIP runtime (tests/cpp/simt_emu, as in tests/test_eval_classes_on_cpu.py) and checked by tests/test_gpu_render.py itself: every
case but the full-size one -- the three modes, host and device inputs, order independence, points on pixel edges, the extremes of the
tile sort, the image sizes, the empty cloud and the errors, the error map's counts, voxel_leaf and the resident map.  No GPU needed."""
import pytest

import simt

pytestmark = pytest.mark.timeout(3600)


@pytest.fixture(scope="module")
def simt_lib(tmp_path_factory):
    simt.build_oracle()  # (tests/scenarios.py takes its parameters and poses from the oracle's helpers)
    return simt.build_simt_lib(tmp_path_factory.mktemp("simt_render"))


def test_the_renderer_passes_its_gpu_tests_on_the_cpu_stand_in(simt_lib):
    # modes + order + 2 lattices + tile extremes + 7 sizes + errors + eval counts + 2 resident maps + fit + in flight
    simt.run_gpu_tests_on_stand_in(simt_lib, "test_gpu_render.py", "not full_size", 18)
