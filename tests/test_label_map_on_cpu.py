"""label_map and the static complement (nearest.hip.h and their host code in analysis_host.hip.h), compiled UNMODIFIED against the CPU
stand-in of the HIP runtime (tests/cpp/simt_emu, as in tests/test_overlap_on_cpu.py) and checked by tests/test_gpu_label_map.py itself:
the labelled world (host and device inputs), the float32 metric and its ties, far and degenerate clouds, subnormal differences, the
VoxelGrid pass-through, empty and invalid inputs, the complement against evalmap.static_complement, the errors and the struct layout.
No GPU needed."""
import pytest

import simt

pytestmark = pytest.mark.timeout(3600)


@pytest.fixture(scope="module")
def simt_lib(tmp_path_factory):
    return simt.build_simt_lib(tmp_path_factory.mktemp("simt_label_map"))


def test_label_map_and_complement_pass_their_gpu_tests_on_the_cpu_stand_in(simt_lib):
    expr = "world or metric or degenerate or subnormal or overflow or empty or threshold or errors_and_struct_layout"
    simt.run_gpu_tests_on_stand_in(simt_lib, "test_gpu_label_map.py", expr, 16)  # 4 world labels + 2 world complements + the metric + 4 degenerate + subnormal + overflow + 2 empty + threshold + errors
