"""The overlap report (nearest.hip.h and its host code in analysis_host.hip.h), compiled UNMODIFIED against the CPU stand-in of the HIP
runtime (tests/cpp/simt_emu, as in tests/test_evaluate_on_cpu.py) and checked by tests/test_gpu_overlap.py itself: the reference's
golden numbers (host and device inputs), the per-point distances against cKDTree and nearest indices against brute force, the errors
and the struct layout.  No GPU needed."""
import pytest

import simt

pytestmark = pytest.mark.timeout(3600)


@pytest.fixture(scope="module")
def simt_lib(tmp_path_factory):
    return simt.build_simt_lib(tmp_path_factory.mktemp("simt_overlap"))


def test_the_overlap_report_passes_its_gpu_tests_on_the_cpu_stand_in(simt_lib):
    expr = "golden or per_point or voxel_leaf or errors_and_struct_layout"
    simt.run_gpu_tests_on_stand_in(simt_lib, "test_gpu_overlap.py", expr, 16)  # 2 golden + 11 per-point distances + the tie rule + voxel_leaf + errors
