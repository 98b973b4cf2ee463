"""Every frame's pose against the map (align.hip.h and its host code in analysis_host.hip.h), compiled UNMODIFIED against the CPU stand-in of
the HIP runtime (tests/cpp/simt_emu, as in tests/test_overlap_on_cpu.py) and checked by tests/test_gpu_align.py itself: bit for bit
against evalmap.align_frames on the small scenario (host and device scans, a caller map and the handle's), the edge cases, the faults
it finds, steps and tickets after the check, the errors and the struct layout.  No GPU needed."""
import pytest

import simt

pytestmark = pytest.mark.timeout(3600)


@pytest.fixture(scope="module")
def simt_lib(tmp_path_factory):
    return simt.build_simt_lib(tmp_path_factory.mktemp("simt_align"))


def test_the_frame_check_passes_its_gpu_tests_on_the_cpu_stand_in(simt_lib):
    expr = "match_the_host_oracle or no_frames or finds or leaves_later or errors_and_struct_layout"
    simt.run_gpu_tests_on_stand_in(simt_lib, "test_gpu_align.py", expr, 10)  # 4 exactness + 2 edge cases + no frames + the faults + steps after + errors
