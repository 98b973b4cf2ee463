"""The scans' labelling (label_scans.hip.h and its host code in analysis_host.hip.h), compiled UNMODIFIED against the CPU stand-in of the
HIP runtime (tests/cpp/simt_emu, as in tests/test_align_on_cpu.py) and checked by tests/test_gpu_label_scans.py itself: byte for byte
against evalmap.label_scans on a short scenario after its steps (host and device scans, a caller map and the handle's, with and without
a raw map, every split), the edge shapes, the threshold, the exact properties, the bounded search's effort, the errors and the struct
layout, a step and a ticket after the call.  No GPU needed."""
import pytest

import simt

pytestmark = pytest.mark.timeout(3600)


@pytest.fixture(scope="module")
def simt_lib(tmp_path_factory):
    return simt.build_simt_lib(tmp_path_factory.mktemp("simt_label_scans"))


def test_the_scans_labelling_passes_its_gpu_tests_on_the_cpu_stand_in(simt_lib):
    expr = ("match_the_host_oracle or frame_sizes or frames_of_one_code or dropped_points or at_the_threshold or around_one_leaf or an_empty_static_map "
            "or shrinking_tau or never_works_harder or errors_capacity or leaves_later")
    # 8 exactness + 5 size sets + one code + dropped + 4 thresholds + 4 map sizes + empty maps + properties + 4 effort + errors + steps after
    simt.run_gpu_tests_on_stand_in(simt_lib, "test_gpu_label_scans.py", expr, 31)
