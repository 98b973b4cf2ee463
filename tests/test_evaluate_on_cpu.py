"""The device evaluator of PR / RR (evaluate.hip.h and its host code in analysis_host.hip.h), compiled UNMODIFIED against the CPU stand-in of
the HIP runtime (tests/cpp/simt_emu, as in tests/test_full_step_on_cpu.py) and checked by tests/test_gpu_evaluate.py itself: the
reference's golden vectors (host and device inputs), the per-point decisions against cKDTree, the errors and the struct layout, and
the handle's map after two steps.  No GPU needed."""
import pytest

import simt

pytestmark = pytest.mark.timeout(3600)


@pytest.fixture(scope="module")
def simt_lib(tmp_path_factory):
    simt.build_oracle()
    return simt.build_simt_lib(tmp_path_factory.mktemp("simt_eval"))


def test_the_evaluator_passes_its_gpu_tests_on_the_cpu_stand_in(simt_lib):
    expr = ("golden or per_point or threshold or device_inputs or tied or out_of_range or errors_and_struct_layout or "
            "(end_to_end_protocol and False-2)")
    simt.run_gpu_tests_on_stand_in(simt_lib, "test_gpu_evaluate.py", expr, 16)  # 2 golden + 8 per-point + threshold + device + tied + labels + errors + the handle's map
