"""What the analysis entry points refuse and the words they refuse it with (their shared argument checks and cloud loading in
erasor_amd/csrc/analysis_host.hip.h), compiled UNMODIFIED against the CPU stand-in of the HIP runtime (tests/cpp/simt_emu, as in
tests/test_evaluate_on_cpu.py) and checked by tests/test_gpu_analysis_errors.py itself: every case.  No GPU needed."""
import pytest

import simt

pytestmark = pytest.mark.timeout(3600)


@pytest.fixture(scope="module")
def simt_lib(tmp_path_factory):
    return simt.build_simt_lib(tmp_path_factory.mktemp("simt_analysis_errors"))


def test_the_analyses_refuse_the_same_things_in_the_same_words_on_the_cpu_stand_in(simt_lib):
    # 26 valid calls + 131 single faults + the table's own completeness
    simt.run_gpu_tests_on_stand_in(simt_lib, "test_gpu_analysis_errors.py", "one_fault or every_case", 158, no_skips=True)
