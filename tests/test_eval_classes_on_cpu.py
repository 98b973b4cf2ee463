"""PR / RR by class and by dynamic instance (the k_ev_*_keys kernels onwards in evaluate.hip.h and their host code in analysis_host.hip.h),
compiled UNMODIFIED against the CPU stand-in of the HIP runtime (tests/cpp/simt_emu, as in tests/test_evaluate_on_cpu.py) and checked by
tests/test_gpu_eval_classes.py itself: the oracle and the invariants on host and device inputs, ties, one class everywhere, empty clouds,
voxel_leaf, the errors, the sizing and the struct layout.  No GPU needed."""
import pytest

import simt

pytestmark = pytest.mark.timeout(3600)


@pytest.fixture(scope="module")
def simt_lib(tmp_path_factory):
    return simt.build_simt_lib(tmp_path_factory.mktemp("simt_eval_classes"))


def test_the_breakdown_passes_its_gpu_tests_on_the_cpu_stand_in(simt_lib):
    expr = "rows_match or one_class or empty or voxel_leaf or errors_sizing"
    simt.run_gpu_tests_on_stand_in(simt_lib, "test_gpu_eval_classes.py", expr, 8)  # 4 oracle / invariant cases + one class + empty clouds + voxel_leaf + errors and sizing
