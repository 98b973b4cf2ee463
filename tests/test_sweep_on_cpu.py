"""K estimates against one ground truth and the parameter sweep (the k_evm_* kernels in evaluate.hip.h and erasor_hip_evaluate_many /
erasor_hip_sweep in analysis_host.hip.h), compiled UNMODIFIED against the CPU stand-in of the HIP runtime (tests/cpp/simt_emu, as in
tests/test_eval_classes_on_cpu.py) and checked by tests/test_gpu_sweep.py itself: evaluate_many against evaluate_clouds (K = 1, 3, 7,
voxel_leaf 0 and 0.2), the sweep against one configuration at a time, the scheduling, a failing configuration.  The stand-in cannot drive
two handles from two host threads at once, so there the sweeps run with concurrency=1; a step takes seconds there, so they step two
nodes of a small scene for four of the six configurations, and the scheduling case is the permuted sweep scored in pairs.  No GPU
needed."""
import pytest

import simt

pytestmark = pytest.mark.timeout(3600)


@pytest.fixture(scope="module")
def simt_lib(tmp_path_factory):
    return simt.build_simt_lib(tmp_path_factory.mktemp("simt_sweep"))


def test_the_sweep_passes_its_gpu_tests_on_the_cpu_stand_in(simt_lib):
    expr = "rows_match_evaluate_clouds or one_configuration_at_a_time or scheduling or failing_configuration"
    # 6 evaluate_many cases + one configuration at a time + scheduling + a failing configuration
    simt.run_gpu_tests_on_stand_in(simt_lib, "test_gpu_sweep.py", expr, 9)
