"""K estimates against one ground truth and the parameter sweep (the k_evm_* kernels in evaluate.hip.h and erasor_hip_evaluate_many /
erasor_hip_sweep in erasor_hip.hip), compiled UNMODIFIED against the CPU stand-in of the HIP runtime (tests/cpp/simt_emu, as in
tests/test_eval_classes_on_cpu.py) and checked by tests/test_gpu_sweep.py itself: evaluate_many against evaluate_clouds (K = 1, 3, 7,
voxel_leaf 0 and 0.2), the sweep against one configuration at a time, the scheduling, a failing configuration.  The stand-in cannot drive
two handles from two host threads at once, so there the sweeps run with concurrency=1; a step takes seconds there, so they step two
nodes of a small scene for four of the six configurations, and the scheduling case is the permuted sweep scored in pairs.  No GPU
needed."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
pytestmark = pytest.mark.timeout(3600)


@pytest.fixture(scope="module")
def simt_lib(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("simt_sweep") / "liberasor_hip_simt.so")
    subprocess.check_call(["g++", "-x", "c++", "-O1", "-std=c++20", "-pthread", "-ffp-contract=off", "-fPIC", "-shared", "-DERASOR_HIP_TEST_HOOKS",
                           "-I" + os.path.join(HERE, "cpp", "simt_emu"), "-o", lib, os.path.join(ROOT, "erasor_amd", "csrc", "erasor_hip.hip")])
    return lib


def test_the_sweep_passes_its_gpu_tests_on_the_cpu_stand_in(simt_lib):
    expr = "rows_match_evaluate_clouds or one_configuration_at_a_time or scheduling or failing_configuration"
    env = dict(os.environ, ERASOR_TEST_SIMT_LIB=simt_lib)
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(HERE, "test_gpu_sweep.py"), "-m", "gpu", "-q", "-x", "-k", expr,
                          "-p", "no:cacheprovider"], capture_output=True, text=True, timeout=3000, cwd=ROOT, env=env)
    tail = out.stdout[-1500:]
    sys.stdout.write(tail)
    assert out.returncode == 0 and " passed" in tail and "failed" not in tail, out.stdout[-4000:] + out.stderr[-2000:]
    n_passed = int(tail.split(" passed")[0].split()[-1])
    assert n_passed >= 9, tail  # 6 evaluate_many cases + one configuration at a time + scheduling + a failing configuration
