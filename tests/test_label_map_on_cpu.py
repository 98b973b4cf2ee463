"""label_map and the static complement (nearest.hip.h and their host code in erasor_hip.hip), compiled UNMODIFIED against the CPU
stand-in of the HIP runtime (tests/cpp/simt_emu, as in tests/test_overlap_on_cpu.py) and checked by tests/test_gpu_label_map.py itself:
the labelled world (host and device inputs), the float32 metric and its ties, far and degenerate clouds, subnormal differences, the
VoxelGrid pass-through, empty and invalid inputs, the complement against evalmap.static_complement, the errors and the struct layout.
No GPU needed."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
pytestmark = pytest.mark.timeout(3600)


@pytest.fixture(scope="module")
def simt_lib(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("simt_label_map") / "liberasor_hip_simt.so")
    subprocess.check_call(["g++", "-x", "c++", "-O1", "-std=c++20", "-pthread", "-ffp-contract=off", "-fPIC", "-shared", "-DERASOR_HIP_TEST_HOOKS",
                           "-I" + os.path.join(HERE, "cpp", "simt_emu"), "-o", lib, os.path.join(ROOT, "erasor_amd", "csrc", "erasor_hip.hip")])
    return lib


def test_label_map_and_complement_pass_their_gpu_tests_on_the_cpu_stand_in(simt_lib):
    expr = "world or metric or degenerate or subnormal or overflow or empty or threshold or errors_and_struct_layout"
    env = dict(os.environ, ERASOR_TEST_SIMT_LIB=simt_lib)
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(HERE, "test_gpu_label_map.py"), "-m", "gpu", "-q", "-x", "-k", expr,
                          "-p", "no:cacheprovider"], capture_output=True, text=True, timeout=3000, cwd=ROOT, env=env)
    tail = out.stdout[-1500:]
    sys.stdout.write(tail)
    assert out.returncode == 0 and " passed" in tail and "failed" not in tail, out.stdout[-4000:] + out.stderr[-2000:]
    n_passed = int(tail.split(" passed")[0].split()[-1])
    assert n_passed >= 16, tail  # 4 world labels + 2 world complements + the metric + 4 degenerate + subnormal + overflow + 2 empty + threshold + errors
