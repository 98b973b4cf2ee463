"""Every frame's pose against the map (align.hip.h and its host code in erasor_hip.hip), compiled UNMODIFIED against the CPU stand-in of
the HIP runtime (tests/cpp/simt_emu, as in tests/test_overlap_on_cpu.py) and checked by tests/test_gpu_align.py itself: bit for bit
against evalmap.align_frames on the small scenario (host and device scans, a caller map and the handle's), the edge cases, the faults
it finds, steps and tickets after the check, the errors and the struct layout.  No GPU needed."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
pytestmark = pytest.mark.timeout(3600)


@pytest.fixture(scope="module")
def simt_lib(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("simt_align") / "liberasor_hip_simt.so")
    subprocess.check_call(["g++", "-x", "c++", "-O1", "-std=c++20", "-pthread", "-ffp-contract=off", "-fPIC", "-shared", "-DERASOR_HIP_TEST_HOOKS",
                           "-I" + os.path.join(HERE, "cpp", "simt_emu"), "-o", lib, os.path.join(ROOT, "erasor_amd", "csrc", "erasor_hip.hip")])
    return lib


def test_the_frame_check_passes_its_gpu_tests_on_the_cpu_stand_in(simt_lib):
    expr = "match_the_host_oracle or no_frames or finds or leaves_later or errors_and_struct_layout"
    env = dict(os.environ, ERASOR_TEST_SIMT_LIB=simt_lib)
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(HERE, "test_gpu_align.py"), "-m", "gpu", "-q", "-x", "-k", expr,
                          "-p", "no:cacheprovider"], capture_output=True, text=True, timeout=3000, cwd=ROOT, env=env)
    tail = out.stdout[-1500:]
    sys.stdout.write(tail)
    assert out.returncode == 0 and " passed" in tail and "failed" not in tail, out.stdout[-4000:] + out.stderr[-2000:]
    n_passed = int(tail.split(" passed")[0].split()[-1])
    assert n_passed >= 10, tail  # 4 exactness + 2 edge cases + no frames + the faults + steps after + errors
