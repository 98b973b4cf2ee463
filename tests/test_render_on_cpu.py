"""The bird's-eye renderer (erasor_amd/csrc/render.hip.h and its host code in erasor_hip.hip), compiled UNMODIFIED against the CPU stand-in
of the HIP runtime (tests/cpp/simt_emu, as in tests/test_eval_classes_on_cpu.py) and checked by tests/test_gpu_render.py itself: every
case but the full-size one -- the three modes, host and device inputs, order independence, points on pixel edges, the extremes of the
tile sort, the image sizes, the empty cloud and the errors, the error map's counts, voxel_leaf and the resident map.  No GPU needed."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
pytestmark = pytest.mark.timeout(3600)


@pytest.fixture(scope="module")
def simt_lib(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("simt_render") / "liberasor_hip_simt.so")
    subprocess.check_call(["g++", "-x", "c++", "-O1", "-std=c++20", "-pthread", "-ffp-contract=off", "-fPIC", "-shared", "-DERASOR_HIP_TEST_HOOKS",
                           "-I" + os.path.join(HERE, "cpp", "simt_emu"), "-o", lib, os.path.join(ROOT, "erasor_amd", "csrc", "erasor_hip.hip")])
    sys.path.insert(0, ROOT)
    from oracle import orc
    orc.build()  # (tests/scenarios.py takes its parameters and poses from the oracle's helpers)
    return lib


def test_the_renderer_passes_its_gpu_tests_on_the_cpu_stand_in(simt_lib):
    env = dict(os.environ, ERASOR_TEST_SIMT_LIB=simt_lib)
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(HERE, "test_gpu_render.py"), "-m", "gpu", "-q", "-x", "-k", "not full_size",
                          "-p", "no:cacheprovider"], capture_output=True, text=True, timeout=3000, cwd=ROOT, env=env)
    tail = out.stdout[-1500:]
    sys.stdout.write(tail)
    assert out.returncode == 0 and " passed" in tail and "failed" not in tail, out.stdout[-4000:] + out.stderr[-2000:]
    n_passed = int(tail.split(" passed")[0].split()[-1])
    assert n_passed >= 18, tail  # modes + order + 2 lattices + tile extremes + 7 sizes + errors + eval counts + 2 resident maps + fit + in flight
