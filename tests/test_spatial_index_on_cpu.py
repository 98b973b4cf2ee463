"""The spatial-index tests (tests/test_gpu_spatial_index.py: the tree's and the grid's structure, the search's effort, the float32
overflow cases, and the smaller boundary-size and adversarial-geometry cases through the public calls) and the radix sort at its
callers' key widths (tests/test_gpu_hooks.py), run against erasor_hip.hip compiled UNMODIFIED, with the test hooks, for the CPU stand-in
of the HIP runtime (tests/cpp/simt_emu, as in tests/test_overlap_on_cpu.py).  No GPU needed."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
pytestmark = pytest.mark.timeout(3600)


@pytest.fixture(scope="module")
def simt_lib(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("simt_spatial") / "liberasor_hip_simt.so")
    subprocess.check_call(["g++", "-x", "c++", "-O1", "-std=c++20", "-pthread", "-ffp-contract=off", "-fPIC", "-shared", "-DERASOR_HIP_TEST_HOOKS",
                           "-I" + os.path.join(HERE, "cpp", "simt_emu"), "-o", lib, os.path.join(ROOT, "erasor_amd", "csrc", "erasor_hip.hip")])
    return lib


def run_on_stand_in(simt_lib, module, expr):
    env = dict(os.environ, ERASOR_TEST_SIMT_LIB=simt_lib)
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(HERE, module), "-m", "gpu", "-q", "-x", "-k", expr, "-p", "no:cacheprovider"],
                         capture_output=True, text=True, timeout=3000, cwd=ROOT, env=env)
    tail = out.stdout[-1500:]
    sys.stdout.write(tail)
    assert out.returncode == 0 and " passed" in tail and "failed" not in tail and "skipped" not in tail, out.stdout[-4000:] + out.stderr[-2000:]
    return int(tail.split(" passed")[0].split()[-1])


def test_the_spatial_index_tests_pass_on_the_cpu_stand_in(simt_lib):
    # everything but the boundary-size pairs with a tree of 32 * 1024 +- 1 points (the "large-" ids)
    n_passed = run_on_stand_in(simt_lib, "test_gpu_spatial_index.py", "not large")
    assert n_passed >= 97, n_passed  # the module's 103 cases without the 6 large size pairs


def test_the_radix_sort_at_its_callers_key_widths_on_the_cpu_stand_in(simt_lib):
    n_passed = run_on_stand_in(simt_lib, "test_gpu_hooks.py", "stable_radix_bucketing and bit")
    assert n_passed >= 30, n_passed  # 2 widths x 3 kinds of keys x 5 sizes
