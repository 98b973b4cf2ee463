"""The spatial-index tests (tests/test_gpu_spatial_index.py: the tree's and the grid's structure, the search's effort, the float32
overflow cases, and the smaller boundary-size and adversarial-geometry cases through the public calls) and the radix sort at its
callers' key widths (tests/test_gpu_hooks.py), run against erasor_hip.hip compiled UNMODIFIED, with the test hooks, for the CPU stand-in
of the HIP runtime (tests/cpp/simt_emu, as in tests/test_overlap_on_cpu.py).  No GPU needed."""
import pytest

import simt

pytestmark = pytest.mark.timeout(3600)


@pytest.fixture(scope="module")
def simt_lib(tmp_path_factory):
    return simt.build_simt_lib(tmp_path_factory.mktemp("simt_spatial"))


def test_the_spatial_index_tests_pass_on_the_cpu_stand_in(simt_lib):
    # everything but the boundary-size pairs with a tree of 32 * 1024 +- 1 points (the "large-" ids):
    # the module's 103 cases without the 6 large size pairs
    simt.run_gpu_tests_on_stand_in(simt_lib, "test_gpu_spatial_index.py", "not large", 97, no_skips=True)


def test_the_radix_sort_at_its_callers_key_widths_on_the_cpu_stand_in(simt_lib):
    # 2 widths x 3 kinds of keys x 5 sizes
    simt.run_gpu_tests_on_stand_in(simt_lib, "test_gpu_hooks.py", "stable_radix_bucketing and bit", 30, no_skips=True)
