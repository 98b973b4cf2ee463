"""The k nearest neighbours, radius counts and density filters (knn.hip.h and their host code in analysis_host.hip.h), compiled
UNMODIFIED against the CPU stand-in of the HIP runtime (tests/cpp/simt_emu, as in tests/test_cluster_on_cpu.py) and checked by
tests/test_gpu_knn.py itself: byte for byte against evalmap.knn / radius_count / density_filter and the all-pairs versions on ties at
the k-th place, one float32 step at the k-th place, the radius and the threshold, every cell border, duplicates, short clouds, every
size and list class, degenerate boxes, the prefix property, the mean's order, every score with every rule, the buffers, the errors and
the struct layout, the synthetic world, and the handle's map with a step after it.  Everything except the 200 000-point case (the
driver's run, tests/test_knn_driver.py, links the product library).  No GPU needed."""
import pytest

import simt

pytestmark = pytest.mark.timeout(3600)


@pytest.fixture(scope="module")
def simt_lib(tmp_path_factory):
    return simt.build_simt_lib(tmp_path_factory.mktemp("simt_knn"))


def test_the_density_analyses_pass_their_gpu_tests_on_the_cpu_stand_in(simt_lib):
    # 6 ties + 5 + 4 + 2 + 1 steps + 3 + 1 duplicates + 3 short + 63 sizes + 6 classes + 3 boxes + prefix + mean + 6 filters + buffer + errors
    # + world + map and step
    simt.run_gpu_tests_on_stand_in(simt_lib, "test_gpu_knn.py", "not random_world_of_200000", 109)
