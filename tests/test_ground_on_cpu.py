"""The ground (ground.hip.h and its host code in analysis_host.hip.h), compiled UNMODIFIED against the CPU stand-in of the HIP runtime
(tests/cpp/simt_emu, as in tests/test_carve_on_cpu.py) and checked by tests/test_gpu_ground.py itself: byte for byte against
evalmap.ground_scans / ground_votes and their pure-Python twins on the known planes, the grid's edges, the seeds, the thresholds at their
exact ends, the degenerate patches, every patch size around every size class, the batches, every combination of outputs, the refusals and
the struct layout, the map form with its budget and its decision, the handle's map with a step before and after it, and the synthetic
world.  The whole file.  No GPU needed."""
import pytest

import simt

pytestmark = pytest.mark.timeout(3600)


@pytest.fixture(scope="module")
def simt_lib(tmp_path_factory):
    return simt.build_simt_lib(tmp_path_factory.mktemp("simt_ground"))


def test_the_ground_passes_its_gpu_tests_on_the_cpu_stand_in(simt_lib):
    # lattice + 3 tilts + wall + edges + permutations + 3 candidate counts + 2 num_lpr + min_z + no candidate + th_dist + uprightness +
    # elevation + 3 degenerate iterations + identical and collinear + header + sizes + whole scan + 5 batch sizes + nothing + outputs +
    # refusals + gathered clouds + budget + ratio + map and step + world
    assert simt.run_gpu_tests_on_stand_in(simt_lib, "test_gpu_ground.py", "test_", 37, no_skips=True) == 37
