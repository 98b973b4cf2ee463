"""Surface normals, curvature and eigenvalues (normals.hip.h and its host code in analysis_host.hip.h), compiled UNMODIFIED against the
CPU stand-in of the HIP runtime (tests/cpp/simt_emu, as in tests/test_knn_on_cpu.py) and checked by tests/test_gpu_normals.py itself:
byte for byte against evalmap.normals and the pure-Python normals_brute on the lattices' known answers, the tilted plane near and far,
ties at the k-th place in every index permutation, every list class at every size, the degenerate, collinear and signed-zero
neighbourhoods, both orientation rules, every combination of outputs, the refusals and the struct layout, the synthetic world, and the
handle's map with a step after it.  Everything except the 200 000-point case.  No GPU needed."""
import pytest

import simt

pytestmark = pytest.mark.timeout(3600)


@pytest.fixture(scope="module")
def simt_lib(tmp_path_factory):
    return simt.build_simt_lib(tmp_path_factory.mktemp("simt_normals"))


def test_the_normals_pass_their_gpu_tests_on_the_cpu_stand_in(simt_lib):
    # 3 lattices + 1 + 2 planes + 3 ties + 6 list classes + 4 degenerate and ambiguous + 3 orientation + buffers + refusals + world + map and step
    assert simt.run_gpu_tests_on_stand_in(simt_lib, "test_gpu_normals.py", "not random_world_of_200000", 26, no_skips=True) == 26
