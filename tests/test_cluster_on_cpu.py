"""The Euclidean clustering (cluster.hip.h and its host code in analysis_host.hip.h), compiled UNMODIFIED against the CPU stand-in of the
HIP runtime (tests/cpp/simt_emu, as in tests/test_label_map_on_cpu.py) and checked by tests/test_gpu_cluster.py itself: byte for byte
against evalmap.cluster / cluster_brute at the predicate's edge, at every cell border, on chains in every order, under contention, at
every size, on far points and the clamp, the table, the limits and the buffers, the errors and the struct layout, the synthetic world,
the handle's map with a step after it, and the residue.  Everything except the 100 000- and 200 000-point cases and the driver's run
(the driver links the product library).  No GPU needed."""
import pytest

import simt

pytestmark = pytest.mark.timeout(3600)


@pytest.fixture(scope="module")
def simt_lib(tmp_path_factory):
    return simt.build_simt_lib(tmp_path_factory.mktemp("simt_cluster"))


def test_the_clustering_passes_its_gpu_tests_on_the_cpu_stand_in(simt_lib):
    expr = "not hundred_thousand and not random_world_of_200000 and not driver"
    # 4 edges + 4 margins + 6 chains + interleaved + contention + 18 + 12 sizes + far + 2 table + 12 limits + buffers + errors + world
    # + map and step + residue
    simt.run_gpu_tests_on_stand_in(simt_lib, "test_gpu_cluster.py", expr, 66)
