"""The decision per object (objects.hip.h and its host code in analysis_host.hip.h), compiled UNMODIFIED against the CPU stand-in of the
HIP runtime (tests/cpp/simt_emu, as in tests/test_cluster_on_cpu.py) and checked by tests/test_gpu_object_vote.py itself: byte for byte
against evalmap.object_vote / object_vote_brute on the scene with the hand-written answer, the ground outside the graph, the
predicate's edge through the compaction, every decision at its edge, the vote threshold, the indexing, every size, contention, many
rows and short buffers, the handle's map with a step after it, the errors and the struct layout, and the synthetic world.  Every case
of that file.  No GPU needed."""
import pytest

import simt

pytestmark = pytest.mark.timeout(3600)


@pytest.fixture(scope="module")
def simt_lib(tmp_path_factory):
    return simt.build_simt_lib(tmp_path_factory.mktemp("simt_object_vote"))


def test_the_decision_per_object_passes_its_gpu_tests_on_the_cpu_stand_in(simt_lib):
    # 2 known + no mask + bridge + 2 edges + 6 remove + 5 revert + gates + 3 thresholds + 7 positions + degenerate sizes + 10 sizes + ball
    # + rows and buffers + map and step + errors + world
    simt.run_gpu_tests_on_stand_in(simt_lib, "test_gpu_object_vote.py", "test_", 44)
