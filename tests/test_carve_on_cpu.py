"""The carving of free space (carve.hip.h and its host code in analysis_host.hip.h), compiled UNMODIFIED against the CPU stand-in of the
HIP runtime (tests/cpp/simt_emu, as in tests/test_visibility_on_cpu.py) and checked by tests/test_gpu_carve.py itself: byte for byte
against evalmap.carve and the pure-Python carve_brute on the known walks under three poses, the long rays in all eight octants,
stop_short, the occupancy structure, the precedence of hits, the integration and its clamps, the batches, every size, the gates, every
combination of outputs, the refusals and the struct layout, the handle's map with a step after it, and the synthetic world.  The whole
file.  No GPU needed."""
import pytest

import simt

pytestmark = pytest.mark.timeout(3600)


@pytest.fixture(scope="module")
def simt_lib(tmp_path_factory):
    return simt.build_simt_lib(tmp_path_factory.mktemp("simt_carve"))


def test_the_carving_passes_its_gpu_tests_on_the_cpu_stand_in(simt_lib):
    # 4 walks x 3 poses + the fifth of a metre + 8 octants + 5 stop_shorts + the lidar's voxel + block + corner + two in one + lattice +
    # non-finite + precedence + box and wall + clamps + 6 batch sizes + 8 map sizes + empty + drops + buffers + refusals + map and step + world
    assert simt.run_gpu_tests_on_stand_in(simt_lib, "test_gpu_carve.py", "test_", 55, no_skips=True) == 55
