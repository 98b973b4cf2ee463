"""The see-through check (visibility.hip.h and its host code in analysis_host.hip.h), compiled UNMODIFIED against the CPU stand-in of the
HIP runtime (tests/cpp/simt_emu, as in tests/test_normals_on_cpu.py) and checked by tests/test_gpu_visibility.py itself: byte for byte
against evalmap.visibility and the pure-Python visibility_brute on the known answers, the margin band, the pixel edges in all eight
octants, the windows, the minimum in every order, every size and batch, the incidence gate, the decision, the ray-cast scene, every
combination of outputs, the refusals and the struct layout, the handle's map with a step after it, and the synthetic world.  The whole
file.  No GPU needed."""
import pytest

import simt

pytestmark = pytest.mark.timeout(3600)


@pytest.fixture(scope="module")
def simt_lib(tmp_path_factory):
    return simt.build_simt_lib(tmp_path_factory.mktemp("simt_visibility"))


def test_the_see_through_check_passes_its_gpu_tests_on_the_cpu_stand_in(simt_lib):
    # 3 poses + drops + 2 bands + 8 octants + all columns + 2 row edges + 3 windows + priority + minimum + 8 map sizes + empty + 3 budgets
    # + lattice + NaN normals + decision + scene + buffers + refusals + map and step + world
    assert simt.run_gpu_tests_on_stand_in(simt_lib, "test_gpu_visibility.py", "test_", 42, no_skips=True) == 42
